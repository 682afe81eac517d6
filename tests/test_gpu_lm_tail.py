"""The fused iteration's serial tail (moments.hip, DESIGN.md §4 "LM step" and
"Launch structure"): the last block of k_moments<true, true> to arrive reads
the other blocks' slab rows, takes the LM step and publishes the state to
pinned memory without a full-block fence (per-wave drains, sc1 loads of the
state, one release store), the three tie words, which other blocks of the
same launch write, fetched by returning atomics.

The reference is never the fused path: it is the project's own
kernel-boundary route.  The same context with set_profiling(True) runs eager
with an unfused k_lm_step and copies the state back with hipMemcpy after a
stream synchronise; a second context with GRID_OFF runs the walk, whose
k_lm_step sits behind a kernel boundary.

Bars: every comparison is assert_array_equal / == on pose, final_hessian,
final_cost, lm_lambda, iterations_run, nr_iterations, converged, lm_trials
and num_correspondences; on the tied target also ties_resolved, and pose /
iterations / trials against the oracle as test_gpu_ties.test_align_on_tied_target.
"""
import math

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
import np_gicp as NP
from dynamic_direct_lidar_odometry_amd import SOURCE, TARGET, scene
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KW = dict(k_correspondences=10, max_correspondence_distance=2.0, max_iterations=32, transformation_epsilon=0.01)
N_ALIGNS = 200


def make(tgt, src, tcov, scov, grid, **kw):
    c = P.Context(0)
    c.set_params(P.default_params(**kw))
    c.set_target_grid(grid)
    c.set_target(tgt)
    c.set_covariances(TARGET, tcov)
    c.set_source(src)
    c.set_covariances(SOURCE, scov)
    return c


def record(pose, res):
    """Everything the align reports that the LM tail computes, as one float64 row (ints are exact in it)."""
    return np.concatenate([np.asarray(pose, np.float64).ravel(), np.array(res.final_hessian, np.float64),
                           [res.final_cost, res.lm_lambda, res.iterations_run, res.nr_iterations, res.converged,
                            res.lm_trials, res.num_correspondences]])


@pytest.fixture(scope="module")
def scans():
    """A two-scan target and a two-scan source (64 x 1024 each, the source in its first scan's frame) with
    oracle covariances, computed once; the cases below take subsets of the source."""
    seed, stride, rows, cols = 1100, 3, 64, 1024
    sc = scene.make_scene(seed)
    poses = scene.trajectory(4 * stride + 2, seed)
    tgt = np.concatenate([scene.transform(scene.raycast(sc, poses[k], rows, cols, seed=seed + i), poses[k])
                          for i, k in enumerate((0, stride))])
    T = poses[2 * stride]
    s0 = scene.raycast(sc, T, rows, cols, seed=seed + 2)
    s1 = scene.raycast(sc, poses[2 * stride + 1], rows, cols, seed=seed + 3)
    src = np.concatenate([s0, scene.transform(s1, np.linalg.inv(T) @ poses[2 * stride + 1])])
    tgt, src = np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32)
    return dict(tgt=tgt, src=src, n0=len(s0), T=T, tcov=O.covariances(tgt, 10), scov=O.covariances(src, 10))


def guesses_around(T):
    """The spread of bench.py's varied_guesses (0.36 m and 2 degrees at scale 1, rotated about z), one of them
    shrunk to a few centimetres so that the aligns converge in different iteration counts."""
    out = []
    for i, (sc, yaw) in enumerate([(1.0, 0), (0.5, 30), (1.5, 60), (0.05, 90), (1.2, 140), (0.75, 200), (1.0, 250),
                                   (0.4, 310)]):
        a = math.radians(yaw)
        t = np.array([0.30 * math.cos(a) + 0.20 * math.sin(a), 0.30 * math.sin(a) - 0.20 * math.cos(a), 0.05])
        D = scene.make_pose(sc * t, (math.radians(0.5 * sc), math.radians(-0.5 * sc if i % 2 else 0.5 * sc),
                                     math.radians(2.0 * sc * (1 if i % 3 else -1))))
        out.append((T @ D).astype(np.float32))
    return out


# source sizes by 32,768-point bucket: 64, 128, 192 and 256 slab rows (linearize_geometry); at 3,000 points
# six blocks work and 58 arrive at once, 256 rows is the production fan-in over every CU
@pytest.mark.parametrize("n_src, rows", [(3000, 64), (40000, 128), (70000, 192), (100000, 256)])
def test_handoff_and_publication_per_slab_geometry(scans, n_src, rows):
    """200 graph aligns cycling 8 guesses (consecutive aligns differ in every working slab row; both pinned
    slots and the speculative chunk are used): each equals the profiled align of its guess and the walk's."""
    src_all, scov_all = scans["src"], scans["scov"]
    if n_src > scans["n0"]:   # two scans, truncated
        assert len(src_all) >= 98305, len(src_all)
        idx = np.arange(min(n_src, len(src_all)))
    else:                     # a subset of the first scan
        idx = np.sort(np.random.default_rng(n_src).choice(scans["n0"], n_src, replace=False))
    assert 64 * ((len(idx) + 32767) // 32768) == rows
    src, scov = np.ascontiguousarray(src_all[idx]), np.ascontiguousarray(scov_all[idx])
    cg = make(scans["tgt"], src, scans["tcov"], scov, P.GRID_ON, **KW)
    cw = make(scans["tgt"], src, scans["tcov"], scov, P.GRID_OFF, **KW)
    G = guesses_around(scans["T"])
    cg.set_profiling(True)
    ref_prof = [record(*cg.align(g)) for g in G]
    cg.set_profiling(False)
    ref_walk = [record(*cw.align(g)) for g in G]
    info = cg.grid_info()
    assert info["built"] == 1 and info["uses_walk"] == 0, info   # the one-kernel lookup path: the LM step is fused
    iters = sorted({int(r[-5]) for r in ref_prof})
    print("n_src", len(idx), "rows", rows, "iterations_run per guess", [int(r[-5]) for r in ref_prof])
    assert len(iters) >= 2, iters   # different iteration counts: first chunks of different lengths, no-op chunks
    for k in range(N_ALIGNS):
        got = record(*cg.align(G[k % len(G)]))
        np.testing.assert_array_equal(got, ref_prof[k % len(G)], err_msg=f"align {k} vs the profiled route")
        np.testing.assert_array_equal(got, ref_walk[k % len(G)], err_msg=f"align {k} vs the walk")
    cg.close()
    cw.close()


def spd_covs(n, seed, scale=0.05):
    rng = np.random.default_rng(seed)
    A = rng.normal(0, scale, (n, 3, 3))
    return np.ascontiguousarray(NP.mat_to_sym6(A @ np.transpose(A, (0, 2, 1)) + 1e-3 * np.eye(3)))


def test_tie_words_across_blocks():
    """A 20 x 20 x 12 lattice of spacing 0.5 queried at its 3,971 cell centres (8 corners at exactly the same
    fp32 distance: 8 working blocks of tied queries) with 20,000 untied queries behind them, so a tied block
    is not always the last to arrive: the tie words the last block publishes are the other blocks'."""
    h = 0.5
    gx, gy, gz = np.meshgrid(np.arange(20), np.arange(20), np.arange(12), indexing="ij")
    tgt = np.ascontiguousarray(np.stack([gx, gy, gz], -1).reshape(-1, 3) * h, np.float32)
    cx, cy, cz = np.meshgrid(np.arange(19), np.arange(19), np.arange(11), indexing="ij")
    centres = (np.stack([cx, cy, cz], -1).reshape(-1, 3) + 0.5) * h
    rng = np.random.default_rng(7)
    untied = rng.uniform([0.0, 0.0, 0.0], [19 * h, 19 * h, 11 * h], (20000, 3))
    src = np.ascontiguousarray(np.concatenate([centres, untied]), np.float32)
    n_tied = len(centres)
    assert n_tied > 7 * 512 and len(src) <= 32768   # 8 of the 64 blocks hold the tied queries
    tcov, scov = spd_covs(len(tgt), 1), spd_covs(len(src), 2)
    kw = dict(k_correspondences=10, max_correspondence_distance=2.0, max_iterations=32, transformation_epsilon=5e-4)
    cg = make(tgt, src, tcov, scov, P.GRID_ON, **kw)
    cw = make(tgt, src, tcov, scov, P.GRID_OFF, **kw)
    o = O.Gicp(src, tgt, O.default_params(**kw))
    o.set_covariances(0, scov)
    o.set_covariances(1, tcov)
    # from the identity every centre is tied in the first iteration; from the small offsets (almost) none is
    guesses = [np.eye(4, dtype=np.float32)]
    for _ in range(2):
        g = np.eye(4, dtype=np.float32)
        g[:3, :3] = NP.so3_exp(rng.normal(0, 0.01, 3))
        g[:3, 3] = rng.normal(0, 0.05, 3)
        guesses.append(g)
    oracle = [o.align(g) for g in guesses]
    order = [0, 1, 0, 2] * 5
    # the first align meets ties before the target has nanoflann's tree: built, and the align run again
    pose, res = cg.align(guesses[0])
    assert res.tie_reruns == 1
    assert res.ties_resolved >= n_tied
    info = cg.grid_info()
    assert info["built"] == 1 and info["uses_walk"] == 0, info
    cg.set_profiling(True)
    prof = [cg.align(g) for g in guesses]
    cg.set_profiling(False)
    walk = [cw.align(g) for g in guesses]
    print("ties_resolved per guess", [r.ties_resolved for _, r in prof], "walk", [r.ties_resolved for _, r in walk])
    for k, gi in enumerate(order):
        pose, res = cg.align(guesses[gi])
        assert res.tie_reruns == 0
        assert res.ties_resolved == prof[gi][1].ties_resolved, (k, gi)
        assert res.ties_resolved == walk[gi][1].ties_resolved, (k, gi)
        np.testing.assert_array_equal(record(pose, res), record(*prof[gi]), err_msg=f"align {k} vs the profiled route")
        opose, ores = oracle[gi]
        assert (res.iterations_run, res.converged, res.lm_trials, res.lm_failed) == \
            (ores.iterations_run, ores.converged, ores.lm_trials, ores.lm_failed)
        np.testing.assert_allclose(pose, opose, atol=1e-6)
    cg.close()
    cw.close()
