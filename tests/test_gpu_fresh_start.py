"""Aligns that start without the init kernel (DESIGN.md §4 "Launch structure"): when only the
guess changed since the context's previous align, that align ended cleanly on the graph path and
reported no tie, the first iteration is k_moments_fresh (moments.hip) -- the guess, the ticket and
rec0 are its kernel arguments, nothing of the state is read at its start, and its LM step stores
every word k_align_init would have reset.  Every other align starts with k_align_init as before.

The reference is never the path under test: the same context with set_profiling(True) (eager,
k_align_init, an unfused k_lm_step, the state copied back after a stream synchronise) and a
GRID_OFF context (the walk, always behind k_align_init).

Bars: assert_array_equal / == on pose, final_hessian, final_cost, lm_lambda, iterations_run,
nr_iterations, converged, lm_failed, lm_trials, num_correspondences and ties_resolved, and
lookup_walk_groups() against the profiled route's; every case asserts through start_counts()
which start each align took.
"""
import math

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
import grid_cases as GC
import np_gicp as NP
from dynamic_direct_lidar_odometry_amd import SOURCE, TARGET, scene
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KW = dict(k_correspondences=10, max_correspondence_distance=2.0, max_iterations=32, transformation_epsilon=0.01)


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
    """Everything the align reports, as one float64 row (ints are exact in it)."""
    return np.concatenate([np.asarray(pose, np.float64).ravel(), np.array(res.final_hessian, np.float64),
                           [res.final_cost, res.lm_lambda, res.iterations_run, res.nr_iterations, res.converged,
                            res.lm_failed, res.lm_trials, res.num_correspondences, res.ties_resolved]])


ITERS = -7   # record()[ITERS] = iterations_run


def spd_covs(n, seed, scale=0.05):
    rng = np.random.default_rng(seed)
    A = rng.normal(0, scale, (n, 3, 3))
    return np.ascontiguousarray(NP.mat_to_sym6(A @ np.transpose(A, (0, 2, 1)) + 1e-3 * np.eye(3)))


def raycast_problem():
    """A one-scan target (64 x 1024, world frame) and a later scan as the source (its own frame), with
    oracle covariances: (tgt, src, tcov, scov, T) with T the source's true pose."""
    seed, stride, rows, cols = 1100, 3, 64, 1024
    sc = scene.make_scene(seed)
    poses = scene.trajectory(stride + 2, seed)
    tgt = scene.transform(scene.raycast(sc, poses[0], rows, cols, seed=seed), poses[0])
    T = poses[stride]
    src = scene.raycast(sc, T, rows, cols, seed=seed + 2)
    tgt, src = np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32)
    return dict(tgt=tgt, src=src, T=T, tcov=O.covariances(tgt, 10), scov=O.covariances(src, 10))


@pytest.fixture(scope="module")
def scans():
    return raycast_problem()


def subset(scans, n, seed=None):
    """n source points: a random subset of the scan (seeded by n unless told otherwise)."""
    idx = np.sort(np.random.default_rng(n if seed is None else seed).choice(len(scans["src"]), n, replace=False))
    return np.ascontiguousarray(scans["src"][idx]), np.ascontiguousarray(scans["scov"][idx])


def guesses_around(T, scale=1.0):
    """test_gpu_lm_tail.guesses_around: the spread of bench.py's varied guesses, one of them shrunk to
    a few centimetres, so that the aligns converge in different iteration counts."""
    out = []
    for i, (sc, yaw) in enumerate([(1.0, 0), (0.5, 30), (1.5, 60), (0.05, 90), (1.2, 140), (0.75, 200), (1.0, 250),
                                   (0.4, 310)]):
        sc *= scale
        a = math.radians(yaw)
        t = np.array([0.30 * math.cos(a) + 0.20 * math.sin(a), 0.30 * math.sin(a) - 0.20 * math.cos(a), 0.05])
        D = scene.make_pose(sc * t, (math.radians(0.5 * sc), math.radians(-0.5 * sc if i % 2 else 0.5 * sc),
                                     math.radians(2.0 * sc * (1 if i % 3 else -1))))
        out.append((np.asarray(T, np.float64) @ D).astype(np.float32))
    return out


class Pair:
    """The context under test (cells on) with its two references for a list of guesses."""

    def __init__(self, tgt, src, tcov, scov, guesses, **kw):
        self.cg = make(tgt, src, tcov, scov, P.GRID_ON, **kw)
        self.cw = make(tgt, src, tcov, scov, P.GRID_OFF, **kw)
        self.G = guesses
        self.reference()
        info = self.cg.grid_info()
        assert info["built"] == 1 and info["uses_walk"] == 0, info   # the fused one-kernel lookup

    def reference(self):
        """The profiled (eager) route of the context under test and the walk, per guess."""
        self.cg.set_profiling(True)
        self.ref_prof, self.ref_groups = [], []
        for g in self.G:
            self.ref_prof.append(record(*self.cg.align(g)))
            self.ref_groups.append(self.cg.lookup_walk_groups())
        self.cg.set_profiling(False)
        self.ref_walk = [record(*self.cw.align(g)) for g in self.G]

    def align(self, gi, expect_fresh, msg=""):
        """One align of guess gi on the context under test: the start it took, every word against both
        references; returns the record."""
        f0, i0 = self.cg.start_counts()
        got = record(*self.cg.align(self.G[gi]))
        f1, i1 = self.cg.start_counts()
        assert (f1 - f0, i1 - i0) == ((1, 0) if expect_fresh else (0, 1)), (msg, gi, expect_fresh, f1 - f0, i1 - i0)
        np.testing.assert_array_equal(got, self.ref_prof[gi], err_msg=f"{msg} guess {gi} vs the profiled route")
        np.testing.assert_array_equal(got, self.ref_walk[gi], err_msg=f"{msg} guess {gi} vs the walk")
        return got

    def check_groups(self, gi):
        assert self.cg.lookup_walk_groups() == self.ref_groups[gi] == 0

    def close(self):
        self.cg.close()
        self.cw.close()


def cycle(p, n_aligns, tag):
    """n_aligns aligns cycling the guesses: the first after the references takes the init kernel
    (the profiled route ran last), every later one the fresh start."""
    for k in range(n_aligns):
        gi = k % len(p.G)
        got = p.align(gi, expect_fresh=k > 0, msg=f"{tag} align {k}")
        assert got[-1] == 0   # no tie: the next align may start fresh
        if k % 5 == 0:
            p.check_groups(gi)


# ---------------------------------------------------------------------------
# 1. the guess cycle
@pytest.mark.parametrize("n_src, rows", [(3000, 64), (33000, 128)])
def test_guess_cycle_raycast(scans, n_src, rows):
    """104 aligns cycling 8 guesses of different iteration counts (first chunks of different lengths,
    both pinned slots, the speculative chunk): 3,000 points work in 6 of 64 blocks, 58 arrive at
    once; 33,000 points are the 128-row geometry."""
    src, scov = subset(scans, n_src)
    assert 64 * ((n_src + 32767) // 32768) == rows
    p = Pair(scans["tgt"], src, scans["tcov"], scov, guesses_around(scans["T"]), **KW)
    iters = [int(r[ITERS]) for r in p.ref_prof]
    print("n_src", n_src, "iterations_run per guess", iters)
    assert len(set(iters)) >= 2, iters
    cycle(p, 104, f"n_src {n_src}")
    assert p.cg.start_counts()[0] == 103
    p.close()


def small_guesses():
    """Eight small offsets from the identity (the synthetic cases' pose)."""
    rng = np.random.default_rng(5)
    out = []
    for i in range(8):
        s = (0.2, 1.0, 0.5, 2.0)[i % 4]
        g = np.eye(4)
        g[:3, :3] = NP.so3_exp(rng.normal(0, 0.004 * s, 3))
        g[:3, 3] = rng.normal(0, 0.01 * s, 3)
        out.append(g.astype(np.float32))
    return out


@pytest.mark.parametrize("n_src", [1, 16, 63, 64, 65])
def test_guess_cycle_synthetic(n_src):
    """grid_cases.dense_cube (2,632 target points, refined cells, lists of every length) with source
    prefixes of 1, 16, 63, 64 and 65 points: block 0 is the only working block of 64, and with 65
    points its second wavefront holds one query."""
    case = GC.dense_cube(1.0)
    src = np.ascontiguousarray(case.source[:n_src])
    tcov, scov = spd_covs(len(case.target), 1), spd_covs(len(case.source), 2)[:n_src]
    kw = dict(k_correspondences=10, max_correspondence_distance=case.bound, max_iterations=16, transformation_epsilon=1e-3)
    p = Pair(case.target, src, tcov, scov, small_guesses(), **kw)
    print("n_src", n_src, "iterations_run per guess", [int(r[ITERS]) for r in p.ref_prof])
    cycle(p, 24, f"dense_cube prefix {n_src}")
    p.close()


# ---------------------------------------------------------------------------
# 2. short first chunks: the fresh kernel is also the publishing kernel when the chunk is one iteration
@pytest.mark.parametrize("kw", [dict(max_iterations=1), dict(max_iterations=2),
                                dict(optimizer=P.GAUSS_NEWTON, fixed_iterations=1),
                                dict(optimizer=P.GAUSS_NEWTON, fixed_iterations=3)],
                         ids=["lm_max1", "lm_max2", "gn_fixed1", "gn_fixed3"])
def test_short_first_chunks(scans, kw):
    src, scov = subset(scans, 3000)
    p = Pair(scans["tgt"], src, scans["tcov"], scov, guesses_around(scans["T"]), **dict(KW, **kw))
    print(kw, "iterations_run per guess", [int(r[ITERS]) for r in p.ref_prof])
    cycle(p, 24, str(kw))
    p.close()


# ---------------------------------------------------------------------------
# 3. stale state
def test_stale_converged_then_far(scans):
    """The state the fresh kernel finds is the previous align's, done and converged set after one
    iteration: then a far guess that needs more iterations, and back."""
    src, scov = subset(scans, 3000)
    T = np.asarray(scans["T"], np.float64)
    near = scene.make_pose(np.array([0.004, -0.003, 0.001]), (0.0, 0.0, math.radians(0.02)))
    far = scene.make_pose(np.array([0.45, -0.30, 0.08]), (math.radians(0.7), math.radians(-0.7), math.radians(3.0)))
    p = Pair(scans["tgt"], src, scans["tcov"], scov, [(T @ D).astype(np.float32) for D in (near, far)], **KW)
    it = [int(r[ITERS]) for r in p.ref_prof]
    conv = [int(r[ITERS + 2]) for r in p.ref_prof]
    print("iterations", it, "converged", conv)
    assert conv == [1, 1] and it[0] == 1 and it[1] >= 3
    p.align(0, expect_fresh=False, msg="first")
    for k, gi in enumerate([1, 0, 0, 1, 1, 0, 1]):
        p.align(gi, expect_fresh=True, msg=f"stale {k}")
    p.close()


REJECTED = 6   # of small_guesses(), on dense_cube's first 16 source points with one LM trial per step


def test_stale_failed_and_rejected_first_step():
    """One LM trial per step (lm_max_iterations = 1): a step whose trial is rejected and has not
    converged ends the align with lm_failed = 1.  On grid_cases.dense_cube's first 16 source points
    guess REJECTED does so at its first step (found with the oracle on the CPU; asserted here on the
    references), so the pose it leaves is the guess itself -- the fresh kernel has to store it, the
    state holds the previous align's -- and the other guesses converge, the first of them from a
    state with lm_failed and done set and converged clear.

    final_hessian is stored only with an accepted step and no kernel resets it (k_align_init does
    not either), so an align that accepts none reports the one its context's previous align left.
    The references therefore go through the same sequence of guesses as the aligns under test, and
    the test asserts that carried-over block too."""
    case = GC.dense_cube(1.0)
    n_src = 16
    src = np.ascontiguousarray(case.source[:n_src])
    tcov, scov = spd_covs(len(case.target), 1), spd_covs(len(case.source), 2)[:n_src]
    kw = dict(k_correspondences=10, max_correspondence_distance=case.bound, max_iterations=16, transformation_epsilon=1e-3,
              lm_max_iterations=1)
    G = small_guesses()
    p = Pair(case.target, src, tcov, scov, G, **kw)
    it = [int(r[ITERS]) for r in p.ref_prof]
    conv = [int(r[ITERS + 2]) for r in p.ref_prof]
    failed = [int(r[ITERS + 3]) for r in p.ref_prof]
    print("iterations", it, "converged", conv, "lm_failed", failed)
    assert failed[REJECTED] == 1 and it[REJECTED] == 1 and conv[REJECTED] == 0
    np.testing.assert_array_equal(p.ref_prof[REJECTED][:16], np.asarray(G[REJECTED], np.float64).ravel())
    others = [g for g in range(len(G)) if g != REJECTED]
    assert all(conv[g] == 1 and failed[g] == 0 and it[g] > 1 for g in others)
    seq = [0, REJECTED, 1, REJECTED, REJECTED, 2, 3, REJECTED, 0, 4, REJECTED, 5, 7]
    p.cg.set_profiling(True)
    prof = [record(*p.cg.align(G[gi])) for gi in seq]
    p.cg.set_profiling(False)
    walk = [record(*p.cw.align(G[gi])) for gi in seq]
    for k, gi in enumerate(seq):
        f0, i0 = p.cg.start_counts()
        got = record(*p.cg.align(G[gi]))
        f1, i1 = p.cg.start_counts()
        assert (f1 - f0, i1 - i0) == ((1, 0) if k > 0 else (0, 1)), (k, gi)
        np.testing.assert_array_equal(got, prof[k], err_msg=f"align {k} guess {gi} vs the profiled route")
        np.testing.assert_array_equal(got, walk[k], err_msg=f"align {k} guess {gi} vs the walk")
        for name, lo, hi in (("pose", 0, 16), ("final_cost ..", 52, len(got))):   # all but final_hessian: no history in them
            np.testing.assert_array_equal(got[lo:hi], p.ref_prof[gi][lo:hi], err_msg=f"align {k} guess {gi} {name}")
        if gi == REJECTED:
            np.testing.assert_array_equal(got[16:52], prof[k - 1][16:52], err_msg=f"align {k}: final_hessian carried over")
            np.testing.assert_array_equal(got[:16], np.asarray(G[gi], np.float64).ravel())
    p.close()


# ---------------------------------------------------------------------------
# 4. fallback triggers
def test_fallback_triggers(scans):
    """Whatever changes more than the guess sends exactly one align through k_align_init on the fused
    path, after which the fresh start resumes."""
    src, scov = subset(scans, 3000)
    p = Pair(scans["tgt"], src, scans["tcov"], scov, guesses_around(scans["T"]), **KW)
    cg = p.cg

    def resumes(tag):
        p.align(1, expect_fresh=False, msg=tag + ": the one init-path align")
        p.align(2, expect_fresh=True, msg=tag + ": resumed")
        p.align(3, expect_fresh=True, msg=tag + ": resumed")

    resumes("after the profiled references")
    # set_params with a changed epsilon: its own references
    kw2 = dict(KW, transformation_epsilon=0.002)
    cg.set_params(P.default_params(**kw2))
    p.cw.set_params(P.default_params(**kw2))
    p.reference()
    resumes("changed epsilon")
    cg.set_params(P.default_params(**KW))
    p.cw.set_params(P.default_params(**KW))
    p.reference()
    resumes("epsilon changed back")
    # set_params with a changed bound: the target's cells are built again for it
    kw3 = dict(KW, max_correspondence_distance=1.5)
    cg.set_params(P.default_params(**kw3))
    p.cw.set_params(P.default_params(**kw3))
    p.reference()
    assert cg.grid_info()["uses_walk"] == 0
    resumes("changed bound")
    cg.set_params(P.default_params(**KW))
    p.cw.set_params(P.default_params(**KW))
    p.reference()
    resumes("bound changed back")
    # the same source set again
    cg.set_source(src)
    cg.set_covariances(SOURCE, scov)
    resumes("set_source")
    # swapped and swapped back
    cg.swap_source_target()
    cg.swap_source_target()
    resumes("swap_source_target")
    # profiling: the profiled align itself takes the eager route with the init kernel, and so does the one after it
    cg.set_profiling(True)
    f0, i0 = cg.start_counts()
    got = record(*cg.align(p.G[4]))
    assert cg.start_counts() == (f0, i0 + 1)
    np.testing.assert_array_equal(got, p.ref_prof[4])
    cg.set_profiling(False)
    resumes("profiling toggled")
    # cells off (the walk) and on again
    cg.set_target_grid(P.GRID_OFF)
    f0, i0 = cg.start_counts()
    got = record(*cg.align(p.G[5]))
    assert cg.start_counts() == (f0, i0 + 1)
    np.testing.assert_array_equal(got, p.ref_walk[5])
    cg.set_target_grid(P.GRID_ON)
    resumes("cells toggled")
    p.close()


# ---------------------------------------------------------------------------
# 5. ties
def test_ties_take_the_init_path():
    """The construction of test_gpu_lm_tail.test_tie_words_across_blocks at two blocks of tied queries
    (a 10 x 10 x 8 lattice queried at its 567 cell centres, 2,000 untied queries behind them): the tie
    words are not 0 after an align that met ties, so the align after it starts with k_align_init;
    results as there (the profiled route's in every word, the oracle's counts and pose)."""
    h = 0.5
    gx, gy, gz = np.meshgrid(np.arange(10), np.arange(10), np.arange(8), indexing="ij")
    tgt = np.ascontiguousarray(np.stack([gx, gy, gz], -1).reshape(-1, 3) * h, np.float32)
    cx, cy, cz = np.meshgrid(np.arange(9), np.arange(9), np.arange(7), indexing="ij")
    centres = (np.stack([cx, cy, cz], -1).reshape(-1, 3) + 0.5) * h
    rng = np.random.default_rng(7)
    untied = rng.uniform([0.0, 0.0, 0.0], [9 * h, 9 * h, 7 * h], (2000, 3))
    src = np.ascontiguousarray(np.concatenate([centres, untied]), np.float32)
    n_tied = len(centres)
    assert 512 < n_tied <= 1024
    tcov, scov = spd_covs(len(tgt), 1), spd_covs(len(src), 2)
    kw = dict(k_correspondences=10, max_correspondence_distance=2.0, max_iterations=32, transformation_epsilon=5e-4)
    cg = make(tgt, src, tcov, scov, P.GRID_ON, **kw)
    o = O.Gicp(src, tgt, O.default_params(**kw))
    o.set_covariances(0, scov)
    o.set_covariances(1, tcov)
    guesses = [np.eye(4, dtype=np.float32)]
    for _ in range(2):
        g = np.eye(4, dtype=np.float32)
        g[:3, :3] = NP.so3_exp(rng.normal(0, 0.01, 3))
        g[:3, 3] = rng.normal(0, 0.05, 3)
        guesses.append(g)
    oracle = [o.align(g) for g in guesses]
    # the first align meets ties before the target has nanoflann's tree: built, and the align run again
    pose, res = cg.align(guesses[0])
    assert res.tie_reruns == 1 and res.ties_resolved >= n_tied
    assert cg.start_counts() == (0, 2)
    info = cg.grid_info()
    assert info["built"] == 1 and info["uses_walk"] == 0, info
    cg.set_profiling(True)
    prof = [cg.align(g) for g in guesses]
    cg.set_profiling(False)
    print("ties_resolved per guess", [r.ties_resolved for _, r in prof])
    assert prof[0][1].ties_resolved >= n_tied
    prev_clean = False   # the profiled route ran last
    fresh_seen = 0
    for k, gi in enumerate([0, 1, 0, 2, 2, 1, 1, 0, 0, 2, 1, 2]):
        f0, i0 = cg.start_counts()
        pose, res = cg.align(guesses[gi])
        f1, i1 = cg.start_counts()
        # an align that follows one that reported ties starts with k_align_init; one that follows a clean align is fresh
        assert (f1 - f0, i1 - i0) == ((1, 0) if prev_clean else (0, 1)), (k, gi, prev_clean)
        fresh_seen += f1 - f0
        prev_clean = res.ties_resolved == 0
        assert res.tie_reruns == 0
        np.testing.assert_array_equal(record(pose, res), record(*prof[gi]), err_msg=f"align {k} vs the profiled route")
        opose, ores = oracle[gi]
        assert (res.iterations_run, res.converged, res.lm_trials, res.lm_failed) == \
            (ores.iterations_run, ores.converged, ores.lm_trials, ores.lm_failed)
        np.testing.assert_allclose(pose, opose, atol=1e-6)
    print("fresh starts among the 12 aligns:", fresh_seen)
    cg.close()


# ---------------------------------------------------------------------------
# 6. two contexts alternating on one device
def test_two_contexts_alternating(scans):
    a_src, a_cov = subset(scans, 3000, seed=1)
    b_src, b_cov = subset(scans, 5000, seed=2)
    G = guesses_around(scans["T"])
    a = Pair(scans["tgt"], a_src, scans["tcov"], a_cov, G, **KW)
    b = Pair(scans["tgt"], b_src, scans["tcov"], b_cov, G[::-1], **KW)
    for k in range(40):
        a.align(k % 8, expect_fresh=k > 0, msg=f"ctx a align {k}")
        b.align((3 * k) % 8, expect_fresh=k > 0, msg=f"ctx b align {k}")
    assert a.cg.start_counts()[0] == 39 and b.cg.start_counts()[0] == 39
    a.close()
    b.close()
