"""The remainder phase of the fused lookup (k_moments<*, true>, csrc/moments.hip): lists
longer than E0 = 32 entries are finished by teams of the wavefront's lanes and merged
back into the owner's lane.  Inputs: tests/lookup_tail_cases.py over tests/grid_cases.py
(proven in tests/test_lookup_tail_cases_cpu.py).

Bars, all exact (test_gpu_grid_cases.run_case): correspondences and squared distances of
every query assert_array_equal to the oracle; cells on against cells off bit for bit in
correspondences, distances, H, b, cost and count; on tie-free cases the numpy brute
force's index and distance; grid_info() shows the fused lookup (uses_walk == 0,
lookup_walk_groups() == 0).
"""
import functools
import json

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
import grid_cases as GC
import lookup_tail_cases as LT
import test_gpu_grid_cases as T
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def fused(info):
    assert info["built"] == 1 and info["uses_walk"] == 0


def run(name, bound, gen, nsrc=None):
    """test_gpu_grid_cases.run_case on a case that names the fused lookup: run_case itself
    then asserts lookup_walk_groups() == 0 (check_info, from expect["walk_groups"] = False)
    and uses_walk == 0 beside its exact bars."""
    e = T.brute(name, bound, gen)[0].expect
    assert e["walk_groups"] is False and e["uses_walk"] == 0
    corr, sqd, info = T.run_case(name, bound, gen, nsrc=nsrc)
    fused(info)
    return corr, sqd, info


@pytest.mark.parametrize("H", LT.TEAM_H)
@pytest.mark.parametrize("n", LT.TEAM_N)
def test_team_sizes(n, H):
    """One wavefront, H lanes with a list of n > E0 entries, 64 - H with a list of one: every
    team size F = 64 .. 1, idle teams, one chunk, a partial last chunk, many chunks."""
    gen = lambda: LT.team_case(n, H)[0]
    _, _, info = run(f"team_n{n}_H{H}", LT.BOUND, gen)
    fused(info)
    assert info["entries"] >= n + 1


@pytest.mark.parametrize("n", LT.EDGE_N)
def test_list_edges(n):
    """Lists of E0 - 1, E0 (no remainder), E0 + 1, E0 + 16, E0 + 17 entries in wavefronts of
    heavy, light and empty lanes; source prefixes that end inside a wavefront (an
    inactive lane is not heavy)."""
    gen = functools.partial(GC.shell, n, LT.BOUND)
    corr, sqd, info = run(f"shell{n}", LT.BOUND, gen)
    fused(info)
    for m in LT.EDGE_PREFIXES:
        c, s, _ = run(f"shell{n}", LT.BOUND, gen, nsrc=m)
        np.testing.assert_array_equal(c, corr[:m])
        np.testing.assert_array_equal(s, sqd[:m])


@pytest.mark.parametrize("bound", LT.PAIR_BOUNDS)
@pytest.mark.parametrize("pos", LT.PAIR_POSITIONS)
def test_ties_across_seams(pos, bound):
    """Two tied entries: the best in the common rounds and the tie in a member's chunk, in two
    members' chunks, in one chunk.  The case's source (one wavefront of long lists), and
    its first query alone (H = 1: a team of 64)."""
    gen = functools.partial(LT.seam_pair, pos, bound)
    name = f"tail_tie_pair{pos}"
    corr, _, info = run(name, bound, gen)
    fused(info)
    case = T.brute(name, bound, gen)[0]
    assert corr[0] == case.expect["pair"][1]        # the reference's choice, not the lowest list position
    c1, _, _ = run(name, bound, gen, nsrc=1)
    assert c1[0] == case.expect["pair"][1]


def test_sharded_tail():
    """shell(E0 + 17) cut by a slab and by interleaved 16-query groups: a lane that is not
    owned has no list and joins no team; the owned ones have the unsharded result; all as
    the walk's."""
    bound = LT.BOUND
    name = f"shell{LT.SHARD_N}"
    gen = functools.partial(GC.shell, LT.SHARD_N, bound)
    corr, sqd, _ = run(name, bound, gen)
    case = T.brute(name, bound, gen)[0]
    rng = np.random.default_rng(1)
    tcov, scov = T.spd(len(case.target), rng), T.spd(len(case.source), rng)
    kw = dict(k_correspondences=10, max_correspondence_distance=bound)
    lo = float(case.expect["centre"][0])
    rank = np.empty(len(case.source), np.int64)
    rank[GC.morton_order(case.source)[0]] = np.arange(len(case.source))
    own = (case.source[:, 0] >= np.float32(lo)) & ((rank // 16) % 3 == 1)
    assert own.any() and (~own).any() and (corr[own] >= 0).any() and (corr[~own] >= 0).any()
    got = {}
    for grid in (P.GRID_ON, P.GRID_OFF):
        c = T.make(case.target, case.source, tcov, scov, grid, **kw)
        c.set_shard(0, lo, np.inf)
        c.set_shard_groups(3, 1)
        H, b, cost, n = c.linearize(case.pose)
        got[grid] = (H, b, cost, n) + c.correspondences()
        if grid == P.GRID_ON:
            fused(c.grid_info())
            assert c.lookup_walk_groups() == 0
        c.close()
    H, b, cost, n, scorr, ssqd = got[P.GRID_ON]
    np.testing.assert_array_equal(scorr[own], corr[own])
    np.testing.assert_array_equal(ssqd[own], sqd[own])
    assert np.all(scorr[~own] == -1)
    assert n == int((corr[own] >= 0).sum())
    Hw, bw, costw, nw, wcorr, wsqd = got[P.GRID_OFF]
    np.testing.assert_array_equal(scorr, wcorr)
    np.testing.assert_array_equal(ssqd, wsqd)
    np.testing.assert_array_equal(H, Hw)
    np.testing.assert_array_equal(b, bw)
    assert cost == costw and n == nw


def test_align_with_tail():
    """One align of shell(E0 + 33) from a small perturbed guess through the fused LM kernel:
    the walk's pose, iterations and LM trials bit for bit, the oracle's pose to 1e-6."""
    bound = LT.BOUND
    case = GC.shell(LT.ALIGN_N, bound)
    rng = np.random.default_rng(1)
    tcov, scov = T.spd(len(case.target), rng), T.spd(len(case.source), rng)
    kw = dict(k_correspondences=10, max_correspondence_distance=bound, max_iterations=32, transformation_epsilon=0.01)
    cg = T.make(case.target, case.source, tcov, scov, P.GRID_ON, **kw)
    cw = T.make(case.target, case.source, tcov, scov, P.GRID_OFF, **kw)
    o = O.Gicp(case.source, case.target, O.default_params(**kw))
    o.set_covariances(0, scov)
    o.set_covariances(1, tcov)
    G = T.perturbed(0.05, 0.005)
    try:
        pg, rg = cg.align(G)
        pw, rw = cw.align(G)
        info = cg.grid_info()
        print(json.dumps(info), (rg.iterations_run, rg.lm_trials, rg.converged))
        fused(info)
        assert cg.lookup_walk_groups() == 0
        np.testing.assert_array_equal(pg, pw)
        assert (rg.iterations_run, rg.lm_trials, rg.converged) == (rw.iterations_run, rw.lm_trials, rw.converged)
        po, ro = o.align(G)
        np.testing.assert_allclose(pg, po, atol=1e-6)
        assert (rg.iterations_run, rg.lm_trials, rg.converged) == (ro.iterations_run, ro.lm_trials, ro.converged)
        np.testing.assert_array_equal(cg.correspondences()[0], o.last_correspondences()[0])
        np.testing.assert_array_equal(cg.correspondences()[0], cw.correspondences()[0])
    finally:
        cg.close()
        cw.close()
