"""The key-only scan of the fused lookup (k_moments<*, true> and k_moments_fresh,
csrc/moments.hip): rounds loaded from one address up to 15 entries past the list's end, a
branch-free scan in which such an entry reaches neither the key nor the second distance,
and the match's coordinates loaded after the scan.  Inputs: tests/lookup_scan_cases.py
(proven in tests/test_lookup_scan_cases_cpu.py).

Bars, all exact.  test_gpu_grid_cases.run_case (one linearize, k_moments<false, true>):
correspondences and squared distances of every query assert_array_equal to the oracle;
cells on against cells off bit for bit in correspondences, distances, H, b, cost and
count; on tie-free cases the numpy brute force's index and distance; uses_walk == 0 and
lookup_walk_groups() == 0.  align_pair (one iteration through the fused LM kernel, then
the same align again, which starts in k_moments_fresh): pose, iterations, LM trials,
correspondences and the result's tie counters equal to the walk's; on a tie-free case the
counters are 0 -- a copy of the winning entry that reaches the second distance shows up
as a resolved tie and nowhere else.
"""
import functools

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
import grid_cases as GC
import lookup_scan_cases as LS
import test_gpu_grid_cases as T

pytestmark = pytest.mark.gpu


def fused(info):
    assert info["built"] == 1 and info["uses_walk"] == 0


def run(name, bound, gen, nsrc=None):
    e = T.brute(name, bound, gen)[0].expect
    assert e["walk_groups"] is False and e["uses_walk"] == 0
    corr, sqd, info = T.run_case(name, bound, gen, nsrc=nsrc)
    fused(info)
    return corr, sqd, info


def align_pair(case, corr, tie_free):
    """One outer iteration from the identity, cells on and off, twice each (the second align
    of the cells-on context starts without the init kernel where the first met no tie).
    Returns the cells-on tie counters of the two aligns."""
    rng = np.random.default_rng(1)
    tcov, scov = T.spd(len(case.target), rng), T.spd(len(case.source), rng)
    kw = dict(k_correspondences=10, max_correspondence_distance=case.bound, max_iterations=1, transformation_epsilon=0.01)
    cg = T.make(case.target, case.source, tcov, scov, P.GRID_ON, **kw)
    cw = T.make(case.target, case.source, tcov, scov, P.GRID_OFF, **kw)
    G = np.eye(4, dtype=np.float32)
    ties = []
    try:
        for rep in range(2):
            pg, rg = cg.align(G)
            pw, rw = cw.align(G)
            fused(cg.grid_info())
            assert cg.lookup_walk_groups() == 0
            cgc, cgs = cg.correspondences()
            cwc, cws = cw.correspondences()
            print(case.expect["name"], case.bound, rep, "ties", (rg.ties_resolved, rg.tie_reruns), "walk",
                  (rw.ties_resolved, rw.tie_reruns), "fresh/init", cg.start_counts())
            np.testing.assert_array_equal(pg, pw)
            assert (rg.iterations_run, rg.lm_trials, rg.converged, rg.num_correspondences) == \
                (rw.iterations_run, rw.lm_trials, rw.converged, rw.num_correspondences)
            np.testing.assert_array_equal(cgc, cwc)
            np.testing.assert_array_equal(cgs, cws)
            np.testing.assert_array_equal(cgc, corr)
            assert (rg.ties_resolved, rg.tie_reruns) == (rw.ties_resolved, rw.tie_reruns)
            if tie_free:
                assert (rg.ties_resolved, rg.tie_reruns) == (0, 0)
            ties.append((rg.ties_resolved, rg.tie_reruns))
        if tie_free:
            assert cg.start_counts()[0] >= 1        # k_moments_fresh ran the second align
    finally:
        cg.close()
        cw.close()
    return ties


@pytest.mark.parametrize("bound", LS.BOUNDS)
@pytest.mark.parametrize("n", LS.MEMBER_N)
def test_every_list_position_wins(n, bound):
    """One query per list member, nudged towards it: the first, an inner and the last entry
    of lists of n entries win; no tie counted."""
    gen = functools.partial(LS.member_case, n, bound)
    name = f"member_n{n}"
    corr, _, info = run(name, bound, gen)
    assert info["entries"] >= n
    np.testing.assert_array_equal(corr, np.arange(n))
    align_pair(T.brute(name, bound, gen)[0], corr, True)


@pytest.mark.parametrize("m", (1, 2, 16, 17))
def test_source_prefixes(m):
    """A wavefront with m active lanes (the others have no list) over lists that end inside
    a round."""
    n, bound = 33, 1.0
    gen = functools.partial(LS.member_case, n, bound)
    corr, sqd, _ = run(f"member_n{n}", bound, gen)
    c, s, _ = run(f"member_n{n}", bound, gen, nsrc=m)
    np.testing.assert_array_equal(c, corr[:m])
    np.testing.assert_array_equal(s, sqd[:m])


@pytest.mark.parametrize("bound", LS.BOUNDS)
def test_two_wavefronts(bound):
    """shell(17)'s own source and its first 65 queries: more than one wavefront, lists of 17."""
    gen = functools.partial(GC.shell, 17, bound)
    corr, sqd, _ = run("shell17", bound, gen)
    c, s, _ = run("shell17", bound, gen, nsrc=65)
    np.testing.assert_array_equal(c, corr[:65])
    np.testing.assert_array_equal(s, sqd[:65])
    case = T.brute("shell17", bound, gen)[0]
    align_pair(case, corr, True)


@pytest.mark.parametrize("bound", LS.BOUNDS)
@pytest.mark.parametrize("n", LS.FACE_N)
def test_neighbouring_lists_share_the_winner(n, bound):
    """Queries on both sides of the fine faces through the centre: adjacent fine cells whose
    lists both hold the nearest point; no tie counted."""
    gen = functools.partial(LS.face_case, n, bound)
    name = f"face_n{n}"
    corr, _, _ = run(name, bound, gen)
    align_pair(T.brute(name, bound, gen)[0], corr, True)


@pytest.mark.parametrize("bound", LS.BOUNDS)
@pytest.mark.parametrize("pos,total", LS.PAIRS)
def test_second_distance(pos, total, bound):
    """Two entries at a bit-equal distance: inside one round, across the two common rounds,
    across the remainder phase, first against last.  The reference's choice (the higher
    list position) is answered, so the nanoflann re-run changed j: H and b are the walk's
    (run_case), with the coordinates of the new match."""
    gen = functools.partial(LS.pair_case, pos, total, bound)
    name = f"scan_pair{pos}of{total}"
    corr, _, _ = run(name, bound, gen)
    case = T.brute(name, bound, gen)[0]
    assert corr[0] == case.expect["pair"][1]
    c1, _, _ = run(name, bound, gen, nsrc=1)
    assert c1[0] == case.expect["pair"][1]
    ties = align_pair(case, corr, False)
    assert ties[0][0] >= 1 and ties[1][0] >= 1


def test_list_of_one_entry_gives_no_tie():
    """A single entry leaves the second distance at +inf: nothing ties with it."""
    for bound in LS.BOUNDS:
        gen = functools.partial(LS.member_case, 1, bound)
        corr, _, info = run("member_n1", bound, gen)
        assert corr[0] == 0
        assert align_pair(T.brute("member_n1", bound, gen)[0], corr, True) == [(0, 0), (0, 0)]


def test_winner_found_by_a_team_member():
    """n = 161, H = 9 (teams of 4): winners in the remainder chunks of other lanes; the match's
    coordinates are loaded by the owner after the merge -- H and b bit for bit the walk's."""
    gen = lambda: LS.team()[0]
    name = "team_n%d_H%d" % LS.TEAM
    corr, _, info = run(name, LS.team()[0].bound, gen)
    assert info["entries"] >= LS.TEAM[0] + 1
    align_pair(T.brute(name, LS.team()[0].bound, gen)[0], corr, True)
