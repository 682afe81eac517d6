"""The inputs of tests/test_gpu_lookup_scan.py (tests/lookup_scan_cases.py) proven on the CPU
with the oracle's nanoflann search, a numpy brute force and GC.Grid's list rule:

  * member_case(n): every query's cell, at whatever level the build stops, lists exactly
    the n shell points; query k's nearest point is shell point k, alone at its distance;
    over the n queries the winners' list positions are 0 .. n - 1, each once -- among them
    the last entry of a list that ends inside a round (n = 1, 2, 15, 17, 31, 33, 49);
  * face_case(n): on every axis the queries lie on both sides of the fine face through
    the centre (different level-3 fine cells), every one of those cells lists exactly the
    n shell points, and no query has a tied minimum;
  * pair_case: the list is the ``total`` shell points, the tied points sit at the named
    positions, nanoflann keeps the one at the higher position, no other query ties; the
    positions lie inside one round, across the two common rounds, across the remainder
    phase, and include (first, last) of lists that end inside a round;
  * the team case's heavy queries have winners past the common rounds, in chunks that
    other lanes of the team scan.
"""
import numpy as np
import pytest

import grid_cases as GC
import lookup_scan_cases as LS
import lookup_tail_cases as LT
from oracle import oracle as O

F32 = np.float32


def exact_list(case, q, n):
    """The list of q's cell holds the n shell points and nothing else, at every level."""
    g = GC.Grid(case.target, case.bound)
    assert g.inside(q)
    for lv, lo, hi in LT.list_bounds(case.target, g, q):
        assert lo == n == hi, (lv, lo, hi, n)


@pytest.mark.parametrize("bound", LS.BOUNDS)
@pytest.mark.parametrize("n", LS.MEMBER_N)
def test_member_case(n, bound):
    case = LS.member_case(n, bound)
    assert case.source.shape == (n, 3) and n <= 64
    for q in case.source:
        exact_list(case, q, n)
    m, arg, count = GC.brute(case.target, case.source)
    assert np.all(count == 1) and np.array_equal(arg, np.arange(n))
    assert np.all(m.astype(np.float64) < bound ** 2)
    idx, d = O.knn(case.target, case.source, 1)
    assert np.array_equal(idx[:, 0], arg) and np.array_equal(d[:, 0], m)
    pos = LS.list_position(case.target, n)
    assert sorted(pos[arg]) == list(range(n))          # every list position wins once


def test_member_sizes_end_inside_and_on_rounds():
    ends = {n: n % LS.ROUND for n in LS.MEMBER_N}
    assert ends == {1: 1, 2: 2, 15: 15, 16: 0, 17: 1, 31: 15, 32: 0, 33: 1, 48: 0, 49: 1}
    assert {n > LS.E0 for n in LS.MEMBER_N} == {True, False}       # with and without a remainder phase
    assert LS.E0 == 2 * LS.ROUND and GC.LIST_MAX == LS.E0


@pytest.mark.parametrize("bound", LS.BOUNDS)
@pytest.mark.parametrize("n", LS.FACE_N)
def test_face_case(n, bound):
    case = LS.face_case(n, bound)
    assert n > GC.LIST_MAX and (n - LS.E0) % LS.ROUND != 0
    g = GC.Grid(case.target, bound)
    for q in case.source:
        exact_list(case, q, n)
    fine = g.fine(case.source, GC.MAX_LEVEL)
    cell = g.cell(case.source)
    per = 2 * len(LS.FACE_EPS)
    for a in range(3):
        rows = slice(a * per, (a + 1) * per)
        assert len(np.unique(cell[rows], axis=0)) == 1
        lo, hi = fine[rows][0::2, a], fine[rows][1::2, a]
        assert np.all(hi == lo + 1), (a, fine[rows])            # the two sides of one fine face
    m, arg, count = GC.brute(case.target, case.source)
    assert np.all(count == 1) and np.all(arg < n)
    idx, d = O.knn(case.target, case.source, 1)
    assert np.array_equal(idx[:, 0], arg) and np.array_equal(d[:, 0], m)


@pytest.mark.parametrize("bound", LS.BOUNDS)
@pytest.mark.parametrize("pos,total", LS.PAIRS)
def test_pair_case(pos, total, bound):
    case = LS.pair_case(pos, total, bound)
    i, j = pos
    ns = len(case.target) - len(GC.anchors())
    assert ns == total == case.expect["shell_n"]
    exact_list(case, case.source[0], total)
    m, _, count = GC.brute(case.target, case.source)
    assert count[0] == 2 and np.all(count[1:] == 1)
    d = GC.NP.nanoflann_sqd(case.source[0][None], case.target)
    assert set(np.flatnonzero(d == d.min())) == set(case.expect["pair"])
    lp = LS.list_position(case.target, total)
    a, b = case.expect["pair"]
    assert (int(lp[a]), int(lp[b])) == (i, j)
    # nanoflann keeps the point at the higher list position: a scan that misses the tie answers the other
    assert LT.ref_choice(case) == b and lp[b] > lp[a]


def test_pairs_cover_the_rounds():
    where = lambda p: p // LS.ROUND if p < LS.E0 else "remainder"
    assert all(where(i) == where(j) == 0 for (i, j), _ in LS.PAIRS_ONE_ROUND)
    assert all((where(i), where(j)) == (0, 1) for (i, j), _ in LS.PAIRS_TWO_ROUNDS)
    assert all(where(j) == "remainder" for (_, j), _ in LS.PAIRS_REMAINDER)
    assert ((0, 1), 2) in LS.PAIRS                                   # two entries, tied
    first_last = [(p, t) for p, t in LS.PAIRS if p == (0, t - 1)]
    assert {t % LS.ROUND != 0 for _, t in first_last} == {True, False} and len(first_last) >= 6


def test_team_winners_lie_in_other_members_chunks():
    case, heavy = LS.team()
    n, H = LS.TEAM
    F = LT.team_size(H)
    assert F == 4 and n > LS.E0
    _, arg, count = GC.brute(case.target, case.source)
    assert np.all(count == 1)
    pos = LS.list_position(case.target, n)[arg[heavy]]
    late = pos[pos >= LS.E0]
    assert len(late) >= 3
    members = {int((p - LS.E0) // LS.ROUND) % F for p in late}
    assert len(members) >= 2        # at least one winner is found by a lane that is not the chunk-0 member
