"""The inputs of tests/test_gpu_lookup_tail.py (tests/lookup_tail_cases.py) proven on the
CPU with GC.Grid's list rule, in plain numpy:

  * team_case(n, H): 64 queries; each heavy query's cell, at whatever level the build
    stops, lists exactly the n shell points (so n > E0 entries are left after the common
    rounds), each light query's cell lists one point or, outside the grid box, none
    (<= 16: done within the first round); H of the 64 are heavy, and in the device's lane
    order they follow at least one light lane (rank != lane); no query has a tied minimum;
    the grid about the shell's centre is the shell case's own;
  * why the light queries come from a distant point: for every "around" query of the
    shell case the list rule's radius admits more than 16 shell points;
  * the team size of every H run, and that the runs cover F = 1 .. 64 and idle teams;
  * the shell sources of the list-edge runs hold wavefronts with provably heavy and
    provably light lanes side by side, and the prefixes end inside a wavefront;
  * seam_pair (GC.tie_pair itself where the positions fit its list of 48) puts the tied
    points at the positions about E0 of lists of 48 or 96 entries, with the reference's
    choice at the higher position; the positions fall in the common rounds, in different members'
    chunks and in one chunk as named.
"""
import functools

import numpy as np
import pytest

import grid_cases as GC
import lookup_tail_cases as LT
from oracle import oracle as O

F32 = np.float32


@functools.lru_cache(maxsize=None)
def cell_lists(n):
    """{(level, cell, fine): (lower, upper) list length} of the cells the queries of every
    team_case(n, .) map to (the H = 64 and H = 1 sources hold every kind)."""
    tgt = LT.team_target(n)
    g = GC.Grid(tgt, LT.BOUND)
    t = tgt.astype(np.float64)
    out = {}
    for H in (64, 1):
        case, heavy = LT.team_case(n, H)
        for q, hv in zip(case.source, heavy):
            for lv, bc, hb in LT.final_cells(g, q):
                key = (lv, tuple(np.round(bc, 6)), bool(hv))
                if key in out:
                    continue
                Rlo, Rhi = GC.list_radius_bounds(t, bc, hb, g.capm)
                d = GC.box_dist(t, bc, hb)
                lo_set = d <= Rlo
                if hv:   # the n shell points, within the smallest radius, none dominated
                    assert lo_set[:n].all() and not GC.dominated_by_any(t, bc, hb)[:n].any(), (n, lv)
                    assert np.all(np.abs(GC.CENTRE - bc) <= hb), "a cell that holds the centre"
                out[key] = (int(lo_set[:n].sum()) if hv else 0, int((d <= Rhi).sum()))
    return out


@pytest.mark.parametrize("n", LT.TEAM_N)
def test_team_case_lists(n):
    lists = cell_lists(n)
    heavy = [v for k, v in lists.items() if k[2]]
    light = [v for k, v in lists.items() if not k[2]]
    assert len(heavy) >= 4 and len(light) >= 4
    assert all(lo == n and hi == n for lo, hi in heavy), heavy       # all n, at every level
    assert all(hi <= 1 for _, hi in light), light                    # FAR alone, or nothing: <= 16
    assert n > LT.E0
    # the far point moves neither the origin nor the cells about the centre
    g, g0 = GC.Grid(LT.team_target(n), LT.BOUND), GC.Grid(GC.shell(n, LT.BOUND).target, LT.BOUND)
    np.testing.assert_array_equal(g.origin, g0.origin)
    assert g.outside_nomatch and g.inside(LT.FAR.astype(F32))


@pytest.mark.parametrize("n", LT.TEAM_N)
def test_team_case_sources(n):
    tgt = LT.team_target(n)
    for H in LT.TEAM_H:
        case, heavy = LT.team_case(n, H)
        assert case.source.shape == (64, 3) and case.source.dtype == F32 and int(heavy.sum()) == H
        assert np.array_equal(case.target, tgt)
        g = GC.Grid(tgt, LT.BOUND)
        a = LT.before(n, H)
        src64 = case.source.astype(np.float64)
        d = np.linalg.norm(src64 - GC.CENTRE, axis=1)
        f = np.linalg.norm(src64 - LT.FAR, axis=1)
        out = np.linalg.norm(src64 - LT.OUT, axis=1) < LT.LIGHT_R + 1e-6
        assert np.all(d[heavy] < LT.HEAVY_R + 1e-6) and np.all((f[~heavy] < LT.LIGHT_R + 1e-6) | out[~heavy])
        assert int(out.sum()) == a and not g.inside(case.source[out]).any() and g.inside(case.source[~out]).all()
        m, arg, count = GC.brute(tgt, case.source)
        assert np.all(count == 1)
        assert np.all(arg[heavy] < n) and np.all(arg[~heavy & ~out] == len(tgt) - 1)
        assert np.array_equal(m.astype(np.float64) < LT.BOUND ** 2, ~out)
        # the device's lane order: the empty lanes, the heavy ones, the rest
        lanes = LT.lanes_of(case.source)
        assert len(lanes) == 1
        assert out[lanes[0]][:a].all() and heavy[lanes[0]][a:a + H].all()
        if H < 64:
            assert a >= 1


def test_heavy_lanes_sit_in_serving_and_in_idle_teams():
    """Runs exist whose heavy lanes all lie among the serving teams' lanes (below H F), and
    runs where some lie among the idle teams' lanes: such a lane is read by its team while
    it serves nobody itself."""
    kinds = set()
    for n in LT.TEAM_N:
        for H in LT.TEAM_H:
            F = LT.team_size(H)
            if H * F < 64:
                kinds.add(LT.before(n, H) + H > H * F)
    assert kinds == {True, False}
    late = [(n, H) for n in LT.TEAM_N for H in (3, 5, 9, 17) if LT.before(n, H) + H > H * LT.team_size(H)]
    assert {H for _, H in late} == {3, 5, 9, 17}, late


def test_team_sizes_cover_every_path():
    F = {H: LT.team_size(H) for H in LT.TEAM_H}
    assert F == {1: 64, 2: 32, 3: 16, 4: 16, 5: 8, 8: 8, 9: 4, 16: 4, 17: 2, 32: 2, 33: 1, 64: 1}
    assert {H * f < 64 for H, f in F.items()} == {True, False}        # idle teams, and none
    # chunks per member: none, one, several, and a last partial chunk
    for n in LT.TEAM_N:
        assert n > LT.E0
    chunks = {n: -(-(n - LT.E0) // LT.ROUND) for n in LT.TEAM_N}
    assert chunks == {33: 1, 47: 1, 48: 1, 49: 2, 161: 9, 2048: 126}
    assert [(n - LT.E0) % LT.ROUND for n in LT.TEAM_N] == [1, 15, 0, 1, 1, 0]


def test_around_queries_are_not_provably_light():
    """The shell's own "around" queries: the radius rule admits more than 16 points for every
    one of them (what dominance removes is not provable here), hence the distant point."""
    for n in (LT.TEAM_N[0], LT.TEAM_N[-1]):
        sh = GC.shell(n, LT.BOUND)
        g = GC.Grid(sh.target, LT.BOUND)
        t = sh.target.astype(np.float64)
        around = sh.source[256:512]
        cells = {tuple(c) for c in g.cell(around)}
        assert len(cells) >= 8
        for c in cells:
            bc, hb = g.box(np.array(c))
            R = GC.list_radius_bounds(t, bc, hb, g.capm)[1]
            assert int((GC.box_dist(t, bc, hb) <= R).sum()) > 16


@pytest.mark.parametrize("n", (LT.E0 + 1, LT.E0 + 17))
def test_edge_sources_mix_heavy_and_light_lanes(n):
    sh = GC.shell(n, LT.BOUND)
    g = GC.Grid(sh.target, LT.BOUND)
    near = np.flatnonzero(np.linalg.norm(sh.source.astype(np.float64) - GC.CENTRE, axis=1) < 0.1)
    lo = np.zeros(len(sh.source), np.int64)
    for i in near:
        lo[i] = min(b[1] for b in LT.list_bounds(sh.target, g, sh.source[i]))
    outside = ~g.inside(sh.source)
    waves = LT.lanes_of(sh.source)
    heavy = [int((lo[w] > LT.E0).sum()) for w in waves]
    assert max(heavy) >= 16 and sum(h > 0 for h in heavy) >= 3       # lower bounds: at least so many
    assert outside.any()                                              # lanes with an empty list
    assert len(sh.source) > max(LT.EDGE_PREFIXES) and {m % 64 for m in LT.EDGE_PREFIXES} == {1, 63}


def test_edge_sizes_straddle_e0():
    assert LT.E0 % LT.ROUND == 0 and GC.LIST_MAX == LT.E0    # (a list of E0 + 1 is also the first refined one)
    assert [n - LT.E0 for n in LT.EDGE_N] == [-1, 0, 1, 16, 17]
    assert LT.SHARD_N == LT.E0 + 17 and LT.ALIGN_N == LT.E0 + 33


@pytest.mark.parametrize("pos", LT.PAIR_POSITIONS)
@pytest.mark.parametrize("bound", LT.PAIR_BOUNDS)
def test_tie_pair_positions_about_e0(pos, bound):
    case = LT.seam_pair(pos, bound)
    i, j = pos
    ns = len(case.target) - len(GC.anchors())          # the shell points = the list
    assert ns == (48 if j < 48 else LT.SEAM_TOTAL) == case.expect["shell_n"]
    if j < 48:
        ref = GC.tie_pair(pos, bound)
        assert np.array_equal(ref.target, case.target) and np.array_equal(ref.source, case.source)
    m, _, count = GC.brute(case.target, case.source)
    assert count[0] == 2 and np.all(count[1:] == 1)
    d = GC.NP.nanoflann_sqd(case.source[0][None], case.target)
    assert set(np.flatnonzero(d == d.min())) == set(case.expect["pair"])
    order, key = GC.morton_order(case.target)
    assert len(np.unique(key[:ns])) == ns
    t = case.target.astype(np.float64)
    g = GC.Grid(case.target, bound)
    for lv, bc, hb in LT.final_cells(g, case.source[0]):
        Rlo, Rhi = GC.list_radius_bounds(t, bc, hb, g.capm)
        for R in (Rlo, Rhi):
            listed = [int(k) for k in order if GC.box_dist(t[k], bc, hb) <= R]
            assert len(listed) == ns and max(listed) < ns
            assert (listed.index(case.expect["pair"][0]), listed.index(case.expect["pair"][1])) == pos
        assert not GC.dominated_by_any(t, bc, hb)[:ns].any()
    # the reference keeps the point at the higher list position
    assert LT.ref_choice(case) == case.expect["pair"][1] and listed.index(case.expect["pair"][1]) == j > i
    assert ns > LT.E0 and j >= LT.E0


def test_tie_pair_positions_cover_the_seams():
    """Which scan meets each tied point when the centre query's list is shared by a team of
    F = 64 (the one-query source) -- chunk c = (position - E0) // 16, member c % F."""
    where = lambda p: "common" if p < LT.E0 else (p - LT.E0) // LT.ROUND
    got = {pos: (where(pos[0]), where(pos[1])) for pos in LT.PAIR_POSITIONS}
    assert got == {(0, 32): ("common", 0), (31, 32): ("common", 0), (32, 48): (0, 1), (47, 48): (0, 1),
                   (35, 72): (0, 2), (33, 34): (0, 0)}
