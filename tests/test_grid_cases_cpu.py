"""The synthetic candidate-cell targets (tests/grid_cases.py) proven on the CPU, in plain
numpy with np_gicp.nanoflann_sqd for the fp32 distance: the device tests
(tests/test_gpu_grid_cases.py) rest on these properties of their inputs.

  * a case called tie-free has no query with two target points at a bit-equal fp32
    minimum distance (allowed share: 0);
  * the tie cases have exactly the intended number of bit-equal minima at every query, and
    the positioned pairs sit at the intended positions of the centre cell's list;
  * the face queries straddle: the lookup's fp32 cell mapping sends the -1 ulp and +1 ulp
    neighbours of every face to different cells (coarse faces) and different level-3 fine
    cells (all faces);
  * the cells that hold a shell's centre have exactly the n shell points within their
    list radius, none dominated by any other target point;
  * every source has matches and non-matches against the bound where the case says both;
  * wide_box's first query is mapped by the lookup into a cell whose unexpanded box does
    not hold it, and its nearest point is on that cell's list only through delta.
"""
import numpy as np
import pytest

import grid_cases as GC
from oracle import oracle as O

F32 = np.float32


def ids(cases):
    return [f"{c.expect['name']}-{c.bound}" for c in cases]


TIE_FREE = GC.tie_free_cases()


@pytest.mark.parametrize("case", TIE_FREE, ids=ids(TIE_FREE))
def test_tie_free_cases_have_no_tied_minimum(case):
    assert case.expect["tie_free"]
    assert case.target.dtype == F32 and case.source.dtype == F32
    assert len(case.target) <= 4096 and len(case.source) <= 2048
    np.testing.assert_array_equal(case.pose, np.eye(4))
    m, _, count = GC.brute(case.target, case.source)
    assert int((count > 1).sum()) == 0, np.flatnonzero(count > 1)
    if case.expect["both"]:
        match = m.astype(np.float64) < case.bound ** 2
        assert match.any() and (~match).any()


def centre_cells(case):
    """The boxes (centre, half size) of the cells that can hold the shell's centre: every
    level's fine cells whose expanded box contains it."""
    g = GC.Grid(case.target, case.bound)
    c = case.expect["centre"]
    out = []
    kc = g.cell(c.astype(F32))
    for level in range(GC.MAX_LEVEL + 1):
        m = 1 << level
        for f in np.ndindex(m, m, m):
            bc, hb = g.box(kc, level, f)
            if np.all(np.abs(c - bc) <= hb):
                out.append((level, bc, hb))
    return g, out


SHELLS = [GC.shell(n, b) for n, b in GC.shell_runs()] + [GC.shell_over(n, 1.0) for n in GC.SHELL_OVER_NS] + \
         [GC.tie_rounds(b) for b in GC.BOUNDS] + [GC.tie_pair(p, 1.0) for p in GC.PAIR_POSITIONS] + [GC.faces(1.0)]


@pytest.mark.parametrize("case", SHELLS, ids=ids(SHELLS))
def test_shell_points_are_the_centre_cells_candidates(case):
    """Exactly the n shell points lie within the list radius of every cell that holds the
    centre (for the smallest and the largest radius the build can take), and no target
    point dominates one of them over such a cell: its list is the n points."""
    n = case.expect["shell_n"]
    g, cells = centre_cells(case)
    assert [lv for lv, _, _ in cells].count(0) == 1 and len(cells) >= 1 + 3 * 1
    t = case.target.astype(np.float64)
    for level, bc, hb in cells:
        for R in GC.list_radius_bounds(t, bc, hb, g.capm):
            within = GC.box_dist(t, bc, hb) <= R
            assert int(within.sum()) == n and within[:n].all(), (level, R, int(within.sum()))
        assert not GC.dominated_by_any(t, bc, hb)[:n].any(), level


def test_geometry_restated():
    """The restated grid at the three bounds: the reach, the margin, and which bounds take
    the fused lookup (capm <= nomatch_dist) or keep the walk."""
    tgt = GC.shell(33, 1.0).target
    for bound, r, M, fused in ((0.5, 3, 1.6, True), (1.0, 4, 2.0, True), (5.0, 11, 4.8, False)):
        g = GC.Grid(tgt, bound)
        assert g.r == r and abs(g.M - M) < 1e-12 and g.outside_nomatch == fused
        np.testing.assert_array_equal(g.dims, [int(np.ceil((4.0 + 2 * g.M) / GC.CELL)) + 1] * 3)
        # the shell's centre is the centre of a coarse cell (to the rounding of the fp32 origin)
        c, _ = g.box(g.cell(GC.CENTRE.astype(F32)))
        assert np.abs(c - GC.CENTRE).max() < 1e-6


@pytest.mark.parametrize("bound", GC.BOUNDS)
def test_tie_rounds_multiplicities(bound):
    case = GC.tie_rounds(bound)
    _, _, count = GC.brute(case.target, case.source)
    want = np.array([case.expect["ties"].get(i, 1) for i in range(len(case.source))])
    np.testing.assert_array_equal(count, want)
    assert sorted(set(case.expect["ties"].values())) == [2, 4, 6, 8, 48]
    # the 48 tied points of the centre query, in list (sorted) order: three fused rounds, all four slices
    d = GC.NP.nanoflann_sqd(case.source[0][None], case.target)
    tied = np.flatnonzero(d == d.min())
    assert len(tied) == 48 and set(tied) == set(range(48))
    # the reference's choices differ from the lowest list position at most tied queries
    order, _ = GC.morton_order(case.target)
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    pick = O.knn(case.target, case.source, 1)[0][:, 0]
    differ = 0
    for q in case.expect["ties"]:
        dq = GC.NP.nanoflann_sqd(case.source[q][None], case.target)
        cand = np.flatnonzero(dq == dq.min())
        assert pick[q] in cand
        differ += int(pick[q] != cand[np.argmin(rank[cand])])
    assert differ >= len(case.expect["ties"]) // 2
    assert 48 == 3 * GC.ROUND and 48 % GC.SLICES == 0


@pytest.mark.parametrize("pos", GC.PAIR_POSITIONS)
@pytest.mark.parametrize("bound", GC.BOUNDS)
def test_tie_pair_positions(pos, bound):
    """The two tied points sit at the intended positions of the centre cell's list: their
    ranks, in sorted target order, among the points within the list radius (the 48 shell
    points, none dominated: test_shell_points_are_the_centre_cells_candidates)."""
    case = GC.tie_pair(pos, bound)
    _, _, count = GC.brute(case.target, case.source)
    want = np.array([case.expect["ties"].get(i, 1) for i in range(len(case.source))])
    np.testing.assert_array_equal(count, want)
    d = GC.NP.nanoflann_sqd(case.source[0][None], case.target)
    assert set(np.flatnonzero(d == d.min())) == set(case.expect["pair"])
    order, key = GC.morton_order(case.target)
    assert len(np.unique(key[:48])) == 48
    g, cells = centre_cells(case)
    for level, bc, hb in cells:
        R = GC.list_radius_bounds(case.target, bc, hb, g.capm)[1]
        listed = [int(i) for i in order if GC.box_dist(case.target[i].astype(np.float64), bc, hb) <= R]
        assert len(listed) == 48
        assert (listed.index(case.expect["pair"][0]), listed.index(case.expect["pair"][1])) == pos
    # the reference's choice is the point at the higher list position: a lookup that misses the tie
    # (and so keeps the lowest position) differs from it
    assert int(O.knn(case.target, case.source[:1], 1)[0][0, 0]) == case.expect["pair"][1]
    i, j = pos
    assert (i // GC.ROUND != j // GC.ROUND) and (pos == (0, 16) or i % GC.SLICES != j % GC.SLICES)


FACES = [GC.faces(b) for b in GC.BOUNDS] + [c for b in GC.BOUNDS for c in GC.far_origin(b) if "face_rows" in c.expect]


@pytest.mark.parametrize("case", FACES, ids=ids(FACES))
def test_face_queries_straddle(case):
    g = GC.Grid(case.target, case.bound)
    rows = case.expect["face_rows"]
    assert len(rows) == 27
    kc = g.cell(case.expect["centre"].astype(F32))
    for a, f, r0 in rows:
        q = case.source[r0:r0 + 5]
        assert g.inside(q).all()
        assert np.all(np.diff(q[:, a].astype(np.float64)) > 0) and q[2, a] == g.face(a, int(kc[a]), f)
        for b in range(3):
            if b != a:   # the other two coordinates stay inside the centre's coarse cell
                assert np.all(g.cell(q)[:, b] == kc[b])
        coarse = g.cell(q)[:, a]
        fine = coarse * 8 + g.fine(q, 3)[:, a]
        assert fine[1] != fine[3], (a, f, fine)          # -1 ulp and +1 ulp: different level-3 cells
        assert fine[1] == fine[0] and fine[3] == fine[4]
        assert fine[3] - fine[1] == 1 and fine[3] == kc[a] * 8 + f
        if f in (0, 8):
            assert coarse[1] != coarse[3], (a, f, coarse)


def test_far_origin_cases_keep_their_shape():
    """Far from the origin the rounded clouds still hold matches and non-matches, and delta
    has grown as the build computes it."""
    for bound in GC.BOUNDS:
        for case in GC.far_origin(bound):
            g = GC.Grid(case.target, bound)
            assert g.delta > (0.1 if "far2" in case.expect["name"] else 0.03)
            m, _, _ = GC.brute(case.target, case.source)
            match = m.astype(np.float64) < bound ** 2
            assert match.any() and (~match).any()
            assert len(np.unique(case.target, axis=0)) == len(case.target)


@pytest.mark.parametrize("bound", GC.BOUNDS)
def test_degenerate_targets(bound):
    for kind in GC.DEGENERATE:
        case = GC.degenerate(kind, bound)
        g = GC.Grid(case.target, bound)
        ext = case.target.max(0) - case.target.min(0)
        flat = int((ext == 0).sum())
        assert flat == {"one": 3, "coincident": 3, "collinear": 2, "planar": 1}[kind]
        assert np.all(g.dims[ext == 0] == int(np.ceil(2 * g.M / GC.CELL)) + 1)   # the margins alone
        m, _, count = GC.brute(case.target, case.source)
        match = m.astype(np.float64) < bound ** 2
        assert match.any() and (~match).any() and (m == 0).any() and g.inside(case.source).any() and (~g.inside(case.source)).any()
        np.testing.assert_array_equal(count, 2 if kind == "coincident" else 1)


def test_sizes_are_prefixes_that_cross_the_group_sizes():
    case = GC.sizes(1.0)
    assert max(GC.SIZES) <= len(case.source)
    assert {m % 16 for m in GC.SIZES} >= {0, 1, 15} and {m % 64 for m in GC.SIZES} >= {0, 1, 63}


@pytest.mark.parametrize("bound", GC.BOUNDS)
def test_wide_box_needs_delta(bound):
    case = GC.wide_box(bound)
    g = GC.Grid(case.target, bound)
    w = case.expect["wide"]
    q = case.source[0]
    # mapped into the cell behind the face, though before the face
    assert tuple(g.cell(q)) == w["cell"] and float(q[0]) < w["X0"]
    bc, hb = g.box(w["cell"])
    assert w["X0"] - float(q[0]) < 0.1 * g.delta and abs((bc[0] - (hb - g.delta)) - w["X0"]) < 1e-9
    # its nearest point is p, by far more than the fp32 rounding of the distances
    d = GC.NP.nanoflann_sqd(q[None], case.target).astype(np.float64)
    assert int(np.argmin(d)) == w["p"] and np.sort(d)[1] / d[w["p"]] - 1.0 > 1e-5 and d[w["p"]] < bound ** 2
    # d beats p over the unexpanded cell by more than the margin; over the expanded one it does not
    P_, D_ = case.target[w["p"]], case.target[w["d"]]
    assert GC.margin_dominated(P_, D_, bc, hb - g.delta) and not GC.margin_dominated(P_, D_, bc, hb)
    # d is a dominator of the cell (the point nearest to its centre), p is within the list radius
    t = case.target.astype(np.float64)
    assert int(np.argmin(((t - bc) ** 2).sum(1))) == w["d"]
    assert GC.box_dist(t[w["p"]], bc, hb) <= GC.list_radius_bounds(t, bc, hb, g.capm)[0]
