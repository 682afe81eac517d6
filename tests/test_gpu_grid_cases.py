"""The candidate-cell build (cellgrid.hip, cellgrid_build in cellgrid_host.hip) and its three
lookups on synthetic targets that force each path (tests/grid_cases.py; their
properties are proven in tests/test_grid_cases_cpu.py): the fused lookup inside
k_moments<*, true> (moments.hip; bounds 0.5 and 1.0, no fallback cell), k_cell_lookup
with the walk behind it (corr_search.hip; bound 5.0, and the over-cap targets at every
bound), and the walk alone (cells off).

Bars, all exact: correspondences and squared distances of every query, ties included,
assert_array_equal to the oracle's (nanoflann's own order); cells on and cells off bit
for bit in correspondences, distances, H, b, cost and count; on the tie-free cases the
index and distance of the numpy brute-force fp32 minimum, which shares no code with the
other two; grid_info() shows the path the case names, and its coarse_cells equals the
dimensions restated in grid_cases.Grid.  Aligns: the walk's pose, iterations and LM
trials bit for bit, the oracle's pose to 1e-6 and its counts exactly (the bars of
test_gpu_grid.test_grid_align_equals_walk_and_oracle).
"""
import functools
import json

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
import grid_cases as GC
import np_gicp as NP
from dynamic_direct_lidar_odometry_amd import SOURCE, TARGET, scene
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def spd(n, rng):
    """Random SPD covariances, as test_gpu_grid.test_grid_tied_targets makes them."""
    A = rng.normal(0, 0.05, (n, 3, 3))
    return np.ascontiguousarray(NP.mat_to_sym6(A @ np.transpose(A, (0, 2, 1)) + 1e-3 * np.eye(3)))


def make(tgt, src, tcov, scov, grid, **kw):
    c = P.Context(0)
    c.set_params(P.default_params(**kw))
    c.set_target_grid(grid)
    c.set_target(tgt)
    c.set_covariances(TARGET, tcov)
    c.set_source(src)
    c.set_covariances(SOURCE, scov)
    return c


_BRUTE = {}


def brute(name, bound, gen):
    """(case, brute-force minimum, argmin, tie count), computed once per (name, bound)."""
    if (name, bound) not in _BRUTE:
        case = gen()
        _BRUTE[name, bound] = (case,) + GC.brute(case.target, case.source)
    return _BRUTE[name, bound]


def check_info(case, info, walk_groups):
    e = case.expect
    print(e["name"], case.bound, json.dumps(info), "walk_groups", walk_groups)
    g = GC.Grid(case.target, case.bound)
    assert info["built"] == 1 and info["build_status"] == 0
    assert info["coarse_cells"] == g.coarse_cells, (info["coarse_cells"], g.dims)
    assert info["uses_walk"] == e["uses_walk"]
    for l in e["levels"]:
        assert info["level_cells"][l] > 0, (l, info["level_cells"])
    if e["refined"]:
        assert sum(info["level_cells"][1:]) > 0
    for key, counter in (("overflow", "overflow_cells"), ("fallback", "fallback_fine")):
        if e[key] is not None:
            assert (info[counter] > 0) == e[key], (counter, info[counter])
    if e["over_cap"]:
        assert info["overflow_cells"] > 0 or info["fallback_fine"] > 0
    assert info["entries"] >= e["min_entries"]
    if e["walk_groups"] is not None:
        assert (walk_groups > 0) == e["walk_groups"], walk_groups


def run_case(name, bound, gen, nsrc=None):
    """One linearize at the case's pose with the cells on and off, against the oracle and
    (tie-free cases) the brute force.  Returns (correspondences, distances, info)."""
    case, bmin, barg, bcnt = brute(name, bound, gen)
    src = case.source if nsrc is None else np.ascontiguousarray(case.source[:nsrc])
    rng = np.random.default_rng(1)
    tcov, scov = spd(len(case.target), rng), spd(len(case.source), rng)[:len(src)]
    kw = dict(k_correspondences=10, max_correspondence_distance=case.bound)
    cg = make(case.target, src, tcov, scov, P.GRID_ON, **kw)
    cw = make(case.target, src, tcov, scov, P.GRID_OFF, **kw)
    o = O.Gicp(src, case.target, O.default_params(**kw))
    o.set_covariances(0, scov)
    o.set_covariances(1, tcov)
    try:
        Hg, bg, costg, ng = cg.linearize(case.pose)
        walk_groups = cg.lookup_walk_groups()
        Hw, bw, costw, nw = cw.linearize(case.pose)
        corr_g, sqd_g = cg.correspondences()
        corr_w, sqd_w = cw.correspondences()
        info = cg.grid_info()
        check_info(case, info, walk_groups)
        assert cw.grid_info()["built"] == 0
        _, _, _, ocorr, osqd = o.linearize(case.pose)
        # the oracle, every query, ties included
        np.testing.assert_array_equal(corr_g, ocorr)
        np.testing.assert_array_equal(sqd_g, osqd)
        # the walk, bit for bit
        np.testing.assert_array_equal(corr_g, corr_w)
        np.testing.assert_array_equal(sqd_g, sqd_w)
        np.testing.assert_array_equal(Hg, Hw)
        np.testing.assert_array_equal(bg, bw)
        assert costg == costw and ng == nw
        m = len(src)
        match = bmin[:m].astype(np.float64) < case.bound ** 2
        assert ng == int(match.sum())
        if case.expect["tie_free"]:
            assert not (bcnt[:m] > 1).any()
            np.testing.assert_array_equal(corr_g, np.where(match, barg[:m], -1))
            np.testing.assert_array_equal(sqd_g, bmin[:m])
        else:   # the distance is the minimum whichever tied point is taken, and the point is one of the tied
            np.testing.assert_array_equal(sqd_g, bmin[:m])
            d = NP.nanoflann_sqd(src[match], case.target[corr_g[match]])
            np.testing.assert_array_equal(d, bmin[:m][match])
        return corr_g, sqd_g, info
    finally:
        cg.close()
        cw.close()


@pytest.mark.parametrize("n,bound", GC.shell_runs())
def test_shell(n, bound):
    """Lists of n entries: within one fused round, at its end, one past it, up to LIST_CAP."""
    run_case(f"shell{n}", bound, functools.partial(GC.shell, n, bound))


@pytest.mark.parametrize("bound", GC.BOUNDS)
@pytest.mark.parametrize("n", GC.SHELL_OVER_NS)
def test_shell_over_cap(n, bound):
    """More candidates than kCgCandMax about the centre: its cells have no list, the walk
    answers their queries (at every bound: the fused lookup is not taken)."""
    _, _, info = run_case(f"shell_over{n}", bound, functools.partial(GC.shell_over, n, bound))
    print("over-cap counters:", {k: info[k] for k in ("overflow_cells", "fallback_fine")})


@pytest.mark.parametrize("bound", GC.BOUNDS)
def test_dense_cube(bound):
    """The coarse candidate set overflows and is split directly; the fine lists are stored."""
    run_case("dense_cube", bound, functools.partial(GC.dense_cube, bound))


@pytest.mark.parametrize("bound", GC.BOUNDS)
def test_tie_rounds(bound):
    """Ties of 48, 8, 6, 4 and 2 list entries across fused rounds and k_cell_lookup's slices:
    found from the list and re-run in nanoflann's order."""
    run_case("tie_rounds", bound, functools.partial(GC.tie_rounds, bound))


@pytest.mark.parametrize("bound", GC.BOUNDS)
@pytest.mark.parametrize("pos", GC.PAIR_POSITIONS)
def test_tie_pair(pos, bound):
    """Two tied entries at list positions (0, 16), (15, 16), (0, 47): the second distance must
    survive from one round, or one slice, to another."""
    run_case(f"tie_pair{pos}", bound, functools.partial(GC.tie_pair, pos, bound))


@pytest.mark.parametrize("bound", GC.BOUNDS)
def test_faces(bound):
    """Queries on, and 1 and 2 ulp off, every coarse and level-3 fine face of the refined cell."""
    run_case("faces", bound, functools.partial(GC.faces, bound))


@pytest.mark.parametrize("bound", GC.BOUNDS)
@pytest.mark.parametrize("k", range(4))
def test_far_origin(k, bound):
    run_case(f"far{k}", bound, lambda: GC.far_origin(bound)[k])


@pytest.mark.parametrize("bound", GC.BOUNDS)
@pytest.mark.parametrize("kind", GC.DEGENERATE)
def test_degenerate(kind, bound):
    run_case(f"degenerate_{kind}", bound, functools.partial(GC.degenerate, kind, bound))


@pytest.mark.parametrize("bound", GC.BOUNDS)
def test_wide_box(bound):
    """A query the fp32 mapping puts into the cell behind a face it has not reached: its nearest
    point is on that cell's list only because every box is expanded by delta."""
    run_case("wide_box", bound, functools.partial(GC.wide_box, bound))


@pytest.mark.parametrize("bound", GC.BOUNDS)
def test_sizes(bound):
    """Source lengths about the fused kernel's 64-query and k_cell_lookup's 16-query groups:
    every prefix is answered exactly as the full set is."""
    gen = functools.partial(GC.sizes, bound)
    corr, sqd, _ = run_case("sizes", bound, gen)
    for m in GC.SIZES:
        c, s, _ = run_case("sizes", bound, gen, nsrc=m)
        np.testing.assert_array_equal(c, corr[:m])
        np.testing.assert_array_equal(s, sqd[:m])


def perturbed(dt, yaw):
    return scene.make_pose(np.array([dt, -0.5 * dt, 0.1 * dt]), (0.2 * yaw, -0.1 * yaw, yaw)).astype(np.float32)


@pytest.mark.parametrize("name", ["shell33", "dense_cube", "tie_rounds"])
def test_align_equals_walk_and_oracle(name):
    """One align from a small perturbed guess through the fused LM kernel with the lookup inside."""
    bound = 1.0
    case = {"shell33": lambda: GC.shell(33, bound), "dense_cube": lambda: GC.dense_cube(bound),
            "tie_rounds": lambda: GC.tie_rounds(bound)}[name]()
    rng = np.random.default_rng(1)
    tcov, scov = spd(len(case.target), rng), spd(len(case.source), rng)
    kw = dict(k_correspondences=10, max_correspondence_distance=bound, max_iterations=32, transformation_epsilon=0.01)
    cg = make(case.target, case.source, tcov, scov, P.GRID_ON, **kw)
    cw = make(case.target, case.source, tcov, scov, P.GRID_OFF, **kw)
    o = O.Gicp(case.source, case.target, O.default_params(**kw))
    o.set_covariances(0, scov)
    o.set_covariances(1, tcov)
    G = perturbed(0.05, 0.005)
    pg, rg = cg.align(G)
    pw, rw = cw.align(G)
    info = cg.grid_info()
    print(name, json.dumps(info), (rg.iterations_run, rg.lm_trials, rg.converged))
    assert info["built"] == 1 and info["uses_walk"] == 0 and cg.lookup_walk_groups() == 0
    np.testing.assert_array_equal(pg, pw)
    assert (rg.iterations_run, rg.lm_trials, rg.converged) == (rw.iterations_run, rw.lm_trials, rw.converged)
    po, ro = o.align(G)
    np.testing.assert_allclose(pg, po, atol=1e-6)
    assert (rg.iterations_run, rg.lm_trials, rg.converged) == (ro.iterations_run, ro.lm_trials, ro.converged)
    np.testing.assert_array_equal(cg.correspondences()[0], o.last_correspondences()[0])
    np.testing.assert_array_equal(cg.correspondences()[0], cw.correspondences()[0])
    cg.close()
    cw.close()


@pytest.mark.parametrize("bound", [1.0, 5.0])
def test_sharded_lookup(bound):
    """shell(33) cut through by a slab (x >= the centre's) and by interleaved 16-query groups
    (part 1 of 3, set_shard_groups): the owned queries have the unsharded result, the others no match, in the
    fused lookup (bound 1.0) and in k_cell_lookup (bound 5.0), as in the walk."""
    gen = functools.partial(GC.shell, 33, bound)
    corr, sqd, _ = run_case("shell33", bound, gen)
    case = brute("shell33", bound, gen)[0]
    rng = np.random.default_rng(1)
    tcov, scov = spd(len(case.target), rng), spd(len(case.source), rng)
    kw = dict(k_correspondences=10, max_correspondence_distance=bound)
    lo = float(case.expect["centre"][0])
    # the groups are 16 consecutive points of the source in its sorted (Morton) order on the device
    rank = np.empty(len(case.source), np.int64)
    rank[GC.morton_order(case.source)[0]] = np.arange(len(case.source))
    own = (case.source[:, 0] >= np.float32(lo)) & ((rank // 16) % 3 == 1)
    assert own.any() and (~own).any() and (corr[own] >= 0).any() and (corr[~own] >= 0).any()
    got = {}
    for grid in (P.GRID_ON, P.GRID_OFF):
        c = make(case.target, case.source, tcov, scov, grid, **kw)
        c.set_shard(0, lo, np.inf)
        c.set_shard_groups(3, 1)
        H, b, cost, n = c.linearize(case.pose)
        got[grid] = (H, b, cost, n) + c.correspondences()
        if grid == P.GRID_ON:
            info = c.grid_info()
            assert info["built"] == 1 and info["uses_walk"] == int(bound > 1.0)
        c.close()
    H, b, cost, n, scorr, ssqd = got[P.GRID_ON]
    np.testing.assert_array_equal(scorr[own], corr[own])
    np.testing.assert_array_equal(ssqd[own], sqd[own])
    assert np.all(scorr[~own] == -1)
    assert n == int((corr[own] >= 0).sum())
    Hw, bw, costw, nw, wcorr, wsqd = got[P.GRID_OFF]
    np.testing.assert_array_equal(scorr, wcorr)
    np.testing.assert_array_equal(H, Hw)
    np.testing.assert_array_equal(b, bw)
    assert cost == costw and n == nw
