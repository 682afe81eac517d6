"""The generators of tests/walk_cases.py, proven with the brute force and the two bounds on
B2 (no device): every scripted step shows what its docstring names, at least 90 % of its
queries are decided (the pass rule gives one answer for B2 at both bounds), the steps built
to show passes hold at least one sure pass and one sure search, and the edge sweeps list
which queries are undecided on purpose.  The oracle's truncated aligns show that LM records
naturally on the align case."""
import numpy as np
import pytest

import np_gicp as NP
import walk_cases as WC
from oracle import oracle as O

F32 = np.float32


def moved(case, s):
    a = NP.transform_f32(case.script[s - 1][0], case.source).astype(np.float64)
    b = NP.transform_f32(case.script[s][0], case.source).astype(np.float64)
    return np.linalg.norm(b - a, axis=1)


def common(case, sim, decided_share=0.9):
    purpose = np.zeros(len(case.source), bool)
    purpose[list(case.expect["purpose"])] = True
    for s, st in enumerate(sim):
        pose = case.script[s][0]
        assert np.array_equal(pose, pose.astype(F32).astype(np.float64)), "poses are exact float32 values"
        if case.expect["tie_free"]:
            assert (st.cnt == 1).all(), (case.name, s, np.flatnonzero(st.cnt > 1))
        assert not (st.sure_pass & st.sure_search).any()
        own = st.owned & ~purpose
        if own.any():
            share = 1.0 - (st.undecided & own).sum() / own.sum()
            print(case.name, "step", s, "rec", case.script[s][1], "sure pass", int((st.sure_pass & own).sum()),
                  "sure search", int((st.sure_search & own).sum()), "undecided", int((st.undecided & own).sum()))
            if not case.expect.get("gap0"):   # (a live reference of iteration 0: see walk_cases.steps)
                assert share >= decided_share, (case.name, s, share)
    for s in case.expect["pass_steps"]:
        assert sim[s].sure_pass.any() and sim[s].sure_search.any(), (case.name, s)
    for s in case.expect.get("all_pass_steps", ()):
        assert sim[s].sure_pass.all(), (case.name, s)
    assert len(case.target) <= 20000 and len(case.source) <= 2000


def test_rule_and_bounds():
    """The restated rule on hand-made references: a tie can never be proven, the bound's two
    ends order, and a wider B2 never turns a pass into a search."""
    cap2 = WC.cap2_of(1.0)
    assert cap2 == np.nextafter(F32(1.0), F32(2.0))
    q = np.array([[0.0, 0.0, 0.0]], F32)
    p1 = np.array([[0.1, 0.0, 0.0]], F32)
    d1 = NP.nanoflann_sqd(q, p1)
    yes = np.array([True])
    assert not WC.pass_rule(q, q, d1, p1, yes, cap2)[0]                       # B2 <= d1 (a tie): never
    assert WC.pass_rule(q, q, F32(0.04), p1, yes, cap2)[0]                    # the next point at 0.2 m
    assert not WC.pass_rule(q + F32(0.08), q, F32(0.04), p1, yes, cap2)[0]    # moved 0.14 m
    assert not WC.pass_rule(q, q, F32(-1.0), p1, yes, cap2)[0]                # no reference
    assert WC.pass_rule(q, q, F32(1.21), p1, ~yes, cap2)[0]                   # nothing within 1.1 m
    assert not WC.pass_rule(q + F32(0.1), q, F32(1.21), p1, ~yes, cap2)[0]
    lo, hi = WC.b2_bounds(np.array([0.01, 0.01, 4.0], F32), np.array([0.012, 0.5, 9.0], F32), cap2, WC.REUSE_GAP)
    assert (lo <= hi).all()
    assert lo[0] == hi[0] == F32(0.012)                                       # d2 inside the widened radius: exact
    assert lo[1] == np.nextafter(F32((0.1 + 0.05) ** 2), F32(1)) or abs(float(lo[1]) - 0.0225) < 1e-8
    assert hi[2] == F32(4.0) and abs(float(lo[2]) - 1.05 ** 2) < 1e-6         # none within the bound
    lo0, _ = WC.b2_bounds(np.array([0.01], F32), np.array([0.5], F32), cap2, 0.0)
    assert lo0[0] == F32(0.01)                                                # gap 0: not widened


@pytest.mark.parametrize("variant", sorted(WC.STEPS_RECS))
def test_steps(variant):
    case, sim = WC.cached("steps", variant)
    common(case, sim)
    assert len(case.target) > WC.LEAF * WC.FANOUT and len(case.source) == 1000
    cap2 = WC.cap2_of(case.bound)
    assert (sim[0].d1 < cap2).mean() > 0.95, "the queries at the guess lie near the target"
    for s, lo, hi in ((1, 0.029, 0.031), (2, 0.009, 0.011), (3, 0.0015, 0.0025), (4, 0.059, 0.061)):
        m = moved(case, s)
        assert (m > lo).all() and (m < hi).all(), (s, m.min(), m.max())
    assert (moved(case, 5) < WC.TRI_MV).all() and (moved(case, 5) > 0.18).all()      # the triangle bound
    assert (moved(case, 6) > WC.TRI_MV).all() and (moved(case, 6) < 0.26).all()      # the previous match + window
    assert (sim[7].d1.astype(np.float64) >= case.bound ** 2).mean() > 0.5            # most lose their match
    assert np.array_equal(case.script[8][0], case.script[3][0])
    my = moved(case, 9)
    assert (my < WC.REUSE_REC_EPS).sum() >= 10 and (my > WC.TRI_MV).sum() >= 100
    assert np.array_equal(case.script[10][0], case.script[3][0])
    if variant == "natural":
        assert not sim[1].sure_pass.any()                    # nothing recorded before step 1
        assert sim[2].sure_pass.mean() > 0.5                 # + 0.01 m: most pass
        assert sim[4].sure_pass.sum() < sim[2].sure_pass.sum() // 4   # beyond the gap: few
        assert sim[8].sure_pass.sum() >= 100                 # references recorded long ago prove again


def test_far_origin():
    case, sim = WC.cached("far_origin")
    common(case._replace(expect=dict(case.expect, tie_free=False)), sim)
    assert np.abs(case.target).max() > 8000


@pytest.mark.parametrize("bound", [0.5, 1.0])
def test_bound(bound):
    case, sim = WC.cached("bound_case", bound)
    common(case, sim)
    kinds = case.expect["kinds"]
    cap2 = WC.cap2_of(bound)
    b2 = F32(bound * bound)
    at, below, above = (kinds.index(k) for k in ("at", "below", "above"))
    assert np.array_equal(NP.transform_f32(case.script[0][0], case.source), case.source)
    assert sim[0].d1[at] == b2 and sim[0].d1[below] == np.nextafter(b2, F32(0)) and sim[0].d1[above] == cap2
    assert float(sim[0].d1[below]) < bound ** 2 <= float(sim[0].d1[at])   # the oracle's <: only `below` is matched
    assert case.expect["purpose"] == (at, below, above)
    lo1, hi1 = WC.b2_bounds(sim[1].d1, sim[1].d2, cap2, WC.REUSE_GAP)
    radius = WC.widened(cap2, WC.REUSE_GAP)
    for i, k in enumerate(kinds):
        if isinstance(k, str):
            continue
        assert abs(np.sqrt(float(sim[0].d1[i])) - (bound + k)) < 1e-5 and sim[0].d1[i] > cap2
        assert sim[1].sure_search[i]                      # recorded at gap0 = 0: B2 = cap2 proves nothing
        if k >= 0.06:
            assert lo1[i] == radius and hi1[i] == sim[1].d1[i]       # B2 from the widened radius, rounded up, ...
            assert radius < sim[1].d1[i]                             # ... to its nearest distance
        else:
            assert lo1[i] == hi1[i] == sim[1].d1[i]                  # B2: its own nearest distance
        assert sim[2].sure_pass[i] == (k >= 0.04) and sim[2].sure_search[i] == (k < 0.04), (i, k)
        assert sim[3].sure_search[i] and float(sim[3].d1[i]) < bound ** 2
        assert float(sim[4].d1[i]) >= bound ** 2


def test_near_ties():
    case, sim = WC.cached("near_ties")
    common(case, sim)
    assert case.expect["purpose"] == tuple(range(len(case.source)))     # every query: results, not status
    ulps = [int(sim[0].d2[i].view(np.int32)) - int(sim[0].d1[i].view(np.int32)) for i in range(3)]
    assert sorted(ulps) == [1, 2, 3], ulps
    switched = np.zeros(len(case.source), bool)
    for s in range(1, len(sim)):
        m = moved(case, s)
        assert (m > 0.5e-5).all() and (m < 1.5e-5).all()
        switched |= sim[s].j1 != sim[s - 1].j1
        # the only candidates are the pair's two points: the nearest is one of them
        assert (sim[s].j1 < 20).all()
    assert switched.sum() >= 10, "queries cross their bisector"
    for o in WC.NEAR_OFFSETS:   # the offsets are there on both sides
        assert o >= 1e-6 and o <= 1e-3


@pytest.mark.parametrize("variant", ["first", "late"])
def test_ties(variant):
    case, sim = WC.cached("ties", variant)
    common(case._replace(expect=dict(case.expect, tie_free=False)), sim)
    for s, n in enumerate(case.expect["tied"]):
        assert (sim[s].cnt == n).all(), (s, np.unique(sim[s].cnt))
        q = NP.transform_f32(case.script[s][0], case.source).astype(np.float64)
        exact = case.source.astype(np.float64) + case.script[s][0][:3, 3]
        assert np.array_equal(q, exact), "the fp32 query is exact"
        if n > 1:   # a tie forces B2 <= d1: never proven
            lo, hi = WC.b2_bounds(sim[s].d1, sim[s].d2, WC.cap2_of(case.bound), WC.REUSE_GAP)
            assert (hi == sim[s].d1).all()
            assert not sim[s].sure_pass.any(), "a tied query is never proven"
    s8 = case.expect["tied"].index(8)
    assert (sim[s8].d1 == F32(0.75)).all()
    if variant == "late":   # the references of step 0 are live when the tie is first met
        assert case.script[0][1] == 1 and case.script[1][1] == 0 and sim[0].has_ref.all() and s8 == 1


@pytest.mark.parametrize("nt", WC.SIZES_TGT)
def test_sizes(nt):
    case, sim = WC.cached("sizes", nt)
    common(case, sim)
    assert len(case.target) == nt and len(case.source) == max(WC.SIZES_SRC)
    assert [r for _, r in case.script] == [0, 1, 0]
    assert abs(moved(case, 1).mean() - 0.02) < 1e-3 and abs(moved(case, 2).mean() - 0.005) < 1e-3
    assert WC.SIZES_TGT == (1, 31, 32, 33, 2047, 2049) and WC.LEAF * WC.FANOUT == 2048


def test_second_run():
    first, _ = WC.cached("steps", "all")
    case, sim = WC.cached("second_run")
    common(case, sim)
    assert case.target.shape == first.target.shape and case.source.shape == first.source.shape
    assert not np.array_equal(case.target, first.target) and not np.array_equal(case.source, first.source)
    assert [r for _, r in case.script[:2]] == [0, 0] and case.script[2][1] == 1
    assert not sim[0].sure_pass.any() and not sim[1].sure_pass.any() and not sim[2].sure_pass.any()


@pytest.mark.parametrize("kind", sorted(WC.SHARDS))
def test_shards(kind):
    case, sim = WC.cached("shards", kind)
    common(case, sim)
    own = np.array([st.owned for st in sim])
    assert own.any() and (~own).any()
    gained = (~own[:-1] & own[1:]).any(0)
    lost = (own[:-1] & ~own[1:]).any(0)
    few = 3 if kind == "slab" else 1
    assert gained.sum() >= few and lost.sum() >= few, "queries cross SHARD_LO in both directions"
    recs = [r for _, r in case.script]
    first = recs.index(1)
    assert first >= 1 and (~own[first]).any()
    late = ~own[first] & own[first + 1:].any(0)     # first owned after the first recording step
    assert late.sum() >= few
    for i in np.flatnonzero(late):
        for s in range(first, len(sim)):
            searched_rec = any(recs[k] and own[k, i] for k in range(first, s + 1))
            assert sim[s].has_ref[i] == searched_rec, (i, s)
    # the interleaved groups: a third of the sub-groups
    assert 0.2 < WC.owned_mask(case.source, sim[0].q, (0, -np.inf, np.inf, 3, 1)).mean() < 0.5


def test_cells():
    case, sim = WC.cached("cells")
    common(case, sim)
    assert case.bound == 5.0 and [r for _, r in case.script] == [0, 1, 0, 1]


@pytest.mark.parametrize("which", sorted(WC.ALIGN_PARAMS))
def test_align_records_naturally(which):
    """The oracle's truncated aligns of the two align problems: some iteration's step has the
    restated mv bound below reuse_rec_eps and is_converged's measure above reuse_rec_conv (each
    with 5 % to spare), and at least two iterations follow it: the one that records and one
    that can pass."""
    tgt, src, G, bound, g = WC.align_problem(which)
    kw = WC.ALIGN_PARAMS[which]
    poses, iters = [G], []
    for m in range(1, WC.ALIGN_M + 1):
        o = O.Gicp(src, tgt, O.default_params(max_iterations=m, **kw))
        if g is not None:
            o.set_covariances(0, g["cov_src_PLANE"])
            o.set_covariances(1, g["cov_tgt"])
        pose, res = o.align(G.astype(F32))
        poses.append(pose.astype(np.float64))
        iters.append(res.iterations_run)
    radius = float(np.linalg.norm(src.astype(np.float64), axis=1).max())
    p = O.default_params(**kw)
    rec = WC.natural_recording(poses, radius, p.transformation_epsilon, p.rotation_epsilon)
    total = iters[-1]
    print(which, "iterations", iters, "recording iterations", rec)
    assert total < WC.ALIGN_M, "the last runs converge on their own"
    assert any(k + 1 <= total - 1 for k in rec), (rec, iters)   # iteration k records, k + 1 can pass
