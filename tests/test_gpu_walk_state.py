"""The walk search across outer iterations (k_nn_seed -> k_nn_scan, the reference recording
of k_moments<*, false>): seeds carried over and verified reuse, driven pose by pose through
gicp_debug_search_begin / _step / _state on the scripts of tests/walk_cases.py (their
properties are proven in tests/test_walk_cases_cpu.py).

After every step of every script:
  - the same answer as a stateless search, bit for bit: correspondences, distances of the
    matched queries, H, b, cost and count of linearize(pose) on a fresh context (same
    kernels, have_prev = 0): state may change how a query is answered, never the answer;
  - the oracle's linearize: correspondences and distances assert_array_equal, ties included,
    H, b and cost at the project's relative 1e-11;
  - the numpy brute force on the tie-free queries: index and distance of the fp32 minimum,
    matched iff float64(d2) < bound^2;
  - every exported reference is a true statement: p1 is a brute-force nearest point of q_ref
    (or none, with nothing within the bound), min(d2, widened(d1)) <= B2 <= d2 against the
    brute force (walk_cases.b2_bounds), q_ref is bit for bit the query of the step that
    recorded it, a query not searched in a recording step keeps its reference bit for bit,
    and before the first recording step any_rec is 0, whatever an earlier run left in ref;
  - status: for every query the restated rule decides from the device's own reference, it is
    unsearched (a negative walk radius; sec == 0xffffffff wherever the tie test runs) iff the
    rule passes; at the steps built to show passes at least the CPU test's sure passes.  With
    the cells in front of the walk only the searched queries are held to it.  The per-step
    counts are printed.
A tie error raises in search_step.  Truncated real aligns show the same of iterations whose
recording k_lm_step chose itself.
"""
import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
import np_gicp as NP
import walk_cases as WC
from dynamic_direct_lidar_odometry_amd import SOURCE, TARGET
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ALL = np.uint32(0xFFFFFFFF)
F32 = np.float32


def spd(n, rng):
    """Random SPD covariances (test_gpu_grid_cases.spd)."""
    A = rng.normal(0, 0.05, (n, 3, 3))
    return np.ascontiguousarray(NP.mat_to_sym6(A @ np.transpose(A, (0, 2, 1)) + 1e-3 * np.eye(3)))


def covs(case):
    rng = np.random.default_rng(1)
    return spd(len(case.target), rng), spd(len(case.source), rng)


def params(case, **kw):
    return dict(k_correspondences=10, max_correspondence_distance=case.bound, **kw)


def make(case, tcov, scov, nsrc=None, grid=P.GRID_OFF, shard=None):
    c = P.Context(0)
    c.set_params(P.default_params(**params(case)))
    c.set_target_grid(grid)
    load(c, case, tcov, scov, nsrc)
    if shard is not None:
        c.set_shard(shard[0], shard[1], shard[2])
        if shard[3]:
            c.set_shard_groups(shard[3], shard[4])
    return c


def load(c, case, tcov, scov, nsrc=None):
    m = len(case.source) if nsrc is None else nsrc
    c.set_target(case.target)
    c.set_covariances(TARGET, tcov)
    c.set_source(np.ascontiguousarray(case.source[:m]))
    c.set_covariances(SOURCE, np.ascontiguousarray(scov[:m]))


def oracle(case, tcov, scov, nsrc=None):
    m = len(case.source) if nsrc is None else nsrc
    o = O.Gicp(np.ascontiguousarray(case.source[:m]), case.target, O.default_params(**params(case)))
    o.set_covariances(0, np.ascontiguousarray(scov[:m]))
    o.set_covariances(1, tcov)
    return o


def close_rel(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-11 * max(np.abs(b).max(), 1e-300), err_msg=what)


def check_results(case, s, st_sim, m, got, state, fresh, orc, own):
    """Step s's answers against the fresh context, the oracle and the brute force."""
    H, b, cost, n = got
    pose = case.script[s][0]
    tag = f"{case.name} step {s}"
    corr, sqd = state["corr"], state["sqd"]
    matched = corr >= 0
    # a stateless search on a fresh context, bit for bit
    Hf, bf, costf, nf = fresh.linearize(pose)
    fcorr, fsqd = fresh.correspondences()
    np.testing.assert_array_equal(corr, fcorr, err_msg=tag)
    np.testing.assert_array_equal(sqd[matched], fsqd[matched], err_msg=tag)
    np.testing.assert_array_equal(H, Hf, err_msg=tag)
    np.testing.assert_array_equal(b, bf, err_msg=tag)
    assert cost == costf and n == nf, tag
    # the oracle (every query; the queries another shard owns have no match here)
    Ho, bo, co, ocorr, osqd = orc.linearize(pose)
    np.testing.assert_array_equal(corr, np.where(own, ocorr, -1), err_msg=tag)
    np.testing.assert_array_equal(sqd[matched], osqd[matched], err_msg=tag)
    if own.all():
        close_rel(H, Ho, tag + " H")
        close_rel(b, bo, tag + " b")
        assert abs(cost - co) <= 1e-11 * abs(co), tag
    assert n == int(matched.sum()), tag
    # the brute force
    d1, j1, cnt = st_sim.d1[:m], st_sim.j1[:m], st_sim.cnt[:m]
    want = own & (d1.astype(np.float64) < case.bound ** 2)
    np.testing.assert_array_equal(matched, want, err_msg=tag)
    free = cnt == 1
    np.testing.assert_array_equal(corr[free], np.where(want, j1, -1)[free], err_msg=tag)
    np.testing.assert_array_equal(sqd[matched], d1[matched], err_msg=tag)
    found = np.isfinite(sqd)
    np.testing.assert_array_equal(sqd[found], d1[found], err_msg=tag)      # whatever was found is the minimum
    q = st_sim.q[:m]
    np.testing.assert_array_equal(NP.nanoflann_sqd(q[matched], case.target[corr[matched]]), d1[matched], err_msg=tag)


def eff_b2(state):
    """B2 as the search reads it: the raw word only when the state's any_rec is set (check_ref)."""
    return state["ref"][:, 3] if state["any_rec"] else np.full(len(state["ref"]), -1.0, F32)


def check_refs(case, sim, s, m, state, prev, ref_step, searched, recs):
    """The exported references after step s are true statements (prev: the export before it).
    The export is raw: what an earlier run left lies in ref until a recording step of this one
    rewrites or clears it, and any_rec says whether the search reads it."""
    tag = f"{case.name} step {s}"
    cap2 = WC.cap2_of(case.bound)
    ref, refp, refj = state["ref"], state["ref_p"], state["ref_j"]
    assert state["any_rec"] == int(any(recs[:s + 1])), tag + ": any_rec"
    if not any(recs[:s + 1]):
        return   # no recording step yet: any_rec = 0 keeps the search from whatever the buffers hold
    has = ref[:, 3] >= 0
    first = not any(recs[:s])
    if recs[s]:
        ref_step[searched] = s
        if first:
            ref_step[~searched] = -1
    keep = ~searched if recs[s] else np.ones(m, bool)
    if prev is not None and not (recs[s] and first):   # not searched in a recording step: kept bit for bit
        for k in ("ref", "ref_p", "ref_j"):
            np.testing.assert_array_equal(state[k][keep].view(np.uint32), prev[k][keep].view(np.uint32), err_msg=f"{tag} {k} kept")
    np.testing.assert_array_equal(has, ref_step >= 0, err_msg=tag + ": who holds a reference")
    for r in np.unique(ref_step[has]):
        i = np.flatnonzero(has & (ref_step == r))
        R = sim[r]
        np.testing.assert_array_equal(ref[i, :3].view(np.uint32), R.q[i].view(np.uint32), err_msg=f"{tag}: q_ref of step {r}")
        d1, d2 = R.d1[i], R.d2[i]
        none = refj[i] < 0
        assert (d1[none] >= cap2).all(), tag + ": no match recorded with a point within the bound"
        j = refj[i][~none]
        assert (j < len(case.target)).all()
        np.testing.assert_array_equal(refp[i][~none].view(np.uint32), case.target[j].view(np.uint32), err_msg=tag + ": p1")
        np.testing.assert_array_equal(NP.nanoflann_sqd(R.q[i][~none], case.target[j]), d1[~none],
                                      err_msg=tag + ": p1 is not a nearest point of q_ref")
        assert (d1[~none] <= cap2).all(), tag
        lo, hi = WC.b2_bounds(d1, d2, cap2, WC.REUSE_GAP if r >= 1 else WC.REUSE_GAP0, none=none)
        B2 = ref[i, 3]
        bad = np.flatnonzero(~((lo <= B2) & (B2 <= hi)))
        assert bad.size == 0, f"{tag}: B2 outside its bounds at step {r}'s references: rows {i[bad][:8]}, " \
                              f"lo {lo[bad][:8]} B2 {B2[bad][:8]} hi {hi[bad][:8]}"
        tied = R.cnt[i] > 1
        assert (B2[tied & ~none] <= d1[tied & ~none]).all(), tag + ": a tied query's B2 above d1"


def check_status(case, sim, s, m, state, prev, own, recs, purpose, mode="sec"):
    """A query is unsearched iff the restated rule, fed the reference the step consumed (the export
    before it, read as the search reads it), passes.  Unsearched is a negative walk radius, which
    k_nn_seed stores for every query in both of its branches; mode "sec": sec == all ones says the
    same (the tie test is on, so sec is written at every step); "wr": a shard without a tie tree
    runs no tie test; "lookup": the cells answered most queries in front of the walk (they are
    unsearched whatever the rule says), so only a searched query is held to the rule: it did not pass.
    Returns (passed, searched, undecided) counts over the owned queries."""
    tag = f"{case.name} step {s}"
    cap2 = WC.cap2_of(case.bound)
    unsearched = state["wr"] < 0
    if mode == "sec":
        np.testing.assert_array_equal(state["sec"] == ALL, unsearched, err_msg=tag + ": sec and the walk radius disagree")
    assert unsearched[~own].all(), tag + ": a query of another shard was searched"
    if prev is None or not prev["any_rec"]:
        assert s == 0 or not any(recs[:s]), tag
        if mode != "lookup":
            assert not unsearched[own].any(), tag + ": a pass without a reference"
        return 0, int((own & ~unsearched).sum()), 0
    q = sim[s].q[:m]
    B2 = eff_b2(prev)
    passes, dec = WC.decided(q, prev["ref"][:, :3], B2, prev["ref_p"], prev["ref_j"] >= 0, cap2)
    ok = own & dec
    bad = np.flatnonzero(ok & (~unsearched & passes if mode == "lookup" else unsearched != passes))
    assert bad.size == 0, f"{tag}: status differs from the rule at rows {bad[:8]}: passes {passes[bad][:8]}"
    if mode == "lookup":
        return int((passes & ok).sum()), int((own & ~unsearched).sum()), int((own & ~dec).sum())
    assert not unsearched[own & ~(B2 >= 0)].any(), tag
    want = sim[s].sure_pass[:m] & ~purpose
    assert unsearched[want].all(), f"{tag}: a sure pass was searched (rows {np.flatnonzero(want & ~unsearched)[:8]})"
    return int((unsearched & own).sum()), int((~unsearched & own).sum()), int((own & ~dec).sum())


def run_script(case, sim, ctx, fresh, orc, m=None, mode="sec", hook=None):
    """Drive ctx through the script with every check; returns the per-step (passed, searched,
    undecided) counts and every step's exported state.  hook(s, got, state): the caller's own checks."""
    m = len(case.source) if m is None else m
    recs = [r for _, r in case.script]
    purpose = np.zeros(m, bool)
    purpose[[i for i in case.expect["purpose"] if i < m]] = True
    ref_step = np.full(m, -1)
    prev, counts, states = None, [], []
    ctx.search_begin()
    for s, (pose, rec) in enumerate(case.script):
        got = ctx.search_step(pose, rec)
        state = ctx.search_state()
        own = sim[s].owned[:m]
        check_results(case, s, sim[s], m, got, state, fresh, orc, own)
        check_refs(case, sim, s, m, state, prev, ref_step, state["wr"] >= 0, recs)
        counts.append(check_status(case, sim, s, m, state, prev, own, recs, purpose, mode))
        print(f"{case.name} step {s} rec {rec}: passed {counts[-1][0]} searched {counts[-1][1]} undecided {counts[-1][2]}"
              f" (sure passes {int(sim[s].sure_pass[:m].sum())})")
        if hook is not None:
            hook(s, got, state)
        states.append(state)
        prev = state
    for s in case.expect["pass_steps"]:
        assert counts[s][0] >= int((sim[s].sure_pass[:m] & ~purpose).sum()) > 0, (case.name, s, counts[s])
    return counts, states


def run_case(name, *args, **kw):
    case, sim = WC.cached(name, *args)
    tcov, scov = covs(case)
    ctx, fresh, orc = make(case, tcov, scov), make(case, tcov, scov), oracle(case, tcov, scov)
    try:
        return run_script(case, sim, ctx, fresh, orc, **kw)
    finally:
        ctx.close()
        fresh.close()


@pytest.mark.parametrize("variant", sorted(WC.STEPS_RECS))
def test_steps(variant):
    """Case 1: the scripted steps, recording where production would, also at step 0, and at every step."""
    counts, _ = run_case("steps", variant)
    if variant == "natural":
        assert counts[2][0] > 500 and counts[8][0] == 1000 and counts[4][0] < 100


@pytest.mark.parametrize("bound", [0.5, 1.0])
def test_bound(bound):
    """Case 2: queries beyond the bound are proven unmatched from the widened radius; d2 at the bound's ulps."""
    counts, states = run_case("bound_case", bound)
    assert counts[2][0] >= 24   # (the three queries at the bound's ulps pass too, at step 3 as well: their match is 6 m from every other point)
    case, sim = WC.cached("bound_case", bound)
    cap2 = WC.cap2_of(bound)
    radius = WC.widened(cap2, WC.REUSE_GAP)
    for i, k in enumerate(case.expect["kinds"]):
        if isinstance(k, str):
            continue
        # step 0 (iteration 0, gap0 = 0): nothing within the bound, nothing examined inside it: B2 is cap2 itself
        assert states[0]["ref"][i, 3] == cap2 and states[0]["ref_j"][i] == -1, (i, k)
        # step 1 records again: the widened radius, rounded up, exactly -- or the nearest distance inside it
        want = radius if k >= 0.06 else sim[1].d1[i]
        assert states[1]["ref"][i, 3] == want and states[1]["ref_j"][i] == -1, (i, k, states[1]["ref"][i, 3], want)
        assert (want == radius) == (sim[1].d1[i] >= radius)


def test_near_ties():
    """Case 3: no reference keeps the old match once the other point of the pair is nearer."""
    run_case("near_ties")


@pytest.mark.parametrize("variant", ["first", "late"])
def test_ties(knn_golden, variant):
    """Case 4: tied 8-way, unique, tied 4-way, unique, recording throughout: nanoflann's order at every
    step, a tied query is never unsearched and its B2 never above d1.  The step that first meets a tie builds the
    tie tree and runs again on the same state ("late": the references of the step before it survive it); a later
    align finds the tree (tie_reruns 0), a fresh context's does not."""
    case, sim = WC.cached("ties", variant)
    np.testing.assert_array_equal(case.target, knn_golden["lat_pts"])
    tcov, scov = covs(case)
    ctx, fresh, orc = make(case, tcov, scov), make(case, tcov, scov), oracle(case, tcov, scov)
    other = make(case, tcov, scov)

    def tied_are_searched(s, got, state):
        tied = sim[s].cnt > 1
        assert tied.all() == (case.expect["tied"][s] > 1)
        assert not (state["sec"][tied] == ALL).any() and (state["wr"][tied] >= 0).all(), "a tied query was not searched"

    try:
        counts, _ = run_script(case, sim, ctx, fresh, orc, hook=tied_are_searched)
        for s, n in enumerate(case.expect["tied"]):
            assert (counts[s][0] == 0) or n == 1, (s, counts[s])
        _, res = ctx.align()
        _, res2 = other.align()
        assert res.tie_reruns == 0 and res2.tie_reruns == 1 and res.ties_resolved > 0
        assert (res.iterations_run, res.lm_trials) == (res2.iterations_run, res2.lm_trials)
    finally:
        for c in (ctx, fresh, other):
            c.close()


def test_far_origin():
    """Case 5: case 1 at fp32 coordinates of 4-8 km."""
    run_case("far_origin")


@pytest.mark.parametrize("nt", WC.SIZES_TGT)
def test_sizes(nt):
    """Case 6: source lengths about the 16- and 64-query groups against targets shorter than the Morton
    window, of one box level and of two."""
    case, sim = WC.cached("sizes", nt)
    tcov, scov = covs(case)
    for m in WC.SIZES_SRC:
        ctx, fresh, orc = make(case, tcov, scov, m), make(case, tcov, scov, m), oracle(case, tcov, scov, m)
        try:
            run_script(case, sim, ctx, fresh, orc, m=m)
        finally:
            ctx.close()
            fresh.close()


def test_two_aligns_on_one_context():
    """Case 7: after a script that recorded at every step, other clouds of the same sizes on the same
    context: the second script's first steps do not record, and nothing of the first run's references is used."""
    first, sim1 = WC.cached("steps", "all")
    case, sim = WC.cached("second_run")
    tcov1, scov1 = covs(first)
    rng = np.random.default_rng(2)
    tcov, scov = spd(len(case.target), rng), spd(len(case.source), rng)
    ctx, fresh, orc = make(first, tcov1, scov1), make(case, tcov, scov), oracle(case, tcov, scov)
    try:
        ctx.search_begin()
        for pose, rec in first.script[:5]:
            ctx.search_step(pose, rec)
        assert (ctx.search_state()["ref"][:, 3] >= 0).all()
        load(ctx, case, tcov, scov)
        counts, states = run_script(case, sim, ctx, fresh, orc)
        assert counts[0][0] == counts[1][0] == counts[2][0] == 0 and counts[3][0] > 500
        for st in states[:2]:   # the first run's references still lie in the buffers; any_rec = 0 keeps the search from them
            assert st["any_rec"] == 0 and (st["ref"][:, 3] >= 0).all()
    finally:
        ctx.close()
        fresh.close()


@pytest.mark.parametrize("kind", sorted(WC.SHARDS))
def test_shards(kind):
    """Case 8: under a slab through the cloud (and a third of the 16-query groups) the owned queries equal
    the unsharded oracle's at every step and the others are -1; a query first owned after the first recording
    step has no reference until a recording step searches it.  The context ran an unsharded script before, so
    stale references lie in its buffers.  A shard without a tie tree runs no tie test, so sec is not written at
    every step: unsearched is read from the walk radius, and held to the rule as everywhere."""
    first, _ = WC.cached("steps", "all")
    case, sim = WC.cached("shards", kind)
    shard = case.expect["shard"]
    tcov, scov = covs(case)
    ctx, fresh, orc = make(case, tcov, scov), make(case, tcov, scov, shard=shard), oracle(case, tcov, scov)
    try:
        ctx.search_begin()
        for pose, rec in first.script[:3]:
            ctx.search_step(pose, rec)
        assert (ctx.search_state()["ref"][:, 3] >= 0).all()
        ctx.set_shard(shard[0], shard[1], shard[2])
        if shard[3]:
            ctx.set_shard_groups(shard[3], shard[4])
        with pytest.raises(P.GicpError):   # the shard changed the job: the old sequence is over
            ctx.search_step(case.script[0][0], 0)
        _, states = run_script(case, sim, ctx, fresh, orc, mode="wr")
        assert states[0]["any_rec"] == 0 and (states[0]["ref"][:, 3] >= 0).all()   # stale, and not read
        m = len(case.source)
        recs = [r for _, r in case.script]
        own = np.array([st.owned for st in sim])
        want = np.array([any(recs[k] and own[k, i] for k in range(len(recs))) for i in range(m)])
        np.testing.assert_array_equal(states[-1]["ref"][:, 3] >= 0, want)
    finally:
        ctx.close()
        fresh.close()


def test_cells_in_front_of_the_walk():
    """Case 9: with the candidate cells on, k_cell_lookup hands the walk only the listed sub-groups'
    unanswered queries: cells on and off bit for bit in correspondences, distances, H, b, cost and count,
    the walk's references true statements in both.  The cells-off context gets every check of the other
    scripts, pass counts included; on the cells-on one every query the walk searched is one the rule does not pass."""
    case, sim = WC.cached("cells")
    tcov, scov = covs(case)
    cg, cw = make(case, tcov, scov, grid=P.GRID_ON), make(case, tcov, scov)
    fresh, orc = make(case, tcov, scov), oracle(case, tcov, scov)
    m = len(case.source)
    recs = [r for _, r in case.script]
    purpose = np.zeros(m, bool)
    steps_g, prev_g, walked = np.full(m, -1), [None], []

    def cells_on(s, gw, sw):
        gg = cg.search_step(*case.script[s])
        sg = cg.search_state()
        np.testing.assert_array_equal(sg["corr"], sw["corr"])
        np.testing.assert_array_equal(sg["sqd"], sw["sqd"])
        np.testing.assert_array_equal(gg[0], gw[0])
        np.testing.assert_array_equal(gg[1], gw[1])
        assert gg[2] == gw[2] and gg[3] == gw[3]
        check_refs(case, sim, s, m, sg, prev_g[0], steps_g, sg["wr"] >= 0, recs)
        c = check_status(case, sim, s, m, sg, prev_g[0], sim[s].owned, recs, purpose, mode="lookup")
        print(f"cells on, step {s}: the walk searched {c[1]} queries, the rule passes {c[0]}")
        walked.append(c[1])
        prev_g[0] = sg

    try:
        cg.search_begin()
        counts, _ = run_script(case, sim, cw, fresh, orc, hook=cells_on)
        assert counts[2][0] > 0 and counts[3][0] > 0
        info = cg.grid_info()
        assert info["built"] == 1 and info["uses_walk"] == 1 and cg.lookup_walk_groups() > 0
        assert walked[0] > 0 and walked[1] > 0 and max(walked) < m, walked   # (before any reference: every listed query)
    finally:
        for c in (cg, cw, fresh):
            c.close()


@pytest.mark.parametrize("which", sorted(WC.ALIGN_PARAMS))
def test_truncated_aligns(which, s2s_golden):
    """Real aligns, recording where k_lm_step chooses to: align(G) with max_iterations = m leaves the
    correspondences and distances of the oracle's linearize and of the brute force at the float32 pose the
    m - 1 run returned; iterations and LM trials of consecutive runs are consistent; at some m matched
    queries were answered by their references (sec all ones)."""
    tgt, src, G, bound, g = WC.align_problem(which)
    kw = WC.ALIGN_PARAMS[which]
    orc = O.Gicp(src, tgt, O.default_params(**kw))
    if g is None:   # the covariances the CPU test's aligns computed (the oracle's own, k = 10, PLANE)
        orc.compute_covariances(0)
        orc.compute_covariances(1)
        scov, tcov = orc.get_covariances(0), orc.get_covariances(1)
    else:
        tcov, scov = g["cov_tgt"], g["cov_src_PLANE"]
        orc.set_covariances(0, scov)
        orc.set_covariances(1, tcov)
    ctx = P.Context(0)
    ctx.set_target(tgt)
    ctx.set_covariances(TARGET, tcov)
    ctx.set_source(src)
    ctx.set_covariances(SOURCE, scov)
    poses, runs, passes = [G], [], []
    try:
        for m in range(1, WC.ALIGN_M + 1):
            ctx.set_params(P.default_params(max_iterations=m, **kw))
            pose, res = ctx.align(G.astype(F32))
            it = res.iterations_run
            assert 1 <= it <= m and not res.lm_failed
            if runs:
                pit, ptr, ppose = runs[-1]
                assert it >= pit and res.lm_trials >= ptr
                if it == pit:   # converged before m: the same align
                    assert res.lm_trials == ptr
                    np.testing.assert_array_equal(pose, ppose)
                else:
                    assert it == m and pit == m - 1
            runs.append((it, res.lm_trials, pose))
            if it == m:
                poses.append(pose.astype(np.float64))
            at = poses[it - 1]   # the last search ran at the pose the it - 1 run returned
            st = ctx.search_state()
            _, _, _, ocorr, osqd = orc.linearize(at)
            matched = st["corr"] >= 0
            np.testing.assert_array_equal(st["corr"], ocorr, err_msg=f"{which} m {m}")
            np.testing.assert_array_equal(st["sqd"][matched], osqd[matched], err_msg=f"{which} m {m}")
            d1, j1, _, cnt = WC.brute2(tgt, NP.transform_f32(at, src))
            want = d1.astype(np.float64) < bound ** 2
            np.testing.assert_array_equal(matched, want)
            np.testing.assert_array_equal(st["corr"][cnt == 1], np.where(want, j1, -1)[cnt == 1])
            np.testing.assert_array_equal(st["sqd"][matched], d1[matched])
            passes.append(int((st["sec"][matched] == ALL).sum()))
        print(which, "iterations", [r[0] for r in runs], "matched queries answered by their reference", passes)
        assert passes[0] == 0 and max(passes) > 0
    finally:
        ctx.close()
