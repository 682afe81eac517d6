"""Scripted pose sequences for the walk search's state machine (k_nn_seed -> k_nn_scan and
the reference recording of k_moments<*, false>; tests/test_walk_cases_cpu.py proves the
generators, tests/test_gpu_walk_state.py runs them): numpy only, deterministic.

From the second outer iteration on a query is answered by verified reuse (a recorded
reference proves the old match, no search), from a seed carried over (the triangle bound
below tri_mv, else the previous match's distance and the Morton window), or from the
stateless seeds.  Whichever it is, the answer must be the one a fresh search gives.

Every generator returns a ``WalkCase``: target f32[N,3], source f32[M,3], the bound and a
script, a list of (pose, rec) steps: float64 4x4 poses that are exact float32 values (what
the search's fp32 transform uses) and the 0/1 recording flag k_lm_step would have chosen.
``simulate`` restates what is true at every step without the device: the fp32 queries
(np_gicp.transform_f32), the brute-force nearest and second distances, and which queries
must pass their reference, must be searched, or are undecided.

Restated from the product, with the source lines they come from:

  search_knobs(), dynamic_direct_lidar_odometry_amd/csrc/align.hip:
    reuse_gap 0.05, reuse_gap0 0, tri_mv 0.2, reuse_rec_eps 0.05, reuse_rec_conv 10
  "Verified reuse", csrc/corr_search.hip (k_nn_seed), in float64 from the fp32 values,
  d2(.,.) the fp32 squared distance of np_gicp.nanoflann_sqd:
    eps = |q - q_ref| (1 + 1e-9) + 1e-12
    b   = sqrt(B2 / (1 + 1e-6))
    lb2 = (b - eps)^2 (1 - 1e-6) if b > eps else -1
    with a match p1: pass iff d2(q, p1) < lb2;  with none: pass iff lb2 > cap2,
    cap2 = nextafter(float32(bound^2), +inf)   (search_cap2, align.hip)
  the walk radius of a recording search, csrc/corr_search.hip ("walk radius"):
    nextup(float32((sqrt(seed bound) + gap)^2)), gap = reuse_gap with a previous
    iteration, reuse_gap0 without (0: not widened)
  the recorded bound, csrc/moments.hip ("reuse reference"): B2 = min(sec, walk radius)
  the recording rule of k_lm_step, csrc/lm_step.hpp: mv = |dR - I|_F (src_radius + |t|) + |dt|
    below reuse_rec_eps and is_converged's measure above reuse_rec_conv.

Two bounds on a recorded B2 that do not depend on the implementation.  d1 <= d2 are the
two smallest fp32 squared distances from q_ref over the whole target (d2 over every point
other than the match); with nothing within the bound d1 is cap2 and d2 the smallest
distance overall:

    min(d2, widened(d1)) <= B2 <= d2

The upper bound is the soundness of the proof (every point other than p1 is at B2 or
more).  The lower one holds because the seed bound is never below d1 and every point
inside the walk radius is examined.  An exact tie (d2 == d1) forces B2 <= d1: a tied
query can never be proven.
"""
import functools
import math
import os
from typing import NamedTuple

import numpy as np

import grid_cases as GC
import np_gicp as NP

F32 = np.float32
F64 = np.float64

REUSE_GAP = 0.05        # search_knobs: reuse_gap
REUSE_GAP0 = 0.0        # reuse_gap0
TRI_MV = 0.2            # tri_mv
REUSE_REC_EPS = 0.05    # reuse_rec_eps
REUSE_REC_CONV = 10.0   # reuse_rec_conv
LEAF = 32               # kLeafSize
FANOUT = 64             # kFanout: more than LEAF * FANOUT = 2048 points make two box levels
MARGIN = 1e-9           # decided(): relative margin on lb2

SIZES_SRC = GC.SIZES                       # 1, 15, 16, 17, 63, 64, 65, 255, 257
SIZES_TGT = (1, 31, 32, 33, 2047, 2049)
BOUND_DELTAS = (0.02, 0.04, 0.06, 0.2)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class WalkCase(NamedTuple):
    name: str
    target: np.ndarray
    source: np.ndarray
    bound: float
    script: list        # [(pose float64[4,4], rec 0/1)]
    expect: dict        # tie_free, pass_steps, purpose (source rows undecided on purpose), ...


def cap2_of(bound):
    return np.nextafter(F32(float(bound) * float(bound)), F32(np.inf))


def nextup(x):
    return np.nextafter(np.asarray(x, F32), F32(np.inf))


def f32_pose(T):
    """The pose as exact float32 values in float64 (the search casts st->R, st->t to float)."""
    return np.asarray(T, F64).astype(F32).astype(F64)


def translation(v):
    T = np.eye(4)
    T[:3, 3] = v
    return T


def yaw_about(angle, centre):
    c, s = math.cos(angle), math.sin(angle)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.asarray(centre, F64) - R @ np.asarray(centre, F64)
    return T


# ---------------------------------------------------------------------------
# brute force and the restated rule
def brute2(target, q, chunk=256):
    """Per query: (d1, j1, d2, count): the fp32 minimum squared distance, its lowest index, the
    smallest distance over every other point (== d1 at a tie; +inf for a single-point target)
    and the number of bit-equal minima.  An M x N float32 matrix in chunks."""
    t = np.asarray(target, F32)
    q = np.asarray(q, F32)
    m = len(q)
    d1, j1, d2, cnt = np.empty(m, F32), np.empty(m, np.int64), np.empty(m, F32), np.empty(m, np.int64)
    for a in range(0, m, chunk):
        d = NP.nanoflann_sqd(q[a:a + chunk, None, :], t[None, :, :])
        r = np.arange(len(d))
        j = d.argmin(1)
        lo = d[r, j]
        cnt[a:a + chunk] = (d == lo[:, None]).sum(1)
        d[r, j] = np.inf
        d1[a:a + chunk], j1[a:a + chunk], d2[a:a + chunk] = lo, j, d.min(1)
    return d1, j1, d2, cnt


def widened(d1, gap):
    """The walk radius of a recording search whose seed bound is d1 (its smallest possible)."""
    d1 = np.asarray(d1, F32)
    if gap <= 0.0:
        return d1
    r = np.sqrt(d1.astype(F64)) + gap
    return nextup((r * r).astype(F32))


def b2_bounds(d1, d2, cap2, gap, tight=False, none=None):
    """(lower, upper) of the B2 a search at q_ref records, from the brute force's d1, d2
    (brute2): with nothing within the bound (d1 >= cap2) d1 is cap2 and d2 the minimum.
    tight (simulate only, never asserted of the device): with nothing within the bound the
    seed bound is the search's own cap2 and nothing else, and B2 = min(sec, walk radius)
    never exceeds the radius, so the upper end is the lower one.  none: which references hold
    no match (the device's own word; at d1 == cap2 exactly either is a true statement)."""
    d1 = np.asarray(d1, F32)
    none = d1 >= cap2 if none is None else np.asarray(none, bool)
    e1 = np.where(none, cap2, d1).astype(F32)
    e2 = np.where(none, d1, np.asarray(d2, F32)).astype(F32)
    lo = np.minimum(e2, widened(e1, gap)).astype(F32)
    return lo, (np.where(none, lo, e2).astype(F32) if tight else e2)


def lb2_of(q, qref, B2):
    ex = q[:, 0].astype(F64) - qref[:, 0].astype(F64)
    ey = q[:, 1].astype(F64) - qref[:, 1].astype(F64)
    ez = q[:, 2].astype(F64) - qref[:, 2].astype(F64)
    eps = np.sqrt(ex * ex + ey * ey + ez * ez) * (1.0 + 1e-9) + 1e-12
    with np.errstate(invalid="ignore"):
        b = np.sqrt(np.asarray(B2, F32).astype(F64) / (1.0 + 1e-6))
    b = np.where(np.isnan(b), -1.0, b)
    return np.where(b > eps, (b - eps) * (b - eps) * (1.0 - 1e-6), -1.0)


def pass_rule(q, qref, B2, p1, has_p1, cap2, margin=0.0):
    """The pass rule of k_nn_seed for fp32 queries q against references (qref, B2, p1):
    lb2 is scaled by (1 + margin).  A reference with B2 < 0 never passes."""
    q, qref, p1 = np.asarray(q, F32), np.asarray(qref, F32), np.asarray(p1, F32)
    lb2 = lb2_of(q, qref, B2) * (1.0 + margin)
    with np.errstate(all="ignore"):   # (a cleared reference keeps whatever p1 lay there: B2 < 0 masks it below)
        dn = NP.nanoflann_sqd(q, p1).astype(F64)
    ok = np.where(has_p1, dn < lb2, lb2 > float(cap2))
    return ok & (np.asarray(B2, F32) >= 0)


def decided(q, qref, B2, p1, has_p1, cap2):
    """(passes, decided): the rule's answer, and whether it is the same with lb2 a relative
    MARGIN lower and higher (the device's double arithmetic should be bit-equal to numpy's;
    the margin makes it not matter)."""
    lo = pass_rule(q, qref, B2, p1, has_p1, cap2, -MARGIN)
    hi = pass_rule(q, qref, B2, p1, has_p1, cap2, +MARGIN)
    return lo, lo == hi


def mv_bound(T_prev, T_next, src_radius):
    """k_lm_step's bound on how far the step T_prev -> T_next moved a source point, and
    is_converged's measure of the step (lm_step.hpp), with the reference's epsilons."""
    D = np.asarray(T_next, F64) @ np.linalg.inv(np.asarray(T_prev, F64))
    dR, dt = D[:3, :3] - np.eye(3), D[:3, 3]
    mv = np.linalg.norm(dR) * (src_radius + np.linalg.norm(np.asarray(T_next, F64)[:3, 3])) + np.linalg.norm(dt)
    return float(mv), D


def group_rank(source):
    """Rank of every source point in the device's sorted (Morton) order: 16 consecutive
    ranks are one sub-group (set_shard_groups owns whole sub-groups)."""
    rank = np.empty(len(source), np.int64)
    rank[GC.morton_order(source)[0]] = np.arange(len(source))
    return rank


def owned_mask(source, q, shard):
    """The queries a shard owns at fp32 positions q: shard = (axis, lo, hi, nparts, part)."""
    if shard is None:
        return np.ones(len(q), bool)
    axis, lo, hi, nparts, part = shard
    own = (q[:, axis] >= F32(lo)) & (q[:, axis] < F32(hi))
    if nparts:
        own &= (group_rank(source) // 16) % nparts == part
    return own


class Step(NamedTuple):
    q: np.ndarray           # fp32 queries
    d1: np.ndarray
    j1: np.ndarray
    d2: np.ndarray
    cnt: np.ndarray
    owned: np.ndarray
    sure_pass: np.ndarray   # proven by whichever reference the query can hold, at both bounds
    sure_search: np.ndarray
    undecided: np.ndarray
    has_ref: np.ndarray     # a reference exists after the step (certain: "no reference" is never in doubt)


def simulate(case, shard=None):
    """What holds at every step of the script without the device.  A query's reference is
    that of the last recording step that searched it; where a pass was undecided at a
    recording step both that step and the earlier ones stay candidates."""
    tgt, src = case.target, case.source
    cap2 = cap2_of(case.bound)
    S, M = len(case.script), len(src)
    cand = np.zeros((S, M), bool)
    steps = []
    any_rec = False
    for s, (pose, rec) in enumerate(case.script):
        q = NP.transform_f32(pose, src)
        d1, j1, d2, cnt = brute2(tgt, q)
        own = owned_mask(src, q, shard)
        every = np.ones(M, bool)
        some = np.zeros(M, bool)
        if s >= 1 and any_rec:   # check_ref = reuse && have_prev && any_rec
            for r in np.flatnonzero(cand.any(1)):
                R = steps[r]
                lo, hi = b2_bounds(R.d1, R.d2, cap2, REUSE_GAP if r >= 1 else REUSE_GAP0, tight=True)
                has_p1 = R.d1 < cap2
                p1 = tgt[R.j1]
                sp = pass_rule(q, R.q, lo, p1, has_p1, cap2, -MARGIN)
                pp = pass_rule(q, R.q, hi, p1, has_p1, cap2, +MARGIN)
                every &= np.where(cand[r], sp, True)
                some |= cand[r] & pp
        sure_pass = own & cand.any(0) & every & (s >= 1 and any_rec)
        sure_search = own & ~some
        und = own & ~sure_pass & ~sure_search
        if rec:
            if not any_rec:
                cand[:] = False   # the first recording step clears what it does not search
            cand[:, sure_search] = False
            cand[s, sure_search | und] = True
            any_rec = True
        steps.append(Step(q, d1, j1, d2, cnt, own, sure_pass, sure_search, und, cand.any(0).copy()))
    return steps


# ---------------------------------------------------------------------------
# case 1: steps
STEP_DIR = np.array([0.6, 0.64, 0.48])   # unit


def walls(n_floor=3600, n_wall=1200, seed=3, jitter=0.01):
    """Two walls and a floor of a 10 m room, about 6,000 points (two box levels)."""
    rng = np.random.default_rng(seed)
    f = np.stack([rng.uniform(0, 10, n_floor), rng.uniform(0, 10, n_floor), np.zeros(n_floor)], 1)
    w1 = np.stack([np.zeros(n_wall), rng.uniform(0, 10, n_wall), rng.uniform(0, 3, n_wall)], 1)
    w2 = np.stack([rng.uniform(0, 10, n_wall), np.zeros(n_wall), rng.uniform(0, 3, n_wall)], 1)
    t = np.concatenate([f, w1, w2])
    return t + rng.normal(0, jitter, t.shape)


def near_walls(m=1000, seed=4):
    """m points within 0.15 m of the same surfaces, in the room's frame."""
    rng = np.random.default_rng(seed)
    k = m // 2
    f = np.stack([rng.uniform(0.3, 9.7, k), rng.uniform(0.3, 9.7, k), rng.uniform(0, 0.15, k)], 1)
    k2 = (m - k) // 2
    w1 = np.stack([rng.uniform(0, 0.15, k2), rng.uniform(0.3, 9.7, k2), rng.uniform(0.2, 2.8, k2)], 1)
    k3 = m - k - k2
    w2 = np.stack([rng.uniform(0.3, 9.7, k3), rng.uniform(0, 0.15, k3), rng.uniform(0.2, 2.8, k3)], 1)
    return np.concatenate([f, w1, w2])


STEPS_GUESS = NP._delta(np.array([0.002, -0.001, 0.01, 0.08, -0.05, 0.02]))
STEPS_RECS = {"natural": (0, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0), "rec0": (1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0),
              "all": (1,) * 11}
YAW_AXIS = np.array([-1.0, -1.0, 0.0])   # see steps()


def steps_script(G, recs, shift):
    cum = np.cumsum([0.0, 0.03, 0.01, 0.002, 0.06, 0.19, 0.25, 3.0])
    poses = [f32_pose(translation(STEP_DIR * c) @ G) for c in cum]
    poses.append(poses[3])                                          # back to exactly the fourth pose
    poses.append(f32_pose(yaw_about(0.02, YAW_AXIS + shift) @ poses[3]))   # near queries < 0.05 m, far ones > 0.2 m
    poses.append(poses[3])                                          # the same yaw back
    return list(zip(poses, recs))


def steps(variant="natural", shift=None, seed=3):
    """Case 1.  The source is the room's points seen from a frame the guess G maps back, so
    the queries at G lie near the target.  Steps, cumulative from G along STEP_DIR: G; 0.03 m
    (recording); + 0.01 (most pass); + 0.002 (recording: passes keep, searches re-record);
    + 0.06 (beyond the gap); + 0.19 (the triangle bound just below tri_mv); + 0.25 (just above:
    the previous match's distance and the window); + 3 m (no seed from the past); back to the
    fourth pose (old references prove again: every query, since each either passed there or was
    recorded there, so this step has no sure search); a yaw of 0.02 rad (recording) and back.
    Variants: rec0 also records at step 0 and all at every step.  Iteration 0 has gap0 = 0: its
    walk radius is the seed bound itself, so its B2 is d1 (the seed found the match: nothing
    provable) or d2 (it found another point) and the two bounds cannot tell which; while such a
    reference is live the share of decided queries is printed, not held to 90 %.  The yaw's
    vertical axis stands 1 m outside the room's corner, not 30 m away: at 0.02 rad a query moves
    0.02 m per metre from the axis, so only an axis near the cloud leaves queries below
    reuse_rec_eps (within 2.5 m of it) and above tri_mv (beyond 10 m) in one step."""
    shift = np.zeros(3) if shift is None else np.asarray(shift, F64)
    tgt = walls(seed=seed) + shift
    G = translation(shift) @ STEPS_GUESS
    src = (near_walls(seed=seed + 1) - STEPS_GUESS[:3, 3]) @ STEPS_GUESS[:3, :3]   # G^-1 of the room points
    return WalkCase(f"steps_{variant}", np.ascontiguousarray(tgt, F32), np.ascontiguousarray(src, F32), 1.0,
                    steps_script(G, STEPS_RECS[variant], shift),
                    dict(tie_free=True, pass_steps=(2, 3, 10), all_pass_steps=(8,) if variant == "natural" else (), purpose=(),
                         gap0=variant != "natural"))


def far_origin(variant="natural"):
    """Case 5: case 1 shifted by grid_cases.FAR1 (fp32 coordinates of 4-8 km)."""
    c = steps(variant, shift=GC.FAR1)
    return c._replace(name=f"far_{variant}", expect=dict(c.expect, pass_steps=(), all_pass_steps=(), tie_free=False))


# ---------------------------------------------------------------------------
# case 2: bound
def _sq_search(target_value, base):
    """A float32 dz near base whose fp32 square is exactly target_value, helped by a small dx:
    (dx, dz) with fl(fl(dx dx) + fl(dz dz)) == target_value."""
    tv = F32(target_value)
    dz = F32(base)
    for _ in range(64):
        dz = np.nextafter(dz, F32(0))
    for _ in range(128):
        for k in range(0, 64):
            dx = F32(k * 2.0 ** -14)
            if F32(dx * dx) + F32(dz * dz) == tv and F32(F32(dx * dx) + F32(0)) + F32(dz * dz) == tv:
                return dx, dz
        dz = np.nextafter(dz, F32(np.inf))
    raise AssertionError(f"no fp32 offset squares to {target_value!r}")


def bound_case(bound):
    """Case 2.  A floor of 2,100 jittered points (two box levels) far below, and isolated
    posts 3 m apart with one query straight above each at bound + 0.02, 0.04, 0.06 and 0.2 m
    (8 of each), plus three whose fp32 d2 is float32(bound^2), one ulp below and one above
    (the last is cap2 itself).  Poses are pure translations from the identity, so the first
    queries are the source points bit for bit.  Script: the identity recording (iteration 0:
    gap0 = 0, the radius is not widened); the same pose recording again (a previous iteration
    exists now: the widened radius, the step the issue calls "step 0"); 0.03 m sideways (0.04 m
    and beyond: proven unmatched; 0.02 m: searched); 0.3 m towards the posts (searched,
    matched); back out."""
    rng = np.random.default_rng(5)
    floor = np.stack([rng.uniform(0, 30, 2100), rng.uniform(0, 12, 2100), np.full(2100, -6.0)], 1)
    floor += rng.normal(0, 0.01, floor.shape)
    posts, src, kinds = [], [], []
    k = 0
    for d in BOUND_DELTAS:
        for _ in range(8):
            p = np.array([3.0 * (k % 10) + 1.0, 3.0 * (k // 10) + 1.0, 0.0])
            posts.append(p)
            src.append(p + np.array([0.0, 0.0, bound + d]))
            kinds.append(d)
            k += 1
    b2 = F32(bound * bound)
    for tv, kind in ((b2, "at"), (np.nextafter(b2, F32(0)), "below"), (np.nextafter(b2, F32(np.inf)), "above")):
        dx, dz = _sq_search(tv, bound)
        p = np.array([3.0 * (k % 10) + 1.0, 3.0 * (k // 10) + 1.0, 0.0])
        posts.append(p)
        src.append(p + np.array([float(dx), 0.0, float(dz)]))
        kinds.append(kind)
        k += 1
    tgt = np.concatenate([np.array(posts), floor])
    side, down = np.array([0.03, 0.0, 0.0]), np.array([0.0, 0.0, -0.3])
    poses = [np.eye(4), np.eye(4), f32_pose(translation(side)), f32_pose(translation(side + down)),
             f32_pose(translation(side))]
    edge = tuple(i for i, kd in enumerate(kinds) if isinstance(kd, str))
    return WalkCase(f"bound{bound}", np.ascontiguousarray(tgt, F32), np.ascontiguousarray(np.array(src), F32), float(bound),
                    list(zip(poses, (1, 1, 0, 0, 0))),
                    dict(tie_free=True, pass_steps=(2,), purpose=edge, kinds=kinds))


# ---------------------------------------------------------------------------
# case 3: near ties
NEAR_OFFSETS = (1e-6, 3e-6, 1e-5, 1.5e-5, 2.5e-5, 4.5e-5, 1e-4, 1e-3)
NEAR_HALF = 0.1     # the pair's points at -+ NEAR_HALF from the bisector plane
ULP_HALF = 0.01     # ... of the pair at the origin: x steps of 1e-9 there move d2 - d1 by a fraction of an ulp


def _ulp_queries():
    """x offsets from the bisector of the pair at the origin whose fp32 d2 - d1 is exactly 1, 2
    and 3 ulps (y = 0.05 off the pair's axis): found by search over multiples of 1e-9."""
    out = {}
    a, b = np.array([-ULP_HALF, 0, 0], F32), np.array([ULP_HALF, 0, 0], F32)
    for k in range(1, 4000):
        q = np.array([k * 1e-9, 0.05, 0.0], F32)
        da, db = NP.nanoflann_sqd(q, a), NP.nanoflann_sqd(q, b)
        lo, hi = min(da, db), max(da, db)
        n = int(hi.view(np.int32)) - int(lo.view(np.int32))
        if n in (1, 2, 3) and n not in out:
            out[n] = q.astype(F64)
        if len(out) == 3:
            break
    assert len(out) == 3, out
    return out


def near_ties():
    """Case 3.  Pairs of target points 0.2 m apart (0.02 m at the origin), 3 m from one another, and queries
    NEAR_OFFSETS off their bisector planes on both sides; the pair at the origin also has the
    three queries whose d2 - d1 is 1, 2 and 3 float32 ulps.  Six steps of 1e-5 m along the
    pairs' axis carry queries across the bisector, recording at every step.  These queries are
    undecided on purpose: their results are asserted, not their status."""
    rng = np.random.default_rng(6)
    floor = np.stack([rng.uniform(-2, 28, 2100), rng.uniform(-2, 4, 2100), np.full(2100, -6.0)], 1)
    floor += rng.normal(0, 0.01, floor.shape)
    tgt, src = [], []
    for p in range(10):
        c = np.array([3.0 * p, 0.0, 0.0])
        h = ULP_HALF if p == 0 else NEAR_HALF
        tgt += [c - [h, 0, 0], c + [h, 0, 0]]
        if p == 0:
            src += [v for v in _ulp_queries().values()]
        for o in NEAR_OFFSETS:
            for sgn in (-1.0, 1.0):
                src.append(c + np.array([sgn * o, 0.03 + 0.01 * (p % 4), 0.02]))
    poses = [f32_pose(translation([k * 1e-5, 0.0, 0.0])) for k in range(7)]
    src = np.ascontiguousarray(np.array(src), F32)
    return WalkCase("near_ties", np.ascontiguousarray(np.concatenate([np.array(tgt), floor]), F32), src, 1.0,
                    list(zip(poses, (1,) * 7)), dict(tie_free=False, pass_steps=(), purpose=tuple(range(len(src)))))


# ---------------------------------------------------------------------------
# case 4: ties
def ties(variant="first"):
    """Case 4.  The integer lattice of the kNN goldens (tests/golden/knn_ref.npz, lat_pts)
    queried at 200 cell centres: 8 equidistant corners each.  Steps by exact binary fractions
    (the fp32 query is exact): tied 8-way; unique by 2^-10 on every axis; tied 4-way on a face
    (2^-10 on x only); unique (2^-10, 2^-11, 2^-12).  Recording throughout.
    Variant "late": a unique pose first, recording, then the 8-way tie without recording: the
    step that first meets a tie (and makes the device build its tie tree and run the step
    again) then has a carried state to keep, the references of the step before it."""
    lat = np.load(os.path.join(GOLDEN, "knn_ref.npz"))["lat_pts"]
    rng = np.random.default_rng(8)
    hi = int(lat.max())
    cells = np.unique(rng.integers(0, hi, (260, 3)), axis=0)[:200]
    src = cells.astype(F64) + 0.5
    e = 2.0 ** -10
    poses = [np.eye(4), translation([e, e, e]), translation([e, 0, 0]), translation([e, e / 2, e / 4])]
    recs, tied = (1, 1, 1, 1), (8, 1, 4, 1)
    if variant == "late":
        poses, recs, tied = [poses[3], poses[0], poses[2], poses[1]], (1, 0, 1, 0), (1, 8, 4, 1)
    return WalkCase(f"ties_{variant}", np.ascontiguousarray(lat, F32), np.ascontiguousarray(src, F32), 2.0,
                    list(zip(poses, recs)), dict(tie_free=False, pass_steps=(), purpose=(), tied=tied))


# ---------------------------------------------------------------------------
# case 6: sizes
def sizes(nt):
    """Case 6.  nt target points in a 2 m cube (1 .. 2,049: a target shorter than the Morton
    window, one and two box levels) and 257 source points in it; the device test runs every
    prefix of SIZES_SRC.  No recording, recording 0.02 m on, then a 0.005 m step."""
    rng = np.random.default_rng(100 + nt)
    tgt = rng.uniform(0, 2, (nt, 3))
    src = rng.uniform(0.1, 1.9, (257, 3))
    poses = [np.eye(4), f32_pose(translation(STEP_DIR * 0.02)), f32_pose(translation(STEP_DIR * 0.025))]
    return WalkCase(f"sizes{nt}", np.ascontiguousarray(tgt, F32), np.ascontiguousarray(src, F32), 1.0,
                    list(zip(poses, (0, 1, 0))), dict(tie_free=True, pass_steps=(), purpose=()))


# ---------------------------------------------------------------------------
# case 7: two aligns on one context
def second_run():
    """Case 7's second run: a room of the same sizes with other points (another seed), whose
    first two steps do not record.  Nothing the first run (steps("all")) recorded may be used."""
    c = steps("natural", seed=13)
    poses = [p for p, _ in c.script[:5]]
    return c._replace(name="second_run", script=list(zip(poses, (0, 0, 1, 0, 0))),
                      expect=dict(tie_free=True, pass_steps=(3,), all_pass_steps=(), purpose=(), gap0=False))


# ---------------------------------------------------------------------------
# case 8: shards
SHARD_LO = 5.0


SHARDS = {"slab": (0, SHARD_LO, np.inf, 0, 0), "both": (0, SHARD_LO, np.inf, 3, 1)}


def shards(kind="slab"):
    """Case 8.  Case 1's clouds under set_shard(axis 0, SHARD_LO, +inf) through the room, alone
    ("slab") and with set_shard_groups(3, 1) on top ("both": a third of the 16-query groups).  Steps of 0.01 to 0.32 m along x carry queries across SHARD_LO in both
    directions; the first recording step (step 1) happens while some queries are not owned, and
    queries first owned later have no reference until a recording step searches them."""
    c = steps("natural")
    G = c.script[0][0]
    xs = (0.0, 0.15, 0.16, 0.31, 0.32, 0.0, -0.15, -0.14)
    poses = [f32_pose(translation([x, 0.0, 0.0]) @ G) for x in xs]
    return c._replace(name=f"shards_{kind}", script=list(zip(poses, (0, 1, 0, 1, 0, 0, 1, 0))),
                      expect=dict(tie_free=True, pass_steps=(2, 4, 7), all_pass_steps=(), purpose=(), gap0=False,
                                  shard=SHARDS[kind]))


# ---------------------------------------------------------------------------
# case 9: cells in front of the walk
def cells():
    """Case 9.  grid_cases.shell_over(2049, 5.0): with the cells on, k_cell_lookup hands only
    the listed sub-groups' unanswered queries to the walk.  Four steps with recording."""
    g = GC.shell_over(2049, 5.0)
    poses = [np.eye(4), f32_pose(translation(STEP_DIR * 0.02)), f32_pose(translation(STEP_DIR * 0.03)),
             f32_pose(translation(STEP_DIR * 0.032))]
    return WalkCase("cells", g.target, g.source, 5.0, list(zip(poses, (0, 1, 0, 1))),
                    dict(tie_free=True, pass_steps=(2, 3), purpose=()))


# ---------------------------------------------------------------------------
# real aligns with natural recording
ALIGN_GUESS = translation([0.25, -0.15, 0.1])
ALIGN_M = 8


def align_case():
    """Case 1's clouds for truncated aligns from ALIGN_GUESS (a pure translation off the
    solution: LM's later steps are small and far from converged, so k_lm_step records)."""
    c = steps("natural")
    G = f32_pose(ALIGN_GUESS @ c.script[0][0])
    return c._replace(name="align", script=[(G, 0)])


S2S_OFFSET = np.array([0.08, -0.04, 0.016])   # the s2s golden's guess: this far off its T_true
S2S_TRANS_EPS = 1e-4                          # (at the default 5e-4 its align ends with the iteration that records)
ALIGN_PARAMS = {"case1": dict(k_correspondences=10, max_correspondence_distance=1.0),
                "s2s": dict(k_correspondences=10, max_correspondence_distance=1.0, transformation_epsilon=S2S_TRANS_EPS)}


def align_problem(which):
    """(target, source, guess as exact float32, bound, golden or None) of the truncated aligns:
    case 1 from ALIGN_GUESS, and tests/golden/gicp_s2s.npz from S2S_OFFSET off its T_true."""
    if which == "case1":
        c = align_case()
        return c.target, c.source, c.script[0][0], c.bound, None
    g = np.load(os.path.join(GOLDEN, "gicp_s2s.npz"))
    return g["tgt"], g["src"], f32_pose(translation(S2S_OFFSET) @ g["T_true"]), 1.0, g


def natural_recording(poses, src_radius, trans_eps, rot_eps):
    """From the poses after 0 .. n iterations (poses[0] the guess): the iterations k whose step
    poses[k - 1] -> poses[k] makes k_lm_step set rec for iteration k's search (0-based iteration
    k runs at poses[k])."""
    out = []
    for k in range(1, len(poses)):
        mv, D = mv_bound(poses[k - 1], poses[k], src_radius)
        cm = max(np.abs(D[:3, :3] - np.eye(3)).max() / rot_eps, np.abs(D[:3, 3]).max() / trans_eps)
        if mv < 0.95 * REUSE_REC_EPS and cm > 1.05 * REUSE_REC_CONV:   # (5 %: the device's src_radius is a box bound)
            out.append(k)
    return out


@functools.lru_cache(maxsize=None)
def cached(name, *args):
    """(case, simulate(case)) of a generator by name, computed once per process."""
    case = globals()[name](*args)
    return case, simulate(case, case.expect.get("shard"))
