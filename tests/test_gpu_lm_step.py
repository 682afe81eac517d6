"""The LM / GN step kernel alone (gicp_debug_lm_step: one 512-thread launch of k_lm_step on given
moments) against tests/lm_ref.py, the reference's sequential trial loop evaluated over the points.

Through gicp_align the step never rejects a trial (nearest-neighbour pairings always lower the frozen
cost), so here the pairing is given: n = 40 points, a ~ N(0, diag(4, 4, 1)), b = s R(theta axis) a +
0.05 noise, random SPD M_i with eigenvalues in [0.2, 5] (lm_ref.make_problem), for which LM rejects 7 or
8 trials in a row.  Every case first asserts on the CPU that the reference's own min |rho| over the
trials is >= 0.01 and cond(H + lambda I) <= 1e8: the decisions are far from their thresholds, so a
correct kernel takes the reference's.

Tolerances:
  decisions, counts, flags          exact
  H, b                              rel 1e-11 (the project's figure for moments)
  pose after an accepted step       against x_ref = [so3_exp(d) | d_t] * x_in with d = Eigen's LDLT
      (oracle.ldlt_solve6) on the DEVICE's own H, b and the trial's lambda, so d is the same operations
      on the same bits and only so3_exp's sin / cos differ (device sincos vs libm, <= 2 ulp each,
      u = 2^-53 = eps / 2).  imag = sin / theta: 3u relative; a quaternion entry: 4u; a product
      t_ij = 2 q_i q_j (|t_ij| <= 2): 9u relative, 18u = 9 eps absolute; an entry of Rd adds two of them
      and rounds twice: <= 20 eps.  Rn = Rd R (|R[:, j]|_1 <= sqrt 3) then differs by <= 35 eps plus the
      3 roundings of the dot: POSE_EPS = 40 eps; tn = Rd t + td by <= 40 eps |t|_1 + 2 eps |tn|
      ("a few eps (1 + |t|)").  From a pose with t = 0 the new translation is td itself: d[3:] bit for bit,
      which is what tells Eigen's tie rule in the pivot search from the other one (they differ by an ulp).
  lambda of the deciding trial      bit for bit lambda_0 2^(i (i + 1) / 2) (doubling is exact), seen directly
      after a rejected-but-converged step and through lambda_i * (1 / 3) whenever the update factor is clamped
  updated lambda                    16 x the float64 / longdouble spread of the reference's update factor
      max(1/3, 1 - (2 rho - 1)^3).  The spread is the larger of the factor's own two-run difference and
      |d factor / d rho| |rho| times the relative spread of rho: the largest two-run difference over the
      step's trials (one trial's difference can vanish by chance; tests/test_lm_ref_cpu.py measures the
      same figure), and at least the formats' floor eps (y0 + y_i) / (2 |y0 - y_i|), one rounding of
      each of the two costs whose difference is rho's numerator.  A clamped factor has spread 0: lambda
      is then bit for bit.  Measured on an MI355X: |device - reference| is 0.01 .. 1.1 times the spread
      (2.5e-12 relative at the most): the device's moment form agrees with the longdouble run, and the
      float64 sum over the points carries the difference.

On failure the device leaves lambda_{n-1} * 2 where the sequential loop leaves lambda_{n-1} * 2^n; the
reference has no accessor for it and the align ends, so it is not compared.

Measured on an MI355X: the whole file takes 2.3 s of wall time (1.6 s of it the first context).
"""
import functools

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
import lm_ref as LR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
POSE_EPS = 40 * EPS
LD = np.longdouble
I6 = np.eye(6)
CASE_IDS = [f"s{c[0]:g}_th{c[1]:g}" for c in LR.REJECTING]
PATHS = ["premom", "slab"]
NROWS = 7


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def set_params(ctx, p: LR.Params):
    ctx.set_params(P.default_params(optimizer=p.optimizer, lm_max_iterations=p.lm_max_iterations,
                                    lm_init_lambda_factor=p.lm_init_lambda_factor,
                                    transformation_epsilon=p.transformation_epsilon,
                                    rotation_epsilon=p.rotation_epsilon, max_iterations=p.max_iterations,
                                    fixed_iterations=p.fixed_iterations))


def device_step(ctx, p, prob, path="premom"):
    a, b, M, R, t, lam, it, ntr = prob
    set_params(ctx, p)
    if path == "premom":
        return ctx.lm_step(R, t, lam, it, ntr, mom=LR.moments(a, b, M, R, t))
    return ctx.lm_step(R, t, lam, it, ntr, slab=LR.moment_rows(a, b, M, R, t, NROWS))


def pose_of(out):
    return np.array(out.R).reshape(3, 3), np.array(out.t)


def kind_of(out, prob):
    R, t = pose_of(out)
    if out.lm_failed:
        return "failed"
    moved = not (np.array_equal(R, np.asarray(prob[3], np.float64)) and np.array_equal(t, np.asarray(prob[4], np.float64)))
    return "accepted" if moved else "rejected_converged"


@functools.lru_cache(maxsize=None)
def rejecting(k):
    """Case k's rejecting step and its reference outcome (float64 and longdouble), computed once; the CPU
    preconditions of the issue are asserted here, for every test that uses the case."""
    prob = LR.rejecting_step(*LR.REJECTING[k])
    a, b, M, R, t, lam, it, ntr = prob
    p = LR.Params(lm_max_iterations=64)
    ref = LR.step(a, b, M, R, t, lam, p, it=it, lm_trials=ntr)
    refl = LR.step(a, b, M, R, t, lam, p, it=it, lm_trials=ntr, dt=LD)
    check_preconditions(ref)
    assert ref.kind == refl.kind == "accepted" and 8 <= ref.trials_used == refl.trials_used <= 10
    return prob, ref, refl


def check_preconditions(ref):
    assert min(abs(float(x[1])) for x in ref.trials) >= 0.01
    assert max(np.linalg.cond(ref.H + float(x[0]) * I6) for x in ref.trials) <= 1e8


def assert_bookkeeping(out, ref, prob):
    assert kind_of(out, prob) == ref.kind
    got = (out.lm_trials - prob[7], out.lm_trials, out.iter, out.nr_iterations, out.converged, out.lm_failed, out.done,
           out.num_corr)
    want = (ref.trials_used, ref.lm_trials, ref.iter, ref.nr_iterations, ref.converged, ref.lm_failed, ref.done,
            ref.num_corr)
    assert got == want, f"(trials, lm_trials, iter, nr_iterations, converged, lm_failed, done, num_corr): {got} != {want}"


def trial_lambda(out, prob, p, H_dev):
    """lambda of the deciding trial i = trials used - 1: lambda_0 2^(i (i + 1) / 2), lambda_0 the carried value or,
    at the first step, lm_init_lambda_factor * max |diag H| of the device's own H (one product: the same bits)."""
    lam0 = prob[5] if prob[5] >= 0 else p.lm_init_lambda_factor * np.abs(np.diag(H_dev)).max()
    i = out.lm_trials - prob[7] - 1
    return float(np.ldexp(lam0, i * (i + 1) // 2))


def assert_pose_from_device_system(out, prob, lam_i):
    """The new pose is [so3_exp(d) | d_t] * x_in for d = Eigen's LDLT on the device's own H + lambda I and b."""
    H = np.array(out.final_hessian).reshape(6, 6)
    bb = np.array(out.last_b)
    d = O.ldlt_solve6(H + lam_i * I6, -bb)
    Rd = O.so3_exp(d[:3])
    R0, t0 = np.asarray(prob[3], np.float64), np.asarray(prob[4], np.float64)
    Rn = np.array([[Rd[i, 0] * R0[0, j] + Rd[i, 1] * R0[1, j] + Rd[i, 2] * R0[2, j] for j in range(3)] for i in range(3)])
    tn = np.array([(Rd[i, 0] * t0[0] + Rd[i, 1] * t0[1] + Rd[i, 2] * t0[2]) + d[3 + i] for i in range(3)])
    R, t = pose_of(out)
    assert np.abs(R - Rn).max() <= POSE_EPS, f"R differs by {np.abs(R - Rn).max() / EPS:.1f} eps"
    tol = POSE_EPS * np.abs(t0).sum() + 2 * EPS * np.abs(tn).max()
    assert np.abs(t - tn).max() <= tol, f"t differs by {np.abs(t - tn).max() / EPS:.1f} eps (allowed {tol / EPS:.1f})"
    if not t0.any():   # Rd * 0 + td: the new translation IS the solve's translation part, to the bit
        np.testing.assert_array_equal(t, d[3:])
    return d


def factor_spread(ref, refl):
    """float64 / longdouble spread of the accepted trial's update factor (module docstring)."""
    if ref.factor == 1.0 / 3.0 and refl.factor == LD(1) / LD(3):
        return 0.0   # clamped in both runs
    own = abs(float(refl.factor) - float(ref.factor))
    lam, rho, _ = (float(x) for x in ref.trials[-1])
    rel = max(abs(float(xl[1]) - float(x[1])) / abs(float(x[1])) for x, xl in zip(ref.trials, refl.trials))
    # the formats' floor of that figure: rho's numerator y0 - y_i is the difference of two sums rounded to
    # fp64 once each at least, eps (y0 + y_i) / 2 absolute
    dy = rho * float(ref.d @ (lam * ref.d - ref.b))
    y0 = float(ref.y0)
    rel = max(rel, 0.5 * EPS * (2 * y0 - dy) / abs(dy))
    return max(own, 6 * (2 * rho - 1) ** 2 * abs(rho) * rel)


def assert_updated_lambda(out, ref, refl, lam_i):
    spread = factor_spread(ref, refl)
    want = lam_i * float(ref.factor)
    err = abs(out.lambda_ - want) / lam_i
    print(f"lambda {out.lambda_:.17g}: factor {float(ref.factor):.6g}, |device - reference| {err:.3g}, spread {spread:.3g}")
    assert err <= 16 * spread


# ---- single steps --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", range(len(LR.REJECTING)), ids=CASE_IDS)
def test_rejecting_step_decisions_solve_pose_and_lambda(ctx, k, path):
    """A step that rejects 7 or 8 trials before it accepts: the reference's decisions and counts exactly,
    H and b at rel 1e-11, the pose from the device's own system through Eigen's LDLT, lambda_i bit for
    bit and the updated lambda within the reference's spread (module docstring)."""
    prob, ref, refl = rejecting(k)
    p = LR.Params()
    out = device_step(ctx, p, prob, path)
    assert_bookkeeping(out, ref, prob)
    H = np.array(out.final_hessian).reshape(6, 6)
    np.testing.assert_allclose(H, ref.H, rtol=1e-11, atol=1e-11 * np.abs(ref.H).max())
    np.testing.assert_allclose(np.array(out.last_b), ref.b, rtol=1e-11, atol=1e-11 * np.abs(ref.b).max())
    assert abs(out.final_cost - float(ref.y0)) <= 1e-11 * float(ref.y0)
    lam_i = trial_lambda(out, prob, p, H)
    np.testing.assert_allclose(lam_i, float(ref.lam_trial), rtol=1e-11)
    assert_pose_from_device_system(out, prob, lam_i)
    assert_updated_lambda(out, ref, refl, lam_i)
    # and the pose the reference reached (np.linalg.solve on its own H, b): the two solves agree to
    # cond * (1e-11 + 64 eps) |d|, amplified by the pose like POSE_EPS
    R, t = pose_of(out)
    c = np.linalg.cond(ref.H + lam_i * I6) * (1e-11 + 64 * EPS) * max(1.0, np.abs(ref.d).max())
    assert np.abs(R - ref.R).max() <= c and np.abs(t - ref.t).max() <= c * (1 + np.abs(prob[4]).sum())


def test_control_never_rejects(ctx):
    """(s, theta) = (1, 0.3): one trial per step until convergence, through both paths alternately."""
    a, b, M = LR.make_problem(*LR.CONTROL)
    p = LR.Params()
    R, t, lam, it, ntr = np.eye(3), np.zeros(3), -1.0, 0, 0
    for k in range(8):
        prob = (a, b, M, R, t, lam, it, ntr)
        ref = LR.step(*prob[:6], p, it=it, lm_trials=ntr)
        check_preconditions(ref)
        out = device_step(ctx, p, prob, PATHS[k % 2])
        assert ref.trials_used == 1
        assert_bookkeeping(out, ref, prob)
        H = np.array(out.final_hessian).reshape(6, 6)
        assert_pose_from_device_system(out, prob, trial_lambda(out, prob, p, H))
        (R, t), lam, it, ntr = pose_of(out), out.lambda_, out.iter, out.lm_trials
        if out.done:
            break
    assert out.converged and 2 <= k < 7


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", range(len(LR.REJECTING)), ids=CASE_IDS)
def test_lm_max_iterations_sweep(ctx, k, path):
    """lm_max_iterations below the needed trial count fails the step (lm_failed, done, lm_trials +=
    lm_max_iterations, the pose kept bit for bit); from the needed count on the result does not depend on
    it.  100 equals 64 and 10: the kernel evaluates at most 64 trials (one wavefront), but that clamp is
    unobservable, lambda_i = lambda_0 2^(i (i + 1) / 2) overflows to inf at i = 45 and no trial beyond
    can be the first to be taken."""
    prob, ref, _ = rejecting(k)
    need = ref.trials_used
    outs = {}
    for n in (1, 4, 8, 9, 10, 64, 100):
        p = LR.Params(lm_max_iterations=n)
        out = outs[n] = device_step(ctx, p, prob, path)
        R, t = pose_of(out)
        if n < need:
            assert (out.lm_failed, out.done, out.converged, out.lm_trials) == (1, 1, 0, prob[7] + n), n
            np.testing.assert_array_equal(R, prob[3])
            np.testing.assert_array_equal(t, prob[4])
            assert (out.iter, out.nr_iterations, out.num_corr) == (prob[6] + 1, prob[6], len(prob[0]))
        else:
            assert_bookkeeping(out, ref, prob)
    assert need in (8, 9)

    def same(x, y):
        return bytes(x) == bytes(y)
    assert same(outs[100], outs[64]) and same(outs[64], outs[10])
    if need <= 9:
        assert same(outs[10], outs[9])


@pytest.mark.parametrize("k", range(len(LR.REJECTING)), ids=CASE_IDS)
def test_rejected_but_converged(ctx, k):
    """With both epsilons at 1e3 the first (rejected) trial has converged: the step ends with converged,
    one more trial, the pose and lambda_0 untouched bit for bit (lambda_0 handed in, so that it is known
    to the bit)."""
    prob, ref, _ = rejecting(k)
    prob = prob[:5] + (float(ref.trials[0][0]),) + prob[6:]
    p = LR.Params(transformation_epsilon=1e3, rotation_epsilon=1e3)
    r = LR.step(*prob[:6], p, it=prob[6], lm_trials=prob[7])
    assert r.kind == "rejected_converged" and r.trials_used == 1
    for path in PATHS:
        out = device_step(ctx, p, prob, path)
        assert_bookkeeping(out, r, prob)
        assert (out.converged, out.lm_failed, out.done, out.lm_trials) == (1, 0, 1, prob[7] + 1)
        R, t = pose_of(out)
        np.testing.assert_array_equal(R, prob[3])
        np.testing.assert_array_equal(t, prob[4])
        assert out.lambda_ == prob[5]


@pytest.mark.parametrize("k", [2, 3], ids=[CASE_IDS[2], CASE_IDS[3]])
def test_rejected_then_converged_at_a_later_trial(ctx, k):
    """chosen > 0 through the converged branch: the epsilons lie between the step size of the last
    rejected trial j and those of the trials before it (geometric means; a measure that does not shrink
    is switched off with 1e3), so the reference rejects, goes on, and ends on trial j, rejected but
    converged; lambda is that trial's, lambda_0 2^(j (j + 1) / 2), bit for bit."""
    prob, ref, _ = rejecting(k)
    prob = prob[:5] + (float(ref.trials[0][0]),) + prob[6:]
    a, b, M, R, t, lam0 = prob[:6]
    ds = [np.linalg.solve(ref.H + float(x[0]) * I6, -ref.b) for x in ref.trials[:-1]]
    mr = [np.abs(LR.so3_exp(d[:3]) - np.eye(3)).max() for d in ds]
    mt = [np.abs(d[3:]).max() for d in ds]
    eps_r = float(np.sqrt(mr[-1] * min(mr[:-1]))) if mr[-1] < 0.95 * min(mr[:-1]) else 1e3
    eps_t = float(np.sqrt(mt[-1] * min(mt[:-1]))) if mt[-1] < 0.95 * min(mt[:-1]) else 1e3
    assert min(eps_r, eps_t) < 1e3
    p = LR.Params(transformation_epsilon=eps_t, rotation_epsilon=eps_r)
    r = LR.step(a, b, M, R, t, lam0, p, it=prob[6], lm_trials=prob[7])
    j = ref.trials_used - 2
    assert r.kind == "rejected_converged" and r.trials_used == j + 1 >= 2
    for path in PATHS:
        out = device_step(ctx, p, prob, path)
        assert_bookkeeping(out, r, prob)
        assert out.lambda_ == float(np.ldexp(lam0, j * (j + 1) // 2)) == float(r.lam)
        np.testing.assert_array_equal(pose_of(out)[0], R)
        np.testing.assert_array_equal(pose_of(out)[1], t)


def _converging_control_step():
    """The control problem's last step (the one that converges) of the reference chain."""
    a, b, M = LR.make_problem(*LR.CONTROL)
    p = LR.Params()
    R, t, lam, it, ntr = np.eye(3), np.zeros(3), -1.0, 0, 0
    for _ in range(8):
        s = LR.step(a, b, M, R, t, lam, p, it=it, lm_trials=ntr)
        if s.converged:
            return (a, b, M, R, t, lam, it, ntr)
        R, t, lam, it, ntr = s.R, s.t, float(s.lam), s.iter, s.lm_trials
    raise AssertionError("the control chain did not converge")


def test_fixed_iterations_and_max_iterations(ctx):
    """A step that converges sets converged and done; with fixed_iterations > 0 it never sets converged,
    and done only at the fixed count; iter + 1 >= max_iterations sets done without converged."""
    prob = _converging_control_step()
    it = prob[6]
    for p, want in ((LR.Params(), (1, 1)), (LR.Params(fixed_iterations=it + 3), (0, 0)),
                    (LR.Params(fixed_iterations=it + 1), (0, 1)), (LR.Params(fixed_iterations=it + 1, max_iterations=1), (0, 1))):
        ref = LR.step(*prob[:6], p, it=it, lm_trials=prob[7])
        assert (ref.converged, ref.done) == want
        for path in PATHS:
            assert_bookkeeping(device_step(ctx, p, prob, path), ref, prob)
    # a step far from convergence, at the last allowed iteration
    rprob, _, _ = rejecting(1)
    p = LR.Params(max_iterations=rprob[6] + 1)
    ref = LR.step(*rprob[:6], p, it=rprob[6], lm_trials=rprob[7])
    assert (ref.converged, ref.done, ref.kind) == (0, 1, "accepted")
    assert_bookkeeping(device_step(ctx, p, rprob), ref, rprob)
    p = LR.Params(max_iterations=rprob[6] + 2)
    out = device_step(ctx, p, rprob)
    assert (out.converged, out.done) == (0, 0)


@pytest.mark.parametrize("k", [0, 3], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_gauss_newton_step(ctx, k):
    """GN: one trial at lambda 0, always taken; lm_trials and lambda are untouched."""
    prob, _, _ = rejecting(k)
    prob = prob[:5] + (0.125,) + prob[6:]
    p = LR.Params(optimizer=LR.GN)
    ref = LR.step(*prob[:6], p, it=prob[6], lm_trials=prob[7])
    assert np.linalg.cond(ref.H) <= 1e8
    for path in PATHS:
        out = device_step(ctx, p, prob, path)
        assert (out.lm_trials, out.lambda_) == (prob[7], 0.125)
        assert (out.iter, out.nr_iterations, out.converged, out.lm_failed, out.done, out.num_corr) == \
            (ref.iter, ref.nr_iterations, ref.converged, ref.lm_failed, ref.done, ref.num_corr)
        H = np.array(out.final_hessian).reshape(6, 6)
        np.testing.assert_allclose(H, ref.H, rtol=1e-11, atol=1e-11 * np.abs(ref.H).max())
        assert_pose_from_device_system(out, prob, 0.0)


@pytest.mark.parametrize("factor", [1e-9, 1e-3])
def test_first_and_carried_lambda(ctx, factor):
    """lambda_pre < 0: lambda_0 = lm_init_lambda_factor * max |diag H|; lambda_pre >= 0 is used as given
    (0 included).  Seen through a rejected-but-converged step, which returns the trial's lambda itself."""
    a, b, M = LR.make_problem(*LR.REJECTING[0])
    R, t = LR.so3_exp([0.1, -0.2, 0.05]), np.array([0.3, -0.1, 0.2])
    H, _, _ = LR.linearize(a, b, M, R, t)
    p = LR.Params(lm_init_lambda_factor=factor, transformation_epsilon=1e3, rotation_epsilon=1e3)
    for lam_pre in (-1.0, 0.0, 0.75 * factor * np.abs(np.diag(H)).max()):
        prob = (a, b, M, R, t, lam_pre, 0, 0)
        ref = LR.step(*prob[:6], p)
        check_preconditions(ref)
        assert ref.kind == "rejected_converged"
        for path in PATHS:
            out = device_step(ctx, p, prob, path)
            assert_bookkeeping(out, ref, prob)
            if lam_pre >= 0:
                assert out.lambda_ == lam_pre
            else:
                np.testing.assert_allclose(out.lambda_, factor * np.abs(np.diag(H)).max(), rtol=1e-11)
    # and at an accepted first step, where the device's own H is returned: the product to the bit
    p = LR.Params(lm_init_lambda_factor=factor)
    prob = (a, b, M, R, t, -1.0, 0, 0)
    ref = LR.step(*prob[:6], p)
    refl = LR.step(*prob[:6], p, dt=LD)
    check_preconditions(ref)
    out = device_step(ctx, p, prob)
    assert_bookkeeping(out, ref, prob)
    lam_i = trial_lambda(out, prob, p, np.array(out.final_hessian).reshape(6, 6))
    assert_pose_from_device_system(out, prob, lam_i)
    assert_updated_lambda(out, ref, refl, lam_i)


def test_all_zero_moments(ctx):
    """No correspondences: H = b = 0, the solve's zero pivots give d = 0, rho = 0 / 0 is NaN and NaN is
    not < 0, so the trial is accepted (as the sequential loop does): the pose is unchanged bit for bit,
    converged, one trial, num_corr 0, lambda 0."""
    R, t = LR.so3_exp([0.3, 0.1, -0.2]), np.array([1.5, -2.5, 0.25])
    e = np.zeros((0, 3))
    prob = (e, e, np.zeros((0, 3, 3)), R, t, -1.0, 2, 5)
    p = LR.Params()
    ref = LR.step(*prob[:6], p, it=2, lm_trials=5, solve=O.ldlt_solve6)
    assert ref.kind == "accepted" and np.isnan(float(ref.trials[0][1])) and float(ref.lam) == 0.0
    for path in PATHS:
        out = device_step(ctx, p, prob, path)
        np.testing.assert_array_equal(pose_of(out)[0], R)
        np.testing.assert_array_equal(pose_of(out)[1], t)
        assert (out.lm_trials, out.iter, out.nr_iterations, out.converged, out.lm_failed, out.done, out.num_corr) == \
            (6, 3, 2, 1, 0, 1, 0) == (ref.lm_trials, ref.iter, ref.nr_iterations, ref.converged, ref.lm_failed, ref.done, 0)
        assert out.lambda_ == 0.0 and out.final_cost == 0.0
        assert not np.array(out.final_hessian).any() and not np.array(out.last_mom).any()


def test_invalid_arguments(ctx):
    R, t = np.eye(3), np.zeros(3)
    for kw in (dict(), dict(slab=np.zeros((1, 80)), mom=np.zeros(80)), dict(slab=np.zeros((0, 80))),
               dict(slab=np.zeros((257, 80)))):
        with pytest.raises(P.GicpError) as e:
            ctx.lm_step(R, t, **kw)
        assert e.value.status == 1   # GICP_EINVAL
    L = P.load()
    assert L.gicp_debug_lm_step(ctx.h, None, None, 0, None, None) == 1
    assert L.gicp_debug_lm_step(None, None, None, 0, None, None) == 1


# ---- rank-deficient and tied systems of the LDLT -------------------------------------------------------------
def _dyadic_problem(kind):
    """Problems whose moments are exact in fp64 (coordinates and offsets are multiples of 1/4, M = I or
    diag(0, 0, 1), identity pose), so zeros and ties on H's diagonal are exact."""
    rng = np.random.default_rng(5)
    n = 24
    if kind == "line":        # all points on the x axis: rotation about it is free, H[0, :] = 0 exactly
        a = np.zeros((n, 3))
        a[:, 0] = rng.integers(-20, 21, n) / 4.0
    elif kind in ("plane", "plane_normal"):
        a = np.zeros((n, 3))
        a[:, :2] = rng.integers(-20, 21, (n, 2)) / 4.0
    elif kind == "tied_random":   # no structure but M = I: H_tt = n I
        a = np.random.default_rng(1).integers(-20, 21, (n, 3)) / 4.0
    else:                     # symmetric under x <-> y: every point with its mirror image
        h = rng.integers(-20, 21, (n // 2, 3)) / 4.0
        a = np.concatenate([h, h[:, [1, 0, 2]]])
    off = np.array([0.25, 0.25, -0.5]) if kind == "xy_symmetric" else np.array([0.25, -0.5, 0.75])
    b = a + off
    if kind == "xy_symmetric":
        w = rng.integers(-2, 3, (n // 2, 3)) / 4.0
        b = b + np.concatenate([w, w[:, [1, 0, 2]]])
    if kind == "tied_random":
        b = b + np.random.default_rng(2).integers(-2, 3, (n, 3)) / 4.0
    M = np.broadcast_to(np.diag([0.0, 0.0, 1.0]) if kind == "plane_normal" else np.eye(3), (n, 3, 3)).copy()
    return a, b, M


@pytest.mark.parametrize("optimizer", [LR.GN, LR.LM], ids=["gn", "lm"])
@pytest.mark.parametrize("kind", ["line", "plane", "plane_normal", "xy_symmetric", "tied_random"])
def test_ldlt_rank_deficient_and_tied(ctx, kind, optimizer):
    """Eigen's pivoted LDLT as the device restates it, on systems where its rules decide d: zero pivots
    (line with M = I: rank 5; plane with M = n n^T: rank 3; GN adds no lambda, so they are exact zeros and
    the zero-pivot rule sets those entries of d to 0) and tied diagonal entries (M = I makes
    H_tt = n I, a three-way tie; the x <-> y symmetric problem also ties H[0, 0] and H[1, 1]), where the
    first largest entry is the pivot.  The pose must be the one Eigen's LDLT (oracle.ldlt_solve6) gives on
    the device's own H, b and lambda; the pose is the identity, so the translation is d[3:] bit for bit,
    and for the two tied problems the last-largest rule is shown to give other bits there.  No
    condition-number precondition: the reference solve is the bit-faithful restatement."""
    a, b, M = _dyadic_problem(kind)
    R, t = np.eye(3), np.zeros(3)
    mom = LR.moments(a, b, M, R, t)
    Hm, gm, _ = LR.normal_equations(mom)
    dg = np.diag(Hm)
    if kind == "line":
        assert dg[0] == 0 and not Hm[0].any()
    if kind == "plane_normal":
        assert dg[2] == dg[3] == dg[4] == 0 and np.linalg.matrix_rank(Hm) == 3
    if kind != "plane_normal":
        assert dg[3] == dg[4] == dg[5] == len(a)
    if kind == "xy_symmetric":
        assert dg[0] == dg[1]
    p = LR.Params(optimizer=optimizer)
    set_params(ctx, p)
    out = ctx.lm_step(R, t, -1.0, 0, 0, mom=mom)
    prob = (a, b, M, R, t, -1.0, 0, 0)
    assert kind_of(out, prob) == "accepted" and not out.lm_failed
    H = np.array(out.final_hessian).reshape(6, 6)
    np.testing.assert_array_equal(H, Hm)      # exact moments: the device's H and b are the same to the bit
    np.testing.assert_array_equal(np.array(out.last_b), gm)
    lam_i = 0.0 if optimizer == LR.GN else trial_lambda(out, prob, p, H)
    d = assert_pose_from_device_system(out, prob, lam_i)
    if kind in ("xy_symmetric", "tied_random"):
        np.testing.assert_array_equal(LR.ldlt_solve6(Hm + lam_i * I6, -gm), d)
        assert (LR.ldlt_solve6(Hm + lam_i * I6, -gm, first_largest=False)[3:] != d[3:]).any()
    if optimizer == LR.GN and kind == "line":
        assert d[0] == 0.0                    # the free rotation: Eigen's zero-pivot rule
    if optimizer == LR.GN and kind == "plane_normal":
        assert d[2] == d[3] == d[4] == 0.0


# ---- chains --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,later", [(0, True), (2, False), (4, True)], ids=[CASE_IDS[0], CASE_IDS[2], CASE_IDS[4]])
def test_chain_of_eight_steps(ctx, k, later):
    """8 steps from identity, the moments rebuilt on the host from the device's returned pose after each.
    Every step is compared with lm_ref at the device's own pose and lambda, so rounding does not
    accumulate into a decision: kind, counts and flags exactly, the pose through the device's own system
    and against the reference's, the updated lambda within the reference's spread.  The reference must
    have produced a step of at least 8 trials and, for (3, 1) and (10, 3), a later step of 2 or more
    ((8, 0.5) never rejects again: none of 149 seeds does)."""
    a, b, M = LR.make_problem(*LR.REJECTING[k])
    p = LR.Params()
    R, t, lam, it, ntr = np.eye(3), np.zeros(3), -1.0, 0, 0
    used = []
    for n in range(8):
        prob = (a, b, M, R, t, lam, it, ntr)
        ref = LR.step(*prob[:6], p, it=it, lm_trials=ntr)
        refl = LR.step(*prob[:6], p, it=it, lm_trials=ntr, dt=LD)
        check_preconditions(ref)
        assert ref.kind == refl.kind == "accepted" and ref.trials_used == refl.trials_used
        out = device_step(ctx, p, prob, PATHS[n % 2])
        assert_bookkeeping(out, ref, prob)
        H = np.array(out.final_hessian).reshape(6, 6)
        lam_i = trial_lambda(out, prob, p, H)
        assert_pose_from_device_system(out, prob, lam_i)
        assert_updated_lambda(out, ref, refl, lam_i)
        Rn, tn = pose_of(out)
        c = np.linalg.cond(ref.H + lam_i * I6) * (1e-11 + 64 * EPS) * max(1.0, np.abs(ref.d).max())
        assert np.abs(Rn - ref.R).max() <= c and np.abs(tn - ref.t).max() <= c * (1 + np.abs(t).sum())
        used.append(ref.trials_used)
        R, t, lam, it, ntr = Rn, tn, out.lambda_, out.iter, out.lm_trials
        assert not out.done
    first = next(i for i, u in enumerate(used) if u >= 8)
    assert (max(used[first + 1:]) >= 2) == later, used
    assert ntr == sum(used) and it == 8


# ---- the slab reduction --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows", [1, 2, 11, 12, 13, 23, 24, 25, 255, 256])
def test_reduce_slab_fixed_order(ctx, nrows):
    """The step's slab sum in its fixed order (partition p adds rows p, p + 12, ... from 0.0, then the 12
    partials 0..11 from 0.0), bit for bit, on rows whose magnitudes spread over 1e-8 .. 1e8 with mixed
    signs so that the order shows in the last bits (asserted: the reversed order gives another double
    from 3 rows on, the plain row-by-row order from 13 rows on, where a partition first holds two rows).
    The slab behind the rows is NaN up to the 256th row: a row read at or beyond nrows shows."""
    rows = LR.slab_rows(nrows, 100 + nrows)
    want = LR.reduce_rows(rows)
    assert np.isfinite(want).all()
    if nrows >= 3:
        assert not np.array_equal(LR.reduce_rows(rows[::-1]), want)
    if nrows > LR.PARTS:
        assert not np.array_equal(np.add.reduce(rows, axis=0), want)
    set_params(ctx, LR.Params())
    out = ctx.lm_step(np.eye(3), np.zeros(3), -1.0, 0, 0, slab=rows)
    got = np.array(out.last_mom)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, f"columns {bad[:8]}: {got[bad[:4]]} != {want[bad[:4]]}"
    assert out.final_cost == want[LR.MOM_Y0]
