"""CPU tests of tests/lm_ref.py, the plain reference the GPU tests of the LM / GN step compare with: it
is pinned to the oracle (oracle.Gicp.align on the golden S2S pair) and to np_gicp, and its restatement of
the device step's moment algebra is pinned to its own per-point evaluation.

Tolerances come from the reference's own precision: every chain / step is run in float64 and in
np.longdouble, and a compared quantity may differ by 16 times the difference between those two runs.
Measured here (x86-64, 80-bit longdouble), relative:
  lm_lambda after whole aligns of the golden pair (5 guesses)
      spread per align 1.3e-16, 1.4e-15, 4.6e-15, 9.9e-16, 8.8e-16; the largest, 4.6e-15, is the spread
      (lm_ref.LAMBDA_SPREAD_REL); oracle vs float64 chain 3.4e-15, 7.0e-16, 5.2e-15, 7.9e-16, 1.4e-15
  rho over the trials of each rejecting step
      spread 1.2e-14, 1.7e-14, 4.1e-14, 5.3e-15, 1.1e-13; moment form vs per-point form 1.2e-14, 1.7e-14,
      3.8e-14, 3.2e-15, 1.1e-13 (the moment form agrees with the longdouble run: the float64 per-point
      sum carries the error)
"""
import numpy as np
import pytest

import lm_ref as LR
import np_gicp as NP
from oracle import oracle as O

LD = np.longdouble
S2S = dict(k_correspondences=10, max_correspondence_distance=1.0, max_iterations=32, transformation_epsilon=5e-4)

# guesses of the aligns (translation sigma, rotation sigma, seed): identity (the golden's own align) and offsets
GUESSES = [None, (0.02, 0.002, 4), (0.1, 0.01, 5), (0.35, 0.03, 6), (0.45, 0.04, 7)]
GUESS_IDS = ["identity", "offset_2cm", "offset_10cm", "offset_35cm", "offset_45cm"]


def _guess(spec):
    if spec is None:
        return None
    dt, dr, seed = spec
    rng = np.random.default_rng(seed)
    g = np.eye(4, dtype=np.float32)
    g[:3, :3] = NP.so3_exp(rng.normal(0, 1, 3) * dr)
    g[:3, 3] = rng.normal(0, 1, 3) * dt
    return g


@pytest.fixture(scope="module")
def golden_oracle(s2s_golden):
    g = s2s_golden
    o = O.Gicp(g["src"], g["tgt"], O.default_params(**S2S))
    o.set_covariances(0, g["cov_src_PLANE"])
    o.set_covariances(1, g["cov_tgt"])
    ca, cb = NP.sym6_to_mat(g["cov_src_PLANE"]), NP.sym6_to_mat(g["cov_tgt"])
    return o, (lambda R, t: LR.pairing_from_oracle(o, g["src"], g["tgt"], ca, cb, R, t))


@pytest.fixture(scope="module")
def aligns(golden_oracle):
    """Every guess once: the oracle's align and the float64, longdouble and float64-with-Eigen's-LDLT chains."""
    o, pairing = golden_oracle
    p = LR.Params(max_iterations=S2S["max_iterations"], transformation_epsilon=S2S["transformation_epsilon"])
    out = []
    for spec in GUESSES:
        guess = _guess(spec)
        opose, ores = o.align(guess)
        out.append((opose, ores, LR.align_chain(pairing, guess, p), LR.align_chain(pairing, guess, p, dt=LD),
                    LR.align_chain(pairing, guess, p, solve=O.ldlt_solve6)))
    return out


def _lam_spread(aligns):
    return max(abs(float(cld[-1].lam) - float(c64[-1].lam)) / float(c64[-1].lam) for _, _, c64, cld, _ in aligns)


@pytest.mark.parametrize("k", range(len(GUESSES)), ids=GUESS_IDS)
def test_chain_of_steps_reproduces_the_oracle_align(s2s_golden, aligns, k):
    """lm_ref steps chained over the oracle's correspondences give the oracle's align: iteration and
    trial counts and the flags exactly, the pose within the project's 1e-6, lm_lambda within 16 x the
    float64 / longdouble spread of the chains' lm_lambda (the largest over the guesses: one align's
    spread alone can fall below an ulp, lambda being lambda_0 / 3^k when every step's factor is clamped)."""
    opose, ores, c64, cld, cll = aligns[k]
    if GUESSES[k] is None:
        assert ores.iterations_run == int(s2s_golden["lm_iters"]) and ores.lm_trials == int(s2s_golden["lm_trials"])
    for c in (c64, cld, cll):
        last = c[-1]
        assert (len(c), last.lm_trials, last.converged, last.lm_failed) == \
            (ores.iterations_run, ores.lm_trials, ores.converged, ores.lm_failed)
        assert last.nr_iterations == ores.nr_iterations
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = last.R, last.t
        np.testing.assert_allclose(pose, opose, atol=1e-6)
    lam = float(c64[-1].lam)
    spread = _lam_spread(aligns)
    err = abs(ores.lm_lambda - lam) / lam
    print(f"lm_lambda {lam:.17g} ({len(c64)} steps): own f64/longdouble spread {abs(float(cld[-1].lam) - lam) / lam:.3g}, "
          f"largest {spread:.3g}; oracle vs chain {err:.3g}, ldlt chain vs chain {abs(float(cll[-1].lam) - lam) / lam:.3g}")
    assert spread > 0
    assert err <= 16 * spread
    assert abs(float(cll[-1].lam) - lam) / lam <= 16 * spread


def test_moments_give_np_gicp_normal_equations(s2s_golden, golden_oracle):
    """The moment builder and the H / b / cost recovered from the 80 doubles against np_gicp's per-point
    linearize on the golden pair (rel 1e-11, the project's figure for moments), at two poses."""
    g = s2s_golden
    _, pairing = golden_oracle
    prob = NP.Problem(g["src"], g["tgt"], NP.sym6_to_mat(g["cov_src_PLANE"]), NP.sym6_to_mat(g["cov_tgt"]),
                      max_corr=S2S["max_correspondence_distance"])
    for T in (np.eye(4), np.block([[NP.so3_exp([0.02, -0.01, 0.03]), np.array([[0.1], [-0.2], [0.05]])],
                                    [np.zeros((1, 3)), np.ones((1, 1))]])):
        Hn, bn, costn = prob.linearize(T)
        a, b, M = pairing(T[:3, :3], T[:3, 3])
        assert len(a) == int(np.sum(prob.corr >= 0))
        mom = LR.moments(a, b, M, T[:3, :3], T[:3, 3])
        H, bb, y0 = LR.normal_equations(mom)
        np.testing.assert_allclose(H, Hn, rtol=1e-11, atol=1e-11 * np.abs(Hn).max())
        np.testing.assert_allclose(bb, bn, rtol=1e-11, atol=1e-11 * np.abs(bn).max())
        assert abs(y0 - costn) <= 1e-11 * abs(costn)
        assert mom[LR.MOM_COUNT] == len(a) and not mom[74:].any()
        # the same moments split into slab rows and summed in the step's order
        rows = LR.moment_rows(a, b, M, T[:3, :3], T[:3, 3], 7)
        np.testing.assert_allclose(LR.reduce_rows(rows), mom, rtol=1e-11, atol=1e-11 * np.abs(mom).max())
        Hl, bl, _ = LR.linearize(a, b, M, T[:3, :3], T[:3, 3])
        np.testing.assert_allclose(Hl, Hn, rtol=1e-11, atol=1e-11 * np.abs(Hn).max())
        np.testing.assert_allclose(bl, bn, rtol=1e-11, atol=1e-11 * np.abs(bn).max())


@pytest.mark.parametrize("case", LR.REJECTING, ids=lambda c: f"s{c[0]:g}_th{c[1]:g}")
def test_moment_form_of_rho_matches_reevaluation(case):
    """The gain ratio from the 74 moments (what the device evaluates) against the reference's own, which
    re-evaluates the error over the points, on every trial of the rejecting steps: within 16 x the
    float64 / longdouble spread of the per-point rho over the step's trials (a single trial's spread can
    be zero by chance; the step's trials share H, b and y0, so their largest spread is the scale)."""
    a, b, M, R, t, lam, it, ntr = LR.rejecting_step(*case)
    p = LR.Params()
    s64 = LR.step(a, b, M, R, t, lam, p, it=it, lm_trials=ntr)
    sld = LR.step(a, b, M, R, t, lam, p, it=it, lm_trials=ntr, dt=LD)
    assert s64.kind == sld.kind == "accepted" and s64.trials_used == sld.trials_used >= 8
    assert min(abs(float(x[1])) for x in s64.trials) >= 0.01
    mom = LR.moments(a, b, M, R, t)
    spread = max(abs(float(xl[1]) - float(x[1])) / abs(float(x[1])) for x, xl in zip(s64.trials, sld.trials))
    errs = []
    for lam_i, rho, _ in s64.trials:
        d = np.linalg.solve(s64.H + lam_i * np.eye(6), -s64.b)
        errs.append(abs(LR.moment_rho(mom, d, lam_i) - rho) / abs(rho))
    print(f"rho spread {spread:.3g}, moment form vs per-point {max(errs):.3g}")
    assert spread > 0 and max(errs) <= 16 * spread


def test_reduce_rows_order_is_observable():
    """The restated summation order differs from a plain row-by-row sum in the last bits on the rows the
    GPU test uses, and equals it where no rounding occurs."""
    rows = LR.slab_rows(25, 3)
    assert not np.array_equal(LR.reduce_rows(rows), np.add.reduce(rows, axis=0))
    ints = np.arange(13 * 80, dtype=np.float64).reshape(13, 80)
    np.testing.assert_array_equal(LR.reduce_rows(ints), ints.sum(axis=0))


def test_ldlt_restatement_is_the_oracles_bit_for_bit():
    """lm_ref.ldlt_solve6 (plain Python, with the tie rule as a switch) against oracle.ldlt_solve6 on
    well-conditioned, tied and rank-deficient systems: the same bits.  With the last-largest tie rule it
    gives other bits on a tied system."""
    rng = np.random.default_rng(11)
    differs = 0
    for k in range(60):
        B = rng.standard_normal((6, 6))
        A = B @ B.T + 0.1 * np.eye(6)
        if k % 3 == 1:      # a three-way tie on the diagonal
            A[3, 3] = A[4, 4] = A[5, 5] = np.abs(np.diag(A)).max() * (0.5 if k % 2 else 2.0)
        if k % 3 == 2:      # an exactly zero row and column, and a tie
            A[k % 6, :] = 0
            A[:, k % 6] = 0
            A[(k + 1) % 6, (k + 1) % 6] = A[(k + 2) % 6, (k + 2) % 6]
        rhs = rng.standard_normal(6)
        want = O.ldlt_solve6(A, rhs)
        np.testing.assert_array_equal(LR.ldlt_solve6(A, rhs), want)
        differs += int((LR.ldlt_solve6(A, rhs, first_largest=False) != want).any())
    assert differs >= 10
