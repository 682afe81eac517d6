"""Plain reference of ONE LM / GN step of LsqRegistration — TEST HELPER ONLY.

The step is computed from the points (a_i, b_i, M_i with a given pairing
i -> i), not from moments: H, b and y0 as np_gicp.Problem.linearize, then the
reference's sequential trial loop (lsq_registration_impl.hpp:155-232), which
re-evaluates the error over the points at every trial.  Everything is written
for a dtype dt, float64 or np.longdouble; the difference between the two runs
is the reference's own precision spread, which the tests turn into tolerances.

Also here: the 80 moment doubles of the device's step (DESIGN.md
"Normal-equation moments") built from the same points, H / b / rho recovered
from them with plain matrix algebra, and the fixed summation order of the
step's slab reduction.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

GN, LM = 0, 1
STRIDE = 80          # doubles per slab row
MOM_Y0, MOM_COUNT = 72, 73
PARTS = 12           # slab row partitions of the device's reduction


@dataclass
class Params:
    optimizer: int = LM
    lm_max_iterations: int = 10
    lm_init_lambda_factor: float = 1e-9
    transformation_epsilon: float = 5e-4
    rotation_epsilon: float = 2e-3
    max_iterations: int = 64
    fixed_iterations: int = 0


@dataclass
class Step:
    kind: str                 # accepted / rejected_converged / failed / gn
    trials_used: int          # compute_error evaluations of this step
    trials: list              # per trial (lambda, rho, is_converged)
    lam_trial: float          # lambda of the deciding trial, before the update
    factor: float             # the accepted trial's update factor max(1/3, 1 - (2 rho - 1)^3), else 1
    lam: float                # lm_lambda_ after the step
    R: np.ndarray
    t: np.ndarray
    H: np.ndarray
    b: np.ndarray
    y0: float
    iter: int
    nr_iterations: int
    lm_trials: int
    converged: int
    lm_failed: int
    done: int
    num_corr: int
    d: np.ndarray = field(default=None)


def so3_exp(w, dt=np.float64):
    """Sophus SO3::exp (gicp/so3.hpp:101-124) as a rotation matrix, in dtype dt."""
    w = np.asarray(w, dt)
    th2 = w @ w
    if th2 < 1e-10:
        imag = dt(0.5) - th2 / dt(48) + th2 * th2 / dt(3840)
        real = dt(1) - th2 / dt(8) + th2 * th2 / dt(384)
    else:
        th = np.sqrt(th2)
        imag = np.sin(dt(0.5) * th) / th
        real = np.cos(dt(0.5) * th)
    x, y, z = imag * w
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * real), 2 * (x * z + y * real)],
                     [2 * (x * y + z * real), 1 - 2 * (x * x + z * z), 2 * (y * z - x * real)],
                     [2 * (x * z - y * real), 2 * (y * z + x * real), 1 - 2 * (x * x + y * y)]], dtype=dt)


def skew(v):
    z = np.zeros(len(v), v.dtype)
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], -1),
                     np.stack([v[:, 2], z, -v[:, 0]], -1),
                     np.stack([-v[:, 1], v[:, 0], z], -1)], 1)


def solve_ge(A, rhs):
    """Gaussian elimination with partial pivoting in the dtype of A (np.linalg has no longdouble)."""
    A = A.copy()
    x = rhs.copy()
    n = len(x)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            x[[k, p]] = x[[p, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]
            x[i] -= f * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def _errors(a, b, R, t):
    q = a @ R.T + t
    return q, b - q


def linearize(a, b, M, R, t, dt=np.float64):
    """H = sum J^T M J, b = sum J^T M e, y0 = sum e^T M e, J = [skew(R a + t) | -I] (nano_gicp_impl.hpp:277-336)."""
    a, b, M, R, t = (np.asarray(x, dt) for x in (a, b, M, R, t))
    if len(a) == 0:
        return np.zeros((6, 6), dt), np.zeros(6, dt), dt(0)
    q, e = _errors(a, b, R, t)
    J = np.concatenate([skew(q), -np.broadcast_to(np.eye(3, dtype=dt), (len(q), 3, 3))], axis=2)
    MJ = M @ J
    H = np.einsum("nki,nkj->ij", J, MJ)
    g = np.einsum("nki,nk->i", MJ, e)
    return H, g, np.einsum("ni,nij,nj->", e, M, e)


def cost(a, b, M, R, t, dt=np.float64):
    a, b, M, R, t = (np.asarray(x, dt) for x in (a, b, M, R, t))
    if len(a) == 0:
        return dt(0)
    _, e = _errors(a, b, R, t)
    return np.einsum("ni,nij,nj->", e, M, e)


def is_converged(D, td, p: Params):
    """lsq_registration_impl.hpp:128-139 (never with fixed_iterations)."""
    if p.fixed_iterations > 0:
        return False
    dt = D.dtype.type
    mr = np.abs(D - np.eye(3, dtype=D.dtype)).max()
    mt = np.abs(td).max()
    return bool(max(dt(1) / dt(p.rotation_epsilon) * mr, dt(1) / dt(p.transformation_epsilon) * mt) < 1)


def step(a, b, M, R, t, lam_pre, p: Params, it=0, lm_trials=0, solve=None, dt=np.float64) -> Step:
    """One step_lm / step_gn followed by computeTransformation's bookkeeping of that iteration.
    solve(A, rhs) is the 6x6 solve (float64: np.linalg.solve or oracle.ldlt_solve6); None = solve_ge in dt."""
    if solve is None:
        solve = solve_ge if dt is not np.float64 else np.linalg.solve
    R = np.asarray(R, dt)
    t = np.asarray(t, dt)
    H, g, y0 = linearize(a, b, M, R, t, dt)
    I6 = np.eye(6, dtype=dt)
    max_it = p.fixed_iterations if p.fixed_iterations > 0 else p.max_iterations
    out = dict(H=H, b=g, y0=y0, iter=it + 1, nr_iterations=it, num_corr=len(a), lm_failed=0, factor=dt(1))

    def delta(d):
        return so3_exp(d[:3], dt), d[3:]

    if p.optimizer == GN:
        d = np.asarray(solve(H, -g), dt)
        D, td = delta(d)
        conv = is_converged(D, td, p)
        return Step(kind="gn", trials_used=1, trials=[(dt(0), dt(1), conv)], lam_trial=dt(0), lam=dt(lam_pre),
                    R=D @ R, t=D @ t + td, lm_trials=lm_trials, converged=int(conv),
                    done=int(conv or it + 1 >= max_it), d=d, **out)
    lam = dt(lam_pre)
    if lam < 0:
        lam = dt(p.lm_init_lambda_factor) * np.abs(np.diag(H)).max()
    nu = dt(2)
    trials = []
    for i in range(p.lm_max_iterations):
        d = np.asarray(solve(H + lam * I6, -g), dt)
        D, td = delta(d)
        Rn, tn = D @ R, D @ t + td
        yi = cost(a, b, M, Rn, tn, dt)
        with np.errstate(invalid="ignore", divide="ignore"):
            rho = (y0 - yi) / (d @ (lam * d - g))
        conv = is_converged(D, td, p)
        trials.append((lam, rho, conv))
        if rho < 0:
            if conv:
                return Step(kind="rejected_converged", trials_used=i + 1, trials=trials, lam_trial=lam, lam=lam, R=R,
                            t=t, lm_trials=lm_trials + i + 1, converged=1, done=1, d=d, **out)
            lam = nu * lam
            nu = 2 * nu
            continue
        c = 2 * rho - 1
        f = max(dt(1) / dt(3), 1 - c * c * c)   # (std::max(a, b) keeps a when b is NaN)
        out["factor"] = f
        return Step(kind="accepted", trials_used=i + 1, trials=trials, lam_trial=lam, lam=lam * f, R=Rn, t=tn,
                    lm_trials=lm_trials + i + 1, converged=int(conv), done=int(conv or it + 1 >= max_it), d=d, **out)
    out["lm_failed"] = 1
    return Step(kind="failed", trials_used=p.lm_max_iterations, trials=trials, lam_trial=trials[-1][0], lam=lam, R=R,
                t=t, lm_trials=lm_trials + p.lm_max_iterations, converged=0, done=1, **out)


# ---- the device step's moments ---------------------------------------------------------------------------
def mom_ab(a, b):
    """Symmetric 3 x 3 (a, b) -> 0..5: xx, xy, xz, yy, yz, zz."""
    a, b = min(a, b), max(a, b)
    return b if a == 0 else (2 + b if a == 1 else 5)


def mom_w(k, l, a, b):
    """Slot of the (a, b) entry of W(k, l) = sum M qt_k qt_l, qt = [q; 1]."""
    if k == 3 and l == 3:
        return mom_ab(a, b)
    if k == 3 or l == 3:
        return 6 + 6 * min(k, l) + mom_ab(a, b)
    return 24 + 6 * mom_ab(k, l) + mom_ab(a, b)


def mom_g(m, k):
    """Slot of G(m, k) = sum (M e)_m qt_k."""
    return 60 + 4 * m + k


def moments(a, b, M, R, t, dt=np.float64):
    """The 80 moment doubles of the pairing a_i -> b_i at pose (R, t): q = R a + t, e = b - q."""
    a, b, M, R, t = (np.asarray(x, dt) for x in (a, b, M, R, t))
    mom = np.zeros(STRIDE, dt)
    if len(a) == 0:
        return mom
    q, e = _errors(a, b, R, t)
    qt = np.concatenate([q, np.ones((len(q), 1), dt)], axis=1)
    Me = np.einsum("nij,nj->ni", M, e)
    for k in range(4):
        for l in range(k, 4):
            Wkl = np.einsum("nij,n->ij", M, qt[:, k] * qt[:, l])
            for i in range(3):
                for j in range(i, 3):
                    mom[mom_w(k, l, i, j)] = Wkl[i, j]
    for m in range(3):
        for k in range(4):
            mom[mom_g(m, k)] = Me[:, m] @ qt[:, k]
    mom[MOM_Y0] = np.einsum("ni,ni->", e, Me)
    mom[MOM_COUNT] = len(a)
    return mom


def moment_rows(a, b, M, R, t, nrows):
    """The moments split into nrows slab rows (point i in row i % nrows), as the moment kernel's blocks would."""
    rows = np.zeros((nrows, STRIDE))
    idx = np.arange(len(a))
    for r in range(nrows):
        s = idx % nrows == r
        rows[r] = moments(a[s], b[s], M[s], R, t)
    return rows


def reduce_rows(rows):
    """The step's fixed summation order: partition p adds rows p, p + 12, ... in order from 0.0, then the
    12 partials are added 0..11 from 0.0."""
    rows = np.asarray(rows, np.float64).reshape(-1, STRIDE)
    out = np.zeros(STRIDE)
    for p in range(PARTS):
        s = np.zeros(STRIDE)
        for r in range(p, len(rows), PARTS):
            s = s + rows[r]
        out = out + s
    return out


# generators of skew(q) = sum_c q_c S_c
_S = np.zeros((3, 3, 3))
_S[0, 1, 2], _S[0, 2, 1] = -1, 1
_S[1, 0, 2], _S[1, 2, 0] = 1, -1
_S[2, 0, 1], _S[2, 1, 0] = -1, 1


def _W(mom, k, l):
    return np.array([[mom[mom_w(k, l, i, j)] for j in range(3)] for i in range(3)], dtype=mom.dtype)


def _G(mom, k):
    return np.array([mom[mom_g(m, k)] for m in range(3)], dtype=mom.dtype)


def normal_equations(mom):
    """H, b, y0 from the moments: J = [sum_c q_c S_c | -I]."""
    dt = mom.dtype
    S = _S.astype(dt)
    H = np.zeros((6, 6), dt)
    g = np.zeros(6, dt)
    for c in range(3):
        for d in range(3):
            H[:3, :3] += S[c].T @ _W(mom, c, d) @ S[d]
        H[:3, 3:] -= S[c].T @ _W(mom, c, 3)
        g[:3] += S[c].T @ _G(mom, c)
    H[3:, :3] = H[:3, 3:].T
    H[3:, 3:] = _W(mom, 3, 3)
    g[3:] = -_G(mom, 3)
    return H, g, mom[MOM_Y0]


def moment_rho(mom, d, lam):
    """The gain ratio of step d from the moments alone: with the correspondences frozen e' = e - D qt,
    D = [so3_exp(d_r) - I | d_t], so y0 - y(d) = 2 <G, D> - sum_kl D_k^T W(k,l) D_l."""
    dt = mom.dtype.type
    d = np.asarray(d, mom.dtype)
    _, g, _ = normal_equations(mom)
    D = np.concatenate([so3_exp(d[:3], dt) - np.eye(3, dtype=mom.dtype), d[3:, None]], axis=1)   # 3 x 4
    lin = sum(_G(mom, k) @ D[:, k] for k in range(4))
    quad = sum(D[:, k] @ _W(mom, k, l) @ D[:, l] for k in range(4) for l in range(4))
    return (2 * lin - quad) / (d @ (dt(lam) * d - g))


# ---- chains ------------------------------------------------------------------------------------------------
def pairing_from_oracle(o, src, tgt, cov_src, cov_tgt, R, t):
    """The frozen problem of one outer iteration of a real align: correspondences from the oracle's
    linearize at the pose (an oracle.Gicp with covariances set), M = (C_B + R C_A R^T)^-1
    (nano_gicp_impl.hpp:234-275).  cov_*: (n, 3, 3) float64."""
    T = np.eye(4)
    T[:3, :3] = np.asarray(R, np.float64)
    T[:3, 3] = np.asarray(t, np.float64)
    corr = o.linearize(T)[3]
    ok = corr >= 0
    M = np.linalg.inv(cov_tgt[corr[ok]] + T[:3, :3] @ cov_src[ok] @ T[:3, :3].T)
    return src[ok].astype(np.float64), tgt[corr[ok]].astype(np.float64), M


def align_chain(pairing, guess, p: Params, dt=np.float64, solve=None):
    """computeTransformation (lsq_registration_impl.hpp:95-126) as a chain of step()s; pairing(R, t) gives
    each outer iteration's (a, b, M).  Returns the steps."""
    g = np.eye(4) if guess is None else np.asarray(guess, np.float32).astype(np.float64)
    R, t, lam, it, ntr = np.asarray(g[:3, :3], dt), np.asarray(g[:3, 3], dt), dt(-1), 0, 0
    steps = []
    max_it = p.fixed_iterations if p.fixed_iterations > 0 else p.max_iterations
    while it < max_it:
        a, b, M = pairing(R, t)
        s = step(a, b, M, R, t, lam, p, it=it, lm_trials=ntr, solve=solve, dt=dt)
        steps.append(s)
        R, t, lam, it, ntr = s.R, s.t, s.lam, s.iter, s.lm_trials
        if s.done:
            break
    return steps


# float64 / longdouble spread of lm_lambda after whole aligns of the golden S2S pair, relative: the
# largest of the five aligns of tests/test_lm_ref_cpu.py (4.55e-15, its docstring), rounded up.  The GPU
# aligns compared with the live oracle allow 16 times this.
LAMBDA_SPREAD_REL = 4.6e-15


# ---- the issue's problems ----------------------------------------------------------------------------------
# (s, theta, seed): LM rejects 7 or 8 trials in a row early in the align from identity.  The seeds are
# chosen on the CPU so that every trial's |rho| >= 0.01 and cond(H + lambda I) <= 1e8 (the GPU test
# asserts both before it runs a case); (3, 1, 67) and (10, 3, 8) also reject again at a later step.
REJECTING = [(3.0, 1.0, 67), (5.0, 2.0, 2), (8.0, 0.5, 1), (3.0, 2.8, 1), (10.0, 3.0, 8)]
CONTROL = (1.0, 0.3, 1)   # never rejects


def make_problem(s, theta, seed, n=40):
    """n source points a ~ N(0, diag(4, 4, 1)), target b = s R(theta axis) a + 0.05 noise, random SPD M_i with
    eigenvalues in [0.2, 5], pairing i -> i."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, 3)) * np.array([2.0, 2.0, 1.0])
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    b = s * a @ so3_exp(theta * axis).T + 0.05 * rng.standard_normal((n, 3))
    M = np.empty((n, 3, 3))
    for i in range(n):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        M[i] = Q @ np.diag(rng.uniform(0.2, 5.0, 3)) @ Q.T
        M[i] = 0.5 * (M[i] + M[i].T)
    return a, b, M


def rejecting_step(s, theta, seed, min_trials=8):
    """The first step of the align from identity (reference parameters) that needs at least min_trials
    trials: (a, b, M, R, t, lambda before the step, iter, lm_trials).  For (3, 2.8) and (10, 3) it is not
    the first step, so the pose is not the identity and lambda is carried."""
    a, b, M = make_problem(s, theta, seed)
    p = Params()
    R, t, lam, it, ntr = np.eye(3), np.zeros(3), -1.0, 0, 0
    for _ in range(8):
        st = step(a, b, M, R, t, lam, p, it=it, lm_trials=ntr)
        if st.trials_used >= min_trials:
            return a, b, M, R, t, lam, it, ntr
        R, t, lam, it, ntr = st.R, st.t, float(st.lam), st.iter, st.lm_trials
    raise AssertionError(f"no step of ({s}, {theta}, seed {seed}) needs {min_trials} trials")


def slab_rows(nrows, seed):
    """Slab rows whose magnitudes spread over 1e-8 .. 1e8 with mixed signs: their sum depends on the order."""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], (nrows, STRIDE)) * 10.0 ** rng.uniform(-8, 8, (nrows, STRIDE))


def ldlt_solve6(A, rhs, first_largest=True):
    """Eigen::LDLT<Matrix6d>(A).solve(rhs) in plain Python floats: pivoted (the largest |diagonal| entry,
    the FIRST of equal ones), lower storage, left-looking, zero pivots skipped and their solution entries
    set to 0.  Bit for bit oracle.ldlt_solve6 (tests/test_lm_ref_cpu.py); first_largest=False takes the
    last of equal diagonal entries instead, the wrong tie rule, to show that a test can tell the two."""
    n = 6
    m = [[float(A[i][j]) for j in range(n)] for i in range(n)]
    tr = [0] * n
    for k in range(n):
        big, bigv = k, abs(m[k][k])
        for i in range(k + 1, n):
            if abs(m[i][i]) > bigv or (not first_largest and abs(m[i][i]) == bigv):
                big, bigv = i, abs(m[i][i])
        tr[k] = big
        if k != big:
            for j in range(k):
                m[k][j], m[big][j] = m[big][j], m[k][j]
            for i in range(big + 1, n):
                m[i][k], m[i][big] = m[i][big], m[i][k]
            m[k][k], m[big][big] = m[big][big], m[k][k]
            for i in range(k + 1, big):
                m[i][k], m[big][i] = m[big][i], m[i][k]
        if k > 0:
            temp = [m[j][j] * m[k][j] for j in range(k)]
            s = 0.0
            for j in range(k):
                s += m[k][j] * temp[j]
            m[k][k] -= s
            for i in range(k + 1, n):
                acc = 0.0
                for j in range(k):
                    acc += m[i][j] * temp[j]
                m[i][k] -= acc
        if k < n - 1 and abs(m[k][k]) > 0.0:
            for i in range(k + 1, n):
                m[i][k] /= m[k][k]
    y = [float(v) for v in rhs]
    for k in range(n):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    for i in range(n):
        for j in range(i):
            y[i] -= m[i][j] * y[j]
    tiny = float(np.finfo(np.float64).tiny)
    for i in range(n):
        y[i] = y[i] / m[i][i] if abs(m[i][i]) > tiny else 0.0
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            y[i] -= m[j][i] * y[j]
    for k in range(n - 1, -1, -1):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    return np.array(y)
