"""Sequence-independent reference of the regularised covariances — TEST HELPER ONLY.

calculate_covariances (reference nano_gicp_impl.hpp:392-437) restated in
np.longdouble from the points and a neighbour list: mean, biased covariance
(divided by k) and its eigen-decomposition.  The decomposition is this file's
own: LAPACK's float64 eigh as a starting basis, re-orthonormalised and polished
by full-matrix Jacobi rotations in extended precision.  It shares no operation
sequence with oracle/cpu_ref.cpp sym_eig3 or the device's.

What a regularisation gives on a rank-deficient covariance depends on the
rounding noise of the SVD that computed it: a null eigenvalue comes out with
either sign and the vectors inside the null space are arbitrary.  The
"envelope" below is what holds under ANY correct SVD:

  NONE        the covariance itself.
  FROBENIUS   ||(C + 1e-3 I)^-1||_F (C + 1e-3 I), the norm from the eigenvalues.
  JacobiSVD routes (MIN_EIG, NORMALIZED_MIN_EIG, PLANE), with the output R
  taken to the eigenbasis, B = V^T R V, and the eigenvalues grouped in clusters
  (the null eigenvalues are one cluster; every resolved eigenvalue is its own,
  except that under PLANE resolved eigenvalues within a relative 1e-3 of each
  other share one, see `left_out`):
    - an entry of B between two clusters is zero;
    - a resolved cluster's block has the eigenvalues the method assigns to its
      positions, f(lambda_i): its own diagonal entry for a single eigenvalue;
    - the null block's eigenvalues have the absolute values the method assigns
      to the trailing singular values (PLANE: the tail of (1, 1, 1e-3);
      MIN_EIG and NORMALIZED_MIN_EIG: 1e-3), their signs are free.
  NORMALIZED_MIN_EIG on a covariance that is exactly zero: all entries NaN
  (the reference's clamp is `a < 1e-3 ? 1e-3 : a`, which keeps the NaN of
  0 / 0).  Everything else is finite.

Deviations are relative to max(lambda_max, 1).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LD = np.longdouble
REGS = ("NONE", "MIN_EIG", "NORMALIZED_MIN_EIG", "PLANE", "FROBENIUS")
SVD_REGS = ("MIN_EIG", "NORMALIZED_MIN_EIG", "PLANE")
CLAMP = 1e-3                 # the double constant of the reference
NULL_BELOW = 1e-12           # an eigenvalue is null below this share of lambda_max ...
RESOLVED_ABOVE = 1e-8        # ... and resolved above this one; nothing may lie between
PLANE_CLUSTER_REL = 1e-3     # PLANE: resolved eigenvalues this close are not told apart

# The oracle's largest deviation from the envelope over every case and k of
# tests/cov_cases.py, per regularisation (measured by tests/test_cov_cases_cpu.py
# test_oracle_inside_envelope, which prints them and holds the oracle to 2x;
# the GPU tests allow 16x, the suite's margin for a second fp64 implementation
# of the same formula, which covers the device's 3x3 adjugate against the
# oracle's 4x4 inverse under FROBENIUS).
#
# FROBENIUS is ten orders above the rest.  On a rank-deficient covariance
# C + 1e-3 I has condition lambda_max / 1e-3 (6e5 on line_generic at k = 64,
# which sets the figure), the result is 1e3 lambda_max in size, and two
# cofactor inverses in a row lose about condition^2 x 2^-53 of it.
ORACLE_DEV = {
    "NONE": 7.7e-16,                 # measured 7.63e-16 (line_generic, k = 64)
    "MIN_EIG": 9.8e-15,              # measured 9.76e-15 (lattice, k = 20)
    "NORMALIZED_MIN_EIG": 6.5e-15,   # measured 6.41e-15 (lattice, k = 20)
    "PLANE": 7.4e-15,                # measured 7.34e-15 (generic, k = 3)
    "FROBENIUS": 2.1e-4,             # measured 2.08e-4 (line_generic, k = 64)
}
CPU_MARGIN, GPU_MARGIN = 2, 16


def sym6_to_mat(c6):
    c6 = np.asarray(c6)
    return c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def _mm(a, b):
    return np.einsum("nij,njk->nik", a, b)


def _t(a):
    return np.transpose(a, (0, 2, 1))


def jacobi_ld(A, V=None, sweeps=40):
    """Eigenvalues (descending) and vectors (columns) of a batch (n, m, m) of symmetric longdouble matrices:
    whole-matrix rotations B <- G^T B G over the pairs (m-2, m-1), ..., (0, 1) until no off-diagonal entry is
    above 2^-62 of the diagonal's size."""
    B = np.array(A, LD)
    n, m, _ = B.shape
    V = np.broadcast_to(np.eye(m, dtype=LD), B.shape).copy() if V is None else np.array(V, LD)
    pairs = [(p, q) for q in range(m - 1, 0, -1) for p in range(q - 1, -1, -1)]
    diag = np.arange(m)
    for _ in range(sweeps):
        size = np.abs(B[:, diag, diag]).sum(1)
        off = sum((np.abs(B[:, p, q]) for p, q in pairs), np.zeros(n, LD))
        if np.all(off <= size * LD(2.0) ** -62):
            break
        for p, q in pairs:
            apq = B[:, p, q]
            live = apq != 0
            den = np.where(live, 2 * apq, LD(1))
            theta = (B[:, q, q] - B[:, p, p]) / den
            t = np.where(theta >= 0, LD(1), LD(-1)) / (np.abs(theta) + np.sqrt(theta * theta + 1))
            t = np.where(live, t, LD(0))
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            G = np.broadcast_to(np.eye(m, dtype=LD), B.shape).copy()
            G[:, p, p] = c
            G[:, q, q] = c
            G[:, p, q] = s
            G[:, q, p] = -s
            B = _mm(_t(G), _mm(B, G))
            B = (B + _t(B)) / 2
            V = _mm(V, G)
    lam = B[:, diag, diag]
    order = np.argsort(-lam, axis=1, kind="stable")
    lam = np.take_along_axis(lam, order, 1)
    V = np.take_along_axis(V, order[:, None, :], 2)
    return lam, V


def eigh_ld(C):
    """Eigen-decomposition of (n, 3, 3) symmetric longdouble matrices, eigenvalues descending."""
    C = np.asarray(C, LD)
    size = np.abs(C).max(axis=(1, 2))
    A = (C / np.where(size > 0, size, LD(1))[:, None, None]).astype(np.float64)
    _, V0 = np.linalg.eigh(A)
    V0 = V0.astype(LD)
    # float64-orthonormal to 1e-16: one Newton step of the polar iteration takes that to its square
    V0 = _mm(V0, (3 * np.eye(3, dtype=LD) - _mm(_t(V0), V0)) / 2)
    B = _mm(_t(V0), _mm(C, V0))
    lam, W = jacobi_ld((B + _t(B)) / 2)
    return lam, _mm(V0, W)


@dataclass
class Ref:
    k: int
    C: np.ndarray          # (n, 3, 3) longdouble
    lam: np.ndarray        # (n, 3) descending
    V: np.ndarray          # (n, 3, 3) eigenvectors in columns
    lmax: np.ndarray       # (n,)
    scale: np.ndarray      # (n,) max(lambda_max, 1)
    null: np.ndarray       # (n, 3) bool
    zero: np.ndarray       # (n,) bool: the covariance is exactly zero
    rank: np.ndarray       # (n,)
    gap_ok: np.ndarray     # (n,) bool: no eigenvalue between NULL_BELOW and RESOLVED_ABOVE of lambda_max


def covariance_ld(pts, idx, ddof=0):
    P = np.asarray(pts, np.float32).astype(LD)[np.asarray(idx)]
    k = P.shape[1]
    mean = P.sum(axis=1) / LD(k)
    D = P - mean[:, None, :]
    return np.einsum("nki,nkj->nij", D, D) / LD(k - ddof)


def build(pts, idx, ddof=0):
    """The reference of a cloud under the neighbour lists idx (n, k).  ddof = 1 is the (k - 1) mutant."""
    C = covariance_ld(pts, idx, ddof)
    lam, V = eigh_ld(C)
    lmax = lam[:, 0]
    zero = np.all(C == 0, axis=(1, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(lmax[:, None] > 0, lam / np.where(lmax > 0, lmax, LD(1))[:, None], LD(0))
    null = share < NULL_BELOW
    gap_ok = np.all(null | (share > RESOLVED_ABOVE), axis=1)
    return Ref(idx.shape[1], C, lam, V, lmax, np.maximum(lmax, LD(1)), null, zero, (~null).sum(1), gap_ok)


def assigned_values(ref, reg, variant=None):
    """(n, 3) values the method gives the singular values in descending order.  variant: a mutant of the
    restatement (tests only)."""
    n = len(ref.lam)
    clamp = LD(1e-4 if variant == "clamp_1e-4" else CLAMP)
    sv = np.where(ref.null, LD(0), ref.lam)
    if reg == "PLANE":
        vals = (1.0, CLAMP, 1.0) if variant == "plane_order" else (1.0, 1.0, CLAMP)
        return np.broadcast_to(np.array(vals, LD), (n, 3)).copy()
    if reg == "MIN_EIG":
        return np.where(sv < clamp, clamp, sv)
    if reg == "NORMALIZED_MIN_EIG":
        with np.errstate(invalid="ignore", divide="ignore"):
            r = sv / (sv[:, 2:3] if variant == "normalise_by_smallest" else sv[:, 0:1])
            if variant == "fmax_clamp":
                return np.fmax(r, clamp)
            return np.where(r < clamp, clamp, r)       # keeps the NaN of 0 / 0
    raise ValueError(reg)


@dataclass
class Verdict:
    dev: np.ndarray        # (n,) deviation from the envelope / max(lambda_max, 1); 0 where NaN is expected
    want_nan: np.ndarray   # (n,) bool: all six entries must be NaN
    nan_ok: np.ndarray     # (n,) bool: the row's NaN / finite pattern is the expected one
    left_out: np.ndarray   # (n,) bool: PLANE rows with close resolved eigenvalues (held to the cluster envelope)


def _clusters(ref, reg):
    """(n, 3) cluster label per eigenvalue: 3 = null; resolved eigenvalues their own index, merged under PLANE."""
    n = len(ref.lam)
    lab = np.tile(np.arange(3), (n, 1))
    left = np.zeros(n, bool)
    if reg == "PLANE":
        for i in (0, 1):
            close = ~ref.null[:, i] & ~ref.null[:, i + 1] & \
                (ref.lam[:, i] - ref.lam[:, i + 1] <= PLANE_CLUSTER_REL * ref.lam[:, i])
            lab[close, i + 1] = lab[close, i]
            left |= close
    lab[ref.null] = 3
    return lab, left


def check(ref, cov6, reg, variant=None):
    """Hold cov6 (n, 6 float64: xx xy xz yy yz zz) to the envelope of `reg`."""
    R = sym6_to_mat(np.asarray(cov6, np.float64))
    n = len(R)
    got_nan = np.isnan(R).all(axis=(1, 2))
    finite = np.isfinite(R).all(axis=(1, 2))
    want_nan = np.zeros(n, bool)
    left = np.zeros(n, bool)
    Rl = R.astype(LD)
    if reg == "NONE":
        dev = np.abs(Rl - ref.C).max(axis=(1, 2))
    elif reg == "FROBENIUS":
        Cl = ref.C + LD(CLAMP) * np.eye(3, dtype=LD)
        nrm = np.sqrt((1 / (ref.lam + LD(CLAMP)) ** 2).sum(1))
        dev = np.abs(Rl - nrm[:, None, None] * Cl).max(axis=(1, 2))
    else:
        f = assigned_values(ref, reg, variant)
        want_nan = np.isnan(f).any(1)
        f = np.where(want_nan[:, None], LD(0), f)
        Rl = np.where(want_nan[:, None, None], LD(0), Rl)
        B = _mm(_t(ref.V), _mm(Rl, ref.V))
        lab, left = _clusters(ref, reg)
        dev = np.zeros(n, LD)
        pats, inv = np.unique(lab, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for pi, pat in enumerate(pats):
            rows = np.flatnonzero(inv == pi)
            Bp, fp = B[rows], f[rows]
            d = np.zeros(len(rows), LD)
            for i in range(3):
                for j in range(i + 1, 3):
                    if pat[i] != pat[j]:
                        d = np.maximum(d, np.maximum(np.abs(Bp[:, i, j]), np.abs(Bp[:, j, i])))
            for c in np.unique(pat):
                pos = np.flatnonzero(pat == c)
                blk = Bp[:, pos][:, :, pos]
                d = np.maximum(d, np.abs(blk - _t(blk)).max(axis=(1, 2)))
                ev = blk[:, 0, :1] if len(pos) == 1 else jacobi_ld((blk + _t(blk)) / 2)[0]
                want = -np.sort(-fp[:, pos], axis=1)
                if c == 3:
                    ev = -np.sort(-np.abs(ev), axis=1)
                d = np.maximum(d, np.abs(ev - want).max(1))
            dev[rows] = d
    dev = np.where(want_nan, LD(0), dev / ref.scale)
    nan_ok = np.where(want_nan, got_nan, finite)
    return Verdict(dev.astype(np.float64), want_nan, nan_ok, left)


# ---------------------------------------------------------------------------
# the catalogue's references, computed once per (case, k) and shared
# ---------------------------------------------------------------------------
_CACHE = {}


def case_knn(name, k):
    """The oracle's (idx, sqd) of every point of a catalogue cloud among the cloud, k + 1 neighbours."""
    import cov_cases as CC
    from oracle import oracle as O
    key = ("knn", name, k)
    if key not in _CACHE:
        pts = CC.cloud(name)
        _CACHE[key] = O.knn(pts, pts, min(k + 1, len(pts)))
    return _CACHE[key]


def case_ref(name, k, ddof=0):
    """The reference of a catalogue case under the oracle's neighbour lists."""
    import cov_cases as CC
    key = ("ref", name, k, ddof)
    if key not in _CACHE:
        _CACHE[key] = build(CC.cloud(name), case_knn(name, k)[0][:, :k], ddof)
    return _CACHE[key]


def case_oracle(name, k, reg):
    """The oracle's covariances of a catalogue case (read-only)."""
    import cov_cases as CC
    from oracle import oracle as O
    key = ("cov", name, k, reg)
    if key not in _CACHE:
        c = O.covariances(CC.cloud(name), k, reg)
        c.setflags(write=False)
        _CACHE[key] = c
    return _CACHE[key]
