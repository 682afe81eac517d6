"""Per-point covariances on the catalogue of tests/cov_cases.py: rank 0, 1, 2
and 3 neighbourhoods, duplicates, a far and a tiny cloud and a tied lattice,
every k of the catalogue x the five regularisations, through every device path
that computes mean, covariance and regularize() (cov_math.hpp):

  default   k_covariances2<10|20> at k = 10, 20, k_covariances<16|32|64> else
  tasks     OPT_COV_TASKS = 1: the select step of knn_tasks.hip (k <= 32); on
            clouds this small it finishes every group, so its one-lane
            k_covariances<10|20> fallback is launched but has nothing to do
  lazy0/1   OPT_TIE_LAZY = 0 / 1: the tie resolvers of nftree.hip on the whole
            and on the partial tree (they recompute every tied query)
  morton    OPT_TIE_ORDER = 0: ties by Morton position, no resolver

Asserted per row (tolerances: tests/cov_ref.py, measured on the oracle in
tests/test_cov_cases_cpu.py; the device is allowed 16 x the constants):

  1. Bit equality with the oracle (int64 views) on the tie-free cases under
     NONE, MIN_EIG, NORMALIZED_MIN_EIG and PLANE: the library is built with
     -ffp-contract=off, both sides sum the neighbours in ascending distance
     and run the same Jacobi sequence, and fp64 divide and sqrt are correctly
     rounded on both.  One thing is not compared: the sign and payload of a
     NaN.  0 / 0 is the negative quiet NaN on x86 and the positive one on the
     device; rows that are NaN on both sides count as equal.
     FROBENIUS: the device inverts 3x3 by the adjugate (inv3), the oracle the
     4x4 with last row and column (0, 0, 0, 1) by cofactors (inv4, as
     Matrix4d::inverse()).  Every 4x4 cofactor of the upper block is the 3x3
     one's two products, each times the exact 1, plus four products that hold
     an exact zero, and the determinant gains one zero term: the same values
     in the same order, except that adding a +0 can turn a -0 into +0.  So
     FROBENIUS is held to the envelope's measured tolerance AND to equality
     in value (-0 == +0) with the oracle; the operation that differs in bits
     is that addition of a signed zero (seen on plane_axis, whose covariances
     have exact zero entries: 149 of 300 rows at k = 10, 142 at k = 20 differ
     in the sign of a zero, none in value).
  2. The longdouble envelope, also on the tied cases; those meet
     assert_cov_parity against the oracle too in nanoflann's tie order.
     Morton order is held to the envelope over its own neighbour lists, read
     with knn_target under the same option.
  3. The NaN / finite pattern is the oracle's row for row (all six entries NaN
     exactly where the covariance is zero under NORMALIZED_MIN_EIG).
  4. Every path in nanoflann's tie order returns the default path's bytes;
     so does Morton order on the tie-free cases.
"""
import numpy as np
import pytest

import cov_cases as CC
import cov_ref as CR
import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import TARGET
from oracle import oracle as O
from parity import assert_cov_parity

pytestmark = pytest.mark.gpu

PATHS = {
    "default": {},
    "tasks": {P.OPT_COV_TASKS: 1},
    "lazy0": {P.OPT_TIE_LAZY: 0},
    "lazy1": {P.OPT_TIE_LAZY: 1},
    "morton": {P.OPT_TIE_ORDER: 0},
}
_GOT = {}
RATIO = {reg: 0.0 for reg in CR.REGS}   # largest device deviation / recorded constant seen so far (printed)


def device_cov(name, k, reg, path):
    """Covariances of a catalogue cloud on a fresh context (and, in Morton order, its own neighbour lists)."""
    key = (name, k, reg, path)
    if key not in _GOT:
        pts = CC.cloud(name)
        c = P.Context(0)
        for opt, val in PATHS[path].items():
            c.set_option(opt, val)
        c.set_params(P.default_params(k_correspondences=k, regularization=O.REG[reg]))
        c.set_target(pts)
        c.compute_covariances(TARGET)
        cov = c.get_covariances(TARGET)
        nbr = c.knn_target(pts, k) if path == "morton" else None
        c.close()
        cov.setflags(write=False)
        _GOT[key] = (cov, nbr)
    return _GOT[key]


def same_bits(a, b):
    """Rows equal bit for bit; NaN equals NaN whatever its sign and payload."""
    eq = (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    return eq.all(axis=1)


def hold_to_envelope(ref, got, reg, what):
    v = CR.check(ref, got, reg)
    ratio = float(np.nanmax(v.dev)) / CR.ORACLE_DEV[reg] if len(v.dev) else 0.0
    RATIO[reg] = max(RATIO[reg], ratio)
    print(f"{what}: deviation {np.nanmax(v.dev):.3g} = {ratio:.3g} x the oracle's constant")
    assert v.nan_ok.all(), f"{what}: {(~v.nan_ok).sum()} rows with a wrong NaN / finite pattern, first {np.flatnonzero(~v.nan_ok)[:8]}"
    bad = np.flatnonzero(~(v.dev <= CR.GPU_MARGIN * CR.ORACLE_DEV[reg]))
    assert len(bad) == 0, f"{what}: {len(bad)} rows outside the envelope, first {bad[:8]}, worst {np.nanmax(v.dev):.3g}"


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(CC.CASES))
def test_cov_cases(name, path):
    case = CC.CASES[name]
    pts = CC.cloud(name)
    for k in case.ks:
        if path == "tasks" and k > 32:
            continue                      # the task kNN holds at most 32 neighbours; k = 64 is the default launch
        for reg in CR.REGS:
            what = f"{name} k={k} {reg} {path}"
            got, nbr = device_cov(name, k, reg, path)
            oracle = CR.case_oracle(name, k, reg)
            base, _ = device_cov(name, k, reg, "default")
            if path == "morton":
                idx, sqd = nbr
                np.testing.assert_array_equal(sqd, CR.case_knn(name, k)[1][:, :k], err_msg=what)
                hold_to_envelope(CR.build(pts, idx), got, reg, what)
                assert np.array_equal(np.isnan(got), np.isnan(oracle)), what
                if case.tie_free:
                    assert got.tobytes() == base.tobytes(), f"{what}: differs from nanoflann order without a tie"
                continue
            hold_to_envelope(CR.case_ref(name, k), got, reg, what)
            nan = np.isnan(oracle)
            assert np.array_equal(np.isnan(got), nan), \
                f"{what}: NaN pattern differs from the oracle's in {(np.isnan(got) != nan).any(axis=1).sum()} rows"
            if case.tie_free:
                diff = np.flatnonzero(~same_bits(got, oracle))
                if reg == "FROBENIUS":
                    vdiff = np.flatnonzero((got != oracle).any(axis=1))
                    print(f"{what}: {len(diff)} rows differ from the oracle in bits, {len(vdiff)} in value")
                    diff = vdiff
                assert len(diff) == 0, f"{what}: {len(diff)} rows differ from the oracle, first {diff[:8]}"
            else:
                assert_cov_parity(pts, k, np.where(nan, 0.0, got), np.where(nan, 0.0, oracle))
            assert got.tobytes() == base.tobytes(), f"{what}: bytes differ from the default path's"
    print("largest device / oracle-constant ratios so far:", {r: f"{v:.3g}" for r, v in RATIO.items()})
