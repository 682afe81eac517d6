"""GPU parity of the GICP path (covariances, correspondences, linearization,
LM / GN alignment, residuals) through the C-ABI, against the oracle's golden
vectors (tests/golden/gicp_*.npz) and the live oracle.

Tolerances (floating point, stated per check):
  covariances   |d| <= 1e-12 * max|C|   (fp64, different summation order)
  H, b, cost    rel 1e-11               (fp64 moment reduction vs per-point sums)
  correspondences / sq. distances       bit-exact
  poses         |d| <= 1e-6             (fp32 output of an fp64 state)
  iterations / convergence flags        exact
  lm_lambda     rel 16 x lm_ref.LAMBDA_SPREAD_REL (the float64 / longdouble spread of the reference's own
                lm_lambda over whole aligns of the golden pair, measured in tests/test_lm_ref_cpu.py)
"""
import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
import lm_ref as LR
import np_gicp as NP
from dynamic_direct_lidar_odometry_amd import SOURCE, TARGET
from oracle import oracle as O
from parity import assert_cov_parity

pytestmark = pytest.mark.gpu

S2S = dict(k_correspondences=10, max_correspondence_distance=1.0, max_iterations=32, transformation_epsilon=5e-4)
S2M = dict(k_correspondences=20, max_correspondence_distance=2.0, max_iterations=32, transformation_epsilon=0.01)


def assert_lm_outcome(res, ores):
    """lm_lambda, final_cost and nr_iterations of an align against the live oracle's."""
    print(f"lm_lambda rel {abs(res.lm_lambda / ores.lm_lambda - 1):.3g}, final_cost rel "
          f"{abs(res.final_cost / ores.final_cost - 1):.3g}")
    assert res.nr_iterations == ores.nr_iterations
    assert abs(res.final_cost - ores.final_cost) <= 1e-11 * abs(ores.final_cost)
    assert abs(res.lm_lambda - ores.lm_lambda) <= 16 * LR.LAMBDA_SPREAD_REL * abs(ores.lm_lambda), \
        f"lm_lambda {res.lm_lambda!r} vs {ores.lm_lambda!r}: rel {abs(res.lm_lambda / ores.lm_lambda - 1):.3g}"


def s2s_ctx(g, **kw):
    c = P.Context(0)
    c.set_params(P.default_params(**{**S2S, **kw}))
    c.set_target(g["tgt"])
    c.set_source(g["src"])
    c.set_covariances(SOURCE, g["cov_src_PLANE"])
    c.set_covariances(TARGET, g["cov_tgt"])
    return c


@pytest.mark.parametrize("reg", ["NONE", "MIN_EIG", "NORMALIZED_MIN_EIG", "PLANE", "FROBENIUS"])
def test_covariances_all_regularizations(s2s_golden, reg):
    g = s2s_golden
    c = P.Context(0)
    c.set_params(P.default_params(k_correspondences=10, regularization=O.REG[reg]))
    c.set_source(g["src"])
    assert not c.has_covariances(SOURCE)
    c.compute_covariances(SOURCE)
    assert c.has_covariances(SOURCE)
    cov = c.get_covariances(SOURCE)
    assert_cov_parity(g["src"], 10, cov, g[f"cov_src_{reg}"])


@pytest.mark.parametrize("k", [5, 20, 32, 64])
def test_covariances_other_k_vs_oracle(s2s_golden, k):
    src = s2s_golden["src"][:3000]
    c = P.Context(0)
    c.set_params(P.default_params(k_correspondences=k))
    c.set_target(src)
    c.compute_covariances(TARGET)
    assert_cov_parity(src, k, c.get_covariances(TARGET), O.covariances(src, k))


@pytest.mark.parametrize("n,k", [(n, k) for n in [10, 20, 31, 32, 33, 63, 65, 1000, 2049] for k in [10, 20] if k <= n])
def test_covariances_ragged_sizes_vs_oracle(n, k):
    """k = 10 / 20 covariances (two lanes per query, 32 queries per wavefront:
    partial leaves, single and partial wavefronts) against the oracle."""
    rng = np.random.default_rng(n * 7 + k)
    pts = (rng.standard_normal((n, 3)) * [8, 8, 1]).astype(np.float32)
    c = P.Context(0)
    c.set_params(P.default_params(k_correspondences=k))
    c.set_target(pts)
    c.compute_covariances(TARGET)
    assert_cov_parity(pts, k, c.get_covariances(TARGET), O.covariances(pts, k))


@pytest.mark.parametrize("k", [10, 20, 7, 32])
def test_covariances_task_knn_matches(s2s_golden, k, monkeypatch):
    """The opt-in task-based kNN (knn_tasks.hip, OPT_COV_TASKS) and the
    lane-per-query kernel both give the reference's covariances, on the
    ray-cast scan (dense near range, sparse far range: exercises the second
    round) and on a sparse random cloud with exact ties and duplicates
    (integer lattice): nanoflann's neighbour set at every point, within
    1e-12 x scale (the order among equidistant neighbours inside the set
    only changes the double rounding)."""
    rng = np.random.default_rng(7)
    lattice = rng.integers(0, 40, size=(20000, 3)).astype(np.float32)
    for name, cloud in (("scan", s2s_golden["src"]), ("lattice", lattice)):
        ref = O.covariances(cloud, k)
        scale = max(np.abs(ref).max(), 1.0)
        for flag in ("0", "1"):
            c = P.Context(0)
            c.set_option(P.OPT_COV_TASKS, int(flag))
            c.set_params(P.default_params(k_correspondences=k))
            c.set_target(cloud)
            c.compute_covariances(TARGET)
            got = c.get_covariances(TARGET)
            c.close()
            bad = np.where(np.abs(got - ref).max(axis=1) > 1e-12 * scale)[0]
            assert len(bad) == 0, f"{name} tasks={flag}: {len(bad)} rows differ, e.g. {bad[:8]}"


def test_covariance_layouts_roundtrip(s2s_golden):
    g = s2s_golden
    c = P.Context(0)
    c.set_source(g["src"])
    c.set_covariances(SOURCE, g["cov_src_PLANE"])
    m = c.get_covariances(SOURCE, P.COV_MAT4D).reshape(-1, 4, 4)
    np.testing.assert_array_equal(NP.mat_to_sym6(m[:, :3, :3]), g["cov_src_PLANE"])
    assert np.all(m[:, 3, :] == 0) and np.all(m[:, :, 3] == 0)   # Matrix4d with zero 4th row/col (:438)
    c.set_covariances(SOURCE, m.reshape(-1, 16))
    np.testing.assert_array_equal(c.get_covariances(SOURCE), g["cov_src_PLANE"])
    with pytest.raises(P.GicpError):
        c.set_covariances(SOURCE, g["cov_src_PLANE"][:-1])
    c.set_source(g["src"][:100])                                  # new cloud clears covariances
    assert not c.has_covariances(SOURCE)


def test_linearize_vs_golden(s2s_golden):
    g = s2s_golden
    c = s2s_ctx(g)
    H, b, cost, nc = c.linearize(np.eye(4))
    corr, sqd = c.correspondences()
    np.testing.assert_array_equal(corr, g["lin_corr"])
    np.testing.assert_array_equal(sqd, g["lin_sqd"])
    assert nc == int(np.sum(g["lin_corr"] >= 0))
    np.testing.assert_allclose(H, g["lin_H"], rtol=1e-11, atol=1e-11 * np.abs(g["lin_H"]).max())
    np.testing.assert_allclose(b, g["lin_b"], rtol=1e-11, atol=1e-11 * np.abs(g["lin_b"]).max())
    assert abs(cost - float(g["lin_cost"])) <= 1e-11 * abs(float(g["lin_cost"]))


def test_linearize_random_poses_vs_oracle(s2s_golden):
    g = s2s_golden
    c = s2s_ctx(g)
    o = O.Gicp(g["src"], g["tgt"], O.default_params(**S2S))
    o.set_covariances(0, g["cov_src_PLANE"])
    o.set_covariances(1, g["cov_tgt"])
    rng = np.random.default_rng(2)
    for _ in range(5):
        T = np.eye(4)
        T[:3, :3] = NP.so3_exp(rng.normal(0, 0.03, 3))
        T[:3, 3] = rng.normal(0, 0.2, 3)
        H, b, cost, nc = c.linearize(T)
        Ho, bo, co, corr, sqd = o.linearize(T)
        gc, gs = c.correspondences()
        np.testing.assert_array_equal(gc, corr)
        np.testing.assert_array_equal(gs, sqd)
        np.testing.assert_allclose(H, Ho, rtol=1e-11, atol=1e-11 * np.abs(Ho).max())
        np.testing.assert_allclose(b, bo, rtol=1e-11, atol=1e-11 * np.abs(bo).max())
        assert abs(cost - co) <= 1e-11 * abs(co)


def test_align_lm_s2s_vs_golden(s2s_golden):
    g = s2s_golden
    c = s2s_ctx(g)
    pose, res = c.align()
    assert res.iterations_run == int(g["lm_iters"])
    assert res.nr_iterations == int(g["lm_nr"])
    assert res.converged == int(g["lm_converged"]) and not res.lm_failed
    assert res.lm_trials == int(g["lm_trials"])
    np.testing.assert_allclose(pose, g["lm_pose"], atol=1e-6)
    np.testing.assert_allclose(np.array(res.final_hessian).reshape(6, 6), g["lm_hessian"], rtol=1e-9,
                               atol=1e-9 * np.abs(g["lm_hessian"]).max())
    corr, sqd = c.correspondences()
    np.testing.assert_array_equal(corr, g["lm_last_corr"])
    np.testing.assert_array_equal(sqd, g["lm_last_sqd"])
    r = c.residuals()                                   # getResiduals: sqrt of the last sq. distances (:225-232)
    np.testing.assert_array_equal(r, np.sqrt(g["lm_last_sqd"].astype(np.float64)))


def test_align_gn_fixed_vs_golden(s2s_golden):
    g = s2s_golden
    c = s2s_ctx(g, max_iterations=10, optimizer=P.GAUSS_NEWTON, fixed_iterations=10)
    pose, res = c.align()
    assert res.iterations_run == 10 == int(g["gn_iters"])
    np.testing.assert_allclose(pose, g["gn_pose"], atol=1e-6)


def test_align_s2m_vs_golden(s2m_golden):
    g = s2m_golden
    c = P.Context(0)
    c.set_params(P.default_params(**S2M))
    c.set_target(g["sub"])
    c.set_covariances(TARGET, g["cov_sub"])
    c.set_source(g["src"])
    c.set_covariances(SOURCE, g["cov_src"])
    pose, res = c.align(g["guess"])
    assert res.iterations_run == int(g["iters"]) and res.converged == int(g["converged"])
    np.testing.assert_allclose(pose, g["pose"], atol=1e-6)
    # repeated aligns are deterministic
    pose2, res2 = c.align(g["guess"])
    np.testing.assert_array_equal(pose, pose2)


def test_align_computes_missing_covariances(s2s_golden):
    """computeTransformation computes covariances that were not supplied (nano_gicp_impl.hpp:186-193)."""
    g = s2s_golden
    c = P.Context(0)
    c.set_params(P.default_params(**S2S))
    c.set_target(g["tgt"])
    c.set_source(g["src"])
    pose, res = c.align()
    assert c.has_covariances(SOURCE) and c.has_covariances(TARGET)
    np.testing.assert_allclose(c.get_covariances(SOURCE), g["cov_src_PLANE"], atol=1e-12)
    np.testing.assert_allclose(c.get_covariances(TARGET), g["cov_tgt"], atol=1e-12)
    assert res.iterations_run == int(g["lm_iters"])
    np.testing.assert_allclose(pose, g["lm_pose"], atol=1e-6)


def test_align_with_guess_and_param_variants(s2s_golden):
    g = s2s_golden
    rng = np.random.default_rng(9)
    for trial in range(3):
        kw = dict(S2S)
        kw["max_correspondence_distance"] = [0.5, 1.0, 3.0][trial]
        kw["transformation_epsilon"] = [1e-3, 5e-4, 1e-2][trial]
        guess = np.eye(4, dtype=np.float32)
        guess[:3, :3] = NP.so3_exp(rng.normal(0, 0.01, 3))
        guess[:3, 3] = rng.normal(0, 0.1, 3)
        c = s2s_ctx(g, **kw)
        o = O.Gicp(g["src"], g["tgt"], O.default_params(**kw))
        o.set_covariances(0, g["cov_src_PLANE"])
        o.set_covariances(1, g["cov_tgt"])
        pose, res = c.align(guess)
        opose, ores = o.align(guess)
        assert (res.iterations_run, res.converged, res.lm_trials) == (ores.iterations_run, ores.converged, ores.lm_trials)
        np.testing.assert_allclose(pose, opose, atol=1e-6)
        assert_lm_outcome(res, ores)


def test_align_no_correspondences(s2s_golden):
    """Source far from the target: zero correspondences, pose stays at the guess (as the oracle)."""
    g = s2s_golden
    c = P.Context(0)
    c.set_params(P.default_params(**S2S))
    c.set_target(g["tgt"])
    c.set_source(g["src"] + np.float32(1000.0))
    pose, res = c.align()
    o = O.Gicp(g["src"] + np.float32(1000.0), g["tgt"], O.default_params(**S2S))
    opose, ores = o.align()
    assert res.num_correspondences == 0
    assert (res.iterations_run, res.converged) == (ores.iterations_run, ores.converged)
    np.testing.assert_array_equal(pose, opose)
    assert res.lm_lambda == ores.lm_lambda == 0.0   # lambda_0 = 1e-9 * max |diag 0|, times the NaN-rho factor 1/3


def test_align_errors():
    c = P.Context(0)
    with pytest.raises(P.GicpError) as e:
        c.align()
    assert e.value.status in (2, 3)                     # ENOSOURCE / ENOTARGET
    c.set_source(np.random.default_rng(0).standard_normal((50, 3)).astype(np.float32))
    with pytest.raises(P.GicpError) as e:
        c.align()
    assert e.value.status == 2                          # ENOTARGET
    with pytest.raises(P.GicpError) as e:
        c.residuals()
    assert e.value.status == 7                          # ESTATE (no linearization yet)
    c.set_target(np.random.default_rng(1).standard_normal((5, 3)).astype(np.float32))
    with pytest.raises(P.GicpError) as e:
        c.align()                                       # default k=20 > 5 target points
    assert e.value.status == 4                          # ETOOFEW
    with pytest.raises(P.GicpError):
        c.set_params(P.default_params(k_correspondences=0))


def test_transform_source(s2s_golden):
    g = s2s_golden
    c = s2s_ctx(g)
    pose, _ = c.align()
    out = c.transform_source()
    ref = (g["src"].astype(np.float64) @ pose[:3, :3].T.astype(np.float64) + pose[:3, 3]).astype(np.float32)
    np.testing.assert_allclose(out, ref, atol=2e-5)


def test_swap_and_share(s2s_golden):
    g = s2s_golden
    a = s2s_ctx(g)
    pose, _ = a.align()
    # swapSourceAndTarget: clouds and covariances trade places (nano_gicp_impl.hpp:97-106)
    a.swap_source_target()
    assert a.size(SOURCE) == len(g["tgt"]) and a.size(TARGET) == len(g["src"])
    np.testing.assert_array_equal(a.get_covariances(SOURCE), g["cov_tgt"])
    np.testing.assert_array_equal(a.get_covariances(TARGET), g["cov_src_PLANE"])
    inv, _ = a.align(np.linalg.inv(pose.astype(np.float64)).astype(np.float32))
    np.testing.assert_allclose(inv @ pose, np.eye(4), atol=5e-3)
    # shareSourceFrom: S2M uses the S2S source cloud + covariances (odom.cc:530,765)
    b = P.Context(0)
    b.set_params(P.default_params(**S2S))
    b.set_target(g["src"])
    b.set_covariances(TARGET, g["cov_src_PLANE"])
    b.share_source_from(a)
    np.testing.assert_array_equal(b.get_covariances(SOURCE), g["cov_tgt"])
    p2, _ = b.align(np.linalg.inv(pose.astype(np.float64)).astype(np.float32))
    np.testing.assert_array_equal(p2, inv)
    # copy-on-write: new covariances on b do not change a's
    b.set_covariances(SOURCE, g["cov_tgt"] * 2.0)
    np.testing.assert_array_equal(a.get_covariances(SOURCE), g["cov_tgt"])


def test_align_sequence_on_one_ctx_matches_fresh_ctx(s2s_golden):
    """Aligns whose iteration counts go up and down on ONE ctx (the launch
    prediction and speculation adapt to the previous align) give the same
    pose, iteration count, LM trials and flags as each align on a fresh ctx
    and as the oracle."""
    g = s2s_golden
    c = s2s_ctx(g)
    o = O.Gicp(g["src"], g["tgt"], O.default_params(**S2S))
    o.set_covariances(0, g["cov_src_PLANE"])
    o.set_covariances(1, g["cov_tgt"])
    # small -> large -> tiny -> large -> medium -> identity
    offsets = [(0.02, 0.002), (0.35, 0.03), (0.0, 0.0), (0.45, 0.04), (0.1, 0.01), (0.3, 0.0)]
    rng = np.random.default_rng(41)
    seen = []
    for dt, dr in offsets:
        guess = np.eye(4, dtype=np.float32)
        guess[:3, :3] = NP.so3_exp(rng.normal(0, 1, 3) * dr)
        guess[:3, 3] = rng.normal(0, 1, 3) * dt
        pose, res = c.align(guess)
        f = s2s_ctx(g)
        fpose, fres = f.align(guess)
        f.close()
        opose, ores = o.align(guess)
        assert (res.iterations_run, res.nr_iterations, res.converged, res.lm_failed, res.lm_trials) == \
            (fres.iterations_run, fres.nr_iterations, fres.converged, fres.lm_failed, fres.lm_trials)
        np.testing.assert_array_equal(pose, fpose)
        assert (res.iterations_run, res.converged, res.lm_trials) == (ores.iterations_run, ores.converged, ores.lm_trials)
        np.testing.assert_allclose(pose, opose, atol=1e-6)
        assert_lm_outcome(res, ores)
        # state read after the align (the trailing chunk may still be queued)
        out = c.transform_source()
        ref = (g["src"].astype(np.float64) @ pose[:3, :3].T.astype(np.float64) + pose[:3, 3]).astype(np.float32)
        np.testing.assert_allclose(out, ref, atol=2e-5)
        seen.append(res.iterations_run)
    # the sequence really exercised rising and falling iteration counts
    assert any(b > a for a, b in zip(seen, seen[1:])) and any(b < a for a, b in zip(seen, seen[1:])), seen


def test_context_reused_across_cloud_sizes():
    """One context aligning a sequence whose source grows a little and whose
    target grows (same graph-key bucket before the fix: the captured collect
    grid and LDS box cache were sized for the first clouds) gives exactly
    what a fresh context gives for every pair."""
    from dynamic_direct_lidar_odometry_amd import scene
    src, tgt, _ = scene.s2s_pair(64, 1024, 1)
    p = P.default_params(k_correspondences=10, max_correspondence_distance=1.0)
    c = P.Context(0)
    c.set_params(p)
    n0, m0 = 40000, 30000
    # the repeats make the next align reuse the first-chunk graph captured for
    # the previous clouds (same predicted iteration count)
    for ds, dt in ((0, 0), (0, 0), (700, 0), (900, 0), (900, 0), (900, 9000), (300, 20000), (300, 20000)):
        a, b = src[: n0 + ds], tgt[: m0 + dt]
        c.set_target(b)
        c.set_source(a)
        T, r = c.align()
        corr, sqd = c.correspondences()
        f = P.Context(0)
        f.set_params(p)
        f.set_target(b)
        f.set_source(a)
        T2, r2 = f.align()
        corr2, sqd2 = f.correspondences()
        f.close()
        np.testing.assert_array_equal(corr, corr2)
        np.testing.assert_array_equal(sqd, sqd2)
        np.testing.assert_array_equal(T, T2)
        assert r.iterations_run == r2.iterations_run
    c.close()
