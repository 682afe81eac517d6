"""CPU tests that pin the numpy restatement of the preprocessing kernels
(tests/preprocess_ref.py) to the oracle's PCL restatements, on the edge clouds
the GPU tests (tests/test_gpu_preprocess.py) run.

Centroid bound: a voxel's float32 centroid is c - 1 sequential additions (the
first one, 0 + p, is exact) and one division.  With u = eps32 / 2 and M the
largest |coordinate| among the voxel's points, the k-th partial sum is at most
k M, so the additions err by at most u M (2 + ... + c) < u M c^2 / 2 and the
quotient by at most u M c / 2 + u M: within c eps32 M of the exact mean for
every c >= 1, in any summation order (so the oracle's std::sort order obeys it
too).
"""
import numpy as np
import pytest

import preprocess_ref as PR
from oracle import oracle as O

EPS32 = float(np.finfo(np.float32).eps)


def _clouds():
    out = dict(PR.edge_clouds())
    base = PR.uniform(3000, seed=11)
    for name, idx in PR.nonfinite_patterns(len(base)).items():
        out[f"nan_{name}"] = PR.with_nonfinite(base, idx, np.nan)
    out["inf_every7th"] = PR.with_nonfinite(base, PR.nonfinite_patterns(len(base))["every7th"], np.inf)
    out["ninf_first"] = PR.with_nonfinite(base, [0], -np.inf)
    return out


CLOUDS = _clouds()


def check_centroids(c32, c64, counts, x, leaf, what):
    """|c32 - c64| <= c eps32 M per voxel, M = the largest |coordinate| of the voxel's points."""
    key, _ = PR.voxel_keys(x, leaf)
    order = np.argsort(key, kind="stable")
    _, start = np.unique(key[order], return_index=True)
    M = np.maximum.reduceat(np.abs(x[order]).max(axis=1).astype(np.float64), start)
    err = np.abs(c32.astype(np.float64) - c64).max(axis=1)
    bad = np.flatnonzero(err > counts * EPS32 * M)
    assert len(bad) == 0, f"{what}: voxel {bad[:5]} err {err[bad[:5]]} bound {(counts * EPS32 * M)[bad[:5]]}"


@pytest.mark.parametrize("leaf", PR.LEAVES)
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_voxel_grid_vs_oracle(name, leaf):
    pts = CLOUDS[name]
    ref = O.voxel_grid(pts, leaf)
    got = PR.voxel_grid(pts, leaf)
    assert got is not None
    c32, c64, counts = got
    assert c32.dtype == np.float32 and c32.shape == ref.shape
    x = pts[PR.finite_mask(pts)]
    assert counts.sum() == len(x)
    if len(x) == 0:
        assert len(c32) == 0
        return
    check_centroids(c32, c64, counts, x, leaf, "restatement")
    check_centroids(ref, c64, counts, x, leaf, "oracle")      # same voxel order, or this fails by metres
    np.testing.assert_array_equal(PR.preprocess(pts, 0.0, leaf), c32)


def test_edge_clouds_are_what_they_claim():
    lat = PR.lattice()
    assert len(lat) == 17**3 and lat.min() < 0 < lat.max() and (lat == 0).any()
    for leaf in (0.1, 0.25, 0.3):     # lattice points on voxel faces: p * inv is an integer for some of them
        q = lat * (np.float32(1) / np.float32(leaf))
        assert ((q == np.floor(q)) & (lat != 0)).any(), leaf
    for leaf in PR.LEAVES:
        assert len(PR.voxel_grid(PR.single_voxel(), leaf)[0]) == 1
    assert PR.voxel_grid(PR.sites(), 0.3)[2].max() >= 40          # long runs
    assert (PR.negative() < 0).all()
    c32, _, counts = PR.voxel_grid(PR.one_point(), 0.1)
    np.testing.assert_array_equal(c32, PR.one_point())
    assert counts.tolist() == [1]


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_crop_keep_vs_oracle(name):
    pts = CLOUDS[name]
    for s in (1.0, 12.5):
        np.testing.assert_array_equal(PR.crop_keep(pts, s), O.crop_box_negative(pts, s))


def test_crop_faces():
    s = np.float32(1.0)
    up, dn = np.nextafter(s, np.float32(np.inf)), np.nextafter(-s, np.float32(-np.inf))
    pts = np.array([[s, 0, 0], [up, 0, 0], [-s, 0, 0], [dn, 0, 0], [0, s, -s], [0, 0, up], [-0.0, -0.0, -0.0],
                    [s, s, s], [np.nan, 5, 5], [5, np.inf, 5]], np.float32)
    assert PR.crop_mask(pts, 1.0).tolist() == [False, True, False, True, False, True, False, False, False, False]
    np.testing.assert_array_equal(PR.crop_keep(pts, 1.0), O.crop_box_negative(pts, 1.0))
    # a translated box: the point moves by -centre in float32 before the test
    c = np.array([10.0, -3.0, 0.5], np.float32)
    moved = (pts + c).astype(np.float32)
    back = moved - c
    fin = np.isfinite(back).all(axis=1)
    with np.errstate(invalid="ignore"):
        expect = fin & ((back < -s).any(axis=1) | (back > s).any(axis=1))
    assert PR.crop_mask(moved, 1.0, c).tolist() == expect.tolist()


@pytest.mark.parametrize("name", ["uniform", "lattice", "sites", "nan_every7th"])
@pytest.mark.parametrize("leaf", [0.1, 0.3])
def test_fused_crop_voxel_is_crop_then_voxel(name, leaf):
    pts = CLOUDS[name]
    s = 0.45 if name == "lattice" else 12.5
    fused = PR.voxel_grid(pts, leaf, crop=s)
    two = PR.voxel_grid(PR.crop_keep(pts, s), leaf)
    for a, b in zip(fused, two):
        np.testing.assert_array_equal(a, b)
    ref = O.voxel_grid(O.crop_box_negative(pts, s), leaf)
    assert ref.shape == fused[0].shape
    check_centroids(ref, fused[1], fused[2], PR.crop_keep(pts, s), leaf, "oracle")


def test_overflow_states():
    """The clouds of the GPU overflow cases: the restatement returns None exactly where the oracle
    returns its input unchanged, at a known side of INT_MAX."""
    wide = PR.wide(PR.OVERFLOW_HALF_Z)
    nan = PR.with_nonfinite(wide, [1500])
    for pts in (wide, nan):
        assert PR.voxel_grid(pts, 0.1) is not None and len(O.voxel_grid(pts, 0.1)) < len(pts)
        assert PR.voxel_grid(pts, 0.05) is None
        np.testing.assert_array_equal(O.voxel_grid(pts, 0.05), pts)          # unchanged, NaN included
        np.testing.assert_array_equal(PR.preprocess(pts, 0.0, 0.05), pts)
        np.testing.assert_array_equal(PR.preprocess(pts, 1.0, 0.05), O.crop_box_negative(pts, 1.0))
    under, over = PR.wide(PR.UNDER_HALF_Z), PR.wide(PR.OVER_HALF_Z)
    inv = np.float32(1) / np.float32(0.05)
    d = lambda p: [int(np.int64((p[:, a].max() - p[:, a].min()) * inv)) + 1 for a in range(3)]
    assert d(under) == [4001, 4001, 134] and d(over) == [4001, 4001, 135]
    assert np.prod(d(under)) <= PR.INT_MAX < np.prod(d(over))
    assert PR.voxel_grid(over, 0.05) is None
    np.testing.assert_array_equal(O.voxel_grid(over, 0.05), over)
    c32, c64, counts = PR.voxel_grid(under, 0.05)
    key, _ = PR.voxel_keys(under, 0.05)
    assert 0.99 * 2**31 < int(key.max()) < 2**31                             # keys close to 2^31
    ref = O.voxel_grid(under, 0.05)
    assert ref.shape == c32.shape
    check_centroids(c32, c64, counts, under, 0.05, "restatement")
    check_centroids(ref, c64, counts, under, 0.05, "oracle")


def test_median_range_and_chain():
    rng = np.random.default_rng(0)
    pts = rng.uniform(-50, 50, (1001, 3)).astype(np.float32)
    r = np.sort(np.sqrt((pts.astype(np.float64) ** 2).sum(axis=1)))
    m = PR.median_range(pts)
    assert m.dtype == np.float32 and abs(float(m) - r[500]) <= EPS32 * r[500]
    assert PR.median_range(np.zeros((0, 3), np.float32)) == 0
    assert PR.median_range([[3, 4, 0], [0, 0, 0]]) == 5 and PR.median_range([[3, 4, 0], [0, 0, 0], [0, 0, 1]]) == 1
    # the first scan: (float)(0.95 m + 0.05 m) == m
    vals = np.abs(rng.standard_normal(20000) * 30).astype(np.float32)
    assert all(PR.spaciousness_chain([v])[0][0] == v for v in vals[:2000])
    chain = PR.spaciousness_chain([4.0, 30.0, 30.0])
    assert chain[0] == (np.float32(4.0), 0.5)
    assert chain[1][0] == np.float32(0.95 * 4.0 + 0.05 * 30.0) and chain[1][1] == 1.0
    assert chain[2][0] == np.float32(0.95 * float(chain[1][0]) + 0.05 * 30.0)
    assert [PR.threshold(v) for v in (5.0, 5.01, 10.0, 10.01, 20.0, 20.01)] == [0.5, 1.0, 1.0, 5.0, 5.0, 10.0]
