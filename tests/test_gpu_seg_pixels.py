"""k_seg_pixels (csrc/segment.hip) bit for bit at its edges, through
``Segmentation.process`` / ``images()``, against oracle/segment_ref.py's literal bottom-up
loop with the rounded-double atan2 (``atan2_rd``, the kernel's stated definition of atan2f).

The inputs (tests/seg_pixel_cases.py) are tiny images that ray-cast scans never produce:
x = +-0 ("no info" marks and their overwrites of a 1 from the pair below), NaN and +-inf
coordinates, duplicated vertical neighbours, a point on the sensor, a square that overflows,
points exactly at ``minimum_range`` and one float ulp beside it, pairs within 32 float ulps
of the angle threshold, widths around the 256-thread block, ``ground_rows`` 0, 1 and H - 1.
tests/test_seg_pixel_ref_cpu.py pins the reference and proves that no input depends on the
last ulps of the double atan2, so the ground image is compared with no margin.
"""
import numpy as np
import pytest

import label_ref as LR
import seg_pixel_cases as K
from dynamic_direct_lidar_odometry_amd import segmentation as S
from oracle import segment_ref as R

pytestmark = pytest.mark.gpu


def run(p, xyz, T, resid=None, labelling="host", seg=None):
    own = seg is None
    if own:
        seg = S.Segmentation(0, p, labelling=labelling)
    res = seg.process(xyz, T, resid)
    out = dict(res=(res.segments, res.ground_pixels, res.range_pixels, res.rejected_pixels), images=seg.images(),
               ground_indices=seg.ground_indices(), avg=seg.avg_residuals())
    if own:
        seg.close()
    return out


def check(p, xyz, T, resid=None, labelling="host", seg=None):
    """One scan against the reference; returns the device's result (run())."""
    out = run(p, xyz, T, resid, labelling, seg)
    rng, ground, label = out["images"]
    segments, ground_pixels, range_pixels, rejected_pixels = out["res"]
    orng, oground, oinit = K.reference_init(p, xyz, T)
    assert np.array_equal(rng.view(np.uint32), orng.view(np.uint32))
    assert np.array_equal(ground, oground)
    assert np.array_equal(label == -1, (oground == 1) | (orng == 0))
    # the labelling of the device's own images
    z = np.ascontiguousarray(xyz[:, 2]).reshape(p.rows, p.cols)
    init = np.where((ground == 1) | (rng == 0), -1, 0).astype(np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        olabel, oavg, on = R.label_components(p, rng, z, init, float(T[2, 3]), resid)
    assert np.array_equal(label, olabel)
    assert segments == on
    if labelling == "host":
        assert np.array_equal(out["avg"], oavg)
    else:
        LR.assert_avg_within_bound(out["avg"], oavg, LR.residual_terms(olabel, resid, on) if resid is not None
                                   else [0] * (on + 1))
    assert ground_pixels == int((oground == 1).sum())
    assert range_pixels == int((orng > 0).sum())
    assert rejected_pixels == int((olabel == R.REJECTED).sum())
    assert np.array_equal(out["ground_indices"], R.ground_indices(oground, p.ground_rows))
    return out


def same(a, b):
    return a["res"] == b["res"] and all(x.tobytes() == y.tobytes() for x, y in zip(a["images"], b["images"])) and \
        np.array_equal(a["ground_indices"], b["ground_indices"])


@pytest.mark.parametrize("H,W,ground_rows", K.shape_cases())
def test_special_values_at_every_shape(H, W, ground_rows):
    xyz, T = K.special_scan(H, W, seed=H * W + ground_rows)
    check(K.special_params(H, W, ground_rows), xyz, T, K.residual(H, W, H + W))


@pytest.mark.parametrize("name", sorted(K.MINRANGE))
def test_points_exactly_at_the_minimum_range(name):
    xyz, T, p, exact = K.min_range_scan(name)
    out = check(p, xyz, T)
    rng = out["images"][0].reshape(-1)
    assert (rng[exact].view(np.uint32) == np.float32(p.minimum_range).view(np.uint32)).all()   # !(d < min): kept


@pytest.mark.parametrize("mount,thr", K.RAZOR)
@pytest.mark.parametrize("placement", ["bottom", "first"])
def test_pairs_on_the_angle_threshold(mount, thr, placement):
    xyz, T, p, sweeps = K.razor_scan(mount, thr, placement, seed=len(placement) + int(mount + thr))
    out = check(p, xyz, T)
    ground = out["images"][1]
    lower = p.rows - 1 if placement == "bottom" else p.rows - 2
    for c0, c1 in sweeps:   # (the reference's marks, by the equality above: both decisions in every sweep)
        assert set(ground[lower, c0:c1].tolist()) == {0, 1}


def test_record_layouts_with_nan_padding():
    H, W, g = 12, 300, 6
    xyz, T = K.special_scan(H, W, seed=H * W + g)
    p = K.special_params(H, W, g)
    resid = K.residual(H, W, 3)
    base = check(p, xyz, T, resid)
    for floats in (4, 8):       # 16 and 32 byte records
        assert same(run(p, K.padded(xyz, floats), T, resid), base), floats


@pytest.mark.parametrize("H,W,ground_rows", [(12, 300, 6), (12, 300, 11), (64, 513, 32), (5, 257, 4)])
def test_both_labelling_modes(H, W, ground_rows):
    """The device mode's counts (k_lbl_init) and labelling on -1 marks and an infinite range."""
    xyz, T = K.special_scan(H, W, seed=H * W + ground_rows)
    p = K.special_params(H, W, ground_rows, win_col0=1, win_col1=W - 2)
    resid = K.residual(H, W, H)
    host = check(p, xyz, T, resid, "host")
    dev = check(p, xyz, T, resid, "device")
    assert same(host, dev)
    assert np.isinf(host["images"][0]).any() and (host["images"][1] == -1).any()
    assert H < 12 or host["res"][0] >= 1


def test_handle_reuse():
    (H, W, g, seed_a), (_, _, _, seed_b) = K.REUSE_SCANS
    p = K.special_params(H, W, g)
    a, T = K.special_scan(H, W, seed_a)
    b, _ = K.special_scan(H, W, seed_b)
    for mode in ("host", "device"):
        seg = S.Segmentation(0, p, labelling=mode)
        first = check(p, a, T, K.residual(H, W, 1), mode, seg)
        second = check(p, b, T, None, mode, seg)
        seg.close()
        fresh = run(p, b, T, None, mode)
        assert same(second, fresh) and second["avg"].tobytes() == fresh["avg"].tobytes()
        assert not same(first, second)
