"""CPU side of the per-pixel segmentation tests: the reference that
tests/test_gpu_seg_pixels.py holds k_seg_pixels to, and the inputs it uses
(tests/seg_pixel_cases.py).

* libm's atan2f against the rounded double atan2 in the oracle's ground pass: the same range
  image, and ground images that differ only at pixels written by a pair whose two float
  angles are at most one float ulp apart and straddle the threshold;
* every generator produces what it claims, and no generated pair is undecided (its float
  atan2 does not depend on the last ulps of the double atan2);
* hand-built cases with the expected images written out.
"""
import numpy as np
import pytest

import seg_pixel_cases as K
from oracle import segment_ref as R

F32 = np.float32


def ulp_distance(a, b):
    """Float32 steps between a and b (finite, the same sign or zero)."""
    return abs(K._ord(a) - K._ord(b))


def angle_of(at):
    return F32(np.float64(F32(at) * F32(180)) / np.pi)


# ---- libm against the rounded double ---------------------------------------------------------------
def razor_inputs():
    for mount, thr in K.RAZOR:
        for placement in ("bottom", "first"):
            yield (mount, thr, placement), K.razor_scan(mount, thr, placement, seed=len(placement) + int(mount + thr))


def libm_differences(p, xyz, T):
    """The pixels at which the oracle's ground image differs between libm's atan2f and the
    rounded double, after asserting that each is written by a one-ulp threshold pair."""
    with np.errstate(over="ignore", invalid="ignore"):
        rng, full = R.project_scan(xyz, T, p.rows, p.cols, p.minimum_range)
        gm, _ = R.ground_removal(full, rng, p.ground_rows, p.sensor_mount_angle, p.ground_angle_threshold)
        gd, _ = R.ground_removal(full, rng, p.ground_rows, p.sensor_mount_angle, p.ground_angle_threshold, R.atan2_rd)
    H = p.rows
    first = H - p.ground_rows
    mount, thr = F32(p.sensor_mount_angle), F32(p.ground_angle_threshold)
    diff = np.argwhere(gm != gd)
    for r, c in diff:
        explained = False
        for lower in (r, r + 1):          # the pairs that write pixel (r, c)
            if lower < first or lower > H - 1:
                continue
            with np.errstate(over="ignore", invalid="ignore"):
                d = full[lower - 1, c] - full[lower, c]
                s = np.sqrt(d[0] * d[0] + d[1] * d[1])
            am, ad = R.atan2f(d[2], s), R.atan2_rd(d[2], s)
            if not (np.isfinite(am) and np.isfinite(ad)):
                continue
            gm_pair = bool(np.abs(angle_of(am) - mount) <= thr)
            gd_pair = bool(np.abs(angle_of(ad) - mount) <= thr)
            explained |= ulp_distance(am, ad) <= 1 and gm_pair != gd_pair
        assert explained, (r, c)
    return len(diff)


def test_libm_and_rounded_double_differ_only_in_one_ulp_threshold_pairs():
    total = 0
    for _, (xyz, T, p, _) in razor_inputs():
        total += libm_differences(p, xyz, T)
    # the range image does not depend on the atan2
    assert R.segment(p, xyz, T)[0].tobytes() == K.reference(p, xyz, T)[0].tobytes()
    for H, W, g in [(12, 300, 6), (12, 300, 11), (64, 513, 32)]:
        xyz, T = K.special_scan(H, W, seed=H * W + g)
        libm_differences(K.special_params(H, W, g), xyz, T)
    if total == 0:
        pytest.skip("0 differing pixels on the razor-edge inputs: the local libm's atan2f is correctly rounded there")
    assert total > 0


# ---- the generators --------------------------------------------------------------------------------
@pytest.mark.parametrize("mount,thr", K.RAZOR)
@pytest.mark.parametrize("placement", ["bottom", "first"])
def test_razor_sweeps_hold_both_decisions(mount, thr, placement):
    xyz, T, p, sweeps = K.razor_scan(mount, thr, placement, seed=len(placement) + int(mount + thr))
    assert K.undecided_pairs(p, xyz, T) == 0
    rng, ground, _, _, _ = K.reference(p, xyz, T)
    lower = p.rows - 1 if placement == "bottom" else p.rows - 2
    assert len(sweeps) >= 2
    for c0, c1 in sweeps:
        marks = ground[lower, c0:c1]
        assert set(marks.tolist()) == {0, 1}, (c0, marks.tolist())
        if thr == 0.0:   # ground is the single angle mount: dz = 0 alone, every denormal beside it is not
            assert np.flatnonzero(marks).tolist() == [K.SWEEP]
        else:            # the decision is monotone across the sweep: one flip, in its middle
            flips = np.flatnonzero(np.diff(marks))
            assert len(flips) == 1 and abs(int(flips[0]) - K.SWEEP) <= 1
        # the upper pixel carries the pair's write and nothing else
        assert np.array_equal(ground[lower - 1, c0:c1], marks)
    assert (rng[lower] > 0).all() and (rng[lower - 1] > 0).all()


def test_special_images_hold_every_special_value():
    seen = {-1: 0, 0: 0, 1: 0}
    for H, W, g in K.shape_cases():
        xyz, T = K.special_scan(H, W, seed=H * W + g)
        p = K.special_params(H, W, g)
        assert K.undecided_pairs(p, xyz, T) == 0, (H, W, g)
        rng, ground, label, _, _ = K.reference(p, xyz, T)
        for m in seen:
            seen[m] += int((ground == m).sum())
        if (H, W) in ((12, 300), (64, 513)) and g >= H // 2:
            pts = xyz.reshape(H, W, 3)
            assert all((ground == m).sum() > 20 for m in (-1, 0, 1))
            assert K.overwrites(p, xyz, T) >= 1 if H == 12 else True
            finite = np.isfinite(pts).all(axis=2)
            assert ((rng == 0) & finite).any()                    # a finite point on the sensor
            assert np.isinf(rng).any()                            # a square that overflows
            assert ((pts[..., 0] == 0) & np.signbit(pts[..., 0])).any() and \
                ((pts[..., 0] == 0) & ~np.signbit(pts[..., 0])).any()
            assert np.isinf(pts).any() and np.isnan(pts).any()
            assert (pts[:-1] == pts[1:]).all(axis=2).any()        # vertical duplicates
            assert ((label == -1) == ((ground == 1) | (rng == 0))).all()
    assert all(v > 0 for v in seen.values())
    for H, W, g, seed in K.REUSE_SCANS:
        xyz, T = K.special_scan(H, W, seed)
        assert K.undecided_pairs(K.special_params(H, W, g), xyz, T) == 0, seed


@pytest.mark.parametrize("name", sorted(K.MINRANGE))
def test_min_range_points_sit_exactly_on_the_limit(name):
    xyz, T, p, exact = K.min_range_scan(name)
    assert K.undecided_pairs(p, xyz, T) == 0
    rng = K.reference(p, xyz, T)[0].reshape(-1)
    limit = F32(p.minimum_range)
    assert len(exact) >= 24
    assert (rng[exact].view(np.uint32) == limit.view(np.uint32)).all()     # kept: !(d < min)
    n = len(exact) * 7
    moved = np.setdiff1d(np.arange(n), exact)
    assert (rng[moved] == 0).sum() >= len(exact) // 2     # an ulp inward: dropped
    assert (rng[moved] > limit).sum() >= len(exact) // 2  # an ulp outward: kept, farther
    assert ((rng[moved] == 0) | (rng[moved] >= limit)).all()


def test_undecided_helper_sees_a_midpoint():
    lo = F32(0.7853981)
    hi = np.nextafter(lo, F32(1))
    mid = 0.5 * (np.float64(lo) + np.float64(hi))
    steps = np.array([mid, np.nextafter(mid, 1), mid + 4 * np.spacing(mid), mid - 4 * np.spacing(mid),
                      mid + 6 * np.spacing(mid), np.float64(lo), np.float64(hi), 0.0, np.nan, np.inf])
    assert K.near_f32_midpoint(steps).tolist() == [True, True, True, True, False, False, False, False, False, False]


# ---- hand cases ------------------------------------------------------------------------------------
def ground_of(xyz, H, W, ground_rows, mount, thr):
    p = K.params(H, W, ground_rows, mount, thr)
    return K.reference_init(p, np.asarray(xyz, np.float32).reshape(-1, 3), np.eye(4, dtype=np.float32))


def test_hand_overwrite_case():
    """tests/test_segment_cpu.py's 5 x 2 case under the rounded-double atan2."""
    H, W = 5, 2
    xyz = np.zeros((H, W, 3), np.float32)
    xyz[..., 0] = 1.0
    xyz[..., 1] = np.arange(H)[::-1, None] + 1.0
    xyz[1, 0, 0] = 0.0
    _, g, lab = ground_of(xyz, H, W, 3, 0.0, 10.0)
    assert g.tolist() == [[0, 0], [0, 1], [-1, 1], [1, 1], [1, 1]]
    assert lab.tolist() == [[0, 0], [0, -1], [0, -1], [-1, -1], [-1, -1]]
    assert R.ground_indices(g, 3).tolist() == [8, 6, 9, 7, 5]


def test_hand_45_degrees_is_ground_at_threshold_45():
    """dz == s: atan2 gives float(pi / 4), * 180 / pi = exactly 45.0f; |45 - 0| <= 45 holds."""
    assert K.pair_is_ground(F32(3), F32(3), 0.0, 45.0) and angle_of(R.atan2_rd(F32(3), F32(3))) == F32(45)
    xyz = [[[1, 1, 3], [2, 2, -3]],       # row 0: 3 above / below the row 1 points, 3 away along x
           [[4, 1, 0], [5, 2, 0]]]
    rng, g, lab = ground_of(xyz, 2, 2, 1, 0.0, 45.0)
    assert g.tolist() == [[1, 1], [1, 1]]
    assert lab.tolist() == [[-1, -1], [-1, -1]]
    assert (rng > 0).all()
    # four float ulps steeper (more than one ulp of the angle) is not ground
    xyz[0][0][2] = 3.000001
    assert ground_of(xyz, 2, 2, 1, 0.0, 45.0)[1].tolist() == [[0, 1], [0, 1]]


def test_hand_identical_points_are_ground_at_threshold_0():
    """upper == lower: atan2(0, 0) = 0, |0 - 0| <= 0 holds."""
    xyz = [[[2, 1, 5], [3, 1, 5.5]],
           [[2, 1, 5], [3, 1, 5]]]
    _, g, lab = ground_of(xyz, 2, 2, 1, 0.0, 0.0)
    assert g.tolist() == [[1, 0], [1, 0]]
    assert lab.tolist() == [[-1, 0], [-1, 0]]
