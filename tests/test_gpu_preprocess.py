"""Bit-exact GPU tests of the scan preprocessing kernels (csrc/preprocess.hip)
against their plain numpy restatement (tests/preprocess_ref.py, pinned to the
oracle by tests/test_preprocess_ref_cpu.py).

The file is built with -ffp-contract=off, the radix sort is stable and a
voxel's sum runs in input order, so the crop box, the voxel filter and the
median range are predictable bit for bit: every comparison here is on the
uint32 view of the float32 arrays (-0.0 and NaN payloads included), never a
tolerance.

The median cases build ranges from chosen bit patterns with points (r, 0, 0),
whose range sqrt(r * r) is r exactly.  A range is a non-negative float, so its
first digit (bits >> 21) is below 1024, and at most 1019 when finite
(FLT_MAX >> 21): bin 2047 and the boundaries 1023|1024 and 1535|1536 of the
first histogram cannot hold a range; the first digit is placed at 0, at 1019
and around 511|512 and thread boundaries, the middle and low digits
everywhere the block scan has a boundary.
"""
import ctypes as C

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import scene

import preprocess_ref as PR

pytestmark = pytest.mark.gpu


def bits_equal(got, ref, what=""):
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=what)


def gpu_preprocess(buf, crop=0.0, leaf=0.0):
    """ddlo_preprocess of the rows of buf (float32, >= 3 columns: the stride is the row size)."""
    buf = np.ascontiguousarray(buf, np.float32)
    n = buf.shape[0]
    out = np.zeros((max(n, 1), 3), np.float32)
    m = C.c_size_t()
    st = OD._lib().ddlo_preprocess(0, P._ptr(buf), n, buf.shape[1] * 4, float(crop), float(leaf), P._ptr(out), out.shape[0],
                                   C.byref(m))
    assert st == 0, P.load().gicp_last_error().decode()
    return out[:m.value]


def check(x, crop, leaf, what):
    got = gpu_preprocess(x, crop, leaf)
    bits_equal(got, PR.preprocess(x, crop, leaf), f"{what} crop {crop} leaf {leaf}")
    return got


CLOUDS = PR.edge_clouds()


# ---- voxel filter and crop box ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_voxel_clouds_bit_exact(name):
    x = CLOUDS[name]
    crops = (0.0, 1.0) + ((0.5,) if name == "lattice" else ())     # 0.5: lattice points on the crop faces
    for leaf in PR.LEAVES:
        for crop in crops:
            got = check(x, crop, leaf, name)
            if crop > 0:   # the fused pass == the voxel filter of the cropped cloud
                two = PR.voxel_grid(PR.crop_keep(x, crop), leaf)
                bits_equal(got, two[0], f"{name} fused vs crop then voxel, leaf {leaf}")
    if name == "lattice":
        assert len(gpu_preprocess(x, 0.0, 0.05)) == len(x)          # as many runs as points
        assert 0 < len(gpu_preprocess(x, 0.5, 0.1)) < len(gpu_preprocess(x, 0.0, 0.1))
        assert len(gpu_preprocess(x, 1.0, 0.1)) == 0                # everything cropped


@pytest.mark.parametrize("pattern", ["first", "last", "one", "all_but_one", "all", "every7th"])
def test_nonfinite_points_leave_the_voxel_pass(pattern):
    """NaN / +-inf in one coordinate: the output is the restatement's on the finite points alone
    (k_voxel_tail with and without a sentinel run; lattice at leaf 0.05: one run per valid point)."""
    for cname, leaf in (("uniform3k", 0.1), ("uniform3k", 0.3), ("lattice", 0.05), ("sites", 0.25)):
        base = PR.uniform(3000, seed=11) if cname == "uniform3k" else CLOUDS[cname]
        idx = PR.nonfinite_patterns(len(base))[pattern]
        for value in (np.nan, np.inf, -np.inf) if (cname, leaf) == ("uniform3k", 0.1) else (np.nan,):
            x = PR.with_nonfinite(base, idx, value)
            fin = x[PR.finite_mask(x)]
            assert len(fin) == len(x) - len(idx)
            for crop in (0.0, 1.0):
                got = gpu_preprocess(x, crop, leaf)
                bits_equal(got, PR.preprocess(fin, crop, leaf), f"{cname} {pattern} {value} crop {crop} leaf {leaf}")
                if cname == "lattice" and crop == 0:
                    assert len(got) == len(fin)
                if pattern == "all":
                    assert len(got) == 0
            if value is np.nan or pattern == "every7th":
                bits_equal(gpu_preprocess(x, 12.5, 0.0), PR.crop_keep(fin, 12.5), "crop only")


def test_crop_faces():
    s = np.float32(1.0)
    up, dn = np.nextafter(s, np.float32(np.inf)), np.nextafter(-s, np.float32(-np.inf))
    pts = np.array([[s, 0, 0], [up, 0, 0], [-s, 0, 0], [dn, 0, 0], [0, s, -s], [0, 0, up], [-0.0, -0.0, -0.0],
                    [s, s, s], [np.nan, 5, 5], [5, np.inf, 5], [-0.0, up, -0.0], [dn, -0.0, 7]], np.float32)
    got = gpu_preprocess(pts, 1.0, 0.0)
    bits_equal(got, pts[[1, 3, 5, 10, 11]], "crop faces")           # input order, -0.0 kept as it is
    bits_equal(got, PR.crop_keep(pts, 1.0))
    for leaf in (0.1, 0.3):
        check(pts, 1.0, leaf, "crop faces")
    rng = np.random.default_rng(21)
    far = CLOUDS["negative"]                                        # nothing cropped
    bits_equal(gpu_preprocess(far, 1.0, 0.0), far, "nothing cropped")
    check(far, 1.0, 0.1, "nothing cropped")
    inside = rng.uniform(-1.0, 1.0, (5000, 3)).astype(np.float32)   # everything cropped
    inside[:6] = np.array([[1, 1, 1], [-1, -1, -1], [1, -1, 0], [0, 0, 1], [-1, 0, 0], [0, -0.0, 0]], np.float32)
    for leaf in (0.0, 0.1):
        assert gpu_preprocess(inside, 1.0, leaf).shape == (0, 3)
    inside[4000, 1] = up                                            # all but one
    for leaf in (0.0, 0.1):
        bits_equal(gpu_preprocess(inside, 1.0, leaf), inside[4000:4001])


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 70001]


@pytest.fixture(scope="module")
def sized():
    """70001 points of +-4 m (several points per 0.3 m voxel), every 11th with a NaN."""
    x = PR.uniform(SIZES[-1], half=4.0, seed=31)
    return x, PR.with_nonfinite(x, np.arange(5, len(x), 11))


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_blocks(sized, n):
    """Around the 256-thread blocks and the 64 x 256 grid stride of the bbox pass; the cloud's
    extreme points are its first and its last one, so a missed tail moves the grid."""
    for base in sized:
        x = base[:n].copy()
        x[n - 1] = [-5.0, -5.25, -5.5]
        x[0] = [5.0, 5.25, 5.5] if n > 1 else x[0]
        bits_equal(gpu_preprocess(x, 2.0, 0.0), PR.crop_keep(x, 2.0), f"crop only n {n}")
        check(x, 0.0, 0.3, f"voxel only n {n}")
        check(x, 2.0, 0.1, f"fused n {n}")


@pytest.mark.parametrize("cols", [4, 8])
def test_strided_layouts(cols):
    """16 B and 32 B points with NaN in the intensity and padding words == the packed 12 B call."""
    x = PR.with_nonfinite(PR.uniform(5001, half=6.0, seed=41), np.arange(3, 5001, 13))
    buf = np.full((len(x), cols), np.nan, np.float32)
    buf[:, :3] = x
    for crop, leaf in ((0.0, 0.1), (2.0, 0.0), (2.0, 0.25), (0.0, 0.0)):
        packed = gpu_preprocess(x, crop, leaf)
        bits_equal(gpu_preprocess(buf, crop, leaf), packed, f"stride {cols * 4} crop {crop} leaf {leaf}")
        bits_equal(packed, PR.preprocess(x, crop, leaf) if (crop or leaf) else x)


def test_grid_overflow_returns_the_input():
    wide = PR.wide(PR.OVERFLOW_HALF_Z)
    nan = PR.with_nonfinite(wide, [1500])
    for x in (wide, nan):
        assert PR.voxel_grid(x, 0.05) is None and PR.voxel_grid(x, 0.1) is not None
        bits_equal(gpu_preprocess(x, 0.0, 0.05), x, "overflow, voxel only: unchanged, NaN points in place")
        bits_equal(gpu_preprocess(x, 1.0, 0.05), PR.crop_keep(x, 1.0), "overflow, fused: the crop alone")
        got = check(x, 0.0, 0.1, "no overflow")
        assert len(got) < len(x)
    over, under = PR.wide(PR.OVER_HALF_Z), PR.wide(PR.UNDER_HALF_Z)
    assert PR.voxel_grid(over, 0.05) is None
    bits_equal(gpu_preprocess(over, 0.0, 0.05), over, "just over INT_MAX")
    key, overflow = PR.voxel_keys(under, 0.05)
    assert not overflow and 0.99 * 2**31 < int(key.max()) < 2**31
    got = check(under, 0.0, 0.05, "just under INT_MAX")
    assert len(got) == len(under) - 200
    check(PR.with_nonfinite(under, [0, 7, 99]), 2.0, 0.05, "just under INT_MAX, fused")


# ---- median range ------------------------------------------------------------------------------------
FLT_MAX_BITS = 0x7F7FFFFF


def from_bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def range_points(r, seed=0):
    """Points whose ranges are exactly r: (r, 0, 0) with the sign and the axis varied."""
    r = np.asarray(r, np.float32)
    rng = np.random.default_rng(seed)
    p = np.zeros((len(r), 3), np.float32)
    p[np.arange(len(r)), rng.integers(0, 3, len(r))] = r * rng.choice(np.float32([-1, 1]), len(r))
    return p


def check_median(r, expect_bits=None, what=""):
    r = np.asarray(r, np.float32)
    pts = range_points(r)
    ref = PR.median_range(pts)
    assert ref.view(np.uint32) == np.sort(r.view(np.uint32))[len(r) // 2]     # exact ranges: bits order like floats
    if expect_bits is not None:
        assert int(ref.view(np.uint32)) == expect_bits, what                   # the case is what it claims
    got = OD.median_range(pts)
    assert got.view(np.uint32) == ref.view(np.uint32), f"{what}: got {got!r} ({int(got.view(np.uint32)):#x}) " \
                                                        f"want {ref!r} ({int(ref.view(np.uint32)):#x})"


def around(lo_bits, hi_bits, n, side, floor_bits, ceil_bits, seed):
    """n range bit patterns in [floor, ceil] whose element n // 2 is lo (side 0) or hi (side 1),
    with lo and hi = lo + 1 both present: the median sits on one side of the boundary between them."""
    rng = np.random.default_rng(seed)
    k = n // 2
    nlow = k + 1 if side == 0 else k                   # values <= lo
    low = rng.integers(floor_bits, lo_bits + 1, nlow, dtype=np.int64)
    high = rng.integers(hi_bits, ceil_bits + 1, n - nlow, dtype=np.int64)
    if nlow:
        low[0] = lo_bits
    if n - nlow:
        high[0] = hi_bits
    u = np.concatenate([low, high]).astype(np.uint32)
    return u[rng.permutation(n)]


@pytest.mark.parametrize("n", [1, 2, 3, 20, 21, 255, 256, 257, 2048, 2049, 70001])
def test_median_sizes(n):
    rng = np.random.default_rng(n)
    check_median(from_bits(rng.integers(0, FLT_MAX_BITS + 1, n, dtype=np.int64)), what=f"any float, n {n}")
    check_median(rng.uniform(0, 60, n).astype(np.float32), what=f"uniform ranges, n {n}")
    # 3-4-5 points among them: q a multiple of 2^-4, so 3q, 4q and the range 5q are exact
    q = (rng.integers(1, 4000, n) / 16.0).astype(np.float32)
    pts = range_points(rng.uniform(0, 900, n).astype(np.float32), seed=1)
    pts[::3] = np.stack([3 * q, -4 * q, 0 * q], 1)[::3]
    ref = PR.median_range(pts)
    assert OD.median_range(pts).view(np.uint32) == ref.view(np.uint32)


def test_median_equal_ranges_and_strides():
    for n in (1, 2, 257, 5000):
        check_median(np.zeros(n, np.float32), 0, "all ranges 0")
        check_median(np.full(n, 7.25, np.float32), 0x40E80000, "all ranges equal")
        check_median(from_bits(np.full(n, FLT_MAX_BITS)), FLT_MAX_BITS, "all FLT_MAX: last bins 1019 / 2047 / 1023")
        check_median(from_bits(np.full(n, 1)), 1, "all the smallest denormal: bins 0 / 0 / 1")
    assert OD.median_range(np.zeros((0, 3), np.float32)) == 0
    r = np.random.default_rng(3).uniform(0, 50, 3001).astype(np.float32)
    pts = range_points(r)
    for cols in (4, 8):
        buf = np.full((len(pts), cols), np.nan, np.float32)
        buf[:, :3] = pts
        assert OD.median_range(buf, stride=cols * 4).view(np.uint32) == PR.median_range(pts).view(np.uint32)
    L, m = OD._lib(), C.c_float()
    assert L.ddlo_median_range(0, P._ptr(pts), len(pts), 8, C.byref(m)) == 1        # EINVAL, as ddlo_preprocess
    assert L.ddlo_median_range(0, P._ptr(pts), len(pts), 14, C.byref(m)) == 1
    assert L.ddlo_median_range(0, None, 5, 12, C.byref(m)) == 1
    assert L.ddlo_median_range(0, P._ptr(pts), len(pts), 12, None) == 1


def test_median_single_digit_differences():
    rng = np.random.default_rng(5)
    for n in (1000, 4097):
        top = (rng.integers(0, 1020, n, dtype=np.int64) << 21) | 0x155555                  # top 11 bits only
        mid = (521 << 21) | (rng.integers(0, 2048, n, dtype=np.int64) << 10) | 0x2AA       # middle 11 bits only
        low = (0x41200000 >> 10 << 10) | rng.integers(0, 1024, n, dtype=np.int64)          # low 10 bits only
        for name, u in (("top", top), ("middle", mid), ("low", low)):
            check_median(from_bits(u), what=f"ranges differing in the {name} digit only, n {n}")


def _boundaries():
    cases = []
    # first digit (bits >> 21): bins b-1 | b
    for b in (1, 8, 9, 16, 504, 511, 512, 513, 520, 1016, 1019):
        cases.append(("d0", b, (b << 21) - 1, b << 21, 0, FLT_MAX_BITS))
    # middle digit at a fixed first digit (521: the ranges around 10 m)
    d0 = 521
    for b in (1, 8, 15, 16, 511, 512, 1023, 1024, 1535, 1536, 2040, 2047):
        hi = (d0 << 21) | (b << 10)
        cases.append(("d1", b, hi - 1, hi, d0 << 21, (d0 << 21) | 0x1FFFFF))
    # low digit (1024 bins, 4 per thread) at a fixed 22-bit prefix
    pre = 0x41A00000 >> 10
    for b in (1, 4, 7, 8, 255, 256, 511, 512, 767, 768, 1020, 1023):
        hi = (pre << 10) | b
        cases.append(("d2", b, hi - 1, hi, pre << 10, (pre << 10) | 0x3FF))
    return cases


@pytest.mark.parametrize("digit,b,lo,hi,floor,ceil", _boundaries(), ids=lambda v: str(v))
def test_median_on_bin_boundaries(digit, b, lo, hi, floor, ceil):
    """The median in bin b - 1 or in bin b of one digit: thread ranges (8 bins, 4 in the low digit),
    the wavefront boundaries of the block scan, the first and the last bin."""
    for n in (21, 1500):
        for side in (0, 1):
            u = around(lo, hi, n, side, floor, ceil, seed=b + n + side)
            check_median(from_bits(u), hi if side else lo, f"{digit} bins {b - 1}|{b} side {side} n {n}")
    # the extreme bins themselves: every range in the digit's first / last bin
    if digit == "d1" and b in (1, 2047):
        bin_ = 0 if b == 1 else 2047
        u = (521 << 21) | (bin_ << 10) | np.random.default_rng(b).integers(0, 1024, 999, dtype=np.int64)
        check_median(from_bits(u), what=f"middle digit {bin_}")
    if digit == "d0" and b in (1, 1019):
        f, c = (0, (1 << 21) - 1) if b == 1 else (1019 << 21, FLT_MAX_BITS)
        u = np.random.default_rng(b).integers(f, c + 1, 999, dtype=np.int64)
        check_median(from_bits(u), what=f"first digit {b - 1 if b == 1 else b}")


@pytest.mark.parametrize("n", [1000, 1001, 70001])
def test_median_rank_in_a_duplicated_bin(n):
    """40 % of the points share one range (more than half could not have n // 2 on their first or
    last copy); n // 2 falls on its first copy, its last copy, and one place outside either end."""
    rng = np.random.default_rng(n)
    V, dup, k = np.float32(12.625), (4 * n) // 10, n // 2
    below_v = np.nextafter(V, np.float32(0))            # neighbours one ulp away: a rank off by one shows
    above_v = np.nextafter(V, np.float32(np.inf))
    for nbelow, expect in ((k, V), (k - dup + 1, V), (k + 1, below_v), (k - dup, above_v)):
        nabove = n - dup - nbelow
        assert nbelow >= 1 and nabove >= 1
        lo = rng.uniform(0, 12, nbelow).astype(np.float32)
        hi = rng.uniform(13, 80, nabove).astype(np.float32)
        lo[0], hi[0] = below_v, above_v
        r = np.concatenate([lo, np.full(dup, V, np.float32), hi])[rng.permutation(n)]
        check_median(r, int(np.float32(expect).view(np.uint32)), f"n {n}: {nbelow} below the duplicated range")


def test_median_of_a_random_cloud():
    """uniform +-50 m, 70001 points: here the ranges go through the device's double sqrt."""
    pts = np.random.default_rng(9).uniform(-50, 50, (70001, 3)).astype(np.float32)
    assert OD.median_range(pts).view(np.uint32) == PR.median_range(pts).view(np.uint32)


# ---- the driver: spaciousness and the adaptive keyframe threshold ----------------------------------------
def _driver(**kw):
    return OD.Odometry(0, OD.default_odom_params(skip_first_scan=0, crop_use=0, vf_scan_use=0, **kw))


@pytest.fixture(scope="module")
def scan():
    return np.ascontiguousarray(scene.s2s_pair(32, 512, 3)[1], np.float32)


def test_first_frame_spaciousness_and_threshold(scan):
    m0 = float(PR.median_range(scan))
    seen = []
    for target, thresh in ((3.0, 0.5), (7.5, 1.0), (15.0, 5.0), (30.0, 10.0)):
        x = (scan * np.float32(target / m0)).astype(np.float32)
        m = PR.median_range(x)
        assert PR.threshold(float(m)) == thresh                      # the scale puts the median in this band
        assert PR.spaciousness_chain([m]) == [(m, thresh)]           # (float)(0.95 m + 0.05 m) == m
        gpu = _driver()
        res = gpu.process(x)
        gpu.close()
        assert res.status == OD.FIRST and res.scan_points == len(x)
        assert res.spaciousness == float(m), (res.spaciousness, float(m))
        assert res.keyframe_thresh_dist == thresh
        seen.append(res.keyframe_thresh_dist)
    assert seen == [0.5, 1.0, 5.0, 10.0]


def test_three_frames_spaciousness_chain(scan):
    frames = [(scan * np.float32(s)).astype(np.float32) for s in (1.0, 1.02, 1.04)]
    chain = PR.spaciousness_chain([PR.median_range(f) for f in frames])
    assert len({float(c[0]) for c in chain}) == 3
    gpu = _driver()
    for i, (f, (lpf, thresh)) in enumerate(zip(frames, chain)):
        res = gpu.process(f)
        assert res.status == (OD.FIRST if i == 0 else OD.TRACKED), i
        assert res.spaciousness == float(lpf), (i, res.spaciousness, float(lpf))
        assert res.keyframe_thresh_dist == thresh, i
    gpu.close()


def test_overflowed_voxel_grid_does_not_hide_nan_points():
    """crop box off, voxel filter on, grid overflow: the scan reaches the index build as it came, so
    its NaN point must be found there (GICP_ENONFINITE), on the first and on a tracked frame."""
    clean = PR.wide(PR.OVERFLOW_HALF_Z)
    bad = PR.with_nonfinite(clean, [1500])
    assert PR.voxel_grid(bad, 0.05) is None and PR.voxel_grid(clean, 0.05) is None     # the overflow branch
    kw = dict(skip_first_scan=0, crop_use=0, vf_scan_use=1, vf_scan_res=0.05)
    first = OD.Odometry(0, OD.default_odom_params(**kw))
    with pytest.raises(P.GicpError) as e:
        first.process(bad)
    assert e.value.status == 8                                                          # GICP_ENONFINITE
    first.close()
    gpu = OD.Odometry(0, OD.default_odom_params(**kw))
    res = gpu.process(clean)
    assert res.status == OD.FIRST and res.scan_points == len(clean)                     # the input, unchanged
    with pytest.raises(P.GicpError) as e:
        gpu.process(bad)
    assert e.value.status == 8
    gpu.close()
