"""Inputs and helpers of the per-pixel segmentation tests (tests/test_seg_pixel_ref_cpu.py,
tests/test_gpu_seg_pixels.py): organized scans that reach the edges of k_seg_pixels
(csrc/segment.hip), which ray-cast scans never do.

The reference of the device is oracle/segment_ref.py's literal bottom-up loop with
``atan2_rd`` (the float rounding of the double atan2, the kernel's stated definition).
The device's double atan2 and numpy's may differ in the last double ulps, which changes
the float only next to a float32 rounding midpoint: ``undecided_pairs`` counts the tested
pairs whose float64 atan2 lies within 4 double ulps of one, and every input generated
here has none (tests/test_seg_pixel_ref_cpu.py asserts it).
"""
import math

import numpy as np

from dynamic_direct_lidar_odometry_amd import segmentation as S
from oracle import segment_ref as R

F32 = np.float32

SHAPES = [(2, 1), (3, 7), (5, 255), (5, 256), (5, 257), (12, 300), (64, 513)]
RAZOR = [(0.0, 10.0), (10.0, 10.0), (0.0, 80.0), (-5.0, 45.0), (0.0, 0.0)]   # (mount, threshold) in degrees
SWEEP = 32                       # float ulps of dz on either side of the flip
SWEEP_COLS = 2 * SWEEP + 1


def ground_rows_of(H):
    return sorted({0, 1, H // 2, H - 1})


def shape_cases():
    return [(H, W, g) for H, W in SHAPES for g in ground_rows_of(H)]


def params(H, W, ground_rows, mount, thr, minimum_range=0.0, **kw):
    """Labelling parameters under which small random images form segments; the window is
    the whole image unless given."""
    d = dict(rows=H, cols=W, ang_bottom=15.0, ground_rows=ground_rows, ground_angle_threshold=thr,
             minimum_range=minimum_range, sensor_mount_angle=mount, theta=0.3, valid_point_num=3, min_line_num=1,
             valid_line_num=1, min_delta_z=0.05, max_delta_z=50.0, max_distance=100.0, max_elevation=50.0,
             win_row0=0, win_row1=H - 1, win_col0=0, win_col1=W - 1)
    d.update(kw)
    return S.default_seg_params(**d)


def pose(t):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = t
    return T


def reference(p, xyz, T, resid=None):
    """(range, ground, label, avg, segments) of the literal loop with the rounded-double atan2."""
    with np.errstate(over="ignore", invalid="ignore"):
        return R.segment(p, xyz, T, resid, atan2=R.atan2_rd)


def reference_init(p, xyz, T):
    """(range, ground, label init) of the same, without the labelling."""
    with np.errstate(over="ignore", invalid="ignore"):
        rng, full = R.project_scan(xyz, np.asarray(T, np.float32).reshape(4, 4), p.rows, p.cols, p.minimum_range)
        ground, init = R.ground_removal(full, rng, p.ground_rows, p.sensor_mount_angle, p.ground_angle_threshold,
                                        R.atan2_rd)
    return rng, ground, init


def residual(H, W, seed):
    g = np.random.default_rng(seed)
    r = np.abs(g.normal(0, 0.2, (H, W))).astype(np.float32)
    r[g.random((H, W)) < 0.3] = 0.0
    return r


# ---- double rounding ------------------------------------------------------------------------------
def near_f32_midpoint(a64, ulps=4):
    """True where the float64 value lies within ``ulps`` double ulps of the midpoint of two
    neighbouring float32 values, i.e. where a last-ulp difference of the double can change
    its float32 rounding.  NaN and infinities are never near one."""
    a = np.asarray(a64, np.float64)
    out = np.zeros(a.shape, bool)
    ok = np.isfinite(a)
    v = a[ok]
    f = v.astype(np.float32)
    lo = np.where(f.astype(np.float64) <= v, f, np.nextafter(f, F32(-np.inf)))
    hi = np.nextafter(lo, F32(np.inf))
    mid = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))   # exact: two 24-bit neighbours
    out[ok] = np.abs(v - mid) <= ulps * np.spacing(np.abs(v))
    return out


def tested_pairs(p, xyz, T):
    """(dz, s) as float32 of every pair groundRemoval tests, in the oracle's arithmetic."""
    first = p.rows - p.ground_rows
    with np.errstate(over="ignore", invalid="ignore"):
        _, full = R.project_scan(xyz, T, p.rows, p.cols, p.minimum_range)
        d = full[first - 1:p.rows - 1] - full[first:p.rows] if p.ground_rows else np.zeros((0, p.cols, 3), np.float32)
        s = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    return d[..., 2], s


def undecided_pairs(p, xyz, T):
    """The tested pairs whose float atan2 depends on the last ulps of the double atan2."""
    dz, s = tested_pairs(p, xyz, T)
    with np.errstate(invalid="ignore"):
        a = np.arctan2(dz.astype(np.float64), s.astype(np.float64))
    return int(near_f32_midpoint(a).sum())


# ---- random images with special values ------------------------------------------------------------
SPECIAL_MOUNT, SPECIAL_THR = 3.0, 12.0
SPECIAL_T = (4.0, -8.0, 2.0)      # the sensor position: powers of two, x != 0


def special_scan(H, W, seed):
    """Columns that walk away from the sensor with slopes on both sides of the ground
    threshold, then: x = +0 and x = -0 (10 %), NaN points, one +-inf coordinate, a point
    equal to its lower neighbour, a point on the sensor (range exactly 0, minimum_range 0)
    and a coordinate of 3e19 (its square overflows: range inf).  Returns (xyz, T)."""
    g = np.random.default_rng(seed)
    t = np.array(SPECIAL_T)
    az = 2 * np.pi * np.arange(W) / W
    dist = np.empty((H, W))
    z = np.empty((H, W))
    dist[H - 1] = 5.0 + 2.0 * np.sin(3 * az) + 0.05 * g.normal(size=W)
    z[H - 1] = -1.5 + 0.05 * g.normal(size=W)
    for r in range(H - 2, -1, -1):
        step = g.uniform(0.2, 1.0, W)
        slope = np.deg2rad(SPECIAL_MOUNT + g.uniform(-30.0, 30.0, W))
        dist[r] = dist[r + 1] + step
        z[r] = z[r + 1] + step * np.tan(slope)
    xyz = np.stack([t[0] + dist * np.cos(az), t[1] + dist * np.sin(az), t[2] + z], -1).astype(np.float32)
    kind = g.random((H, W))
    sign = g.random((H, W)) < 0.5
    axis = g.integers(0, 3, (H, W))
    for r in range(H - 1, -1, -1):     # bottom-up, so a duplicate copies its lower neighbour's final value
        for c in range(W):
            k = kind[r, c]
            if k < 0.10:
                xyz[r, c, 0] = F32(-0.0) if sign[r, c] else F32(0.0)
            elif k < 0.13:
                xyz[r, c] = np.nan
            elif k < 0.14:
                xyz[r, c, axis[r, c]] = np.nan
            elif k < 0.16:
                xyz[r, c, axis[r, c]] = -np.inf if sign[r, c] else np.inf
            elif k < 0.22 and r + 1 < H:
                xyz[r, c] = xyz[r + 1, c]
            elif k < 0.24:
                xyz[r, c] = t.astype(np.float32)
            elif k < 0.26:
                xyz[r, c, axis[r, c]] = F32(-3e19) if sign[r, c] else F32(3e19)
    return xyz.reshape(-1, 3), pose(t)


REUSE_SCANS = [(12, 300, 11, 1), (12, 300, 11, 2)]   # (H, W, ground_rows, seed) of the handle-reuse test


def special_params(H, W, ground_rows, **kw):
    return params(H, W, ground_rows, SPECIAL_MOUNT, SPECIAL_THR, 0.0, **kw)


def overwrites(p, xyz, T):
    """How many -1 marks replaced a 1 written by the pair below, from the oracle alone: the
    images after k and after k + 1 steps of the bottom-up walk."""
    n = 0
    with np.errstate(over="ignore", invalid="ignore"):
        rng, full = R.project_scan(xyz, T, p.rows, p.cols, p.minimum_range)
        prev = R.ground_removal(full, rng, 0, p.sensor_mount_angle, p.ground_angle_threshold, R.atan2_rd)[0]
        for k in range(1, p.ground_rows + 1):
            cur = R.ground_removal(full, rng, k, p.sensor_mount_angle, p.ground_angle_threshold, R.atan2_rd)[0]
            n += int(((prev == 1) & (cur == -1)).sum())
            prev = cur
    return n


# ---- points exactly at the minimum range ----------------------------------------------------------
MINRANGE_T = (4.0, -8.0, 2.0)
MINRANGE = {"3-4-0": ((3, 4, 0), 0.5, 2.5), "2-3-6": ((2, 3, 6), 2.0, 14.0)}   # triple, scale, minimum_range


def _signed_permutations(triple):
    import itertools
    out = set()
    for perm in itertools.permutations(triple):
        for sg in itertools.product((1, -1), repeat=3):
            out.add(tuple(float(a * b) for a, b in zip(perm, sg)))
    return sorted(out)


def min_range_scan(name):
    """Every signed permutation of an integer triple scaled by a power of two, moved by a
    power-of-two translation (so the sum of squares and its root are exact: the float range
    is exactly minimum_range), each followed by the six copies moved one float ulp up and
    down along one axis.  Returns (xyz, T, p, exact) with ``exact`` the pixels of the
    unmoved points; 4 rows, NaN padding."""
    triple, scale, minimum = MINRANGE[name]
    t = np.array(MINRANGE_T, np.float32)
    pts, exact = [], []
    for q in _signed_permutations(triple):
        w = (np.array(q, np.float32) * F32(scale)) + t
        exact.append(len(pts))
        pts.append(w)
        for ax in range(3):
            for towards in (np.inf, -np.inf):
                m = w.copy()
                m[ax] = np.nextafter(m[ax], F32(towards))
                pts.append(m)
    H = 4
    W = -(-len(pts) // H)
    xyz = np.full((H * W, 3), np.nan, np.float32)
    xyz[:len(pts)] = np.array(pts)
    p = params(H, W, 2, 0.0, 30.0, minimum)
    return xyz, pose(t), p, np.array(exact)


# ---- pairs on the angle threshold -----------------------------------------------------------------
def _ord(f):
    """float32 -> integer with the floats' order."""
    i = int(np.float32(f).view(np.int32))
    return i if i >= 0 else -(i & 0x7fffffff)


def _unord(i):
    return np.uint32(i if i >= 0 else (-i) | 0x80000000).view(np.float32)


def pair_is_ground(dz, s, mount, thr, atan2=R.atan2_rd):
    """One pair's decision in the oracle's arithmetic (used to place the sweeps; the tests
    take the decisions from the oracle itself)."""
    a = F32(atan2(F32(dz), F32(s)))
    angle = F32(np.float64(a * F32(180)) / np.pi)
    return bool(np.abs(angle - F32(mount)) <= F32(thr))


def flip_point(s, mount, thr, side):
    """The last ground dz (as an ordered integer) going from tan(mount) s outward on ``side``
    (+1 / -1): the decision is monotone in dz between the two brackets."""
    inside = _ord(F32(math.tan(math.radians(mount)) * float(s)))
    outside = _ord(F32(math.tan(math.radians(mount + side * (thr + 5.0))) * float(s)))
    assert pair_is_ground(_unord(inside), s, mount, thr) and not pair_is_ground(_unord(outside), s, mount, thr)
    while abs(outside - inside) > 1:
        mid = (inside + outside) // 2
        if pair_is_ground(_unord(mid), s, mount, thr):
            inside = mid
        else:
            outside = mid
    return inside


def razor_scan(mount, thr, placement, seed, per_side=3):
    """4 x W image, ground_rows 2 (first = 2), one pair per column: lower (x, y, 0), upper
    (x + dx, y + dy, dz), dz sweeping +-32 float ulps around the value at which the decision
    flips on either side of the mount angle (tan(mount +- threshold) s up to rounding; for an
    edge at 0 degrees with a non-zero mount, where the float subtraction angle - mount
    absorbs the angle, the flip the arithmetic really has).  placement "bottom": the pair in
    rows (H - 2, H - 1); "first": in rows (first - 1, first), whose upper row is never a
    lower one.  Returns (xyz, T, p, sweeps) with sweeps the column ranges."""
    g = np.random.default_rng(seed)
    H = 4
    nsweep = 2 * per_side
    W = nsweep * SWEEP_COLS
    xyz = np.full((H, W, 3), np.nan, np.float32)
    lower = H - 1 if placement == "bottom" else H - 2
    sweeps = []
    for k in range(nsweep):
        side = 1 if k % 2 == 0 else -1
        lo_xy = g.uniform(1.0, 9.0, 2).astype(np.float32) * F32(g.choice([-1.0, 1.0]))
        # s <= 1 keeps a denormal dz / s a non-zero float (threshold 0); otherwise up to 8 m
        off = g.uniform(0.3, 0.7 if thr == 0.0 else 5.0, 2).astype(np.float32)
        up_xy = lo_xy + off
        d = up_xy - lo_xy
        s = np.sqrt(d[0] * d[0] + d[1] * d[1])
        centre = flip_point(s, mount, thr, side)
        c0 = k * SWEEP_COLS
        for j in range(SWEEP_COLS):
            dz = _unord(centre + (j - SWEEP))
            xyz[lower, c0 + j] = (lo_xy[0], lo_xy[1], 0.0)
            xyz[lower - 1, c0 + j] = (up_xy[0], up_xy[1], dz)
        sweeps.append((c0, c0 + SWEEP_COLS))
    p = params(H, W, 2, mount, thr, 0.0)
    return xyz.reshape(-1, 3), pose((0.5, 0.25, -1.0)), p, sweeps


def padded(xyz, floats, fill=np.nan):
    """The scan as records of ``floats`` floats, xyz first, the padding ``fill``."""
    rec = np.full((xyz.shape[0], floats), fill, np.float32)
    rec[:, :3] = xyz
    return rec
