"""Plain numpy restatement of the intensity channel (include/ddlo_intensity.h) on
top of the existing restatements' masks, voxel keys and orders (preprocess_ref,
pcl_order_ref): it imports neither the product nor the oracle.
tests/test_intensity_ref_cpu.py checks it against itself; tests/test_gpu_intensity.py
compares the kernels with it bit for bit.

The rules (PCL 1.10, VoxelGrid with downsample_all_data_, CentroidPoint /
AccumulatorIntensity):
  * no decision reads intensity: masks and keys come from x, y, z alone;
  * a voxel's intensity is the sequential float32 sum of its points' intensities,
    from 0, in the order the x, y, z sums run in, over float32(count);
  * everything else (crop box, compaction, a voxel-index overflow) hands a point's
    intensity on bit for bit.

Clouds are (n, 4) float32 rows x, y, z, intensity.
"""
import numpy as np

import pcl_order_ref as PO
import preprocess_ref as PR

ORDER_INPUT, ORDER_PCL = 0, 1


def _xyzi(points):
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
    assert p.ndim == 2 and p.shape[1] == 4, p.shape
    return p


def pass_mask(points, crop=0.0, centre=(0, 0, 0)):
    """The points a filter pass sees: finite x, y, z and, with crop > 0, outside the box."""
    p = _xyzi(points)
    return PR.crop_mask(p[:, :3], crop, centre) if crop > 0 else PR.finite_mask(p[:, :3])


def run_order(key, order=ORDER_INPUT):
    """The permutation that groups equal keys, each group in the summation order."""
    if order == ORDER_PCL:
        return PO.sort_order(key)[0]
    return np.argsort(key, kind="stable")


def voxel_grid(points, leaf, crop=0.0, centre=(0, 0, 0), order=ORDER_INPUT):
    """(centroids (m, 4) float32, float64 per-voxel mean of the intensity, counts) in voxel-index order,
    or None when the grid overflows an int index."""
    p = _xyzi(points)
    x = p[pass_mask(p, crop, centre)]
    if len(x) == 0:
        return np.zeros((0, 4), np.float32), np.zeros(0, np.float64), np.zeros(0, np.int64)
    key, overflow = PR.voxel_keys(np.ascontiguousarray(x[:, :3]), leaf)
    if overflow:
        return None
    perm = run_order(key, order)
    _, start, cnt = np.unique(key[perm], return_index=True, return_counts=True)
    xs = x[perm]
    s32 = np.zeros((len(start), 4), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(cnt.max())):            # the k-th point of every run that has one
            runs = np.flatnonzero(cnt > k)
            s32[runs] = s32[runs] + xs[start[runs] + k]
        c32 = s32 / cnt.astype(np.float32)[:, None]
        m64 = np.add.reduceat(xs[:, 3].astype(np.float64), start) / cnt
    assert c32.dtype == np.float32
    return c32, m64, cnt.astype(np.int64)


def preprocess(points, crop=0.0, leaf=0.0, centre=(0, 0, 0), order=ORDER_INPUT):
    """ddlo_preprocess_xyzi: crop box, then voxel filter; a grid overflow leaves the (cropped) cloud
    as it is, intensity included.  (m, 4) float32."""
    p = _xyzi(points)
    if leaf > 0:
        v = voxel_grid(p, leaf, crop, centre, order)
        if v is not None:
            return v[0]
    return p[pass_mask(p, crop, centre)] if crop > 0 else p


def map_add(points, leaf):
    """What a keyframe adds to the map (ddlo_map.h): the voxel filter in input order, or (leaf == 0,
    or an index overflow) the finite points in input order."""
    p = _xyzi(points)
    if leaf > 0:
        v = voxel_grid(p, leaf)
        if v is not None:
            return v[0]
    return p[pass_mask(p)]


def same_bits(a, b):
    """Equal shapes and equal bits, except that NaN equals NaN whatever its sign and payload (a sum
    that meets a NaN keeps one, which one is the adder's business)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- inputs both test files use -------------------------------------------------------------------
def with_intensity(xyz, kind="random", seed=40):
    """(n, 4): xyz with an intensity column.  random: floats of [0, 255); bytes: integers 0..255 (every
    partial sum of fewer than 2^16 of them is exact in float32); x: the x column, bit for bit."""
    xyz = PR._xyz(xyz)
    rng = np.random.default_rng(seed)
    if kind == "random":
        w = rng.uniform(0, 255, len(xyz)).astype(np.float32)
    elif kind == "bytes":
        w = rng.integers(0, 256, len(xyz)).astype(np.float32)
    elif kind == "x":
        w = xyz[:, 0].copy()
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.column_stack([xyz, w]).astype(np.float32))


def nonfinite_intensity(points, seed=41):
    """A copy with NaN, +Inf and -Inf over a third of the intensities (x, y, z untouched)."""
    p = _xyzi(points).copy()
    rng = np.random.default_rng(seed)
    idx = rng.permutation(len(p))[:max(len(p) // 3, 1)]
    p[idx, 3] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(idx))
    return p


def records(points, stride, offset):
    """The (n, 4) rows as records of `stride` bytes: x, y, z at 0, the intensity at `offset`, the rest
    filled with a value no output may show."""
    p = _xyzi(points)
    buf = np.full((len(p), stride // 4), np.float32(-777.25), np.float32)
    buf[:, :3] = p[:, :3]
    buf[:, offset // 4] = p[:, 3]
    return buf
