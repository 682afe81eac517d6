"""Plain numpy restatement of the scan preprocessing kernels (csrc/preprocess.hip)
in their documented operation order, float32 throughout.  It imports neither
the product nor the oracle: tests/test_preprocess_ref_cpu.py pins it to the
oracle on the CPU, tests/test_gpu_preprocess.py compares the kernels with it
bit for bit.

  crop_keep          k_crop_flags + compaction (CropBox, negative, translated)
  voxel_grid         k_minmax_partial / voxel_geometry / k_voxel_keys / stable
                     sort / k_voxel_centroids (VoxelGrid::applyFilter)
  median_range       k_med_hist / k_med_final (computeSpaciousness' median)
  spaciousness_chain the low-pass filter and the adaptive keyframe threshold
                     of the driver (odom.cc:981-1001, 1156-1178)

The cloud generators at the end are the edge clouds both test files use.
"""
import numpy as np

INT_MAX = 2**31 - 1
F32 = np.float32


def _xyz(points):
    return np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3))


def finite_mask(points):
    return np.isfinite(_xyz(points)).all(axis=1)


def crop_mask(points, size, centre=(0, 0, 0)):
    """True where crop_keep keeps the point."""
    p = _xyz(points)
    s = F32(size)
    with np.errstate(invalid="ignore"):
        loc = p - np.asarray(centre, np.float32)[None, :]    # float32 subtraction
        outside = (loc < -s).any(axis=1) | (loc > s).any(axis=1)
    return finite_mask(p) & outside


def crop_keep(points, size, centre=(0, 0, 0)):
    """The finite points with a coordinate of p - centre (float32) below -s or above s, in input
    order; a coordinate exactly at +-s is inside the box."""
    p = _xyz(points)
    return p[crop_mask(p, size, centre)]


def voxel_keys(x, leaf):
    """(keys uint32, overflow) of the finite (n, 3) float32 points x, n > 0."""
    inv = F32(1) / F32(leaf)
    mn, mx = x.min(axis=0), x.max(axis=0)
    with np.errstate(over="ignore"):
        d = [int(np.int64((mx[a] - mn[a]) * inv)) + 1 for a in range(3)]     # float32 product, truncated
    if d[0] * d[1] * d[2] > INT_MAX:
        return None, True
    minb = np.floor(mn * inv).astype(np.int32)
    maxb = np.floor(mx * inv).astype(np.int32)
    divb = (maxb - minb + 1).astype(np.int64)
    i = (np.floor(x * inv) - minb.astype(np.float32)).astype(np.int32).astype(np.int64)
    key = (i[:, 0] + i[:, 1] * divb[0] + i[:, 2] * (divb[0] * divb[1])) & 0xFFFFFFFF   # int arithmetic -> unsigned
    return key.astype(np.uint32), False


def voxel_grid(points, leaf, crop=0.0, centre=(0, 0, 0)):
    """(centroids float32, centroids float64, counts) in voxel-index order, or None when the grid
    overflows an int index.  The points that enter the pass: finite and, with crop > 0, kept by
    crop_keep.  The float32 centroid is the sequential float32 sum in input order over float32(count);
    the float64 one is the exact mean to double precision."""
    p = _xyz(points)
    x = p[crop_mask(p, crop, centre) if crop > 0 else finite_mask(p)]
    if len(x) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float64), np.zeros(0, np.int64)
    key, overflow = voxel_keys(x, leaf)
    if overflow:
        return None
    order = np.argsort(key, kind="stable")
    _, start, cnt = np.unique(key[order], return_index=True, return_counts=True)
    xs = x[order]
    s32 = np.zeros((len(start), 3), np.float32)
    for k in range(int(cnt.max())):            # the k-th point of every run that has one: input order per run
        runs = np.flatnonzero(cnt > k)
        s32[runs] = s32[runs] + xs[start[runs] + k]
    c32 = s32 / cnt.astype(np.float32)[:, None]
    c64 = np.add.reduceat(xs.astype(np.float64), start, axis=0) / cnt[:, None]
    assert c32.dtype == np.float32
    return c32, c64, cnt.astype(np.int64)


def preprocess(points, crop=0.0, leaf=0.0, centre=(0, 0, 0)):
    """What the driver's preprocessing returns: crop box, then voxel filter; a grid overflow leaves
    the (cropped) cloud as it is."""
    p = _xyz(points)
    if leaf > 0:
        v = voxel_grid(p, leaf, crop, centre)
        if v is not None:
            return v[0]
    return crop_keep(p, crop, centre) if crop > 0 else p


def ranges(points):
    p = _xyz(points).astype(np.float64)
    return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).astype(np.float32)


def median_range(points):
    """Element n // 2 of the sorted float32 ranges; 0 for no points."""
    r = ranges(points)
    return F32(np.sort(r)[len(r) // 2]) if len(r) else F32(0)


def threshold(lpf):
    """setAdaptiveParams (odom.cc:1156-1178)."""
    if lpf > 20.0:
        return 10.0
    if lpf > 10.0:
        return 5.0
    if lpf > 5.0:
        return 1.0
    return 0.5


def spaciousness_chain(medians):
    """[(spaciousness float32, keyframe threshold)] of consecutive scans' medians."""
    out, prev = [], None
    for m in medians:
        m = F32(m)
        if prev is None:
            prev = m
        lpf = F32(0.95 * float(prev) + 0.05 * float(m))
        prev = lpf
        out.append((lpf, threshold(float(lpf))))
    return out


# ---- edge clouds ------------------------------------------------------------------------------------
LEAVES = (0.05, 0.1, 0.25, 0.3)


def uniform(n=20000, half=20.0, seed=0):
    return np.random.default_rng(seed).uniform(-half, half, (n, 3)).astype(np.float32)


def lattice():
    """17^3 points at multiples of float32(0.1) from -0.8 to 0.8: on voxel faces at leaf 0.1 / 0.25 / 0.3."""
    t = (np.arange(-8, 9).astype(np.float32) * F32(0.1)).astype(np.float32)
    g = np.stack(np.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(g[np.random.default_rng(1).permutation(len(g))])


def sites(nsites=300, per=40, seed=2):
    """Long runs: `per` points within 2 cm of each of `nsites` sites, interleaved."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-15, 15, (nsites, 3))
    p = (c[None, :, :] + rng.uniform(-0.02, 0.02, (per, nsites, 3))).reshape(-1, 3)
    return p.astype(np.float32)


def negative(n=5000, seed=3):
    return np.random.default_rng(seed).uniform(-30, -10, (n, 3)).astype(np.float32)


def single_voxel(n=700, seed=4):
    return (np.array([3.26, -7.13, 1.52]) + np.random.default_rng(seed).uniform(0, 0.01, (n, 3))).astype(np.float32)


def one_point():
    return np.array([[3.0, -4.0, 5.0]], np.float32)


def edge_clouds():
    return {"uniform": uniform(), "lattice": lattice(), "sites": sites(), "negative": negative(),
            "single_voxel": single_voxel(), "one_point": one_point()}


def wide(half_z, n=3000, seed=5):
    """n points over +-100 x +-100 x +-half_z m with the box's corners among them (exact extents);
    200 points come twice, so a voxel pass that runs returns fewer points than it got."""
    h = np.array([100.0, 100.0, half_z])
    p = np.random.default_rng(seed).uniform(-h, h, (n, 3))
    p[:8] = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * h
    p[n - 200:] = p[8:208]
    return p.astype(np.float32)


# the grid of `wide` at its leaf: d = 2001 x 2001 x 101 (no overflow) at 0.1, 4001 x 4001 x 201 (overflow) at 0.05
OVERFLOW_HALF_Z = 5.0
# at leaf 0.05: d = 4001 x 4001 x 134 = 2 145 072 134 <= INT_MAX < 4001 x 4001 x 135 = 2 161 080 135
UNDER_HALF_Z, OVER_HALF_Z = 3.33, 3.36


def with_nonfinite(points, where, value=np.nan, seed=6):
    """A copy with `value` in one (seeded) coordinate of the points `where` (indices or a mask)."""
    p = _xyz(points).copy()
    idx = np.arange(len(p))[where]
    p[idx, np.random.default_rng(seed).integers(0, 3, len(idx))] = value
    return p


def nonfinite_patterns(n):
    """name -> the points that become non-finite."""
    pat = {"first": [0], "last": [n - 1], "one": [n // 3], "all_but_one": [i for i in range(n) if i != n // 2],
           "all": list(range(n)), "every7th": list(range(0, n, 7))}
    return {k: np.asarray(v, np.int64) for k, v in pat.items()}
