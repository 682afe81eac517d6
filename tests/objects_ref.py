"""CPU restatements for the detected objects and the non-static point removal
(include/ddlo_segment.h: ddlo_seg_objects, ddlo_seg_static_cloud), beside
np_gicp.py.  Test helpers only.

getObject (detection.cpp:726-782) in two arithmetics:
  A  float32, sums in input order: PCL's own arithmetic (compute3DCentroid,
     computeCovarianceMatrixNormalized, transformPointCloud, getMinMax3D);
  B  float64 throughout, rounded once at the end.
|A - B| is the size of the float rounding the reference itself carries; the
device result (double sums, rounded once) is compared with B within a multiple
of it.  Both use the header's eigenvector convention: `axis` is the unit
eigenvector of the smaller eigenvalue with axis[0] > 0 (or axis[0] == 0 and
axis[1] > 0), the second axis is (-axis[1], axis[0]), equal eigenvalues give
(1, 0).
"""
import math

import numpy as np

REJECTED = 999999


def minor_axis(cxx, cxy, cyy, T):
    """Closed-form unit eigenvector of the smaller eigenvalue of [[cxx, cxy], [cxy, cyy]] in type T."""
    d = T(cxx) - T(cyy)
    b2 = T(2) * T(cxy)
    h = np.sqrt(d * d + b2 * b2)
    if not h > 0:
        return T(1), T(0)
    if d >= 0:
        mx, my = d + h, b2
    else:
        mx, my = b2, h - d
    n = np.sqrt(mx * mx + my * my)
    ax, ay = -my / n, mx / n
    if ax < 0 or (ax == 0 and ay < 0):
        ax, ay = -ax, -ay
    return T(ax), T(ay)


def _finish(n, cx, cy, ax, ay, umin, umax, vmin, vmax, zmin, zmax, orientation, T):
    half = T(0.5)
    mu, mv = half * (umax + umin), half * (vmax + vmin)
    x = (ax * mu - ay * mv) + cx
    y = (ay * mu + ax * mv) + cy
    du, dv = umax - umin, vmax - vmin
    z32 = np.float32(0.5) * (np.float32(zmax) + np.float32(zmin))      # float in both arithmetics
    dz32 = np.float32(zmax) - np.float32(zmin)
    with np.errstate(divide="ignore", invalid="ignore"):
        if T is np.float32:
            density = np.float32(n) / ((np.float32(du) * np.float32(dv)) * dz32)
        else:
            density = np.float64(n) / ((du * dv) * np.float64(dz32))
    s3 = math.sin(float(orientation) / 2.0)
    return {"num_points": int(n), "state": np.array([x, y, z32, s3, du, dv, dz32], np.float64),
            "axis": np.array([ax, ay], np.float64), "density": float(density)}


def get_object_a(pts):
    """getObject in float32, accumulating in input order."""
    p = np.ascontiguousarray(pts, np.float32)
    n = len(p)
    f = np.float32
    cx = np.cumsum(p[:, 0], dtype=f)[-1] / f(n)
    cy = np.cumsum(p[:, 1], dtype=f)[-1] / f(n)
    dx, dy = p[:, 0] - cx, p[:, 1] - cy
    cxx = np.cumsum(dx * dx, dtype=f)[-1] / f(n)
    cxy = np.cumsum(dx * dy, dtype=f)[-1] / f(n)
    cyy = np.cumsum(dy * dy, dtype=f)[-1] / f(n)
    ax, ay = minor_axis(cxx, cxy, cyy, f)
    # projection_transform = [E^T, -E^T c], applied as (m0 x + m1 y) + (m2 * 0 + m3)
    t0 = -(ax * cx + ay * cy)
    t1 = -(-ay * cx + ax * cy)
    u = (ax * p[:, 0] + ay * p[:, 1]) + t0
    v = (-ay * p[:, 0] + ax * p[:, 1]) + t1
    orientation = f(math.atan2(float(ay), float(ax)))
    return _finish(n, cx, cy, ax, ay, u.min(), u.max(), v.min(), v.max(), p[:, 2].min(), p[:, 2].max(), orientation, f)


def get_object_b(pts):
    """getObject in float64; also returns the eigenvalue ratio of the (x, y) covariance."""
    p32 = np.ascontiguousarray(pts, np.float32)
    p = p32.astype(np.float64)
    n = len(p)
    f = np.float64
    cx, cy = p[:, 0].sum() / n, p[:, 1].sum() / n
    dx, dy = p[:, 0] - cx, p[:, 1] - cy
    cxx, cxy, cyy = (dx * dx).sum(), (dx * dy).sum(), (dy * dy).sum()
    ax, ay = minor_axis(cxx, cxy, cyy, f)
    u = ax * dx + ay * dy
    v = ax * dy - ay * dx
    o = _finish(n, f(cx), f(cy), ax, ay, u.min(), u.max(), v.min(), v.max(), p32[:, 2].min(), p32[:, 2].max(),
                math.atan2(ay, ax), f)
    m, r = 0.5 * (cxx + cyy), 0.5 * math.hypot(cxx - cyy, 2 * cxy)
    with np.errstate(divide="ignore", invalid="ignore"):
        o["eig_ratio"] = float(np.float64(m + r) / np.float64(m - r)) if r > 0 else float("nan")
    return o


def dim_ratio(state):
    """computeAllObjects' ratio (detection.cpp:800-803): double, on the float dimensions."""
    d = np.sort(np.asarray(state, np.float32)[4:7].astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return d[2] / d[1]


def segment_ids(label):
    lab = np.asarray(label).reshape(-1)
    ids = np.unique(lab[(lab > 0) & (lab != REJECTED)])
    return [int(i) for i in ids]


def all_objects(xyz_t, label, max_dim_ratio=10.0, avg=None):
    """computeAllObjects over a label image: [(id, A, B, avg_residuum)] of the kept objects, ascending id."""
    lab = np.asarray(label).reshape(-1)
    xyz = np.asarray(xyz_t, np.float32)[:, :3]
    out = []
    for l in segment_ids(lab):
        pts = xyz[lab == l]
        a, b = get_object_a(pts), get_object_b(pts)
        if dim_ratio(b["state"]) >= np.float32(max_dim_ratio):   # NaN compares false: kept
            continue
        out.append((l, a, b, 0.0 if avg is None or l >= len(avg) else float(avg[l])))
    return out


def static_cloud(xyz_t, label, remove_ids, centre=(0, 0, 0), crop_size=0.0, leaf=0.0):
    """applySegmentation's tail (odom.cc:887-918): the removal, the translated crop box, the voxel grid."""
    xyz = np.ascontiguousarray(np.asarray(xyz_t, np.float32)[:, :3])
    lab = np.asarray(label).reshape(-1)
    keep = np.isfinite(xyz).all(axis=1) & ~np.isin(lab, np.asarray(list(remove_ids), np.int64))
    if crop_size > 0:
        s = np.float32(crop_size)
        loc = xyz - np.asarray(centre, np.float32)[None, :]
        with np.errstate(invalid="ignore"):
            keep &= (loc < -s).any(axis=1) | (loc > s).any(axis=1)
    out = xyz[keep]
    if leaf > 0 and len(out):
        from oracle import oracle as O     # the PCL VoxelGrid restatement tests/test_gpu_odom.py compares against
        out = O.voxel_grid(out, leaf)
    return out


def transform_f32(pts, T):
    """pcl::transformPointCloud in float: (m0 x + m1 y) + (m2 z + m3); non-finite points stay NaN."""
    p = np.asarray(pts, np.float32)
    m = np.asarray(T, np.float32).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore"):
        out = np.stack([(m[r, 0] * x + m[r, 1] * y) + (m[r, 2] * z + m[r, 3]) for r in range(3)], axis=1)
    out[~np.isfinite(p[:, :3]).all(axis=1)] = np.nan
    return out.astype(np.float32)


def field_bounds(a, b, scale):
    """Per-field tolerance and reference: max(4 |A - B|, 2 float32 ulps of `scale`) about float32(B)."""
    ulp = float(np.spacing(np.float32(scale)))
    va = np.concatenate([a["state"], a["axis"], [a["density"]]])
    vb = np.concatenate([b["state"], b["axis"], [b["density"]]])
    with np.errstate(invalid="ignore"):
        tol = np.maximum(4 * np.abs(va - vb), 2 * ulp)
    return vb.astype(np.float32).astype(np.float64), tol, ulp
