"""numpy restatement of the global map's box removal (include/ddlo_map.h,
MapNode::dynamicObjectsCB, map.cc:133-156): one negative pcl::CropBox per box.

A box is a row (x, y, z, orientation_z, dx, dy, dz) of float64.  Two forms of
the point test:

  inside_f32   float32 in the device kernel's operation order, with c = cos(yaw)
               and s = sin(yaw) given by the caller (the device takes them from
               cosf / sinf): d = p - centre, lx = (c dx) + (s dy), ly = (c dy) -
               (s dx), lz = dz; no rotation when yaw == 0; inside iff no
               coordinate is < min or > max
  inside_f64   the same expressions in float64 on the reference's float
               parameters (centre, min, max, yaw are floats there)
"""
import math

import numpy as np


def box_params(box, margin=0.0):
    """The float values dynamicObjectsCB hands to CropBox (map.cc:143-152): centre[3], yaw, min[3], max[3]."""
    b = np.asarray(box, np.float64)
    centre = b[0:3].astype(np.float32)
    yaw = np.float32(2.0 * math.asin(b[3]))
    mn = (-b[4:7] / 2 - margin).astype(np.float32)
    mx = (b[4:7] / 2 + margin).astype(np.float32)
    return centre, yaw, mn, mx


def local_f32(pts, centre, yaw, c, s):
    """Box-frame coordinates, float32, the kernel's operation order."""
    p = np.asarray(pts, np.float32)
    c, s = np.float32(c), np.float32(s)
    dx, dy, dz = p[:, 0] - centre[0], p[:, 1] - centre[1], p[:, 2] - centre[2]
    if yaw != 0:
        lx = (c * dx) + (s * dy)
        ly = (c * dy) - (s * dx)
    else:
        lx, ly = dx, dy
    assert lx.dtype == np.float32 and ly.dtype == np.float32 and dz.dtype == np.float32
    return lx, ly, dz


def local_f64(pts, centre, yaw):
    """Box-frame coordinates in float64 (R(yaw)^T (p - centre))."""
    p = np.asarray(pts, np.float32).astype(np.float64)
    ctr = np.asarray(centre, np.float64)
    dx, dy, dz = p[:, 0] - ctr[0], p[:, 1] - ctr[1], p[:, 2] - ctr[2]
    if yaw != 0:
        c, s = math.cos(float(yaw)), math.sin(float(yaw))
        return c * dx + s * dy, c * dy - s * dx, dz
    return dx, dy, dz


def _inside(l, mn, mx):
    lx, ly, lz = l
    out = (lx < mn[0]) | (ly < mn[1]) | (lz < mn[2]) | (lx > mx[0]) | (ly > mx[1]) | (lz > mx[2])
    return ~out


def inside_f32(pts, box, margin=0.0, c=None, s=None):
    """Points inside one box, float32.  c, s default to float32(cos / sin) of the float yaw."""
    centre, yaw, mn, mx = box_params(box, margin)
    if c is None:
        c, s = np.float32(math.cos(float(yaw))), np.float32(math.sin(float(yaw)))
    return _inside(local_f32(pts, centre, yaw, c, s), mn, mx)


def inside_f64(pts, box, margin=0.0):
    centre, yaw, mn, mx = box_params(box, margin)
    return _inside(local_f64(pts, centre, yaw), mn.astype(np.float64), mx.astype(np.float64))


def finite(pts):
    return np.isfinite(np.asarray(pts, np.float32)).all(axis=1)


def keep_mask(pts, boxes, margin=0.0, form="f32"):
    """The single union pass: finite and outside every box."""
    inside = inside_f32 if form == "f32" else inside_f64
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    hit = np.zeros(len(pts), bool)
    for b in np.asarray(boxes, np.float64).reshape(-1, 7):
        hit |= inside(pts, b, margin)
    return finite(pts) & ~hit


def sequential_passes(pts, boxes, margin=0.0, form="f32"):
    """The reference's loop: one negative CropBox pass per box, each over what the last one left."""
    inside = inside_f32 if form == "f32" else inside_f64
    cloud = np.asarray(pts, np.float32).reshape(-1, 3)
    for b in np.asarray(boxes, np.float64).reshape(-1, 7):
        cloud = cloud[finite(cloud) & ~inside(cloud, b, margin)]
    return cloud


def face_distance(pts, box, margin=0.0):
    """Smallest float64 distance of each point's box-frame coordinates to one of the box's six face planes."""
    centre, yaw, mn, mx = box_params(box, margin)
    l = local_f64(pts, centre, yaw)
    d = np.full(len(l[0]), np.inf)
    for a in range(3):
        d = np.minimum(d, np.minimum(np.abs(l[a] - float(mn[a])), np.abs(l[a] - float(mx[a]))))
    return d
