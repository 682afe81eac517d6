"""CPU checks of the global map: the numpy restatement of the box removal
(tests/map_ref.py) on hand-built cases, and the C-ABI surface of
include/ddlo_map.h: exported symbols, ctypes signatures, struct layouts and
the yaml defaults."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
import map_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ddlo_map.h")


def f32(*v):
    return np.array(v, np.float32).reshape(-1, 3)


# ---- the restatement ---------------------------------------------------------------------------
def test_point_on_a_face_is_removed_and_the_next_float_is_kept():
    # faces at x = 9 / 11, y = 10 / 14, z = 4.5 / 5.5: every face is farther from 0 than its half extent, so
    # one float step of the coordinate is a representable step of d = p - centre as well
    box = [10.0, 12.0, 5.0, 0.0, 2.0, 4.0, 1.0]
    for axis, sign, half in ((0, 1, 1.0), (0, -1, 1.0), (1, 1, 2.0), (1, -1, 2.0), (2, 1, 0.5), (2, -1, 0.5)):
        on = np.array(box[:3], np.float32)
        on[axis] += np.float32(sign * half)
        beyond = on.copy()
        beyond[axis] = np.nextafter(on[axis], np.float32(sign * np.inf))
        for form in ("f32", "f64"):
            keep = R.keep_mask(np.stack([on, beyond]), [box], 0.0, form)
            assert keep.tolist() == [False, True], (axis, sign, form)


def test_yaw_zero_takes_the_unrotated_path():
    box = [1.0, 2.0, 3.0, 0.0, 2.0, 2.0, 2.0]
    pts = np.random.default_rng(0).uniform(-1.5, 1.5, (200, 3)).astype(np.float32) + f32(1, 2, 3)
    centre, yaw, mn, mx = R.box_params(box)
    assert yaw == 0
    # c and s are not read: garbage gives the same local coordinates
    a = R.local_f32(pts, centre, yaw, np.float32(123.0), np.float32(-7.0))
    assert all(np.array_equal(x, pts[:, k] - centre[k]) for k, x in enumerate(a))
    plain = ((np.abs(pts - centre) <= 1.0).all(axis=1))
    assert np.array_equal(R.inside_f32(pts, box, c=np.float32(123.0), s=np.float32(-7.0)), plain)
    assert 0 < plain.sum() < len(pts)


def test_quarter_turn_swaps_dx_and_dy():
    oz = math.sin(math.pi / 4)                               # yaw = 90 deg
    box = [5.0, 5.0, 0.0, oz, 6.0, 1.0, 2.0]                 # long side along the box's x = the world's y
    along_y, along_x = f32(5.0, 7.5, 0.0), f32(7.5, 5.0, 0.0)
    for form in ("f32", "f64"):
        assert R.keep_mask(along_y, [box], 0.0, form).tolist() == [False]
        assert R.keep_mask(along_x, [box], 0.0, form).tolist() == [True]
    # with the exact c = 0, s = 1: lx = dy, ly = -dx
    centre, yaw, _, _ = R.box_params(box)
    pts = f32(6.0, 9.0, 0.5)
    lx, ly, lz = R.local_f32(pts, centre, yaw, 0.0, 1.0)
    assert (lx[0], ly[0], lz[0]) == (4.0, -1.0, 0.5)
    # the unrotated twin of the box removes the other point
    flat = [5.0, 5.0, 0.0, 0.0, 6.0, 1.0, 2.0]
    assert R.keep_mask(np.concatenate([along_y, along_x]), [flat]).tolist() == [True, False]


def test_margin_widens_all_six_faces():
    box = [0.0, 0.0, 0.0, 0.0, 2.0, 2.0, 2.0]
    pts = []
    for axis in range(3):
        for sign in (1, -1):
            p = np.zeros(3, np.float32)
            p[axis] = sign * 1.25
            pts.append(p)
    pts = np.stack(pts)
    assert R.keep_mask(pts, [box], 0.0).all()
    assert not R.keep_mask(pts, [box], 0.25).any()           # the face itself
    assert not R.keep_mask(pts, [box], 0.5).any()
    assert R.keep_mask(pts * np.float32(1.21), [box], 0.5).all()
    centre, yaw, mn, mx = R.box_params(box, 0.5)
    assert mn.tolist() == [-1.5] * 3 and mx.tolist() == [1.5] * 3


@pytest.mark.parametrize("seed", range(20))
def test_sequential_passes_equal_the_union_pass(seed):
    rng = np.random.default_rng(seed)
    n, nb = int(rng.integers(200, 400)), int(rng.integers(1, 12))
    pts = rng.uniform(-10, 10, (n, 3)).astype(np.float32)
    pts[rng.random(n) < 0.05] = np.nan
    yaw = rng.uniform(-math.pi, math.pi, nb)
    yaw[rng.random(nb) < 0.3] = 0.0
    boxes = np.column_stack([rng.uniform(-8, 8, (nb, 3)), np.sin(yaw / 2), rng.uniform(1, 9, (nb, 3))])
    margin = float(rng.choice([0.0, 0.5]))
    for form in ("f32", "f64"):
        keep = R.keep_mask(pts, boxes, margin, form)
        seq = R.sequential_passes(pts, boxes, margin, form)
        assert seq.tobytes() == pts[keep].tobytes()
        assert not keep[~np.isfinite(pts).all(axis=1)].any()
    if nb >= 4:
        assert 0 < keep.sum() < np.isfinite(pts).all(axis=1).sum()      # the boxes do remove something


# ---- the C-ABI surface -------------------------------------------------------------------------
def declared_functions():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[\w\*]+\s*\**\s*(ddlo_map_\w+)\s*\(", txt, flags=re.M)))


def test_header_declares_the_map():
    names = declared_functions()
    assert names == sorted(["ddlo_map_default_params", "ddlo_map_create", "ddlo_map_destroy", "ddlo_map_add_keyframe",
                            "ddlo_map_add_odom_keyframe", "ddlo_map_clear_boxes", "ddlo_map_size", "ddlo_map_points",
                            "ddlo_map_save_pcd"])
    txt = open(HEADER).read()
    assert '#include "ddlo_odom.h"' in txt
    for h in ("ddlo_gicp.h", "ddlo_odom.h", "ddlo_segment.h", "ddlo_seg_objects.h"):
        assert "ddlo_map.h" not in open(os.path.join(ROOT, "include", h)).read(), h


def test_library_exports_and_binding_covers_every_declared_symbol():
    from dynamic_direct_lidar_odometry_amd import mapping as M
    path = P.lib_path()
    assert os.path.exists(path), "build the library first (make lib)"
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    missing = [n for n in declared_functions() if n not in exported]
    assert not missing, f"declared but not exported: {missing}"
    src = open(os.path.join(ROOT, "dynamic_direct_lidar_odometry_amd", "mapping.py")).read()
    L = M._lib()
    for n in declared_functions():
        assert f'"{n}"' in src, f"{n} has no ctypes signature in the binding"
        assert getattr(L, n).argtypes is not None, n


STRUCT_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ddlo_map.h"
#define F(T, m) printf(#T " " #m " %zu %zu\n", offsetof(T, m), sizeof(((T*)0)->m));
int main(void) {
  printf("ddlo_map_params size %zu 0\n", sizeof(ddlo_map_params));
  printf("ddlo_map_box size %zu 0\n", sizeof(ddlo_map_box));
  F(ddlo_map_params, voxel_filter_use) F(ddlo_map_params, leaf_size) F(ddlo_map_params, filter_bboxes)
  F(ddlo_map_params, filter_margin)
  F(ddlo_map_box, position) F(ddlo_map_box, orientation_z) F(ddlo_map_box, dimensions)
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_struct_layout_matches_ctypes(tmp_path):
    from dynamic_direct_lidar_odometry_amd import mapping as M
    c = tmp_path / "probe.c"
    c.write_text(STRUCT_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    types = {"ddlo_map_params": M.MapParams, "ddlo_map_box": M.MapBox}
    seen = 0
    for line in filter(None, out):
        t, m, off, size = line.split()
        if m == "size":
            assert C.sizeof(types[t]) == int(off), t
        else:
            fld = getattr(types[t], m)
            assert fld.offset == int(off) and fld.size == int(size), (t, m)
            seen += 1
    assert seen == len(M.MapParams._fields_) + len(M.MapBox._fields_)


def test_defaults_are_the_yaml_values():
    from dynamic_direct_lidar_odometry_amd import mapping as M
    p = M.default_map_params()                               # cfg/ddlo.yaml:150-156
    assert (p.voxel_filter_use, p.leaf_size, p.filter_bboxes, p.filter_margin) == (1, 0.25, 1, 0.0)
    q = M.default_map_params(leaf_size=0.5, filter_margin=0.1)
    assert (q.leaf_size, q.filter_margin, q.voxel_filter_use) == (0.5, 0.1, 1)
    assert M._lib().ddlo_map_default_params(None) == 1       # GICP_EINVAL


def test_box_from_object_and_null_arguments():
    from dynamic_direct_lidar_odometry_amd import mapping as M
    from dynamic_direct_lidar_odometry_amd import segmentation as S
    obj = np.zeros(1, S.OBJECT_DTYPE)[0]
    obj["state"] = [1.0, 2.0, 3.0, 0.25, 4.0, 5.0, 6.0]
    b = M.box_from_object(obj)
    assert list(b.position) == [1.0, 2.0, 3.0] and b.orientation_z == 0.25 and list(b.dimensions) == [4.0, 5.0, 6.0]
    so = S.SegObject()
    so.state[:] = [7.0, 8.0, 9.0, -0.5, 1.0, 2.0, 3.0]
    b = M.box_from_object(so)
    assert list(b.position) == [7.0, 8.0, 9.0] and b.orientation_z == -0.5 and list(b.dimensions) == [1.0, 2.0, 3.0]
    L = M._lib()
    n = C.c_size_t()
    assert L.ddlo_map_create(0, None, None) == 1
    assert L.ddlo_map_size(None, C.byref(n)) == 1
    assert L.ddlo_map_add_keyframe(None, None, 0, 12, None) == 1
    assert L.ddlo_map_clear_boxes(None, None, 0, None) == 1
    assert L.ddlo_map_points(None, 0.0, None, 0, C.byref(n)) == 1
    assert L.ddlo_map_save_pcd(None, b"x", 0.0) == 1
    assert L.ddlo_map_destroy(None) == 0
    bad = M.default_map_params(leaf_size=0.0)
    h = C.c_void_p()
    assert L.ddlo_map_create(0, C.byref(bad), C.byref(h)) == 1 and not h
