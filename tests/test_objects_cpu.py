"""CPU checks of the object / static-cloud restatements (tests/objects_ref.py)
and of the new C-ABI surface (include/ddlo_seg_objects.h, include/ddlo_odom.h):
exported symbols and struct layouts against the ctypes mirrors."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import segmentation as S
import objects_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rectangle_outline():
    """A 4 m x 1 m x 1.5 m rectangle outline rotated 30 deg about z, centred at (10, -5, 0.75)."""
    t = np.linspace(-1.0, 1.0, 41)
    edge = np.concatenate([np.stack([2 * t, np.full_like(t, 0.5)], 1), np.stack([2 * t, np.full_like(t, -0.5)], 1),
                           np.stack([np.full_like(t, 2.0), 0.5 * t], 1), np.stack([np.full_like(t, -2.0), 0.5 * t], 1)])
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    xy = edge @ np.array([[c, s], [-s, c]]) + np.array([10.0, -5.0])
    pts = np.concatenate([np.column_stack([xy, np.full(len(xy), z)]) for z in (0.0, 0.5, 1.5)])
    return pts.astype(np.float32)


def test_rectangle_outline_matches_analytic_box():
    pts = rectangle_outline()
    a, b = R.get_object_a(pts), R.get_object_b(pts)
    want_axis = np.array([math.cos(math.radians(-60)), math.sin(math.radians(-60))])   # 120 deg mod pi, axis[0] > 0
    for o, tol in ((b, 1e-5), (a, 1e-4)):
        st = o["state"]
        np.testing.assert_allclose(st[[0, 1, 2]], [10.0, -5.0, 0.75], atol=tol)
        np.testing.assert_allclose(st[[4, 5, 6]], [1.0, 4.0, 1.5], atol=tol)
        np.testing.assert_allclose(o["axis"], want_axis, atol=tol)
        assert o["axis"][0] > 0
        np.testing.assert_allclose(st[3], math.sin(math.radians(-60) / 2), atol=tol)
        assert o["num_points"] == len(pts)
        np.testing.assert_allclose(o["density"], len(pts) / 6.0, rtol=1e-4)
    np.testing.assert_allclose(a["state"], b["state"], atol=5e-5)    # A and B agree to float rounding
    np.testing.assert_allclose(a["axis"], b["axis"], atol=5e-5)
    assert b["eig_ratio"] > 3.0
    assert R.dim_ratio(b["state"]) == pytest.approx(4.0 / 1.5, abs=1e-5)


def test_degenerate_segments_follow_the_convention():
    one = R.get_object_b(np.array([[100.0, -70.0, 3.0]], np.float32))
    assert one["axis"].tolist() == [1.0, 0.0] and one["state"][3] == 0.0
    assert one["state"][4:].tolist() == [0.0, 0.0, 0.0] and math.isnan(R.dim_ratio(one["state"]))
    pole = R.get_object_b(np.array([[5.0, 5.0, 0.0], [5.0, 5.0, 1.0], [5.0, 5.0, 2.0]], np.float32))
    assert math.isinf(R.dim_ratio(pole["state"])) and math.isinf(pole["density"])
    two = R.get_object_b(np.array([[0.0, 0.0, 0.0], [0.0, 2.0, 1.0]], np.float32))     # along y: the minor axis is x
    np.testing.assert_allclose(two["axis"], [1.0, 0.0], atol=1e-12)
    np.testing.assert_allclose(two["state"][4:], [0.0, 2.0, 1.0], atol=1e-12)


def test_static_cloud_restatement():
    xyz = np.array([[0.5, 0.5, 0.5], [3, 0, 0], [np.nan, 1, 1], [10.2, 0.1, 0.3], [7, 7, 7]], np.float32)
    lab = np.array([0, 2, 1, -1, R.REJECTED])
    np.testing.assert_array_equal(R.static_cloud(xyz, lab, []), xyz[[0, 1, 3, 4]])
    np.testing.assert_array_equal(R.static_cloud(xyz, lab, [2]), xyz[[0, 3, 4]])
    np.testing.assert_array_equal(R.static_cloud(xyz, lab, [], centre=(10, 0, 0), crop_size=1.0), xyz[[0, 1, 4]])
    np.testing.assert_array_equal(R.static_cloud(xyz, lab, [], crop_size=1.0), xyz[[1, 3, 4]])


NEW_SYMBOLS = ("ddlo_seg_objects", "ddlo_seg_objects_from", "ddlo_seg_static_cloud", "ddlo_odom_process_dynamic",
               "ddlo_odom_keyframe_points", "ddlo_dynamic_default_params")


def test_new_symbols_are_exported_and_bound():
    path = P.lib_path()
    assert os.path.exists(path), "build the library first (make lib)"
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    missing = [n for n in NEW_SYMBOLS if n not in exported]
    assert not missing, f"not exported: {missing}"
    for lib in (S._lib(), OD._lib()):
        for n in NEW_SYMBOLS:
            assert getattr(lib, n).argtypes is not None, n
    hdr = "".join(open(os.path.join(ROOT, "include", h)).read()
                  for h in ("ddlo_segment.h", "ddlo_seg_objects.h", "ddlo_odom.h"))
    assert '#include "ddlo_seg_objects.h"' in hdr      # ddlo_segment.h brings the object calls with it
    for n in NEW_SYMBOLS:
        assert n + "(" in hdr, n


STRUCT_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ddlo_odom.h"
#define F(T, m) printf(#T " " #m " %zu %zu\n", offsetof(T, m), sizeof(((T*)0)->m));
int main(void) {
  printf("ddlo_seg_object size %zu 0\n", sizeof(ddlo_seg_object));
  printf("ddlo_dynamic_params size %zu 0\n", sizeof(ddlo_dynamic_params));
  printf("ddlo_seg_result size %zu 0\n", sizeof(ddlo_seg_result));
  printf("ddlo_odom_result size %zu 0\n", sizeof(ddlo_odom_result));
  F(ddlo_seg_object, id) F(ddlo_seg_object, num_points) F(ddlo_seg_object, state) F(ddlo_seg_object, axis)
  F(ddlo_seg_object, density) F(ddlo_seg_object, avg_residuum)
  F(ddlo_dynamic_params, theta_min) F(ddlo_dynamic_params, theta_max) F(ddlo_dynamic_params, max_dim_ratio)
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_new_struct_layouts_match_ctypes(tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(STRUCT_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    types = {"ddlo_seg_object": S.SegObject, "ddlo_dynamic_params": OD.DynamicParams, "ddlo_seg_result": S.SegResult,
             "ddlo_odom_result": OD.OdomResult}
    for line in filter(None, out):
        t, m, off, size = line.split()
        if m == "size":
            assert C.sizeof(types[t]) == int(off), t
        else:
            fld = getattr(types[t], m)
            assert fld.offset == int(off) and fld.size == int(size), (t, m)
    assert S.OBJECT_DTYPE.itemsize == C.sizeof(S.SegObject)
    for name in ("id", "num_points", "state", "axis", "density", "avg_residuum"):
        assert S.OBJECT_DTYPE.fields[name][1] == getattr(S.SegObject, name).offset, name


def test_dynamic_defaults_and_null_arguments():
    d = OD.default_dynamic_params()
    assert d.theta_min == -60 * math.pi / 180 and d.theta_max == 60 * math.pi / 180 and d.max_dim_ratio == 10.0
    L = OD._lib()
    n = C.c_size_t()
    assert L.ddlo_seg_objects(None, 10.0, None, 0, C.byref(n)) == 1            # GICP_EINVAL
    assert L.ddlo_seg_static_cloud(None, None, 0, None, 0.0, 0.0, None, 0, C.byref(n)) == 1
    assert L.ddlo_odom_keyframe_points(None, 0, None, 0, C.byref(n)) == 1
    assert L.ddlo_odom_process_dynamic(None, None, None, 12, None, C.cast(None, OD.NONSTATIC_FN), None, None, None) == 1
    assert L.ddlo_seg_objects_from(0, None, 12, 4, 4, None, None, 0, 10.0, None, 0, C.byref(n)) == 1
