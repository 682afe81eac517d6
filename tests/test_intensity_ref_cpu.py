"""CPU tests of the intensity channel's numpy restatement (tests/intensity_ref.py) against itself, and of
the new C-ABI surface (include/ddlo_intensity.h): exported, bound, and deaf to null handles.

The restatement reuses preprocess_ref's masks and keys and pcl_order_ref's permutation, which their own
CPU tests pin to the oracle and to std::sort; what is new here is the fourth running sum, checked
  * against a float64 per-voxel mean to within float32 rounding of a sequential sum,
  * exactly where sums are exact (integer intensities 0..255), where both summation orders must agree,
  * for NaN / Inf intensities, which may change no count and no x, y, z.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P

import intensity_ref as IR
import pcl_order_ref as PO
import preprocess_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ddlo_intensity.h")
EPS = float(np.finfo(np.float32).eps)

CLOUDS = {"uniform": PR.uniform(6000, half=6.0, seed=50), "sites": PR.sites(60, 40), "lattice": PR.lattice(),
          "single_voxel": PR.single_voxel()}


@pytest.mark.parametrize("name", sorted(CLOUDS))
@pytest.mark.parametrize("order", [IR.ORDER_INPUT, IR.ORDER_PCL])
def test_xyz_are_the_existing_restatements(name, order):
    p = IR.with_intensity(CLOUDS[name])
    for crop, leaf in ((0.0, 0.25), (1.0, 0.1), (1.0, 0.0), (0.0, 0.0)):
        got = IR.preprocess(p, crop, leaf, order=order)
        if leaf > 0 and order == IR.ORDER_PCL:
            ref = PO.voxel_grid(p[:, :3], leaf, crop)[0]
        else:
            ref = PR.preprocess(p[:, :3], crop, leaf)
        assert got[:, :3].tobytes() == np.ascontiguousarray(ref, np.float32).tobytes(), (name, crop, leaf)


@pytest.mark.parametrize("name", sorted(CLOUDS))
@pytest.mark.parametrize("order", [IR.ORDER_INPUT, IR.ORDER_PCL])
def test_intensity_against_float64_mean(name, order):
    """A sequential float32 sum of c non-negative terms is within (c - 1) eps of the exact sum,
    relatively; the division adds half an eps."""
    p = IR.with_intensity(CLOUDS[name])
    for leaf in (0.1, 0.3):
        c32, m64, cnt = IR.voxel_grid(p, leaf, order=order)
        assert len(c32) == len(cnt) and cnt.sum() == len(p)
        cu = cnt * (EPS / 2)                            # (c - 1) roundings of the sum and one of the division:
        bound = cu / (1 - cu) * np.abs(m64)             # gamma_c of the standard analysis, terms of one sign
        assert (np.abs(c32[:, 3].astype(np.float64) - m64) <= bound).all(), (name, leaf)


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_exact_where_sums_are_exact(name):
    p = IR.with_intensity(CLOUDS[name], "bytes")
    for crop, leaf in ((0.0, 0.1), (0.5, 0.3)):          # (0.5: part of the lattice is inside the box)
        a = IR.voxel_grid(p, leaf, crop, order=IR.ORDER_INPUT)
        b = IR.voxel_grid(p, leaf, crop, order=IR.ORDER_PCL)
        assert a[0][:, 3].tobytes() == b[0][:, 3].tobytes()
        assert (a[2] == b[2]).all() and a[2].max() < 2**16
        x = p[IR.pass_mask(p, crop)]
        key, _ = PR.voxel_keys(np.ascontiguousarray(x[:, :3]), leaf)
        _, inv = np.unique(key, return_inverse=True)
        sums = np.bincount(inv, weights=x[:, 3].astype(np.float64))          # exact: integers below 2^24
        assert sums.max() < 2**24
        exact = sums.astype(np.float32) / a[2].astype(np.float32)
        assert exact.dtype == np.float32 and a[0][:, 3].tobytes() == exact.tobytes()


@pytest.mark.parametrize("order", [IR.ORDER_INPUT, IR.ORDER_PCL])
def test_nonfinite_intensity_changes_no_count_and_no_xyz(order):
    base = IR.with_intensity(PR.uniform(4000, half=5.0, seed=51))
    bad = IR.nonfinite_intensity(base)
    assert (~np.isfinite(bad[:, 3])).sum() >= len(bad) // 3 and np.isfinite(bad[:, :3]).all()
    for crop, leaf in ((0.0, 0.3), (1.0, 0.3), (2.0, 0.0), (0.0, 0.0)):
        a, b = IR.preprocess(base, crop, leaf, order=order), IR.preprocess(bad, crop, leaf, order=order)
        assert a.shape == b.shape and a[:, :3].tobytes() == b[:, :3].tobytes()
        if leaf == 0:                                    # handed on bit for bit, NaN and Inf included
            assert b[:, 3].tobytes() == bad[IR.pass_mask(bad, crop), 3].tobytes()
        else:                                            # a voxel with a bad member is not finite
            assert (~np.isfinite(b[:, 3])).any() and np.isfinite(b[:, 3]).any()
            fin = np.isfinite(b[:, 3])
            assert a[fin, 3].tobytes() == b[fin, 3].tobytes()


def test_self_check_intensity_is_x():
    """intensity := x: the channel is summed over the same points, in the same order, with the same
    division, so it equals the x centroid bit for bit."""
    for order in (IR.ORDER_INPUT, IR.ORDER_PCL):
        p = IR.with_intensity(CLOUDS["sites"], "x")
        for crop, leaf in ((0.0, 0.1), (1.0, 0.25), (1.0, 0.0)):
            got = IR.preprocess(p, crop, leaf, order=order)
            assert got[:, 3].tobytes() == got[:, 0].tobytes()


def test_overflow_and_map_add_pass_through():
    w = IR.with_intensity(PR.wide(PR.OVERFLOW_HALF_Z))
    assert IR.voxel_grid(w, 0.05) is None
    assert IR.preprocess(w, 0.0, 0.05).tobytes() == w.tobytes()
    w[5, 1] = np.nan
    assert IR.map_add(w, 0.05).tobytes() == np.delete(w, 5, axis=0).tobytes()
    assert len(IR.map_add(w, 0.1)) < len(w) - 1


def test_records_place_the_channel():
    p = IR.with_intensity(PR.uniform(10, seed=52))
    for stride, off in ((16, 12), (20, 16), (32, 16)):
        r = IR.records(p, stride, off)
        assert r.shape == (10, stride // 4) and r[:, :3].tobytes() == p[:, :3].tobytes()
        assert r[:, off // 4].tobytes() == p[:, 3].tobytes()


# ---- the C-ABI surface -------------------------------------------------------------------------
NEW_SYMBOLS = ("ddlo_odom_set_intensity", "ddlo_odom_get_intensity", "ddlo_odom_keyframe_points_xyzi",
               "ddlo_preprocess_xyzi", "ddlo_seg_set_intensity", "ddlo_seg_get_intensity",
               "ddlo_seg_static_cloud_xyzi", "ddlo_map_set_intensity", "ddlo_map_get_intensity",
               "ddlo_map_add_keyframe_xyzi", "ddlo_map_points_xyzi")


def test_header_declares_exports_and_bindings():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"^\s*[\w\*]+\s*\**\s*(ddlo_\w+)\s*\(", txt, flags=re.M)))
    assert names == sorted(NEW_SYMBOLS)
    inc = os.path.join(ROOT, "include")
    for h in ("ddlo_odom.h", "ddlo_map.h"):
        assert '#include "ddlo_intensity.h"' in open(os.path.join(inc, h)).read(), h
    out = subprocess.run(["nm", "-D", "--defined-only", P.lib_path()], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [n for n in NEW_SYMBOLS if n not in exported]
    pkg = os.path.join(ROOT, "dynamic_direct_lidar_odometry_amd")
    src = "".join(open(os.path.join(pkg, f)).read() for f in ("odometry.py", "mapping.py", "segmentation.py"))
    assert not [n for n in NEW_SYMBOLS if f'"{n}"' not in src]


def test_null_handles_and_bad_offsets_are_einval_without_a_gpu():
    from dynamic_direct_lidar_odometry_amd import mapping as M
    from dynamic_direct_lidar_odometry_amd import odometry as OD
    from dynamic_direct_lidar_odometry_amd import segmentation as S
    L = OD._lib()
    M._lib()
    S._lib()
    n, u, off = C.c_size_t(), C.c_int(), C.c_size_t()
    assert L.ddlo_odom_set_intensity(None, 1, 16) == 1           # GICP_EINVAL
    assert L.ddlo_odom_get_intensity(None, C.byref(u), C.byref(off)) == 1
    assert L.ddlo_odom_keyframe_points_xyzi(None, 0, None, 0, C.byref(n)) == 1
    assert L.ddlo_seg_set_intensity(None, 1, 16) == 1
    assert L.ddlo_seg_get_intensity(None, C.byref(u), C.byref(off)) == 1
    assert L.ddlo_seg_static_cloud_xyzi(None, None, 0, None, 0.0, 0.0, None, 0, C.byref(n)) == 1
    assert L.ddlo_map_set_intensity(None, 1) == 1
    assert L.ddlo_map_get_intensity(None, C.byref(u)) == 1
    assert L.ddlo_map_add_keyframe_xyzi(None, None, 0, 16, 12, None) == 1
    assert L.ddlo_map_points_xyzi(None, 0.0, None, 0, C.byref(n)) == 1
    one = np.zeros((1, 8), np.float32)
    # the offset rules are checked before a device is asked for
    for stride, bad in ((16, 8), (16, 13), (16, 16), (32, 30), (12, 12), (32, 32)):
        assert L.ddlo_preprocess_xyzi(0, P._ptr(one), 1, stride, bad, 0.0, 0.0, 0, None, 0, C.byref(n)) == 1, (stride, bad)
    assert L.ddlo_preprocess_xyzi(0, P._ptr(one), 1, 16, 12, 0.0, 0.0, 2, None, 0, C.byref(n)) == 1   # unknown order
    assert L.ddlo_preprocess_xyzi(0, P._ptr(one), 1, 16, 12, 0.0, 0.0, 0, None, 0, None) == 1
