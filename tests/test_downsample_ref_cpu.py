"""CPU tests of the row/column filter's restatement (tests/downsample_ref.py) and of the library's
new entries (include/ddlo_downsample.h, ddlo_odom.h): hand-worked cases, the equivalence of
ExtractIndices' NaN fill and the device's compaction through the crop and voxel restatements in both
summation orders, exported symbols and null handles.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import segmentation as S
from oracle import oracle as O
import downsample_ref as D
import pcl_order_ref as PO
import preprocess_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_index_set_by_hand():
    assert D.index_set(3, 4, 2, 3).tolist() == [0, 3, 8, 11]
    assert D.index_set(3, 4, 1, 1).tolist() == list(range(12))
    assert D.index_set(3, 4, 3, 4).tolist() == [0]          # a step of the whole extent, and beyond it
    assert D.index_set(3, 4, 4, 5).tolist() == [0]
    assert D.index_set(2, 5, 1, 10).tolist() == [0, 5]
    # cfg/ddlo.yaml (2, 2) and cfg/DOALS.yaml (1, 10): ceil(H / row) * ceil(W / col)
    assert len(D.index_set(128, 1024, 2, 2)) == 64 * 512
    assert len(D.index_set(64, 2048, 1, 10)) == 64 * 205


def test_extract_keep_organized_by_hand():
    S4 = D.index_set(3, 4, 2, 3)
    assert D.extract_keep_organized(12, S4).tolist() == [i in (0, 3, 8, 11) for i in range(12)]
    # a shorter input: the indices at or beyond n have no effect
    assert D.extract_keep_organized(9, S4).tolist() == [i in (0, 3, 8) for i in range(9)]
    assert D.extract_keep_organized(4, S4).tolist() == [True, False, False, True]
    # |S| > n: the filter reports an error and passes the input on
    assert D.extract_skipped(3, S4) and D.extract_keep_organized(3, S4).tolist() == [True] * 3
    assert not D.extract_skipped(4, S4)


def test_keyframe_pass_by_hand():
    # 2 x 4, steps (1, 2): S = {0, 2, 4, 6}.  Pixel 1 removed: the compacted cloud is the pixels
    # 0 2 3 4 5 6 7, positions 0, 2, 4, 6 of it are the pixels 0, 3, 5, 7, not the pixels of S.
    removed = np.array([0, 1, 0, 0, 0, 0, 0, 0], np.uint8)
    keep, skipped = D.keyframe_keep(removed, 2, 4, 1, 2)
    assert keep.tolist() == [1, 0, 0, 1, 0, 1, 0, 1] and skipped == 0
    none, _ = D.keyframe_keep(np.zeros(8, np.uint8), 2, 4, 1, 2)
    assert none.tolist() == [1, 0, 1, 0, 1, 0, 1, 0]                     # nothing removed: the pixels of S
    # the row of a position is j // cols of the compacted cloud: 3 x 3, steps (2, 1), S = {0 1 2 6 7 8};
    # pixels 0 and 4 removed -> cloud 1 2 3 5 6 7 8 (n' = 7), positions 0 1 2 6 stay: pixels 1 2 3 8
    removed = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], np.uint8)
    keep, skipped = D.keyframe_keep(removed, 3, 3, 2, 1)
    assert keep.tolist() == [0, 1, 1, 1, 0, 0, 0, 0, 1] and skipped == 0


def test_keyframe_pass_indices_exceed_input():
    # 2 x 2, steps (1, 1): |S| = 4 > n' = 3: nothing is filtered, only the removal shows
    removed = np.array([0, 0, 1, 0], np.uint8)
    keep, skipped = D.keyframe_keep(removed, 2, 2, 1, 1)
    assert keep.tolist() == [1, 1, 0, 1] and skipped == 1
    # |S| == n' is not skipped: 2 x 4, steps (1, 2), four removed
    removed = np.array([1, 1, 0, 0, 1, 1, 0, 0], np.uint8)
    keep, skipped = D.keyframe_keep(removed, 2, 4, 1, 2)
    assert skipped == 0 and keep.tolist() == [0, 0, 1, 0, 0, 0, 1, 0]   # positions 0, 2 of the pixels 2 3 6 7
    one_more = removed.copy()
    one_more[7] = 1
    keep, skipped = D.keyframe_keep(one_more, 2, 4, 1, 2)
    assert skipped == 1 and keep.tolist() == [0, 0, 1, 1, 0, 0, 1, 0]


def organized_cloud(rows, cols, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-6, 6, (rows * cols, 3)).astype(np.float32)
    p[rng.random(rows * cols) < 0.15] = np.nan               # no-return pixels
    p[::17, 1] = np.inf
    return p


@pytest.mark.parametrize("steps", [(2, 2), (1, 10), (3, 5)])
def test_nan_fill_equals_compaction(steps):
    """The device compacts where ExtractIndices fills with NaN: the crop box and the voxel grid only ever
    see the finite points in their original order, so both give the same bits, in both summation orders
    and through the oracle's filters."""
    rows, cols = 24, 50
    p = organized_cloud(rows, cols, 3)
    keep = D.extract_keep_organized(len(p), D.index_set(rows, cols, *steps))
    assert 0 < keep.sum() < len(p)
    filled, packed = D.nan_fill(p, keep), p[keep]
    assert len(filled) == len(p) and len(packed) == keep.sum()
    for crop in (0.0, 2.0):
        for leaf in (0.0, 0.5, 1.5):
            if crop == 0.0 and leaf == 0.0:
                continue          # no filter: the NaN points stay in one and never were in the other
            a, b = PR.preprocess(filled, crop, leaf), PR.preprocess(packed, crop, leaf)
            assert len(a) > 0
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
            np.testing.assert_array_equal(
                a.view(np.uint32), D.preprocess_downsampled(p, rows, cols, *steps, crop, leaf).view(np.uint32))
            if leaf > 0:
                va, vb = PO.voxel_grid(filled, leaf, crop), PO.voxel_grid(packed, leaf, crop)
                np.testing.assert_array_equal(va[0].view(np.uint32), vb[0].view(np.uint32))
                np.testing.assert_array_equal(va[1], vb[1])
            oa = O.crop_box_negative(filled, crop) if crop > 0 else filled
            ob = O.crop_box_negative(packed, crop) if crop > 0 else packed
            if leaf > 0:
                oa, ob = O.voxel_grid(oa, leaf), O.voxel_grid(ob, leaf)
            np.testing.assert_array_equal(oa.view(np.uint32), ob.view(np.uint32))


def test_static_cloud_downsampled_by_hand():
    xyz = np.arange(24, dtype=np.float32).reshape(8, 3) + 5
    xyz[3] = np.nan                                         # a no-return pixel keeps its position
    lab = np.array([0, 7, 0, 0, 0, 0, 0, 0])
    got = D.static_cloud_downsampled(xyz, lab, [7], 2, 4, 1, 2)
    np.testing.assert_array_equal(got, xyz[[0, 5, 7]])      # positions 0 2 4 6 = pixels 0 3 5 7, pixel 3 is NaN
    np.testing.assert_array_equal(D.static_cloud_downsampled(xyz, lab, [], 2, 4, 1, 2), xyz[[0, 2, 4, 6]])
    mask = lab == 7
    np.testing.assert_array_equal(D.static_cloud_downsampled(xyz, None, None, 2, 4, 1, 2, removed=mask), got)


NEW_SYMBOLS = ("ddlo_odom_set_downsampling", "ddlo_odom_get_downsampling", "ddlo_seg_set_downsampling",
               "ddlo_seg_get_downsampling", "ddlo_seg_downsampling_skipped", "ddlo_preprocess_downsampled",
               "ddlo_debug_downsample_keep")


def test_new_symbols_are_exported_and_bound():
    path = P.lib_path()
    assert os.path.exists(path), "build the library first (make lib)"
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    missing = [n for n in NEW_SYMBOLS if n not in exported]
    assert not missing, f"not exported: {missing}"
    S._lib()
    lib = OD._lib()
    for n in NEW_SYMBOLS:
        assert getattr(lib, n).argtypes is not None, n
    inc = os.path.join(ROOT, "include")
    assert '#include "ddlo_downsample.h"' in open(os.path.join(inc, "ddlo_segment.h")).read()
    hdr = "".join(open(os.path.join(inc, h)).read() for h in ("ddlo_downsample.h", "ddlo_odom.h"))
    for n in NEW_SYMBOLS:
        assert n + "(" in hdr, n


def test_null_handles_and_bad_arguments():
    L = OD._lib()
    S._lib()
    i = C.c_int()
    n = C.c_size_t()
    assert L.ddlo_odom_set_downsampling(None, 1, 2, 2, 8, 8) == 1           # GICP_EINVAL
    assert L.ddlo_odom_get_downsampling(None, C.byref(i), None, None, None, None) == 1
    assert L.ddlo_seg_set_downsampling(None, 1, 2, 2) == 1
    assert L.ddlo_seg_get_downsampling(None, C.byref(i), None, None) == 1
    assert L.ddlo_seg_downsampling_skipped(None, C.byref(i)) == 1
    one = np.zeros((1, 3), np.float32)
    assert L.ddlo_preprocess_downsampled(0, P._ptr(one), 1, 12, 1, 1, 0, 1, 0.0, 0.0, 0, None, 0, C.byref(n)) == 1
    assert L.ddlo_preprocess_downsampled(0, P._ptr(one), 1, 12, 1, 1, 1, 1, 0.0, 0.0, 0, None, 0, None) == 1
    f = np.zeros(4, np.uint8)
    k = np.zeros(4, np.uint8)
    assert L.ddlo_debug_downsample_keep(0, None, 4, 2, 2, 1, 1, P._ptr(k), None) == 1
    assert L.ddlo_debug_downsample_keep(0, P._ptr(f), 4, 2, 2, 0, 1, P._ptr(k), None) == 1
    assert L.ddlo_debug_downsample_keep(0, P._ptr(f), 5, 2, 2, 1, 1, P._ptr(k), None) == 1   # n != rows * cols
