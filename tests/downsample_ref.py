"""Plain numpy restatement of the organized-scan row/column filter
(include/ddlo_downsample.h; odom.cc:125-130, 219-223, 445-455, 902-906).
Test helper only.

The reference builds one index set S for a rows x cols image and runs one
pcl::ExtractIndices (keep-organized, PCL 1.10) with it twice:
  registration pass  over the organized scan, before the crop box and the voxel filter;
  keyframe pass      over the compacted cloud left after the non-static pixels were extracted
                     (no keep-organized there): position j of that cloud stays if j is in S.
ExtractIndices on n points: |S| > n -> "indices size exceeds the size of the input", the input passes
unchanged; otherwise every position outside S becomes NaN (indices >= n have no effect), n points stay.
"""
import numpy as np

import objects_ref as R
import preprocess_ref as PR
from oracle import odom_ref


def index_set(rows, cols, row_step, col_step):
    """S, ascending (odom.cc:125-130 builds it row by row, column by column: already ascending)."""
    return np.array([r * cols + c for r in range(0, rows, row_step) for c in range(0, cols, col_step)], np.int64)


def extract_skipped(n, S):
    return len(S) > n


def extract_keep_organized(n, S):
    """Keep mask (bool[n]) of ExtractIndices, normal mode, keep-organized: True where the point stays as
    it is, False where it becomes NaN.  |S| > n: everything stays."""
    if extract_skipped(n, S):
        return np.ones(n, bool)
    keep = np.zeros(n, bool)
    S = np.asarray(S, np.int64)
    keep[S[S < n]] = True
    return keep


def nan_fill(points, keep):
    """What ExtractIndices leaves: the points outside the mask NaN, the count unchanged."""
    p = PR._xyz(points).copy()
    p[~np.asarray(keep, bool)] = np.nan
    return p


def preprocess_downsampled(points, rows, cols, row_step, col_step, crop=0.0, leaf=0.0):
    """The registration pass as the device runs it: mask, compress, then preprocess_ref.preprocess."""
    p = PR._xyz(points)
    keep = extract_keep_organized(len(p), index_set(rows, cols, row_step, col_step))
    return PR.preprocess(p[keep], crop, leaf)


def keyframe_keep(removed, rows, cols, row_step, col_step):
    """The keyframe pass per pixel: (keep uint8[rows * cols], skipped).  keep[p] = 1 if pixel p was not
    removed and its position in the compacted cloud survives ExtractIndices."""
    removed = np.asarray(removed).reshape(-1) != 0
    assert len(removed) == rows * cols
    left = np.flatnonzero(~removed)                   # position j holds pixel left[j]
    S = index_set(rows, cols, row_step, col_step)
    keep = np.zeros(len(removed), np.uint8)
    keep[left[extract_keep_organized(len(left), S)]] = 1
    return keep, int(extract_skipped(len(left), S))


def static_cloud_downsampled(xyz_t, label, remove_ids, rows, cols, row_step, col_step, centre=(0, 0, 0), crop_size=0.0,
                             leaf=0.0, removed=None):
    """objects_ref.static_cloud with the keyframe pass between the removal and the crop.  removed
    (optional): the removed pixels as a mask (the union of the tracks' lists) instead of remove_ids."""
    xyz = np.ascontiguousarray(np.asarray(xyz_t, np.float32)[:, :3])
    if removed is None:
        removed = np.isin(np.asarray(label).reshape(-1), np.asarray(list(remove_ids), np.int64))
    keep, _ = keyframe_keep(removed, rows, cols, row_step, col_step)
    return R.static_cloud(nan_fill(xyz, keep), np.zeros(len(xyz), np.int64), [], centre, crop_size, leaf)


class OdomRefDownsampled(odom_ref.OdomRef):
    """OdomRef with the registration pass in front of its preprocessing."""

    def __init__(self, params, rows, cols, row_step, col_step, threads=0):
        super().__init__(params, threads)
        self.S = index_set(rows, cols, row_step, col_step)

    def _preprocess(self, pts):
        p = PR._xyz(pts)
        return super()._preprocess(p[extract_keep_organized(len(p), self.S)])
