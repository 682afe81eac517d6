"""ctypes mirror of the odometry driver C-ABI (include/ddlo_odom.h).

``Odometry`` is the registration half of the reference's ``OdomNode``
(``src/odometry/odom.cc``): per scan the device preprocessing (crop box +
voxel filter), the spaciousness metric and adaptive keyframe threshold, S2S
then S2M GICP with pose propagation, keyframe selection and the
k-nearest / convex-hull / concave-hull submap, all point sets on the GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import GicpError, GicpParams, GicpResult, _ptr, load
from .segmentation import (OBJECT_DTYPE, ClassCounts, ProjectionParams, ProjectionResult, SegObject, SegResult,
                           Segmentation)

__all__ = ["OdomParams", "OdomResult", "DynamicParams", "NONSTATIC_FN", "Odometry", "default_odom_params",
           "default_dynamic_params", "preprocess", "DeskewParams", "deskew", "se3_split_log", "TIME_F32_S", "TIME_U32_NS",
           "TIME_F64_S", "median_range", "convex_hull", "concave_hull", "TRACKED", "FIRST", "SKIPPED", "INIT"]

TRACKED, FIRST, SKIPPED, INIT = 0, 1, 2, 3


class OdomParams(C.Structure):
    _fields_ = [
        ("s2s", GicpParams),
        ("s2m", GicpParams),
        ("min_num_points", C.c_int32),
        ("keyframe_thresh_dist", C.c_double),
        ("keyframe_thresh_rot", C.c_double),
        ("submap_knn", C.c_int32),
        ("submap_kcv", C.c_int32),
        ("submap_kcc", C.c_int32),
        ("adaptive", C.c_int32),
        ("crop_use", C.c_int32),
        ("crop_size", C.c_double),
        ("vf_scan_use", C.c_int32),
        ("vf_scan_res", C.c_double),
        ("vf_submap_use", C.c_int32),
        ("vf_submap_res", C.c_double),
        ("skip_first_scan", C.c_int32),
        ("s2m_target_grid", C.c_int32),
    ]


class OdomResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("scan_points", C.c_int32),
        ("T", C.c_float * 16),
        ("T_s2s", C.c_float * 16),
        ("T_s2s_local", C.c_float * 16),
        ("s2s", GicpResult),
        ("s2m", GicpResult),
        ("keyframe_added", C.c_int32),
        ("submap_changed", C.c_int32),
        ("num_keyframes", C.c_int32),
        ("submap_keyframes", C.c_int32),
        ("submap_points", C.c_int64),
        ("spaciousness", C.c_double),
        ("keyframe_thresh_dist", C.c_double),
    ]

    def pose(self) -> np.ndarray:
        return np.array(self.T, dtype=np.float32).reshape(4, 4)


class DynamicParams(C.Structure):
    """ddlo_dynamic_params."""
    _fields_ = [("theta_min", C.c_double), ("theta_max", C.c_double), ("max_dim_ratio", C.c_float)]


# ddlo_nonstatic_fn: int (*)(void* user, const ddlo_seg_object* objs, size_t n, uint8_t* non_static)
NONSTATIC_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(SegObject), C.c_size_t, C.POINTER(C.c_uint8))


# ddlo_voxel_order: the order a voxel filter sums a voxel's points in
VOXEL_ORDER_INPUT, VOXEL_ORDER_PCL = 0, 1


class SortOrderStats(C.Structure):
    """ddlo_sort_order_stats."""
    _fields_ = [("levels", C.c_int32), ("global_levels", C.c_int32), ("lds_segments", C.c_int32),
                ("heap_segments", C.c_int32), ("heap_longest", C.c_int32), ("threshold", C.c_int32)]


# ddlo_time_type: the per-point time field of the deskew (include/ddlo_deskew.h)
TIME_F32_S, TIME_U32_NS, TIME_F64_S = 0, 1, 2


class DeskewParams(C.Structure):
    """ddlo_deskew_params."""
    _fields_ = [("use", C.c_int32), ("time_type", C.c_int32), ("time_offset_bytes", C.c_size_t),
                ("ref_time", C.c_double), ("period", C.c_double)]


_SIGS_DONE = False


def _lib():
    global _SIGS_DONE
    L = load()
    if not _SIGS_DONE:
        P, S, I, D = C.c_void_p, C.c_size_t, C.c_int, C.c_double
        sig = {
            "ddlo_odom_default_params": (I, [C.POINTER(OdomParams)]),
            "ddlo_odom_create": (I, [I, C.POINTER(OdomParams), C.POINTER(P)]),
            "ddlo_odom_destroy": (I, [P]),
            "ddlo_odom_process": (I, [P, P, S, S, C.POINTER(OdomResult)]),
            "ddlo_odom_keyframe": (I, [P, I, P, C.POINTER(S)]),
            "ddlo_odom_keyframe_points": (I, [P, I, P, S, C.POINTER(S)]),
            "ddlo_dynamic_default_params": (I, [C.POINTER(DynamicParams)]),
            "ddlo_odom_process_dynamic": (I, [P, P, P, S, C.POINTER(DynamicParams), NONSTATIC_FN, P,
                                              C.POINTER(OdomResult), C.POINTER(SegResult)]),
            "ddlo_odom_process_tracked": (I, [P, P, P, P, P, S, D, C.POINTER(DynamicParams), C.POINTER(OdomResult),
                                              C.POINTER(SegResult), P]),
            "ddlo_odom_process_dynamic_cloud": (I, [P, P, P, S, S, C.POINTER(DynamicParams), NONSTATIC_FN, P,
                                                    C.POINTER(ProjectionParams), C.POINTER(OdomResult),
                                                    C.POINTER(SegResult), C.POINTER(ProjectionResult)]),
            "ddlo_odom_process_tracked_cloud": (I, [P, P, P, P, P, S, S, D, C.POINTER(DynamicParams),
                                                    C.POINTER(ProjectionParams), C.POINTER(OdomResult),
                                                    C.POINTER(SegResult), P, C.POINTER(ProjectionResult)]),
            "ddlo_odom_classify": (I, [P, P, C.POINTER(ClassCounts)]),
            "ddlo_odom_submap": (I, [P, P, S, C.POINTER(S)]),
            "ddlo_odom_ctx": (I, [P, I, C.POINTER(P)]),
            "ddlo_preprocess": (I, [I, P, S, S, D, D, P, S, C.POINTER(S)]),
            "ddlo_preprocess_ordered": (I, [I, P, S, S, D, D, I, P, S, C.POINTER(S)]),
            "ddlo_odom_set_voxel_order": (I, [P, I]),
            "ddlo_odom_get_voxel_order": (I, [P, C.POINTER(I)]),
            "ddlo_debug_sort_order": (I, [I, P, S, P, C.POINTER(SortOrderStats)]),
            "ddlo_odom_set_downsampling": (I, [P, I, I, I, I, I]),
            "ddlo_odom_get_downsampling": (I, [P] + [C.POINTER(I)] * 5),
            "ddlo_preprocess_downsampled": (I, [I, P, S, S, I, I, I, I, D, D, I, P, S, C.POINTER(S)]),
            "ddlo_debug_downsample_keep": (I, [I, P, S, I, I, I, I, P, C.POINTER(I)]),
            "ddlo_odom_set_intensity": (I, [P, I, S]),
            "ddlo_odom_get_intensity": (I, [P, C.POINTER(I), C.POINTER(S)]),
            "ddlo_odom_keyframe_points_xyzi": (I, [P, I, P, S, C.POINTER(S)]),
            "ddlo_preprocess_xyzi": (I, [I, P, S, S, S, D, D, I, P, S, C.POINTER(S)]),
            "ddlo_odom_set_deskew": (I, [P, C.POINTER(DeskewParams)]),
            "ddlo_odom_get_deskew": (I, [P, C.POINTER(DeskewParams)]),
            "ddlo_odom_set_deskew_motion": (I, [P, P, P]),
            "ddlo_odom_deskew_motion": (I, [P, P, P, C.POINTER(I)]),
            "ddlo_se3_split_log": (I, [P, P, P]),
            "ddlo_deskew": (I, [I, P, S, S, C.POINTER(DeskewParams), P, P, P]),
            "ddlo_debug_deskew_time": (I, [I, P, S, S, C.POINTER(DeskewParams), P, P, I, P]),
            "ddlo_median_range": (I, [I, P, S, S, C.POINTER(C.c_float)]),
            "ddlo_convex_hull": (I, [P, I, P, I, C.POINTER(I)]),
            "ddlo_concave_hull": (I, [P, I, D, P, I, C.POINTER(I)]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _SIGS_DONE = True
    return L


def _check(st):
    if st != 0:
        raise GicpError(st, load().gicp_last_error().decode())


def default_odom_params(**kw) -> OdomParams:
    """cfg/ddlo.yaml defaults (odom.cc:196-252)."""
    p = OdomParams()
    _check(_lib().ddlo_odom_default_params(C.byref(p)))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_dynamic_params(**kw) -> DynamicParams:
    """The residual image's window (odom.cc:804-805) and detection/maxDimRatio."""
    p = DynamicParams()
    _check(_lib().ddlo_dynamic_default_params(C.byref(p)))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _xyz(points) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3))


def _records(points):
    """Point records as (contiguous array, n, stride): (n, c) float32 rows, (n, stride) uint8 rows or a 1-D
    structured array; x, y, z float32 first in each."""
    a = np.asarray(points)
    if a.dtype.names is not None and a.ndim == 1:
        a = np.ascontiguousarray(a)
        return a, a.shape[0], a.dtype.itemsize
    if a.dtype == np.uint8 and a.ndim == 2:
        a = np.ascontiguousarray(a)
        return a, a.shape[0], a.shape[1]
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("records must be (n, >=3) float32, (n, stride) uint8 or a structured array")
    return a, a.shape[0], a.shape[1] * 4


def _vec3(v):
    a = np.ascontiguousarray(v, np.float64).reshape(-1)
    if a.shape[0] != 3:
        raise ValueError("a twist half has 3 components")
    return a


class Odometry:
    """OdomNode registration pipeline on one GPU."""

    def __init__(self, device: int = 0, params: OdomParams | None = None):
        self.L = _lib()
        self.h = C.c_void_p()
        self._intensity = False     # set_intensity's flag, kept here so that process() asks nothing per frame
        self._deskew = False        # set_deskew's, likewise
        _check(self.L.ddlo_odom_create(device, C.byref(params) if params is not None else None, C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.ddlo_odom_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_voxel_order(self, order: int):
        """ddlo_odom_set_voxel_order: VOXEL_ORDER_INPUT (default) or VOXEL_ORDER_PCL for the scan and the
        keyframe voxel filters, from the next scan on.  The dynamic and tracked entries build keyframes
        through the Segmentation handle too: set it there as well."""
        _check(self.L.ddlo_odom_set_voxel_order(self.h, int(order)))

    @property
    def voxel_order(self) -> int:
        m = C.c_int()
        _check(self.L.ddlo_odom_get_voxel_order(self.h, C.byref(m)))
        return m.value

    def set_downsampling(self, use, row_step: int, col_step: int, rows: int, cols: int):
        """ddlo_odom_set_downsampling: the organized-scan row/column filter (preprocessing/downsampling
        {use, row, col}, detection {rows, columns}) in front of the crop box and the voxel filter, from the
        next scan on.  With it on, scans have rows * cols points, and the dynamic and tracked entries want
        the same setting on the Segmentation handle (Segmentation.set_downsampling)."""
        _check(self.L.ddlo_odom_set_downsampling(self.h, int(bool(use)), int(row_step), int(col_step), int(rows),
                                                 int(cols)))

    def downsampling(self):
        """(use, row_step, col_step, rows, cols) as set."""
        v = [C.c_int() for _ in range(5)]
        _check(self.L.ddlo_odom_get_downsampling(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def set_intensity(self, use, offset_bytes: int = 12):
        """ddlo_odom_set_intensity: carry the float at offset_bytes of every point record (12: packed
        x y z i rows; 16: pcl::PointXYZI) through the filters into the keyframes.  With it on, process()
        takes (n, >= 4) float32 rows, and the row size is the stride.  Not after the first keyframe."""
        _check(self.L.ddlo_odom_set_intensity(self.h, int(bool(use)), int(offset_bytes)))
        self._intensity = bool(use)

    @property
    def intensity(self):
        """(use, offset_bytes) as set."""
        u, off = C.c_int(), C.c_size_t()
        _check(self.L.ddlo_odom_get_intensity(self.h, C.byref(u), C.byref(off)))
        return bool(u.value), off.value

    def set_deskew(self, use, time_offset: int = 12, time_type: int = TIME_F32_S, ref_time: float = 0.0,
                   period: float = 0.1):
        """ddlo_odom_set_deskew (include/ddlo_deskew.h): from the next scan on, every point is moved from the
        sensor frame at its own capture time into the sensor frame at ref_time before anything reads it.  The
        time is the field at time_offset bytes of each record (TIME_F32_S, TIME_U32_NS or TIME_F64_S), ref_time
        is on the same clock, period is what the twist spans.  With it on, process() takes records: (n, c)
        float32 rows (a uint32 time viewed as float32 keeps its bits), (n, stride) uint8 rows or a structured
        array; the dynamic entries take float32 rows.  ref_time usually changes with every scan."""
        p = DeskewParams(int(bool(use)), int(time_type), int(time_offset), float(ref_time), float(period))
        _check(self.L.ddlo_odom_set_deskew(self.h, C.byref(p)))
        self._deskew = bool(use)

    def deskew(self) -> DeskewParams:
        """The setting, as a DeskewParams."""
        p = DeskewParams()
        _check(self.L.ddlo_odom_get_deskew(self.h, C.byref(p)))
        return p

    def set_deskew_motion(self, omega=None, t=None):
        """ddlo_odom_set_deskew_motion: the caller's twist (rotation vector rad, translation m, over one period,
        in the frame of the reference instant) for the next scan that is uploaded, and for that scan only;
        None clears a pending one.  Without one, a deskewing driver predicts from its last two poses."""
        if omega is None or t is None:
            _check(self.L.ddlo_odom_set_deskew_motion(self.h, None, None))
            return
        w, v = _vec3(omega), _vec3(t)
        _check(self.L.ddlo_odom_set_deskew_motion(self.h, _ptr(w), _ptr(v)))

    def deskew_motion(self):
        """(omega, t, source) applied to the last scan: source 0 none, 1 predicted, 2 the caller's."""
        w, v, src = np.zeros(3), np.zeros(3), C.c_int()
        _check(self.L.ddlo_odom_deskew_motion(self.h, _ptr(w), _ptr(v), C.byref(src)))
        return w, v, src.value

    def process(self, points) -> OdomResult:
        r = OdomResult()
        if self._deskew:
            a, n, stride = _records(points)
            _check(self.L.ddlo_odom_process(self.h, _ptr(a) if n else None, n, stride, C.byref(r)))
            return r
        if self._intensity:
            a = np.ascontiguousarray(points, np.float32)
            if a.ndim != 2 or a.shape[1] < 4:
                raise ValueError("with intensity on, points must be (n, >=4)")
            _check(self.L.ddlo_odom_process(self.h, _ptr(a) if a.shape[0] else None, a.shape[0], a.shape[1] * 4,
                                            C.byref(r)))
            return r
        a = _xyz(points)
        _check(self.L.ddlo_odom_process(self.h, _ptr(a), a.shape[0], 12, C.byref(r)))
        return r

    def process_dynamic(self, seg: Segmentation, scan, decide=None, params: DynamicParams | None = None):
        """ddlo_odom_process_dynamic: one organized sensor-frame scan (seg's rows*cols points, NaN = no
        return).  decide(objects) -> iterable of truth values, one per object (true: cut it out), or
        None to abort; objects is an OBJECT_DTYPE array.  decide=None: every object is non-static.
        Returns (OdomResult, SegResult)."""
        a = np.ascontiguousarray(scan, np.float32)
        if a.ndim != 2 or a.shape[0] != seg.params.rows * seg.params.cols or a.shape[1] < 3:
            raise ValueError("scan must be (rows*cols, >=3)")
        return self._process_dynamic(seg, a, decide, params, False, None)

    def _process_dynamic(self, seg, a, decide, params, cloud, projection):
        raised = []

        def trampoline(_user, objs, n, flags):
            try:
                arr = np.zeros(n, OBJECT_DTYPE)
                if n:
                    C.memmove(arr.ctypes.data, objs, n * C.sizeof(SegObject))
                verdict = decide(arr)
                if verdict is None:
                    return 1
                verdict = list(verdict)
                if len(verdict) != n:
                    raise ValueError("decide must return one verdict per object")
                for i, v in enumerate(verdict):
                    flags[i] = 1 if v else 0
                return 0
            except BaseException as e:   # never unwind through the C frames
                raised.append(e)
                return 1

        cb = NONSTATIC_FN(trampoline) if decide is not None else C.cast(None, NONSTATIC_FN)
        r, sr = OdomResult(), SegResult()
        if cloud:
            pr = ProjectionResult()
            st = self.L.ddlo_odom_process_dynamic_cloud(self.h, seg.h, _ptr(a) if a.shape[0] else None, a.shape[1] * 4,
                                                        a.shape[0], C.byref(params) if params is not None else None,
                                                        cb, None, C.byref(projection) if projection is not None else None,
                                                        C.byref(r), C.byref(sr), C.byref(pr))
        else:
            st = self.L.ddlo_odom_process_dynamic(self.h, seg.h, _ptr(a), a.shape[1] * 4,
                                                  C.byref(params) if params is not None else None, cb, None,
                                                  C.byref(r), C.byref(sr))
        if raised:
            raise raised[0]
        _check(st)
        seg.last = sr
        return (r, sr, pr) if cloud else (r, sr)

    def process_dynamic_cloud(self, seg: Segmentation, points, decide=None, params: DynamicParams | None = None,
                              projection: ProjectionParams | None = None):
        """ddlo_odom_process_dynamic_cloud: process_dynamic for an unorganized sensor-frame cloud (n, >=3):
        every point registers; the image is the cloud's projection (projection None: the defaults of seg's
        parameters).  Returns (OdomResult, SegResult, ProjectionResult); seg.projection_maps() and, after a
        classification, seg.point_classes() answer in the indices of points."""
        a = np.ascontiguousarray(points, np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("points must be (n, >=3)")
        return self._process_dynamic(seg, a, decide, params, True, projection)

    def process_tracked_cloud(self, seg: Segmentation, tracker, points, stamp: float, map=None,
                              params: DynamicParams | None = None, projection: ProjectionParams | None = None):
        """ddlo_odom_process_tracked_cloud: process_tracked for an unorganized sensor-frame cloud (n, >=3).
        Returns (OdomResult, SegResult, TrackResult, ProjectionResult)."""
        from .tracking import TrackResult
        a = np.ascontiguousarray(points, np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("points must be (n, >=3)")
        r, sr, tr, pr = OdomResult(), SegResult(), TrackResult(), ProjectionResult()
        _check(self.L.ddlo_odom_process_tracked_cloud(
            self.h, seg.h, tracker.h, map.h if map is not None else None, _ptr(a) if a.shape[0] else None,
            a.shape[1] * 4, a.shape[0], float(stamp), C.byref(params) if params is not None else None,
            C.byref(projection) if projection is not None else None, C.byref(r), C.byref(sr), C.byref(tr),
            C.byref(pr)))
        seg.last = sr
        tracker.last = tr
        return r, sr, tr, pr

    def process_tracked(self, seg: Segmentation, tracker, scan, stamp: float, map=None,
                        params: DynamicParams | None = None):
        """ddlo_odom_process_tracked: process_dynamic with the tracker (tracking.Tracker) on board: its
        UNDEFINED and DYNAMIC tracks' pixel lists, stale ones included, are cut out of the keyframe; with a
        map (mapping.Map) the boxes of tracks that turned dynamic are cleared from it and new keyframes
        added.  stamp: the scan's time in seconds.  Returns (OdomResult, SegResult, TrackResult)."""
        from .tracking import TrackResult
        a = np.ascontiguousarray(scan, np.float32)
        if a.ndim != 2 or a.shape[0] != seg.params.rows * seg.params.cols or a.shape[1] < 3:
            raise ValueError("scan must be (rows*cols, >=3)")
        r, sr, tr = OdomResult(), SegResult(), TrackResult()
        _check(self.L.ddlo_odom_process_tracked(self.h, seg.h, tracker.h, map.h if map is not None else None, _ptr(a),
                                                a.shape[1] * 4, float(stamp), C.byref(params) if params is not None else None,
                                                C.byref(r), C.byref(sr), C.byref(tr)))
        seg.last = sr
        tracker.last = tr
        return r, sr, tr

    def classify(self, seg: Segmentation, tracker) -> ClassCounts:
        """ddlo_odom_classify: the classes of the last scan's pixels from the tracker's live filters, after a
        process_tracked that returned TRACKED.  Read them with seg.class_image(), seg.class_indices(),
        seg.frame_clouds().  Returns the counts."""
        c = ClassCounts()
        _check(self.L.ddlo_odom_classify(seg.h, tracker.h, C.byref(c)))
        return c

    def keyframe_points(self, k: int, intensity: bool = False) -> np.ndarray:
        """World-frame points of keyframe k (after the submap voxel filter), (n, 3) float32; intensity=True
        (a driver with set_intensity on): (n, 4), the same rows with their intensity."""
        n = C.c_size_t()
        if intensity:
            _check(self.L.ddlo_odom_keyframe_points_xyzi(self.h, k, None, 0, C.byref(n)))
            out = np.zeros((max(n.value, 1), 4), np.float32)
            _check(self.L.ddlo_odom_keyframe_points_xyzi(self.h, k, _ptr(out), out.shape[0], C.byref(n)))
            return out[:n.value]
        _check(self.L.ddlo_odom_keyframe_points(self.h, k, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 3), np.float32)
        _check(self.L.ddlo_odom_keyframe_points(self.h, k, _ptr(out), out.shape[0], C.byref(n)))
        return out[:n.value]

    def keyframe(self, k: int):
        pose = (C.c_float * 7)()
        n = C.c_size_t()
        _check(self.L.ddlo_odom_keyframe(self.h, k, pose, C.byref(n)))
        return np.array(pose, dtype=np.float32), n.value

    def submap(self) -> np.ndarray:
        n = C.c_size_t()
        _check(self.L.ddlo_odom_submap(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.int32)
        _check(self.L.ddlo_odom_submap(self.h, _ptr(out), out.size, C.byref(n)))
        return out[:n.value]


def preprocess(points, crop_size: float = 0.0, leaf: float = 0.0, device: int = 0,
               order: int = VOXEL_ORDER_INPUT, intensity_offset: int | None = None) -> np.ndarray:
    """Device crop box (points inside [-s, s]^3 removed) then voxel filter.  order: the voxel filter sums
    each voxel's points in input order (VOXEL_ORDER_INPUT) or in pcl::VoxelGrid's (VOXEL_ORDER_PCL).
    intensity_offset: ddlo_preprocess_xyzi on (n, c) float32 rows (the stride is the row size) whose
    intensity is the float at that byte offset; returns (m, 4): x, y, z, intensity."""
    if intensity_offset is not None:
        a = np.ascontiguousarray(points, np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("points must be (n, >=3)")
        out = np.zeros((max(a.shape[0], 1), 4), np.float32)
        n = C.c_size_t()
        _check(_lib().ddlo_preprocess_xyzi(device, _ptr(a) if a.shape[0] else None, a.shape[0], a.shape[1] * 4,
                                           int(intensity_offset), float(crop_size), float(leaf), int(order),
                                           _ptr(out), out.shape[0], C.byref(n)))
        return out[:n.value]
    a = _xyz(points)
    out = np.zeros((max(a.shape[0], 1), 3), np.float32)
    n = C.c_size_t()
    if order == VOXEL_ORDER_INPUT:
        _check(_lib().ddlo_preprocess(device, _ptr(a), a.shape[0], 12, float(crop_size), float(leaf), _ptr(out),
                                      out.shape[0], C.byref(n)))
    else:
        _check(_lib().ddlo_preprocess_ordered(device, _ptr(a), a.shape[0], 12, float(crop_size), float(leaf),
                                              int(order), _ptr(out), out.shape[0], C.byref(n)))
    return out[:n.value]


def deskew(records, omega, t, time_offset: int, time_type: int = TIME_F32_S, ref_time: float = 0.0,
           period: float = 0.1, device: int = 0) -> np.ndarray:
    """ddlo_deskew: the deskew pass on its own.  records as Odometry.set_deskew describes them; returns the
    (n, 3) float32 points in the sensor frame at ref_time."""
    a, n, stride = _records(records)
    p = DeskewParams(1, int(time_type), int(time_offset), float(ref_time), float(period))
    w, v = _vec3(omega), _vec3(t)
    out = np.zeros((max(n, 1), 3), np.float32)
    _check(_lib().ddlo_deskew(device, _ptr(a) if n else None, n, stride, C.byref(p), _ptr(w), _ptr(v), _ptr(out)))
    return out[:n]


def deskew_time(records, omega, t, time_offset: int, time_type: int = TIME_F32_S, ref_time: float = 0.0,
                period: float = 0.1, reps: int = 100, device: int = 0) -> np.ndarray:
    """ddlo_debug_deskew_time: the device time of the deskew pass alone in milliseconds, reps times, each behind
    a fresh upload of the records."""
    a, n, stride = _records(records)
    p = DeskewParams(1, int(time_type), int(time_offset), float(ref_time), float(period))
    w, v = _vec3(omega), _vec3(t)
    ms = np.zeros(int(reps), np.float32)
    _check(_lib().ddlo_debug_deskew_time(device, _ptr(a), n, stride, C.byref(p), _ptr(w), _ptr(v), int(reps), _ptr(ms)))
    return ms


def se3_split_log(T):
    """ddlo_se3_split_log: (omega, t) of a 4x4 transform taken as float32: the rotation vector of its 3x3 block
    and its translation column."""
    a = np.ascontiguousarray(T, np.float32).reshape(16)
    w, v = np.zeros(3), np.zeros(3)
    _check(_lib().ddlo_se3_split_log(_ptr(a), _ptr(w), _ptr(v)))
    return w, v


def preprocess_downsampled(points, rows: int, cols: int, row_step: int, col_step: int, crop_size: float = 0.0,
                           leaf: float = 0.0, device: int = 0, order: int = VOXEL_ORDER_INPUT) -> np.ndarray:
    """ddlo_preprocess_downsampled: the row/column filter's registration pass over the points taken as the
    first pixels of a rows x cols image, then preprocess()."""
    a = _xyz(points)
    out = np.zeros((max(a.shape[0], 1), 3), np.float32)
    n = C.c_size_t()
    _check(_lib().ddlo_preprocess_downsampled(device, _ptr(a), a.shape[0], 12, int(rows), int(cols), int(row_step),
                                              int(col_step), float(crop_size), float(leaf), int(order), _ptr(out),
                                              out.shape[0], C.byref(n)))
    return out[:n.value]


def downsample_keep(removed, rows: int, cols: int, row_step: int, col_step: int, device: int = 0):
    """ddlo_debug_downsample_keep: (keep uint8[rows * cols], skipped) of the row/column filter's keyframe pass
    over an image whose pixels flagged in `removed` were extracted before it."""
    f = np.ascontiguousarray(removed, dtype=np.uint8).reshape(-1)
    keep = np.zeros(max(f.shape[0], 1), np.uint8)
    sk = C.c_int()
    _check(_lib().ddlo_debug_downsample_keep(device, _ptr(f) if f.shape[0] else None, f.shape[0], int(rows), int(cols),
                                             int(row_step), int(col_step), _ptr(keep), C.byref(sk)))
    return keep[:f.shape[0]], sk.value


def sort_order(keys, device: int = 0):
    """ddlo_debug_sort_order: (perm, stats) of std::sort on the pairs (keys[i], i) compared by key alone,
    computed on the device: perm[r] is the original index at rank r; stats is a SortOrderStats."""
    k = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
    perm = np.zeros(max(k.shape[0], 1), np.int32)
    st = SortOrderStats()
    _check(_lib().ddlo_debug_sort_order(device, _ptr(k) if k.shape[0] else None, k.shape[0], _ptr(perm), C.byref(st)))
    return perm[:k.shape[0]], st


def median_range(points, stride: int = 12, device: int = 0) -> float:
    """Element n // 2 of the sorted ranges of the points (the spaciousness metric's median), no preprocessing.
    stride 12: anything that reshapes to (n, 3); else a float32 array of (n, stride // 4) columns, xyz first."""
    if stride == 12:
        a = _xyz(points)
    else:
        a = np.ascontiguousarray(points, np.float32)
        if a.ndim != 2 or a.shape[1] * 4 != stride:
            raise ValueError("points must be (n, stride // 4) float32")
    m = C.c_float()
    _check(_lib().ddlo_median_range(device, _ptr(a), a.shape[0], stride, C.byref(m)))
    return np.float32(m.value)


def convex_hull(points) -> np.ndarray:
    a = _xyz(points)
    idx = np.zeros(max(a.shape[0], 1), np.int32)
    n = C.c_int()
    _check(_lib().ddlo_convex_hull(_ptr(a), a.shape[0], _ptr(idx), idx.shape[0], C.byref(n)))
    return idx[:n.value]


def concave_hull(points, alpha: float) -> np.ndarray:
    a = _xyz(points)
    idx = np.zeros(max(a.shape[0], 1), np.int32)
    n = C.c_int()
    _check(_lib().ddlo_concave_hull(_ptr(a), a.shape[0], float(alpha), _ptr(idx), idx.shape[0], C.byref(n)))
    return idx[:n.value]
