"""ctypes mirror of the range-image segmentation C-ABI (include/ddlo_segment.h).

``Segmentation`` is the part of the reference's ``DetectionModule``
(``src/detection/detection.cpp``) that OdomNode::applySegmentation drives
(``odom.cc:853-857``): projectScan, projectResiduals, groundRemoval and
cloudSegmentation / labelComponents on one organized scan.  The per-pixel
passes run on the GPU; the labelling on the host (the default: the reference's
breadth-first search, literally) or on the GPU (``labelling="device"``: the
same labels and segment count, average residuals summed in double in row-major
order).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import GicpError, _ptr, load

__all__ = ["SegParams", "SegResult", "SegObject", "OBJECT_DTYPE", "Segmentation", "default_seg_params",
           "yaml_seg_params", "label_components", "label_components_device", "objects_from", "LABELLING", "EXCLUDED", "UNLABELLED", "REJECTED",
           "ClassCounts", "FrameClouds", "CLS_VALID", "CLS_GROUND", "CLS_UNDEFINED", "CLS_STATIC", "CLS_DYNAMIC",
           "CLS_NON_STATIC", "ProjectionParams", "ProjectionResult", "default_projection"]

EXCLUDED, UNLABELLED, REJECTED = -1, 0, 999999
LABELLING = {"host": 0, "device": 1}   # DDLO_SEG_LABEL_*
# DDLO_CLS_*: the bits of the class image (include/ddlo_seg_classes.h)
CLS_VALID, CLS_GROUND, CLS_UNDEFINED, CLS_STATIC, CLS_DYNAMIC = 1, 2, 4, 8, 16
CLS_NON_STATIC = CLS_UNDEFINED | CLS_DYNAMIC


class SegParams(C.Structure):
    _fields_ = [
        ("rows", C.c_int32),
        ("cols", C.c_int32),
        ("ang_bottom", C.c_float),
        ("ground_rows", C.c_int32),
        ("ground_angle_threshold", C.c_float),
        ("minimum_range", C.c_float),
        ("sensor_mount_angle", C.c_float),
        ("theta", C.c_float),
        ("valid_point_num", C.c_int32),
        ("min_line_num", C.c_int32),
        ("valid_line_num", C.c_int32),
        ("min_delta_z", C.c_float),
        ("max_delta_z", C.c_float),
        ("max_distance", C.c_float),
        ("max_elevation", C.c_float),
        ("win_row0", C.c_int32),
        ("win_row1", C.c_int32),
        ("win_col0", C.c_int32),
        ("win_col1", C.c_int32),
    ]

    def replace(self, **kw) -> "SegParams":
        q = SegParams()
        C.pointer(q)[0] = self
        for k, v in kw.items():
            setattr(q, k, v)
        return q


class SegResult(C.Structure):
    _fields_ = [
        ("segments", C.c_int32),
        ("ground_pixels", C.c_int32),
        ("range_pixels", C.c_int32),
        ("rejected_pixels", C.c_int32),
    ]


class SegObject(C.Structure):
    """ddlo_seg_object: one detected object (getObject / computeAllObjects)."""
    _fields_ = [
        ("id", C.c_int32),
        ("num_points", C.c_int32),
        ("state", C.c_float * 7),
        ("axis", C.c_float * 2),
        ("density", C.c_float),
        ("avg_residuum", C.c_double),
    ]


class ClassCounts(C.Structure):
    """ddlo_seg_class_counts: pixels per class bit; non_static = UNDEFINED or DYNAMIC; static_points = VALID
    and not non-static."""
    _fields_ = [(k, C.c_int32) for k in ("valid", "ground", "undefined", "static_tracks", "dynamic", "non_static",
                                         "static_points", "reserved")]


class ProjectionParams(C.Structure):
    """ddlo_seg_projection: elevation of row 0 and the step down to the next row (degrees, > 0), azimuth of
    column 0, and whether columns grow with atan2(y, x) (+1) or against it (-1)."""
    _fields_ = [("elev_top_deg", C.c_float), ("elev_res_deg", C.c_float), ("azim0_deg", C.c_float),
                ("azim_sign", C.c_int32)]


class ProjectionResult(C.Structure):
    """ddlo_seg_projection_result: points = invalid + out_of_view + occupied_pixels + collisions."""
    _fields_ = [(k, C.c_int32) for k in ("points", "invalid", "out_of_view", "occupied_pixels", "collisions")]


class _CloudOut(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("cap", C.c_size_t), ("n", C.c_size_t)]


class _FrameCloudsOut(C.Structure):
    _fields_ = [(k, _CloudOut) for k in ("ground", "non_static", "dynamic", "static_points")]


class FrameClouds:
    """applySegmentation's four clouds of one frame, each (m, 3) float32 in ascending pixel order."""

    def __init__(self, ground, non_static, dynamic, static_points):
        self.ground, self.non_static, self.dynamic, self.static_points = ground, non_static, dynamic, static_points

    def __iter__(self):
        return iter((self.ground, self.non_static, self.dynamic, self.static_points))


# the same layout as a numpy structured type (objects() returns such an array)
OBJECT_DTYPE = np.dtype([("id", np.int32), ("num_points", np.int32), ("state", np.float32, 7),
                         ("axis", np.float32, 2), ("density", np.float32), ("avg_residuum", np.float64)], align=True)


_SIGS_DONE = False


def _lib():
    global _SIGS_DONE
    L = load()
    if not _SIGS_DONE:
        P, S, I, F = C.c_void_p, C.c_size_t, C.c_int, C.c_float
        sig = {
            "ddlo_seg_default_params": (I, [C.POINTER(SegParams)]),
            "ddlo_seg_create": (I, [I, C.POINTER(SegParams), C.POINTER(P)]),
            "ddlo_seg_destroy": (I, [P]),
            "ddlo_seg_process": (I, [P, P, S, P, P, C.POINTER(SegResult)]),
            "ddlo_seg_images": (I, [P, P, P, P]),
            "ddlo_seg_avg_residuals": (I, [P, P, S, C.POINTER(S)]),
            "ddlo_seg_ground_indices": (I, [P, P, S, C.POINTER(S)]),
            "ddlo_seg_label_indices": (I, [P, P, S, P, S, C.POINTER(S)]),
            "ddlo_seg_label": (I, [C.POINTER(SegParams), P, P, P, F, P, P, S, C.POINTER(C.c_int32)]),
            "ddlo_seg_label_device": (I, [I, C.POINTER(SegParams), P, P, P, F, P, P, S, C.POINTER(C.c_int32)]),
            "ddlo_seg_set_labelling": (I, [P, I]),
            "ddlo_seg_get_labelling": (I, [P, C.POINTER(I)]),
            "ddlo_seg_set_voxel_order": (I, [P, I]),
            "ddlo_seg_get_voxel_order": (I, [P, C.POINTER(I)]),
            "ddlo_seg_set_downsampling": (I, [P, I, I, I]),
            "ddlo_seg_get_downsampling": (I, [P, C.POINTER(I), C.POINTER(I), C.POINTER(I)]),
            "ddlo_seg_downsampling_skipped": (I, [P, C.POINTER(I)]),
            "ddlo_seg_labelling_stats": (I, [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
            "ddlo_seg_objects": (I, [P, F, P, S, C.POINTER(S)]),
            "ddlo_seg_objects_from": (I, [I, P, S, I, I, P, P, S, F, P, S, C.POINTER(S)]),
            "ddlo_seg_static_cloud": (I, [P, P, S, P, C.c_double, C.c_double, P, S, C.POINTER(S)]),
            "ddlo_seg_static_cloud_xyzi": (I, [P, P, S, P, C.c_double, C.c_double, P, S, C.POINTER(S)]),
            "ddlo_seg_set_intensity": (I, [P, I, S]),
            "ddlo_seg_get_intensity": (I, [P, C.POINTER(I), C.POINTER(S)]),
            "ddlo_seg_tracks_sync": (I, [P, P, P, S, P, S]),
            "ddlo_seg_static_cloud_tracks": (I, [P, P, S, P, C.c_double, C.c_double, P, S, C.POINTER(S)]),
            "ddlo_seg_track_indices": (I, [P, C.c_int32, P, S, C.POINTER(S)]),
            "ddlo_seg_tracks_stats": (I, [P, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
            "ddlo_seg_classify": (I, [P, P, P, S, C.POINTER(ClassCounts)]),
            "ddlo_seg_class_image": (I, [P, P]),
            "ddlo_seg_class_indices": (I, [P, I, I, P, S, C.POINTER(S)]),
            "ddlo_seg_frame_clouds": (I, [P, C.POINTER(_FrameCloudsOut)]),
            "ddlo_seg_default_projection": (I, [C.POINTER(SegParams), C.POINTER(ProjectionParams)]),
            "ddlo_seg_process_cloud": (I, [P, P, S, S, P, C.POINTER(ProjectionParams), P, C.POINTER(SegResult),
                                           C.POINTER(ProjectionResult)]),
            "ddlo_seg_projection_maps": (I, [P, P, P, S, C.POINTER(S)]),
            "ddlo_seg_point_classes": (I, [P, P, S, C.POINTER(S)]),
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


def default_seg_params(**kw) -> SegParams:
    """DetectionModule::loadParams code defaults (detection.cpp:77-107)."""
    p = SegParams()
    _check(_lib().ddlo_seg_default_params(C.byref(p)))
    return p.replace(**kw) if kw else p


def default_projection(params: SegParams, **kw) -> ProjectionParams:
    """ddlo_seg_default_projection: the ring model of params (row 0 at +ang_bottom, the last row at
    -ang_bottom, column 0 along +x, columns growing with atan2(y, x)): scene.lidar_dirs' model."""
    q = ProjectionParams()
    _check(_lib().ddlo_seg_default_projection(C.byref(params), C.byref(q)))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def yaml_seg_params(**kw) -> SegParams:
    """cfg/ddlo.yaml:206-225 as ROS delivers it to loadParams: the parameters
    whose code default is an int literal are read as int (roscpp rounds a
    double yaml value to the nearest integer), so minimumRange 0.3 -> 0."""
    p = default_seg_params(rows=512, cols=512, ang_bottom=90, ground_rows=150, ground_angle_threshold=80,
                           minimum_range=0, sensor_mount_angle=0, theta=0.25, valid_point_num=10, min_line_num=2,
                           valid_line_num=4, min_delta_z=0.3, max_delta_z=2.0, max_distance=8, max_elevation=8.0)
    return p.replace(**kw) if kw else p


def label_components(p: SegParams, range_img, z_img, label_img, sensor_z: float, residual=None, device=None):
    """The host labelling alone (ddlo_seg_label) over caller images; returns
    (label image, avg residuals by label, segments).  device: the GPU to label on
    instead (ddlo_seg_label_device, see label_components_device)."""
    rng = np.ascontiguousarray(range_img, np.float32).reshape(-1)
    z = np.ascontiguousarray(z_img, np.float32).reshape(-1)
    lab = np.ascontiguousarray(label_img, np.int32).reshape(-1).copy()
    n = p.rows * p.cols
    if rng.size != n or z.size != n or lab.size != n:
        raise ValueError("images must have rows x cols pixels")
    res = None if residual is None else np.ascontiguousarray(residual, np.float32).reshape(-1)
    if res is not None and res.size != n:
        raise ValueError("residual image must have rows x cols pixels")
    avg = np.zeros(n + 1, np.float64)
    seg = C.c_int32()
    args = (C.byref(p), _ptr(rng), _ptr(z), None if res is None else _ptr(res), float(sensor_z), _ptr(lab), _ptr(avg),
            avg.size, C.byref(seg))
    if device is None:
        _check(_lib().ddlo_seg_label(*args))
    else:
        _check(_lib().ddlo_seg_label_device(int(device), *args))
    return lab.reshape(p.rows, p.cols), avg[: seg.value + 1], seg.value


def label_components_device(p: SegParams, range_img, z_img, label_img, sensor_z: float, residual=None, device: int = 0):
    """label_components on the GPU (ddlo_seg_label_device): the same labels and segment
    count; the average residuals are the positive residuals of a segment's pixels without
    its seed, summed in double in row-major order, over their count.  The window must lie
    inside the columns."""
    return label_components(p, range_img, z_img, label_img, sensor_z, residual, device=device)


def objects_from(xyz_t, label, avg_residual=None, max_dim_ratio: float = 10.0, device: int = 0) -> np.ndarray:
    """ddlo_seg_objects_from: the objects of a caller's label image (rows x cols) over the organized
    world-frame cloud xyz_t (rows*cols, >=3); returns an OBJECT_DTYPE array."""
    lab = np.ascontiguousarray(label, np.int32)
    if lab.ndim != 2:
        raise ValueError("label must be a rows x cols image")
    rows, cols = lab.shape
    a = np.ascontiguousarray(xyz_t, np.float32)
    if a.ndim != 2 or a.shape[0] != rows * cols or a.shape[1] < 3:
        raise ValueError("xyz_t must be (rows*cols, >=3)")
    avg = None if avg_residual is None else np.ascontiguousarray(avg_residual, np.float64).reshape(-1)
    L = _lib()
    n = C.c_size_t()
    args = (device, _ptr(a), a.shape[1] * 4, rows, cols, _ptr(lab), None if avg is None else _ptr(avg),
            0 if avg is None else avg.size, float(max_dim_ratio))
    _check(L.ddlo_seg_objects_from(*args, None, 0, C.byref(n)))
    out = np.zeros(n.value, OBJECT_DTYPE)
    if n.value:
        _check(L.ddlo_seg_objects_from(*args, _ptr(out), out.size, C.byref(n)))
    return out


class Segmentation:
    """DetectionModule's segmentation on device ``device`` (ddlo_seg_*)."""

    def __init__(self, device: int = 0, params: SegParams | None = None, labelling: str = "host"):
        self.L = _lib()
        self.params = params if params is not None else default_seg_params()
        self.h = C.c_void_p()
        _check(self.L.ddlo_seg_create(device, C.byref(self.params), C.byref(self.h)))
        self.last: SegResult | None = None
        if labelling != "host":
            self.labelling = labelling

    @property
    def labelling(self) -> str:
        """"host" or "device" (ddlo_seg_set_labelling); setting "device" on a handle whose window
        reaches outside the columns raises GicpError and leaves the mode unchanged."""
        m = C.c_int()
        _check(self.L.ddlo_seg_get_labelling(self.h, C.byref(m)))
        return {v: k for k, v in LABELLING.items()}[m.value]

    @labelling.setter
    def labelling(self, mode: str):
        if mode not in LABELLING:
            raise ValueError('labelling must be "host" or "device"')
        _check(self.L.ddlo_seg_set_labelling(self.h, LABELLING[mode]))

    def set_voxel_order(self, order: int):
        """ddlo_seg_set_voxel_order: 0 (input order, the default) or 1 (pcl::VoxelGrid's order) for the voxel
        pass of static_cloud / static_cloud_tracks, from the next call on."""
        _check(self.L.ddlo_seg_set_voxel_order(self.h, int(order)))

    @property
    def voxel_order(self) -> int:
        m = C.c_int()
        _check(self.L.ddlo_seg_get_voxel_order(self.h, C.byref(m)))
        return m.value

    def set_intensity(self, use, offset_bytes: int = 12):
        """ddlo_seg_set_intensity: static_cloud carries the float at offset_bytes of the records process() /
        process_cloud() are given (from the next scan on), or the channel of the scan an Odometry with
        set_intensity on staged."""
        _check(self.L.ddlo_seg_set_intensity(self.h, int(bool(use)), int(offset_bytes)))

    @property
    def intensity(self):
        """(use, offset_bytes) as set."""
        u, off = C.c_int(), C.c_size_t()
        _check(self.L.ddlo_seg_get_intensity(self.h, C.byref(u), C.byref(off)))
        return bool(u.value), off.value

    def set_downsampling(self, use, row_step: int, col_step: int):
        """ddlo_seg_set_downsampling: the row/column filter's keyframe pass inside static_cloud /
        static_cloud_tracks, between the removal and the crop, from the next call on."""
        _check(self.L.ddlo_seg_set_downsampling(self.h, int(bool(use)), int(row_step), int(col_step)))

    def downsampling(self):
        """(use, row_step, col_step) as set."""
        v = [C.c_int() for _ in range(3)]
        _check(self.L.ddlo_seg_get_downsampling(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    @property
    def downsampling_skipped(self) -> bool:
        """The last static cloud's keyframe pass met |S| > n' and filtered nothing."""
        m = C.c_int()
        _check(self.L.ddlo_seg_downsampling_skipped(self.h, C.byref(m)))
        return bool(m.value)

    def labelling_stats(self):
        """Device mode: (components whose push prefix was replayed, longest prefix) of the last scan."""
        a, b = C.c_int32(), C.c_int32()
        _check(self.L.ddlo_seg_labelling_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self.h:
            self.L.ddlo_seg_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process(self, xyz_t, T, residual=None) -> SegResult:
        """xyz_t: (rows*cols, >=3) float32 organized world-frame cloud (NaN = no return)."""
        a = np.ascontiguousarray(xyz_t, np.float32)
        if a.ndim != 2 or a.shape[0] != self.params.rows * self.params.cols or a.shape[1] < 3:
            raise ValueError("xyz_t must be (rows*cols, >=3)")
        Tm = np.ascontiguousarray(T, np.float32).reshape(16)
        res = None
        if residual is not None:
            res = np.ascontiguousarray(residual, np.float32).reshape(-1)
            if res.size != a.shape[0]:
                raise ValueError("residual image must have rows x cols pixels")
        r = SegResult()
        _check(self.L.ddlo_seg_process(self.h, _ptr(a), a.shape[1] * 4, _ptr(Tm), None if res is None else _ptr(res),
                                       C.byref(r)))
        self.last = r
        return r

    def process_cloud(self, points, T, residual=None, projection: ProjectionParams | None = None):
        """ddlo_seg_process_cloud: points (n, >=3) float32, an unorganized SENSOR-frame cloud (n may be 0),
        projected into the range image (the highest index wins a pixel), moved to the world frame by the pose
        T and segmented.  projection None: default_projection(self.params).  Returns (SegResult,
        ProjectionResult)."""
        a = np.ascontiguousarray(points, np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("points must be (n, >=3)")
        Tm = np.ascontiguousarray(T, np.float32).reshape(16)
        res = None
        if residual is not None:
            res = np.ascontiguousarray(residual, np.float32).reshape(-1)
            if res.size != self.params.rows * self.params.cols:
                raise ValueError("residual image must have rows x cols pixels")
        r, pr = SegResult(), ProjectionResult()
        _check(self.L.ddlo_seg_process_cloud(self.h, _ptr(a) if a.shape[0] else None, a.shape[0], a.shape[1] * 4,
                                             _ptr(Tm), C.byref(projection) if projection is not None else None,
                                             None if res is None else _ptr(res), C.byref(r), C.byref(pr)))
        self.last = r
        return r, pr

    def projection_maps(self):
        """The maps of the last projected scan: (winner (rows, cols) int32: the input index whose point the
        pixel holds, -1 if empty; pixel_of_point (n,) int32: the row-major pixel of every input point, -1 if
        it was invalid or out of view)."""
        n = C.c_size_t()
        _check(self.L.ddlo_seg_projection_maps(self.h, None, None, 0, C.byref(n)))
        win = np.empty((self.params.rows, self.params.cols), np.int32)
        pix = np.empty(n.value, np.int32)
        _check(self.L.ddlo_seg_projection_maps(self.h, _ptr(win), _ptr(pix) if pix.size else None, pix.size,
                                               C.byref(n)))
        return win, pix

    def point_classes(self) -> np.ndarray:
        """ddlo_seg_point_classes: the class byte (CLS_* bits) of every input point of the last projected
        scan, after a classify(): that of the pixel the point fell into, 0 if it was dropped."""
        n = C.c_size_t()
        _check(self.L.ddlo_seg_point_classes(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint8)
        if n.value:
            _check(self.L.ddlo_seg_point_classes(self.h, _ptr(out), out.size, C.byref(n)))
        return out

    def point_class_indices(self, any_bits: int, none_bits: int = 0) -> np.ndarray:
        """The input points with at least one bit of any_bits and no bit of none_bits, ascending (int64):
        class_indices() in the caller's point indices (a host pass over point_classes())."""
        b = self.point_classes()
        return np.flatnonzero(((b & int(any_bits)) != 0) & ((b & int(none_bits)) == 0))

    def images(self):
        H, W = self.params.rows, self.params.cols
        rng = np.empty((H, W), np.float32)
        gr = np.empty((H, W), np.int8)
        lab = np.empty((H, W), np.int32)
        _check(self.L.ddlo_seg_images(self.h, _ptr(rng), _ptr(gr), _ptr(lab)))
        return rng, gr, lab

    def avg_residuals(self) -> np.ndarray:
        n = C.c_size_t()
        _check(self.L.ddlo_seg_avg_residuals(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.float64)
        _check(self.L.ddlo_seg_avg_residuals(self.h, _ptr(out), out.size, C.byref(n)))
        return out

    def ground_indices(self) -> np.ndarray:
        n = C.c_size_t()
        _check(self.L.ddlo_seg_ground_indices(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        _check(self.L.ddlo_seg_ground_indices(self.h, _ptr(out), out.size, C.byref(n)))
        return out

    def label_indices(self) -> list:
        """label_indices_i_: [None] + one int32 array of row-major pixel indices per segment."""
        n = C.c_size_t()
        _check(self.L.ddlo_seg_label_indices(self.h, None, 0, None, 0, C.byref(n)))
        L = self.last.segments if self.last is not None else 0
        off = np.zeros(L + 2, np.int32)
        idx = np.zeros(max(n.value, 1), np.int32)
        _check(self.L.ddlo_seg_label_indices(self.h, _ptr(off), off.size, _ptr(idx), idx.size, C.byref(n)))
        return [None] + [idx[off[l]:off[l + 1]] for l in range(1, L + 1)]


    def objects(self, max_dim_ratio: float = 10.0) -> np.ndarray:
        """computeAllObjects: the objects of the last process(), ascending id, as an OBJECT_DTYPE array."""
        n = C.c_size_t()
        _check(self.L.ddlo_seg_objects(self.h, float(max_dim_ratio), None, 0, C.byref(n)))
        out = np.zeros(n.value, OBJECT_DTYPE)
        if n.value:
            _check(self.L.ddlo_seg_objects(self.h, float(max_dim_ratio), _ptr(out), out.size, C.byref(n)))
        return out

    def static_cloud(self, remove_ids=(), centre=(0.0, 0.0, 0.0), crop_size: float = 0.0, leaf: float = 0.0,
                     intensity: bool = False):
        """applySegmentation's tail (odom.cc:887-918): the last scan without the pixels of the segments in
        remove_ids, cropped around centre and voxel-filtered; (m, 3) float32.  intensity=True (a handle with
        set_intensity on): (m, 4), ddlo_seg_static_cloud_xyzi."""
        ids = np.ascontiguousarray(remove_ids, np.int32).reshape(-1)
        c = np.ascontiguousarray(centre, np.float32).reshape(3)
        n = C.c_size_t()
        args = (self.h, _ptr(ids) if ids.size else None, ids.size, _ptr(c), float(crop_size), float(leaf))
        if intensity:
            _check(self.L.ddlo_seg_static_cloud_xyzi(*args, None, 0, C.byref(n)))
            out = np.zeros((max(n.value, 1), 4), np.float32)
            _check(self.L.ddlo_seg_static_cloud_xyzi(*args, _ptr(out), out.shape[0], C.byref(n)))
            return out[:n.value]
        _check(self.L.ddlo_seg_static_cloud(*args, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 3), np.float32)
        _check(self.L.ddlo_seg_static_cloud(*args, _ptr(out), out.shape[0], C.byref(n)))
        return out[:n.value]

    def tracks_sync(self, set_pairs=(), dead_ids=()):
        """ddlo_seg_tracks_sync: set_pairs = (track id, segment id of the last process()) pairs whose lists
        are (re)set; dead_ids release theirs; every other track keeps its list."""
        pairs = np.ascontiguousarray(list(set_pairs), np.int32).reshape(-1, 2)
        tid = np.ascontiguousarray(pairs[:, 0])
        sid = np.ascontiguousarray(pairs[:, 1])
        dead = np.ascontiguousarray(dead_ids, np.int32).reshape(-1)
        _check(self.L.ddlo_seg_tracks_sync(self.h, _ptr(tid) if tid.size else None, _ptr(sid) if sid.size else None,
                                           tid.size, _ptr(dead) if dead.size else None, dead.size))

    def static_cloud_tracks(self, track_ids=(), centre=(0.0, 0.0, 0.0), crop_size: float = 0.0, leaf: float = 0.0):
        """static_cloud with the union of the listed tracks' pixel lists (stale ones included) removed
        from the last scan; (m, 3) float32."""
        ids = np.ascontiguousarray(track_ids, np.int32).reshape(-1)
        c = np.ascontiguousarray(centre, np.float32).reshape(3)
        n = C.c_size_t()
        args = (self.h, _ptr(ids) if ids.size else None, ids.size, _ptr(c), float(crop_size), float(leaf))
        _check(self.L.ddlo_seg_static_cloud_tracks(*args, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 3), np.float32)
        _check(self.L.ddlo_seg_static_cloud_tracks(*args, _ptr(out), out.shape[0], C.byref(n)))
        return out[:n.value]

    def track_indices(self, track_id: int) -> np.ndarray:
        """The pixel list a track holds (getIndices of one filter), ascending row-major indices."""
        n = C.c_size_t()
        _check(self.L.ddlo_seg_track_indices(self.h, int(track_id), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.int32)
        _check(self.L.ddlo_seg_track_indices(self.h, int(track_id), _ptr(out), out.size, C.byref(n)))
        return out[:n.value]

    def tracks_stats(self):
        """(lists held, indices held, capacity of the pool buffer in use)."""
        a, b, c = C.c_int32(), C.c_int64(), C.c_int64()
        _check(self.L.ddlo_seg_tracks_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def classify(self, tracks=()) -> ClassCounts:
        """ddlo_seg_classify: tracks = (track id, status 0..2) pairs; the class image of the last process():
        VALID and GROUND from the scan, the status bit of every listed track on its list's pixels (stale lists
        included).  Returns the counts."""
        pairs = np.ascontiguousarray(list(tracks), np.int32).reshape(-1, 2)
        tid = np.ascontiguousarray(pairs[:, 0])
        st = np.ascontiguousarray(pairs[:, 1])
        c = ClassCounts()
        _check(self.L.ddlo_seg_classify(self.h, _ptr(tid) if tid.size else None, _ptr(st) if st.size else None,
                                        tid.size, C.byref(c)))
        return c

    def class_image(self) -> np.ndarray:
        """The class image of the last classify(): (rows, cols) uint8 of CLS_* bits."""
        img = np.empty((self.params.rows, self.params.cols), np.uint8)
        _check(self.L.ddlo_seg_class_image(self.h, _ptr(img)))
        return img

    def class_indices(self, any_bits: int, none_bits: int = 0) -> np.ndarray:
        """The pixels with at least one bit of any_bits and no bit of none_bits, ascending (int32): an index
        set as evaluate() writes it; it may name pixels whose current point is not VALID (stale lists)."""
        out = np.empty(self.params.rows * self.params.cols, np.int32)
        n = C.c_size_t()
        _check(self.L.ddlo_seg_class_indices(self.h, int(any_bits), int(none_bits), _ptr(out), out.size, C.byref(n)))
        return out[:n.value].copy()

    def frame_clouds(self) -> FrameClouds:
        """ddlo_seg_frame_clouds: the ground, non-static, dynamic and static clouds of the last classify()."""
        o = _FrameCloudsOut()
        _check(self.L.ddlo_seg_frame_clouds(self.h, C.byref(o)))       # the sizes (the partition runs here)
        names = ("ground", "non_static", "dynamic", "static_points")
        bufs = []
        for k in names:
            f = getattr(o, k)
            a = np.zeros((max(f.n, 1), 3), np.float32)
            f.xyz, f.cap = a.ctypes.data, a.shape[0]
            bufs.append(a)
        _check(self.L.ddlo_seg_frame_clouds(self.h, C.byref(o)))       # the copies
        return FrameClouds(*[a[:getattr(o, k).n] for a, k in zip(bufs, names)])
