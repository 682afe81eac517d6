"""ctypes mirror of the global map C-ABI (include/ddlo_map.h).

``Map`` is the reference's ``MapNode`` (``src/odometry/map.cc``) with its
cloud on the GPU: keyframes are voxel-filtered and appended (``keyframeCB``),
the points inside the bounding-box history of a dynamic object are removed
(``dynamicObjectsCB``), and the map is read back or written as a PCD file,
voxelised on request (``savePcd``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import GicpError, _ptr, load
from .odometry import Odometry

__all__ = ["MapParams", "MapBox", "Map", "default_map_params", "box_from_object"]


class MapParams(C.Structure):
    """ddlo_map_params."""
    _fields_ = [
        ("voxel_filter_use", C.c_int32),
        ("leaf_size", C.c_double),
        ("filter_bboxes", C.c_int32),
        ("filter_margin", C.c_double),
    ]


class MapBox(C.Structure):
    """ddlo_map_box."""
    _fields_ = [
        ("position", C.c_double * 3),
        ("orientation_z", C.c_double),
        ("dimensions", C.c_double * 3),
    ]


_SIGS_DONE = False


def _lib():
    global _SIGS_DONE
    L = load()
    if not _SIGS_DONE:
        P, S, I, D = C.c_void_p, C.c_size_t, C.c_int, C.c_double
        sig = {
            "ddlo_map_default_params": (I, [C.POINTER(MapParams)]),
            "ddlo_map_create": (I, [I, C.POINTER(MapParams), C.POINTER(P)]),
            "ddlo_map_destroy": (I, [P]),
            "ddlo_map_add_keyframe": (I, [P, P, S, S, C.POINTER(S)]),
            "ddlo_map_add_odom_keyframe": (I, [P, P, I, C.POINTER(S)]),
            "ddlo_map_clear_boxes": (I, [P, C.POINTER(MapBox), S, C.POINTER(S)]),
            "ddlo_map_size": (I, [P, C.POINTER(S)]),
            "ddlo_map_points": (I, [P, D, P, S, C.POINTER(S)]),
            "ddlo_map_save_pcd": (I, [P, C.c_char_p, D]),
            "ddlo_map_set_intensity": (I, [P, I]),
            "ddlo_map_get_intensity": (I, [P, C.POINTER(I)]),
            "ddlo_map_add_keyframe_xyzi": (I, [P, P, S, S, S, C.POINTER(S)]),
            "ddlo_map_points_xyzi": (I, [P, D, P, S, C.POINTER(S)]),
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


def default_map_params(**kw) -> MapParams:
    """cfg/ddlo.yaml's mapNode block (map.cc:52-62)."""
    p = MapParams()
    _check(_lib().ddlo_map_default_params(C.byref(p)))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def box_from_object(obj) -> MapBox:
    """The box of a detected object (an OBJECT_DTYPE record or a SegObject), as
    TrackingModule::publishBBoxes fills it: position = state[0:3], orientation.z
    = state[3], dimensions = state[4:7]."""
    st = [float(v) for v in (obj.state if isinstance(obj, C.Structure) else obj["state"])]
    b = MapBox()
    b.position[:] = st[0:3]
    b.orientation_z = st[3]
    b.dimensions[:] = st[4:7]
    return b


def _boxes(boxes):
    """MapBox instances, or rows of (x, y, z, orientation_z, dx, dy, dz), as a ctypes array."""
    if isinstance(boxes, C.Array) and getattr(boxes, "_type_", None) is MapBox:
        return boxes, len(boxes)
    items = list(boxes)
    arr = (MapBox * max(len(items), 1))()
    for i, b in enumerate(items):
        if isinstance(b, MapBox):
            arr[i] = b
        else:
            v = [float(x) for x in b]
            if len(v) != 7:
                raise ValueError("a box is (x, y, z, orientation_z, dx, dy, dz)")
            arr[i].position[:] = v[0:3]
            arr[i].orientation_z = v[3]
            arr[i].dimensions[:] = v[4:7]
    return arr, len(items)


class Map:
    """MapNode's global map on one GPU."""

    def __init__(self, device: int = 0, params: MapParams | None = None):
        self.L = _lib()
        self.h = C.c_void_p()
        _check(self.L.ddlo_map_create(device, C.byref(params) if params is not None else None, C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.ddlo_map_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_intensity(self, use) -> None:
        """ddlo_map_set_intensity: whether the map carries the intensity channel; only while it is empty."""
        _check(self.L.ddlo_map_set_intensity(self.h, int(bool(use))))

    @property
    def intensity(self) -> bool:
        u = C.c_int()
        _check(self.L.ddlo_map_get_intensity(self.h, C.byref(u)))
        return bool(u.value)

    def add_keyframe(self, points, intensity_offset: int | None = None) -> int:
        """keyframeCB for world-frame points (n, 3); returns the number of points appended.
        intensity_offset (a map with set_intensity on): ddlo_map_add_keyframe_xyzi on (n, c) float32 rows
        whose intensity is the float at that byte offset (12 for x y z i rows)."""
        if intensity_offset is not None:
            a = np.ascontiguousarray(points, np.float32)
            if a.ndim != 2 or a.shape[1] < 3:
                raise ValueError("points must be (n, >=3)")
            added = C.c_size_t()
            _check(self.L.ddlo_map_add_keyframe_xyzi(self.h, _ptr(a) if a.shape[0] else None, a.shape[0],
                                                     a.shape[1] * 4, int(intensity_offset), C.byref(added)))
            return added.value
        a = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3))
        added = C.c_size_t()
        _check(self.L.ddlo_map_add_keyframe(self.h, _ptr(a) if a.shape[0] else None, a.shape[0], 12, C.byref(added)))
        return added.value

    def add_odom_keyframe(self, odom: Odometry, k: int) -> int:
        """keyframeCB for keyframe k of an Odometry on the same device, device to device."""
        added = C.c_size_t()
        _check(self.L.ddlo_map_add_odom_keyframe(self.h, odom.h, k, C.byref(added)))
        return added.value

    def clear_boxes(self, boxes) -> int:
        """dynamicObjectsCB: removes the points inside any box; returns how many."""
        arr, n = _boxes(boxes)
        removed = C.c_size_t()
        _check(self.L.ddlo_map_clear_boxes(self.h, arr, n, C.byref(removed)))
        return removed.value

    def __len__(self) -> int:
        n = C.c_size_t()
        _check(self.L.ddlo_map_size(self.h, C.byref(n)))
        return n.value

    def points(self, leaf: float = 0.0, intensity: bool = False) -> np.ndarray:
        """The map (n, 3) float32; leaf > 0: savePcd's voxelised copy, the map unchanged.
        intensity=True (a map with set_intensity on): (n, 4), ddlo_map_points_xyzi."""
        if intensity:
            out = np.zeros((max(len(self), 1), 4), np.float32)
            n = C.c_size_t()
            _check(self.L.ddlo_map_points_xyzi(self.h, float(leaf), _ptr(out), out.shape[0], C.byref(n)))
            return out[:n.value]
        out = np.zeros((max(len(self), 1), 3), np.float32)      # the voxelised copy is never larger
        n = C.c_size_t()
        _check(self.L.ddlo_map_points(self.h, float(leaf), _ptr(out), out.shape[0], C.byref(n)))
        return out[:n.value]

    def save_pcd(self, path, leaf: float = 0.0) -> None:
        """savePcd: binary PCD v0.7 with FIELDS x y z (a map with intensity: x y z intensity)."""
        _check(self.L.ddlo_map_save_pcd(self.h, os.fsencode(path), float(leaf)))
