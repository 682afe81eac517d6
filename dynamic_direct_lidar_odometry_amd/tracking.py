"""ctypes mirror of the object tracker's C-ABI (include/ddlo_track.h).

``Tracker`` is the reference's ``TrackingModule`` (``src/tracking/tracking.cpp``)
with its bounding-box Kalman filters, Hungarian association and rotated-box
IoU.  It is host code without any device work: it needs no GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import GicpError, _ptr, load
from .mapping import MapBox
from .segmentation import OBJECT_DTYPE

__all__ = ["TrackParams", "TrackResult", "Tracker", "TRACK_DTYPE", "BOX_DTYPE", "assign", "default_track_params",
           "UNDEFINED", "STATIC", "DYNAMIC"]

UNDEFINED, STATIC, DYNAMIC = 0, 1, 2


class TrackParams(C.Structure):
    _fields_ = [
        ("max_no_hits", C.c_int32),
        ("min_dynamic_hits", C.c_int32),
        ("max_undefined_hits", C.c_int32),
        ("max_obj_velocity", C.c_float),
        ("min_dist_from_origin", C.c_double),
        ("residuum_height_ratio", C.c_double),
    ]


class TrackResult(C.Structure):
    _fields_ = [
        ("undefined_tracks", C.c_int32),
        ("static_tracks", C.c_int32),
        ("dynamic_tracks", C.c_int32),
        ("matches", C.c_int32),
        ("created", C.c_int32),
        ("erased", C.c_int32),
        ("turned_dynamic", C.c_int32),
        ("boxes_cleared", C.c_int32),
        ("indices_dropped", C.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# ddlo_track_record
TRACK_DTYPE = np.dtype([("id", np.int32), ("status", np.int32), ("hits", np.int32), ("sslu", np.int32),
                        ("state", np.float64, 10), ("num_points", np.int32), ("object_id", np.int32),
                        ("avg_residuum", np.float64), ("dist_to_origin", np.float64), ("history", np.int32),
                        ("reserved", np.int32)], align=True)
# ddlo_map_box
BOX_DTYPE = np.dtype([("position", np.float64, 3), ("orientation_z", np.float64), ("dimensions", np.float64, 3)])
assert BOX_DTYPE.itemsize == C.sizeof(MapBox)

_SIGS_DONE = False


def _lib():
    global _SIGS_DONE
    L = load()
    if not _SIGS_DONE:
        P, S, I, D = C.c_void_p, C.c_size_t, C.c_int, C.c_double
        sig = {
            "ddlo_track_default_params": (I, [C.POINTER(TrackParams)]),
            "ddlo_track_create": (I, [C.POINTER(TrackParams), C.POINTER(P)]),
            "ddlo_track_destroy": (I, [P]),
            "ddlo_track_update": (I, [P, D, P, S, P, C.POINTER(TrackResult)]),
            "ddlo_track_tracks": (I, [P, P, S, C.POINTER(S)]),
            "ddlo_track_count": (I, [P, I, C.POINTER(S)]),
            "ddlo_track_erased": (I, [P, P, S, C.POINTER(S)]),
            "ddlo_track_take_cleared_boxes": (I, [P, P, S, C.POINTER(S)]),
            "ddlo_track_last_costs": (I, [P, P, P, P, S, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
            "ddlo_track_assign": (I, [P, I, I, P]),
            "ddlo_track_decide": (C.c_int, [P, P, S, C.POINTER(C.c_uint8)]),
            "ddlo_track_set_dt": (I, [P, D]),
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


def default_track_params(**kw) -> TrackParams:
    """cfg/ddlo.yaml:224-233: maxNoHits 30, minDynamicHits 5, maxUndefinedHits 1, maxObjVelocity 15,
    minDistFromOrigin 0.75, residuumHeightRatio 0.3."""
    p = TrackParams()
    _check(_lib().ddlo_track_default_params(C.byref(p)))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def assign(cost) -> np.ndarray:
    """HungarianAlgorithm::Solve (ddlo_track_assign): the reference's assignment of a rows x cols cost
    matrix, ties included; -1 = unassigned."""
    m = np.ascontiguousarray(cost, np.float64)
    if m.ndim != 2:
        raise ValueError("cost must be a matrix")
    out = np.full(m.shape[0], -1, np.int32)
    _check(_lib().ddlo_track_assign(_ptr(m), m.shape[0], m.shape[1], _ptr(out)))
    return out


class Tracker:
    """TrackingModule (ddlo_track_*)."""

    def __init__(self, params: TrackParams | None = None):
        self.L = _lib()
        self.params = params if params is not None else default_track_params()
        self.h = C.c_void_p()
        _check(self.L.ddlo_track_create(C.byref(self.params), C.byref(self.h)))
        self.last: TrackResult | None = None

    def close(self):
        if self.h:
            self.L.ddlo_track_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, dt: float, objects) -> np.ndarray:
        """TrackingModule::update for one scan's objects (an OBJECT_DTYPE array, as Segmentation.objects()
        returns); returns the filter id each detection updated or created.  The counts are in ``last``."""
        objs = np.ascontiguousarray(objects, OBJECT_DTYPE).reshape(-1)
        ids = np.full(max(objs.size, 1), -1, np.int32)
        r = TrackResult()
        _check(self.L.ddlo_track_update(self.h, float(dt), _ptr(objs) if objs.size else None, objs.size, _ptr(ids),
                                        C.byref(r)))
        self.last = r
        return ids[:objs.size]

    def tracks(self) -> np.ndarray:
        """The filters in the tracker's order, as a TRACK_DTYPE array."""
        n = C.c_size_t()
        _check(self.L.ddlo_track_tracks(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, TRACK_DTYPE)
        if n.value:
            _check(self.L.ddlo_track_tracks(self.h, _ptr(out), out.size, C.byref(n)))
        return out

    def count(self, *statuses) -> int:
        mask = sum(1 << s for s in set(statuses)) if statuses else 7
        n = C.c_size_t()
        _check(self.L.ddlo_track_count(self.h, mask, C.byref(n)))
        return n.value

    def erased(self) -> np.ndarray:
        n = C.c_size_t()
        _check(self.L.ddlo_track_erased(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.int32)
        _check(self.L.ddlo_track_erased(self.h, _ptr(out), out.size, C.byref(n)))
        return out[:n.value]

    def take_cleared_boxes(self) -> np.ndarray:
        """The box histories of the filters that turned dynamic since the last call (BOX_DTYPE)."""
        n = C.c_size_t()
        _check(self.L.ddlo_track_take_cleared_boxes(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), BOX_DTYPE)
        _check(self.L.ddlo_track_take_cleared_boxes(self.h, _ptr(out), out.size, C.byref(n)))
        return out[:n.value]

    def last_costs(self):
        """(cost float64 rows x cols, displacement float32 rows x cols, assignment int32 rows) of the last
        association; 0 x 0 when the frame had no detections or no filters."""
        r, c = C.c_int32(), C.c_int32()
        _check(self.L.ddlo_track_last_costs(self.h, None, None, None, 0, C.byref(r), C.byref(c)))
        cost = np.zeros((r.value, c.value), np.float64)
        disp = np.zeros((r.value, c.value), np.float32)
        a = np.zeros(r.value, np.int32)
        if cost.size:
            _check(self.L.ddlo_track_last_costs(self.h, _ptr(cost), _ptr(disp), _ptr(a), cost.size + r.value, C.byref(r),
                                                C.byref(c)))
        return cost, disp, a

    def set_dt(self, dt: float):
        _check(self.L.ddlo_track_set_dt(self.h, float(dt)))
