"""ctypes mirror of the evaluation files' C-ABI (include/ddlo_eval.h).

``Evaluation`` writes what the reference's ``DetectionModule::evaluate``
(``src/detection/detection.cpp:936-954``) writes per frame: the dynamic pixel
indices to ``<dir>/<seq as %04u>.txt`` and the pose to ``<dir>/poses.txt``.
``read_eval`` parses such a directory back.  Host code only: no GPU is needed.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

from . import GicpError, _ptr, load

__all__ = ["Evaluation", "read_eval"]

_SIGS_DONE = False


def _lib():
    global _SIGS_DONE
    L = load()
    if not _SIGS_DONE:
        P, S, I = C.c_void_p, C.c_size_t, C.c_int
        sig = {
            "ddlo_eval_open": (I, [C.c_char_p, C.POINTER(P)]),
            "ddlo_eval_write": (I, [P, C.c_uint32, C.c_uint64, P, P, S]),
            "ddlo_eval_close": (I, [P]),
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


class Evaluation:
    """The evaluation directory ``dir`` (created if missing), open for appending."""

    def __init__(self, dir):
        self.L = _lib()
        self.dir = os.fspath(dir)
        self.h = C.c_void_p()
        _check(self.L.ddlo_eval_open(os.fsencode(self.dir), C.byref(self.h)))

    def write(self, seq: int, stamp_ns: int, T, dynamic_idx=()):
        """One frame: the pose T (4 x 4) at stamp_ns and the frame's dynamic pixel indices
        (Segmentation.class_indices(CLS_DYNAMIC))."""
        Tm = np.ascontiguousarray(T, np.float32).reshape(16)
        idx = np.ascontiguousarray(dynamic_idx, np.int32).reshape(-1)
        _check(self.L.ddlo_eval_write(self.h, int(seq), int(stamp_ns), _ptr(Tm), _ptr(idx) if idx.size else None,
                                      idx.size))

    def close(self):
        if self.h:
            self.L.ddlo_eval_close(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_eval(dir):
    """Parses an evaluation directory: ({seq: int32 array of the indices in file order},
    [(stamp_ns, 4 x 4 float64 pose) in file order]).  Only what a parser sees is read: the
    whitespace between a pose's coefficients is free."""
    dir = os.fspath(dir)
    indices = {}
    for name in sorted(os.listdir(dir)):
        m = re.fullmatch(r"(\d{4,})\.txt", name)
        if not m:
            continue
        with open(os.path.join(dir, name)) as f:
            indices[int(m.group(1))] = np.array([int(line) for line in f if line.strip()], np.int32)
    poses = []
    path = os.path.join(dir, "poses.txt")
    if os.path.exists(path):
        with open(path) as f:
            records = f.read().split(";")
        if records[-1].strip():
            raise ValueError("poses.txt: the last record has no ';'")
        for rec in records[:-1]:
            tok = rec.split()
            if len(tok) != 17:
                raise ValueError("poses.txt: a record is not a stamp and sixteen coefficients")
            poses.append((int(tok[0]), np.array([float(t) for t in tok[1:]], np.float64).reshape(4, 4)))
    return indices, poses
