"""Small clouds for the per-point covariances — TEST HELPER ONLY.

Every case is a seeded float32 cloud of at most 2049 points, the k values it
is run at, the exact rank of its k-neighbourhoods' covariances and whether its
neighbourhoods are free of exact distance ties (asserted in
tests/test_cov_cases_cpu.py, never assumed).

The rank-deficient clouds are rank deficient EXACTLY, not up to the float32
rounding of their coordinates: the generic line and the tilted plane are
integer direction vectors times dyadic parameters, so every coordinate is an
exact float32 and the covariance computed in extended precision has null
eigenvalues at its own rounding level (1e-19 lambda_max), far below the
1e-12 lambda_max the envelope of tests/cov_ref.py asks of a null eigenvalue.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np


@dataclass(frozen=True)
class Case:
    name: str
    ks: tuple          # the k values the case runs at
    rank: dict         # k -> exact rank of every neighbourhood's covariance
    tie_free: bool     # no exact distance tie inside or at the edge of any k-neighbourhood


def _generic():
    rng = np.random.default_rng(11)
    return (rng.standard_normal((257, 3)) * [8, 8, 1]).astype(np.float32)


def _dup():
    rng = np.random.default_rng(12)
    base = (rng.standard_normal((10, 3)) * [8, 8, 1]).astype(np.float32)
    return np.ascontiguousarray(np.tile(base, (12, 1))[rng.permutation(120)])


def _line_axis():
    rng = np.random.default_rng(13)
    x = np.cumsum(rng.uniform(0.05, 0.4, 200)).astype(np.float32)
    pts = np.zeros((200, 3), np.float32)
    pts[:, 0] = x[rng.permutation(200)]
    return pts


def _line_generic():
    """(10, 20, 1) + s (3, -7, 2), s = m 2^-16 with distinct integers |m| < 2^19: along (0.3, -0.7, 0.2), at most
    23 significant bits per coordinate."""
    rng = np.random.default_rng(14)
    m = rng.choice(np.arange(-(1 << 19) + 1, 1 << 19), size=200, replace=False).astype(np.float64)
    pts = np.array([10.0, 20.0, 1.0]) + (m / 65536.0)[:, None] * np.array([3.0, -7.0, 2.0])
    out = pts.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), pts)
    return out


def _plane_axis():
    rng = np.random.default_rng(15)
    pts = (rng.standard_normal((300, 3)) * [6, 6, 0]).astype(np.float32)
    pts[:, 2] = np.float32(2.5)
    return pts


def _plane_generic():
    """(4, -3, 2) + a (2, 0, 1) + b (1, 3, -1) with a, b = integers 2^-14, |a|, |b| < 8: a tilted plane, every
    coordinate an exact float32."""
    rng = np.random.default_rng(16)
    ab = rng.integers(-(1 << 17) + 1, 1 << 17, size=(300, 2)).astype(np.float64) / 16384.0
    pts = np.array([4.0, -3.0, 2.0]) + ab[:, :1] * np.array([2.0, 0.0, 1.0]) + ab[:, 1:] * np.array([1.0, 3.0, -1.0])
    out = pts.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), pts)
    return out


def _far():
    return (_generic() + np.array([3000, -2000, 150], np.float32)).astype(np.float32)


def _small():
    return (_generic() * np.float32(1e-3)).astype(np.float32)


def _lattice():
    g = np.arange(12, dtype=np.float32)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


_BUILD = dict(generic=_generic, dup=_dup, line_axis=_line_axis, line_generic=_line_generic, plane_axis=_plane_axis,
              plane_generic=_plane_generic, far=_far, small=_small, lattice=_lattice)

CASES = {c.name: c for c in (
    Case("generic", (1, 2, 3, 4), {1: 0, 2: 1, 3: 2, 4: 3}, True),
    Case("dup", (10,), {10: 0}, False),
    Case("line_axis", (10, 20), {10: 1, 20: 1}, True),
    Case("line_generic", (10, 16, 20, 32, 64), {k: 1 for k in (10, 16, 20, 32, 64)}, True),
    Case("plane_axis", (10, 20), {10: 2, 20: 2}, True),
    Case("plane_generic", (10, 16, 20, 32, 64), {k: 2 for k in (10, 16, 20, 32, 64)}, True),
    Case("far", (10, 20), {10: 3, 20: 3}, True),
    Case("small", (10,), {10: 3}, True),
    Case("lattice", (7, 10, 20), {7: 3, 10: 3, 20: 3}, False),
)}

CASE_K = [(name, k) for name, c in CASES.items() for k in c.ks]


@lru_cache(maxsize=None)
def cloud(name):
    pts = np.ascontiguousarray(_BUILD[name](), np.float32)
    assert pts.shape[1] == 3 and len(pts) <= 2049
    pts.setflags(write=False)
    return pts
