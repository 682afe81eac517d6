"""numpy restatement (float64) of the range-image projection of an unorganized cloud
(include/ddlo_seg_project.h), written from the definition there:

    invalid      any coordinate non-finite, or x == y == z == 0
    e  = atan2(z, sqrt(x*x + y*y)) * (180 / pi);  qr = (elev_top - e) / elev_res;  row = floor(qr + 0.5)
    out of view  unless 0 <= row < rows
    a  = atan2(y, x) * (180 / pi);  qc = azim_sign * (a - azim0) / (360.0 / cols);  c = floor(qc + 0.5)
    col = ((c mod cols) + cols) mod cols
    the highest input index wins a pixel

and the undecided analysis of tests/test_gpu_residual_image.py: the device's and the host's atan2 may differ
by an ulp or so, so a point whose row, column or kept-status changes when e or a moves by +-4 double ulps is
undecided (an atan2 with a zero argument is exact: no move there), and a pixel is excluded from a comparison
only if an undecided point can reach it and outranks the decided points' winner there.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

DEG = 180.0 / np.pi


@dataclass
class Projection:
    """ddlo_seg_projection: the members are float32 values (what the C struct holds), promoted on use."""
    elev_top: float
    elev_res: float
    azim0: float = 0.0
    azim_sign: int = 1

    def __post_init__(self):
        self.elev_top = float(np.float32(self.elev_top))
        self.elev_res = float(np.float32(self.elev_res))
        self.azim0 = float(np.float32(self.azim0))


def default_projection(rows: int, ang_bottom: float) -> Projection:
    """ddlo_seg_default_projection: elev_res = 2 ang_bottom / float(rows - 1) in float32."""
    ab = np.float32(ang_bottom)
    return Projection(float(ab), float(np.float32(np.float32(2) * ab) / np.float32(rows - 1)), 0.0, 1)


def angles(points, de=0, da=0):
    """(valid, e, a) in degrees; de / da move an angle by that many double ulps where both arguments of its
    atan2 are non-zero."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(p).all(axis=1) & ~((p[:, 0] == 0) & (p[:, 1] == 0) & (p[:, 2] == 0))
        x, y, z = (np.where(valid, v, 1.0) for v in (x, y, z))
        rxy = np.sqrt(x * x + y * y)
        e, a = np.arctan2(z, rxy), np.arctan2(y, x)
        e = np.where((z != 0) & (rxy != 0), e + de * np.spacing(e), e)
        a = np.where((x != 0) & (y != 0), a + da * np.spacing(a), a)
    return valid, e * DEG, a * DEG


def quotients(points, proj: Projection, rows: int, cols: int, de=0, da=0):
    """(valid, qr, qc): the float64 quotients whose rounding is a point's row and (unwrapped) column."""
    valid, e, a = angles(points, de, da)
    qr = (proj.elev_top - e) / proj.elev_res
    qc = proj.azim_sign * (a - proj.azim0) / (360.0 / cols)
    return valid, qr, qc


def pixels(points, proj: Projection, rows: int, cols: int, de=0, da=0):
    """(valid, kept, row, col): kept = valid and in view; row / col are meaningful where kept."""
    valid, qr, qc = quotients(points, proj, rows, cols, de, da)
    row = np.floor(qr + 0.5)
    kept = valid & (row >= 0) & (row < rows)
    c = np.floor(qc + 0.5)
    col = np.mod(np.mod(c, cols) + cols, cols)       # exact in float64 (fmod-like on integers)
    row = np.where(kept, row, 0).astype(np.int64)
    col = np.where(kept, col, 0).astype(np.int64)
    return valid, kept, row, col


def project(points, proj: Projection, rows: int, cols: int):
    """The projection: dict(winner (rows, cols) int32, pixel_of_point (n,) int32, and the counts of
    ddlo_seg_projection_result)."""
    n = len(np.asarray(points).reshape(-1, 3))
    valid, kept, row, col = pixels(points, proj, rows, cols)
    pix = np.where(kept, row * cols + col, -1).astype(np.int32)
    winner = np.full(rows * cols, -1, np.int64)
    np.maximum.at(winner, pix[kept], np.flatnonzero(kept))
    occupied = int((winner >= 0).sum())
    invalid = int((~valid).sum())
    oov = int((valid & ~kept).sum())
    return dict(winner=winner.astype(np.int32).reshape(rows, cols), pixel_of_point=pix, points=n, invalid=invalid,
                out_of_view=oov, occupied_pixels=occupied, collisions=n - invalid - oov - occupied)


def analyse(points, proj: Projection, rows: int, cols: int):
    """What the restatement alone says about a cloud in one geometry: project() plus the undecided points and
    the excluded pixels (rows, cols) bool."""
    out = project(points, proj, rows, cols)
    n = out["points"]
    _, kept, row, col = pixels(points, proj, rows, cols)
    moved = [pixels(points, proj, rows, cols, de, da)[1:] for de in (-4, 0, 4) for da in (-4, 0, 4)]
    undecided = np.zeros(n, bool)
    for k2, r2, c2 in moved:
        undecided |= (k2 != kept) | (kept & k2 & ((r2 != row) | (c2 != col)))
    decided = np.full(rows * cols, -1, np.int64)
    m = kept & ~undecided
    np.maximum.at(decided, (row * cols + col)[m], np.flatnonzero(m))
    excluded = np.zeros(rows * cols, bool)
    for k2, r2, c2 in moved:
        m = undecided & k2
        pix = (r2 * cols + c2)[m]
        excluded[pix[np.flatnonzero(m) > decided[pix]]] = True
    out.update(kept=kept, row=row, col=col, undecided=undecided, excluded=excluded.reshape(rows, cols))
    return out


def direction(elev_deg: float, azim_deg: float, r: float = 10.0) -> np.ndarray:
    """The float32 point at range r with that elevation and azimuth (atan2(y, x))."""
    e, a = np.deg2rad(elev_deg), np.deg2rad(azim_deg)
    return np.array([r * np.cos(e) * np.cos(a), r * np.cos(e) * np.sin(a), r * np.sin(e)], np.float32)


def hand_points(proj: Projection, rows: int, cols: int):
    """The hand points of the tests for one geometry (default-like projections: azim0 0, sign +1), as
    [(name, xyz float32, expectation)] with expectation one of
      ("pixel", row or None, col)   kept, decided, at that column (and row, if given)
      ("oov",)                       valid, out of view, decided
      ("invalid",)
      ("undecided",)                 exactly on a half-integer quotient
    """
    w = 360.0 / cols
    mid_e = proj.elev_top - proj.elev_res * (rows // 2)           # the elevation of row rows // 2
    at_q = lambda q: proj.elev_top - q * proj.elev_res            # the elevation whose qr is q
    pts = []
    # (3, 4, 5): sqrt(x*x + y*y) = 5 = z exactly, so e = 45 degrees; where that is a half-integer qr (the
    # 3 x 7 image's projection is chosen so) the point sits exactly between two rows
    half_q = (proj.elev_top - 45.0) / proj.elev_res
    if (half_q * 2) % 2 == 1 and -1 < half_q < rows:
        pts.append(("half-integer qr", np.array([3, 4, 5], np.float32), ("undecided",)))
    zenith_q = (proj.elev_top - 90.0) / proj.elev_res
    assert zenith_q + 0.5 < 0, "the hand points assume that the zenith is out of view"
    pts += [
        ("+x", np.array([1, 0, 0], np.float32), ("pixel", None, 0)),
        ("+y", np.array([0, 1, 0], np.float32), ("pixel", None, cols // 4 if cols % 4 == 0 else None)),
        ("-x", np.array([-1, 0, 0], np.float32), ("pixel", None, cols // 2 if cols % 2 == 0 else None)),
        ("-y", np.array([0, -1, 0], np.float32), ("pixel", None, 3 * cols // 4 if cols % 4 == 0 else None)),
        ("azimuth just below 360", direction(mid_e, 360.0 - 0.25 * w), ("pixel", rows // 2, 0)),
        ("negative azimuth", direction(mid_e, -1.0 * w), ("pixel", rows // 2, cols - 1)),
        ("zenith", np.array([0, 0, 1], np.float32), ("oov",)),
        ("qr -0.49", direction(at_q(-0.49), 0.3 * w), ("pixel", 0, 0)),
        ("qr rows-0.51", direction(at_q(rows - 0.51), 0.3 * w), ("pixel", rows - 1, 0)),
        ("qr -0.51", direction(at_q(-0.51), 0.3 * w), ("oov",)),
        ("qr rows-0.49", direction(at_q(rows - 0.49), 0.3 * w), ("oov",)),
        ("origin", np.zeros(3, np.float32), ("invalid",)),
        ("nan", np.array([np.nan, 1, 1], np.float32), ("invalid",)),
        ("+inf", np.array([1, np.inf, 1], np.float32), ("invalid",)),
    ]
    return pts


def wrap_case(proj: Projection, rows: int, cols: int):
    """A point whose qc rounds to cols itself: with azim0 = -180 the quotient runs over (0, cols], and an
    azimuth a quarter column below +180 degrees gives cols - 0.25.  Returns (projection, xyz, (row, col))."""
    w = 360.0 / cols
    q = Projection(proj.elev_top, proj.elev_res, -180.0, 1)
    mid_e = proj.elev_top - proj.elev_res * (rows // 2)
    return q, direction(mid_e, 180.0 - 0.25 * w), (rows // 2, 0)


# ---- the inputs the tests share -------------------------------------------------------------------
def cast(rows, cols):
    """The ray-cast organized frame (sensor frame) the tests use: the moving-pedestrian scene from a pose with
    a little roll, pitch and yaw.  The scene is closed (ground, facades): every pixel has a return."""
    from dynamic_direct_lidar_odometry_amd import scene
    sc = scene.make_scene(1005, moving=True)
    pose = scene.make_pose([0.5, 0.3, scene.SENSOR_Z], (0.01, -0.02, 0.3))
    return scene.raycast(sc, pose, rows, cols, seed=7, organized=True)


def blank(frame, rows, cols, block, seed):
    """10 % of the pixels and one block of block = (rows, cols) pixels set to NaN (seeded)."""
    rng = np.random.default_rng(seed)
    f = np.array(frame, np.float32)
    f[rng.random(rows * cols) < 0.10] = np.nan
    r0, c0 = int(rng.integers(0, rows - block[0])), int(rng.integers(0, cols - block[1]))
    f.reshape(rows, cols, 3)[r0:r0 + block[0], c0:c0 + block[1]] = np.nan
    return f


# the 3 x 7 image's projection: rows at 60, 30 and 0 degrees (so that (3, 4, 5) lies exactly between two rows),
# column 0 at 10 degrees (with 0 the frames' column at 180 degrees would sit on the boundary qc = 3.5)
SMALL_PROJECTION = Projection(60.0, 30.0, 10.0, 1)
