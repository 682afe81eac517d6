"""Synthetic targets that force each path of the candidate-cell build and of its three
lookups (tests/test_grid_cases_cpu.py proves the generators, tests/test_gpu_grid_cases.py
runs them): numpy only, deterministic.

Every generator returns a ``Case``: (target f32[N,3], source f32[M,3], pose, bound,
expect).  The pose is the identity, so the fp32 query of update_correspondences equals
the source point bit for bit.  ``expect`` names the path the case must hit (the
grid_info counters asserted on the device) and what the CPU test proves of the inputs:

  name         the case's id
  tie_free     no query has two target points at a bit-equal fp32 minimum distance
  ties         {source index: number of bit-equal minima} (tie cases)
  uses_walk    grid_info()["uses_walk"]
  levels       levels l with level_cells[l] > 0
  refined      level_cells[1] + level_cells[2] + level_cells[3] > 0
  overflow     overflow_cells > 0 (True), == 0 (False)
  fallback     fallback_fine > 0 (True), == 0 (False)
  over_cap     overflow_cells > 0 or fallback_fine > 0
  min_entries  entries >= this
  walk_groups  lookup_walk_groups() > 0 (True), == 0 (False), unasserted (None)
  both         the source has matches and non-matches against the bound
  centre       the shell's centre (float64), where the case has one
  shell_n      the number of shell points (the first shell_n target points)
  pair         tie_pair: the target indices of the tied points at list positions (i, j)
  face_rows    faces: (axis, fine face 0..8, first source row) of each face's five queries
  wide         wide_box: the target indices p and d, the cell the lookup takes, the face X0

The grid geometry is restated here (``Grid``) from cellgrid_build
(dynamic_direct_lidar_odometry_amd/csrc/cellgrid_host.hip) and from the lookups' fp32 cell mapping
(cg_cell_list, csrc/gicp_types.hpp), so that queries can be placed on cell faces; the
device test asserts grid_info()["coarse_cells"] == prod(Grid.dims), so a drift of the
formula fails loudly.  The sorted target position that orders every list is restated in
``morton_order`` (morton_key, csrc/search.hpp; k_bbox_final, csrc/index_build.hip).
"""
import itertools
import math
from typing import NamedTuple

import numpy as np

import np_gicp as NP

F32 = np.float32

CELL = 0.4           # kGridCell
MAX_REACH = 4.0      # kGridMaxReach
LIST_MAX = 32        # kGridListMax: a longer list splits its cell
LIST_CAP = 2048      # kGridListCap = kCgCandMax: a longer finest-level list is not stored
ROUND = 16           # kLookupU: list entries per fused round
SLICES = 4           # k_cell_lookup: 64 / kTaskQ lanes scan one list, entry k in slice k % 4
MAX_LEVEL = 3        # kCgMaxLevel

BOUNDS = (0.5, 1.0, 5.0)
CENTRE = np.array([-1.0, -1.0, -1.0])
RADIUS = 0.3
JITTER = 4e-6        # radial, outward: see shell_points
BOX_LO, BOX_HI = -2.0, 2.0
SHELL_NS = (1, 15, 16, 17, 31, 32, 33, 48, 64, 65, 2048)
SHELL_ALL_BOUNDS = (16, 17, 33, 2048)       # the other sizes run at bound 1.0 only
SHELL_OVER_NS = (2049, 2600)
SIZES = (1, 15, 16, 17, 63, 64, 65, 255, 257)
FACE_SHIFT = np.array([-16.0, -16.0, -16.0])   # see faces()
FAR1 = np.array([4096.25, -8191.5, 1024.125])
FAR2 = FAR1 + np.array([30000.0, 0.0, 0.0])
PAIR_POSITIONS = ((0, 16), (15, 16), (0, 47))


class Case(NamedTuple):
    target: np.ndarray
    source: np.ndarray
    pose: np.ndarray
    bound: float
    expect: dict


# ---------------------------------------------------------------------------
# the build's geometry and the lookups' cell mapping, restated
class Grid:
    """cellgrid_build's grid of a target and bound (cellgrid_host.hip): the coarse cells tile the
    target's bounding box plus M on every side."""

    def __init__(self, target, bound):
        t = np.asarray(target, F32)
        lo, hi = t.min(0).astype(np.float64), t.max(0).astype(np.float64)
        cap2 = np.nextafter(F32(float(bound) * float(bound)), F32(np.inf))     # search_cap2
        self.bound = float(bound)
        self.capm = math.sqrt(float(cap2)) * (1.0 + 1e-5) + 1e-6
        self.r = int(math.ceil(min(self.capm, MAX_REACH) / CELL)) + 1
        self.M = (self.r + 1) * CELL
        self.origin = (lo - self.M).astype(F32)
        ext = hi - lo + 2 * self.M
        self.dims = np.ceil(ext / CELL).astype(np.int64) + 1
        amax = float(max(np.abs(lo).max(), np.abs(hi).max()))
        self.delta = 1e-4 + 4e-6 * (amax + self.M + CELL)
        self.nomatch_dist = (self.r - 1) * CELL - 1e-3
        self.outside_nomatch = self.capm <= self.nomatch_dist
        self.inv_s = F32(1.0 / CELL)
        self.s = 1.0 / float(self.inv_s)

    @property
    def coarse_cells(self):
        return int(np.prod(self.dims))

    def coords(self, q):
        """The lookups' fp32 grid coordinates: (q - origin) * inv_s."""
        return (np.asarray(q, F32) - self.origin) * self.inv_s

    def inside(self, q):
        t = self.coords(q)
        return np.all((t >= 0) & (t < self.dims.astype(F32)), axis=-1)

    def cell(self, q):
        """Coarse cell of queries inside the grid box (cg_cell_list)."""
        return np.minimum(self.coords(q).astype(np.int64), self.dims - 1)

    def fine(self, q, level):
        """Fine cell (per axis) of the queries at a level (cg_cell_list's fine index)."""
        t = self.coords(q)
        c = self.cell(q)
        m = 1 << level
        return np.minimum(((t - c.astype(F32)) * F32(m)).astype(np.int64), m - 1)

    def box(self, cell, level=0, fine=(0, 0, 0)):
        """(centre float64[3], half size) of a fine cell's box, expanded by delta (fine_box)."""
        sz = self.s / (1 << level)
        c = self.origin.astype(np.float64) + np.asarray(cell, np.float64) * self.s + (np.asarray(fine, np.float64) + 0.5) * sz
        return c, 0.5 * sz + self.delta

    def face(self, axis, k, f=0):
        """fp32 coordinate of coarse face k plus f level-3 fine cells, on an axis."""
        return F32(float(self.origin[axis]) + (k + f / 8.0) * CELL)


def morton_order(target):
    """The target's sorted order (a stable sort of the 63-bit Morton keys, x in the lowest
    bit) and the keys: list entries follow the sorted position."""
    t = np.asarray(target, F32)
    lo, hi = t.min(0), t.max(0)
    ext = F32(max(hi - lo))
    scale = F32(2097151.0) / ext if ext > 0 else F32(1.0)
    f = np.clip((t - lo) * scale, F32(0.0), F32(2097151.0))
    q = f.astype(np.uint64)
    key = np.zeros(len(t), np.uint64)
    for bit in range(21):
        for a in range(3):
            key |= ((q[:, a] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + a)
    return np.argsort(key, kind="stable"), key


def box_dist(p, c, hb):
    e = np.maximum(np.abs(np.asarray(p, np.float64) - c) - hb, 0.0)
    return np.sqrt((e * e).sum(-1))


def far_dist(p, c, hb):
    e = np.abs(np.asarray(p, np.float64) - c) + hb
    return np.sqrt((e * e).sum(-1))


def list_radius_bounds(target, c, hb, capm):
    """Bounds (lo, hi) of a cell's list radius R = min(D, capm) (1 + 1e-5) + 1e-6
    (list_radius2, csrc/cellgrid.hip): D is the smallest farthest-corner distance of the
    cell's dominators, which are target points (so D >= the minimum over the target) and
    include the point nearest to the box centre (so D <= its farthest-corner distance)."""
    t = np.asarray(target, np.float64)
    far = far_dist(t, c, hb)
    near = int(np.argmin(((t - c) ** 2).sum(1)))
    widen = lambda D: min(D * (1.0 + 2e-6), capm) * (1.0 + 1e-5) + 1e-6
    return widen(far.min()), widen(far[near])


def dominated_by_any(points, c, hb):
    """Per point: some other point dominates it over the box (dominated(), cellgrid.hip,
    in float64 and with half its rounding margin, so a False here is a False there)."""
    p = np.asarray(points, np.float64) - c
    n2 = (p * p).sum(1)
    out = np.zeros(len(p), bool)
    for i in range(len(p)):
        l1 = np.abs(p[i] - p).sum(1)
        f = (n2[i] - n2) - 2.0 * hb * l1
        f[i] = -1.0
        out[i] = bool((f > 1e-5 * (n2[i] + n2 + 6 * hb * hb)).any())
    return out


def brute(target, source):
    """Per query: (fp32 minimum squared distance, its lowest index, number of bit-equal minima)."""
    t = np.asarray(target, F32)
    q = np.asarray(source, F32)
    d = NP.nanoflann_sqd(q[:, None, :], t[None, :, :])
    m = d.min(1)
    return m, d.argmin(1), (d == m[:, None]).sum(1)


# ---------------------------------------------------------------------------
# building blocks
def anchors():
    """The 8 corners of [-2, 2]^3 and 24 points of it at 1.5 m or more from the shell's
    centre: the bounding box spans several cells, and no anchor is on a list of the cells
    about the centre."""
    rng = np.random.default_rng(7)
    pts = [np.array(c) for c in itertools.product((BOX_LO, BOX_HI), repeat=3)]
    while len(pts) < 32:
        p = rng.uniform(BOX_LO, BOX_HI, 3)
        if np.linalg.norm(p - CENTRE) >= 1.5:
            pts.append(p)
    return np.array(pts)


def sphere_dirs(n, seed):
    """n well-separated unit vectors: a Fibonacci lattice under a seeded rotation."""
    rng = np.random.default_rng(seed)
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * math.pi * (3.0 - math.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    d = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return d @ Q.T


def shell_points(n, seed=11):
    """n points at RADIUS (+ up to JITTER, outward) from CENTRE, float64.  Two points at
    one distance from a point of a box never dominate each other over it (the linear
    minimum of dominated() is <= 0 there), so the cells that hold the centre carry all n;
    the jitter keeps the squared radii 0.6 * 4e-6 = 2.4e-6 apart at most, below the margin
    of dominated() (2e-5 * (0.09 + 0.09 + 6 hb^2) >= 3.6e-6)."""
    rng = np.random.default_rng(seed + n)
    return CENTRE + sphere_dirs(n, seed + n) * (RADIUS + rng.uniform(0.0, JITTER, n))[:, None]


def _queries(grid, centre, rng, near=256, around=256, line=32):
    """Near the centre (within 0.1 m), across the 27 coarse cells about it, and three
    lines through it that leave the grid box by 1 m on each side."""
    v = rng.standard_normal((near, 3))
    v *= (0.1 * rng.uniform(0, 1, near) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    q = [centre + v, centre + rng.uniform(-1.5 * CELL, 1.5 * CELL, (around, 3))]
    for a in range(3):
        ln = centre + rng.uniform(-0.05, 0.05, (line, 3))
        o = float(grid.origin[a])
        ln[:, a] = np.linspace(o - 1.0, o + grid.dims[a] * CELL + 1.0, line)
        q.append(ln)
    return np.concatenate(q)


def _case(name, target64, source64, bound, shift=None, **expect):
    shift = np.zeros(3) if shift is None else shift
    e = dict(name=name, tie_free=True, ties={}, uses_walk=int(bound > 1.0), levels=[], refined=None, overflow=None,
             fallback=None, over_cap=False, min_entries=1, walk_groups=False if bound <= 1.0 else None, both=True)
    e.update(expect)
    return Case(np.ascontiguousarray(target64 + shift, F32), np.ascontiguousarray(source64 + shift, F32), np.eye(4), float(bound), e)


def _grid_of(target64, bound, shift=None):
    return Grid((target64 + (0.0 if shift is None else shift)).astype(F32), bound)


# ---------------------------------------------------------------------------
# the cases
def shell(n, bound, shift=None, name=None):
    """n shell points about the centre of a coarse cell, and the anchors.  n > LIST_MAX:
    the centre's cell is refined to level 3 and keeps all n there; n = LIST_CAP is stored."""
    tgt = np.concatenate([shell_points(n), anchors()])
    g = _grid_of(tgt, bound, shift)
    sh = np.zeros(3) if shift is None else shift
    src = _queries(g, CENTRE + sh, np.random.default_rng(100 + n)) - sh
    over = n > LIST_CAP
    levels = [0] if n <= LIST_MAX else [3] if n < LIST_CAP else [2, 3]   # (long lists: the cells about refine too)
    return _case(name or f"shell{n}", tgt, src, bound, shift, levels=levels,
                 overflow=None if over else False, fallback=None if over else False, over_cap=over,
                 min_entries=0 if over else n,
                 uses_walk=1 if over else int(bound > 1.0), walk_groups=True if over else (False if bound <= 1.0 else None),
                 centre=CENTRE + sh, shell_n=n, tie_free=shift is None)


def shell_over(n, bound):
    """Above LIST_CAP: the centre's coarse cell overflows kCgCandMax, is split directly, and
    its finest cells about the centre are not stored (the walk answers their queries)."""
    return shell(n, bound, name=f"shell_over{n}")


def dense_cube(bound, n=2600):
    """n uniform points inside one coarse cell (none dominated over it: each is the nearest
    point of itself): the coarse candidates overflow, the direct level-1 split and the
    levels below give short lists."""
    rng = np.random.default_rng(23)
    tgt = np.concatenate([CENTRE + rng.uniform(-0.5 * CELL + 1e-3, 0.5 * CELL - 1e-3, (n, 3)), anchors()])
    g = _grid_of(tgt, bound)
    src = _queries(g, CENTRE, np.random.default_rng(24))
    return _case("dense_cube", tgt, src, bound, overflow=True, fallback=False, refined=True, levels=[1, 2, 3], min_entries=n, centre=CENTRE,
                 shell_n=n)


TIE_ABC = (0.25, 0.15625, 0.0625)   # dyadic, |(a, b, c)| = 0.3013: every sum of squares below is exact in fp32
TIE_T, TIE_U = 0.03125, 0.015625


def signed_perms(v):
    out = []
    for p in itertools.permutations(v):
        for s in itertools.product((1.0, -1.0), repeat=3):
            out.append(np.array(p) * np.array(s))
    return np.array(out)


def tie_rounds(bound):
    """The 48 signed permutations of (a, b, c) about the centre: 48 bit-equal fp32 distances
    from it, one list of 48 = three fused rounds, twelve entries in each slice.  Queries off
    the centre along an axis, a face diagonal, the space diagonal and in a symmetry plane
    tie 8, 4, 6 and 2 ways."""
    tgt = np.concatenate([CENTRE + signed_perms(TIE_ABC), anchors()])
    t, u = TIE_T, TIE_U
    q, ties = [np.zeros(3)], {0: 48}
    for a in range(3):
        for s in (1.0, -1.0):
            b, c = (a + 1) % 3, (a + 2) % 3
            for off, mult in (({a: t}, 8), ({a: t, b: t}, 4), ({a: t, b: u}, 2), ({a: t, b: t, c: t}, 6)):
                v = np.zeros(3)
                for k, x in off.items():
                    v[k] = s * x
                ties[len(q)] = mult
                q.append(v)
    rng = np.random.default_rng(31)
    src = np.concatenate([CENTRE + np.array(q), CENTRE + rng.uniform(-0.1, 0.1, (40, 3))])
    return _case("tie_rounds", tgt, src, bound, tie_free=False, ties=ties, levels=[3], overflow=False, fallback=False,
                 min_entries=48, both=False, centre=CENTRE, shell_n=48)


def tie_pair(pos, bound):
    """Two tied points at list positions pos = (i, j) of a list of 48.  How the positions
    are controlled: the list of the centre's cell is the 48 shell points in sorted (Morton)
    order.  A and B are sign flips of one dyadic vector about the centre (bit-equal
    distances from it); the 46 others lie JITTER-scale farther out and are chosen from
    well-separated candidates by their Morton keys: i below A's, j - i - 1 between A's and
    B's, 47 - j above B's.  The first (A, B) of the signed permutations that leaves enough
    candidates in each range is taken."""
    i, j = pos
    anc = anchors()
    rng = np.random.default_rng(41)
    cand = CENTRE + sphere_dirs(700, 43) * (np.linalg.norm(TIE_ABC) + rng.uniform(2e-6, JITTER, 700))[:, None]
    flips = [np.array(s) for s in itertools.product((1.0, -1.0), repeat=3)][1:]
    for v in signed_perms(TIE_ABC):
        for fl in flips:
            A, B = CENTRE + v, CENTRE + v * fl
            ok = (np.linalg.norm(cand - A, axis=1) > 0.03) & (np.linalg.norm(cand - B, axis=1) > 0.03)
            pts = np.concatenate([np.array([A, B]), cand[ok], anc])
            _, key = morton_order(pts.astype(F32))
            kA, kB, kc = key[0], key[1], key[2:2 + int(ok.sum())]
            if not kA < kB or len(np.unique(key[:2 + len(kc)])) != 2 + len(kc):
                continue
            below, between, above = np.flatnonzero(kc < kA), np.flatnonzero((kc > kA) & (kc < kB)), np.flatnonzero(kc > kB)
            if len(below) < i or len(between) < j - i - 1 or len(above) < 47 - j:
                continue
            pick = np.concatenate([below[:i], between[:j - i - 1], above[:47 - j]])
            # B first: nanoflann keeps the tied point it meets first, here the lower index, which is
            # the higher list position -- a lookup that misses the tie answers A and fails
            tgt = np.concatenate([np.array([B, A]), cand[ok][pick], anc])
            src = np.concatenate([CENTRE[None], CENTRE + np.random.default_rng(47).uniform(-0.1, 0.1, (62, 3))])
            return _case(f"tie_pair_{i}_{j}", tgt, src, bound, tie_free=False, ties={0: 2}, levels=[3], overflow=False,
                         fallback=False, min_entries=48, both=False, centre=CENTRE, shell_n=48, pair=(1, 0), positions=pos)
    raise AssertionError(f"no tied pair at positions {pos}")


def faces(bound, shift=FACE_SHIFT, name="faces"):
    """shell(48), refined to level 3 about the centre.  On each axis, for the faces of the
    centre's coarse cell and the seven level-3 fine faces between them: the fp32 face
    coordinate and its +-1 and +-2 ulp neighbours, the other two coordinates random inside
    the cell.  The cloud is shifted to -17 m so that one ulp of the query coordinate is
    coarser than the rounding of the lookup's (q - origin) * inv_s: the neighbours then
    really map to different cells (the CPU test asserts it)."""
    tgt = np.concatenate([shell_points(48), anchors()])
    g = _grid_of(tgt, bound, shift)
    c = CENTRE + shift
    kc = g.cell(c.astype(F32))
    rng = np.random.default_rng(53)
    q, face_rows = [], []
    for a in range(3):
        for f in range(9):
            x0 = g.face(a, int(kc[a]), f)
            xs = [x0]
            for _ in range(2):
                xs = [np.nextafter(xs[0], F32(-np.inf))] + xs + [np.nextafter(xs[-1], F32(np.inf))]
            base = c + rng.uniform(-0.5 * CELL + 0.02, 0.5 * CELL - 0.02, 3)
            face_rows.append((a, f, len(q)))          # rows len(q) .. + 4: -2, -1, 0, +1, +2 ulp
            for x in xs:
                p = base.astype(F32)
                p[a] = x
                q.append(p.astype(np.float64))
    q = np.array(q) - shift
    q = np.concatenate([q, _queries(g, c, np.random.default_rng(54), near=64, around=64, line=8) - shift])
    return _case(name, tgt, q, bound, shift, levels=[3], overflow=False, fallback=False, min_entries=48, centre=c, shell_n=48,
                 face_rows=face_rows, tie_free=np.array_equal(shift, FACE_SHIFT))


def far_origin(bound):
    """shell(33) and faces far from the origin: delta grows with the coordinates and the
    fp32 query loses its low bits (ties among the rounded points are the oracle's to order)."""
    return [shell(33, bound, FAR1, "far1_shell33"), faces(bound, FAR1, "far1_faces"),
            shell(33, bound, FAR2, "far2_shell33"), faces(bound, FAR2, "far2_faces")]


def degenerate(kind, bound):
    """Targets whose bounding box collapses in one or more dimensions; queries on and off
    them, within the bound and beyond it."""
    rng = np.random.default_rng(61)
    if kind == "one":
        tgt = np.array([[0.3, -0.2, 0.1]])
    elif kind == "coincident":
        tgt = np.array([[0.3, -0.2, 0.1], [0.3, -0.2, 0.1]])
    elif kind == "collinear":
        tgt = np.stack([0.05 * np.arange(64), np.zeros(64), np.zeros(64)], 1)
    else:
        i, j = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
        tgt = np.stack([0.05 * i.ravel(), 0.05 * j.ravel(), np.zeros(1024)], 1)
    lo, hi = tgt.min(0), tgt.max(0)
    on = tgt[rng.integers(0, len(tgt), 24)]
    near = rng.uniform(lo - 0.3, hi + 0.3, (150, 3))
    far = rng.uniform(lo - 1.3 * bound - 1.0, hi + 1.3 * bound + 1.0, (83, 3))
    src = np.concatenate([on, near, far])
    tie = kind == "coincident"
    return _case(f"degenerate_{kind}", tgt, src, bound, tie_free=not tie, overflow=False, fallback=False, min_entries=1,
                 dup=tie)


DEGENERATE = ("one", "coincident", "collinear", "planar")

WIDE = 400.0        # half extent of wide_box on x
WIDE_A = 0.19


def margin_dominated(p, d, c, hb):
    """dominated() of csrc/cellgrid.hip with its margin, in float64: d beats p at every point
    of the box (centre c, half size hb) by more than the margin."""
    p, d = np.asarray(p, np.float64) - c, np.asarray(d, np.float64) - c
    p2, d2 = (p * p).sum(), (d * d).sum()
    f = (p2 - d2) - 2.0 * hb * np.abs(p - d).sum()
    return f > 2e-5 * (p2 + d2 + 6.0 * hb * hb) + 1e-12


def wide_box(bound):
    """A grid 800 m long: near its far end (q - origin) * inv_s rounds by tens of micrometres,
    so a query just before a coarse face X0 maps into the cell C behind it (the rounding
    goes that way only).  Two points on the face's normal, d inside C and p before the
    face, with their bisector plane between that query and X0: d beats p over the unexpanded C by more than dominated()'s margin,
    so only the delta expansion (which covers the mapping's rounding) keeps p, the query's
    nearest point, on C's list.  Source row 0 is that query."""
    corners = np.array(list(itertools.product((-WIDE, WIDE), (-2.0, 2.0), (-2.0, 2.0))))
    g = Grid(corners.astype(F32), bound)
    ox = float(g.origin[0])
    best = None
    for k in range(int(g.dims[0]) - 60, int(g.dims[0]) - int(g.M / CELL) - 8):
        X0 = ox + k * CELL
        x = F32(X0)
        for _ in range(16):
            x = np.nextafter(x, F32(-np.inf))
            t = (x - g.origin[0]) * g.inv_s            # the lookup's fp32 mapping
            if float(x) < X0 and int(t) == k and (best is None or X0 - float(x) > best[0]):
                best = (X0 - float(x), k, x)
    mq, k, qx = best
    X0 = ox + k * CELL
    jc = g.cell(np.array([0.1, 0.1, 0.1], F32))
    yc, zc = (g.box(jc)[0][1:]).astype(F32).astype(np.float64)
    px = F32(X0 - WIDE_A)
    dx = F32(2.0 * (X0 - 0.6 * mq) - float(px))
    pair = np.array([[float(px), yc, zc], [float(dx), yc, zc]])
    rng = np.random.default_rng(71)
    filler = np.array([float(qx), yc, zc]) + rng.uniform(-1.5, 1.5, (40, 3)) * [8.0, 1.0, 1.0]
    filler = filler[np.linalg.norm(filler - pair[0], axis=1) > 1.0]
    tgt = np.concatenate([pair, filler, corners])
    xs = [qx]
    for _ in range(3):
        xs = [np.nextafter(xs[0], F32(-np.inf))] + xs + [np.nextafter(xs[-1], F32(np.inf))]
    q = [[float(qx), yc, zc]] + [[float(x), yc, zc] for x in xs if x != qx]
    q = np.concatenate([np.array(q), np.array([float(qx), yc, zc]) + rng.uniform(-0.6, 0.6, (120, 3)),
                        rng.uniform([-WIDE - 8, -8, -8], [WIDE + 8, 8, 8], (64, 3))])
    keep = brute(tgt.astype(F32), q.astype(F32))[2] == 1     # (a neighbour exactly on the bisector is dropped)
    keep[0] = True
    return _case("wide_box", tgt, q[keep], bound, overflow=False, fallback=False, min_entries=2,
                 wide=dict(p=0, d=1, cell=(k, int(jc[1]), int(jc[2])), X0=X0))


def sizes(bound):
    """shell(33)'s target and queries: the device test runs the prefixes SIZES of the source."""
    return shell(33, bound)


def shell_runs():
    """(n, bound) of the shell sweep."""
    return [(n, b) for n in SHELL_NS for b in BOUNDS if b == 1.0 or n in SHELL_ALL_BOUNDS]


def tie_free_cases():
    """Every case called tie-free, at every bound it runs at (the CPU test brute-forces them)."""
    out = [shell(n, b) for n, b in shell_runs()]
    for b in BOUNDS:
        out += [shell_over(n, b) for n in SHELL_OVER_NS] + [dense_cube(b), faces(b)]
        out += [degenerate(k, b) for k in DEGENERATE if k != "coincident"] + [wide_box(b)]
    return out
