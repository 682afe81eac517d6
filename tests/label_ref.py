"""TEST INFRASTRUCTURE ONLY — the order-free formulation of the range-image
labelling, in plain Python: what the device labelling
(csrc/seg_label.hip) computes, stage by stage, with no breadth-first search
over whole components.

The segments of cloudSegmentation / labelComponents (detection.cpp:510-724,
oracle/segment_ref.py:label_components) are the connected components of an
undirected graph on the eligible pixels (label-init 0, inside the window) as
long as the window does not reach outside the columns.  From that:

  components   union-find, the larger root hooked under the smaller: the root
               is the seed, the component's smallest row-major index;
  statistics   size, distinct rows of the non-seed pixels, largest range,
               min_z: all independent of the visiting order;
  max_z        the reference's if / else-if makes it the maximum over the
               pushes that did not take the minimum.  Only a prefix of the
               push sequence has to be replayed literally: up to the first push
               p whose z is non-zero, not NaN and not a new strict minimum.
               After p every minimum-taker lies below max_z, so the rest
               contributes the plain maximum of its non-NaN z;
  numbering    feasible components 1, 2, ... in seed order, the rest 999999;
  residual     the positive residuals of the non-seed pixels summed in double
               in row-major order, divided by their count.  The reference sums
               them in float in push order: the two differ by at most
               (m + 1) 2^-24 of the value (m float additions and one float
               division, each within 2^-24 relative, all terms positive).

Shared by tests/test_label_ref_cpu.py and tests/test_gpu_label_device.py: the
random generator and the hand-built cases of the two live here as well.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from oracle import segment_ref as R

F32 = np.float32
REJECTED = R.REJECTED
NEIGHBOURS = [(-1, 0), (0, 1), (0, -1), (1, 0)]   # neighbor_iterator_ (detection.cpp:133-145)


def window(p):
    """The labelling window with the rows clamped; the columns must lie inside the image."""
    if p.win_col0 < 0 or p.win_col1 > p.cols - 1:
        raise ValueError("the window reaches outside the columns: the result depends on the visiting order")
    return max(0, p.win_row0), min(p.rows - 1, p.win_row1), p.win_col0, p.win_col1


class _Edge:
    """The reference's angle test between two neighbouring pixels (symmetric in the two)."""

    def __init__(self, p, rng):
        self.rng = rng
        self.sx, self.cx, self.sy, self.cy = R._trig(p.rows, p.cols, p.ang_bottom)
        self.theta = F32(p.theta)

    def __call__(self, a, b, vertical):
        ra, rb = self.rng[a], self.rng[b]
        d1, d2 = max(ra, rb), min(ra, rb)
        sa, ca = (self.sy, self.cy) if vertical else (self.sx, self.cx)
        return bool(R.atan2f(F32(d2 * sa), F32(d1 - F32(d2 * ca))) > self.theta)


def _find(parent, x):
    while parent[x] != x:   # roots only decrease along the chain
        x = parent[x]
    return x


def label_components(p, rng, z, label, sensor_z, residual=None, stats=None):
    """(label, avg_residuals, segments) as oracle.segment_ref.label_components returns them,
    by the order-free formulation.  stats (a dict) receives 'replayed' (components that reached
    the prefix replay) and 'longest_prefix' (pushes replayed, the stopping one included)."""
    H, W = p.rows, p.cols
    rng = np.asarray(rng, np.float32).reshape(H, W)
    z = np.asarray(z, np.float32).reshape(H, W)
    res = None if residual is None else np.asarray(residual, np.float32).reshape(H, W)
    out = np.asarray(label, np.int32).reshape(H, W).copy()
    r0, r1, c0, c1 = window(p)
    edge = _Edge(p, rng)
    elig = np.zeros((H, W), bool)
    elig[r0:r1 + 1, c0:c1 + 1] = out[r0:r1 + 1, c0:c1 + 1] == 0

    # 1. components: each undirected edge (right, down) once, larger root under the smaller
    parent = {(i, j): (i, j) for i in range(r0, r1 + 1) for j in range(c0, c1 + 1) if elig[i, j]}
    for a in list(parent):
        i, j = a
        for b, vertical in (((i, j + 1), False), ((i + 1, j), True)):
            if b in parent and edge(a, b, vertical):
                ra, rb = _find(parent, a), _find(parent, b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    # 2. lists in (seed, row-major pixel) order
    comps = {}
    for a in sorted(parent):
        comps.setdefault(_find(parent, a), []).append(a)

    n_replayed, longest = 0, 0
    label_count = 1
    avg = [0.0]
    for seed in sorted(comps):
        pix = comps[seed]
        rest = pix[1:]   # the seed is the list's first entry
        # 3. order-free statistics
        n = len(pix)
        lines = len({a[0] for a in rest})
        max_dist = max(rng[a] for a in pix) if n >= 2 else F32(-1e6)
        zs = [z[a] for a in rest if z[a] != 0 and not math.isnan(z[a]) and z[a] < F32(1e6)]
        min_z = min(zs) if zs else F32(1e6)
        feasible = (n >= 50 and lines >= p.min_line_num) or (n >= p.valid_point_num and lines >= p.valid_line_num)
        feasible = feasible and bool(max_dist <= F32(p.max_distance))
        feasible = feasible and bool(F32(min_z - F32(sensor_z)) <= F32(p.max_elevation))
        if feasible:
            # 4. the literal prefix of the push sequence
            n_replayed += 1
            marked = {seed}
            queue = [seed]
            lit_min, max_z = F32(1e6), F32(-1e6)
            stop = False
            pushes = 0
            while queue and not stop:
                f = queue.pop(0)
                for dy, dx in NEIGHBOURS:
                    t = (f[0] + dy, f[1] + dx)
                    if t not in parent or t in marked or not edge(f, t, dx == 0):
                        continue
                    marked.add(t)
                    queue.append(t)
                    pushes += 1
                    zz = z[t]
                    if zz < lit_min and zz != 0:
                        lit_min = zz
                    else:
                        if zz > max_z:
                            max_z = zz
                        if zz != 0 and not math.isnan(zz):
                            stop = True
                            break
            longest = max(longest, pushes)
            # 5. the rest in any order
            for a in rest:
                if a not in marked and not math.isnan(z[a]) and z[a] > max_z:
                    max_z = z[a]
            dz = F32(max_z - min_z)
            feasible = bool(F32(p.min_delta_z) <= dz <= F32(p.max_delta_z))
        if feasible:
            a = 0.0
            if res is not None:
                terms = [float(res[q]) for q in rest if res[q] > 0]
                total = 0.0
                for v in terms:
                    total += v
                a = total / len(terms) if terms else 0.0
            avg.append(a)
            for q in pix:
                out[q] = label_count
            label_count += 1
        else:
            for q in pix:
                out[q] = REJECTED
    if stats is not None:
        stats["replayed"] = n_replayed
        stats["longest_prefix"] = longest
    return out, np.array(avg), label_count - 1


def residual_terms(label, residual, segments):
    """m per label: the positive residuals among a segment's pixels without its seed (the
    first in row-major order)."""
    flat = np.asarray(label).reshape(-1)
    res = np.asarray(residual, np.float32).reshape(-1)
    m = [0]
    for l in range(1, segments + 1):
        idx = np.nonzero(flat == l)[0][1:]
        m.append(int((res[idx] > 0).sum()))
    return m


def assert_avg_within_bound(avg, ref_avg, m):
    """|avg - ref| <= (m + 1) 2^-24 ref per label: the reference's m float additions and one
    float division of positive terms, against a double sum (whose own error is 2^-29 of that)."""
    assert len(avg) == len(ref_avg) == len(m)
    for l in range(len(m)):
        bound = (m[l] + 1) * 2.0 ** -24 * abs(ref_avg[l])
        assert abs(avg[l] - ref_avg[l]) <= bound, (l, avg[l], ref_avg[l], m[l])


# ---- the inputs both test files use ----

def params(rows, cols, **kw):
    """The ddlo_seg_params fields the labelling reads (an attribute bag for the oracle)."""
    d = dict(rows=rows, cols=cols, ang_bottom=15.0, theta=math.radians(60.0), valid_point_num=3, min_line_num=1,
             valid_line_num=1, min_delta_z=0.1, max_delta_z=3.0, max_distance=30.0, max_elevation=2.0, win_row0=0,
             win_row1=rows - 1, win_col0=0, win_col1=cols - 1)
    d.update(kw)
    return SimpleNamespace(**d)


def random_case(seed):
    """One 20 x 30 image of the random generator: (p, range, z, label-init, sensor_z, residual)."""
    g = np.random.default_rng(seed)
    H, W = 20, 30
    p = params(H, W, valid_point_num=int(g.integers(1, 6)), min_line_num=int(g.integers(0, 4)),
               valid_line_num=int(g.integers(0, 4)), min_delta_z=float(g.choice([-3e6, 0.0, 0.1, 0.5])),
               max_distance=float(g.choice([8.0, 30.0])), max_elevation=float(g.choice([0.5, 2.0])),
               win_row0=int(g.integers(0, 4)), win_row1=int(g.integers(15, 20)), win_col0=int(g.integers(0, 5)),
               win_col1=int(g.integers(22, 30)))
    depth = g.choice([3.0, 5.0, 9.0, 14.0], size=(H // 4, W // 5))
    rng = (np.kron(depth, np.ones((4, 5))) * (1.0 + 0.01 * g.normal(size=(H, W)))).astype(np.float32)
    init = np.where(g.random((H, W)) < 0.25, -1, 0).astype(np.int32)
    rows, cols = np.mgrid[0:H, 0:W]
    kind = seed % 4
    if kind == 0:
        z = g.choice([-1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 2.0], size=(H, W))
    elif kind == 1:
        z = 2.0 - 0.2 * rows + 0.05 * g.normal(size=(H, W))
    elif kind == 2:
        z = 2.0 - 0.2 * rows - 0.01 * cols
    else:
        z = g.normal(size=(H, W))
    z = z.astype(np.float32)
    z[g.random((H, W)) < 0.05] = 0.0
    z[g.random((H, W)) < 0.03] = np.nan
    resid = np.abs(g.normal(0, 0.2, (H, W))).astype(np.float32)
    resid[g.random((H, W)) < 0.3] = 0.0
    return p, rng, z, init, 0.3, resid


def _blank(H, W, **kw):
    """Nothing eligible, range 5 m (every neighbouring pair of equal range passes the angle
    test at 15 degrees ang_bottom and these sizes), z = 1."""
    p = params(H, W, **kw)
    return p, np.full((H, W), 5.0, np.float32), np.ones((H, W), np.float32), np.full((H, W), -1, np.int32)


def hand_cases():
    """name -> (p, range, z, label-init, sensor_z, residual, expected) where expected is a dict
    of known answers: 'segments', and optionally 'labels' {(row, col): label}."""
    out = {}
    resid = lambda H, W: (np.arange(H * W, dtype=np.float32).reshape(H, W) % 7) * 0.125

    # a 1-pixel-wide column with strictly falling z: every push takes the minimum, max_z stays -1e6
    p, rng, z, init = _blank(64, 8)
    init[2:62, 3] = 0
    z[2:62, 3] = 3.0 - 0.04 * np.arange(60, dtype=np.float32)
    out["falling_pole_rejected"] = (p, rng, z, init, 0.3, resid(64, 8), dict(segments=0, labels={(2, 3): REJECTED, (61, 3): REJECTED}))
    # the same with one repeated z: that push goes to the else branch
    z2 = z.copy()
    z2[30, 3] = z2[29, 3]
    out["pole_one_repeat_accepted"] = (p, rng, z2, init, 0.3, resid(64, 8), dict(segments=1, labels={(2, 3): 1, (61, 3): 1}))
    # pushes with z = 5, 0, 3 in BFS order (seed (1, 1): right (1, 2), down (2, 1), then (1, 3) from (1, 2)):
    # the zero goes to the else branch (max_z = 0), 3 takes the minimum: dz = -3
    p3, rng, z, init = _blank(6, 8, valid_point_num=3, valid_line_num=1, min_delta_z=-4.0, max_elevation=8.0)
    for a, v in (((1, 1), 9.0), ((1, 2), 5.0), ((2, 1), 0.0), ((1, 3), 3.0)):
        init[a] = 0
        z[a] = v
    out["zero_goes_to_else"] = (p3, rng, z, init, 0.3, resid(6, 8), dict(segments=1, labels={(1, 3): 1}))
    out["zero_goes_to_else_rejected"] = (params(6, 8, valid_point_num=3, valid_line_num=1, min_delta_z=-2.5, max_elevation=8.0), rng, z, init,
                                         0.3, resid(6, 8), dict(segments=0, labels={(1, 3): REJECTED}))
    # a singleton (rejected: min_z stays 1e6, above any elevation), and a component whose seed row
    # holds only the seed: 2 lines, not 3
    p, rng, z, init = _blank(8, 8, valid_point_num=1, valid_line_num=0, min_delta_z=-3e6)
    init[1, 1] = 0
    init[3, 4] = init[4, 4] = init[5, 4] = 0
    z[4, 4], z[5, 4] = 0.5, 0.5
    out["singleton_and_seed_row"] = (p, rng, z, init, 0.3, resid(8, 8), dict(segments=1, labels={(1, 1): REJECTED, (3, 4): 1}))
    out["seed_row_not_counted"] = (params(8, 8, valid_point_num=1, valid_line_num=3, min_delta_z=-3e6), rng, z, init, 0.3,
                                   resid(8, 8), dict(segments=0, labels={(3, 4): REJECTED}))
    # two blobs touching only diagonally stay two components
    p, rng, z, init = _blank(8, 8, valid_point_num=4, valid_line_num=1, min_delta_z=0.0)
    init[1:3, 1:3] = 0
    init[3:5, 3:5] = 0
    out["diagonal_blobs"] = (p, rng, z, init, 0.3, resid(8, 8), dict(segments=2, labels={(2, 2): 1, (3, 3): 2}))
    # a range pair that passes vertically and fails horizontally: 8 x 64 at 45 degrees has
    # ang_res_y = 12.86 deg, ang_res_x = 5.625 deg; the pair (5, 5.5) m makes 1.059 rad
    # vertically and 0.752 rad horizontally, theta = 0.9.  A 2 x 2 checkerboard of the two
    # ranges: every edge is that pair, only the vertical ones join
    p, rng, z, init = _blank(8, 64, ang_bottom=45.0, valid_point_num=2, valid_line_num=1, min_delta_z=-3e6, theta=0.9)
    init[3:5, 10:12] = 0
    rng[3, 10], rng[3, 11], rng[4, 10], rng[4, 11] = 5.0, 5.5, 5.5, 5.0
    out["vertical_passes_horizontal_fails"] = (p, rng, z, init, 0.3, resid(8, 64),
                                               dict(segments=2, labels={(3, 10): 1, (4, 10): 1, (3, 11): 2, (4, 11): 2}))
    # a component cut by the window border: the part outside stays unlabelled
    p, rng, z, init = _blank(10, 12, valid_point_num=4, valid_line_num=1, min_delta_z=0.0, win_row0=2, win_row1=7,
                             win_col0=3, win_col1=8)
    init[1:6, 6:11] = 0
    out["window_cut"] = (p, rng, z, init, 0.3, resid(10, 12), dict(segments=1, labels={(2, 6): 1, (5, 8): 1, (1, 6): 0, (3, 9): 0}))
    # feasible and rejected components interleaved in seed order: 2-pixel pairs are too small
    p, rng, z, init = _blank(12, 16, valid_point_num=4, valid_line_num=1, min_delta_z=0.0)
    for k, c in enumerate((1, 4, 7, 10, 13)):
        if k % 2 == 0:
            init[1 + k:3 + k, c:c + 2] = 0       # 2 x 2 blob
        else:
            init[1 + k, c:c + 2] = 0             # pair
    out["interleaved_numbering"] = (p, rng, z, init, 0.3, resid(12, 16),
                                    dict(segments=3, labels={(1, 1): 1, (2, 4): REJECTED, (3, 7): 2, (4, 10): REJECTED, (5, 13): 3}))
    return out


def serpentine_case(cols):
    """40 x cols: one serpentine component (full rows joined at alternating ends, every other
    row) next to about 200 singletons below it."""
    H = 40
    p, rng, z, init = _blank(H, cols, valid_point_num=10, valid_line_num=2, min_delta_z=0.0)
    turns = 0
    for r in range(0, 24, 2):
        init[r, :] = 0
        if r + 2 < 24:
            init[r + 1, cols - 1 if turns % 2 == 0 else 0] = 0
            turns += 1
    g = np.random.default_rng(cols)
    z[:24] = (0.3 * g.normal(size=(24, cols))).astype(np.float32)
    k = 0
    for r in range(25, H, 2):
        for c in range(k % 3, cols, max(3, (cols * 8) // 200)):
            init[r, c] = 0
        k += 1
    resid = np.abs(g.normal(0, 0.2, (H, cols))).astype(np.float32)
    return p, rng, z, init, 0.3, resid
