"""Inputs for the fused lookup's remainder phase (k_moments<*, true>, csrc/moments.hip: lists
longer than E0 entries are finished by teams of the wavefront's lanes), built from
tests/grid_cases.py as it is.  tests/test_lookup_tail_cases_cpu.py proves what is said of
them here, tests/test_gpu_lookup_tail.py runs them.  numpy only, deterministic.

``team_case(n, H)``: GC.shell(n, 1.0)'s target plus one distant point FAR, and a source of
exactly 64 queries = one wavefront: H heavy ones within 1 mm of the shell's centre (their
cell lists all n shell points) and 64 - H light ones: about FAR (their cell lists FAR
alone) and, ``before(n, H)`` of them, about OUT, outside the grid box (no list at all).  The
device orders a source by its Morton keys, so the wavefront's lanes are: the OUT queries,
then the heavy ones, then the FAR ones -- the heavy lanes' ranks differ from their lanes
and the block of heavy lanes straddles team boundaries.
The shell's own "around" queries cannot serve as light ones: their cells touch the shell,
the list radius of such a cell covers the whole shell, and what the dominance test then
removes is not provable with GC.Grid's list rule (the CPU test records the radius rule's
count for them).  FAR lies beyond the box on the + side, so the grid's origin and the cells
about the centre are the shell case's own.

``seam_pair(pos, bound)``: GC.tie_pair(pos, bound) where that case does what the tests need
-- the tied points at list positions pos, and the reference's choice the one at the higher
position, so that a lookup which misses the tie answers the other one.  GC.tie_pair builds
a list of 48, which cannot hold a position beyond 47, and for the positions from 48 on
its result (a longer list, by its slicing) has the reference choose the lower position.
For those, the same construction is repeated here with a list of SEAM_TOTAL entries, and
the first (A, B) is taken for which the reference chooses the higher position.
"""
import itertools

import numpy as np

import grid_cases as GC
from oracle import oracle as O

F32 = np.float32

E0 = 32                      # kTailE0: entries every lane scans alone
ROUND = GC.ROUND             # kLookupU: a team member's chunk
BOUND = 1.0
FAR = np.array([6.1, 5.9, 6.3])
OUT = np.array([-9.3, -9.1, -9.2])
HEAVY_R = 1e-3
LIGHT_R = 0.05

TEAM_H = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
TEAM_N = (E0 + 1, E0 + 15, E0 + 16, E0 + 17, E0 + 16 * 8 + 1, 2048)
EDGE_N = (E0 - 1, E0, E0 + 1, E0 + 16, E0 + 17)
EDGE_PREFIXES = (1, 63, 65)
PAIR_POSITIONS = ((0, E0), (E0 - 1, E0), (E0, E0 + 16), (E0 + 15, E0 + 16), (E0 + 3, E0 + 40), (E0 + 1, E0 + 2))
PAIR_BOUNDS = (0.5, 1.0)
SEAM_TOTAL = 96              # list length of the pairs with a position beyond 47
SHARD_N = E0 + 17
ALIGN_N = E0 + 33


def team_size(H, cap=64):
    """F of a wavefront with H heavy lanes: the largest power of two with H F <= 64."""
    F = 1
    while H * 2 * F <= 64 and 2 * F <= cap:
        F *= 2
    return F


def _ball(rng, m, radius):
    v = rng.standard_normal((m, 3))
    return v * (radius * rng.uniform(0, 1, m) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]


def before(n, H):
    """The number of light lanes in front of the heavy ones: a few, or (n + H even) nearly all
    of them, which puts heavy lanes among the lanes of idle teams (lanes from H F on)."""
    x = (5 * H + n) % 13
    return min(64 - H, 1 + x) if (n + H) % 2 else max(64 - H - x % 3, 0)


def team_target(n):
    return np.ascontiguousarray(np.concatenate([GC.shell(n, BOUND).target, FAR[None].astype(F32)]))


def team_case(n, H):
    """(Case, heavy mask): 64 queries, H of them heavy, spread over the wavefront's lanes."""
    tgt = team_target(n)
    rng = np.random.default_rng(1000 * n + H)
    # heavy candidates: tie-free ones only (the brute force is then a third reference)
    cand = (GC.CENTRE + _ball(rng, 96, HEAVY_R)).astype(F32)
    cand = cand[GC.brute(tgt, cand)[2] == 1][:H]
    assert len(cand) == H
    a = before(n, H)
    light = np.concatenate([OUT + _ball(rng, a, LIGHT_R), FAR + _ball(rng, 64 - H - a, LIGHT_R)]).astype(F32)
    src = np.concatenate([cand, light])
    heavy = np.arange(64) < H
    perm = rng.permutation(64)
    src, heavy = np.ascontiguousarray(src[perm]), heavy[perm]
    e = dict(GC.shell(n, BOUND).expect)
    e.update(name=f"team_n{n}_H{H}", tie_free=True, both=False, min_entries=n + 1)
    return GC.Case(tgt, src, np.eye(4), BOUND, e), heavy


def lanes_of(source):
    """The device's wavefronts: 64 consecutive queries of the source in its sorted order."""
    order = GC.morton_order(source)[0]
    return [order[i:i + 64] for i in range(0, len(order), 64)]


def final_cells(grid, q):
    """(level, centre, half size) of the cell a query maps to at every level."""
    q = np.asarray(q, F32)
    c = grid.cell(q)
    return [(lv,) + grid.box(c, lv, grid.fine(q, lv)) for lv in range(GC.MAX_LEVEL + 1)]


def list_bounds(target, grid, q):
    """Per level: (lower, upper) bound of the length of the list of the query's cell, by the
    list rule's radius alone (GC.list_radius_bounds) -- the lower one counts only points
    that no other point dominates (GC.dominated_by_any)."""
    t = np.asarray(target, np.float64)
    out = []
    for lv, bc, hb in final_cells(grid, q):
        Rlo, Rhi = GC.list_radius_bounds(t, bc, hb, grid.capm)
        d = GC.box_dist(t, bc, hb)
        kept = (d <= Rlo) & ~GC.dominated_by_any(t, bc, hb)
        out.append((lv, int(kept.sum()), int((d <= Rhi).sum())))
    return out


def ref_choice(case):
    """The reference's match of the case's first query (nanoflann's own order)."""
    return int(O.knn(case.target, case.source[:1], 1)[0][0, 0])


def seam_pair(pos, bound):
    i, j = pos
    if j < 48:
        case = GC.tie_pair(pos, bound)
        assert ref_choice(case) == case.expect["pair"][1]
        return case
    total = SEAM_TOTAL
    anc = GC.anchors()
    rng = np.random.default_rng(41)
    cand = GC.CENTRE + GC.sphere_dirs(700, 43) * (np.linalg.norm(GC.TIE_ABC) + rng.uniform(2e-6, GC.JITTER, 700))[:, None]
    flips = [np.array(s) for s in itertools.product((1.0, -1.0), repeat=3)][1:]
    for v in GC.signed_perms(GC.TIE_ABC):
        for fl in flips:
            A, B = GC.CENTRE + v, GC.CENTRE + v * fl
            ok = (np.linalg.norm(cand - A, axis=1) > 0.03) & (np.linalg.norm(cand - B, axis=1) > 0.03)
            pts = np.concatenate([np.array([A, B]), cand[ok], anc])
            _, key = GC.morton_order(pts.astype(F32))
            kA, kB, kc = key[0], key[1], key[2:2 + int(ok.sum())]
            if not kA < kB or len(np.unique(key[:2 + len(kc)])) != 2 + len(kc):
                continue
            below, between, above = np.flatnonzero(kc < kA), np.flatnonzero((kc > kA) & (kc < kB)), np.flatnonzero(kc > kB)
            if len(below) < i or len(between) < j - i - 1 or len(above) < total - 1 - j:
                continue
            pick = np.concatenate([below[:i], between[:j - i - 1], above[:total - 1 - j]])
            tgt = np.concatenate([np.array([B, A]), cand[ok][pick], anc])
            src = np.concatenate([GC.CENTRE[None], GC.CENTRE + np.random.default_rng(47).uniform(-0.1, 0.1, (62, 3))])
            case = GC._case(f"seam_pair_{i}_{j}", tgt, src, bound, tie_free=False, ties={0: 2}, levels=[3], overflow=False,
                            fallback=False, min_entries=total, both=False, centre=GC.CENTRE, shell_n=total, pair=(1, 0),
                            positions=pos)
            if ref_choice(case) == 0 and GC.brute(case.target, case.source)[2][1:].max() == 1:
                return case
    raise AssertionError(f"no tied pair at positions {pos}")
