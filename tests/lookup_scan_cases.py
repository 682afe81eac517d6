"""Inputs for the fused lookup's key-only scan (k_moments<*, true>, csrc/moments.hip: every
round of 16 entries is loaded from one address, up to 15 entries past the list's end, and
scanned without a branch; an entry past the end must reach neither the key nor the second
distance; the match's coordinates are loaded after the scan), built from
tests/grid_cases.py and tests/lookup_tail_cases.py as they are.
tests/test_lookup_scan_cases_cpu.py proves what is said of them here,
tests/test_gpu_lookup_scan.py runs them.  numpy only, deterministic.

``member_case(n, bound)``: GC.shell(n, bound)'s target and one query per shell point, NUDGE
from the centre towards it: the query's cell lists exactly the n shell points (in sorted
order), and its nearest point is "its" member, so over the case's n queries every list
position is the winner once -- the first, the inner ones and the last entry of a list that
ends inside a round.  One wavefront (n <= 64), no tie.

``face_case(n, bound)``: shell(n) for an n that is refined to level 3, and queries on both
sides of the three fine faces through the centre: neighbouring fine cells, both lists the
n shell points, so one list's over-read meets the other's copies of the same points.

``pair_case(pos, total, bound)``: GC.tie_pair's construction for a list of ``total`` entries
-- two points at a bit-equal distance from the centre at list positions pos = (i, j), the
reference's choice the one at the higher position (the lower target index), so a scan
that misses the tie answers the other one.  GC.tie_pair itself where total is its 48.
"""
import itertools

import numpy as np

import grid_cases as GC
import lookup_tail_cases as LT

F32 = np.float32

E0 = LT.E0                   # kTailE0: entries every lane scans alone (two common rounds)
ROUND = GC.ROUND             # kLookupU
BOUNDS = (0.5, 1.0)          # the fused lookup answers (uses_walk == 0)
NUDGE = 1e-3
MEMBER_N = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49)
FACE_N = (41, 49)            # refined (> LIST_MAX); 9 and 1 entries in the remainder chunk
FACE_EPS = (2e-4, 7e-4)
TEAM = (161, 9)              # lookup_tail_cases.team_case: F = 4, nine remainder chunks

# (positions, list length): where the two tied entries lie
PAIRS_ONE_ROUND = (((0, 1), 2), ((0, 1), 10), ((0, 9), 10), ((3, 12), 13), ((0, 15), 16))
PAIRS_TWO_ROUNDS = (((0, 16), 17), ((15, 16), 20), ((0, 19), 20), ((5, 27), 28), ((0, 31), 32))
PAIRS_REMAINDER = (((0, 32), 33), ((31, 32), 41), ((0, 40), 41), ((33, 40), 41), ((0, 47), 48), ((35, 47), 48))
PAIRS = PAIRS_ONE_ROUND + PAIRS_TWO_ROUNDS + PAIRS_REMAINDER


def member_case(n, bound):
    sh = GC.shell(n, bound)
    pts = GC.shell_points(n)
    d = (pts - GC.CENTRE) / np.linalg.norm(pts - GC.CENTRE, axis=1)[:, None]
    e = dict(sh.expect)
    e.update(name=f"member_n{n}", tie_free=True, both=False)
    return GC.Case(sh.target, np.ascontiguousarray(GC.CENTRE + NUDGE * d, F32), np.eye(4), float(bound), e)


def list_position(target, n):
    """Per shell point (the first n target points): its position in a list of all n."""
    order = GC.morton_order(target)[0]
    listed = [int(k) for k in order if k < n]
    pos = np.empty(n, np.int64)
    pos[listed] = np.arange(n)
    return pos


def face_case(n, bound):
    sh = GC.shell(n, bound)
    rng = np.random.default_rng(300 + n)
    q = []
    for a in range(3):
        for eps in FACE_EPS:
            for s in (-1.0, 1.0):
                v = rng.uniform(1e-4, 9e-4, 3) * rng.choice([-1.0, 1.0], 3)
                v[a] = s * eps
                q.append(GC.CENTRE + v)
    e = dict(sh.expect)
    e.update(name=f"face_n{n}", both=False)
    return GC.Case(sh.target, np.ascontiguousarray(np.array(q), F32), np.eye(4), float(bound), e)


def pair_case(pos, total, bound):
    i, j = pos
    assert 0 <= i < j < total
    if total == 48:
        case = GC.tie_pair(pos, bound)
        assert LT.ref_choice(case) == case.expect["pair"][1]
        return case
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
            # spread the picks over each range, so that a short list is not one cluster
            take = lambda r, m: r[np.linspace(0, len(r) - 1, m).astype(np.int64)] if m else r[:0]
            pick = np.concatenate([take(below, i), take(between, j - i - 1), take(above, total - 1 - j)])
            tgt = np.concatenate([np.array([B, A]), cand[ok][pick], anc])
            src = np.concatenate([GC.CENTRE[None], GC.CENTRE + np.random.default_rng(47).uniform(-0.1, 0.1, (62, 3))])
            case = GC._case(f"scan_pair_{i}_{j}_of{total}", tgt, src, bound, tie_free=False, ties={0: 2}, levels=[],
                            overflow=False, fallback=False, min_entries=total, both=False, centre=GC.CENTRE,
                            shell_n=total, pair=(1, 0), positions=pos)
            if LT.ref_choice(case) == 0 and GC.brute(case.target, case.source)[2][1:].max() == 1:
                return case
    raise AssertionError(f"no tied pair at positions {pos} of {total}")


def team():
    return LT.team_case(*TEAM)
