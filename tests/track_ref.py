"""CPU restatement of the object tracker (include/ddlo_track.h), beside
objects_ref.py.  Test helper only: written from the reference's
src/tracking/*.cpp and include/util/bbox_iou.h, separately from
csrc/track_core.hpp, in plain Python.

  - the IoU in np.float32, cosf / sinf from the C library through ctypes;
  - the Kalman filter as scalar loops over Python floats (no BLAS: its FMA
    would change bits), a term whose left factor is exactly 0 skipped (it adds
    +-0 to a sum that started at +0, which changes no bit for finite values);
  - Buehren's Munkres with its column-major working copy and scan orders.
"""
import ctypes
import ctypes.util
import math
import sys

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.restype = _libm.sinf.restype = ctypes.c_float
_libm.cosf.argtypes = _libm.sinf.argtypes = [ctypes.c_float]

F = np.float32
UNDEFINED, STATIC, DYNAMIC = 0, 1, 2
DBL_EPSILON = sys.float_info.epsilon
DBL_MAX = sys.float_info.max


def cosf(x):
    return F(_libm.cosf(float(x)))


def sinf(x):
    return F(_libm.sinf(float(x)))


# ---- bbox_iou.h ----
def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def _line(v1, v2):                                   # Line::Line :50-55
    return (v2[1] - v1[1], v1[0] - v2[0], _cross(v2[0], v2[1], v1[0], v1[1]))


def _call(l, p):                                     # :39-42
    return l[0] * p[0] + l[1] * p[1] + l[2]


def _isect(l, o):                                    # :43-47
    w = l[0] * o[1] - l[1] * o[0]
    return ((l[1] * o[2] - l[2] * o[1]) / w, (l[2] * o[0] - l[0] * o[2]) / w)


def rectangle_vertices(cx, cy, w, h, r):             # :57-73
    angle = r
    dx = F(np.float64(w) / 2.0)
    dy = F(np.float64(h) / 2.0)
    dxcos, dxsin = dx * cosf(angle), dx * sinf(angle)
    dycos, dysin = dy * cosf(angle), dy * sinf(angle)
    return [(cx + (-dxcos - -dysin), cy + (-dxsin + -dycos)), (cx + (dxcos - -dysin), cy + (dxsin + -dycos)),
            (cx + (dxcos - dysin), cy + (dxsin + dycos)), (cx + (-dxcos - dysin), cy + (-dxsin + dycos))]


def intersection_area(cx1, cy1, w1, h1, r1, cx2, cy2, w2, h2, r2):   # :75-129
    rect2 = rectangle_vertices(cx2, cy2, w2, h2, r2)
    inter = rectangle_vertices(cx1, cy1, w1, h1, r1)
    for i in range(4):
        if len(inter) <= 2:
            break
        line = _line(rect2[i], rect2[(i + 1) % 4])
        vals = [_call(line, p) for p in inter]
        new = []
        n = len(inter)
        for k in range(n):
            s_value, t_value = vals[k], vals[(k + 1) % n]
            s, t = inter[k], inter[(k + 1) % n]
            if s_value <= 0.0:
                new.append(s)
            if s_value * t_value < 0:
                new.append(_isect(line, _line(s, t)))
        inter = new
    if len(inter) <= 2:
        return np.float64(0.0)
    area = F(0.0)
    n = len(inter)
    for i in range(n):
        p, q = inter[i], inter[(i + 1) % n]
        area = area + (p[0] * q[1] - p[1] * q[0])
    return np.float64(0.5) * np.float64(area)


def _max(a, b):                                      # std::max: (a < b) ? b : a
    return b if a < b else a


def _min(a, b):                                      # std::min: (b < a) ? b : a
    return b if b < a else a


def obb_iou(s1, s2):                                 # OBBIoU :131-157
    with np.errstate(all="ignore"):
        b1 = [F(v) for v in s1[:7]]
        b2 = [F(v) for v in s2[:7]]
        inter = intersection_area(b1[0], b1[1], b1[4], b1[5], b1[3], b2[0], b2[1], b2[4], b2[5], b2[3])
        min_1 = F(np.float64(b1[2]) - np.float64(b1[6]) / 2.0)
        min_2 = F(np.float64(b2[2]) - np.float64(b2[6]) / 2.0)
        max_1 = F(np.float64(b1[2]) + np.float64(b1[6]) / 2.0)
        max_2 = F(np.float64(b2[2]) + np.float64(b2[6]) / 2.0)
        max_min = _max(min_1, min_2)
        min_max = _min(max_1, max_2)
        height_overlap = _max(min_max - max_min, F(0.0))
        iv = F(np.float64(height_overlap) * inter)
        total = b1[4] * b1[5] * b1[6] + b2[4] * b2[5] * b2[6] - iv
        ratio = iv / total
        if ratio != ratio:                           # the project's convention for 0 / 0 (ddlo_track.h)
            return 0.0
        v = _max(ratio, F(0.0))
        v = _min(v, F(1.0))
        return float(v)


# ---- hungarian.cpp ----
def hungarian(cost):
    """assignmentoptimal (:83-210) and steps 2a .. 5 (:244-436) for a rows x cols matrix."""
    cost = np.asarray(cost, np.float64)
    R, Cn = cost.shape
    d = [[float(cost[i, j]) for i in range(R)] for j in range(Cn)]   # d[col][row]: the column-major copy
    covC, covR = [False] * Cn, [False] * R
    star = [[False] * R for _ in range(Cn)]
    prime = [[False] * R for _ in range(Cn)]

    def zero(r, c):
        return abs(d[c][r]) < DBL_EPSILON

    if R <= Cn:
        min_dim = R
        for r in range(R):
            mv = d[0][r]
            for c in range(1, Cn):
                if d[c][r] < mv:
                    mv = d[c][r]
            for c in range(Cn):
                d[c][r] -= mv
        for r in range(R):
            for c in range(Cn):
                if zero(r, c) and not covC[c]:
                    star[c][r] = True
                    covC[c] = True
                    break
    else:
        min_dim = Cn
        for c in range(Cn):
            mv = d[c][0]
            for r in range(1, R):
                if d[c][r] < mv:
                    mv = d[c][r]
            for r in range(R):
                d[c][r] -= mv
        for c in range(Cn):
            for r in range(R):
                if zero(r, c) and not covR[r]:
                    star[c][r] = True
                    covC[c] = True
                    covR[r] = True
                    break
        covR = [False] * R

    def step3():
        """returns the (row, col) step 4 starts from, running step 5 as often as needed"""
        while True:
            found = True
            while found:
                found = False
                for c in range(Cn):
                    if covC[c]:
                        continue
                    for r in range(R):
                        if not covR[r] and zero(r, c):
                            prime[c][r] = True
                            sc = 0
                            while sc < Cn and not star[sc][r]:
                                sc += 1
                            if sc == Cn:
                                return r, c
                            covR[r] = True
                            covC[sc] = False
                            found = True
                            break
            h = DBL_MAX                              # step 5
            for r in range(R):
                if not covR[r]:
                    for c in range(Cn):
                        if not covC[c] and d[c][r] < h:
                            h = d[c][r]
            assert h < DBL_MAX, "no finite uncovered element"
            for r in range(R):
                if covR[r]:
                    for c in range(Cn):
                        d[c][r] += h
            for c in range(Cn):
                if not covC[c]:
                    for r in range(R):
                        d[c][r] -= h

    while sum(covC) != min_dim:                      # step 2b
        row, col = step3()
        new = [list(x) for x in star]                # step 4
        new[col][row] = True
        sc = col
        sr = 0
        while sr < R and not star[sc][sr]:
            sr += 1
        while sr < R:
            new[sc][sr] = False
            pc = 0
            while pc < Cn and not prime[pc][sr]:
                pc += 1
            new[pc][sr] = True
            sc = pc
            sr = 0
            while sr < R and not star[sc][sr]:
                sr += 1
        star = new
        prime = [[False] * R for _ in range(Cn)]
        covR = [False] * R
        for c in range(Cn):                          # step 2a
            if any(star[c]):
                covC[c] = True
    out = [-1] * R                                   # buildassignmentvector
    for r in range(R):
        for c in range(Cn):
            if star[c][r]:
                out[r] = c
                break
    return out


# ---- kalman.cpp with bounding_box_filter.cpp's matrices ----
KN, KM = 10, 7


def _mm(A, B):
    n, m, p = len(A), len(B), len(B[0])
    out = []
    for i in range(n):
        Ai = A[i]
        row = [0.0] * p
        for k in range(m):
            a = Ai[k]
            if a == 0.0:
                continue
            Bk = B[k]
            for j in range(p):
                row[j] += a * Bk[j]
        out.append(row)
    return out


def _T(A):
    return [list(r) for r in zip(*A)]


_C = [[1.0 if i == j else 0.0 for j in range(KN)] for i in range(KM)]
_Ct = _T(_C)
_Q = [[(1.0 if i < KM else .01) if i == j else 0.0 for j in range(KN)] for i in range(KN)]


class Kalman:
    def __init__(self, x0):
        self.x = [float(v) for v in x0]
        self.P = [[(1000.0 if i < KM else 10000.0) if i == j else 0.0 for j in range(KN)] for i in range(KN)]

    def predict(self, dt):                           # kalman.cpp:69-81
        A = [[1.0 if i == j else (dt if (i < 3 and j == i + 7) else 0.0) for j in range(KN)] for i in range(KN)]
        self.x = [sum_in_order([A[i][k] * self.x[k] for k in range(KN)]) for i in range(KN)]
        AP = _mm(A, self.P)
        APAt = _mm(AP, _T(A))
        self.P = [[APAt[i][j] + _Q[i][j] for j in range(KN)] for i in range(KN)]

    def update(self, y):                             # kalman.cpp:83-92
        PCt = _mm(self.P, _Ct)
        S = _mm(_C, PCt)
        S = [[S[i][j] + (1.0 if i == j else 0.0) for j in range(KM)] for i in range(KM)]
        K = [[PCt[i][j] * (1.0 / S[j][j]) for j in range(KM)] for i in range(KN)]
        innov = [y[j] - sum_in_order([_C[j][k] * self.x[k] for k in range(KN)]) for j in range(KM)]
        self.x = [self.x[i] + sum_in_order([K[i][j] * innov[j] for j in range(KM)]) for i in range(KN)]
        KC = _mm(K, _C)
        IKC = [[(1.0 if i == k else 0.0) - KC[i][k] for k in range(KN)] for i in range(KN)]
        self.P = _mm(IKC, self.P)


def sum_in_order(terms):
    s = 0.0
    for t in terms:
        s += t
    return s


# ---- BoundingBoxFilter / TrackingModule ----
class Det:
    """Object as getObject fills it: state[7..9] = 0, avg_residuum a float."""

    def __init__(self, id, num_points, state7, avg_residuum):
        self.id = int(id)
        self.num_points = int(num_points)
        self.state = [float(F(v)) for v in state7] + [0.0, 0.0, 0.0]
        self.avg_residuum = F(avg_residuum)
        self.status = UNDEFINED

    def copy(self):
        d = Det(self.id, self.num_points, self.state[:7], self.avg_residuum)
        d.state = list(self.state)
        d.status = self.status
        return d


def dets_from(objects):
    """Det list from an OBJECT_DTYPE array (Segmentation.objects())."""
    return [Det(o["id"], o["num_points"], o["state"], o["avg_residuum"]) for o in objects]


class Params:
    def __init__(self, max_no_hits=30, min_dynamic_hits=5, max_undefined_hits=1, max_obj_velocity=15.0,
                 min_dist_from_origin=0.75, residuum_height_ratio=0.3):
        self.max_no_hits = max_no_hits
        self.min_dynamic_hits = min_dynamic_hits
        self.max_undefined_hits = max_undefined_hits
        self.max_obj_velocity = F(max_obj_velocity)
        self.min_travel_dist = float(min_dist_from_origin)
        self.res_height_ratio = float(residuum_height_ratio)


class Filter:
    def __init__(self, det, fid):                    # bounding_box_filter.cpp:3-51
        self.id = fid
        self.hits = 1
        self.sslu = 0
        self.obj = det.copy()
        self.kf = Kalman(det.state[:7] + [0.0, 0.0, 0.0])
        self.first = list(det.state[:3])
        self.cur = [0.0, 0.0, 0.0]
        self.boxes = []
        self.turned = False

    def predict(self, dt):                           # :53-62
        self.kf.predict(dt)
        self.sslu += 1

    def get_object(self):                            # :87-91
        self.obj.state = list(self.kf.x)
        return self.obj

    def update(self, det, p):                        # :64-85
        self.hits += 1
        self.sslu = 0
        old = self.obj.status
        self.obj = det.copy()
        self.obj.status = old
        s = self.obj.state
        self.cur = [s[0], s[1], s[2] - s[6] / 2]
        self.update_status(p)
        if self.obj.status == STATIC:                # updateBBoxHistory :219-243
            self.boxes.append((s[0], s[1], s[2], s[3], s[4], s[5], s[6]))
            if len(self.boxes) > 5:
                del self.boxes[0]
        self.kf.update(s[:7])

    def update_status(self, p):                      # updateDynamicStatus :169-217
        o = self.obj
        if o.status == DYNAMIC:
            self.turned = False
            return
        if o.status == UNDEFINED:
            if self.hits > p.max_undefined_hits:
                o.status = STATIC
                return
            if self.hits < p.min_dynamic_hits:
                return
        min_required = F(o.state[6] * p.res_height_ratio)
        if o.avg_residuum < min_required:
            return
        dx, dy = self.cur[0] - self.first[0], self.cur[1] - self.first[1]
        if dx * dx + dy * dy >= p.min_travel_dist * p.min_travel_dist:
            o.status = DYNAMIC
            self.turned = len(self.boxes) > 0

    def dist_to_origin(self):                        # :245-252
        if self.hits < 2:
            return 0.0
        d = [self.cur[k] - self.first[k] for k in range(3)]
        return math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


def cost_simple(d, t):                               # tracking.cpp:152-161
    a, b = d.state, t.state
    return math.sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]))


def cost_full(d, t):                                 # :172-190
    bbox_cost = 1 - obb_iou(d.state, t.state)
    np_det, np_track = F(d.num_points), F(t.num_points)
    with np.errstate(all="ignore"):
        inv = np_det / np_track if np_track >= np_det else np_track / np_det
        rel = F(1) - inv
        return float(np.float64(F(0.8)) * np.float64(bbox_cost) + np.float64(F(0.1) * rel))


class Tracker:
    def __init__(self, params=None):
        self.p = params or Params()
        self.next_id = 0
        self.filters = []
        self.cleared = []

    def update(self, dt, dets):                      # tracking.cpp:27-78
        dt32 = F(dt)                                 # update(float dt, ...)
        dtd = float(dt32)
        p = self.p
        self.matches, self.unmatched_dets, self.unmatched_states = [], [], []
        self.gated = 0
        tracked = []
        for f in self.filters:
            f.predict(dtd)
            tracked.append(f.get_object())
        self.cost = np.zeros((0, 0))
        self.disp = np.zeros((0, 0), F)
        self.assignment = []
        if not tracked:                              # associate :80-150
            self.unmatched_dets = list(range(len(dets)))
        elif dets:
            R, Cn = len(dets), len(tracked)
            self.cost = np.array([[cost_full(d, t) for t in tracked] for d in dets], np.float64)
            self.disp = np.array([[F(cost_simple(d, t)) for t in tracked] for d in dets], F)
            self.assignment = hungarian(self.cost)
            for i in range(R):
                if self.assignment[i] != -1:
                    self.matches.append((i, self.assignment[i]))
                else:
                    self.unmatched_dets.append(i)
            for j in range(Cn):
                if j not in self.assignment:
                    self.unmatched_states.append(j)
            kept = []
            for (i, j) in self.matches:
                if self.disp[i, j] > p.max_obj_velocity * dt32:
                    self.unmatched_dets.append(i)
                    self.unmatched_states.append(j)
                    self.gated += 1
                else:
                    kept.append((i, j))
            self.matches = kept
        self.track_of = [-1] * len(dets)
        for (i, j) in self.matches:
            self.filters[j].update(dets[i], p)
            self.track_of[i] = self.filters[j].id
        for i in self.unmatched_dets:
            self.filters.append(Filter(dets[i], self.next_id))
            self.track_of[i] = self.next_id
            self.next_id += 1
        self.erased = [f.id for f in self.filters if f.sslu >= p.max_no_hits]
        self.filters = [f for f in self.filters if f.sslu < p.max_no_hits]
        self.turned = 0
        self.new_boxes = []
        for f in self.filters:                       # publishBBoxes :259-275 / getStaticBBoxes :157-167
            if f.turned:
                self.new_boxes += f.boxes
                f.turned = False
                f.boxes = []
                self.turned += 1
        self.cleared += self.new_boxes
        return self.track_of

    def count(self, *statuses):
        return sum(1 for f in self.filters if f.obj.status in statuses)

    def non_static_ids(self):
        return [f.id for f in self.filters if f.obj.status != STATIC]
