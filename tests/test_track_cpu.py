"""The object tracker (include/ddlo_track.h) through the C-ABI against the
Python restatement tests/track_ref.py and the reference's Hungarian
assignments (tests/golden/hungarian_ref.npz, tests/golden/make_track_golden.py).
No GPU: the tracker has no device work.

Parity of the IoU, the Kalman filter and the filter's status machine with the
reference is unpinned (Eigen is not available to compile them from it): both
sides here are restatements of the same source lines, written separately.
"""
import os

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd.tracking as T
from dynamic_direct_lidar_odometry_amd.segmentation import OBJECT_DTYPE

import track_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
N_SEQ, N_FRAMES = 50, 40


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "hungarian_ref.npz"))
    mats, at, ar = [], 0, 0
    for (r, c) in z["shapes"]:
        mats.append((z["costs"][at:at + r * c].reshape(r, c), z["assign"][ar:ar + r]))
        at += r * c
        ar += r
    return z, mats


def test_fixture_covers_the_shapes(golden):
    z, mats = golden
    sh = [tuple(m.shape) for m, _ in mats]
    assert len(mats) >= 300
    assert (1, 1) in sh and (40, 40) in sh
    assert any(r == 1 and c > 1 for r, c in sh) and any(c == 1 and r > 1 for r, c in sh)
    assert any(1 < r < c for r, c in sh) and any(r > c > 1 for r, c in sh) and any(r == c > 1 for r, c in sh)
    assert any(np.all(m == m.flat[0]) and m.size > 1 for m, _ in mats)
    assert any(np.all(m == 0) for m, _ in mats)
    # the reference does not return on every NaN matrix: the project's rule is IoU 0 for a 0 / 0 pair
    assert not z["nan_terminated"].all()


def test_assign_reproduces_the_reference(golden):
    _, mats = golden
    for m, a in mats:
        np.testing.assert_array_equal(T.assign(m), a, err_msg=f"shape {m.shape}")


def test_restated_hungarian_reproduces_the_reference(golden):
    _, mats = golden
    for m, a in mats:
        assert R.hungarian(m) == list(a), f"shape {m.shape}"


def test_assign_rejects_nan():
    with pytest.raises(Exception):
        T.assign(np.array([[np.nan, 1.0], [1.0, 0.5]]))


def test_default_params_are_the_yaml():
    p = T.default_track_params()
    assert (p.max_no_hits, p.min_dynamic_hits, p.max_undefined_hits) == (30, 5, 1)
    assert (p.max_obj_velocity, p.min_dist_from_origin, p.residuum_height_ratio) == (15.0, 0.75, 0.3)


# ---------------------------------------------------------------- random sequences
def make_objects(rows):
    """rows: (id, num_points, state7, avg_residuum)"""
    o = np.zeros(len(rows), OBJECT_DTYPE)
    for k, (i, n, s, a) in enumerate(rows):
        o[k]["id"], o[k]["num_points"], o[k]["state"], o[k]["avg_residuum"] = i, n, s, a
    return o


def sequence(seed):
    """40 frames of 0-12 objects: actors are born, walk, pause, vanish for a few frames and cross; frame 0
    and one later frame have no detections; until the first detection there are no tracks."""
    rng = np.random.default_rng(1000 + seed)
    n_act = int(rng.integers(4, 13))
    actors = []
    for a in range(n_act):
        birth = int(rng.integers(1, 22))
        life = int(rng.integers(3, 40))
        pos = rng.uniform(-12, 12, 2)
        speed = rng.choice([0.0, 0.0, 0.8, 1.5, 3.0, 8.0])
        ang = rng.uniform(0, 2 * np.pi)
        if a % 4 == 1 and actors:                   # head for an earlier actor: they cross
            tgt = actors[-1]["pos"]
            ang = float(np.arctan2(tgt[1] - pos[1], tgt[0] - pos[0]))
            speed = max(speed, 0.8)
        actors.append(dict(birth=birth, death=birth + life, pos=pos, vel=speed * np.array([np.cos(ang), np.sin(ang)]),
                           pause=(int(rng.integers(0, 40)), int(rng.integers(0, 6))),
                           gone=(int(rng.integers(0, 40)), int(rng.integers(2, 5))),
                           dims=rng.uniform(0.3, 1.6, 3), z=rng.uniform(-0.5, 1.0), yaw=rng.uniform(-0.7, 0.7),
                           npts=int(rng.integers(15, 600)), res=rng.choice([0.0, 0.05, 0.3, 0.6, 1.2])))
    # actor 0 stands far from the others for three frames and is never seen again: its filter coasts until it
    # is erased, even with max_no_hits 30; actor 1 lives throughout and jumps 5 m once: a gate rejection
    actors[0].update(birth=1, death=4, pos=np.array([30.0, 30.0]), vel=np.zeros(2), gone=(50, 0))
    actors[1].update(birth=2, death=N_FRAMES, gone=(50, 0))
    jump = int(rng.integers(10, 30))
    empty = {0, int(rng.integers(8, 35))}
    frames, dts = [], []
    for f in range(N_FRAMES):
        dt = float(rng.choice([0.1, 0.1, 0.1, 0.05, 0.2]))
        rows = []
        if f == jump:
            actors[1]["pos"] = actors[1]["pos"] + np.array([5.0, 0.0])
        for a in actors:
            if a["birth"] <= f < a["death"] and not (a["pause"][0] <= f < a["pause"][0] + a["pause"][1]):
                a["pos"] = a["pos"] + a["vel"] * dt
            visible = a["birth"] <= f < a["death"] and not (a["gone"][0] <= f < a["gone"][0] + a["gone"][1])
            if visible and f not in empty and len(rows) < 12:
                jit = rng.normal(0, 0.02, 7)
                s = np.array([a["pos"][0], a["pos"][1], a["z"], a["yaw"], *a["dims"]]) + jit
                s[4:] = np.abs(s[4:])
                rows.append((len(rows) + 1, max(1, a["npts"] + int(rng.integers(-10, 11))), s.astype(np.float32),
                             float(a["res"]) * float(rng.uniform(0.8, 1.2))))
        frames.append(make_objects(rows))
        dts.append(dt)
    params = dict(max_no_hits=int(rng.choice([2, 3, 5, 8, 30])), min_dynamic_hits=int(rng.choice([2, 3, 5])),
                  max_undefined_hits=int(rng.choice([1, 1, 3, 10])), max_obj_velocity=float(rng.choice([10.0, 15.0])),
                  min_dist_from_origin=float(rng.choice([0.5, 0.75])), residuum_height_ratio=float(rng.choice([0.0, 0.3])))
    return frames, dts, params


def run_ref(frames, dts, params):
    t = R.Tracker(R.Params(**params))
    out, seen = [], dict(match=False, gate=False, erase=False, status=False, no_det=False, no_track=False)
    prev = {}
    for objs, dt in zip(frames, dts):
        seen["no_track"] |= len(t.filters) == 0
        seen["no_det"] |= len(objs) == 0
        t.update(dt, R.dets_from(objs))
        seen["match"] |= len(t.matches) > 0
        seen["gate"] |= t.gated > 0
        seen["erase"] |= len(t.erased) > 0
        cur = {f.id: f.obj.status for f in t.filters}
        seen["status"] |= any(k in prev and prev[k] != v for k, v in cur.items())
        prev = cur
        out.append(dict(cost=t.cost.copy(), disp=t.disp.copy(), assignment=list(t.assignment), matches=list(t.matches),
                        unmatched_dets=list(t.unmatched_dets), track_of=list(t.track_of), erased=list(t.erased),
                        turned=t.turned, boxes=list(t.new_boxes),
                        tracks=[(f.id, f.obj.status, f.hits, f.sslu, list(f.kf.x), f.obj.num_points, f.obj.id,
                                 float(f.obj.avg_residuum), f.dist_to_origin(), len(f.boxes)) for f in t.filters]))
    return out, seen


@pytest.fixture(scope="module")
def sequences():
    return [(s,) + sequence(s) for s in range(N_SEQ)]


@pytest.fixture(scope="module")
def ref_runs(sequences):
    return [run_ref(fr, dts, p) for _, fr, dts, p in sequences]


def test_sequences_exercise_the_tracker(ref_runs):
    """>= 90 % of the sequences contain a match, a gate rejection, an erasure and a status change; every one
    has a frame without detections and a frame without tracks (judged on the restatement alone)."""
    full = sum(all(seen[k] for k in ("match", "gate", "erase", "status")) for _, seen in ref_runs)
    assert full >= 0.9 * N_SEQ, full
    assert all(seen["no_det"] and seen["no_track"] for _, seen in ref_runs)


def test_sequences_match_the_restatement(sequences, ref_runs):
    for (seed, frames, dts, params), (ref, _) in zip(sequences, ref_runs):
        trk = T.Tracker(T.default_track_params(**params))
        for k, (objs, dt, want) in enumerate(zip(frames, dts, ref)):
            where = f"sequence {seed} frame {k}"
            ids = trk.update(dt, objs)
            cost, disp, asg = trk.last_costs()
            assert cost.shape == want["cost"].shape, where
            np.testing.assert_array_equal(cost, want["cost"], err_msg=where)
            np.testing.assert_array_equal(disp, want["disp"], err_msg=where)
            assert list(asg) == want["assignment"], where
            assert list(ids) == want["track_of"], where
            r = trk.last
            assert (r.matches, r.created, r.erased, r.turned_dynamic, r.boxes_cleared) == (
                len(want["matches"]), len(want["unmatched_dets"]), len(want["erased"]), want["turned"],
                len(want["boxes"])), where
            assert list(trk.erased()) == want["erased"], where
            tr = trk.tracks()
            assert len(tr) == len(want["tracks"]), where
            for rec, w in zip(tr, want["tracks"]):
                assert (rec["id"], rec["status"], rec["hits"], rec["sslu"]) == w[:4], where
                np.testing.assert_array_equal(rec["state"], np.array(w[4]), err_msg=where)
                assert (rec["num_points"], rec["object_id"], rec["avg_residuum"], rec["dist_to_origin"],
                        rec["history"]) == w[5:], where
            assert (r.undefined_tracks, r.static_tracks, r.dynamic_tracks) == tuple(
                sum(1 for w in want["tracks"] if w[1] == s) for s in (0, 1, 2)), where
            boxes = trk.take_cleared_boxes()
            assert len(boxes) == len(want["boxes"]), where
            for b, w in zip(boxes, want["boxes"]):
                assert (tuple(b["position"]) + (b["orientation_z"],) + tuple(b["dimensions"])) == tuple(w), where
        trk.close()


# ---------------------------------------------------------------- hand-built cases
def obj(x, y, z=0.5, yaw=0.0, d=(0.6, 0.6, 1.0), n=100, res=1.0, id=1):
    return (id, n, np.array([x, y, z, yaw, *d], np.float32), res)


def walk(trk, xs, res=1.0, dt=0.1, d=(0.6, 0.6, 1.0)):
    """one object at (x, 0) per frame; returns the track's status after every frame"""
    out = []
    for x in xs:
        trk.update(dt, make_objects([obj(x, 0.0, res=res, d=d)]))
        out.append(int(trk.tracks()[0]["status"]))
    return out


def test_walker_turns_dynamic_exactly_at_min_dynamic_hits():
    # hits starts at 1: the fourth update is hits == 5.  0.25 m per frame: 1.0 m >= 0.75 m by then
    trk = T.Tracker(T.default_track_params(max_undefined_hits=10))
    st = walk(trk, [0.25 * k for k in range(7)])
    assert st == [T.UNDEFINED] * 4 + [T.DYNAMIC] * 3
    assert len(trk.take_cleared_boxes()) == 0          # UNDEFINED -> DYNAMIC emits no boxes


def test_travel_gate_holds_dynamic_back():
    # 0.1 m per frame: 0.75 m is reached at frame 8 (float32 0.8), well after min_dynamic_hits
    trk = T.Tracker(T.default_track_params(max_undefined_hits=100))
    st = walk(trk, [0.1 * k for k in range(10)])
    first = st.index(T.DYNAMIC)
    assert first == 8 and st[first:] == [T.DYNAMIC] * 2


def test_residuum_gate_holds_dynamic_back():
    # height 1.0 * ratio 0.3: an average residuum of 0.29 never passes, 0.31 does
    trk = T.Tracker(T.default_track_params(max_undefined_hits=10))
    assert T.DYNAMIC not in walk(trk, [0.25 * k for k in range(12)], res=0.29)
    trk = T.Tracker(T.default_track_params(max_undefined_hits=10))
    assert T.DYNAMIC in walk(trk, [0.25 * k for k in range(12)], res=0.31)


def test_undefined_to_static_then_dynamic_emits_boxes_once():
    # yaml: maxUndefinedHits 1 -> STATIC at the first update (hits 2 > 1); the STATIC check runs from the
    # next update on, whatever min_dynamic_hits says
    trk = T.Tracker(T.default_track_params())
    xs = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.4, 0.8, 1.2, 1.6]
    emitted = []
    st = []
    for x in xs:
        trk.update(0.1, make_objects([obj(x, 0.0)]))
        st.append(int(trk.tracks()[0]["status"]))
        emitted.append((trk.last.turned_dynamic, len(trk.take_cleared_boxes())))
    assert st[0] == T.UNDEFINED and st[1:9] == [T.STATIC] * 8 and st[9:] == [T.DYNAMIC] * 3   # never reverts
    assert emitted[9] == (1, 5)                        # the rolling five of the eight static frames
    assert [e for k, e in enumerate(emitted) if k != 9] == [(0, 0)] * 11
    assert trk.tracks()[0]["history"] == 0


def test_erasure_at_max_no_hits():
    trk = T.Tracker(T.default_track_params(max_no_hits=3))
    trk.update(0.1, make_objects([obj(0, 0)]))
    for k in range(1, 3):
        trk.update(0.1, make_objects([]))
        assert len(trk.tracks()) == 1 and trk.tracks()[0]["sslu"] == k
    trk.update(0.1, make_objects([]))
    assert len(trk.tracks()) == 0 and list(trk.erased()) == [0] and trk.last.erased == 1


def test_velocity_gate_splits_a_match():
    trk = T.Tracker(T.default_track_params())
    trk.update(0.1, make_objects([obj(0, 0)]))
    ids = trk.update(0.1, make_objects([obj(1.6, 0)]))   # 1.6 m > 15 m/s * 0.1 s
    tr = trk.tracks()
    assert list(ids) == [1] and trk.last.matches == 0 and trk.last.created == 1
    assert [(r["id"], r["sslu"], r["hits"]) for r in tr] == [(0, 1, 1), (1, 0, 1)]
    _, disp, asg = trk.last_costs()
    assert list(asg) == [0] and disp[0, 0] == np.float32(1.6)


def test_costs_of_identical_disjoint_and_flat_boxes():
    trk = T.Tracker(T.default_track_params())
    trk.update(0.1, make_objects([obj(0, 0, n=100), obj(5, 5, n=50, id=2)]))
    trk.update(0.1, make_objects([obj(0, 0, n=100), obj(5, 5, d=(0.6, 0.6, 0.0), n=50, id=2)]))
    cost, _, asg = trk.last_costs()
    assert list(asg) == [0, 1]
    assert abs(cost[0, 0]) < 1e-6                      # identical boxes: IoU ~ 1
    assert cost[0, 1] == np.float64(np.float32(0.8)) + np.float64(np.float32(0.1) * np.float32(0.5))   # disjoint
    assert cost[1, 1] == np.float64(np.float32(0.8))   # a flat box has no volume to share: IoU 0
    # two flat boxes: 0 / 0, IoU 0 by the project's rule
    trk.update(0.1, make_objects([obj(5, 5, d=(0.0, 0.0, 0.0), n=50)]))
    trk2 = T.Tracker(T.default_track_params())
    trk2.update(0.1, make_objects([obj(5, 5, d=(0.0, 0.0, 0.0), n=50)]))
    trk2.update(0.1, make_objects([obj(5, 5, d=(0.0, 0.0, 0.0), n=50)]))
    cost, _, _ = trk2.last_costs()
    assert cost[0, 0] == np.float64(np.float32(0.8))


def test_decide_flags_non_static_objects():
    import ctypes as C
    trk = T.Tracker(T.default_track_params())
    L = T._lib()
    flags = np.zeros(2, np.uint8)
    o = make_objects([obj(0, 0), obj(4, 4, id=2)])
    for want in ([1, 1], [0, 0]):                      # UNDEFINED at birth, STATIC after the first update
        assert L.ddlo_track_decide(trk.h, o.ctypes.data_as(C.c_void_p), 2, flags.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
        assert list(flags) == want
