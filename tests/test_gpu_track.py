"""The tracks' pixel lists on the device (include/ddlo_seg_tracks.h,
csrc/seg_tracks.hip) and the tracked driver entry (ddlo_odom_process_tracked).

Pool: synthetic 16 x 256 and 64 x 256 scans whose segments have 1, 63, 64, 65,
255, 256, 257 (and, on the taller image, 2800) pixels: every point lies 15 m
from the sensor, so pixels that touch are one segment, and blank pixels keep
the segments apart.  References: ddlo_seg_label_indices for the lists, a numpy
restatement (scan with the union of the recorded lists set to NaN, then the
crop of tests/preprocess_ref.py) for the removal.

Driver: the 12-frame moving-pedestrian sequence of tests/test_gpu_label_device.py
against ddlo_odom_process_dynamic driven by a Python ``decide`` built on
tests/track_ref.py (max_no_hits = 1: no coasting track), and with coasting
tracks against track_ref.py fed with every frame's objects(); one 18-frame run
with a ddlo_map in which the pedestrian's track goes STATIC -> DYNAMIC, its box
history is cleared from the map and later keyframes hold none of its pixels.
"""
import ctypes as C

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import scene
from dynamic_direct_lidar_odometry_amd import segmentation as S
from dynamic_direct_lidar_odometry_amd import tracking as T
import preprocess_ref as PR
import track_ref as TR

pytestmark = pytest.mark.gpu

W = 256
SMALL = [1, 63, 64, 65, 255, 256, 257]
EYE = np.eye(4, dtype=np.float32)


def synth_scan(H, sizes, seed):
    """(xyz (H*W, 3) float32 with NaN blanks, [pixel index arrays, one per size, in `sizes` order])."""
    rng = np.random.default_rng(seed)
    xyz = np.full((H * W, 3), np.nan, np.float32)
    row, col, shared = 0, 0, True
    segs = []
    for sz in sizes:
        if not (shared and sz <= W - col):
            row, col = row + 2, 0                  # a blank row above the new band
        rows_needed = -(-sz // W)
        pix = np.arange(sz) + (row * W + col)
        assert pix[-1] < H * W, "the image is too small for these sizes"
        d = rng.normal(size=(sz, 3))
        xyz[pix] = (15.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        segs.append(pix.astype(np.int32))
        if rows_needed == 1 and col + sz < W:
            col, shared = col + sz + 1, True       # one blank pixel, then the row is shared
        else:
            row, col, shared = row + rows_needed - 1, 0, False
    return xyz, segs


def synth_params(H):
    return S.default_seg_params(rows=H, cols=W, ground_rows=0, minimum_range=0, valid_point_num=1, min_line_num=0,
                                valid_line_num=0, min_delta_z=-1e7, max_delta_z=1e7, max_distance=100, max_elevation=1e7,
                                win_row0=0, win_row1=H - 1, win_col0=0, win_col1=W - 1)


def seg_of(lists, pix):
    """the segment id whose list is exactly pix"""
    for l in range(1, len(lists)):
        if len(lists[l]) == len(pix) and np.array_equal(lists[l], pix):
            return l
    raise AssertionError("the labelling did not produce the planned segment")


def without(xyz, drop, centre=(0, 0, 0), crop=0.0):
    """numpy restatement of the removal: the listed pixels NaN, non-finite points dropped, then the crop"""
    w = np.array(xyz, np.float32)
    if len(drop):
        w[np.asarray(drop)] = np.nan
    w = w[np.isfinite(w).all(axis=1)]
    return PR.crop_keep(w, crop, centre) if crop > 0 else w


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("H,sizes", [(16, SMALL), (64, SMALL + [2800])])
def test_pool_lists_stale_removal_and_growth(mode, H, sizes):
    seg = S.Segmentation(0, synth_params(H), labelling=mode)
    assert seg.tracks_stats() == (0, 0, 0)
    scans = [synth_scan(H, sizes, 1), synth_scan(H, sizes[::-1], 2), synth_scan(H, sizes[2:] + sizes[:2], 3)]
    centre = np.array([14.0, 0.0, 0.0], np.float32)
    # ---- scan 0: every segment becomes a track (track id 100 + k for sizes[k])
    xyz0, planned0 = scans[0]
    r = seg.process(xyz0, EYE)
    assert r.segments == len(sizes)
    lists0 = seg.label_indices()
    assert sorted(len(l) for l in lists0[1:]) == sorted(sizes)
    ids0 = [seg_of(lists0, p) for p in planned0]
    seg.tracks_sync([(100 + k, ids0[k]) for k in range(len(sizes))])
    held = {100 + k: lists0[ids0[k]].copy() for k in range(len(sizes))}
    for t, want in held.items():
        np.testing.assert_array_equal(seg.track_indices(t), want)
    n_lists, n_idx, cap = seg.tracks_stats()
    assert (n_lists, n_idx) == (len(sizes), sum(sizes)) and cap >= n_idx
    assert sum(sizes) <= 4096 and cap == 4096          # still the initial capacity
    # current-frame tracks only: the same cloud as ddlo_seg_static_cloud(remove_ids), bit for bit
    for ks in ([], [0], [1, 4], list(range(len(sizes)))):
        tr, sg = [100 + k for k in ks], [ids0[k] for k in ks]
        np.testing.assert_array_equal(seg.static_cloud_tracks(tr), seg.static_cloud(sg))
        np.testing.assert_array_equal(seg.static_cloud_tracks(tr, centre, 3.0), seg.static_cloud(sg, centre, 3.0))
        a, b = seg.static_cloud_tracks(tr, centre, 3.0, 0.5), seg.static_cloud(sg, centre, 3.0, 0.5)
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=0, atol=4e-6 * 15.0)   # tests/test_gpu_objects.py::voxel_close
        assert a.tobytes() == b.tobytes()                             # (and in fact the same bits)
        np.testing.assert_array_equal(seg.static_cloud_tracks(tr), without(xyz0, np.concatenate([held[t] for t in tr] + [[]]).astype(int)))
    assert len(seg.static_cloud_tracks([100, 104], centre, 3.0)) < len(seg.static_cloud_tracks([100, 104]))
    # ---- scan 1: other segments; the old lists are stale but still held and still removed
    xyz1, planned1 = scans[1]
    seg.process(xyz1, EYE)
    lists1 = seg.label_indices()
    ids1 = [seg_of(lists1, p) for p in planned1]
    for t, want in held.items():
        np.testing.assert_array_equal(seg.track_indices(t), want)
    # a frame in which nothing is set and nothing dies changes nothing
    before = seg.tracks_stats()
    seg.tracks_sync()
    assert seg.tracks_stats() == before
    # track 200 takes the largest segment of this scan: it shares pixels with stale lists
    big = int(np.argmax([len(p) for p in planned1]))
    seg.tracks_sync([(200, ids1[big])], dead_ids=[101, 103])
    del held[101], held[103]
    held[200] = lists1[ids1[big]].copy()
    shared = set(held[200].tolist()) & set(np.concatenate([held[t] for t in held if t != 200]).tolist())
    assert shared, "no pixel is in two lists: the scans do not overlap as planned"
    assert seg.tracks_stats()[:2] == (len(held), sum(len(v) for v in held.values()))
    if H == 64:
        # 3633 surviving indices + 2800 new ones: the pool grew past its initial capacity, contents kept (below)
        assert seg.tracks_stats()[1] > 4096 and seg.tracks_stats()[2] > 4096
    else:
        assert seg.tracks_stats()[2] == 4096
    for t, want in held.items():                      # unchanged across the swap
        np.testing.assert_array_equal(seg.track_indices(t), want)
    for tr in ([], [200], [100, 102, 200], sorted(held)):
        drop = np.concatenate([held[t] for t in tr] + [[]]).astype(int)
        np.testing.assert_array_equal(seg.static_cloud_tracks(tr), without(xyz1, drop))
        np.testing.assert_array_equal(seg.static_cloud_tracks(tr, centre, 3.0), without(xyz1, drop, centre, 3.0))
    np.testing.assert_array_equal(seg.static_cloud_tracks([]), seg.static_cloud([]))
    # ---- scan 2: lists set at scan 0 are two scans old
    xyz2, planned2 = scans[2]
    seg.process(xyz2, EYE)
    lists2 = seg.label_indices()
    seg.tracks_sync([(102, seg_of(lists2, planned2[0]))])          # a held track is re-set: its list is replaced
    held[102] = lists2[seg_of(lists2, planned2[0])].copy()
    for t, want in held.items():
        np.testing.assert_array_equal(seg.track_indices(t), want)
    drop = np.concatenate([held[t] for t in sorted(held)]).astype(int)
    got = seg.static_cloud_tracks(sorted(held), centre, 3.0)
    np.testing.assert_array_equal(got, without(xyz2, drop, centre, 3.0))
    assert got.tobytes() == seg.static_cloud_tracks(sorted(held), centre, 3.0).tobytes()   # two runs, the same bits
    # ---- invalid ids: GICP_EINVAL, the pool untouched
    L = S._lib()
    before = seg.tracks_stats()

    def sync_status(pairs, dead):
        a = np.array([p[0] for p in pairs], np.int32)
        b = np.array([p[1] for p in pairs], np.int32)
        d = np.array(dead, np.int32)
        return L.ddlo_seg_tracks_sync(seg.h, P._ptr(a) if len(a) else None, P._ptr(b) if len(b) else None, len(a),
                                      P._ptr(d) if len(d) else None, len(d))

    assert sync_status([(300, 0)], []) == 1 and sync_status([(300, len(sizes) + 1)], []) == 1
    assert sync_status([(300, 1)], [101]) == 1                      # 101 was released at scan 1
    assert sync_status([(300, 1), (300, 2)], []) == 1
    assert sync_status([], [999]) == 1
    n = C.c_size_t()
    c = np.zeros(3, np.float32)
    bad = np.array([101], np.int32)
    assert L.ddlo_seg_static_cloud_tracks(seg.h, P._ptr(bad), 1, P._ptr(c), 0.0, 0.0, None, 0, C.byref(n)) == 1
    assert L.ddlo_seg_track_indices(seg.h, 101, None, 0, C.byref(n)) == 1
    assert seg.tracks_stats() == before
    for t, want in held.items():
        np.testing.assert_array_equal(seg.track_indices(t), want)
    # every track released: an empty pool
    seg.tracks_sync(dead_ids=sorted(held))
    assert seg.tracks_stats()[:2] == (0, 0)
    np.testing.assert_array_equal(seg.static_cloud_tracks([]), seg.static_cloud([]))
    seg.close()


def all_tracks(segments):
    """every segment l of the last scan as track 100 + l"""
    return [(100 + l, l) for l in range(1, segments + 1)]


@pytest.mark.parametrize("mode", ["host", "device"])
def test_segments_csr_made_once_by_whoever_asks_first(mode):
    """The last scan's segments reach the device once per scan, for the tracks or for the objects, whichever
    asks first: both orders give the same lists and records, and a new scan never meets the old lists."""
    H = 16
    xyz0, _ = synth_scan(H, SMALL, 11)
    xyz1, _ = synth_scan(H, SMALL[::-1], 12)           # segment l has another length than in scan 0
    a = S.Segmentation(0, synth_params(H), labelling=mode)
    b = S.Segmentation(0, synth_params(H), labelling=mode)
    n = a.process(xyz0, EYE).segments
    assert n == len(SMALL) and b.process(xyz0, EYE).segments == n
    a.tracks_sync(all_tracks(n))                       # a: the tracks first, then the objects
    oa = a.objects()
    ob = b.objects()                                   # b: the other order
    b.tracks_sync(all_tracks(n))
    lists = a.label_indices()
    assert len(set(len(l) for l in lists[1:])) >= 3
    for l in range(1, n + 1):
        np.testing.assert_array_equal(a.track_indices(100 + l), lists[l])
        np.testing.assert_array_equal(b.track_indices(100 + l), lists[l])
    assert len(oa) == len(ob) > 0
    for f in S.OBJECT_DTYPE.names:
        np.testing.assert_array_equal(oa[f], ob[f], err_msg=f)
    for o in oa:
        assert o["num_points"] == len(lists[o["id"]])
    # a second, different scan, and only the tracks ask: the lists are this scan's
    assert a.process(xyz1, EYE).segments == n
    a.tracks_sync(all_tracks(n))
    lists1 = a.label_indices()
    assert any(len(lists1[l]) != len(lists[l]) for l in range(1, n + 1))
    for l in range(1, n + 1):
        np.testing.assert_array_equal(a.track_indices(100 + l), lists1[l])
    # ... and the objects that follow them are those of a handle that saw this scan alone
    b.process(xyz1, EYE)
    oa1, ob1 = a.objects(), b.objects()
    assert len(oa1) == len(ob1) > 0
    for f in S.OBJECT_DTYPE.names:
        np.testing.assert_array_equal(oa1[f], ob1[f], err_msg=f)
    a.close()
    b.close()


@pytest.mark.parametrize("mode", ["host", "device"])
def test_mode_switch_drops_the_scan(mode):
    """After ddlo_seg_set_labelling to the other mode the handle holds no scan: what needs one is
    GICP_EINVAL, and no track's list changes."""
    H = 16
    seg = S.Segmentation(0, synth_params(H), labelling=mode)
    xyz, _ = synth_scan(H, SMALL, 21)
    n = seg.process(xyz, EYE).segments
    assert n == len(SMALL)
    seg.tracks_sync(all_tracks(n))
    held = {t: seg.track_indices(t).copy() for t, _ in all_tracks(n)}
    assert len(set(len(v) for v in held.values())) >= 3
    before = seg.tracks_stats()
    seg.objects()
    seg.classify([(101, 0)])
    seg.labelling = "device" if mode == "host" else "host"
    for call in (seg.objects, lambda: seg.tracks_sync([(300, 1)]), lambda: seg.static_cloud([1]),
                 lambda: seg.static_cloud_tracks([101]), lambda: seg.classify([(101, 0)])):
        with pytest.raises(P.GicpError) as e:
            call()
        assert e.value.status == 1                     # GICP_EINVAL
    assert seg.tracks_stats() == before
    for t, want in held.items():
        np.testing.assert_array_equal(seg.track_indices(t), want)
    # switching back does not bring the scan back; a new scan in the new mode does
    seg.labelling = mode
    with pytest.raises(P.GicpError):
        seg.objects()
    seg.labelling = "device" if mode == "host" else "host"
    assert seg.process(xyz, EYE).segments == n
    assert len(seg.objects()) > 0
    seg.tracks_sync([(300, 1)])
    np.testing.assert_array_equal(seg.track_indices(300), seg.label_indices()[1])
    seg.close()


# ---- the driver -----------------------------------------------------------------------------------
def result_key(r):
    def g(x):
        return (x.converged, x.nr_iterations, x.iterations_run, x.lm_failed, x.lm_trials, x.num_correspondences,
                x.final_cost, bytes(np.array(x.final_hessian)), x.lm_lambda)
    return (r.status, r.scan_points, bytes(r.T), bytes(r.T_s2s), bytes(r.T_s2s_local), g(r.s2s), g(r.s2m),
            r.keyframe_added, r.num_keyframes, r.spaciousness, r.keyframe_thresh_dist)


@pytest.fixture(scope="module")
def cfg5_frames():
    """The first 12 organized 64 x 2048 frames of the moving-pedestrian sequence (sensor frame, NaN = no return)."""
    sc = scene.make_scene(1005, moving=True)
    poses = scene.trajectory(12, 1005)
    return [scene.raycast(sc, poses[k], 64, 2048, seed=1005 + k, t=0.1 * k, organized=True) for k in range(12)]


def cfg5_params():
    return S.yaml_seg_params(rows=64, cols=2048, ground_rows=20, win_row0=0, win_row1=63, win_col0=0, win_col1=2047,
                             max_distance=30)


TRACK_KW = dict(min_dynamic_hits=3, max_undefined_hits=2, max_obj_velocity=15.0, min_dist_from_origin=0.3,
                residuum_height_ratio=0.0)


@pytest.mark.parametrize("mode", ["host", "device"])
def test_tracked_equals_dynamic_without_coasting(cfg5_frames, mode):
    """max_no_hits = 1: a track that is not matched is erased in the same update, so only current-frame
    objects are ever cut: process_tracked must equal process_dynamic with a decide built on track_ref.py."""
    kw = dict(TRACK_KW, max_no_hits=1)
    runs = []
    for which in ("tracked", "dynamic"):
        od = OD.Odometry(0)
        seg = S.Segmentation(0, cfg5_params(), labelling=mode)
        trk = T.Tracker(T.default_track_params(**kw))
        ref = TR.Tracker(TR.Params(**kw))
        state = {"t": 0.0, "prev": 0.0}

        def decide(objs):
            track_of = ref.update(state["t"] - state["prev"], TR.dets_from(objs))
            state["prev"] = state["t"]
            non_static = set(ref.non_static_ids())
            return [t in non_static for t in track_of]

        frames = []
        for k, f in enumerate(cfg5_frames):
            state["t"] = 0.1 * (k + 1)
            if which == "tracked":
                r, sr, _ = od.process_tracked(seg, trk, f, state["t"])
            else:
                r, sr = od.process_dynamic(seg, f, decide)
            frames.append((result_key(r), (sr.segments, sr.ground_pixels, sr.range_pixels, sr.rejected_pixels),
                           od.submap().tobytes()))
        runs.append((frames, [od.keyframe_points(k) for k in range(r.num_keyframes)]))
        od.close()
        seg.close()
        trk.close()
    (fa, ka), (fb, kb) = runs
    for k, (a, b) in enumerate(zip(fa, fb)):
        assert a == b, f"frame {k}: poses / statuses / keyframe decisions / segments / submaps differ"
    assert len(ka) == len(kb) >= 2
    for a, b in zip(ka, kb):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("mode", ["host", "device"])
def test_tracked_with_coasting_tracks(cfg5_frames, mode):
    """Coasting allowed: per frame the tracker's records equal track_ref.py fed with that frame's objects(),
    the removed pixels are the union of the restatement's non-static tracks' lists (stale ones included),
    and a keyframe added on the frame is the crop + voxel passes of that cloud."""
    kw = dict(TRACK_KW, max_no_hits=30)
    p = OD.default_odom_params()
    od = OD.Odometry(0, p)
    seg = S.Segmentation(0, cfg5_params(), labelling=mode)
    trk = T.Tracker(T.default_track_params(**kw))
    ref = TR.Tracker(TR.Params(**kw))
    lists = {}                                         # the restatement's per-track pixel lists
    prev, stale_frames, keyframes_checked = 0.0, 0, 0
    for k, f in enumerate(cfg5_frames):
        stamp = 0.1 * (k + 1)
        r, sr, tr = od.process_tracked(seg, trk, f, stamp)
        if r.status != OD.TRACKED:
            assert (tr.matches, tr.created, tr.erased) == (0, 0, 0) and len(trk.tracks()) == 0
            continue
        objs = seg.objects(10.0)
        track_of = ref.update(stamp - prev, TR.dets_from(objs))
        prev = stamp
        li = seg.label_indices()
        for o, t in zip(objs, track_of):
            lists[t] = li[int(o["id"])].copy()
        for t in ref.erased:
            lists.pop(t, None)
        recs = trk.tracks()
        assert [(int(x["id"]), int(x["status"]), int(x["hits"]), int(x["sslu"])) for x in recs] == \
            [(fl.id, fl.obj.status, fl.hits, fl.sslu) for fl in ref.filters], f"frame {k}"
        for x, fl in zip(recs, ref.filters):
            np.testing.assert_array_equal(x["state"], np.array(fl.kf.x), err_msg=f"frame {k}")
        assert (tr.matches, tr.created, tr.erased) == (len(ref.matches), len(ref.unmatched_dets), len(ref.erased))
        assert seg.tracks_stats()[0] == len(ref.filters)
        for fl in ref.filters:
            np.testing.assert_array_equal(seg.track_indices(fl.id), lists[fl.id])
        ns = ref.non_static_ids()
        assert tr.indices_dropped == sum(len(lists[t]) for t in ns)
        current = set(int(t) for t in track_of)
        stale_frames += any(t not in current for t in ns)
        # the removed pixel set: the scan as the handle holds it, without the union
        world = np.full((f.shape[0], 3), np.nan, np.float32)
        world[np.isfinite(f[:, :3]).all(axis=1)] = seg.static_cloud([])
        drop = np.concatenate([lists[t] for t in ns] + [[]]).astype(int)
        want = without(world, drop)
        np.testing.assert_array_equal(seg.static_cloud_tracks(ns), want)
        if r.keyframe_added:
            pose = np.array(r.T, np.float32).reshape(4, 4)[:3, 3]
            kf = PR.preprocess(want, p.crop_size if p.crop_use else 0.0, p.vf_scan_res if p.vf_scan_use else 0.0, pose)
            if p.vf_submap_use:
                kf = PR.preprocess(kf, 0.0, p.vf_submap_res)
            np.testing.assert_array_equal(od.keyframe_points(r.num_keyframes - 1), kf)
            keyframes_checked += 1
    assert stale_frames >= 1, "no frame removed a stale list: the sequence does not exercise coasting"
    assert keyframes_checked >= 1, "no keyframe was added on a tracked frame"
    od.close()
    seg.close()
    trk.close()


# Chosen on the restatement (track_ref.py over the objects of this sequence): the pedestrian near the sensor
# walks 0.14 m per frame and every object's average residuum is 0 on these frames, so the yaml's residuum
# ratio of 0.3 never lets a track through (0 < 0.3 * height); with the ratio 0 and the yaml's other values
# (maxUndefinedHits 1, minDistFromOrigin 0.75) its track is STATIC from its second detection and turns DYNAMIC
# about six frames later, with a full history of five boxes.  18 frames, a keyframe every 0.45 m (the sensor
# moves 0.1 m per frame): one keyframe while the track is STATIC, two after it turned DYNAMIC.
E2E_FRAMES = 18
E2E_TRACK = dict(residuum_height_ratio=0.0)
E2E_ODOM = dict(adaptive=0, keyframe_thresh_dist=0.45)


def test_tracked_end_to_end_with_map():
    import map_ref as MR
    from dynamic_direct_lidar_odometry_amd import mapping as M
    sc = scene.make_scene(1005, moving=True)
    poses = scene.trajectory(E2E_FRAMES, 1005)
    frames = [scene.raycast(sc, poses[k], 64, 2048, seed=1005 + k, t=0.1 * k, organized=True) for k in range(E2E_FRAMES)]
    p = OD.default_odom_params(**E2E_ODOM)
    od = OD.Odometry(0, p)
    seg = S.Segmentation(0, cfg5_params(), labelling="device")
    trk = T.Tracker(T.default_track_params(**E2E_TRACK))
    ref = TR.Tracker(TR.Params(**E2E_TRACK))
    mp = M.Map(0)
    lists, status_seen = {}, {}
    turned = set()                                     # tracks that went STATIC -> DYNAMIC
    prev, prev_len = 0.0, 0
    cleared_events, shrank, later_keyframes = 0, 0, 0
    first_seen = False
    for k, f in enumerate(frames):
        stamp = 0.1 * (k + 1)
        r, sr, tr = od.process_tracked(seg, trk, f, stamp, map=mp)
        if r.status != OD.TRACKED:
            if r.status == OD.FIRST:
                # keyframe 0 enters the map as every other keyframe does
                fresh = M.Map(0)
                fresh.add_odom_keyframe(od, 0)
                assert r.keyframe_added == 1 and len(mp) == len(fresh) > 0
                np.testing.assert_array_equal(mp.points(), fresh.points())
                fresh.close()
                first_seen = True
            else:
                assert len(mp) == 0
            prev_len = len(mp)
            continue
        objs = seg.objects(10.0)
        track_of = ref.update(stamp - prev, TR.dets_from(objs))
        prev = stamp
        li = seg.label_indices()
        for o, t in zip(objs, track_of):
            lists[t] = li[int(o["id"])].copy()
        for t in ref.erased:
            lists.pop(t, None)
        if r.keyframe_added and not ref.new_boxes:
            # the map gained exactly this keyframe
            fresh = M.Map(0)
            added = fresh.add_odom_keyframe(od, r.num_keyframes - 1)
            assert len(mp) == prev_len + added
            fresh.close()
        assert (tr.turned_dynamic, tr.boxes_cleared) == (ref.turned, len(ref.new_boxes)), f"frame {k}"
        for fl in ref.filters:
            was = status_seen.get(fl.id)
            if was == TR.STATIC and fl.obj.status == TR.DYNAMIC:
                turned.add(fl.id)
            assert not (was == TR.DYNAMIC and fl.obj.status != TR.DYNAMIC), "a DYNAMIC track reverted"
            status_seen[fl.id] = fl.obj.status
        assert sorted(int(x["id"]) for x in trk.tracks() if x["status"] == T.DYNAMIC) == \
            sorted(fl.id for fl in ref.filters if fl.obj.status == TR.DYNAMIC)
        if ref.new_boxes:
            cleared_events += 1
            boxes = np.array(ref.new_boxes, np.float64)   # x, y, z, sin(yaw / 2), dx, dy, dz
            pts = mp.points()
            if not r.keyframe_added:
                # the map after the clearing holds no point inside the boxes, and it lost points
                assert MR.keep_mask(pts, boxes).all(), f"frame {k}: a map point is inside a cleared box"
                shrank += len(mp) < prev_len
        if r.keyframe_added and turned:
            # a keyframe added after the turn holds no point of the turned tracks' lists
            world = np.full((f.shape[0], 3), np.nan, np.float32)
            world[np.isfinite(f[:, :3]).all(axis=1)] = seg.static_cloud([])
            ns = ref.non_static_ids()
            assert turned & set(lists) <= set(ns)
            drop = np.concatenate([lists[t] for t in ns] + [[]]).astype(int)
            want = without(world, drop)
            gone = np.concatenate([world[lists[t]] for t in turned if t in lists] + [np.zeros((0, 3), np.float32)])
            gone = gone[np.isfinite(gone).all(axis=1)]
            if len(gone):
                keys = set(map(bytes, want))
                assert not any(bytes(q) in keys for q in gone)
                pose = np.array(r.T, np.float32).reshape(4, 4)[:3, 3]
                kf = PR.preprocess(PR.preprocess(want, p.crop_size, p.vf_scan_res, pose), 0.0, p.vf_submap_res)
                np.testing.assert_array_equal(od.keyframe_points(r.num_keyframes - 1), kf)
                later_keyframes += 1
        prev_len = len(mp)
    assert first_seen, "no FIRST frame"
    assert turned, "no track went from STATIC to DYNAMIC"
    assert cleared_events >= 1 and shrank >= 1, (cleared_events, shrank)
    assert later_keyframes >= 1, "no keyframe was added after the track turned DYNAMIC"
    for h in (od, seg, trk, mp):
        h.close()
