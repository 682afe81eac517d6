"""ddlo_odom_classify after ddlo_odom_process_tracked, and the evaluation files
written from it (include/ddlo_odom.h, ddlo_seg_classes.h, ddlo_eval.h).

The 18-frame moving-pedestrian recipe of tests/test_gpu_track.py::
test_tracked_end_to_end_with_map (constants copied): its pedestrian's track
goes STATIC -> DYNAMIC and other tracks coast.  Per TRACKED frame the index
sets and clouds must equal those built in numpy from tests/track_ref.py's
filters (fed with the frame's objects()) and the pixel lists recorded from
ddlo_seg_label_indices; the world-frame scan is read back through
ddlo_seg_static_cloud as that test reads it.  A second run that never
classifies must give the same poses, statuses, keyframes and track records.
"""
import numpy as np
import pytest

from dynamic_direct_lidar_odometry_amd import evaluation as E
from dynamic_direct_lidar_odometry_amd import mapping as M
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import scene
from dynamic_direct_lidar_odometry_amd import segmentation as S
from dynamic_direct_lidar_odometry_amd import tracking as T
import track_ref as TR

pytestmark = pytest.mark.gpu

E2E_FRAMES = 18
E2E_TRACK = dict(residuum_height_ratio=0.0)
E2E_ODOM = dict(adaptive=0, keyframe_thresh_dist=0.45)
BITS = [S.CLS_VALID, S.CLS_GROUND, S.CLS_UNDEFINED, S.CLS_STATIC, S.CLS_DYNAMIC]


def cfg5_params():
    return S.yaml_seg_params(rows=64, cols=2048, ground_rows=20, win_row0=0, win_row1=63, win_col0=0, win_col1=2047,
                             max_distance=30)


def result_key(r):
    def g(x):
        return (x.converged, x.nr_iterations, x.iterations_run, x.lm_failed, x.lm_trials, x.num_correspondences,
                x.final_cost, bytes(np.array(x.final_hessian)), x.lm_lambda)
    return (r.status, r.scan_points, bytes(r.T), bytes(r.T_s2s), bytes(r.T_s2s_local), g(r.s2s), g(r.s2m),
            r.keyframe_added, r.num_keyframes, r.spaciousness, r.keyframe_thresh_dist)


def six_digits(x):
    return np.array([float("%.6g" % float(v)) for v in np.asarray(x, np.float32).reshape(-1)])


def run(frames, classify, eval_dir=None):
    p = OD.default_odom_params(**E2E_ODOM)
    od = OD.Odometry(0, p)
    seg = S.Segmentation(0, cfg5_params(), labelling="device")
    trk = T.Tracker(T.default_track_params(**E2E_TRACK))
    mp = M.Map(0)
    ref = TR.Tracker(TR.Params(**E2E_TRACK))
    ev = E.Evaluation(eval_dir) if eval_dir is not None else None
    lists, prev = {}, 0.0
    record, written = [], {}
    dynamic_frames = coasting_frames = tracked = 0
    for k, f in enumerate(frames):
        stamp = 0.1 * (k + 1)
        r, sr, tr = od.process_tracked(seg, trk, f, stamp, map=mp)
        record.append((result_key(r), trk.tracks().tobytes()))
        if not classify or r.status != OD.TRACKED:
            continue
        tracked += 1
        objs = seg.objects(10.0)
        track_of = ref.update(stamp - prev, TR.dets_from(objs))
        prev = stamp
        li = seg.label_indices()
        for o, t in zip(objs, track_of):
            lists[t] = li[int(o["id"])].copy()
        for t in ref.erased:
            lists.pop(t, None)
        # the restatement: the world-frame scan as the handle holds it, the ground set, the filters' lists
        finite = np.isfinite(f[:, :3]).all(axis=1)
        world = np.full((f.shape[0], 3), np.nan, np.float32)
        world[finite] = seg.static_cloud([])
        want = np.zeros(f.shape[0], np.uint8)
        want[finite] |= S.CLS_VALID
        want[seg.ground_indices()] |= S.CLS_GROUND
        for fl in ref.filters:
            want[lists[fl.id]] |= S.CLS_UNDEFINED << fl.obj.status
        ns = (want & S.CLS_NON_STATIC) != 0
        counts = od.classify(seg, trk)
        np.testing.assert_array_equal(seg.class_image().reshape(-1), want, err_msg=f"frame {k}")
        got = [counts.valid, counts.ground, counts.undefined, counts.static_tracks, counts.dynamic, counts.non_static,
               counts.static_points]
        assert got == [int(((want & b) != 0).sum()) for b in BITS] + [int(ns.sum()), int((finite & ~ns).sum())]
        for any_bits in BITS + [S.CLS_NON_STATIC]:
            np.testing.assert_array_equal(seg.class_indices(any_bits), np.flatnonzero(want & any_bits),
                                          err_msg=f"frame {k}, set {any_bits}")
        dyn = seg.class_indices(S.CLS_DYNAMIC)
        valid = (want & S.CLS_VALID) != 0
        clouds = seg.frame_clouds()
        for got_c, mask in zip(clouds, ((want & S.CLS_GROUND) != 0, ns, (want & S.CLS_DYNAMIC) != 0, ~ns)):
            np.testing.assert_array_equal(got_c, world[valid & mask], err_msg=f"frame {k}")
        # the static cloud is what the keyframe is made of before its crop and voxel passes
        np.testing.assert_array_equal(clouds.static_points, seg.static_cloud_tracks(ref.non_static_ids()))
        dynamic_frames += dyn.size > 0
        coasting_frames += any(fl.sslu > 0 and len(lists[fl.id]) > 0 for fl in ref.filters)
        if ev is not None:
            ev.write(k, int(round(stamp * 1e9)), np.array(r.T, np.float32), dyn)
            written[k] = (int(round(stamp * 1e9)), np.array(r.T, np.float32), dyn)
    keyframes = [od.keyframe_points(j) for j in range(r.num_keyframes)]
    if ev is not None:
        ev.close()
    for h in (od, seg, trk, mp):
        h.close()
    return record, keyframes, written, (tracked, dynamic_frames, coasting_frames)


def test_classify_per_tracked_frame_and_eval_files(tmp_path):
    sc = scene.make_scene(1005, moving=True)
    poses = scene.trajectory(E2E_FRAMES, 1005)
    frames = [scene.raycast(sc, poses[k], 64, 2048, seed=1005 + k, t=0.1 * k, organized=True)
              for k in range(E2E_FRAMES)]
    rec_a, kf_a, written, (tracked, dynamic_frames, coasting_frames) = run(frames, True, tmp_path / "eval")
    assert tracked >= 10
    assert dynamic_frames >= 1, "the dynamic set was empty on every frame"
    assert coasting_frames >= 1, "no coasting track held pixels on any frame"
    # the files give the sets and the poses back
    idx, pose_recs = E.read_eval(tmp_path / "eval")
    assert sorted(idx) == sorted(written) and len(pose_recs) == len(written)
    for (stamp, Tm), k in zip(pose_recs, sorted(written)):
        np.testing.assert_array_equal(idx[k], written[k][2])
        assert stamp == written[k][0]
        np.testing.assert_array_equal(Tm.reshape(-1), six_digits(written[k][1]))
    assert any(v.size for v in idx.values())
    # classifying changes nothing the driver computes
    rec_b, kf_b, _, _ = run(frames, False)
    for k, (a, b) in enumerate(zip(rec_a, rec_b)):
        assert a == b, f"frame {k}: poses / statuses / keyframe decisions / track records differ"
    assert len(kf_a) == len(kf_b) >= 2
    for a, b in zip(kf_a, kf_b):
        np.testing.assert_array_equal(a, b)
