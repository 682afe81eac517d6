"""The odometry driver on unorganized clouds (ddlo_odom_process_tracked_cloud / _dynamic_cloud, ddlo_odom.h)
against its organized twins, on the 64 x 2048 moving-pedestrian frames and the parameters of
test_gpu_track.py.

An organized frame with NaN pixels and its finite points in row-major order must give the same run, bit for
bit: the registration half drops non-finite points and keeps the input order (crop, voxel filter, compaction:
csrc/preprocess.hip), every finite point projects onto the pixel it came from (test_project_ref_cpu.py), and
the fill writes the bits of the organized transform.  A difference is a bug in the new path, not a tolerance.

The segmentation parameters are test_gpu_track.py's (the yaml's ang_bottom of 90 degrees among them), so the
projection is passed explicitly: the ring model of the frames' sensor, 22.5 degrees.
"""
import numpy as np
import pytest

from dynamic_direct_lidar_odometry_amd import evaluation as EV
from dynamic_direct_lidar_odometry_amd import mapping as M
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import scene
from dynamic_direct_lidar_odometry_amd import segmentation as S
from dynamic_direct_lidar_odometry_amd import tracking as T
import project_ref as PJ

pytestmark = pytest.mark.gpu

ROWS, COLS = 64, 2048
TRACK_KW = dict(min_dynamic_hits=3, max_undefined_hits=2, max_obj_velocity=15.0, min_dist_from_origin=0.3,
                residuum_height_ratio=0.0, max_no_hits=30)
E2E_FRAMES = 18
E2E_TRACK = dict(residuum_height_ratio=0.0)
E2E_ODOM = dict(adaptive=0, keyframe_thresh_dist=0.45)


def cfg5_params():
    return S.yaml_seg_params(rows=ROWS, cols=COLS, ground_rows=20, win_row0=0, win_row1=ROWS - 1, win_col0=0,
                             win_col1=COLS - 1, max_distance=30)


def sensor_projection():
    return S.default_projection(cfg5_params().replace(ang_bottom=22.5))


def result_key(r):
    def g(x):
        return (x.converged, x.nr_iterations, x.iterations_run, x.lm_failed, x.lm_trials, x.num_correspondences,
                x.final_cost, bytes(np.array(x.final_hessian)), x.lm_lambda)
    return (r.status, r.scan_points, bytes(r.T), bytes(r.T_s2s), bytes(r.T_s2s_local), g(r.s2s), g(r.s2m),
            r.keyframe_added, r.num_keyframes, r.spaciousness, r.keyframe_thresh_dist)


def seg_key(sr):
    return (sr.segments, sr.ground_pixels, sr.range_pixels, sr.rejected_pixels)


def frames(n):
    sc = scene.make_scene(1005, moving=True)
    poses = scene.trajectory(n, 1005)
    return [scene.raycast(sc, poses[k], ROWS, COLS, seed=1005 + k, t=0.1 * k, organized=True) for k in range(n)]


@pytest.fixture(scope="module")
def blanked_frames():
    """the first 12 frames, each with 10 % of its pixels and one 8 x 300 block blanked (seeded per frame)"""
    return [PJ.blank(f, ROWS, COLS, (8, 300), 100 + k) for k, f in enumerate(frames(12))]


def run_tracked(frames_, mode, cloud):
    od = OD.Odometry(0)
    seg = S.Segmentation(0, cfg5_params(), labelling=mode)
    trk = T.Tracker(T.default_track_params(**TRACK_KW))
    proj = sensor_projection()
    out = []
    for k, f in enumerate(frames_):
        stamp = 0.1 * (k + 1)
        finite = np.isfinite(f).all(axis=1)
        if cloud:
            r, sr, tr, pr = od.process_tracked_cloud(seg, trk, np.ascontiguousarray(f[finite]), stamp, projection=proj)
            if r.status == OD.TRACKED:
                n = int(finite.sum())
                assert (pr.points, pr.invalid, pr.out_of_view, pr.occupied_pixels, pr.collisions) == (n, 0, 0, n, 0)
                np.testing.assert_array_equal(seg.projection_maps()[1], np.flatnonzero(finite))
            else:
                assert (pr.points, pr.occupied_pixels) == (0, 0)
        else:
            r, sr, tr = od.process_tracked(seg, trk, f, stamp)
        recs = trk.tracks()
        lists = [seg.track_indices(int(x["id"])).tobytes() for x in recs] if r.status == OD.TRACKED else []
        out.append((result_key(r), seg_key(sr), od.submap().tobytes(), (tr.matches, tr.created, tr.erased,
                                                                         tr.indices_dropped), recs.tobytes(), lists))
    kfs = [od.keyframe_points(k) for k in range(r.num_keyframes)]
    for h in (od, seg, trk):
        h.close()
    return out, kfs


@pytest.mark.parametrize("mode", ["host", "device"])
def test_tracked_cloud_equals_tracked(blanked_frames, mode):
    (fa, ka), (fb, kb) = run_tracked(blanked_frames, mode, False), run_tracked(blanked_frames, mode, True)
    names = ("OdomResult", "SegResult", "submap", "TrackResult", "track records", "track_indices")
    tracked = 0
    for k, (a, b) in enumerate(zip(fa, fb)):
        for name, u, v in zip(names, a, b):
            assert u == v, f"frame {k}: {name} differs"
        tracked += a[0][0] == OD.TRACKED and a[1][0] > 0 and len(a[5]) > 0
    assert tracked >= 6, "too few tracked frames with segments and tracks: the comparison is vacuous"
    assert len(ka) == len(kb) >= 2
    for a, b in zip(ka, kb):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("mode", ["host", "device"])
def test_dynamic_cloud_equals_dynamic(blanked_frames, mode):
    runs = []
    proj = sensor_projection()
    for cloud in (False, True):
        od = OD.Odometry(0)
        seg = S.Segmentation(0, cfg5_params(), labelling=mode)
        out = []
        for f in blanked_frames[:6]:
            if cloud:
                r, sr, pr = od.process_dynamic_cloud(seg, np.ascontiguousarray(f[np.isfinite(f).all(axis=1)]),
                                                     projection=proj)
            else:
                r, sr = od.process_dynamic(seg, f)
            objs = seg.objects(10.0).tobytes() if r.status == OD.TRACKED else b""
            out.append((result_key(r), seg_key(sr), od.submap().tobytes(), objs))
        runs.append((out, [od.keyframe_points(k) for k in range(r.num_keyframes)]))
        od.close()
        seg.close()
    (fa, ka), (fb, kb) = runs
    for k, (a, b) in enumerate(zip(fa, fb)):
        assert a == b, f"frame {k}"
    assert sum(a[0][0] == OD.TRACKED and a[1][0] > 0 for a in fa) >= 3
    assert len(ka) == len(kb) >= 1
    for a, b in zip(ka, kb):
        np.testing.assert_array_equal(a, b)


def test_tracked_cloud_end_to_end_with_map(tmp_path):
    """test_gpu_track.py's 18-frame end-to-end sequence with a map: the organized run and the run on the
    flattened frames give the same map; on every tracked frame the dynamic points are the preimage of the
    dynamic pixels (winners and losers alike), and they go through the evaluation files unchanged."""
    fr = frames(E2E_FRAMES)
    proj = sensor_projection()
    maps, dyn_frames, later_keyframes = [], 0, 0
    for cloud in (False, True):
        od = OD.Odometry(0, OD.default_odom_params(**E2E_ODOM))
        seg = S.Segmentation(0, cfg5_params(), labelling="device")
        trk = T.Tracker(T.default_track_params(**E2E_TRACK))
        mp = M.Map(0)
        written = {}
        ev = EV.Evaluation(tmp_path / "eval") if cloud else None
        for k, f in enumerate(fr):
            stamp = 0.1 * (k + 1)
            if not cloud:
                od.process_tracked(seg, trk, f, stamp, map=mp)
                continue
            finite = np.isfinite(f).all(axis=1)
            pts = np.ascontiguousarray(f[finite])
            r, sr, tr, pr = od.process_tracked_cloud(seg, trk, pts, stamp, map=mp, projection=proj)
            if r.status != OD.TRACKED:
                continue
            non_static = [x for x in trk.tracks() if x["status"] != T.STATIC]
            later_keyframes += bool(r.keyframe_added and non_static)
            od.classify(seg, trk)
            win, pix = seg.projection_maps()
            dyn_pix = seg.class_indices(S.CLS_DYNAMIC)
            dyn_pts = seg.point_class_indices(S.CLS_DYNAMIC)
            np.testing.assert_array_equal(dyn_pts, np.flatnonzero(np.isin(pix, dyn_pix)))
            winners = win.ravel()[dyn_pix]
            assert set(winners[winners >= 0].tolist()) <= set(dyn_pts.tolist())
            dyn_frames += len(dyn_pts) > 0
            ev.write(k, int(round(stamp * 1e9)), r.pose(), dyn_pts.astype(np.int32))
            written[k] = dyn_pts.astype(np.int32)
        if cloud:
            ev.close()
            idx, poses = EV.read_eval(tmp_path / "eval")
            assert sorted(idx) == sorted(written) and len(poses) == len(written)
            for k, v in written.items():
                np.testing.assert_array_equal(idx[k], v)
        maps.append(mp.points())
        for h in (od, seg, trk, mp):
            h.close()
    assert len(maps[0]) > 0
    np.testing.assert_array_equal(maps[0], maps[1])
    assert later_keyframes >= 1, "no keyframe was added on a tracked frame while a non-static track existed"
    assert dyn_frames >= 1, "no frame had a dynamic point"
