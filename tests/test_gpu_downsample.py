"""GPU tests of the organized-scan row/column filter (include/ddlo_downsample.h,
ddlo_odom_set_downsampling, ddlo_seg_set_downsampling, ddlo_preprocess_downsampled,
ddlo_debug_downsample_keep) against the numpy restatement tests/downsample_ref.py.

Exact everywhere except where a device voxel filter in its default (input) summation order meets the
oracle's pcl::VoxelGrid: equal counts and coordinates within 4e-6 x the extent there, the bound
tests/test_gpu_odom.py holds for the voxel filter.  Poses against the CPU chain: 1e-4, that file's bound
too (tests/parity.py itself holds the covariance bound only).
"""
import ctypes as C
import math

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import scene
from dynamic_direct_lidar_odometry_amd import segmentation as S
from dynamic_direct_lidar_odometry_amd import tracking as T
from oracle import oracle as O
import downsample_ref as D
import objects_ref as R
import preprocess_ref as PR
import track_ref as TR

pytestmark = pytest.mark.gpu

PCL, INPUT = OD.VOXEL_ORDER_PCL, OD.VOXEL_ORDER_INPUT
EINVAL = 1


# ---- 1. the rank kernels against numpy ------------------------------------------------------------
WG = 256                                  # pixels per workgroup of k_ds_count / k_ds_keep
SHAPES = [(1, 1), (3, 85), (16, 16), (1, 257), (1, 3 * 256 + 1), (7, 37)]


def step_sets(rows, cols):
    return [(1, 1), (2, 2), (1, 10), (3, 5), (rows, cols), (rows + 1, cols + 1)]


def flag_patterns(n, size_s):
    """name -> removed flags.  size_s: |S|, for the pattern that removes enough to make |S| > n'."""
    pat = {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8)}
    first = np.zeros(n, np.uint8)
    first[0] = 1
    last = np.zeros(n, np.uint8)
    last[n - 1] = 1
    alt = (np.arange(n) % 2).astype(np.uint8)
    pat.update(first=first, last=last, alternating=alt)
    run = np.zeros(n, np.uint8)                       # one run over two workgroup boundaries, where there are two
    run[min(WG - 3, n - 1):min(2 * WG + 5, n)] = 1
    pat["run"] = run
    many = np.zeros(n, np.uint8)                      # n' = |S| - 1 pixels left (scattered), if |S| > 1
    keep_left = max(size_s - 1, 0)
    many[np.random.default_rng(n).permutation(n)[keep_left:]] = 1
    pat["exceeds"] = many
    return pat


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_rank_kernel_against_numpy(rows, cols):
    n = rows * cols
    for rs, cs in step_sets(rows, cols):
        size_s = len(D.index_set(rows, cols, rs, cs))
        if (rs, cs) in ((rows, cols), (rows + 1, cols + 1)):
            assert size_s == 1
        for name, removed in flag_patterns(n, size_s).items():
            keep, skipped = OD.downsample_keep(removed, rows, cols, rs, cs)
            want, want_skipped = D.keyframe_keep(removed, rows, cols, rs, cs)
            np.testing.assert_array_equal(keep, want, err_msg=f"{rows}x{cols} steps {rs},{cs} {name}")
            assert skipped == want_skipped, (rows, cols, rs, cs, name)
            if name == "exceeds":
                assert skipped == 1
                np.testing.assert_array_equal(keep, 1 - removed)
            if name == "none":
                assert skipped == 0 and np.flatnonzero(keep).tolist() == D.index_set(rows, cols, rs, cs).tolist()
            if name == "all":
                assert not keep.any() and skipped == 1          # n' = 0 < |S|


def test_rank_kernel_many_workgroups():
    """A 64 x 256 image: 64 workgroups, random and banded removals, the shipped step pairs."""
    rows, cols = 64, 256
    rng = np.random.default_rng(5)
    for rs, cs in ((2, 2), (1, 10), (3, 5)):
        for frac in (0.02, 0.5):
            removed = (rng.random(rows * cols) < frac).astype(np.uint8)
            removed[5 * cols + 17:9 * cols + 3] = 1           # a band over several workgroups
            keep, skipped = OD.downsample_keep(removed, rows, cols, rs, cs)
            want, want_skipped = D.keyframe_keep(removed, rows, cols, rs, cs)
            np.testing.assert_array_equal(keep, want)
            assert skipped == want_skipped == 0


# ---- 2. the registration pass -----------------------------------------------------------------------
def raycast_scan(rows, cols, seed):
    """A ray-cast organized sensor-frame scan with no-return pixels: 10 % at random and one block."""
    sc = scene.make_scene(1005, moving=True)
    pose = scene.make_pose([0.3, -0.2, scene.SENSOR_Z], (0.0, 0.0, math.radians(7.0)))
    pts = scene.raycast(sc, pose, rows, cols, seed, t=0.1, organized=True).astype(np.float32)
    pts[np.random.default_rng(seed).random(rows * cols) < 0.1] = np.nan
    pts[cols + 3:cols + 3 + cols // 4] = np.nan
    return pts


@pytest.fixture(scope="module")
def small_scans():
    return {(8, 64): raycast_scan(8, 64, 11), (64, 256): raycast_scan(64, 256, 12)}


@pytest.mark.parametrize("steps", [(2, 2), (1, 10)])
@pytest.mark.parametrize("shape", [(8, 64), (64, 256)])
def test_preprocess_downsampled(small_scans, shape, steps):
    rows, cols = shape
    x = small_scans[shape]
    idx = D.index_set(rows, cols, *steps)
    extent = float(np.nanmax(np.abs(x)))
    for order in (INPUT, PCL):
        for crop in (0.0, 1.0):
            for leaf in (0.1, 0.0):
                got = OD.preprocess_downsampled(x, rows, cols, *steps, crop_size=crop, leaf=leaf, order=order)
                twin = OD.preprocess(x[idx], crop_size=crop, leaf=leaf, order=order)
                assert len(got) > 0
                np.testing.assert_array_equal(got.view(np.uint32), twin.view(np.uint32))
                if crop == 0.0 and leaf == 0.0:
                    assert len(got) == len(idx)          # no filter: the pixels of S as they are, NaN included
                    continue
                if order == INPUT:      # the kernels' own restatement: bit for bit; the oracle's: the voxel bound
                    ref = D.preprocess_downsampled(x, rows, cols, *steps, crop, leaf)
                    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
                kept = O.crop_box_negative(x[idx], crop) if crop > 0 else x[idx]
                oracle = O.voxel_grid(kept, leaf) if leaf > 0 else kept
                if order == PCL or leaf == 0.0:
                    np.testing.assert_array_equal(got, oracle)
                else:
                    assert got.shape == oracle.shape
                    np.testing.assert_allclose(got, oracle, rtol=0, atol=4e-6 * extent)


def test_preprocess_downsampled_indices_exceed_input():
    """S built for a larger image than the scan: |S| > n passes the scan on unfiltered; a scan shorter than
    the image but no shorter than |S| loses the pixels outside S, and the indices beyond it have no effect."""
    x = PR.uniform(600, 10.0, seed=8)
    got = OD.preprocess_downsampled(x, 64, 64, 2, 2, crop_size=1.0, leaf=0.0)          # |S| = 1024 > 600
    np.testing.assert_array_equal(got, OD.preprocess(x, crop_size=1.0, leaf=0.0))
    got = OD.preprocess_downsampled(x, 40, 30, 2, 3, crop_size=0.0, leaf=0.0)          # |S| = 200 <= 600 < 1200
    keep = D.extract_keep_organized(600, D.index_set(40, 30, 2, 3))
    assert 0 < keep.sum() < 200
    np.testing.assert_array_equal(got, x[keep])


# ---- 3 - 6: the driver at 256 x 256 --------------------------------------------------------------------
ROWS = COLS = 256


def organized_scan(frame):
    """tests/test_gpu_objects.py::organized_scan's poses and seeds (sensor frame), 2 % of the pixels without
    a return."""
    sc = scene.make_scene(1005, moving=True)
    pose = scene.make_pose([0.3 * frame, -0.2 * frame, scene.SENSOR_Z], (0.0, 0.0, math.radians(7.0 * frame)))
    pts = scene.raycast(sc, pose, ROWS, COLS, 1005 + frame, t=0.1 * frame, organized=True).astype(np.float32)
    pts[np.random.default_rng(frame).random(ROWS * COLS) < 0.02] = np.nan
    return pts


@pytest.fixture(scope="module")
def scans():
    return [organized_scan(f) for f in range(12)]


def seg_params():
    return S.yaml_seg_params(rows=ROWS, cols=COLS, ground_rows=75, win_row0=50, win_row1=250, win_col0=0, win_col1=255,
                             max_distance=30)


def odom_params():
    return OD.default_odom_params(skip_first_scan=0, adaptive=0, keyframe_thresh_dist=1.0)


def result_bytes(r):
    """Poses and gicp_results (not the device timings)."""
    def g(x):
        return (x.converged, x.nr_iterations, x.iterations_run, x.lm_failed, x.lm_trials, x.num_correspondences,
                x.final_cost, bytes(np.array(x.final_hessian)), x.lm_lambda)
    return (r.status, r.scan_points, bytes(r.T), bytes(r.T_s2s), bytes(r.T_s2s_local), g(r.s2s), g(r.s2m),
            r.keyframe_added, r.num_keyframes, r.spaciousness, r.keyframe_thresh_dist)


def keyframes_of(od, n):
    return [od.keyframe_points(k) for k in range(n)]


def test_plain_chain(scans):
    p = odom_params()
    idx = D.index_set(ROWS, COLS, 2, 2)
    on = OD.Odometry(0, p)
    on.set_downsampling(1, 2, 2, ROWS, COLS)
    assert on.downsampling() == (1, 2, 2, ROWS, COLS)
    twin = OD.Odometry(0, p)                                 # never configured, fed the pixels of S
    off = OD.Odometry(0, p)
    off.set_downsampling(0, 2, 2, ROWS, COLS)                # off, set explicitly
    assert off.downsampling() == (0, 2, 2, ROWS, COLS)
    untouched = OD.Odometry(0, p)
    assert untouched.downsampling()[0] == 0
    ref = D.OdomRefDownsampled(p, ROWS, COLS, 2, 2)
    added = 0
    for f, scan in enumerate(scans):
        a, b = on.process(scan), twin.process(scan[idx])
        assert result_bytes(a) == result_bytes(b), f
        c, d = off.process(scan), untouched.process(scan)
        assert result_bytes(c) == result_bytes(d), f
        o = ref.process(scan)
        assert a.status == o["status"] and a.scan_points == o["scan_points"], f
        assert a.keyframe_added == o["keyframe_added"], f
        added += a.keyframe_added
        if a.status != OD.TRACKED:
            continue
        for g in (a, b):
            Tg = g.pose()
            print(f"frame {f}: max |dt| {np.abs(Tg[:3, 3] - o['T'][:3, 3]).max():.2e} "
                  f"max |dR| {np.abs(Tg[:3, :3] - o['T'][:3, :3]).max():.2e}")
            np.testing.assert_allclose(Tg[:3, 3], o["T"][:3, 3], atol=1e-4, err_msg=f"frame {f}")
            np.testing.assert_allclose(Tg[:3, :3], o["T"][:3, :3], atol=1e-4, err_msg=f"frame {f}")
    assert added >= 2, "no keyframe beyond the first: extend the sequence"
    assert a.scan_points < c.scan_points
    for x, y in zip(keyframes_of(on, a.num_keyframes), keyframes_of(twin, a.num_keyframes)):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    for x, y in zip(keyframes_of(off, c.num_keyframes), keyframes_of(untouched, c.num_keyframes)):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    for h in (on, twin, off, untouched):
        h.close()


def residual_of(od, dp):
    """The residual image the driver's dynamic step took from its S2M context for the last scan."""
    ctx = C.c_void_p()
    assert od.L.ddlo_odom_ctx(od.h, 1, C.byref(ctx)) == 0
    img = np.zeros((ROWS, COLS), np.float32)
    assert P.load().gicp_residual_image(ctx, dp.theta_min, dp.theta_max, COLS, ROWS, img.ctypes.data_as(C.c_void_p),
                                        None) == 0
    return img


def world_of(seg, scan):
    """The world-frame scan as the handle holds it (T_ * scan, computed on the device), pixel by pixel."""
    setting = seg.downsampling()
    seg.set_downsampling(0, *setting[1:])
    world = np.full((scan.shape[0], 3), np.nan, np.float32)
    world[np.isfinite(scan[:, :3]).all(axis=1)] = seg.static_cloud([])
    seg.set_downsampling(*setting)
    return world


def keyframe_restatement(world, pose, removed, steps, p):
    cloud = D.static_cloud_downsampled(world, None, None, ROWS, COLS, *steps, centre=pose,
                                       crop_size=p.crop_size if p.crop_use else 0.0,
                                       leaf=p.vf_scan_res if p.vf_scan_use else 0.0, removed=removed)
    return O.voxel_grid(cloud, p.vf_submap_res) if p.vf_submap_use else cloud


# (1, 10) leaves 26 of these scans' 256 columns: too few for the registration to follow the sequence's 7 degree
# steps (the pose stays within millimetres of the origin, on the device and in the reference alike), so no
# keyframe would ever be due; a threshold below that jitter makes the first tracked frame add one.  The test is
# about what the keyframe is made of, not about where the pose is.
@pytest.mark.parametrize("order", [PCL, INPUT])
@pytest.mark.parametrize("steps,mode,thresh", [((2, 2), "host", 1.0), ((1, 10), "device", 1e-5)])
def test_dynamic_chain(scans, steps, mode, thresh, order):
    p = odom_params()
    p.keyframe_thresh_dist = thresh
    dp = OD.default_dynamic_params()
    od = OD.Odometry(0, p)
    seg = S.Segmentation(0, seg_params(), labelling=mode)
    plain = OD.Odometry(0, p)
    lone = S.Segmentation(0, seg_params(), labelling=mode)        # downsampling never set
    for h in (od, plain):
        h.set_downsampling(1, *steps, ROWS, COLS)
        h.set_voxel_order(order)
    seg.set_downsampling(1, *steps)
    seg.set_voxel_order(order)
    assert seg.downsampling() == (1, *steps)
    checked = False
    for f, scan in enumerate(scans):
        r, sr = od.process_dynamic(seg, scan, None)               # every object is cut out
        print(f"frame {f}: status {r.status} scan points {r.scan_points} keyframe added {r.keyframe_added} "
              f"t {np.array(r.T).reshape(4, 4)[:3, 3]} segments {sr.segments}")
        # the registration half is the plain driver's with the same setting
        assert result_bytes(r) == result_bytes(plain.process(scan)), f
        if r.status != OD.TRACKED:
            np.testing.assert_array_equal(od.keyframe_points(0), plain.keyframe_points(0))   # keyframe 0
            continue
        # the segmentation saw the whole scan: a handle without the setting, given the frame as the driver
        # built it (T_ * scan, the S2M context's residual image), finds the same segments and objects
        Tm = np.array(r.T, np.float32).reshape(4, 4)
        world = world_of(seg, scan)
        lr = lone.process(world, Tm, residual_of(od, dp))
        assert (lr.segments, lr.ground_pixels, lr.range_pixels, lr.rejected_pixels) == \
            (sr.segments, sr.ground_pixels, sr.range_pixels, sr.rejected_pixels), f
        objs = seg.objects(dp.max_dim_ratio)
        assert objs.tobytes() == lone.objects(dp.max_dim_ratio).tobytes(), f
        label = seg.images()[2]
        np.testing.assert_array_equal(label, lone.images()[2])
        if not r.keyframe_added:
            continue
        ids = [int(i) for i in objs["id"]]
        assert len(ids) >= 1, "the frame that adds the keyframe has no object"
        removed = np.isin(label.reshape(-1), ids)
        want = keyframe_restatement(world, Tm[:3, 3], removed, steps, p)
        got = od.keyframe_points(r.num_keyframes - 1)
        full = keyframe_restatement(world, Tm[:3, 3], removed, (1, 1), p)
        assert 0 < len(want) < len(full)
        # the pass ranks positions, not pixels: the pixels of S give another cloud once a pixel was removed
        by_pixel = D.nan_fill(world, D.extract_keep_organized(ROWS * COLS, D.index_set(ROWS, COLS, *steps)))
        pix = R.static_cloud(by_pixel, label, ids)
        pos = D.static_cloud_downsampled(world, label, ids, ROWS, COLS, *steps)
        assert pix.shape != pos.shape or (pix != pos).any()
        if order == PCL:
            np.testing.assert_array_equal(got, want)
        else:
            assert got.shape == want.shape
            np.testing.assert_allclose(got, want, rtol=0, atol=4e-6 * float(np.nanmax(np.abs(world))))
        assert not seg.downsampling_skipped
        checked = True
        break
    assert checked, "no keyframe within the frames given: extend the sequence"
    for h in (od, plain, seg, lone):
        h.close()


TRACK_KW = dict(min_dynamic_hits=3, max_undefined_hits=2, max_obj_velocity=15.0, min_dist_from_origin=0.3,
                residuum_height_ratio=0.0, max_no_hits=30)


def test_tracked_chain():
    """tests/test_gpu_track.py::test_tracked_with_coasting_tracks' sequence (64 x 2048, coasting tracks) with the
    filter on: a keyframe added on a tracked frame is the restatement over the union of the non-static tracks'
    lists, stale ones included; in input order the device filters equal their restatement bit for bit."""
    rows, cols, steps = 64, 2048, (2, 2)
    sc = scene.make_scene(1005, moving=True)
    poses = scene.trajectory(12, 1005)
    frames = [scene.raycast(sc, poses[k], rows, cols, seed=1005 + k, t=0.1 * k, organized=True) for k in range(12)]
    # a keyframe threshold below the sensor's step per frame: most tracked frames add a keyframe, so that some
    # keyframe is made of a scan that lost a stale list
    p = OD.default_odom_params(adaptive=0, keyframe_thresh_dist=0.1)
    od = OD.Odometry(0, p)
    od.set_downsampling(1, *steps, rows, cols)
    seg = S.Segmentation(0, S.yaml_seg_params(rows=rows, cols=cols, ground_rows=20, win_row0=0, win_row1=63, win_col0=0,
                                              win_col1=2047, max_distance=30))
    seg.set_downsampling(1, *steps)
    trk = T.Tracker(T.default_track_params(**TRACK_KW))
    ref = TR.Tracker(TR.Params(**TRACK_KW))
    lists, prev, stale_frames, stale_keyframes, keyframes_checked = {}, 0.0, 0, 0, 0
    for k, f in enumerate(frames):
        stamp = 0.1 * (k + 1)
        r, sr, tr = od.process_tracked(seg, trk, f, stamp)
        if r.status != OD.TRACKED:
            continue
        objs = seg.objects(10.0)
        track_of = ref.update(stamp - prev, TR.dets_from(objs))
        prev = stamp
        li = seg.label_indices()
        for o, t in zip(objs, track_of):
            lists[t] = li[int(o["id"])].copy()
        for t in ref.erased:
            lists.pop(t, None)
        ns = ref.non_static_ids()
        current = set(int(t) for t in track_of)
        stale = any(t not in current and len(lists[t]) for t in ns)
        stale_frames += stale
        removed = np.zeros(rows * cols, bool)
        removed[np.concatenate([lists[t] for t in ns] + [[]]).astype(int)] = True
        world = world_of(seg, f)
        keep, skipped = D.keyframe_keep(removed, rows, cols, *steps)
        filled = D.nan_fill(world, keep)
        # what a keyframe of this frame is made from: the handle's own entry, the union removed and the pass run
        np.testing.assert_array_equal(seg.static_cloud_tracks(ns), filled[np.isfinite(filled).all(axis=1)])
        assert skipped == 0 and not seg.downsampling_skipped
        if not r.keyframe_added:
            continue
        pose = np.array(r.T, np.float32).reshape(4, 4)[:3, 3]
        kf = PR.preprocess(filled, p.crop_size if p.crop_use else 0.0, p.vf_scan_res if p.vf_scan_use else 0.0, pose)
        if p.vf_submap_use:
            kf = PR.preprocess(kf, 0.0, p.vf_submap_res)
        np.testing.assert_array_equal(od.keyframe_points(r.num_keyframes - 1), kf)
        keyframes_checked += 1
        stale_keyframes += stale
    print(f"tracked frames with a stale list removed: {stale_frames}; keyframes checked: {keyframes_checked}, "
          f"of them with a stale list: {stale_keyframes}")
    assert stale_frames >= 1, "no frame removed a stale list: the sequence does not exercise coasting"
    assert keyframes_checked >= 1, "no keyframe was added on a tracked frame"
    assert stale_keyframes >= 1, "no keyframe was made of a scan that lost a stale list"
    for h in (od, seg, trk):
        h.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------
def test_refusals(scans):
    p = odom_params()
    od = OD.Odometry(0, p)
    twin = OD.Odometry(0, p)
    seg = S.Segmentation(0, seg_params())
    seg_twin = S.Segmentation(0, seg_params())
    for h in (od, twin):
        h.set_downsampling(1, 2, 2, ROWS, COLS)
    for h in (seg, seg_twin):
        h.set_downsampling(1, 2, 2)
    L = OD._lib()
    # steps, rows, cols < 1: nothing changes
    for bad in ((0, 2, ROWS, COLS), (2, 0, ROWS, COLS), (-1, 2, ROWS, COLS), (2, 2, 0, COLS), (2, 2, ROWS, 0)):
        assert L.ddlo_odom_set_downsampling(od.h, 1, *bad) == EINVAL
    assert L.ddlo_seg_set_downsampling(seg.h, 1, 0, 2) == EINVAL and L.ddlo_seg_set_downsampling(seg.h, 1, 2, -3) == EINVAL
    assert od.downsampling() == (1, 2, 2, ROWS, COLS) and seg.downsampling() == (1, 2, 2)
    other = S.Segmentation(0, S.yaml_seg_params(rows=128, cols=512, ground_rows=40, win_row0=20, win_row1=120, win_col0=0,
                                                win_col1=511, max_distance=30))
    other.set_downsampling(1, 2, 2)
    differs = S.Segmentation(0, seg_params())
    differs.set_downsampling(1, 1, 10)
    unset = S.Segmentation(0, seg_params())
    trk = T.Tracker(T.default_track_params())

    def refused(fn):
        with pytest.raises(P.GicpError) as e:
            fn()
        assert e.value.status == EINVAL

    def bad_calls(scan):
        refused(lambda: od.process(scan[:-1]))                                    # n != rows * cols
        refused(lambda: od.process(np.concatenate([scan, scan[:1]])))
        refused(lambda: od.process_dynamic_cloud(seg, scan, None))                # both _cloud entries
        refused(lambda: od.process_tracked_cloud(seg, trk, scan, 0.1))
        small = np.zeros((128 * 512, 3), np.float32)
        refused(lambda: od.process_dynamic(other, small, None))                   # a seg of other dimensions
        refused(lambda: od.process_dynamic(differs, scan, None))                  # a seg whose setting differs
        refused(lambda: od.process_dynamic(unset, scan, None))
        refused(lambda: od.process_tracked(differs, trk, scan, 0.1))

    for f, scan in enumerate(scans[:3]):
        bad_calls(scan)                                  # before the first scan, after FIRST, after a TRACKED frame
        a, b = od.process_dynamic(seg, scan, None), twin.process_dynamic(seg_twin, scan, None)
        assert result_bytes(a[0]) == result_bytes(b[0]), f
        assert (a[1].segments, a[1].range_pixels) == (b[1].segments, b[1].range_pixels), f
    assert a[0].status == OD.TRACKED
    # a driver without the setting refuses a segmentation that has it
    loose = OD.Odometry(0, p)
    refused(lambda: loose.process_dynamic(seg, scans[0], None))
    for h in (od, twin, seg, seg_twin, other, differs, unset, trk, loose):
        h.close()
