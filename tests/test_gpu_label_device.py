"""The device labelling (csrc/seg_label.hip) against the literal
restatement oracle/segment_ref.py:label_components run on the same images,
through ``label_components_device`` and ``Segmentation(labelling="device")``:

* labels ``array_equal``, segment count equal;
* average residuals within (m + 1) 2^-24 of the oracle's value for a segment
  with m positive terms (the oracle's sequential float sum and float division
  against the device's double sum: derived in tests/label_ref.py, not measured);
* two runs bit-identical, averages included.

The inputs (random generator, hand-built cases, serpentine) are those of
tests/test_label_ref_cpu.py, which pins the formulation itself to the oracle.
"""
import math

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
import label_ref as LR
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import scene
from dynamic_direct_lidar_odometry_amd import segmentation as S
from oracle import segment_ref as R

pytestmark = pytest.mark.gpu


def seg_params(ns) -> S.SegParams:
    """The attribute bag of tests/label_ref.py as ddlo_seg_params (no ground rows: the labelling alone)."""
    return S.default_seg_params(ground_rows=0, **vars(ns))


def check_images(ns, rng, z, init, sensor_z, resid):
    """Device labelling of caller images against the oracle; returns the oracle's (label, segments)."""
    olab, oavg, on = R.label_components(ns, rng, z, init, sensor_z, resid)
    p = seg_params(ns)
    lab, avg, n = S.label_components_device(p, rng, z, init, sensor_z, resid)
    assert n == on
    assert np.array_equal(lab, olab)
    LR.assert_avg_within_bound(avg, oavg, LR.residual_terms(olab, resid, on))
    lab2, avg2, n2 = S.label_components_device(p, rng, z, init, sensor_z, resid)
    assert n2 == n and lab2.tobytes() == lab.tobytes() and avg2.tobytes() == avg.tobytes()
    # no residual image: every average is 0, the labels are the same
    lab3, avg3, n3 = S.label_components_device(p, rng, z, init, sensor_z, None)
    assert n3 == n and np.array_equal(lab3, lab) and not avg3.any()
    return olab, on


def test_random_images():
    with_segment = 0
    for seed in range(60):
        _, on = check_images(*LR.random_case(seed))
        with_segment += on > 0
    assert with_segment >= 54   # 90 % of the seeds: the test cannot pass on empty output


@pytest.mark.parametrize("name", sorted(LR.hand_cases()))
def test_hand_built_cases(name):
    ns, rng, z, init, sensor_z, resid, want = LR.hand_cases()[name]
    olab, on = check_images(ns, rng, z, init, sensor_z, resid)
    assert on == want["segments"]
    for (r, c), l in want.get("labels", {}).items():
        assert olab[r, c] == l, (r, c)


@pytest.mark.parametrize("cols", [130, 256, 300])
def test_serpentine_and_singletons(cols):
    """One long winding component across every 64-lane and 256-thread boundary of a row, next
    to about 200 singletons."""
    ns, rng, z, init, sensor_z, resid = LR.serpentine_case(cols)
    olab, on = check_images(ns, rng, z, init, sensor_z, resid)
    assert on == 1 and (olab == 1).sum() == 12 * cols + 11
    assert cols < 300 or (olab == 1).sum() >= 3000
    assert 190 <= (olab == R.REJECTED).sum() <= 215


# ---- whole frames through a handle ----------------------------------------------------------------
def avg_bound_ok(avg, ref, label, resid):
    LR.assert_avg_within_bound(avg, ref, LR.residual_terms(label, resid, len(ref) - 1))


def residual_image(rows, cols, seed):
    r = np.abs(np.random.default_rng(seed).normal(0, 0.2, (rows, cols))).astype(np.float32)
    r[np.random.default_rng(seed + 7).random((rows, cols)) < 0.3] = 0.0
    return r


@pytest.fixture(scope="module")
def cfg5_frames():
    """The first 12 organized 64 x 2048 frames of the moving-pedestrian sequence (sensor frame, NaN = no return)."""
    sc = scene.make_scene(1005, moving=True)
    poses = scene.trajectory(12, 1005)
    return [scene.raycast(sc, poses[k], 64, 2048, seed=1005 + k, t=0.1 * k, organized=True) for k in range(12)]


def organized_world_scan(frame: int, rows=512, cols=512):
    """tests/test_gpu_segment.py's frames."""
    sc = scene.make_scene(1005, moving=True)
    pose = scene.make_pose([0.3 * frame, -0.2 * frame, scene.SENSOR_Z], (0.0, 0.0, math.radians(7.0 * frame)))
    pts = scene.raycast(sc, pose, rows, cols, 1005 + frame, t=0.1 * frame, organized=True)
    bad = ~np.isfinite(pts).all(axis=1)
    xyz_t = scene.transform(np.nan_to_num(pts, nan=0.0), pose).astype(np.float32)
    xyz_t[bad] = np.nan
    return xyz_t, pose.astype(np.float32)


def cfg5_params():
    return S.yaml_seg_params(rows=64, cols=2048, ground_rows=20, win_row0=0, win_row1=63, win_col0=0, win_col1=2047,
                             max_distance=30)


def test_frame_64x2048_both_modes():
    xyz_t, T = organized_world_scan(1, 64, 2048)
    p = cfg5_params()
    resid = residual_image(64, 2048, 1)
    host = S.Segmentation(0, p)
    dev = S.Segmentation(0, p, labelling="device")
    assert host.labelling == "host" and dev.labelling == "device"
    rh = host.process(xyz_t, T, resid)
    rd = dev.process(xyz_t, T, resid)
    assert (rd.segments, rd.ground_pixels, rd.range_pixels, rd.rejected_pixels) == \
        (rh.segments, rh.ground_pixels, rh.range_pixels, rh.rejected_pixels)
    assert rd.segments == 17
    assert dev.labelling_stats()[1] == 18
    ih, idv = host.images(), dev.images()
    for a, b in zip(ih, idv):
        assert np.array_equal(a, b)
    label = idv[2]
    assert np.array_equal(dev.ground_indices(), host.ground_indices())
    lh, ld = host.label_indices(), dev.label_indices()
    assert len(lh) == len(ld) == rd.segments + 1
    for a, b in zip(lh[1:], ld[1:]):
        assert np.array_equal(a, b)
    avg = dev.avg_residuals()
    avg_bound_ok(avg, host.avg_residuals(), label, resid)
    objs = dev.objects(10.0)
    assert len(objs) >= 1
    assert objs.tobytes() == S.objects_from(xyz_t, label, avg, 10.0).tobytes()
    ids = [int(i) for i in objs["id"]]
    for remove in ([], ids[:1], ids):
        assert np.array_equal(dev.static_cloud(remove), host.static_cloud(remove))
        assert np.array_equal(dev.static_cloud(remove, T[:3, 3], 20.0, 0.1), host.static_cloud(remove, T[:3, 3], 20.0, 0.1))
    assert len(dev.static_cloud(ids)) < len(dev.static_cloud([]))
    # a second run on the handle: bit-identical, averages included
    rd2 = dev.process(xyz_t, T, resid)
    assert rd2.segments == rd.segments and rd2.rejected_pixels == rd.rejected_pixels
    assert dev.images()[2].tobytes() == label.tobytes() and dev.avg_residuals().tobytes() == avg.tobytes()
    # no residual image: zero averages
    dev.process(xyz_t, T)
    assert not dev.avg_residuals().any() and np.array_equal(dev.images()[2], label)
    host.close()
    dev.close()


WIDE = dict(win_row0=100, win_row1=500, win_col0=0, win_col1=511, max_distance=30)


@pytest.mark.parametrize("frame,kw,segments,prefix", [(0, {}, 2, 3), (3, WIDE, 12, 137)])
def test_frame_512x512(frame, kw, segments, prefix):
    """Frame 0 with the yaml parameters holds a thin vertical component whose push prefix is 118
    long -- the whole component; the order-free tests reject it before the replay, so the longest
    prefix replayed there is 3.  Frame 3 with the wide window replays a prefix of 137 pushes.
    (Figures from tests/label_ref.py on these images.)"""
    p = S.yaml_seg_params(**kw)
    xyz_t, T = organized_world_scan(frame)
    resid = residual_image(512, 512, frame)
    dev = S.Segmentation(0, p, labelling="device")
    res = dev.process(xyz_t, T, resid)
    rng, ground, label = dev.images()
    z = xyz_t[:, 2].reshape(p.rows, p.cols)
    init = np.where((ground == 1) | (rng == 0), -1, 0).astype(np.int32)
    olab, oavg, on = R.label_components(p, rng, z, init, float(T[2, 3]), resid)
    assert res.segments == on == segments
    assert np.array_equal(label, olab)
    avg = dev.avg_residuals()
    avg_bound_ok(avg, oavg, olab, resid)
    assert res.rejected_pixels == int((olab == R.REJECTED).sum())
    assert res.ground_pixels == int((ground == 1).sum()) and res.range_pixels == int((rng > 0).sum())
    assert dev.labelling_stats()[1] == prefix
    # the same images through the caller-image entry: the same labels and, bit for bit, the same averages
    lab, avg2, n = S.label_components_device(p, rng, z, init, float(T[2, 3]), resid)
    assert n == on and np.array_equal(lab, olab) and avg2.tobytes() == avg.tobytes()
    dev.close()


def test_mode_errors_and_round_trip():
    p = S.yaml_seg_params()
    seg = S.Segmentation(0, p)
    assert seg.labelling == "host"
    seg.labelling = "device"
    assert seg.labelling == "device"
    seg.labelling = "host"
    assert seg.labelling == "host"
    L = S._lib()
    assert L.ddlo_seg_set_labelling(seg.h, 2) == 1                      # GICP_EINVAL
    assert L.ddlo_seg_set_labelling(None, 1) == 1 and L.ddlo_seg_get_labelling(seg.h, None) == 1
    seg.close()
    for bad in (dict(win_col1=512), dict(win_col0=-1)):
        wide = S.Segmentation(0, S.yaml_seg_params(**bad))
        assert L.ddlo_seg_set_labelling(wide.h, S.LABELLING["device"]) == 1
        assert wide.labelling == "host"
        with pytest.raises(P.GicpError):
            wide.labelling = "device"
        assert wide.labelling == "host"
        wide.close()
    with pytest.raises(P.GicpError):
        S.Segmentation(0, S.yaml_seg_params(win_col1=512), labelling="device")
    ns, rng, z, init, sensor_z, resid = LR.random_case(0)
    ns.win_col1 = ns.cols
    with pytest.raises(P.GicpError):
        S.label_components_device(seg_params(ns), rng, z, init, sensor_z, resid)
    # a window cut by the rows is clamped, as the host labelling clamps it
    ns, rng, z, init, sensor_z, resid = LR.random_case(1)
    ns.win_row0, ns.win_row1 = -3, ns.rows + 5
    check_images(ns, rng, z, init, sensor_z, resid)
    fresh = S.Segmentation(0, p, labelling="device")
    with pytest.raises(P.GicpError):
        fresh.images()
    with pytest.raises(P.GicpError):
        fresh.labelling_stats()
    fresh.close()


# ---- the driver -----------------------------------------------------------------------------------
def result_key(r):
    def g(x):
        return (x.converged, x.nr_iterations, x.iterations_run, x.lm_failed, x.lm_trials, x.num_correspondences,
                x.final_cost, bytes(np.array(x.final_hessian)), x.lm_lambda)
    return (r.status, r.scan_points, bytes(r.T), bytes(r.T_s2s), bytes(r.T_s2s_local), g(r.s2s), g(r.s2m),
            r.keyframe_added, r.num_keyframes, r.spaciousness, r.keyframe_thresh_dist)


def test_driver_follows_the_mode(cfg5_frames):
    """ddlo_odom_process_dynamic (NULL callback: every object cut out of the keyframes) with a
    device-mode and a host-mode segmentation: the same poses, statuses, keyframes and submaps."""
    runs = {}
    for mode in ("host", "device"):
        od = OD.Odometry(0)
        seg = S.Segmentation(0, cfg5_params(), labelling=mode)
        frames = []
        for f in cfg5_frames:
            r, sr = od.process_dynamic(seg, f, None)
            frames.append((result_key(r), (sr.segments, sr.ground_pixels, sr.range_pixels, sr.rejected_pixels),
                           od.submap().tobytes()))
        label = seg.images()[2]
        kfs = [od.keyframe_points(k) for k in range(r.num_keyframes)]
        runs[mode] = (frames, label, kfs)
        od.close()
        seg.close()
    (fh, lh, kh), (fd, ld, kd) = runs["host"], runs["device"]
    for k, (a, b) in enumerate(zip(fh, fd)):
        assert a[0] == b[0], f"frame {k}: poses / statuses / keyframe decisions differ"
        assert a[1] == b[1], f"frame {k}: segment counts differ"
        assert a[2] == b[2], f"frame {k}: submaps differ"
    assert sum(a[1][0] for a in fh) >= 12, "the sequence has hardly any segment"
    assert np.array_equal(lh, ld)
    assert len(kh) == len(kd) >= 2
    for a, b in zip(kh, kd):
        assert np.array_equal(a, b)
