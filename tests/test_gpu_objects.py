"""GPU tests of the detected objects, the non-static point removal and the
driver's dynamic step (ddlo_seg_objects / ddlo_seg_objects_from /
ddlo_seg_static_cloud, ddlo_odom_process_dynamic / ddlo_odom_keyframe_points)
against the CPU restatements of tests/objects_ref.py.

Object bounds, per segment and per field, about float32(B) (B = getObject in
float64, A = in PCL's float32): max(4 |A - B|, 2 float32 ulps of the segment's
largest |coordinate|); id, num_points, avg_residuum, state[2] and state[6] are
exact.  Voxel-filtered clouds: equal counts, coordinates within 4e-6 x the
extent (the bound tests/test_gpu_odom.py holds for the voxel filter).
"""
import ctypes as C
import math

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import scene
from dynamic_direct_lidar_odometry_amd import segmentation as S
import objects_ref as R
import preprocess_ref as PR

pytestmark = pytest.mark.gpu

ROWS = COLS = 256


def check_objects(got, ref, xyz, label):
    """got: OBJECT_DTYPE array; ref: objects_ref.all_objects' list.  Returns the largest error / (2 ulp)."""
    assert [int(i) for i in got["id"]] == [r[0] for r in ref]
    lab = np.asarray(label).reshape(-1)
    worst = 0.0
    for g, (l, a, b, avg) in zip(got, ref):
        pts = xyz[lab == l][:, :3]
        assert g["num_points"] == b["num_points"] == len(pts)
        assert g["avg_residuum"] == avg
        want, tol, ulp = R.field_bounds(a, b, float(np.abs(pts).max()))
        have = np.concatenate([g["state"], g["axis"], [g["density"]]]).astype(np.float64)
        names = ["x", "y", "z", "sin", "dx", "dy", "dz", "ax0", "ax1", "density"]
        ratio = b["eig_ratio"]
        for k, name in enumerate(names):
            if name in ("z", "dz"):
                assert have[k] == want[k], (l, name)                      # float expressions: exact
                continue
            if name in ("sin", "ax0", "ax1") and math.isfinite(ratio) and ratio < 1.5:
                continue                                                  # ill-conditioned axes
            if not math.isfinite(want[k]):
                assert have[k] == want[k] or (math.isnan(have[k]) and math.isnan(want[k])), (l, name)
                continue
            err = abs(have[k] - want[k])
            print(f"segment {l} n {len(pts)} {name}: err {err:.3e} tol {tol[k]:.3e} ({err / (2 * ulp):.2f} x 2ulp)")
            assert err <= tol[k], (l, name, have[k], want[k], tol[k])
            worst = max(worst, err / (2 * ulp))
    return worst


# ---- 2. ddlo_seg_objects_from on a synthetic 16 x 256 image ------------------------------------
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 2800]


def synthetic_image():
    rng = np.random.default_rng(42)
    H, W = 16, 256
    n = H * W
    label = np.zeros(n, np.int32)
    xyz = rng.uniform(-120, 120, (n, 3)).astype(np.float32)
    filler = [-1, 0, R.REJECTED]
    pos, fill_k = 0, 0

    def fill(count):
        nonlocal pos, fill_k
        for _ in range(count):
            label[pos] = filler[fill_k % 3]
            if fill_k % 5 == 0:
                xyz[pos] = np.nan
            fill_k += 1
            pos += 1

    for sid, sz in enumerate(SIZES, start=1):
        fill(7)
        ang = rng.uniform(0, math.pi)
        centre = np.array([rng.choice([-1, 1]) * rng.uniform(80, 110), rng.choice([-1, 1]) * rng.uniform(60, 100), 20.0])
        uv = rng.uniform(-1, 1, (sz, 2)) * np.array([2.4, 0.6])          # eigenvalue ratio ~16
        if sz == 2:
            # along x: the box is exactly flat (a zero extent in any arithmetic), so its density is inf and
            # not the quotient of a rounding residue
            ang, uv = 0.0, np.array([[-1.0, 0.0], [1.0, 0.0]])
        c, s = math.cos(ang), math.sin(ang)
        pts = np.column_stack([centre[0] + c * uv[:, 0] - s * uv[:, 1], centre[1] + s * uv[:, 0] + c * uv[:, 1],
                               centre[2] + rng.uniform(0, 1.7, sz)]).astype(np.float32)
        for k in range(sz):
            if sz == 65:          # this segment's pixels are not contiguous in the image
                fill(1)
            label[pos] = sid
            xyz[pos] = pts[k]
            pos += 1
    # a pole: two zero dimensions, one non-zero -> ratio inf, dropped
    fill(5)
    pole = len(SIZES) + 1
    for k in range(3):
        label[pos] = pole
        xyz[pos] = np.array([-90.0, 75.0, 10.0 + k], np.float32)
        pos += 1
    fill(n - pos)
    avg = np.linspace(0.0, 0.9, pole + 1) ** 2
    return xyz, label.reshape(H, W), avg, pole


def test_objects_from_synthetic_image():
    xyz, label, avg, pole = synthetic_image()
    got = S.objects_from(xyz, label, avg, 10.0)
    ref = R.all_objects(xyz, label, 10.0, avg)
    ids = [r[0] for r in ref]
    assert 1 in ids, "the one-point segment's NaN ratio passes the test"
    assert pole not in ids and pole not in got["id"], "x / 0 = inf is dropped"
    assert ids == list(range(1, len(SIZES) + 1))
    for l, a, b, _ in ref:
        if b["num_points"] > 2:
            assert b["eig_ratio"] >= 1.5, (l, b["eig_ratio"])
    worst = check_objects(got, ref, xyz, label)
    print(f"largest error: {worst:.2f} x (2 float32 ulps of the segment's largest coordinate)")
    one = got[0]
    assert one["axis"].tolist() == [1.0, 0.0] and one["state"][4:].tolist() == [0.0, 0.0, 0.0]
    assert math.isinf(one["density"])
    again = S.objects_from(xyz, label, avg, 10.0)
    assert got.tobytes() == again.tobytes()
    # strided layout (pcl::PointXYZI) and no residuals
    rec = np.zeros((xyz.shape[0], 8), np.float32)
    rec[:, :3] = xyz
    third = S.objects_from(rec, label, None, 10.0)
    assert not third["avg_residuum"].any()
    third["avg_residuum"] = got["avg_residuum"]
    assert third.tobytes() == got.tobytes()
    # a tiny ratio drops everything but the one-point segment, whose NaN ratio compares false
    assert S.objects_from(xyz, label, avg, 1e-3)["id"].tolist() == [1]


# ---- 3 - 5: ray-cast scans at 256 x 256 ----------------------------------------------------------
def organized_scan(frame):
    """tests/test_gpu_segment.py::organized_world_scan's pose and seed formula; also the sensor-frame scan."""
    sc = scene.make_scene(1005, moving=True)
    pose = scene.make_pose([0.3 * frame, -0.2 * frame, scene.SENSOR_Z], (0.0, 0.0, math.radians(7.0 * frame)))
    pts = scene.raycast(sc, pose, ROWS, COLS, 1005 + frame, t=0.1 * frame, organized=True)
    bad = ~np.isfinite(pts).all(axis=1)
    xyz_t = scene.transform(np.nan_to_num(pts, nan=0.0), pose).astype(np.float32)
    xyz_t[bad] = np.nan
    return pts.astype(np.float32), xyz_t, pose.astype(np.float32)


@pytest.fixture(scope="module")
def scans():
    return [organized_scan(f) for f in range(4)]


def seg_params():
    return S.yaml_seg_params(rows=ROWS, cols=COLS, ground_rows=75, win_row0=50, win_row1=250, win_col0=0, win_col1=255,
                             max_distance=30)


def residual_for(frame):
    r = np.abs(np.random.default_rng(frame).normal(0, 0.2, (ROWS, COLS))).astype(np.float32)
    r[np.random.default_rng(frame + 7).random((ROWS, COLS)) < 0.3] = 0.0
    return r


EXPECTED_SEGMENTS = [4, 7, 5, 5]


@pytest.mark.parametrize("frame", [0, 1, 2, 3])
def test_objects_after_process(scans, frame):
    _, xyz_t, T = scans[frame]
    seg = S.Segmentation(0, seg_params())
    res = seg.process(xyz_t, T, residual_for(frame))
    assert res.segments == EXPECTED_SEGMENTS[frame]
    _, _, label = seg.images()
    avg = seg.avg_residuals()
    got = seg.objects(10.0)
    ref = R.all_objects(xyz_t, label, 10.0, avg)
    every = R.all_objects(xyz_t, label, float("inf"), avg)
    assert len(every) == res.segments
    for l, a, b, _ in every:
        assert b["eig_ratio"] >= 1.5
    check_objects(got, ref, xyz_t, label)
    assert got.tobytes() == seg.objects(10.0).tobytes()
    # a ratio midway between two adjacent reference ratios drops exactly what the reference drops
    ratios = sorted(R.dim_ratio(b["state"]) for _, _, b, _ in every)
    assert len(ratios) >= 2
    mid = 0.5 * (ratios[len(ratios) // 2 - 1] + ratios[len(ratios) // 2])
    assert ratios[len(ratios) // 2 - 1] < mid < ratios[len(ratios) // 2]
    cut = seg.objects(mid)
    want = R.all_objects(xyz_t, label, mid, avg)
    assert 0 < len(want) < len(every)
    check_objects(cut, want, xyz_t, label)
    seg.close()


def voxel_close(got, ref, extent):
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=0, atol=4e-6 * extent)


def test_static_cloud(scans):
    _, xyz_t, T = scans[1]
    seg = S.Segmentation(0, seg_params())
    res = seg.process(xyz_t, T, residual_for(1))
    _, _, label = seg.images()
    ids = list(range(1, res.segments + 1))
    centre = T[:3, 3]
    extent = float(np.nanmax(np.abs(xyz_t)))
    flat = label.reshape(-1)
    for remove in ([], [ids[len(ids) // 2]], ids):
        got = seg.static_cloud(remove, centre, crop_size=1.0, leaf=0.0)
        ref = R.static_cloud(xyz_t, label, remove, centre, 1.0, 0.0)
        np.testing.assert_array_equal(got, ref)
        plain = seg.static_cloud(remove)
        np.testing.assert_array_equal(plain, R.static_cloud(xyz_t, label, remove))
        # no returned point lies on a removed segment's pixels
        gone = xyz_t[np.isin(flat, remove)]
        if len(gone):
            keys = set(map(bytes, plain))
            assert not any(bytes(p) in keys for p in gone)
            assert len(plain) == np.isfinite(xyz_t).all(axis=1).sum() - len(gone)
        vg = seg.static_cloud(remove, centre, crop_size=1.0, leaf=0.1)
        voxel_close(vg, R.static_cloud(xyz_t, label, remove, centre, 1.0, 0.1), extent)
        # the translated crop box folded into the voxel pass: bit-identical to the kernels' plain restatement
        want = PR.preprocess(R.static_cloud(xyz_t, label, remove), 1.0, 0.1, centre)
        assert vg.shape == want.shape and len(want) < len(plain)
        np.testing.assert_array_equal(vg.view(np.uint32), want.view(np.uint32))
        assert len(PR.crop_keep(plain, 1.0, centre)) != len(PR.crop_keep(plain, 1.0))   # a box at the origin would show
        voxel_close(seg.static_cloud(remove, leaf=0.1), R.static_cloud(xyz_t, label, remove, leaf=0.1), extent)
    assert len(seg.static_cloud(ids)) < len(seg.static_cloud([]))
    # errors: unknown ids, capacity too small
    L = S._lib()
    n = C.c_size_t()
    c = np.zeros(3, np.float32)
    for bad in (0, res.segments + 1, -1, R.REJECTED):
        b = np.array([bad], np.int32)
        assert L.ddlo_seg_static_cloud(seg.h, P._ptr(b), 1, P._ptr(c), 0.0, 0.0, None, 0, C.byref(n)) == 1
    small = np.zeros((10, 3), np.float32)
    assert L.ddlo_seg_static_cloud(seg.h, None, 0, P._ptr(c), 0.0, 0.0, P._ptr(small), 10, C.byref(n)) == 1
    assert n.value == np.isfinite(xyz_t).all(axis=1).sum()
    fresh = S.Segmentation(0, seg_params())
    with pytest.raises(P.GicpError):
        fresh.objects()
    with pytest.raises(P.GicpError):
        fresh.static_cloud([])
    seg.close()
    fresh.close()


# ---- 5. the driver ---------------------------------------------------------------------------------
def odom_params():
    return OD.default_odom_params(skip_first_scan=0, adaptive=0, keyframe_thresh_dist=1.0)


def result_bytes(r):
    """Poses and gicp_results (not the device timings)."""
    def g(x):
        return (x.converged, x.nr_iterations, x.iterations_run, x.lm_failed, x.lm_trials, x.num_correspondences,
                x.final_cost, bytes(np.array(x.final_hessian)), x.lm_lambda)
    return (r.status, r.scan_points, bytes(r.T), bytes(r.T_s2s), bytes(r.T_s2s_local), g(r.s2s), g(r.s2m),
            r.keyframe_added, r.num_keyframes, r.spaciousness, r.keyframe_thresh_dist)


def keyframe_restatement(sensor_scan, T, label, remove, p):
    world = R.transform_f32(sensor_scan, T)
    pose = np.asarray(T, np.float32).reshape(4, 4)[:3, 3]
    cloud = R.static_cloud(world, label, remove, pose, p.crop_size if p.crop_use else 0.0,
                           p.vf_scan_res if p.vf_scan_use else 0.0)
    if p.vf_submap_use:
        from oracle import oracle as O
        cloud = O.voxel_grid(cloud, p.vf_submap_res)
    return world, cloud


def run_dynamic(scans, decide, frames):
    p = odom_params()
    od = OD.Odometry(0, p)
    seg = S.Segmentation(0, seg_params())
    out = []
    for f in frames:
        r, sr = od.process_dynamic(seg, scans[f][0], decide)
        rec = {"res": r, "seg": sr, "label": None, "objects": None}
        if r.status == OD.TRACKED:
            rec["label"] = seg.images()[2]
            rec["objects"] = seg.objects(10.0)
        out.append(rec)
        if r.status == OD.TRACKED and r.keyframe_added:
            break
    return od, seg, out, p


def test_driver_dynamic_step(scans):
    frames = list(range(4))
    seen = []

    def nothing(objs):
        seen.append(objs.copy())
        return [False] * len(objs)

    od_b, seg_b, run_b, p = run_dynamic(scans, nothing, frames)
    od_c, seg_c, run_c, _ = run_dynamic(scans, None, frames)
    last = len(run_b) - 1
    assert run_b[last]["res"].status == OD.TRACKED and run_b[last]["res"].keyframe_added == 1, \
        "no keyframe within the frames given: extend the sequence"
    assert len(run_c) == len(run_b)
    # (a) the registration half is ddlo_odom_process, bit for bit, up to the first added keyframe
    plain = OD.Odometry(0, p)
    for f in range(last + 1):
        r = plain.process(scans[f][0])
        assert result_bytes(r) == result_bytes(run_b[f]["res"]) == result_bytes(run_c[f]["res"]), f
    assert run_b[0]["res"].status == OD.FIRST and run_b[0]["seg"].segments == 0 and run_b[0]["seg"].range_pixels == 0
    np.testing.assert_array_equal(od_b.keyframe_points(0), plain.keyframe_points(0))     # the first keyframe
    np.testing.assert_array_equal(od_c.keyframe_points(0), plain.keyframe_points(0))
    # (e) the callback saw exactly ddlo_seg_objects' array, once per tracked frame
    tracked = [x for x in run_b if x["res"].status == OD.TRACKED]
    assert len(seen) == len(tracked)
    for s, x in zip(seen, tracked):
        assert s.tobytes() == x["objects"].tobytes()
    # (b) nothing marked: crop + scan voxel + submap voxel of the world-frame scan
    k = run_b[last]["res"].num_keyframes - 1
    T = np.array(run_b[last]["res"].T, np.float32).reshape(4, 4)
    world, ref_b = keyframe_restatement(scans[last][0], T, run_b[last]["label"], [], p)
    extent = float(np.nanmax(np.abs(world)))
    kf_b = od_b.keyframe_points(k)
    voxel_close(kf_b, ref_b, extent)
    assert od_b.keyframe(k)[1] == len(kf_b)
    # (c) NULL callback: every object of that frame removed
    ids = [int(i) for i in run_c[last]["objects"]["id"]]
    assert len(ids) >= 1, "the frame that adds the keyframe has no object"
    assert np.array_equal(run_c[last]["label"], run_b[last]["label"])
    _, ref_c = keyframe_restatement(scans[last][0], T, run_c[last]["label"], ids, p)
    kf_c = od_c.keyframe_points(k)
    voxel_close(kf_c, ref_c, extent)
    # (d) strictly fewer points
    assert len(kf_c) < len(kf_b)
    # (f) an aborting callback surfaces as an error status
    od_f = OD.Odometry(0, p)
    seg_f = S.Segmentation(0, seg_params())
    r0, _ = od_f.process_dynamic(seg_f, scans[0][0], lambda objs: None)     # FIRST: the callback does not run
    assert r0.status == OD.FIRST
    with pytest.raises(P.GicpError) as e:
        od_f.process_dynamic(seg_f, scans[1][0], lambda objs: None)
    assert e.value.status == 7      # GICP_ESTATE

    def broken(objs):
        raise KeyError("tracker")

    od_g = OD.Odometry(0, p)
    od_g.process_dynamic(seg_f, scans[0][0], broken)
    with pytest.raises(KeyError):
        od_g.process_dynamic(seg_f, scans[1][0], broken)
    for h in (od_b, od_c, od_f, od_g, plain, seg_b, seg_c, seg_f):
        h.close()
