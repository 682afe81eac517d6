"""Bit-exact GPU tests of the opt-in intensity channel (include/ddlo_intensity.h) against its numpy
restatement (tests/intensity_ref.py, checked by tests/test_intensity_ref_cpu.py).

Every comparison is on bits: array_equal on the uint32 view, or intensity_ref.same_bits where a NaN or
Inf intensity went through a sum (NaN then equals NaN whatever its payload).  Two assertions per filter
case: equality with the restatement, and the self-check that needs none: with intensity := x bit for bit,
every output has intensity == x bit for bit, which holds only if the channel is summed over the same
points, in the same order, with the same division.
"""
import ctypes as C
import math

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import mapping as M
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import scene

import intensity_ref as IR
import map_ref as MR
import objects_ref as R
import preprocess_ref as PR

pytestmark = pytest.mark.gpu

INPUT, PCL = IR.ORDER_INPUT, IR.ORDER_PCL
LAYOUTS = ((16, 12), (20, 16), (32, 16))          # (stride, offset): packed x y z i, 20 B records, pcl::PointXYZI
EINVAL = 1


def bits_equal(got, ref, what=""):
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=what)


def gpu_preprocess(p, crop, leaf, order=INPUT, layout=(16, 12)):
    return OD.preprocess(IR.records(p, *layout), crop, leaf, order=order, intensity_offset=layout[1])


def check(xyz, crop, leaf, order, what, layouts=((16, 12),)):
    """Both assertions for one cloud and one configuration."""
    p = IR.with_intensity(xyz)
    ref = IR.preprocess(p, crop, leaf, order=order)
    for layout in layouts:
        bits_equal(gpu_preprocess(p, crop, leaf, order, layout), ref, f"{what} crop {crop} leaf {leaf} order {order} {layout}")
    px = IR.with_intensity(xyz, "x")
    got = gpu_preprocess(px, crop, leaf, order)
    bits_equal(got[:, :3], ref[:, :3], f"{what}: x, y, z do not depend on the intensity")
    bits_equal(got[:, 3], got[:, 0], f"{what} crop {crop} leaf {leaf} order {order}: intensity := x")
    return ref


# crop only, voxel only, both folded into one pass
CONFIGS = ((1.0, 0.0), (0.0, 0.1), (1.0, 0.1), (0.0, 0.3))


# ---- the filter kernels, through ddlo_preprocess_xyzi ---------------------------------------------------
@pytest.mark.parametrize("order", [INPUT, PCL])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_small_sizes(n, order):
    xyz = PR.uniform(257, half=2.0, seed=60)[:n]
    for crop, leaf in CONFIGS + ((0.0, 0.0),):
        ref = check(xyz, crop, leaf, order, f"n {n}", LAYOUTS)
        assert len(ref) <= n
    if n == 257:
        assert 0 < len(IR.preprocess(IR.with_intensity(xyz), 1.0, 0.3)) < n


@pytest.mark.parametrize("order", [INPUT, PCL])
@pytest.mark.parametrize("name", ["single_voxel", "lattice", "sites", "negative", "uniform"])
def test_edge_clouds(name, order):
    xyz = getattr(PR, name)()
    crops = (1.0, 0.5) if name == "lattice" else (1.0,)
    for crop in crops:
        check(xyz, crop, 0.0, order, name)
        check(xyz, crop, 0.1, order, name)
    for leaf in (0.1, 0.3):
        ref = check(xyz, 0.0, leaf, order, name, LAYOUTS if name == "sites" else ((16, 12),))
    if name == "single_voxel":
        assert len(ref) == 1                       # one run of 700 points
    if name == "uniform":
        assert len(xyz) == 20000 and len(ref) < len(xyz)


@pytest.mark.parametrize("order", [INPUT, PCL])
def test_voxel_index_overflow_passes_the_input_through(order):
    xyz = PR.wide(PR.OVERFLOW_HALF_Z)
    p = IR.with_intensity(xyz)
    assert IR.voxel_grid(p, 0.05) is None
    bits_equal(gpu_preprocess(p, 0.0, 0.05, order), p, "overflow: the cloud as it is")
    ref = check(xyz, 1.0, 0.05, order, "overflow with a crop box")
    assert len(ref) == int(PR.crop_mask(xyz, 1.0).sum())
    assert len(check(xyz, 0.0, 0.1, order, "wide, no overflow")) < len(xyz)


@pytest.mark.parametrize("pattern", ["first", "last", "one", "all_but_one", "all", "every7th"])
def test_nonfinite_xyz(pattern):
    base = PR.uniform(3000, half=4.0, seed=61)
    xyz = PR.with_nonfinite(base, PR.nonfinite_patterns(len(base))[pattern])
    for order in (INPUT, PCL):
        for crop, leaf in CONFIGS + ((0.0, 0.0),):
            p = IR.with_intensity(xyz)
            ref = IR.preprocess(p, crop, leaf, order=order)
            got = gpu_preprocess(p, crop, leaf, order)
            if crop == 0 and leaf == 0:            # nothing ran: the NaN points are handed on, intensity kept
                bits_equal(got, p)
                continue
            bits_equal(got, ref, f"{pattern} crop {crop} leaf {leaf} order {order}")
            assert np.isfinite(got).all()
            if pattern == "all":
                assert len(got) == 0


@pytest.mark.parametrize("order", [INPUT, PCL])
def test_nonfinite_intensity_only(order):
    base = IR.with_intensity(PR.uniform(4000, half=5.0, seed=51))
    bad = IR.nonfinite_intensity(base)
    for crop, leaf in CONFIGS + ((0.0, 0.0),):
        clean, got = gpu_preprocess(base, crop, leaf, order), gpu_preprocess(bad, crop, leaf, order)
        bits_equal(got[:, :3], clean[:, :3], "a NaN / Inf intensity changes no count and no x, y, z")
        ref = IR.preprocess(bad, crop, leaf, order=order)
        assert IR.same_bits(got, ref), (crop, leaf)
        if leaf == 0:
            bits_equal(got, ref)                   # handed on bit for bit
        else:
            fin = np.isfinite(ref[:, 3])
            assert fin.any() and (~fin).any()
            bits_equal(got[fin], ref[fin])
            np.testing.assert_array_equal(np.isposinf(got[:, 3]), np.isposinf(ref[:, 3]))
            np.testing.assert_array_equal(np.isneginf(got[:, 3]), np.isneginf(ref[:, 3]))


def test_exact_sums_agree_across_orders():
    p = IR.with_intensity(PR.sites(), "bytes")
    a, b = gpu_preprocess(p, 0.0, 0.25, INPUT), gpu_preprocess(p, 0.0, 0.25, PCL)
    bits_equal(a[:, 3], b[:, 3], "integer intensities: every partial sum is exact, the order cannot show")
    assert (a[:, :3].view(np.uint32) != b[:, :3].view(np.uint32)).any()      # while x, y, z do show it


def test_invalid_arguments():
    L = OD._lib()
    rec = np.zeros((4, 8), np.float32)
    out = np.zeros((4, 4), np.float32)
    n = C.c_size_t()

    def call(stride, off, order=0, cap=4):
        return L.ddlo_preprocess_xyzi(0, P._ptr(rec), 4, stride, off, 0.0, 0.0, order, P._ptr(out), cap, C.byref(n))

    for stride, off in LAYOUTS + ((32, 28), (32, 12)):
        assert call(stride, off) == 0 and n.value == 4
    for stride, off in ((16, 8), (16, 0), (16, 13), (16, 14), (16, 16), (20, 20), (32, 29), (32, 32), (12, 12), (32, 1 << 40)):
        assert call(stride, off) == EINVAL, (stride, off)
    assert call(16, 12, order=2) == EINVAL
    assert call(16, 12, cap=3) == EINVAL and n.value == 4
    od = OD.Odometry(0, OD.default_odom_params(skip_first_scan=0))
    assert od.intensity == (False, 0)
    od.set_intensity(True, 16)
    assert od.intensity == (True, 16)
    r = OD.OdomResult()
    pts = IR.records(IR.with_intensity(PR.uniform(2000, seed=62)), 16, 12)
    assert L.ddlo_odom_process(od.h, P._ptr(pts), len(pts), 16, C.byref(r)) == EINVAL      # 16 + 4 > 16
    with pytest.raises(P.GicpError):
        od.keyframe_points(0, intensity=True)                                               # no keyframe yet
    od.set_intensity(True, 12)
    assert L.ddlo_odom_process(od.h, P._ptr(pts), len(pts), 16, C.byref(r)) == 0 and r.num_keyframes == 1
    with pytest.raises(P.GicpError) as e:
        od.set_intensity(False)                                                             # a keyframe exists
    assert e.value.status == EINVAL and od.intensity == (True, 12)
    od.close()
    off = OD.Odometry(0, OD.default_odom_params(skip_first_scan=0))
    off.process(pts[:, :3])
    with pytest.raises(P.GicpError) as e:
        off.keyframe_points(0, intensity=True)                                              # carries none
    assert e.value.status == EINVAL
    with pytest.raises(P.GicpError):
        off.set_intensity(True, 12)
    off.close()


# ---- the plain driver -----------------------------------------------------------------------------------
ROWS, COLS, FRAMES = 32, 512, 4


@pytest.fixture(scope="module")
def frames():
    """4 ray-cast frames, 0.1 m apart, with a seeded intensity column."""
    fr, _ = scene.odometry_sequence(ROWS, COLS, FRAMES, cfg_id=7)
    return [IR.with_intensity(f, seed=70 + k) for k, f in enumerate(fr)]


def odom_params(**kw):
    # every tracked frame is 0.1 m from the last keyframe: each becomes one
    return OD.default_odom_params(skip_first_scan=0, adaptive=0, keyframe_thresh_dist=0.05, **kw)


def result_bytes(r):
    """Poses and gicp_results (not the device timings)."""
    def g(x):
        return (x.converged, x.nr_iterations, x.iterations_run, x.lm_failed, x.lm_trials, x.num_correspondences,
                x.final_cost, bytes(np.array(x.final_hessian)), x.lm_lambda)
    return (r.status, r.scan_points, bytes(r.T), bytes(r.T_s2s), bytes(r.T_s2s_local), g(r.s2s), g(r.s2m),
            r.keyframe_added, r.num_keyframes, r.submap_changed, r.submap_keyframes, r.submap_points, r.spaciousness,
            r.keyframe_thresh_dist)


def run_plain(frames, p, order, intensity, layout=(16, 12)):
    """[(OdomResult, submap)] per frame, the keyframe clouds (x y z, and x y z i when on)."""
    od = OD.Odometry(0, p)
    od.set_voxel_order(order)
    if intensity:
        od.set_intensity(True, layout[1])
    out = []
    for f in frames:
        r = od.process(IR.records(f, *layout) if intensity else f[:, :3])
        out.append((r, od.submap().copy()))
    nk = out[-1][0].num_keyframes
    xyz = [od.keyframe_points(k) for k in range(nk)]
    xyzi = [od.keyframe_points(k, intensity=True) for k in range(nk)] if intensity else None
    poses = [od.keyframe(k)[0] for k in range(nk)]
    od.close()
    return out, xyz, xyzi, poses


@pytest.mark.parametrize("order", [INPUT, PCL])
def test_driver_plain(frames, order):
    p = odom_params()
    off, kf_off, _, poses_off = run_plain(frames, p, order, False)
    on, kf_on, kfi, poses_on = run_plain(frames, p, order, True, (32, 16))
    assert len(kf_off) == len(kf_on) >= 2, "fewer than 2 keyframes: lower the threshold"
    for f, ((a, sa), (b, sb)) in enumerate(zip(off, on)):
        assert result_bytes(a) == result_bytes(b), f
        np.testing.assert_array_equal(sa, sb)
    for a, b, c, pa, pb in zip(kf_off, kf_on, kfi, poses_off, poses_on):
        bits_equal(a, b, "keyframe_points with intensity off and on")
        bits_equal(c[:, :3], a, "keyframe_points(k, intensity=True)[:, :3]")
        assert pa.tobytes() == pb.tobytes()
    # the reference chain: the scan's preprocessing, unchanged through the transform, the submap voxel filter
    # over the keyframe's own pre-filter points (rebuilt from the pose the frame reported)
    k = 0
    for f, (r, _) in enumerate(on):
        if not r.keyframe_added:
            continue
        scan = IR.preprocess(frames[f], p.crop_size, p.vf_scan_res, order=order)
        assert len(scan) == r.scan_points
        world = scan.copy()
        world[:, :3] = R.transform_f32(scan[:, :3], np.array(r.T, np.float32).reshape(4, 4))
        want = IR.voxel_grid(world, p.vf_submap_res, order=order)[0]
        bits_equal(kfi[k], want, f"keyframe {k} (frame {f})")
        k += 1
    assert k == len(kfi)


def test_driver_plain_filters_off(frames):
    p = odom_params(vf_scan_use=0, vf_submap_use=0)
    on, _, kfi, _ = run_plain(frames[:2], p, INPUT, True, (20, 16))
    off, kf_off, _, _ = run_plain(frames[:2], p, INPUT, False)
    assert len(kfi) == 2
    for (a, _), (b, _) in zip(off, on):
        assert result_bytes(a) == result_bytes(b)
    for k, f in enumerate(frames[:2]):
        keep = PR.crop_mask(f[:, :3], p.crop_size)
        assert keep.sum() > 0
        bits_equal(kfi[k][:, 3], f[keep, 3], "the crop survivors' intensities in input order")
        bits_equal(kfi[k][:, :3], kf_off[k])


# ---- the map ----------------------------------------------------------------------------------------------
INITIAL_CAPACITY = 16384          # ddlo_map.h: the room a new map starts with


@pytest.fixture(scope="module")
def keyframes():
    """Three world-frame keyframes (x y z i), 7k - 8k points each."""
    sc = scene.make_scene(1005)
    frame = scene.raycast(sc, scene.make_pose([-6.0, 2.0, scene.SENSOR_Z]), 32, 256, seed=1005)
    poses = [scene.make_pose([-6.0, 2.0, scene.SENSOR_Z], (0.0, 0.0, math.radians(15.0))),
             scene.make_pose([-4.5, 2.5, scene.SENSOR_Z], (0.0, 0.0, math.radians(40.0))),
             scene.make_pose([-3.0, 1.0, scene.SENSOR_Z], (0.0, 0.0, math.radians(-20.0)))]
    return [IR.with_intensity(scene.transform(frame, T), seed=80 + k) for k, T in enumerate(poses)]


def new_map(intensity=True, **kw):
    m = M.Map(0, M.default_map_params(**kw))
    if intensity:
        m.set_intensity(True)
        assert m.intensity
    return m


@pytest.mark.parametrize("filtered", [True, False])
def test_map_add_keyframe_xyzi(keyframes, filtered):
    leaf = 0.25
    m = new_map(voxel_filter_use=int(filtered), leaf_size=leaf)
    mx = new_map(voxel_filter_use=int(filtered), leaf_size=leaf)          # intensity := x
    want = []
    for k, (kf, layout) in enumerate(zip(keyframes, LAYOUTS)):
        dirty = kf.copy()
        dirty[k::50, k % 3] = np.nan                                        # dropped, filter on or off
        dirty[5::40, 3] = np.inf                                            # kept
        ref = IR.map_add(dirty, leaf if filtered else 0.0)
        assert m.add_keyframe(IR.records(dirty, *layout), intensity_offset=layout[1]) == len(ref)
        want.append(ref)
        asx = dirty.copy()
        asx[:, 3] = asx[:, 0]
        assert mx.add_keyframe(asx, intensity_offset=12) == len(ref)
    want = np.concatenate(want)
    got = m.points(intensity=True)
    assert IR.same_bits(got, want) and np.isinf(got[:, 3]).any()
    bits_equal(got[:, :3], want[:, :3])
    bits_equal(m.points(), want[:, :3], "ddlo_map_points of a map with intensity")
    gx = mx.points(intensity=True)
    bits_equal(gx[:, :3], want[:, :3])
    bits_equal(gx[:, 3], gx[:, 0], "intensity := x through the map's filter")
    # an x y z keyframe on a map with intensity: intensity 0
    n0 = len(m)
    assert m.add_keyframe(keyframes[0][:100, :3]) > 0
    assert not m.points(intensity=True)[n0:, 3].any()
    m.close()
    mx.close()


def test_map_setting_and_refusals(keyframes):
    m = M.Map(0)
    assert not m.intensity
    with pytest.raises(P.GicpError) as e:
        m.points(intensity=True)
    assert e.value.status == EINVAL
    with pytest.raises(P.GicpError) as e:
        m.add_keyframe(keyframes[0], intensity_offset=12)
    assert e.value.status == EINVAL and len(m) == 0
    m.add_keyframe(keyframes[0][:, :3])
    with pytest.raises(P.GicpError) as e:
        m.set_intensity(True)                                               # not empty
    assert e.value.status == EINVAL
    m.set_intensity(False)                                                  # nothing changes: accepted
    m.close()
    m = new_map()
    L, added = M._lib(), C.c_size_t()
    rec = np.zeros((4, 8), np.float32)
    for stride, off in ((16, 8), (16, 13), (16, 16), (32, 30), (12, 12)):
        assert L.ddlo_map_add_keyframe_xyzi(m.h, P._ptr(rec), 4, stride, off, C.byref(added)) == EINVAL
    assert len(m) == 0
    m.close()


def test_map_growth_keeps_the_channel(keyframes):
    m = new_map(voxel_filter_use=0)
    want, total = [], 0
    while total <= 2 * INITIAL_CAPACITY:
        kf = keyframes[len(want) % 3]
        assert m.add_keyframe(kf, intensity_offset=12) == len(kf)
        want.append(kf)
        total += len(kf)
        assert len(want) <= 12
    assert len(want) >= 3 and len(m) == total
    bits_equal(m.points(intensity=True), np.concatenate(want))
    m.close()


def test_map_clear_boxes(keyframes):
    rng = np.random.default_rng(90)
    allp = np.concatenate(keyframes)
    flat = np.column_stack([rng.uniform(-12, 6, (12, 2)), rng.uniform(0, 3, 12), np.zeros(12), rng.uniform(1, 6, (12, 3))])
    yaw = rng.uniform(-math.pi, math.pi, 12)
    turned = flat.copy()
    turned[:, 3] = np.sin(yaw / 2)
    for boxes, exact in ((flat, True), (turned, False), (np.concatenate([flat, turned]), False)):
        mi, mx = new_map(voxel_filter_use=0, filter_margin=0.1), new_map(False, voxel_filter_use=0, filter_margin=0.1)
        for kf in keyframes:
            mi.add_keyframe(kf, intensity_offset=12)
            mx.add_keyframe(kf[:, :3])
        removed = mi.clear_boxes(boxes)
        assert removed == mx.clear_boxes(boxes) and 0 < removed < len(allp)
        left = mi.points(intensity=True)
        bits_equal(left[:, :3], mx.points(), "the same points leave an x y z map")
        # order and intensity: the survivors are a subsequence of what went in, found by their x, y, z bits
        key = {bytes(r[:3]): i for i, r in enumerate(allp)}
        idx = np.array([key[bytes(r[:3])] for r in left])
        assert (np.diff(idx) > 0).all()
        bits_equal(left, allp[idx])
        if exact:
            bits_equal(left, allp[MR.keep_mask(allp[:, :3], boxes, 0.1)], "unrotated boxes: map_ref's mask")
        mi.close()
        mx.close()


def parse_pcd(path):
    raw = open(path, "rb").read()
    end = raw.index(b"DATA binary\n") + len(b"DATA binary\n")
    lines = raw[:end].decode().splitlines()
    fields = {l.split()[0]: l.split()[1:] for l in lines if l and not l.startswith("#")}
    return fields, raw[end:]


def test_map_export(keyframes, tmp_path):
    m = new_map(leaf_size=0.25)
    for kf in keyframes:
        m.add_keyframe(kf, intensity_offset=12)
    full = m.points(intensity=True)
    got = m.points(0.5, intensity=True)
    ref = IR.voxel_grid(full, 0.5)[0]
    assert 0 < len(ref) < len(full)
    bits_equal(got, ref, "points_xyzi(leaf > 0)")
    bits_equal(m.points(intensity=True), full, "the map itself is unchanged")
    n = C.c_size_t()
    small = np.zeros((10, 4), np.float32)
    assert M._lib().ddlo_map_points_xyzi(m.h, 0.0, P._ptr(small), 10, C.byref(n)) == EINVAL and n.value == len(full)
    # save_pcd: four fields, the payload is points_xyzi
    for leaf in (0.0, 0.5):
        path = tmp_path / f"map_{leaf}.pcd"
        m.save_pcd(path, leaf)
        want = m.points(leaf, intensity=True)
        fields, payload = parse_pcd(path)
        cnt = str(len(want))
        assert fields == {"VERSION": ["0.7"], "FIELDS": ["x", "y", "z", "intensity"], "SIZE": ["4"] * 4,
                          "TYPE": ["F"] * 4, "COUNT": ["1"] * 4, "WIDTH": [cnt], "HEIGHT": ["1"],
                          "VIEWPOINT": ["0", "0", "0", "1", "0", "0", "0"], "POINTS": [cnt], "DATA": ["binary"]}
        assert payload == want.tobytes()
    # a map without intensity writes the file it always wrote
    plain = new_map(False, leaf_size=0.25)
    for kf in keyframes:
        plain.add_keyframe(kf[:, :3])
    plain.save_pcd(tmp_path / "plain.pcd", 0.5)
    fields, payload = parse_pcd(tmp_path / "plain.pcd")
    want = plain.points(0.5)
    assert fields["FIELDS"] == ["x", "y", "z"] and fields["SIZE"] == ["4"] * 3 and fields["COUNT"] == ["1"] * 3
    assert payload == want.tobytes() == got[:, :3].tobytes()
    m.close()
    plain.close()
    # index overflow: the map as it is
    two = np.array([[0.0, 0.0, 0.0, 7.5], [6000.0, 8000.0, 0.0, np.nan]], np.float32)
    far = new_map(voxel_filter_use=0)
    assert far.add_keyframe(two, intensity_offset=12) == 2
    bits_equal(far.points(1e-3, intensity=True), two)
    far.close()


def drive_and_map(frames, order=INPUT):
    """The driver-plus-map sequence: every keyframe goes into a device-to-device map and a host-path map."""
    od = OD.Odometry(0, odom_params())
    od.set_voxel_order(order)
    od.set_intensity(True, 12)
    dev, host = new_map(), new_map()
    out = []
    for f in frames:
        r = od.process(f)
        if r.keyframe_added:
            k = r.num_keyframes - 1
            kp = od.keyframe_points(k, intensity=True)
            assert dev.add_odom_keyframe(od, k) == host.add_keyframe(kp, intensity_offset=12) > 0
            out.append(kp.tobytes())
    boxes = [[3.0, 0.0, -1.5, math.sin(0.3), 4.0, 3.0, 3.0]]        # ground in front of the first pose (the origin)
    assert dev.clear_boxes(boxes) == host.clear_boxes(boxes) > 0
    res = (out, dev.points(intensity=True), host.points(intensity=True), dev.points(0.5, intensity=True))
    # refusals: a map with intensity and a driver without
    bare = OD.Odometry(0, odom_params())
    bare.process(frames[0][:, :3])
    n = len(dev)
    with pytest.raises(P.GicpError) as e:
        dev.add_odom_keyframe(bare, 0)
    assert e.value.status == EINVAL and len(dev) == n
    xyz_map = new_map(False)
    assert xyz_map.add_odom_keyframe(od, 0) > 0          # an x y z map takes a keyframe with the channel, without it
    bits_equal(xyz_map.points(), IR.map_add(np.frombuffer(out[0], np.float32).reshape(-1, 4), 0.25)[:, :3])
    for h in (od, bare, dev, host, xyz_map):
        h.close()
    return res


def test_add_odom_keyframe_and_determinism(frames):
    kfs, dev, host, vox = drive_and_map(frames)
    assert len(kfs) >= 2
    bits_equal(dev, host, "add_odom_keyframe equals keyframe_points_xyzi then add_keyframe_xyzi")
    assert len(vox) < len(dev)
    again = drive_and_map(frames)
    assert again[0] == kfs
    for a, b in zip(again[1:], (dev, host, vox)):
        assert a.tobytes() == b.tobytes()


# ---- the segmentation's static cloud and the dynamic driver ------------------------------------------------
from dynamic_direct_lidar_odometry_amd import segmentation as S   # noqa: E402

SROWS = SCOLS = 256


def organized_scan(frame):
    """tests/test_gpu_objects.py::organized_scan's poses and seeds (sensor frame), 2 % of the pixels without a
    return; also the pose."""
    sc = scene.make_scene(1005, moving=True)
    pose = scene.make_pose([0.3 * frame, -0.2 * frame, scene.SENSOR_Z], (0.0, 0.0, math.radians(7.0 * frame)))
    pts = scene.raycast(sc, pose, SROWS, SCOLS, 1005 + frame, t=0.1 * frame, organized=True).astype(np.float32)
    pts[np.random.default_rng(frame).random(SROWS * SCOLS) < 0.02] = np.nan
    return pts, pose.astype(np.float32)


@pytest.fixture(scope="module")
def scans():
    return [organized_scan(f) for f in range(2)]


def seg_params():
    return S.yaml_seg_params(rows=SROWS, cols=SCOLS, ground_rows=75, win_row0=50, win_row1=250, win_col0=0, win_col1=255,
                             max_distance=30)


def removed_to_nan(world, label, ids):
    out = world.copy()
    out[np.isin(label.reshape(-1), ids), :3] = np.nan
    return out


@pytest.mark.parametrize("mode", ["host", "device"])
def test_seg_static_cloud_xyzi(scans, mode):
    """ddlo_seg_process on pcl::PointXYZI records, then the static cloud with its channel."""
    sensor, T = scans[1]
    world = R.transform_f32(sensor, T)
    p = IR.with_intensity(world, seed=100)
    p[::9, 3] = 0.0                                        # kept and removed pixels of intensity 0 ...
    p[4::9, 3] = 1.0                                       # ... and of the marker's value
    seg = S.Segmentation(0, seg_params(), labelling=mode)
    seg.set_intensity(True, 16)
    assert seg.intensity == (True, 16)
    res = seg.process(IR.records(p, 32, 16), T, None)
    assert res.segments >= 2
    label = seg.images()[2]
    centre = T[:3, 3]
    ids = [1, res.segments]
    for remove in ([], ids):
        gone = removed_to_nan(p, label, remove)
        for order in (INPUT, PCL):
            seg.set_voxel_order(order)
            for crop, leaf in ((0.0, 0.0), (1.0, 0.0), (1.0, 0.1), (0.0, 0.3)):
                got = seg.static_cloud(remove, centre, crop, leaf, intensity=True)
                if crop == 0 and leaf == 0:
                    want = gone[IR.pass_mask(gone)]
                else:
                    want = IR.preprocess(gone, crop, leaf, centre, order)
                bits_equal(got, want, f"{mode} remove {remove} order {order} crop {crop} leaf {leaf}")
                bits_equal(seg.static_cloud(remove, centre, crop, leaf), want[:, :3])
    assert len(seg.static_cloud(ids)) < len(seg.static_cloud([]))
    # the row/column filter's keyframe pass: the same pixels leave as on a handle without the channel
    bare = S.Segmentation(0, seg_params(), labelling=mode)
    bare.process(world, T, None)
    for h in (seg, bare):
        h.set_downsampling(1, 2, 2)
        h.set_voxel_order(INPUT)
    for remove in ([], ids):
        got = seg.static_cloud(remove, centre, 1.0, 0.0, intensity=True)
        xyz = bare.static_cloud(remove, centre, 1.0, 0.0)
        bits_equal(got[:, :3], xyz, f"{mode} downsampled, remove {remove}")
        assert 0 < len(xyz) < len(world) // 3
        key = {bytes(r[:3]): i for i, r in enumerate(p) if np.isfinite(r[:3]).all()}
        idx = np.array([key[bytes(r[:3])] for r in got])
        assert (np.diff(idx) > 0).all()
        bits_equal(got[:, 3], p[idx, 3], "the survivors keep their intensities")
        assert (got[:, 3] == 0).any() and (got[:, 3] == 1).any()
    # refusals
    n = C.c_size_t()
    c = np.zeros(3, np.float32)
    assert S._lib().ddlo_seg_static_cloud_xyzi(bare.h, None, 0, P._ptr(c), 0.0, 0.0, None, 0, C.byref(n)) == EINVAL
    seg.set_intensity(True, 16)
    with pytest.raises(P.GicpError) as e:
        seg.process(p, T, None)                             # 16 + 4 > the 16 B stride
    assert e.value.status == EINVAL
    seg.close()
    bare.close()


def run_dynamic(scans, p, intensity, ds, mode="host"):
    """Two frames through ddlo_odom_process_dynamic, the first object of frame 1 declared non-static.
    intensity: None (off) or a function pixel count -> column.  Returns (results, keyframe 1, label, id, T)."""
    od = OD.Odometry(0, p)
    seg = S.Segmentation(0, seg_params(), labelling=mode)
    if ds:
        od.set_downsampling(1, 2, 2, SROWS, SCOLS)
        seg.set_downsampling(1, 2, 2)
    if intensity is not None:
        od.set_intensity(True, 12)
        seg.set_intensity(True, 12)
    seen = []

    def first_only(objs):
        seen.append(objs.copy())
        return [i == 0 for i in range(len(objs))]

    out = []
    for sensor, _ in scans:
        a = sensor if intensity is None else np.column_stack([sensor, intensity(len(sensor))]).astype(np.float32)
        r, sr = od.process_dynamic(seg, a, first_only)
        out.append(result_bytes(r))
    assert r.status == OD.TRACKED and r.keyframe_added == 1 and r.num_keyframes == 2, "frame 1 adds no keyframe"
    assert len(seen) == 1 and len(seen[0]) >= 1, "frame 1 has no object"
    kf = od.keyframe_points(1, intensity=intensity is not None)
    kf0 = od.keyframe_points(0, intensity=intensity is not None)
    label = seg.images()[2]
    skipped = seg.downsampling_skipped
    od.close()
    seg.close()
    return out, kf0, kf, label, int(seen[0]["id"][0]), np.array(r.T, np.float32).reshape(4, 4), skipped


@pytest.mark.parametrize("ds", [False, True])
def test_driver_dynamic(scans, ds):
    p = odom_params(vf_scan_use=0, vf_submap_use=0)         # no voxel filter: a keyframe point is a pixel
    off = run_dynamic(scans, p, None, ds)
    index = run_dynamic(scans, p, lambda n: np.arange(n, dtype=np.float32), ds)
    marker = run_dynamic(scans, p, lambda n: np.ones(n, np.float32), ds)        # every pixel has the old marker's value
    zero = run_dynamic(scans, p, lambda n: np.zeros(n, np.float32), ds)         # every kept pixel has intensity 0
    for run, value in ((index, None), (marker, 1.0), (zero, 0.0)):
        assert run[0] == off[0], "OdomResults with intensity off and on"
        bits_equal(run[1][:, :3], off[1], "keyframe 0")
        bits_equal(run[2][:, :3], off[2], "the keyframe loses exactly the pixels it loses today")
        np.testing.assert_array_equal(run[3], off[3])
        assert run[4] == off[4] and run[6] == off[6] is False
        if value is not None:
            assert (run[2][:, 3] == value).all() and (run[1][:, 3] == value).all()
    # the survivors keep their intensities: the intensity names the pixel
    _, kf0, kf, label, rid, T, _ = index
    sensor = scans[1][0]
    pix = kf[:, 3].astype(np.int64)
    assert (kf[:, 3] == pix).all() and (np.diff(pix) > 0).all()
    bits_equal(kf[:, :3], R.transform_f32(sensor, T)[pix], "each keyframe point is its pixel's, moved by the pose")
    removed = label.reshape(-1) == rid
    assert removed.sum() > 0 and not removed[pix].any()
    world = R.transform_f32(sensor, T)
    stays = PR.crop_mask(world, p.crop_size, T[:3, 3]) & ~removed
    if not ds:
        np.testing.assert_array_equal(pix, np.flatnonzero(stays))
    else:
        assert 0 < len(pix) < stays.sum() // 3 and stays[pix].all()
    pix0 = kf0[:, 3].astype(np.int64)                       # keyframe 0: the registration scan itself
    bits_equal(kf0[:, :3], scans[0][0][pix0])


def test_driver_dynamic_voxel_filtered(scans):
    """The default filters: the static cloud's fused crop + voxel pass around the pose, then the submap's."""
    p = odom_params()
    off = run_dynamic(scans, p, None, False, "device")
    on = run_dynamic(scans, p, lambda n: IR.with_intensity(np.zeros((n, 3)), seed=110)[:, 3], False, "device")
    assert on[0] == off[0]
    bits_equal(on[2][:, :3], off[2])
    _, _, kf, label, rid, T, _ = on
    world = np.column_stack([R.transform_f32(scans[1][0], T), IR.with_intensity(np.zeros((len(scans[1][0]), 3)), seed=110)[:, 3]])
    gone = removed_to_nan(world.astype(np.float32), label, [rid])
    want = IR.voxel_grid(IR.preprocess(gone, p.crop_size, p.vf_scan_res, T[:3, 3]), p.vf_submap_res)[0]
    bits_equal(kf, want)


def test_driver_dynamic_refusals(scans):
    od = OD.Odometry(0, odom_params())
    seg = S.Segmentation(0, seg_params())
    od.set_intensity(True, 12)
    a = np.column_stack([scans[0][0], np.zeros(len(scans[0][0]), np.float32)]).astype(np.float32)
    with pytest.raises(P.GicpError) as e:
        od.process_dynamic(seg, a, None)                    # on for the driver only
    assert e.value.status == EINVAL
    od.set_intensity(False)
    seg.set_intensity(True, 12)
    with pytest.raises(P.GicpError) as e:
        od.process_dynamic(seg, a, None)                    # on for the segmentation only
    assert e.value.status == EINVAL
    od.close()
    seg.close()


def test_driver_unorganized_cloud(scans):
    """Two points in one pixel: the later one's intensity is the pixel's."""
    p = odom_params(vf_scan_use=0, vf_submap_use=0)
    clouds = []
    for sensor, _ in scans:
        c = sensor[np.isfinite(sensor).all(axis=1)][::4]
        clouds.append(np.concatenate([c, c[:50]]))          # the first 50 points again, at the end
    n0 = len(clouds[1]) - 50
    runs = []
    for intensity in (False, True):
        od = OD.Odometry(0, p)
        seg = S.Segmentation(0, seg_params())
        if intensity:
            od.set_intensity(True, 16)
            seg.set_intensity(True, 16)
        for c in clouds:
            a = c
            if intensity:
                a = IR.records(np.column_stack([c, np.arange(len(c))]).astype(np.float32), 32, 16)
            r, sr, pr = od.process_dynamic_cloud(seg, a, lambda objs: [False] * len(objs))
        assert r.status == OD.TRACKED and r.keyframe_added == 1
        win, pix = seg.projection_maps()
        runs.append((result_bytes(r), od.keyframe_points(1, intensity=intensity), win, pix, pr))
        od.close()
        seg.close()
    (ra, ka, wa, pa, _), (rb, kb, wb, pb, pr) = runs
    assert ra == rb
    bits_equal(kb[:, :3], ka)
    np.testing.assert_array_equal(wa, wb)
    src = kb[:, 3].astype(np.int64)                         # the point every keyframe point came from
    assert (kb[:, 3] == src).all()
    np.testing.assert_array_equal(wb.reshape(-1)[pb[src]], src)      # it is the winner of its pixel
    assert (np.diff(pb[src]) > 0).all()                               # pixel order
    twice = np.flatnonzero(pb[:50] >= 0)
    assert 0 < len(twice) <= pr.collisions
    assert not np.isin(twice, src).any()                              # the earlier of the two never shows
    assert np.isin(n0 + twice, src).any()                             # the later one does, where the crop box lets it


def test_driver_tracked_downsampled(scans):
    """The tracker on board with the row/column filter on: the lists of the tracks frame 1 creates (UNDEFINED,
    so removed at once) are marked in the byte flags when w is the channel."""
    from dynamic_direct_lidar_odometry_amd import tracking as TR
    kw = dict(min_dynamic_hits=3, max_undefined_hits=2, max_obj_velocity=15.0, min_dist_from_origin=0.3,
              residuum_height_ratio=0.0, max_no_hits=30)
    p = odom_params(vf_scan_use=0, vf_submap_use=0)
    runs = []
    for intensity in (False, True):
        od = OD.Odometry(0, p)
        seg = S.Segmentation(0, seg_params(), labelling="device")
        trk = TR.Tracker(TR.default_track_params(**kw))
        od.set_downsampling(1, 2, 2, SROWS, SCOLS)
        seg.set_downsampling(1, 2, 2)
        if intensity:
            od.set_intensity(True, 12)
            seg.set_intensity(True, 12)
        out = []
        for k, (sensor, _) in enumerate(scans):
            a = sensor
            if intensity:
                a = np.column_stack([sensor, np.arange(len(sensor), dtype=np.float32)]).astype(np.float32)
            r, sr, tr = od.process_tracked(seg, trk, a, 0.1 * (k + 1))
            out.append((result_bytes(r), tr.created, tr.indices_dropped))
        assert r.status == OD.TRACKED and r.keyframe_added == 1 and tr.indices_dropped > 0
        runs.append((out, od.keyframe_points(1, intensity=intensity), np.array(r.T, np.float32).reshape(4, 4),
                     seg.downsampling_skipped))
        for h in (od, seg, trk):
            h.close()
    (fa, ka, _, sa), (fb, kb, T, sb) = runs
    assert fa == fb and sa == sb is False
    bits_equal(kb[:, :3], ka, "the keyframe loses exactly the pixels it loses today")
    pix = kb[:, 3].astype(np.int64)
    assert (kb[:, 3] == pix).all() and (np.diff(pix) > 0).all()
    bits_equal(kb[:, :3], R.transform_f32(scans[1][0], T)[pix])
