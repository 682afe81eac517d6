"""GPU tests of the opt-in motion deskew (include/ddlo_deskew.h) against its numpy restatement
(tests/deskew_ref.py, checked on the CPU by tests/test_deskew_ref_cpu.py).

Pure translation is compared on bits; a rotation within one float rounding plus 2^-40 (|p| + |s t|), which
covers the fp64 chain (a dozen operations at 2^-53 plus sin and cos at about an ulp: about 2^-48) with a
256-fold margin; the drivers, deskewing themselves or fed ddlo_deskew's output, on bits again.

A double time needs offset % 8 == 0, offset >= 12 and stride % 8 == 0, so it fits none of the 16 B and 20 B
records: there it is refused (asserted), and it is exercised at 24 B and 32 B.
"""
import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import segmentation as S

import deskew_ref as DR

pytestmark = pytest.mark.gpu

EINVAL = 1
PERIOD = 0.1
TYPES = (DR.F32_S, DR.U32_NS, DR.F64_S)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits_equal(got, ref, what=""):
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=what)


def times(n, time_type, seed):
    """(field values, a reference time inside their range, one outside it)."""
    rng = np.random.default_rng(seed)
    if time_type == DR.F32_S:
        return rng.uniform(0.0, 0.1, n).astype(np.float32), 0.05, -0.07
    if time_type == DR.U32_NS:
        return rng.integers(0, 100_000_000, n).astype(np.uint32), 0.05, 0.13
    return 1.7e9 + rng.uniform(0.0, 0.1, n), 1.7e9 + 0.05, 1.7e9 - 0.1     # absolute stamps


def cloud(n, seed):
    return np.random.default_rng(seed).uniform(-40, 40, (n, 3)).astype(np.float32)


def with_bad_points(xyz, field, time_type):
    """Some NaN / Inf coordinates and, where the type has one, one NaN time."""
    xyz, field = xyz.copy(), field.copy()
    n = len(xyz)
    if n >= 63:
        xyz[3, 0] = np.nan
        xyz[17, 2] = np.inf
        xyz[n - 1, 1] = np.nan
        xyz[40] = np.nan
        if time_type != DR.U32_NS:
            field[n - 2] = np.nan
            field[5] = np.inf
    return xyz, field


def gpu_deskew(rec, time_type, offset, omega, t, ref, period=PERIOD):
    return OD.deskew(rec, omega, t, offset, time_type, ref, period)


# ---- pure translation, bit for bit -----------------------------------------------------------------------
# strides 16, 20 and 32 for every type (a double time is refused at 16 and 20), and 24 for the double
LAYOUTS = [(stride, tt) for tt in TYPES for stride in (16, 20, 32)] + [(24, DR.F64_S)]


@pytest.mark.parametrize("stride,time_type", LAYOUTS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_pure_translation_bits(n, stride, time_type):
    size = DR.TIME_SIZE[time_type]
    offset = stride - size                                   # the record's last bytes
    xyz = cloud(n, 100 + n)
    field, inside, outside = times(n, time_type, 200 + n)
    xyz, field = with_bad_points(xyz, field, time_type)
    t = np.array([0.3, -0.12, 0.021])
    zero = np.zeros(3)
    if time_type == DR.F64_S and stride in (16, 20):
        rec = np.zeros((n, stride), np.uint8)
        with pytest.raises(P.GicpError) as e:
            gpu_deskew(rec, time_type, max(offset, 12), zero, t, inside)
        assert e.value.status == EINVAL
        return
    rec = DR.records(xyz, field, time_type, stride, offset)
    tau = DR.seconds(field, time_type)
    for ref in (inside, outside):
        want = DR.deskew(xyz, tau, zero, t, ref, PERIOD)
        got = gpu_deskew(rec, time_type, offset, zero, t, ref)
        np.testing.assert_array_equal(u32(got), u32(want), err_msg=f"n {n} stride {stride} type {time_type} ref {ref}")
        ok = np.isfinite(xyz).all(axis=1) & np.isfinite(tau)
        assert (u32(got)[~ok] == u32(xyz)[~ok]).all()
        assert (u32(got)[ok] != u32(xyz)[ok]).any()
    # the time really is read from the record's last bytes: another time in the last record moves its point
    if np.isfinite(xyz[-1]).all() and time_type != DR.F64_S:
        rec2 = rec.copy()
        other_field = [np.float32(0.0123)] if time_type == DR.F32_S else [12_300_000]
        rec2[-1] = DR.records(xyz[-1:], other_field, time_type, stride, offset)[0]
        a, b = gpu_deskew(rec, time_type, offset, zero, t, inside), gpu_deskew(rec2, time_type, offset, zero, t, inside)
        assert (u32(a)[:-1] == u32(b)[:-1]).all()
        want = DR.deskew(xyz[-1:], DR.seconds(other_field, time_type), zero, t, inside, PERIOD)
        np.testing.assert_array_equal(u32(b)[-1:], u32(want))
    # zero twist: the output bits are the input's
    np.testing.assert_array_equal(u32(gpu_deskew(rec, time_type, offset, zero, zero, inside)), u32(xyz))
    assert len(OD.deskew(rec[:0], zero, t, offset, time_type, inside, PERIOD)) == 0       # n == 0 is OK


# ---- rotation, against the reference ------------------------------------------------------------------------
ROT_TWISTS = [((0.02, -0.01, 0.5), (0.2, 0.05, 0.0)),
              ((0.6, -0.5, 0.62), (1.0, -2.0, 0.5)),          # |omega| ~ 1
              ((0.0, 0.0, -1.0), (0.0, 0.0, 0.0)),
              ((1e-9, 0.0, 2e-9), (0.1, 0.0, 0.0)),           # a tiny angle
              ((0.0, 1e-3, 0.0), (-0.3, 0.3, 3.0))]


@pytest.mark.parametrize("time_type", TYPES)
@pytest.mark.parametrize("k", range(len(ROT_TWISTS)))
def test_rotation_against_reference(k, time_type):
    omega, t = (np.array(v, np.float64) for v in ROT_TWISTS[k])
    assert np.linalg.norm(omega) <= 1.0
    n = 1500
    xyz = cloud(n, 300 + k)
    xyz[::97] *= 1e-3                                        # small coordinates: cancellation
    rng = np.random.default_rng(400 + k)
    # |s| <= 2 around the reference time
    if time_type == DR.F32_S:
        field, ref = rng.uniform(0.0, 0.4, n).astype(np.float32), 0.2
    elif time_type == DR.U32_NS:
        field, ref = rng.integers(0, 400_000_000, n).astype(np.uint32), 0.2
    else:
        field, ref = 1.7e9 + rng.uniform(0.0, 0.4, n), 1.7e9 + 0.2
    stride = 32 if time_type == DR.F64_S else 20
    offset = stride - DR.TIME_SIZE[time_type]
    xyz, field = with_bad_points(xyz, field, time_type)
    tau = DR.seconds(field, time_type)
    s = DR.fraction(tau, ref, PERIOD)
    ok = np.isfinite(xyz).all(axis=1) & np.isfinite(tau)
    assert np.abs(s[ok]).max() <= 2.0 + 1e-6
    want = DR.deskew(xyz, tau, omega, t, ref, PERIOD)
    got = gpu_deskew(DR.records(xyz, field, time_type, stride, offset), time_type, offset, omega, t, ref)
    assert (u32(got)[~ok] == u32(xyz)[~ok]).all()
    scale = np.linalg.norm(xyz[ok].astype(np.float64), axis=1) + np.linalg.norm(s[ok, None] * t[None, :], axis=1)
    bound = np.spacing(np.abs(want[ok])).astype(np.float64) + 2.0 ** -40 * scale[:, None]
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
    print("twist", k, "type", time_type, "worst error / bound", (err / bound).max(), "differing coordinates",
          int((err > 0).sum()), "of", err.size)
    assert (err <= bound).all()


# ---- geometry: the device's output lies on the room's planes --------------------------------------------------
@pytest.mark.parametrize("time_type", TYPES)
def test_geometry_on_the_room(time_type):
    T_ref = DR.make_T([0.01, -0.02, 0.4], [1.5, -2.0, DR.SENSOR_Z])
    omega, t = DR.TEETH_TWIST
    xyz, s, face = DR.room_scan(T_ref, omega, t)
    if time_type == DR.F32_S:
        field, ref = (s * PERIOD).astype(np.float32), 0.0    # relative to the sweep's start, as Velodyne's
    elif time_type == DR.U32_NS:
        field, ref = np.round(s * 1e8).astype(np.uint32), 0.0
    else:
        field, ref = 1000.0 + s * PERIOD, 1000.0             # (a double near 1.7e9 s resolves 2.4e-7 s: not for this bound)
    stride = 32 if time_type == DR.F64_S else 16
    offset = stride - DR.TIME_SIZE[time_type]
    got = gpu_deskew(DR.records(xyz, field, time_type, stride, offset), time_type, offset, omega, t, ref)
    d = DR.plane_distance(got, T_ref, face)
    print("type", time_type, "max plane distance", d.max())
    assert (DR.plane_distance(xyz, T_ref, face) > DR.BOUND).mean() > 0.5
    assert d.max() <= DR.BOUND


# ---- the drivers ---------------------------------------------------------------------------------------------
def odom_params(**kw):
    # every tracked frame is 0.2 m from the last keyframe: each becomes one
    return OD.default_odom_params(adaptive=0, keyframe_thresh_dist=0.05, vf_scan_res=0.2, vf_submap_res=0.2, **kw)


def seg_params():
    return S.yaml_seg_params(rows=DR.ROWS, cols=DR.COLS, ang_bottom=DR.ANG, ground_rows=8, win_row0=0, win_row1=DR.ROWS - 1,
                             win_col0=0, win_col1=DR.COLS - 1, max_distance=30)


def result_bytes(r):
    """Every field of ddlo_odom_result but the gicp_results' device timings."""
    def g(x):
        return (x.converged, x.nr_iterations, x.iterations_run, x.lm_failed, x.lm_trials, x.num_correspondences,
                x.final_cost, bytes(np.array(x.final_hessian)), x.lm_lambda)
    return (r.status, r.scan_points, bytes(r.T), bytes(r.T_s2s), bytes(r.T_s2s_local), g(r.s2s), g(r.s2m),
            r.keyframe_added, r.num_keyframes, r.submap_changed, r.submap_keyframes, r.submap_points, r.spaciousness,
            r.keyframe_thresh_dist)


def objects_bytes(o):
    return tuple(np.ascontiguousarray(o[k]).tobytes() for k in S.OBJECT_DTYPE.names)


@pytest.fixture(scope="module")
def seq():
    """Per frame: (skewed xyz with no-return pixels, s, omega, t, ref_time, T_ref)."""
    out = []
    for k, (T, omega, t, ref) in enumerate(DR.sequence(7, PERIOD)):
        xyz, s, _ = DR.room_scan(T, omega, t)
        xyz[np.random.default_rng(k).random(len(xyz)) < 0.02] = np.nan
        out.append((xyz, s, omega, t, ref, T))
    return out


def frame_records(frame, layout):
    """(float32 rows for driver A, time offset, intensity or None) of one frame in one record layout:
    'xyzt' 16 B, 'xyz_t' 20 B with the time in the last bytes, 'xyzit' 20 B with the time behind an intensity."""
    xyz, s, _, _, ref, _ = frame
    tau = (ref + s * PERIOD).astype(np.float32)
    if layout == "xyzt":
        return DR.as_f32_rows(DR.records(xyz, tau, DR.F32_S, 16, 12)), 12, None
    if layout == "xyz_t":
        return DR.as_f32_rows(DR.records(xyz, tau, DR.F32_S, 20, 16)), 16, None
    inten = np.arange(len(xyz), dtype=np.float32)
    return DR.as_f32_rows(DR.records(xyz, tau, DR.F32_S, 20, 16, inten, 12)), 16, inten


def run_pair(seq, entry, layout="xyzt", rowcol=False):
    """Driver A (deskew on, skewed records, the true twist through set_deskew_motion) and driver B (deskew off,
    fed ddlo_deskew of the same records with the same twist): everything they report, frame by frame."""
    runs = []
    for which in "AB":
        od = OD.Odometry(0, odom_params())
        seg = S.Segmentation(0, seg_params()) if entry != "process" else None
        inten_on = layout == "xyzit"
        if inten_on:
            od.set_intensity(True, 12)
            if seg is not None:
                seg.set_intensity(True, 12)
        if rowcol:
            od.set_downsampling(1, 2, 2, DR.ROWS, DR.COLS)
            if seg is not None:
                seg.set_downsampling(1, 2, 2)
        out = []
        for frame in seq:
            rows, toff, inten = frame_records(frame, layout)
            _, _, omega, t, ref, _ = frame
            if entry == "cloud":                             # unorganized: the returns only
                rows = rows[np.isfinite(rows[:, :3]).all(axis=1)]
                inten = None if inten is None else rows[:, 3]
            if which == "A":
                od.set_deskew(True, toff, DR.F32_S, ref, PERIOD)
                od.set_deskew_motion(omega, t)
                a = rows
            else:
                a = OD.deskew(rows, omega, t, toff, DR.F32_S, ref, PERIOD)
                if inten_on:
                    a = np.column_stack([a, inten]).astype(np.float32)
            if entry == "process":
                r = od.process(a)
                rec = [result_bytes(r)]
            elif entry == "dynamic":
                r, sr = od.process_dynamic(seg, a, lambda objs: [i == 0 for i in range(len(objs))])
                rec = [result_bytes(r), bytes(sr)]
                if r.status == OD.TRACKED:
                    rec += [x.tobytes() for x in seg.images()] + [objects_bytes(seg.objects())]
            else:
                r, sr, pr = od.process_dynamic_cloud(seg, a, lambda objs: [i == 0 for i in range(len(objs))])
                rec = [result_bytes(r), bytes(sr), bytes(pr)]
                if r.status == OD.TRACKED:
                    rec += [x.tobytes() for x in seg.images()] + [objects_bytes(seg.objects())]
                    rec += [x.tobytes() for x in seg.projection_maps()]
            if which == "A":
                w, v, src = od.deskew_motion()
                if r.status in (OD.TRACKED, OD.FIRST):
                    assert src == 2 and (w == omega).all() and (v == t).all()
                else:
                    assert src == 0
            out.append(rec)
        assert r.status == OD.TRACKED
        kfs = [od.keyframe_points(k, intensity=inten_on) for k in range(r.num_keyframes)]
        runs.append((out, kfs, r.num_keyframes))
        od.close()
        if seg is not None:
            seg.close()
    return runs


def assert_pair_equal(runs):
    (fa, ka, na), (fb, kb, nb) = runs
    assert na == nb and na >= 3, "the sequence adds keyframes"
    for k, (a, b) in enumerate(zip(fa, fb)):
        assert len(a) == len(b)
        for j, (x, y) in enumerate(zip(a, b)):
            assert x == y, f"frame {k}, item {j}"
    for k, (a, b) in enumerate(zip(ka, kb)):
        bits_equal(a, b, f"keyframe {k}")


def test_driver_equivalence_process(seq):
    runs = run_pair(seq, "process", "xyz_t")
    assert_pair_equal(runs)
    # and the deskew does change what the driver computes: a third driver, deskew off, on the skewed records
    od = OD.Odometry(0, odom_params())
    for frame in seq:
        r = od.process(frame[0])
    assert result_bytes(r) != runs[0][0][-1][0]
    od.close()


@pytest.mark.parametrize("layout,rowcol", [("xyzt", False), ("xyzt", True), ("xyzit", False)])
def test_driver_equivalence_dynamic(seq, layout, rowcol):
    assert_pair_equal(run_pair(seq, "dynamic", layout, rowcol))


def test_driver_equivalence_dynamic_cloud(seq):
    assert_pair_equal(run_pair(seq, "cloud", "xyz_t"))


# ---- prediction -------------------------------------------------------------------------------------------------
def test_prediction(seq):
    od = OD.Odometry(0, odom_params())
    poses = []
    seen = 0
    for k, frame in enumerate(seq):
        rows, toff, _ = frame_records(frame, "xyz_t")
        od.set_deskew(True, toff, DR.F32_S, frame[4], PERIOD)
        if k == 4:                                           # a SKIPPED frame in between leaves the history alone
            r = od.process(rows[:5])
            assert r.status == OD.SKIPPED
            assert od.deskew_motion()[2] == 0
        r = od.process(rows)
        w, v, src = od.deskew_motion()
        if len(poses) >= 2 and r.status == OD.TRACKED:
            want_w, want_v = DR.predict(poses[-2], poses[-1])
            assert src == 1
            assert np.abs(w - want_w).max() <= 1e-9 and np.abs(v - want_v).max() <= 1e-9
            lw, lv = OD.se3_split_log(np.linalg.inv(poses[-2].astype(np.float64)) @ poses[-1].astype(np.float64))
            assert np.abs(lw - want_w).max() < 1e-5          # (through a float32 matrix)
            seen += 1
        else:
            assert src == 0 and (w == 0).all() and (v == 0).all()
        if r.status in (OD.FIRST, OD.TRACKED):
            poses.append(np.array(r.T, np.float32).reshape(4, 4))
    assert seen >= 3 and r.status == OD.TRACKED
    # the caller's twist wins over the prediction, for one scan
    od.set_deskew_motion([0, 0, 0.01], [0.1, 0, 0])
    od.process(rows)
    assert od.deskew_motion()[2] == 2
    od.process(rows)
    assert od.deskew_motion()[2] == 1
    od.close()


def test_split_log_binding():
    T = DR.make_T([0.3, -0.2, 0.5], [1, 2, 3]).astype(np.float32)
    w, t = OD.se3_split_log(T)
    rw, rt = DR.se3_split_log(T)
    assert np.abs(w - rw).max() <= 1e-12 and (t == rt).all()
    w, t = OD.se3_split_log(np.eye(4))
    assert (w == 0).all() and (t == 0).all()


# ---- refusals -----------------------------------------------------------------------------------------------------
BAD_FIELDS = [  # (time type, offset, stride): one rule of the header each
    (DR.F32_S, 14, 20),      # offset % 4
    (DR.F64_S, 12, 24),      # offset % 8 for a double
    (DR.F64_S, 16, 28),      # stride % 8 for a double
    (DR.U32_NS, 8, 16),      # offset < 12
    (DR.F32_S, 16, 16),      # offset + 4 > stride
    (DR.F64_S, 16, 16),      # offset + 8 > stride
]


def test_refusals(seq):
    twin, od = OD.Odometry(0, odom_params()), OD.Odometry(0, odom_params())
    for k, frame in enumerate(seq[:5]):
        rows, toff, _ = frame_records(frame, "xyz_t")
        _, _, omega, t, ref, _ = frame
        twin.set_deskew(True, toff, DR.F32_S, ref, PERIOD)
        twin.set_deskew_motion(omega, t)
        want = twin.process(rows)
        od.set_deskew_motion(omega, t)                       # pending across the refused calls
        for tt, off, stride in BAD_FIELDS:
            od.set_deskew(True, off, tt, ref, PERIOD)
            bad = np.zeros((len(rows), stride), np.uint8)
            with pytest.raises(P.GicpError) as e:
                od.process(bad)
            assert e.value.status == EINVAL, (tt, off, stride)
        od.set_deskew(True, toff, DR.F32_S, ref, PERIOD)
        for period in (0.0, -0.1, np.nan, np.inf):
            with pytest.raises(P.GicpError) as e:
                od.set_deskew(True, toff, DR.F32_S, ref, period)
            assert e.value.status == EINVAL
        with pytest.raises(P.GicpError) as e:
            od.set_deskew(True, toff, 3, ref, PERIOD)        # an unknown time type
        assert e.value.status == EINVAL
        with pytest.raises(P.GicpError) as e:
            od.set_deskew_motion([0, np.nan, 0], [0, 0, 0])
        assert e.value.status == EINVAL
        p = od.deskew()
        assert (p.use, p.time_type, p.time_offset_bytes, p.ref_time, p.period) == (1, DR.F32_S, toff, ref, PERIOD)
        got = od.process(rows)
        assert result_bytes(got) == result_bytes(want), f"frame {k}"
        if got.status in (OD.FIRST, OD.TRACKED):
            assert od.deskew_motion()[2] == 2
    assert got.status == OD.TRACKED and got.num_keyframes >= 3
    for k in range(got.num_keyframes):
        bits_equal(od.keyframe_points(k), twin.keyframe_points(k), f"keyframe {k}")
    twin.close()
    od.close()


def test_refusal_overlap_with_intensity(seq):
    rows, _, _ = frame_records(seq[0], "xyzit")
    od = OD.Odometry(0, odom_params(skip_first_scan=0))
    od.set_intensity(True, 12)
    for tt, off in ((DR.F32_S, 12),):                        # the time on the intensity
        od.set_deskew(True, off, tt, 0.0, PERIOD)
        with pytest.raises(P.GicpError) as e:
            od.process(rows)
        assert e.value.status == EINVAL
    od.set_intensity(True, 20)                               # a double time at 16 reaches into an intensity at 20
    od.set_deskew(True, 16, DR.F64_S, 0.0, PERIOD)
    with pytest.raises(P.GicpError) as e:
        od.process(np.zeros((len(rows), 24), np.uint8))
    assert e.value.status == EINVAL
    od.set_intensity(True, 12)
    od.set_deskew(True, 16, DR.F32_S, 0.0, PERIOD)
    assert od.process(rows).status == OD.FIRST               # the driver stayed usable
    od.close()


# ---- off is off ----------------------------------------------------------------------------------------------------
def test_off_is_off(seq):
    twin, od = OD.Odometry(0, odom_params()), OD.Odometry(0, odom_params())
    for k, frame in enumerate(seq):
        xyz = frame[0]
        want = twin.process(xyz)
        od.set_deskew(False, 3 + k, DR.F64_S, 5.0 * k, 7.0)  # use = 0: any other fields
        od.set_deskew_motion([0.1, 0.2, 0.3], [1, 2, 3])
        if k % 2 == 0:
            od.set_deskew_motion(None, None)                 # cleared; on odd frames it is dropped unused
        got = od.process(xyz)
        assert result_bytes(got) == result_bytes(want), f"frame {k}"
        w, v, src = od.deskew_motion()
        assert src == 0 and (w == 0).all() and (v == 0).all()
    assert got.status == OD.TRACKED and got.num_keyframes >= 3
    for k in range(got.num_keyframes):
        bits_equal(od.keyframe_points(k), twin.keyframe_points(k), f"keyframe {k}")
    twin.close()
    od.close()
