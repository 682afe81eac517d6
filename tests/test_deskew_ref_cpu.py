"""CPU checks of the deskew's numpy restatement (tests/deskew_ref.py) against geometry it did not produce:
a plane room swept by a moving sensor, whose every ray records the plane it hit."""
import numpy as np
import pytest

import deskew_ref as DR

PERIOD = 0.1
T_REF = DR.make_T([0.01, -0.02, 0.4], [1.5, -2.0, DR.SENSOR_Z])
TWISTS = [DR.TEETH_TWIST,
          (np.array([0.0, 0.0, 0.0]), np.array([0.3, -0.1, 0.02])),          # pure translation
          (np.array([0.05, 0.02, -0.3]), np.array([0.0, 0.0, 0.0])),         # pure rotation
          (np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.0]))]            # the sensor stands


@pytest.mark.parametrize("k", range(len(TWISTS)))
def test_reference_against_the_room(k):
    omega, t = TWISTS[k]
    xyz, s, face = DR.room_scan(T_REF, omega, t)
    assert len(xyz) == DR.ROWS * DR.COLS and np.isfinite(xyz).all()
    assert len(np.unique(face)) >= 5                         # ground, walls and the box are all seen
    assert np.linalg.norm(xyz, axis=1).max() <= 40.0         # the bound's premise
    got = DR.deskew(xyz, s * PERIOD, omega, t, 0.0, PERIOD)
    d = DR.plane_distance(got, T_REF, face)
    print("twist", k, "max plane distance", d.max())
    assert d.max() <= DR.BOUND
    # the same scan with the reference instant at the sweep's end, every s in [-1, 0): under a pure
    # translation the pose at s relative to the end pose T_ref * (I, t) is exactly (I, (s - 1) t)
    if k == 1:
        T_end = T_REF @ DR.make_T(omega, t)
        got = DR.deskew(xyz, s * PERIOD, omega, t, PERIOD, PERIOD)
        assert DR.plane_distance(got, T_end, face).max() <= DR.BOUND


def test_teeth():
    omega, t = DR.TEETH_TWIST
    xyz, s, face = DR.room_scan(T_REF, omega, t)
    d = DR.plane_distance(xyz, T_REF, face)                  # the sweep taken as an instant
    assert (d > DR.BOUND).mean() > 0.5
    assert d.max() > 0.5                                     # metres, at the far walls
    # a deskew with the wrong sign, or with a screw motion's bent translation, misses the bound too
    wrong = DR.deskew(xyz, s * PERIOD, -omega, -t, 0.0, PERIOD)
    assert (DR.plane_distance(wrong, T_REF, face) > DR.BOUND).mean() > 0.5


def test_special_cases():
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-30, 30, (200, 3)).astype(np.float32)
    tau = rng.uniform(0, 0.1, 200)
    xyz[5, 1] = np.nan
    xyz[6, 0] = np.inf
    tau[7] = np.nan
    tau[8] = np.inf
    omega, t = DR.TEETH_TWIST
    got = DR.deskew(xyz, tau, omega, t, 0.05, PERIOD)
    for i in (5, 6, 7, 8):
        assert got[i].tobytes() == xyz[i].tobytes()
    moved = np.ones(200, bool)
    moved[[5, 6, 7, 8]] = False
    assert (got[moved] != xyz[moved]).any(axis=1).all()
    assert DR.deskew(xyz, tau, [0, 0, 0], [0, 0, 0], 0.05, PERIOD).tobytes() == xyz.tobytes()
    # pure translation: one add per coordinate
    tr = DR.deskew(xyz, tau, [0, 0, 0], t, 0.05, PERIOD)
    s = (tau - 0.05) / PERIOD
    want = (xyz[moved].astype(np.float64) + s[moved, None] * t[None, :]).astype(np.float32)
    assert tr[moved].tobytes() == want.tobytes()


def test_time_types():
    ns = np.array([0, 1, 99_999_999, 4_294_967_295], np.uint32)
    np.testing.assert_array_equal(DR.seconds(ns, DR.U32_NS), ns.astype(np.float64) * 1e-9)
    f = np.array([0.0, 0.05, np.nan], np.float32)
    assert DR.seconds(f, DR.F32_S).dtype == np.float64
    rec = DR.records(np.zeros((3, 3)), f, DR.F32_S, 20)
    assert rec.shape == (3, 20) and rec[:, 16:20].tobytes() == f.tobytes() and (rec[:, 12:16] == 0xA5).all()
    rec = DR.records(np.zeros((2, 3)), [1.5, 2.5], DR.F64_S, 32, intensity=[7, 8], intensity_offset=12)
    assert rec[:, 24:32].tobytes() == np.array([1.5, 2.5]).tobytes()
    assert DR.as_f32_rows(rec)[:, 3].tolist() == [7.0, 8.0]


def test_split_log():
    rng = np.random.default_rng(11)
    worst = 0.0
    for i in range(400):
        w = rng.normal(size=3)
        w *= rng.uniform(0, 1) / np.linalg.norm(w)
        if i % 50 == 0:
            w *= 1e-6                                        # small angles
        if i == 1:
            w = np.array([0.0, 0.0, 1.0])                    # |omega| = 1
        t = rng.normal(size=3)
        got_w, got_t = DR.se3_split_log(DR.make_T(w, t))
        worst = max(worst, np.abs(got_w - w).max())
        assert (got_t == t).all()
    print("split log: worst |omega error|", worst)
    assert worst <= 1e-12
    w0, _ = DR.se3_split_log(np.eye(4))
    assert (w0 == 0).all()
    # the prediction: the twist of a constant motion from two of its poses
    A = DR.make_T([0.1, 0.2, -0.3], [1, 2, 3])
    D = DR.make_T([0.01, -0.02, 0.05], [0.2, 0.0, 0.01])
    w, t = DR.predict(A.astype(np.float32), (A @ D).astype(np.float32))
    assert np.abs(w - [0.01, -0.02, 0.05]).max() < 1e-6 and np.abs(t - [0.2, 0.0, 0.01]).max() < 1e-5


def test_sequence_is_consistent():
    seq = DR.sequence(7)
    signs = [np.sign(w[2]) for _, w, _, _ in seq]
    assert signs[0] > 0 and signs[-1] < 0
    for (Ta, w, t, _), (Tb, _, _, _) in zip(seq, seq[1:]):
        np.testing.assert_allclose(np.linalg.inv(Ta) @ Tb, DR.make_T(w, t), atol=1e-12)
        assert abs(Tb[0, 3]) < 15 and abs(Tb[1, 3]) < 15
