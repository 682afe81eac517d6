"""numpy restatement of the motion deskew (include/ddlo_deskew.h): the per-point arithmetic in the header's
operation order, the split log, and a small plane-room ray caster that produces skewed scans whose true
geometry is known (checked by tests/test_deskew_ref_cpu.py; the GPU tests compare the device against it).

numpy's elementwise float64 operations are single IEEE operations (no contraction), so the pure-translation
case restates the device bit for bit; with a rotation the two sides differ in sin and cos alone.
"""
import numpy as np

F32_S, U32_NS, F64_S = 0, 1, 2
TIME_DTYPE = {F32_S: np.float32, U32_NS: np.uint32, F64_S: np.float64}
TIME_SIZE = {F32_S: 4, U32_NS: 4, F64_S: 8}


# ---- the model -------------------------------------------------------------------------------------------
def seconds(field, time_type):
    """The time field as the kernel takes it: seconds in double."""
    f = np.asarray(field)
    if time_type == U32_NS:
        return f.astype(np.uint32).astype(np.float64) * 1e-9
    return f.astype(TIME_DTYPE[time_type]).astype(np.float64)


def fraction(tau, ref_time, period):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(tau, np.float64) - np.float64(ref_time)) / np.float64(period)


def deskew(xyz, tau, omega, t, ref_time, period):
    """p' = Exp(s omega) p + s t of every float32 point with finite coordinates and a finite time tau
    (seconds, double); the others keep their bits.  An identity twist returns the input."""
    p32 = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = p32.copy()
    wx, wy, wz = (float(v) for v in omega)
    t = [float(v) for v in t]
    if wx == 0 and wy == 0 and wz == 0 and t[0] == 0 and t[1] == 0 and t[2] == 0:
        return out
    tau = np.asarray(tau, np.float64).reshape(-1)
    ok = np.isfinite(p32).all(axis=1) & np.isfinite(tau)
    s = fraction(tau[ok], ref_time, period)
    px, py, pz = (p32[ok, a].astype(np.float64) for a in range(3))
    p = (px, py, pz)
    st = [s * t[a] for a in range(3)]
    theta = np.sqrt(np.float64(wx) * wx + np.float64(wy) * wy + np.float64(wz) * wz)
    with np.errstate(over="ignore", invalid="ignore"):
        if theta == 0:
            res = [p[a] + st[a] for a in range(3)]
        else:
            kx, ky, kz = wx / theta, wy / theta, wz / theta
            k = (kx, ky, kz)
            a_ = s * theta
            sn, cs = np.sin(a_), np.cos(a_)
            c = (ky * pz - kz * py, kz * px - kx * pz, kx * py - ky * px)
            d = (kx * px + ky * py) + kz * pz
            e = d * (1.0 - cs)
            res = [((p[a] * cs + c[a] * sn) + k[a] * e) + st[a] for a in range(3)]
        for a in range(3):
            out[ok, a] = res[a].astype(np.float32)
    return out


def exp_so3(w):
    """Rodrigues' formula in double."""
    w = np.asarray(w, np.float64)
    th = np.sqrt(w @ w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def make_T(omega, t):
    T = np.eye(4)
    T[:3, :3] = exp_so3(omega)
    T[:3, 3] = t
    return T


def se3_split_log(T):
    """(omega, t) of a 4x4 transform (any float type, taken in double): the header's split log."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    a = 0.5 * np.array([T[2, 1] - T[1, 2], T[0, 2] - T[2, 0], T[1, 0] - T[0, 1]])
    na = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    t = T[:3, 3].copy()
    if na == 0:
        return np.zeros(3), t
    theta = np.arctan2(na, ((T[0, 0] + T[1, 1] + T[2, 2]) - 1.0) / 2.0)
    return a * (theta / na), t


def predict(Ta, Tb):
    """The constant-velocity twist: the split log of inv(T_a) T_b, float32 poses taken in double, the
    rigid inverse (R^T, -R^T t)."""
    Ta, Tb = np.asarray(Ta, np.float32).astype(np.float64).reshape(4, 4), np.asarray(Tb, np.float32).astype(np.float64).reshape(4, 4)
    inv = np.eye(4)
    inv[:3, :3] = Ta[:3, :3].T
    inv[:3, 3] = -(Ta[:3, :3].T @ Ta[:3, 3])
    return se3_split_log(inv @ Tb)


# ---- records ---------------------------------------------------------------------------------------------
def records(xyz, field, time_type, stride, offset=None, intensity=None, intensity_offset=None):
    """(n, stride) uint8 rows: x, y, z float32, the time field at `offset` (default: the record's last
    bytes), optionally an intensity; every other byte is 0xA5 filler."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    size = TIME_SIZE[time_type]
    if offset is None:
        offset = stride - size
    rec = np.full((n, stride), 0xA5, np.uint8)
    rec[:, :12] = xyz.view(np.uint8).reshape(n, 12)
    f = np.ascontiguousarray(field, TIME_DTYPE[time_type]).reshape(n)
    rec[:, offset:offset + size] = f.view(np.uint8).reshape(n, size)
    if intensity is not None:
        i = np.ascontiguousarray(intensity, np.float32).reshape(n)
        rec[:, intensity_offset:intensity_offset + 4] = i.view(np.uint8).reshape(n, 4)
    return rec


def as_f32_rows(rec):
    """uint8 records (stride a multiple of 4) as float32 rows, bits kept: what the dynamic entries take."""
    return np.ascontiguousarray(rec).view(np.float32)


# ---- the plane room ----------------------------------------------------------------------------------------
ROWS, COLS = 16, 256
HALF = 20.0            # walls at x, y = +-HALF
SENSOR_Z = 1.8
ANG = 15.0             # beams evenly spaced from +ANG (row 0) to -ANG (the last row), the segmentation's ring model
BOX = ((5.0, 7.0), (-3.0, -1.0), (0.0, 1.5))      # one box on the ground, for the segmentation to find

# (axis, value, bounds of the two other axes or None)
FACES = [(2, 0.0, None), (0, HALF, None), (0, -HALF, None), (1, HALF, None), (1, -HALF, None)]
for _a in range(3):
    for _v in BOX[_a]:
        FACES.append((_a, _v, tuple(BOX[b] for b in range(3) if b != _a)))


def beams(rows=ROWS, cols=COLS):
    """Unit directions (rows * cols, 3), row-major, and each ray's fraction of the period (column-ordered,
    in [0, 1)): column c looks along azimuth 2 pi c / cols and is fired at s = c / cols."""
    el = np.radians(np.linspace(ANG, -ANG, rows))
    az = 2 * np.pi * np.arange(cols) / cols
    e, a = np.meshgrid(el, az, indexing="ij")
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1).reshape(-1, 3)
    s = np.broadcast_to(np.arange(cols) / cols, (rows, cols)).reshape(-1).copy()
    return d, s


def room_scan(T_ref, omega, t, rows=ROWS, cols=COLS):
    """One sweep of the room by a sensor that moves while it scans: ray i is cast from the pose
    T_ref * (Exp(s_i omega), s_i t).  Returns (xyz float32 in each ray's own sensor frame, s, face index)."""
    T_ref = np.asarray(T_ref, np.float64)
    d, s = beams(rows, cols)
    n = len(d)
    xyz = np.zeros((n, 3), np.float32)
    face = np.full(n, -1, np.int64)
    t = np.asarray(t, np.float64)
    for c in range(cols):
        idx = np.arange(rows) * cols + c
        R = T_ref[:3, :3] @ exp_so3(s[idx[0]] * np.asarray(omega, np.float64))
        o = T_ref[:3, :3] @ (s[idx[0]] * t) + T_ref[:3, 3]
        dw = d[idx] @ R.T
        best = np.full(rows, np.inf)
        bf = np.full(rows, -1, np.int64)
        for f, (ax, val, bounds) in enumerate(FACES):
            with np.errstate(divide="ignore", invalid="ignore"):
                r = (val - o[ax]) / dw[:, ax]
            hit = np.isfinite(r) & (r > 1e-9) & (r < best)
            if bounds is not None:
                others = [b for b in range(3) if b != ax]
                for (lo, hi), b in zip(bounds, others):
                    q = o[b] + r * dw[:, b]
                    hit &= (q >= lo) & (q <= hi)
            best = np.where(hit, r, best)
            bf = np.where(hit, f, bf)
        assert (bf >= 0).all()
        xyz[idx] = (d[idx] * best[:, None]).astype(np.float32)
        face[idx] = bf
    return xyz, s, face


def plane_distance(p_ref, T_ref, face):
    """|distance| of T_ref * p (p in the reference-instant frame) to the plane of the face each ray hit."""
    T_ref = np.asarray(T_ref, np.float64)
    w = np.asarray(p_ref, np.float64) @ T_ref[:3, :3].T + T_ref[:3, 3]
    ax = np.array([FACES[f][0] for f in face])
    val = np.array([FACES[f][1] for f in face])
    return np.abs(w[np.arange(len(w)), ax] - val)


BOUND = 5e-5           # float32 storage at <= 40 m costs <= 4e-6 m per coordinate; tenfold margin
TEETH_TWIST = (np.array([0.02, -0.01, 0.5]), np.array([0.2, 0.05, 0.0]))


def sequence(frames=7, period=0.1):
    """A drive through the room whose yaw rate changes sign mid-way: per frame (T_ref, omega, t, ref_time),
    T_ref of frame k + 1 = T_ref of frame k * (Exp(omega_k), t_k)."""
    T = make_T([0, 0, 0.3], [-4.0, 1.0, SENSOR_Z])
    out = []
    for k in range(frames):
        yaw = 0.05 if k < frames // 2 else -0.05          # 30 deg/s at 10 Hz
        omega = np.array([0.002, -0.001, yaw])
        t = np.array([0.2, 0.01 * (k % 3), 0.0])          # 2 m/s
        out.append((T.copy(), omega, t, period * k))
        T = T @ make_T(omega, t)
    return out
