"""An unorganized cloud into the range image on the device (include/ddlo_seg_project.h): the maps, the
counts, the staged scan and everything downstream of it, against project_ref.py (the definition restated in
numpy float64) and against the organized entry on the frame the cloud came from.

Every comparison is array_equal outside the pixels project_ref.analyse excludes (those an undecided point can
reach and win: a point whose row, column or kept-status changes when its elevation or azimuth moves by 4 double
ulps, where the device's and the host's atan2 may differ).  test_project_ref_cpu.py shows that the ray-cast
frames used here have no undecided point in any of the geometries used; the one hand point that is placed
exactly between two rows is excluded by that analysis, the other hand points are decided.

Shapes: the smallest at which the kernels can go wrong: a 3 x 7 image (less than a wavefront), 16 x 256 (16
workgroups), clouds of 0, 1, 255, 256, 257 and 4,096 points (around the 256-thread workgroup), and one
64 x 2048 ray-cast frame for the comparison of the whole segmentation.
"""
import ctypes as C

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import scene
from dynamic_direct_lidar_odometry_amd import segmentation as S
import project_ref as PJ

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)
SMALL = [1, 63, 64, 65, 255, 256, 257]
POSE = np.array(scene.make_pose([0.5, 0.3, scene.SENSOR_Z], (0.01, -0.02, 0.3)), np.float32)


cast, blank = PJ.cast, PJ.blank
SMALL_Q = PJ.SMALL_PROJECTION


def small_projection():
    return S.ProjectionParams(SMALL_Q.elev_top, SMALL_Q.elev_res, SMALL_Q.azim0, SMALL_Q.azim_sign)


def params(rows, cols, **kw):
    """the ring model of scene.lidar_dirs for <= 64 rows, every pixel inside the labelling window"""
    d = dict(rows=rows, cols=cols, ang_bottom=22.5, ground_rows=min(4, rows - 1), minimum_range=0, win_row0=0,
             win_row1=rows - 1, win_col0=0, win_col1=cols - 1)
    d.update(kw)
    return S.default_seg_params(**d)


def ref_of(q: S.ProjectionParams) -> PJ.Projection:
    return PJ.Projection(q.elev_top_deg, q.elev_res_deg, q.azim0_deg, q.azim_sign)


def counts(pr):
    return (pr.points, pr.invalid, pr.out_of_view, pr.occupied_pixels, pr.collisions)


def check_maps(seg, pts, pr, proj=None):
    """the handle's maps and counts against the restatement; returns the analysis"""
    rows, cols = seg.params.rows, seg.params.cols
    q = ref_of(proj if proj is not None else S.default_projection(seg.params))
    a = PJ.analyse(pts, q, rows, cols)
    win, pix = seg.projection_maps()
    assert win.shape == (rows, cols) and pix.shape == (len(pts),)
    keep = ~a["excluded"]
    np.testing.assert_array_equal(win[keep], a["winner"][keep])
    np.testing.assert_array_equal(pix[~a["undecided"]], a["pixel_of_point"][~a["undecided"]])
    if not a["undecided"].any():
        assert counts(pr) == (a["points"], a["invalid"], a["out_of_view"], a["occupied_pixels"], a["collisions"])
    assert pr.points == len(pts) == pr.invalid + pr.out_of_view + pr.occupied_pixels + pr.collisions
    assert pr.occupied_pixels == int((win >= 0).sum()) and pr.invalid + pr.out_of_view == int((pix < 0).sum())
    return a


@pytest.fixture(scope="module")
def frame16():
    """the 16 x 256 ray-cast frame (sensor frame), 10 % of its pixels and one 4 x 60 block blanked"""
    f = cast(16, 256)
    assert np.isfinite(f).all()
    return blank(f, 16, 256, (4, 60), 11)


@pytest.fixture(scope="module")
def cloud16(frame16):
    """(the frame's finite points, shuffled; the pixel each came from)"""
    pix = np.flatnonzero(np.isfinite(frame16).all(axis=1))
    order = np.random.default_rng(12).permutation(pix)
    return np.ascontiguousarray(frame16[order]), order


def test_round_trip(frame16, cloud16):
    pts, order = cloud16
    n = len(pts)
    assert 3000 < n < 16 * 256 - 240
    seg = S.Segmentation(0, params(16, 256))
    org = S.Segmentation(0, params(16, 256))
    _, pr = seg.process_cloud(pts, EYE)
    check_maps(seg, pts, pr)
    win, pix = seg.projection_maps()
    want = np.full(16 * 256, -1, np.int32)
    want[order] = np.arange(n)
    np.testing.assert_array_equal(win.ravel(), want)           # every unblanked pixel -> its own point
    np.testing.assert_array_equal(pix, order)                  # and the inverse
    assert (pr.collisions, pr.occupied_pixels, pr.invalid, pr.out_of_view) == (0, n, 0, 0)
    # the staged scan: under the identity pose the fill returns the input bits
    org.process(frame16, EYE)
    np.testing.assert_array_equal(seg.images()[0], org.images()[0])
    np.testing.assert_array_equal(seg.static_cloud([]), org.static_cloud([]))
    # a pose: the fill computes what the organized transform computes (the numpy twin of its operation order)
    _, pr2 = seg.process_cloud(pts, POSE)
    m = POSE
    x, y, z = (frame16[:, k] for k in range(3))
    world = np.stack([(m[r, 0] * x + m[r, 1] * y) + (m[r, 2] * z + m[r, 3]) for r in range(3)], axis=1)
    np.testing.assert_array_equal(seg.static_cloud([]), world[np.isfinite(world).all(axis=1)])
    assert counts(pr2) == counts(pr)
    seg.close()
    org.close()


@pytest.mark.parametrize("rows,cols", [(3, 7), (16, 256)])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4096])
def test_cloud_sizes(cloud16, rows, cols, n):
    pts = np.concatenate([cloud16[0], cloud16[0][::-1]])[:n]
    assert len(pts) == n
    seg = S.Segmentation(0, params(rows, cols, ground_rows=1))
    proj = small_projection() if rows == 3 else None
    r, pr = seg.process_cloud(pts, EYE, projection=proj)
    a = check_maps(seg, pts, pr, proj)
    assert not a["undecided"].any()
    if n == 0:
        assert counts(pr) == (0, 0, 0, 0, 0) and r.range_pixels == 0
        assert (seg.projection_maps()[0] == -1).all() and len(seg.static_cloud([])) == 0
    if rows == 3 and n >= 255:
        assert pr.collisions > 0 and pr.out_of_view > 0      # the beams below -15 degrees leave the image
    seg.close()


def with_hand_points(pts, proj, rows, cols):
    hp = np.stack([p for _, p, _ in PJ.hand_points(proj, rows, cols)])
    return np.concatenate([hp, pts, hp]).astype(np.float32), len(hp)


def test_collisions(cloud16):
    pts, _ = cloud16
    n = len(pts)
    # the coarse image: every pixel occupied, most points lose
    coarse = S.Segmentation(0, params(8, 64))
    _, pr = coarse.process_cloud(pts, EYE)
    check_maps(coarse, pts, pr)
    assert pr.occupied_pixels <= 8 * 64 and pr.collisions == n - pr.occupied_pixels > 2000 and pr.out_of_view == 0
    # the cloud twice: the second copy wins every pixel
    seg = S.Segmentation(0, params(16, 256))
    both = np.concatenate([pts, pts])
    _, pr = seg.process_cloud(both, EYE)
    check_maps(seg, both, pr)
    win, pix = seg.projection_maps()
    assert (win[win >= 0] >= n).all() and pr.collisions == n and pr.occupied_pixels == n
    np.testing.assert_array_equal(pix[:n], pix[n:])
    # the hand points before and after the scan, in three geometries (one with a point exactly between two rows)
    for s, proj in ((seg, None), (coarse, None), (S.Segmentation(0, params(3, 7, ground_rows=1)), small_projection())):
        q = ref_of(proj if proj is not None else S.default_projection(s.params))
        cloud, nh = with_hand_points(pts, q, s.params.rows, s.params.cols)
        _, pr = s.process_cloud(cloud, POSE, projection=proj)
        a = check_maps(s, cloud, pr, proj)
        assert int(a["undecided"].sum()) == (2 if s.params.rows == 3 else 0) and int(a["excluded"].sum()) <= 2
        first = (s.projection_maps(), [im.copy() for im in s.images()], counts(pr))
        _, pr = s.process_cloud(cloud, POSE, projection=proj)
        second = (s.projection_maps(), s.images(), counts(pr))
        for u, v in zip(first[0] + tuple(first[1]), second[0] + tuple(second[1])):     # two runs: the same bits
            assert u.tobytes() == v.tobytes()
        assert first[2] == second[2]
        # the wrap (qc rounds to cols) and the reversed azimuth, on the device as in the restatement
        wq, wp, _ = PJ.wrap_case(q, s.params.rows, s.params.cols)
        for rq in (wq, PJ.Projection(q.elev_top, q.elev_res, q.azim0 + 90.0, -1)):
            dq = S.ProjectionParams(rq.elev_top, rq.elev_res, rq.azim0, rq.azim_sign)
            c2 = np.concatenate([cloud, wp[None]]).astype(np.float32)
            _, pr = s.process_cloud(c2, EYE, projection=dq)
            check_maps(s, c2, pr, dq)
        s.close()


def test_out_of_view_and_invalid(cloud16):
    pts, _ = cloud16
    # half the field of view: an image of half the rows, its top at elev_top / 2, the same resolution
    seg = S.Segmentation(0, params(8, 256))
    full = S.default_projection(params(16, 256))
    half = S.ProjectionParams(full.elev_top_deg / 2, full.elev_res_deg, 0.0, 1)
    bad = np.array([[np.nan, 1, 1], [1, np.inf, 1], [0, 0, 0], [1, 1, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    cloud = np.empty((len(pts) + len(pts) // 3 + 1, 3), np.float32)
    is_bad = np.zeros(len(cloud), bool)
    is_bad[::4] = True                                           # interleaved
    is_bad[np.flatnonzero(is_bad)[(len(cloud) - len(pts)):]] = False
    assert int((~is_bad).sum()) == len(pts)
    cloud[~is_bad] = pts
    cloud[is_bad] = bad[np.arange(int(is_bad.sum())) % len(bad)]
    _, pr = seg.process_cloud(cloud, EYE, projection=half)
    a = check_maps(seg, cloud, pr, half)
    assert not a["undecided"].any()
    _, pix = seg.projection_maps()
    assert pr.invalid == int(is_bad.sum()) and (pix[is_bad] == -1).all()
    assert 0.4 * len(pts) < pr.out_of_view < 0.6 * len(pts)
    np.testing.assert_array_equal(pix < 0, is_bad | ~a["kept"])
    seg.close()


# ---- the same segmentation as the organized entry ---------------------------------------------------
def synth_frame(H, W, sizes, seed):
    """An organized H x W sensor-frame scan whose points lie on their pixels' rays (scene.lidar_dirs, row 0 the
    top beam) at 15 m, so that pixels that touch are one segment: one run of pixels per size, blank pixels
    between the runs (the layout of test_gpu_track.py's synth_scan)."""
    dirs = scene.lidar_dirs(H, W).reshape(H, W, 3)[::-1].reshape(-1, 3)
    xyz = np.full((H * W, 3), np.nan, np.float32)
    row, col, shared = 0, 0, True
    for sz in sizes:
        if not (shared and sz <= W - col):
            row, col = row + 2, 0
        rows_needed = -(-sz // W)
        pix = np.arange(sz) + (row * W + col)
        assert pix[-1] < H * W
        xyz[pix] = (15.0 * dirs[pix]).astype(np.float32)
        if rows_needed == 1 and col + sz < W:
            col, shared = col + sz + 1, True
        else:
            row, col, shared = row + rows_needed - 1, 0, False
    return xyz


def synth_params(H, W):
    return params(H, W, ground_rows=0, valid_point_num=1, min_line_num=0, valid_line_num=0, min_delta_z=-1e7,
                  max_delta_z=1e7, max_distance=100, max_elevation=1e7)


@pytest.fixture(scope="module")
def frame64():
    return blank(cast(64, 2048), 64, 2048, (8, 300), 13)


def seg_inputs(which, frame64):
    if which == "synthetic":
        return synth_params(16, 256), synth_frame(16, 256, SMALL, 5), len(SMALL)
    p = S.yaml_seg_params(rows=64, cols=2048, ang_bottom=22.5, ground_rows=20, win_row0=0, win_row1=63, win_col0=0,
                          win_col1=2047, max_distance=30)
    return p, frame64, None


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("which", ["synthetic", "raycast64"])
def test_same_segmentation_as_organized(frame64, which, mode):
    p, frame, want_segments = seg_inputs(which, frame64)
    n = p.rows * p.cols
    finite = np.isfinite(frame).all(axis=1)
    pts = np.ascontiguousarray(frame[finite])                      # row-major order
    resid = np.random.default_rng(3).random(n).astype(np.float32)
    org = S.Segmentation(0, p, labelling=mode)
    seg = S.Segmentation(0, p, labelling=mode)
    ra = org.process(frame, EYE, resid)
    rb, pr = seg.process_cloud(pts, EYE, resid)
    win, pix = seg.projection_maps()
    np.testing.assert_array_equal(pix, np.flatnonzero(finite))
    assert counts(pr) == (len(pts), 0, 0, len(pts), 0)
    key = lambda r: (r.segments, r.ground_pixels, r.range_pixels, r.rejected_pixels)
    assert key(ra) == key(rb) and ra.segments >= 1
    if want_segments is not None:
        assert ra.segments == want_segments
    for a, b in zip(org.images(), seg.images()):
        np.testing.assert_array_equal(a, b)
    assert org.avg_residuals().tobytes() == seg.avg_residuals().tobytes()
    oa, ob = org.objects(10.0), seg.objects(10.0)
    assert len(oa) >= 1 and oa.tobytes() == ob.tobytes()
    drop = list(range(1, ra.segments + 1, 2))
    for crop, leaf in ((0.0, 0.0), (1.0, 0.25)):
        ca, cb = org.static_cloud(drop, (0, 0, 0), crop, leaf), seg.static_cloud(drop, (0, 0, 0), crop, leaf)
        assert len(ca) > 0 and ca.tobytes() == cb.tobytes()
    np.testing.assert_array_equal(org.ground_indices(), seg.ground_indices())
    for a, b in zip(org.label_indices()[1:], seg.label_indices()[1:]):
        np.testing.assert_array_equal(a, b)
    org.close()
    seg.close()


def test_point_classes():
    frame = synth_frame(16, 256, SMALL, 5)
    finite = np.isfinite(frame).all(axis=1)
    one = frame[finite]
    bad = np.array([[np.nan, 0, 0], [0, 0, 0], [0, 0, 1]], np.float32)     # invalid, invalid, out of view
    cloud = np.concatenate([one, bad, one]).astype(np.float32)              # the first copy loses every pixel
    seg = S.Segmentation(0, synth_params(16, 256), labelling="device")
    r, pr = seg.process_cloud(cloud, EYE)
    assert r.segments == len(SMALL) and pr.collisions == len(one) and (pr.invalid, pr.out_of_view) == (2, 1)
    with pytest.raises(P.GicpError):                                         # not classified yet
        seg.point_classes()
    ids = list(range(1, r.segments + 1))
    seg.tracks_sync([(100 + l, l) for l in ids])
    seg.classify([(100 + l, l % 3) for l in ids])
    img = seg.class_image()
    win, pix = seg.projection_maps()
    pc = seg.point_classes()
    want = np.where(pix >= 0, img.ravel()[np.maximum(pix, 0)], 0).astype(np.uint8)
    np.testing.assert_array_equal(pc, want)
    assert (pc[len(one):len(one) + 3] == 0).all()
    np.testing.assert_array_equal(pc[:len(one)], pc[len(one) + 3:])         # a loser gets its pixel's byte
    for bits in (S.CLS_DYNAMIC, S.CLS_STATIC, S.CLS_UNDEFINED):
        assert (pc & bits).any()
    np.testing.assert_array_equal(seg.point_class_indices(S.CLS_DYNAMIC), np.flatnonzero(pc & S.CLS_DYNAMIC))
    np.testing.assert_array_equal(seg.point_class_indices(S.CLS_NON_STATIC, S.CLS_DYNAMIC),
                                  np.flatnonzero(((pc & S.CLS_NON_STATIC) != 0) & ((pc & S.CLS_DYNAMIC) == 0)))
    # the winners' points among them are exactly class_indices' pixels
    dyn_pix = seg.class_indices(S.CLS_DYNAMIC)
    np.testing.assert_array_equal(np.sort(win.ravel()[dyn_pix]),
                                  np.intersect1d(seg.point_class_indices(S.CLS_DYNAMIC), win.ravel()[win.ravel() >= 0]))
    # a capacity below n: the first cap bytes
    n = C.c_size_t()
    part = np.full(10, 255, np.uint8)
    assert S._lib().ddlo_seg_point_classes(seg.h, P._ptr(part), 10, C.byref(n)) == 0 and n.value == len(cloud)
    np.testing.assert_array_equal(part, pc[:10])
    seg.close()


def raw_process_cloud(seg, pts, proj, stride=12, T=EYE):
    a = np.ascontiguousarray(pts, np.float32)
    Tm = np.ascontiguousarray(T, np.float32).reshape(16)
    return S._lib().ddlo_seg_process_cloud(seg.h, P._ptr(a), len(a), stride, P._ptr(Tm),
                                           C.byref(proj) if proj is not None else None, None, None, None)


def test_errors(frame16, cloud16):
    pts, _ = cloud16
    L = S._lib()
    seg = S.Segmentation(0, params(16, 256))
    n = C.c_size_t()
    # before any projected scan
    assert L.ddlo_seg_projection_maps(seg.h, None, None, 0, C.byref(n)) == 1
    assert L.ddlo_seg_point_classes(seg.h, None, 0, C.byref(n)) == 1
    seg.process(frame16, EYE)
    assert L.ddlo_seg_projection_maps(seg.h, None, None, 0, C.byref(n)) == 1
    _, pr = seg.process_cloud(pts[:1000], EYE)
    maps = seg.projection_maps()
    images = [im.copy() for im in seg.images()]
    seg.classify([])
    classes = seg.point_classes()
    # rejected calls: GICP_EINVAL, and the scan, its images, maps and classes stay
    d = S.default_projection(seg.params)
    inf, nan = float("inf"), float("nan")
    bad = [S.ProjectionParams(d.elev_top_deg, 0.0, 0.0, 1), S.ProjectionParams(d.elev_top_deg, -3.0, 0.0, 1),
           S.ProjectionParams(d.elev_top_deg, nan, 0.0, 1), S.ProjectionParams(d.elev_top_deg, inf, 0.0, 1),
           S.ProjectionParams(inf, 3.0, 0.0, 1), S.ProjectionParams(nan, 3.0, 0.0, 1),
           S.ProjectionParams(d.elev_top_deg, 3.0, nan, 1), S.ProjectionParams(d.elev_top_deg, 3.0, -inf, 1),
           S.ProjectionParams(d.elev_top_deg, 3.0, 0.0, 0), S.ProjectionParams(d.elev_top_deg, 3.0, 0.0, 2),
           S.ProjectionParams(d.elev_top_deg, 3.0, 0.0, -2)]
    for q in bad:
        assert raw_process_cloud(seg, pts, q) == 1, (q.elev_top_deg, q.elev_res_deg, q.azim0_deg, q.azim_sign)
    for stride in (0, 8, 14):
        assert raw_process_cloud(seg, pts, None, stride=stride) == 1
    Tm = np.ascontiguousarray(EYE).reshape(16)
    assert L.ddlo_seg_process_cloud(seg.h, None, 5, 12, P._ptr(Tm), None, None, None, None) == 1     # no points
    assert L.ddlo_seg_process_cloud(seg.h, P._ptr(pts), len(pts), 12, None, None, None, None, None) == 1   # no pose
    assert L.ddlo_seg_process_cloud(seg.h, P._ptr(pts), (2 ** 31 - 1) // 2 + 1, 12, P._ptr(Tm), None, None, None,
                                    None) == 1
    assert L.ddlo_seg_default_projection(None, C.byref(d)) == 1
    with pytest.raises(P.GicpError):
        seg.process_cloud(pts, EYE, projection=bad[0])
    after = seg.projection_maps()
    for u, v in zip(maps + tuple(images) + (classes,), after + seg.images() + (seg.point_classes(),)):
        assert u.tobytes() == v.tobytes()
    assert len(after[1]) == 1000
    # a stride above 12: the fourth float of every point is skipped
    wide = np.concatenate([pts[:1000], np.full((1000, 1), np.nan, np.float32)], axis=1)
    _, pr2 = seg.process_cloud(wide, EYE)
    assert counts(pr2) == counts(pr)
    for u, v in zip(maps, seg.projection_maps()):
        assert u.tobytes() == v.tobytes()
    with pytest.raises(P.GicpError):          # a new scan: not classified
        seg.point_classes()
    # a later organized scan takes the maps away
    seg.classify([])
    seg.point_classes()
    seg.process(frame16, EYE)
    assert L.ddlo_seg_projection_maps(seg.h, None, None, 0, C.byref(n)) == 1
    seg.classify([])
    assert L.ddlo_seg_point_classes(seg.h, None, 0, C.byref(n)) == 1
    with pytest.raises(P.GicpError):
        seg.projection_maps()
    seg.close()
