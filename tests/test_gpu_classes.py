"""The per-pixel classes of a frame (include/ddlo_seg_classes.h,
csrc/seg_classes.hip): class image, counts, index sets and the four clouds.

Every comparison is array_equal against a numpy restatement built from getters
that existed before the classes did: ddlo_seg_track_indices for the tracks'
lists, ddlo_seg_ground_indices for the ground set, and the scan handed in.
The synthetic scans follow tests/test_gpu_track.py (every point 15 m from the
sensor: pixels that touch are one segment, blank pixels keep segments apart).
"""
import ctypes as C
import math

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import scene
from dynamic_direct_lidar_odometry_amd import segmentation as S

pytestmark = pytest.mark.gpu

W = 256
SMALL = [1, 63, 64, 65, 255, 256, 257]
EYE = np.eye(4, dtype=np.float32)
BITS = [S.CLS_VALID, S.CLS_GROUND, S.CLS_UNDEFINED, S.CLS_STATIC, S.CLS_DYNAMIC]
SETS = BITS + [S.CLS_NON_STATIC]


def synth_scan(H, sizes, seed, width=W):
    """tests/test_gpu_track.py's recipe: (xyz (H*width, 3) float32 with NaN blanks, [pixel index arrays])."""
    rng = np.random.default_rng(seed)
    xyz = np.full((H * width, 3), np.nan, np.float32)
    row, col, shared = 0, 0, True
    segs = []
    for sz in sizes:
        if not (shared and sz <= width - col):
            row, col = row + 2, 0                  # a blank row above the new band
        rows_needed = -(-sz // width)
        pix = np.arange(sz) + (row * width + col)
        assert pix[-1] < H * width, "the image is too small for these sizes"
        d = rng.normal(size=(sz, 3))
        xyz[pix] = (15.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        segs.append(pix.astype(np.int32))
        if rows_needed == 1 and col + sz < width:
            col, shared = col + sz + 1, True       # one blank pixel, then the row is shared
        else:
            row, col, shared = row + rows_needed - 1, 0, False
    return xyz, segs


def synth_params(H, width=W):
    return S.default_seg_params(rows=H, cols=width, ground_rows=0, minimum_range=0, valid_point_num=1, min_line_num=0,
                                valid_line_num=0, min_delta_z=-1e7, max_delta_z=1e7, max_distance=100,
                                max_elevation=1e7, win_row0=0, win_row1=H - 1, win_col0=0, win_col1=width - 1)


def seg_of(lists, pix):
    for l in range(1, len(lists)):
        if len(lists[l]) == len(pix) and np.array_equal(lists[l], pix):
            return l
    raise AssertionError("the labelling did not produce the planned segment")


def restate(seg, xyz, tracks):
    """The class image from the getters that exist without it: (image, finite mask)."""
    xyz = np.asarray(xyz, np.float32)[:, :3]
    finite = np.isfinite(xyz).all(axis=1)
    img = np.zeros(len(xyz), np.uint8)
    img[finite] |= S.CLS_VALID
    img[seg.ground_indices()] |= S.CLS_GROUND
    for t, st in tracks:
        img[seg.track_indices(t)] |= S.CLS_UNDEFINED << st
    return img, finite


def restated_clouds(xyz, img):
    xyz = np.asarray(xyz, np.float32)[:, :3]
    valid = (img & S.CLS_VALID) != 0
    ns = (img & S.CLS_NON_STATIC) != 0
    return [xyz[valid & ((img & S.CLS_GROUND) != 0)], xyz[valid & ns], xyz[valid & ((img & S.CLS_DYNAMIC) != 0)],
            xyz[valid & ~ns]]


def check(seg, xyz, tracks):
    """classify(tracks) against the restatement: image, counts, six index sets, four clouds.  Returns the image."""
    want, finite = restate(seg, xyz, tracks)
    counts = seg.classify(tracks)
    img = seg.class_image()
    assert img.shape == (seg.params.rows, seg.params.cols) and img.dtype == np.uint8
    img = img.reshape(-1)
    np.testing.assert_array_equal(img, want)
    ns = (want & S.CLS_NON_STATIC) != 0
    got = [counts.valid, counts.ground, counts.undefined, counts.static_tracks, counts.dynamic, counts.non_static,
           counts.static_points]
    print("counts", got)
    assert got == [int(((want & b) != 0).sum()) for b in BITS] + [int(ns.sum()), int((finite & ~ns).sum())]
    assert counts.reserved == 0
    for any_bits in SETS:
        ids = seg.class_indices(any_bits)
        assert ids.dtype == np.int32
        np.testing.assert_array_equal(ids, np.flatnonzero(want & any_bits))
    np.testing.assert_array_equal(seg.class_indices(S.CLS_VALID, S.CLS_NON_STATIC), np.flatnonzero(finite & ~ns))
    clouds = seg.frame_clouds()
    for got_c, want_c in zip(clouds, restated_clouds(xyz, want)):
        assert got_c.dtype == np.float32 and got_c.shape == want_c.shape
        np.testing.assert_array_equal(got_c, want_c)
        assert np.isfinite(got_c).all()
    return img


def raw_classify(seg, ids, statuses):
    a, b = np.array(ids, np.int32), np.array(statuses, np.int32)
    return S._lib().ddlo_seg_classify(seg.h, P._ptr(a) if len(a) else None, P._ptr(b) if len(b) else None, len(a),
                                      None)


def touching_blobs():
    """3 x 7: blob A (15 m) on pixels 0-2 and 7-9, blob B (5 m) on 10-13 and 17-20; they touch between pixels 9
    and 10, and the range step keeps them two segments (atan2(5 sin a, 15 - 5 cos a) is 18 degrees at a = 360 / 7)."""
    rng = np.random.default_rng(7)
    xyz = np.full((21, 3), np.nan, np.float32)
    a = np.array([0, 1, 2, 7, 8, 9], np.int32)
    b = np.array([10, 11, 12, 13, 17, 18, 19, 20], np.int32)
    for pix, r in ((a, 15.0), (b, 5.0)):
        d = rng.normal(size=(len(pix), 3))
        xyz[pix] = (r * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return xyz, a, b


@pytest.mark.parametrize("mode", ["host", "device"])
def test_3x7_padding(mode):
    """21 pixels: the image's last word is one pixel and three bytes of padding."""
    xyz, a, b = touching_blobs()
    seg = S.Segmentation(0, synth_params(3, 7), labelling=mode)
    assert seg.process(xyz, EYE).segments == 2
    lists = seg.label_indices()
    seg.tracks_sync([(5, seg_of(lists, a)), (9, seg_of(lists, b))])
    tracks = [(5, 2), (9, 1)]                          # A DYNAMIC, B STATIC
    img = check(seg, xyz, tracks)
    assert img[20] == S.CLS_VALID | S.CLS_STATIC and img[9] == S.CLS_VALID | S.CLS_DYNAMIC and img[14] == 0
    for any_bits in SETS + [0xff]:
        ids = seg.class_indices(any_bits)
        assert ids.size == 0 or (0 <= ids.min() and ids.max() < 21)
    np.testing.assert_array_equal(seg.class_indices(0xff), np.flatnonzero(np.isfinite(xyz).all(axis=1)))
    c = seg.classify(tracks)
    assert (c.valid, c.static_tracks, c.dynamic, c.non_static, c.static_points) == (14, 8, 6, 6, 8)
    seg.close()


def first_scan(seg, H=16, sizes=SMALL, seed=1):
    """scan 0: every segment becomes track 100 + k; returns (xyz, planned pixel lists)."""
    xyz, planned = synth_scan(H, sizes, seed)
    assert seg.process(xyz, EYE).segments == len(sizes)
    lists = seg.label_indices()
    seg.tracks_sync([(100 + k, seg_of(lists, p)) for k, p in enumerate(planned)])
    return xyz, planned


@pytest.mark.parametrize("mode", ["host", "device"])
def test_16x256_every_segment_size(mode):
    seg = S.Segmentation(0, synth_params(16), labelling=mode)
    xyz, planned = first_scan(seg)
    tracks = [(100 + k, k % 3) for k in range(len(SMALL))]
    img = check(seg, xyz, tracks)
    for k, p in enumerate(planned):
        assert (img[p] == (S.CLS_VALID | (S.CLS_UNDEFINED << (k % 3)))).all()
    # two classifications of the same state: the same bytes
    again = seg.classify(tracks)
    assert seg.class_image().tobytes() == img.tobytes()
    assert [a.tobytes() for a in seg.frame_clouds()] == [a.tobytes() for a in restated_clouds(xyz, img)]
    assert again.non_static == sum(SMALL[k] for k in range(len(SMALL)) if k % 3 != 1)
    # the order of the tracks does not matter
    seg.classify(tracks[::-1])
    assert seg.class_image().tobytes() == img.tobytes()
    seg.close()


@pytest.mark.parametrize("mode", ["host", "device"])
def test_second_scan_stale_lists(mode):
    seg = S.Segmentation(0, synth_params(16), labelling=mode)
    xyz0, planned0 = first_scan(seg)
    xyz1, planned1 = synth_scan(16, SMALL[::-1], 2)
    assert seg.process(xyz1, EYE).segments == len(SMALL)
    # the class image belongs to a scan: none yet for this one
    with pytest.raises(P.GicpError):
        seg.class_image()
    lists1 = seg.label_indices()
    big = int(np.argmax([len(p) for p in planned1]))
    seg.tracks_sync([(200, seg_of(lists1, planned1[big]))])
    # the stale lists of scan 0 (statuses cycling; track 104, whose 255 pixels 512 .. 766 lie under this scan's
    # largest segment, UNDEFINED) and the current DYNAMIC track 200
    tracks = [(100 + k, (k + 2) % 3) for k in range(len(SMALL))] + [(200, 2)]
    assert dict(tracks)[104] == 0 and np.isin(planned0[4], planned1[big]).all()
    img = check(seg, xyz1, tracks)
    both = ((img & S.CLS_UNDEFINED) != 0) & ((img & S.CLS_DYNAMIC) != 0)
    assert both.any(), "no pixel is in a stale UNDEFINED list and the current DYNAMIC one"
    assert np.isin(np.flatnonzero(both), planned1[big]).all()       # (the stale lists are disjoint)
    # a stale pixel that is blank in this scan: in its index set, in no cloud
    blank = ~np.isfinite(xyz1).all(axis=1)
    stale = np.concatenate(planned0)
    gone = stale[blank[stale]]
    assert gone.size, "every stale pixel has a point in the new scan"
    assert ((img[gone] & S.CLS_VALID) == 0).all() and ((img[gone] & 0x1c) != 0).all()
    for any_bits in (S.CLS_UNDEFINED, S.CLS_STATIC, S.CLS_DYNAMIC):
        mine = gone[(img[gone] & any_bits) != 0]
        assert np.isin(mine, seg.class_indices(any_bits)).all()
    clouds = seg.frame_clouds()
    n_valid_ns = int((((img & S.CLS_VALID) != 0) & ((img & S.CLS_NON_STATIC) != 0)).sum())
    assert len(clouds.non_static) == n_valid_ns < int(((img & S.CLS_NON_STATIC) != 0).sum())
    # the static-cloud calls write NaN over a packed copy, never over the scan the classes read
    ns_tracks = [t for t, st in tracks if st != 1]
    removed = seg.static_cloud_tracks(ns_tracks)
    np.testing.assert_array_equal(removed, clouds.static_points)   # (no crop, no voxel filter: the same cloud)
    np.testing.assert_array_equal(seg.class_image().reshape(-1), img)
    for a, b in zip(seg.frame_clouds(), clouds):
        np.testing.assert_array_equal(a, b)
    img2 = check(seg, xyz1, tracks)
    assert img2.tobytes() == img.tobytes()
    for a, b in zip(seg.frame_clouds(), clouds):
        assert a.tobytes() == b.tobytes()
    # a released track: GICP_EINVAL, the previous image stays
    seg.tracks_sync(dead_ids=[101])
    assert raw_classify(seg, [100, 101], [0, 1]) == 1
    assert raw_classify(seg, [101], [1]) == 1
    np.testing.assert_array_equal(seg.class_image().reshape(-1), img)
    for a, b in zip(seg.frame_clouds(), clouds):
        np.testing.assert_array_equal(a, b)
    check(seg, xyz1, [tr for tr in tracks if tr[0] != 101])
    seg.close()


@pytest.mark.parametrize("mode", ["host", "device"])
def test_degenerate_cases(mode):
    fresh = S.Segmentation(0, synth_params(16), labelling=mode)
    assert raw_classify(fresh, [], []) == 1            # nothing processed
    n = C.c_size_t()
    assert S._lib().ddlo_seg_class_indices(fresh.h, 1, 0, None, 0, C.byref(n)) == 1
    with pytest.raises(P.GicpError):
        fresh.frame_clouds()
    fresh.close()
    seg = S.Segmentation(0, synth_params(16), labelling=mode)
    xyz, planned = first_scan(seg)
    # n == 0: VALID (and GROUND) only
    img0 = check(seg, xyz, [])
    assert set(np.unique(img0)) == {0, S.CLS_VALID}
    # UNDEFINED and STATIC tracks only: the dynamic cloud is empty between two that are not
    tracks = [(100 + k, k % 2) for k in range(len(SMALL))]
    img = check(seg, xyz, tracks)
    clouds = seg.frame_clouds()
    assert len(clouds.non_static) > 0 and len(clouds.dynamic) == 0 and len(clouds.static_points) > 0
    assert clouds.dynamic.shape == (0, 3) and seg.class_indices(S.CLS_DYNAMIC).shape == (0,)
    # invalid calls change nothing
    assert raw_classify(seg, [100, 101], [0, 3]) == 1
    assert raw_classify(seg, [100, 101], [-1, 0]) == 1
    assert raw_classify(seg, [100, 101, 100], [0, 1, 0]) == 1
    assert raw_classify(seg, [100, 999], [0, 1]) == 1
    assert S._lib().ddlo_seg_classify(seg.h, None, None, 2, None) == 1
    assert S._lib().ddlo_seg_class_indices(seg.h, 0x100, 0, None, 0, C.byref(n)) == 1
    np.testing.assert_array_equal(seg.class_image().reshape(-1), img)
    for a, b in zip(seg.frame_clouds(), clouds):
        np.testing.assert_array_equal(a, b)
    # a capacity that is too small: the count for indices (the first cap come out), an error for a cloud
    two = np.full(2, -1, np.int32)
    assert S._lib().ddlo_seg_class_indices(seg.h, S.CLS_VALID, 0, P._ptr(two), 2, C.byref(n)) == 0
    assert n.value == sum(SMALL) and two.tolist() == np.flatnonzero(img & S.CLS_VALID)[:2].tolist()
    o = S._FrameCloudsOut()
    buf = np.zeros((1, 3), np.float32)
    o.static_points.xyz, o.static_points.cap = buf.ctypes.data, 1
    assert S._lib().ddlo_seg_frame_clouds(seg.h, C.byref(o)) == 1
    # every pixel in one DYNAMIC track
    rng = np.random.default_rng(3)
    d = rng.normal(size=(16 * W, 3))
    full = (15.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    assert seg.process(full, EYE).segments == 1
    seg.tracks_sync([(300, 1)], dead_ids=[100 + k for k in range(len(SMALL))])
    img = check(seg, full, [(300, 2)])
    assert (img == (S.CLS_VALID | S.CLS_DYNAMIC)).all()
    clouds = seg.frame_clouds()
    assert len(clouds.dynamic) == 16 * W and len(clouds.static_points) == 0 and len(clouds.ground) == 0
    seg.close()


def organized_world_scan(frame: int, rows, cols):
    """tests/test_gpu_label_device.py's frames: a ray-cast scan moved to the world frame."""
    sc = scene.make_scene(1005, moving=True)
    pose = scene.make_pose([0.3 * frame, -0.2 * frame, scene.SENSOR_Z], (0.0, 0.0, math.radians(7.0 * frame)))
    pts = scene.raycast(sc, pose, rows, cols, 1005 + frame, t=0.1 * frame, organized=True)
    bad = ~np.isfinite(pts).all(axis=1)
    xyz_t = scene.transform(np.nan_to_num(pts, nan=0.0), pose).astype(np.float32)
    xyz_t[bad] = np.nan
    return xyz_t, pose.astype(np.float32)


@pytest.mark.parametrize("mode", ["host", "device"])
def test_raycast_64x2048_ground(mode):
    xyz, T = organized_world_scan(1, 64, 2048)
    p = S.yaml_seg_params(rows=64, cols=2048, ground_rows=20, win_row0=0, win_row1=63, win_col0=0, win_col1=2047,
                          max_distance=30)
    seg = S.Segmentation(0, p, labelling=mode)
    r = seg.process(xyz, T)
    ground = np.sort(seg.ground_indices())
    assert ground.size >= 1 and r.segments >= 1
    seg.tracks_sync([(10 + l, l) for l in range(1, r.segments + 1)])
    tracks = [(10 + l, l % 3) for l in range(1, r.segments + 1)]
    img = check(seg, xyz, tracks)
    np.testing.assert_array_equal(np.flatnonzero(img & S.CLS_GROUND), ground)
    np.testing.assert_array_equal(seg.class_indices(S.CLS_GROUND), ground)
    g = xyz[ground]
    np.testing.assert_array_equal(seg.frame_clouds().ground, g[np.isfinite(g).all(axis=1)])
    # the ground image marks the row above the tested ones too (ground_mat_ == 1 there is not in the set)
    assert ground.min() >= (64 - 20) * 2048
    seg.close()
