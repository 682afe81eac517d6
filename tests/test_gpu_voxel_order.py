"""GPU tests of the PCL summation order of the device voxel filter (DDLO_VOXEL_ORDER_PCL:
ddlo_preprocess_ordered, ddlo_seg_set_voxel_order, ddlo_odom_set_voxel_order): the centroids
equal the oracle's pcl::VoxelGrid restatement (oracle.voxel_grid, which calls std::sort) bit for
bit, compared with assert_array_equal.  The crop box is restated by tests/preprocess_ref.py
(crop_keep, exact) and the oracle filters its output.

Not vacuous: on the clouds named in test_orders_differ the oracle's centroids differ from the
input-order ones (preprocess_ref.voxel_grid), so a mode that is silently ignored cannot pass."""
import ctypes as C

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import scene
from dynamic_direct_lidar_odometry_amd import segmentation as S
from oracle import oracle as O
import objects_ref as R
import pcl_order_ref as PO
import preprocess_ref as PR

pytestmark = pytest.mark.gpu

PCL, INPUT = OD.VOXEL_ORDER_PCL, OD.VOXEL_ORDER_INPUT


def oracle_filter(pts, crop, leaf):
    """The oracle's voxel grid over the crop restatement's output; None on a grid overflow."""
    kept = PR.crop_keep(pts, crop) if crop > 0 else pts
    x = kept[PR.finite_mask(kept)]
    if len(x) and PR.voxel_keys(x, leaf)[1]:
        return None
    return O.voxel_grid(kept, leaf)


def check(pts, crop, leaf):
    got = OD.preprocess(pts, crop, leaf, order=PCL)
    ref = oracle_filter(pts, crop, leaf)
    assert ref is not None
    np.testing.assert_array_equal(got, ref)
    return ref


@pytest.fixture(scope="module")
def scan():
    """Frame 1 of the 64 x 2048 sequence: with crop 1.0 and leaf 0.1 its sort reaches the depth limit of 34
    with one 29-element segment left (test_realistic_scan asserts the heap sort)."""
    return scene.odometry_sequence(64, 2048, 3, cfg_id=7)[0][1]


@pytest.mark.parametrize("crop", (0.0, 1.0))
@pytest.mark.parametrize("name", sorted(PR.edge_clouds()))
def test_edge_clouds(name, crop):
    pts = PR.edge_clouds()[name]
    for leaf in PR.LEAVES:
        check(pts, crop, leaf)


@pytest.mark.parametrize("pattern", sorted(PR.nonfinite_patterns(8)))
def test_nonfinite_points(pattern):
    """The dropped points are compacted away before the sort: its mid points depend on segment lengths."""
    base = PR.sites()
    idx = PR.nonfinite_patterns(len(base))[pattern]
    for value in (np.nan, np.inf):
        pts = PR.with_nonfinite(base, idx, value)
        for leaf in (0.1, 0.3):
            check(pts, 0.0, leaf)
            check(pts, 1.0, leaf)


def test_line_out_and_back():
    pts = PO.line_cloud()
    for leaf in (0.1, 0.3):
        ref = check(pts, 0.0, leaf)
        _, st = OD.sort_order(PR.voxel_keys(pts, leaf)[0])
        assert st.heap_segments > 0, leaf        # the depth limit is reached
        differ = int((ref != PR.voxel_grid(pts, leaf)[0]).any(axis=1).sum())
        print(f"line, leaf {leaf}: {st.heap_segments} heap-sorted segments (longest {st.heap_longest}), "
              f"{differ} of {len(ref)} centroids differ from input order")
        assert differ > 0


def test_single_large_voxel():
    pts = PR.single_voxel(n=5000)
    for leaf in (0.1, 0.3):
        assert len(check(pts, 0.0, leaf)) == 1


@pytest.mark.parametrize("leaf", (0.1, 0.25))
def test_realistic_scan(scan, leaf):
    ref = check(scan, 1.0, leaf)
    if leaf == 0.1:
        x = scan[PR.crop_mask(scan, 1.0)]
        assert OD.sort_order(PR.voxel_keys(x, leaf)[0])[1].heap_segments >= 1
    differ = int((ref != PR.voxel_grid(scan, leaf, 1.0)[0]).any(axis=1).sum())
    print(f"64 x 2048 scan, leaf {leaf}: {differ} of {len(ref)} centroids ({100.0 * differ / len(ref):.1f} %) "
          f"differ from input order")
    assert differ > 0
    np.testing.assert_array_equal(OD.preprocess(scan, 1.0, leaf), PR.voxel_grid(scan, leaf, 1.0)[0])


def test_overflow_cases():
    """Around the grid overflow both orders behave alike: the cloud passes unfiltered (cropped)."""
    for half_z, leaf in ((PR.OVERFLOW_HALF_Z, 0.05), (PR.OVER_HALF_Z, 0.05)):
        w = PR.wide(half_z)
        assert PR.voxel_grid(w, leaf) is None
        for crop in (0.0, 1.0):
            got = OD.preprocess(w, crop, leaf, order=PCL)
            np.testing.assert_array_equal(got, OD.preprocess(w, crop, leaf))
            np.testing.assert_array_equal(got, PR.preprocess(w, crop, leaf))
    check(PR.wide(PR.OVERFLOW_HALF_Z), 0.0, 0.1)
    check(PR.wide(PR.UNDER_HALF_Z), 0.0, 0.05)
    check(PR.wide(PR.UNDER_HALF_Z), 1.0, 0.05)


def test_orders_differ(scan):
    """The oracle's centroids against the input-order restatement's, on the CPU."""
    cases = [("sites", PR.sites(), 0.1), ("sites", PR.sites(), 0.3), ("lattice", PR.lattice(), 0.3),
             ("line", PO.line_cloud(), 0.1)]
    for name, pts, leaf in cases:
        ref = O.voxel_grid(pts, leaf)
        differ = int((ref != PR.voxel_grid(pts, leaf)[0]).any(axis=1).sum())
        print(f"{name}, leaf {leaf}: {differ} of {len(ref)} centroids differ between the orders")
        assert differ > 0, (name, leaf)
    for leaf in (0.1, 0.25):
        kept = PR.crop_keep(scan, 1.0)
        ref = O.voxel_grid(kept, leaf)
        differ = int((ref != PR.voxel_grid(kept, leaf)[0]).any(axis=1).sum())
        print(f"scan, leaf {leaf}: {differ} of {len(ref)} centroids differ between the orders")
        assert differ > 0, leaf


def test_default_unchanged(scan):
    for pts, crop, leaf in ((PR.sites(), 0.0, 0.1), (PR.lattice(), 1.0, 0.3), (scan, 1.0, 0.1),
                            (PR.with_nonfinite(PR.sites(), PR.nonfinite_patterns(12000)["every7th"]), 0.0, 0.1)):
        a = OD.preprocess(pts, crop, leaf)
        b = OD.preprocess(pts, crop, leaf, order=INPUT)
        assert a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes()
        n = C.c_size_t()
        x = np.ascontiguousarray(pts, np.float32)
        out = np.zeros_like(x)
        assert OD._lib().ddlo_preprocess_ordered(0, P._ptr(x), len(x), 12, crop, leaf, INPUT, P._ptr(out), len(out),
                                                 C.byref(n)) == 0
        assert out[:n.value].view(np.uint32).tobytes() == a.view(np.uint32).tobytes()
        np.testing.assert_array_equal(a, PR.preprocess(pts, crop, leaf))


def test_static_cloud():
    import test_gpu_objects as TO
    _, xyz_t, T = TO.organized_scan(1)
    seg = S.Segmentation(0, TO.seg_params())
    res = seg.process(xyz_t, T, TO.residual_for(1))
    _, _, label = seg.images()
    ids = list(range(1, res.segments + 1))
    centre = T[:3, 3]
    assert seg.voxel_order == INPUT
    before = seg.static_cloud([], centre, crop_size=1.0, leaf=0.1)
    seg.set_voxel_order(PCL)
    assert seg.voxel_order == PCL
    differs = 0
    for remove in ([], [ids[len(ids) // 2]], ids):
        got = seg.static_cloud(remove, centre, crop_size=1.0, leaf=0.1)
        ref = O.voxel_grid(R.static_cloud(xyz_t, label, remove, centre, 1.0, 0.0), 0.1)
        np.testing.assert_array_equal(got, ref)
        if not remove:
            differs = int((got != before).any(axis=1).sum())
    print(f"static cloud: {differs} of {len(before)} centroids differ between the orders")
    assert differs > 0
    seg.set_voxel_order(INPUT)
    after = seg.static_cloud([], centre, crop_size=1.0, leaf=0.1)
    assert after.tobytes() == before.tobytes()


def test_setter_errors():
    L = OD._lib()
    S._lib()
    od = OD.Odometry(0, OD.default_odom_params())
    import test_gpu_objects as TO
    seg = S.Segmentation(0, TO.seg_params())
    m = C.c_int(-1)
    for h, setter, getter in ((od.h, L.ddlo_odom_set_voxel_order, L.ddlo_odom_get_voxel_order),
                              (seg.h, L.ddlo_seg_set_voxel_order, L.ddlo_seg_get_voxel_order)):
        assert getter(h, C.byref(m)) == 0 and m.value == INPUT
        for bad in (-1, 2, 99):
            assert setter(h, bad) == 1                    # GICP_EINVAL
        assert getter(h, C.byref(m)) == 0 and m.value == INPUT
        assert setter(h, PCL) == 0 and getter(h, C.byref(m)) == 0 and m.value == PCL
        assert setter(h, INPUT) == 0 and getter(h, C.byref(m)) == 0 and m.value == INPUT
        assert setter(None, PCL) == 1 and getter(None, C.byref(m)) == 1 and getter(h, None) == 1
    od.set_voxel_order(PCL)
    assert od.voxel_order == PCL
    x = PR.sites()
    out = np.zeros_like(x)
    n = C.c_size_t()
    assert L.ddlo_preprocess_ordered(0, P._ptr(x), len(x), 12, 0.0, 0.1, 2, P._ptr(out), len(out), C.byref(n)) == 1
    od.close()
