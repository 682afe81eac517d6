"""The odometry chain with the voxel filters ON, bit for bit: with DDLO_VOXEL_ORDER_PCL the one
input that differed between the device chain and the oracle chain (the voxel filter's summation
order, tests/test_gpu_odom_long.py) is gone, so 40 frames of the 64 x 2048 loop with the yaml
parameters agree exactly: every decision, every pose (max |dT| == 0) and every keyframe cloud.
The same chain in the default order is run once to show that the comparison can fail: there at
least one keyframe cloud is not bit-identical to the oracle's.

run_chain (test_gpu_odom_long) builds both drivers itself; the two classes it builds are wrapped
here to set the order on the device driver and to keep both sides' keyframe clouds."""
import numpy as np
import pytest

from dynamic_direct_lidar_odometry_amd import odometry as OD
from dynamic_direct_lidar_odometry_amd import scene
from oracle import odom_ref as R
import test_gpu_odom_long as LONG

pytestmark = pytest.mark.gpu

FRAMES = 40   # yields >= 2 keyframes (asserted below)


@pytest.fixture(scope="module")
def frames():
    return scene.loop_sequence(64, 2048, 0, FRAMES, device=0)[0]


def chain(frames, order, monkeypatch, pose_tol):
    kept = {}

    class Device(OD.Odometry):
        def __init__(self, device, params):
            super().__init__(device, params)
            self.set_voxel_order(order)
            assert self.voxel_order == order

        def process(self, points):
            r = super().process(points)
            if r.status == OD.TRACKED:
                kept["nk"] = int(r.num_keyframes)
            return r

        def close(self):
            if self.h and "gpu" not in kept:
                kept["gpu"] = [self.keyframe_points(k) for k in range(kept.get("nk", 0))]
            super().close()

    class Oracle(R.OdomRef):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            kept["ref"] = self

    monkeypatch.setattr(LONG.OD, "Odometry", Device)
    monkeypatch.setattr(LONG.R, "OdomRef", Oracle)
    stats, nk = LONG.run_chain(frames, OD.default_odom_params(), pose_tol=pose_tol)
    ref_clouds = [np.asarray(k[2], np.float32) for k in kept["ref"].keyframes]
    assert len(kept["gpu"]) == len(ref_clouds) == nk
    return stats, kept["gpu"], ref_clouds


def test_chain_with_voxel_filters_is_bit_identical(frames, monkeypatch):
    p = OD.default_odom_params()
    assert p.vf_scan_use and p.vf_submap_use
    stats, gpu, ref = chain(frames, OD.VOXEL_ORDER_PCL, monkeypatch, lambda i: 0.0)
    print(f"PCL order: {stats['frames']} frames, {stats['tracked']} tracked, {len(ref)} keyframes, "
          f"max |dT| {stats['max_dpose']}, max |d step| {stats['max_dstep']}")
    assert len(ref) >= 2, len(ref)
    assert stats["tracked"] >= FRAMES - 5
    assert stats["max_dpose"] == 0.0, stats
    for k, (g, o) in enumerate(zip(gpu, ref)):
        np.testing.assert_array_equal(g, o, err_msg=f"keyframe {k}")


def test_chain_in_input_order_is_not(frames, monkeypatch):
    """The non-vacuity check: the default order passes the existing 1e-4 bar, but its keyframe clouds are
    not the oracle's bits."""
    stats, gpu, ref = chain(frames, OD.VOXEL_ORDER_INPUT, monkeypatch, lambda i: 1e-4)
    same = [g.shape == o.shape and g.tobytes() == o.tobytes() for g, o in zip(gpu, ref)]
    print(f"input order: {len(ref)} keyframes, bit-identical {same}, max |dT| {stats['max_dpose']:.3g}")
    assert not all(same)
