#!/usr/bin/env python3
"""Cost of the intensity channel (ddlo_odom_set_intensity, ddlo_intensity.h) on the cfg 5 chain that
bench.py's odometry leg runs: host wall time per frame of ddlo_odom_process over the same 64 x 2048
frames with the channel off and on, alternating, each pass on a fresh driver.

  off   (n, 3) rows, stride 12: the kernels that always ran
  on    pcl::PointXYZI records (stride 32, intensity at 16): k_pack4<true>, k_voxel_centroids<true>
        for the scan and the keyframes, k_take_w per frame, k_transform4<true> per keyframe; the
        upload is 32 B per point instead of 12
  on16  packed x y z i rows (stride 16, intensity at 12): the same kernels, 16 B per point

Prints one JSON line.  Usage: python tools/intensity_bench.py [--frames 300] [--passes 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--passes", type=int, default=3)
    args = ap.parse_args()
    import dynamic_direct_lidar_odometry_amd as P
    from dynamic_direct_lidar_odometry_amd import odometry as OD
    from dynamic_direct_lidar_odometry_amd import scene
    frames = scene.loop_sequence(64, 2048, 0, args.frames, device=0)[0]
    rng = np.random.default_rng(0)
    inputs = {"off": [np.ascontiguousarray(f, np.float32) for f in frames], "on": [], "on16": []}
    for f in inputs["off"]:
        w = rng.uniform(0, 255, len(f)).astype(np.float32)
        rec = np.zeros((len(f), 8), np.float32)
        rec[:, :3], rec[:, 4] = f, w
        inputs["on"].append(rec)
        inputs["on16"].append(np.ascontiguousarray(np.column_stack([f, w]), np.float32))
    c = P.Context(0)            # every host page read by the DMA engine once, as bench.py does
    for key in inputs:
        for a in inputs[key]:
            c.set_source(np.ascontiguousarray(a[:, :3]))
    c.close()

    def chain(key):
        od = OD.Odometry(0)
        if key != "off":
            od.set_intensity(True, 16 if key == "on" else 12)
        t0 = time.perf_counter()
        for a in inputs[key]:
            r = od.process(a)
        el = time.perf_counter() - t0
        info = (r.num_keyframes, int(r.submap_points), bytes(r.T))
        od.close()
        return 1e3 * el / len(frames), info

    chain("off")                # warm-up: code objects, pools
    chain("on")
    ms = {k: [] for k in inputs}
    infos = set()
    for _ in range(args.passes):
        for key in inputs:
            t, info = chain(key)
            ms[key].append(round(t, 4))
            infos.add(info)
    assert len(infos) == 1, "the chain's poses, keyframes or submaps depend on the channel"
    print(json.dumps({"frames": len(frames), "passes": args.passes, "ms_per_frame": ms,
                      "best": {k: min(v) for k, v in ms.items()}, "keyframes": next(iter(infos))[0]}))


if __name__ == "__main__":
    main()
