#!/usr/bin/env python3
"""Cost of the on-board tracker: ddlo_odom_process_tracked
against ddlo_odom_process_dynamic with a NULL callback on the cfg 5 frames
(64 x 2048, the moving-pedestrian sequence), alternated run by run; the track
pool's size over the frames; ddlo_track_update's host time against the track
count.  Prints one JSON line.

    python tools/track_bench.py [--frames 40] [--rounds 5] [--labelling device]

The two kernels' times come from one profiler run of this script with
--rounds 1 --drop (rocprofv3 --kernel-trace --stats -- python tools/track_bench.py ...).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynamic_direct_lidar_odometry_amd import odometry as OD  # noqa: E402
from dynamic_direct_lidar_odometry_amd import scene  # noqa: E402
from dynamic_direct_lidar_odometry_amd import segmentation as S  # noqa: E402
from dynamic_direct_lidar_odometry_amd import tracking as T  # noqa: E402


def seg_params():
    return S.yaml_seg_params(rows=64, cols=2048, ground_rows=20, win_row0=0, win_row1=63, win_col0=0, win_col1=2047,
                             max_distance=30)


def run(frames, labelling, tracked, drop=False):
    od = OD.Odometry(0)
    seg = S.Segmentation(0, seg_params(), labelling=labelling)
    trk = T.Tracker()
    ms, pool = [], []
    for k, f in enumerate(frames):
        t0 = time.perf_counter()
        if tracked:
            r, _, _ = od.process_tracked(seg, trk, f, 0.1 * (k + 1))
        else:
            r, _ = od.process_dynamic(seg, f, None)
        dt = (time.perf_counter() - t0) * 1e3
        if r.status == OD.TRACKED:
            ms.append(dt)
            if tracked:
                pool.append(seg.tracks_stats())
                if drop:   # (outside the timed part) the removal a keyframe would make on this frame
                    seg.static_cloud_tracks([int(x["id"]) for x in trk.tracks() if x["status"] != T.STATIC])
    od.close()
    seg.close()
    trk.close()
    return ms, pool


def update_cost(counts=(1, 5, 10, 20, 40), reps=200):
    """host time of one ddlo_track_update with n tracks and n detections (every one matched)"""
    out = {}
    rng = np.random.default_rng(0)
    for n in counts:
        objs = np.zeros(n, S.OBJECT_DTYPE)
        objs["id"] = np.arange(1, n + 1)
        objs["num_points"] = rng.integers(20, 500, n)
        st = np.column_stack([rng.uniform(-20, 20, (n, 2)), np.full(n, 0.5), rng.uniform(-0.5, 0.5, n),
                              rng.uniform(0.4, 1.5, (n, 3))]).astype(np.float32)
        objs["state"] = st
        trk = T.Tracker()
        trk.update(0.1, objs)
        t0 = time.perf_counter()
        for _ in range(reps):
            trk.update(0.1, objs)
        out[n] = (time.perf_counter() - t0) / reps * 1e6
        trk.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--labelling", default="device")
    ap.add_argument("--drop", action="store_true",
                    help="also remove the non-static tracks' lists on every tracked frame (k_trk_drop runs on "
                         "keyframes only, which these 40 frames hardly have): for the profiler run")
    a = ap.parse_args()
    sc = scene.make_scene(1005, moving=True)
    poses = scene.trajectory(a.frames, 1005)
    frames = [scene.raycast(sc, poses[k], 64, 2048, seed=1005 + k, t=0.1 * k, organized=True) for k in range(a.frames)]
    run(frames, a.labelling, True)   # warm-up: allocations, first launches
    tr, dy, pool = [], [], []
    for _ in range(a.rounds):
        m, pool = run(frames, a.labelling, True, a.drop)
        tr.append(float(np.median(m)))
        m, _ = run(frames, a.labelling, False)
        dy.append(float(np.median(m)))
    print(json.dumps({
        "frames": a.frames, "labelling": a.labelling,
        "tracked_ms_per_frame_median_by_round": [round(x, 4) for x in tr],
        "dynamic_null_ms_per_frame_median_by_round": [round(x, 4) for x in dy],
        "pool_lists_by_frame": [p[0] for p in pool], "pool_indices_by_frame": [p[1] for p in pool],
        "pool_capacity": pool[-1][2] if pool else 0,
        "track_update_us_by_track_count": {str(k): round(v, 2) for k, v in update_cost().items()},
    }))


if __name__ == "__main__":
    main()
