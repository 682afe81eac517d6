#!/usr/bin/env python3
"""Cost of the per-pixel classes on the cfg 5 frames (64 x 2048,
the moving-pedestrian sequence, device labelling).  Per tracked frame, wall
time of

    tracked    ddlo_odom_process_tracked alone
    dynamic    ... + ddlo_odom_classify + the dynamic index set
    clouds     ... + ddlo_odom_classify + ddlo_seg_frame_clouds (four clouds copied out)
    readback   ... + the route that needs no class image: ddlo_track_tracks, one
               ddlo_seg_track_indices per track, numpy unions per status

alternated variant by variant on fresh handles, the median over the tracked
frames, --rounds times.  Prints one JSON line.

    python tools/classes_bench.py [--frames 40] [--rounds 5]

The kernels' times come from one profiler run with --profile (one run that
classifies and reads the set and the clouds on every tracked frame):
rocprofv3 --kernel-trace --stats -- python tools/classes_bench.py --profile
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

VARIANTS = ("tracked", "dynamic", "clouds", "readback")


def seg_params():
    return S.yaml_seg_params(rows=64, cols=2048, ground_rows=20, win_row0=0, win_row1=63, win_col0=0, win_col1=2047,
                             max_distance=30)


def run(frames, variant):
    od = OD.Odometry(0)
    seg = S.Segmentation(0, seg_params(), labelling="device")
    trk = T.Tracker()
    ms, sizes = [], []
    for k, f in enumerate(frames):
        t0 = time.perf_counter()
        r, _, _ = od.process_tracked(seg, trk, f, 0.1 * (k + 1))
        if r.status == OD.TRACKED:
            if variant == "dynamic":
                od.classify(seg, trk)
                out = seg.class_indices(S.CLS_DYNAMIC)
            elif variant == "clouds":
                od.classify(seg, trk)
                out = seg.frame_clouds()
            elif variant == "all":
                od.classify(seg, trk)
                out = (seg.class_indices(S.CLS_DYNAMIC), seg.frame_clouds())
            elif variant == "readback":
                recs = trk.tracks()
                by = {0: [], 1: [], 2: []}
                for x in recs:
                    by[int(x["status"])].append(seg.track_indices(int(x["id"])))
                out = [np.unique(np.concatenate(v)) if v else np.zeros(0, np.int32) for v in by.values()]
                sizes.append(len(recs))
            dt = (time.perf_counter() - t0) * 1e3
            ms.append(dt)
    od.close()
    seg.close()
    trk.close()
    return ms, sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="one warm-up and one run of everything, for the profiler")
    a = ap.parse_args()
    sc = scene.make_scene(1005, moving=True)
    poses = scene.trajectory(a.frames, 1005)
    frames = [scene.raycast(sc, poses[k], 64, 2048, seed=1005 + k, t=0.1 * k, organized=True) for k in range(a.frames)]
    run(frames, "all")   # warm-up: allocations, first launches
    if a.profile:
        ms, _ = run(frames, "all")
        print(json.dumps({"frames": a.frames, "tracked_frames": len(ms), "all_ms_per_frame_median": float(np.median(ms))}))
        return
    med = {v: [] for v in VARIANTS}
    tracks = []
    for _ in range(a.rounds):
        for v in VARIANTS:
            ms, sizes = run(frames, v)
            med[v].append(round(float(np.median(ms)), 4))
            if sizes:
                tracks = sizes
    print(json.dumps({"frames": a.frames, "tracked_frames": len(ms), "rounds": a.rounds,
                      "ms_per_tracked_frame_median_by_round": med,
                      "tracks_per_frame_min_max": [int(min(tracks)), int(max(tracks))] if tracks else None}))


if __name__ == "__main__":
    main()
