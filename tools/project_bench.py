#!/usr/bin/env python3
"""Cost of feeding unorganized clouds to the dynamic pipeline on
the cfg 5 frames (64 x 2048, the moving-pedestrian sequence, device labelling).
Per tracked frame, wall time of

    organized  ddlo_odom_process_tracked on the organized frame (NaN = no return)
    cloud      ddlo_odom_process_tracked_cloud on the frame's finite points

alternated variant by variant on fresh handles after one warm-up run, the
median over the tracked frames, --rounds times.  --blank F sets the last
fraction F of every frame's columns to no-return first (a sector the sensor
does not see), so that the cloud's upload is smaller than the organized
frame's.  (Blanking random pixels instead breaks the image into hundreds of
segments per frame, each a track that coasts for 30 frames: the run then
measures the host tracker at thousands of tracks.)  Prints one JSON line.

    python tools/project_bench.py [--frames 40] [--rounds 5] [--blank 0.0]

The kernels' times come from one profiler run with --profile: the projection
alone (ddlo_seg_process_cloud, a classification, ddlo_seg_point_classes) of a
64 x 2048 and a 512 x 512 frame, --reps times each, then one tracked run:
rocprofv3 --kernel-trace --stats -- python tools/project_bench.py --profile
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

VARIANTS = ("organized", "cloud")


def seg_params():
    return S.yaml_seg_params(rows=64, cols=2048, ground_rows=20, win_row0=0, win_row1=63, win_col0=0, win_col1=2047,
                             max_distance=30)


def sensor_projection(p, ang_bottom):
    """the ring model of scene.lidar_dirs (the yaml's ang_bottom is the reference's 90 degrees)"""
    return S.default_projection(p.replace(ang_bottom=ang_bottom))


def run(frames, clouds, variant):
    od = OD.Odometry(0)
    seg = S.Segmentation(0, seg_params(), labelling="device")
    trk = T.Tracker()
    proj = sensor_projection(seg.params, 22.5)
    ms = []
    for k, (f, c) in enumerate(zip(frames, clouds)):
        t0 = time.perf_counter()
        if variant == "cloud":
            r = od.process_tracked_cloud(seg, trk, c, 0.1 * (k + 1), projection=proj)[0]
        else:
            r = od.process_tracked(seg, trk, f, 0.1 * (k + 1))[0]
        if r.status == OD.TRACKED:
            ms.append((time.perf_counter() - t0) * 1e3)
    od.close()
    seg.close()
    trk.close()
    return ms


def projection_alone(rows, cols, ang_bottom, reps):
    sc = scene.make_scene(1005, moving=True)
    pose = scene.make_pose([0.5, 0.3, scene.SENSOR_Z], (0.01, -0.02, 0.3))
    f = scene.raycast(sc, pose, rows, cols, seed=7, organized=True)
    pts = np.ascontiguousarray(f[np.isfinite(f).all(axis=1)])
    p = S.yaml_seg_params(rows=rows, cols=cols, ang_bottom=ang_bottom, ground_rows=rows // 4, win_row0=0,
                          win_row1=rows - 1, win_col0=0, win_col1=cols - 1)
    seg = S.Segmentation(0, p, labelling="device")
    T4 = np.array(pose, np.float32)
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        _, pr = seg.process_cloud(pts, T4)
        ms.append((time.perf_counter() - t0) * 1e3)
        seg.classify([])
        seg.point_classes()
    seg.close()
    return {"rows": rows, "cols": cols, "points": len(pts), "occupied": pr.occupied_pixels,
            "process_cloud_ms_median": round(float(np.median(ms[1:])), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--blank", type=float, default=0.0, help="fraction of every frame's columns set to no-return")
    ap.add_argument("--reps", type=int, default=20, help="--profile: projections per image size")
    ap.add_argument("--profile", action="store_true", help="the projection alone at two sizes, then one tracked run")
    a = ap.parse_args()
    sc = scene.make_scene(1005, moving=True)
    poses = scene.trajectory(a.frames, 1005)
    frames = [scene.raycast(sc, poses[k], 64, 2048, seed=1005 + k, t=0.1 * k, organized=True) for k in range(a.frames)]
    if a.blank > 0:
        for f in frames:
            f.reshape(64, 2048, 3)[:, 2048 - int(round(a.blank * 2048)):] = np.nan
    clouds = [np.ascontiguousarray(f[np.isfinite(f).all(axis=1)]) for f in frames]
    run(frames, clouds, "cloud")   # warm-up: allocations, first launches
    if a.profile:
        alone = [projection_alone(64, 2048, 22.5, a.reps), projection_alone(512, 512, 45.0, a.reps)]
        ms = run(frames, clouds, "cloud")
        print(json.dumps({"frames": a.frames, "tracked_frames": len(ms), "projection_alone": alone,
                          "cloud_ms_per_frame_median": float(np.median(ms))}))
        return
    run(frames, clouds, "organized")
    med = {v: [] for v in VARIANTS}
    for _ in range(a.rounds):
        for v in VARIANTS:
            ms = run(frames, clouds, v)
            med[v].append(round(float(np.median(ms)), 4))
    print(json.dumps({"frames": a.frames, "tracked_frames": len(ms), "rounds": a.rounds, "blank": a.blank,
                      "points_per_cloud_mean": float(np.mean([len(c) for c in clouds])),
                      "ms_per_tracked_frame_median_by_round": med}))


if __name__ == "__main__":
    main()
