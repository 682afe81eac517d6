#!/usr/bin/env python3
"""Host labelling against device labelling (ddlo_seg_set_labelling), host wall time over
synchronous calls.

  seg      ddlo_seg_process (and process + objects) in both modes, alternated on handles of the
           same shape: 512 x 512 with the yaml window, 512 x 512 with the wide window, 64 x 2048
           with the whole image as window.  Every handle is warmed up; the figure is the median
           of --reps runs.  Per shape also the segments, the components whose push prefix the
           device replayed and the longest prefix.
  driver   ddlo_odom_process_dynamic (NULL callback) over the cfg 5 frames of
           tools/dynamic_bench.py with a host-mode and a device-mode segmentation, alternated
           three times, best run each; and the histogram of the longest replayed prefix per frame.
  --profile SHAPE   only process that shape --reps times in device mode (for a kernel trace).

Prints one JSON line.  Usage: python tools/label_bench.py [--reps 20] [--frames 40]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def shapes():
    from dynamic_direct_lidar_odometry_amd import scene
    from dynamic_direct_lidar_odometry_amd import segmentation as SG
    sc = scene.make_scene(1005, moving=True)

    def world_scan(frame, rows, cols):
        pose = scene.make_pose([0.3 * frame, -0.2 * frame, scene.SENSOR_Z], (0.0, 0.0, math.radians(7.0 * frame)))
        pts = scene.raycast(sc, pose, rows, cols, 1005 + frame, t=0.1 * frame, organized=True)
        bad = ~np.isfinite(pts).all(axis=1)
        xyz = scene.transform(np.nan_to_num(pts, nan=0.0), pose).astype(np.float32)
        xyz[bad] = np.nan
        return xyz, pose.astype(np.float32)

    def resid(rows, cols, seed):
        return np.abs(np.random.default_rng(seed).normal(0, 0.2, (rows, cols))).astype(np.float32)

    x0, T0 = world_scan(0, 512, 512)
    x3, T3 = world_scan(3, 512, 512)
    x1, T1 = world_scan(1, 64, 2048)
    return {
        "512x512_yaml": (x0, T0, SG.yaml_seg_params(), resid(512, 512, 0)),
        "512x512_wide": (x3, T3, SG.yaml_seg_params(win_row0=100, win_row1=500, win_col0=0, win_col1=511,
                                                    max_distance=30), resid(512, 512, 3)),
        "64x2048_whole": (x1, T1, SG.yaml_seg_params(rows=64, cols=2048, ground_rows=20, win_row0=0, win_row1=63,
                                                     win_col0=0, win_col1=2047, max_distance=30), resid(64, 2048, 1)),
    }


def ms(samples):
    return round(1e3 * statistics.median(samples), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--profile", default=None)
    args = ap.parse_args()
    from dynamic_direct_lidar_odometry_amd import odometry as OD
    from dynamic_direct_lidar_odometry_amd import segmentation as SG
    cases = shapes()
    if args.profile:
        xyz, T, p, resid = cases[args.profile]
        seg = SG.Segmentation(0, p, labelling="device")
        for _ in range(args.reps):
            r = seg.process(xyz, T, resid)
        print(json.dumps({"profile": args.profile, "reps": args.reps, "segments": r.segments}))
        return
    out = {"reps": args.reps, "seg": {}}
    for name, (xyz, T, p, resid) in cases.items():
        segs = {m: SG.Segmentation(0, p, labelling=m) for m in ("host", "device")}
        t = {m: {"process": [], "process_objects": []} for m in segs}
        for m, s in segs.items():
            for _ in range(5):
                s.process(xyz, T, resid)
                s.objects()
        for _ in range(args.reps):
            for m, s in segs.items():
                t0 = time.perf_counter()
                res = s.process(xyz, T, resid)
                t1 = time.perf_counter()
                s.process(xyz, T, resid)
                s.objects()
                t2 = time.perf_counter()
                t[m]["process"].append(t1 - t0)
                t[m]["process_objects"].append(t2 - t1)
        replayed, longest = segs["device"].labelling_stats()
        out["seg"][name] = {"segments": res.segments, "replayed": replayed, "longest_prefix": longest,
                            **{f"{m}_{k}_ms": ms(v) for m in t for k, v in t[m].items()}}
        for s in segs.values():
            s.close()

    from dynamic_bench import COLS, ROWS, cfg5_organized
    frames = cfg5_organized(args.frames)
    sp = SG.yaml_seg_params(rows=ROWS, cols=COLS, ground_rows=24, win_row0=0, win_row1=ROWS - 1, win_col0=0,
                            win_col1=COLS - 1, max_distance=30)
    best = {"host": None, "device": None}
    info = {}
    prefixes = []
    for _ in range(3):
        for m in best:
            od = OD.Odometry(0)
            seg = SG.Segmentation(0, sp, labelling=m)
            objs = 0
            pre = []
            t0 = time.perf_counter()
            for f in frames:
                r, sr = od.process_dynamic(seg, f, None)
                objs += sr.segments
                if m == "device" and r.status == OD.TRACKED:
                    pre.append(seg.labelling_stats())
            el = time.perf_counter() - t0
            info[m] = {"keyframes": r.num_keyframes, "segments": objs}
            od.close()
            seg.close()
            best[m] = el if best[m] is None else min(best[m], el)
            if m == "device":
                prefixes = pre
    out["driver_64x2048"] = {"frames": len(frames),
                             **{m: dict(ms_per_frame=round(1e3 * best[m] / len(frames), 4), **info[m]) for m in best},
                             "replayed_per_frame": [a for a, _ in prefixes],
                             "longest_prefix_per_frame": [b for _, b in prefixes]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
