#!/usr/bin/env python3
"""What the organized-scan row/column filter (ddlo_odom_set_downsampling, ddlo_seg_set_downsampling)
changes in time, host wall time over synchronous calls.  Not a threshold: the filter changes the
workload (fewer points register), not a kernel under test.

  chain      ddlo_odom_process over the first --frames frames of bench.py's odometry leg (the cfg 5
             64 x 2048 loop, yaml parameters): downsampling off, (2, 2) as cfg/ddlo.yaml ships it and
             (1, 10) as cfg/DOALS.yaml does.  A fresh driver per run after a warm-up run of each,
             the variants alternated, best of --rounds; with the mean scan size after preprocessing.
  keyframe   ddlo_seg_static_cloud (crop 1.0 around the origin, leaf 0.1, every object removed) on one
             segmented frame of that loop: the pass off, (2, 2), (1, 10), and with --parent-lib PATH (a
             build of the parent commit) that library's ddlo_seg_static_cloud on the same frame in the
             same process.  Medians of --reps calls after 5 warm-up calls, alternated call by call.

Prints one JSON line.  Usage: python tools/downsample_bench.py [--frames 100] [--reps 30] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, COLS = 64, 2048
STEPS = {"off": None, "2x2": (2, 2), "1x10": (1, 10)}


def ms(samples):
    return round(1e3 * statistics.median(samples), 4)


def spread(samples):
    s = sorted(samples)
    return [round(1e3 * s[len(s) // 10], 4), round(1e3 * s[-1 - len(s) // 10], 4)]    # 10th / 90th percentile


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    import dynamic_direct_lidar_odometry_amd as P
    from dynamic_direct_lidar_odometry_amd import odometry as OD
    from dynamic_direct_lidar_odometry_amd import scene
    from dynamic_direct_lidar_odometry_amd import segmentation as S

    frames = scene.loop_sequence(ROWS, COLS, 0, args.frames, device=0)[0]
    out = {"frames": len(frames), "rounds": args.rounds, "reps": args.reps, "chain_64x2048": {}, "keyframe_64x2048": {}}

    def chain(steps, n):
        od = OD.Odometry(0, OD.default_odom_params())
        if steps:
            od.set_downsampling(1, *steps, ROWS, COLS)
        pts = kfs = 0
        t0 = time.perf_counter()
        for f in frames[:n]:
            r = od.process(f)
            pts += r.scan_points
            kfs += r.keyframe_added
        el = time.perf_counter() - t0
        od.close()
        return el, pts / n, kfs

    best, info = {}, {}
    for name, steps in STEPS.items():
        chain(steps, min(8, len(frames)))
    for _ in range(args.rounds):
        for name, steps in STEPS.items():
            el, pts, kfs = chain(steps, len(frames))
            best[name] = min(best.get(name, el), el)
            info[name] = {"mean_scan_points": round(pts, 1), "keyframes": kfs}
    for name in STEPS:
        out["chain_64x2048"][name] = dict(ms_per_frame=round(1e3 * best[name] / len(frames), 4), **info[name])

    # one segmented frame: the sensor-frame scan taken as the world-frame one (pose identity)
    sp = S.yaml_seg_params(rows=ROWS, cols=COLS, ground_rows=20, win_row0=0, win_row1=63, win_col0=0, win_col1=2047,
                           max_distance=30)
    scan = np.ascontiguousarray(frames[min(5, len(frames) - 1)], np.float32)
    eye = np.eye(4, dtype=np.float32)
    seg = S.Segmentation(0, sp)
    res = seg.process(scan, eye)
    ids = np.arange(1, res.segments + 1, dtype=np.int32)
    centre = np.zeros(3, np.float32)
    buf = np.zeros((ROWS * COLS, 3), np.float32)
    n = C.c_size_t()

    def call(lib, h):
        assert lib.ddlo_seg_static_cloud(h, P._ptr(ids) if ids.size else None, ids.size, P._ptr(centre), 1.0, 0.1,
                                         P._ptr(buf), len(buf), C.byref(n)) == 0
        return n.value

    def with_steps(steps):
        seg.set_downsampling(1 if steps else 0, *(steps or (1, 1)))
        return call(seg.L, seg.h)

    variants = {name: (lambda s=steps: with_steps(s)) for name, steps in STEPS.items()}
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        V = C.c_void_p
        parent.ddlo_seg_create.argtypes = [C.c_int, C.POINTER(S.SegParams), C.POINTER(V)]
        parent.ddlo_seg_process.argtypes = [V, V, C.c_size_t, V, V, C.POINTER(S.SegResult)]
        parent.ddlo_seg_static_cloud.argtypes = [V, V, C.c_size_t, V, C.c_double, C.c_double, V, C.c_size_t,
                                                 C.POINTER(C.c_size_t)]
        parent.ddlo_seg_destroy.argtypes = [V]
        ph = V()
        assert parent.ddlo_seg_create(0, C.byref(sp), C.byref(ph)) == 0
        pres = S.SegResult()
        assert parent.ddlo_seg_process(ph, P._ptr(scan), 12, P._ptr(eye.reshape(16)), None, C.byref(pres)) == 0
        assert pres.segments == res.segments
        variants["parent"] = lambda: call(parent, ph)
        a = call(parent, ph)
        pa = buf[:a].copy()
        b = with_steps(None)
        assert a == b and pa.tobytes() == buf[:b].tobytes()          # off: the parent's bits
    t = {k: [] for k in variants}
    sizes = {}
    for k, f in variants.items():
        for _ in range(5):
            sizes[k] = f()
    for _ in range(args.reps):
        for k, f in variants.items():
            t0 = time.perf_counter()
            f()
            t[k].append(time.perf_counter() - t0)
    out["keyframe_64x2048"] = {"segments_removed": int(ids.size),
                               **{k: {"ms": ms(v), "p10_p90_ms": spread(v), "points": sizes[k]} for k, v in t.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
