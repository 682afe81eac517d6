#!/usr/bin/env python3
"""Cost of the dynamic-object step (ddlo_odom_process_dynamic, ddlo_seg_objects,
ddlo_seg_static_cloud) on the cfg 5 frames, host wall time over synchronous calls.

  driver        ms/frame of process_dynamic (NULL callback: every object cut out) beside
                ddlo_odom_process on the same organized 64 x 2048 scans; with --parent-lib PATH also
                ddlo_odom_process of this library and of that one (built from the parent commit) through
                the same raw-ctypes loop, each in a child process, alternating
  segmentation  seg.process alone beside seg.process + objects on bench.py's 512 x 512 scan, and on
                the cfg 5 frames; us of the objects call (label upload + the one kernel + read-back)
                and of static_cloud (removal + crop + voxel) on a processed scan

Prints one JSON line.  Usage: python tools/dynamic_bench.py [--frames 40] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, COLS = 64, 2048


def cfg5_organized(n):
    """The first n frames of scene.odometry_sequence's cfg 5 chain, organized (NaN = no return)."""
    from dynamic_direct_lidar_odometry_amd import scene
    sc = scene.make_scene(1005, moving=True)
    poses = scene.trajectory(n, 1005)
    return [scene.raycast(sc, poses[k], ROWS, COLS, seed=1005 + k, t=0.1 * k, organized=True) for k in range(n)]


def child_plain(lib_path, npz):
    """ddlo_odom_process of the library at lib_path over the frames in npz (raw ctypes: that library may
    lack the newer entry points).  Prints ms/frame."""
    frames = np.load(npz)["frames"]
    L = C.CDLL(lib_path)
    from dynamic_direct_lidar_odometry_amd.odometry import OdomResult
    P, S = C.c_void_p, C.c_size_t
    L.ddlo_odom_create.argtypes = [C.c_int, P, C.POINTER(P)]
    L.ddlo_odom_process.argtypes = [P, P, S, S, C.POINTER(OdomResult)]
    L.ddlo_odom_destroy.argtypes = [P]
    best = None
    for _ in range(3):
        h = P()
        assert L.ddlo_odom_create(0, None, C.byref(h)) == 0
        r = OdomResult()
        t0 = time.perf_counter()
        for f in frames:
            assert L.ddlo_odom_process(h, f.ctypes.data_as(P), f.shape[0], 12, C.byref(r)) == 0
        el = time.perf_counter() - t0
        L.ddlo_odom_destroy(h)
        best = el if best is None else min(best, el)
    print(json.dumps({"ms_per_frame": 1e3 * best / len(frames), "keyframes": r.num_keyframes}))


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child-plain", nargs=2, metavar=("LIB", "NPZ"), default=None)
    args = ap.parse_args()
    if args.child_plain:
        return child_plain(*args.child_plain)
    from dynamic_direct_lidar_odometry_amd import odometry as OD
    from dynamic_direct_lidar_odometry_amd import scene
    from dynamic_direct_lidar_odometry_amd import segmentation as SG
    out = {}
    frames = cfg5_organized(args.frames)
    sp = SG.yaml_seg_params(rows=ROWS, cols=COLS, ground_rows=24, win_row0=0, win_row1=ROWS - 1, win_col0=0,
                            win_col1=COLS - 1, max_distance=30)

    def chain(dynamic):
        best, info = None, None
        for _ in range(3):
            od = OD.Odometry(0)
            seg = SG.Segmentation(0, sp)
            kf = objs = 0
            t0 = time.perf_counter()
            for f in frames:
                if dynamic:
                    r, sr = od.process_dynamic(seg, f, None)
                    objs += sr.segments
                else:
                    r = od.process(f)
                kf += r.keyframe_added
            el = time.perf_counter() - t0
            pts = sum(od.keyframe(k)[1] for k in range(r.num_keyframes))
            od.close()
            seg.close()
            if best is None or el < best:
                best, info = el, {"keyframes": r.num_keyframes, "keyframe_points": pts, "segments": objs}
        return dict(ms_per_frame=round(1e3 * best / len(frames), 4), **info)

    out["driver_64x2048"] = {"frames": len(frames), "process": chain(False), "process_dynamic": chain(True)}
    if args.parent_lib:
        npz = os.path.join(ROOT, "bench_out", "dynamic_bench_frames.npz")
        os.makedirs(os.path.dirname(npz), exist_ok=True)
        np.savez(npz, frames=np.stack(frames))
        import dynamic_direct_lidar_odometry_amd as pkg
        # the same raw-ctypes loop for both libraries, alternating (the package's wrapper adds its own microseconds)
        for key, lib in (("process_raw_this_lib", pkg.lib_path()), ("process_raw_parent_lib", args.parent_lib)) * 2:
            cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-plain", lib, npz],
                                check=True, capture_output=True, text=True)
            out["driver_64x2048"].setdefault(key, []).append(json.loads(cp.stdout.strip().splitlines()[-1]))

    def seg_case(name, xyz, T, params, resid):
        seg = SG.Segmentation(0, params)
        t_proc = timed(lambda: seg.process(xyz, T, resid), args.reps)
        t_both = timed(lambda: (seg.process(xyz, T, resid), seg.objects()), args.reps)
        res = seg.process(xyz, T, resid)
        # objects() caches per scan: time the first call after each process
        t_obj = 0.0
        for _ in range(args.reps):
            seg.process(xyz, T, resid)
            t0 = time.perf_counter()
            objs = seg.objects()
            t_obj += time.perf_counter() - t0
        ids = [int(i) for i in objs["id"]]
        c = np.ascontiguousarray(T[:3, 3], np.float32)
        t_static = timed(lambda: seg.static_cloud(ids, c, 1.0, 0.1), args.reps)
        t_query = timed(lambda: seg.L.ddlo_seg_static_cloud(seg.h, None, 0, c.ctypes.data_as(C.c_void_p), 1.0, 0.1, None,
                                                            0, C.byref(C.c_size_t())), args.reps)
        out[name] = {"segments": res.segments, "objects": len(ids), "segment_points": int(objs["num_points"].sum()),
                     "process_ms": round(1e3 * t_proc, 4), "process_plus_objects_ms": round(1e3 * t_both, 4),
                     "objects_call_us": round(1e6 * t_obj / args.reps, 1),
                     "static_cloud_call_us": round(1e6 * t_static, 1),
                     "static_cloud_device_only_us": round(1e6 * t_query, 1)}
        seg.close()

    sc = scene.make_scene(1005, moving=True)
    pose = scene.make_pose([0.0, 0.0, scene.SENSOR_Z], (0.0, 0.0, math.radians(20.0)))
    pts = scene.raycast(sc, pose, 512, 512, 1005, organized=True)
    bad = ~np.isfinite(pts).all(axis=1)
    xyz = scene.transform(np.nan_to_num(pts, nan=0.0), pose).astype(np.float32)
    xyz[bad] = np.nan
    resid = np.abs(np.random.default_rng(0).normal(0, 0.2, (512, 512))).astype(np.float32)
    seg_case("seg_512x512_yaml", xyz, pose.astype(np.float32), SG.yaml_seg_params(), resid)
    seg_case("seg_512x512_wide_window", xyz, pose.astype(np.float32),
             SG.yaml_seg_params(win_row0=100, win_row1=500, win_col0=0, win_col1=511, max_distance=30), resid)
    # one cfg 5 frame in its own sensor frame, the whole image as the labelling window (the driver's case)
    seg_case("seg_64x2048_cfg5_frame", frames[min(5, len(frames) - 1)], np.eye(4, dtype=np.float32), sp,
             np.abs(np.random.default_rng(1).normal(0, 0.2, (ROWS, COLS))).astype(np.float32))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
