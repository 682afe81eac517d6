#!/usr/bin/env python3
"""The motion deskew (include/ddlo_deskew.h) measured: what the pass costs, and what it does to a trajectory.

  cost        device time of the in-place pass over one 64 x 2048 frame, stride 16 (x y z + a float time),
              device events around the launch alone, each behind a fresh upload as in the driver: median,
              quartiles, min and max over --reps passes after --warmup, for a rotating twist, a pure
              translation and the three time types (F64 at stride 24).  The pass reads 16 B and writes 12 B
              per point: 2.1 MB and 1.6 MB per frame.
  trajectory  the plane room of tests/deskew_ref.py driven through with a yaw rate that changes sign
              mid-way (--frames sweeps of 16 x 256), registered four ways: the true unskewed scans, the
              skewed scans with deskew off, the skewed scans with the predicted deskew, and the skewed
              scans with the true twist handed in (what an ideal IMU would give).  Reported: the
              translation error of every tracked pose against the true one (mean, max, final), metres, and
              the rotation error in degrees.  Figures for the record; nothing is asserted about their order.

Prints one JSON line.  Usage: python tools/deskew_bench.py [--reps 200] [--warmup 20] [--frames 40]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    us = 1e3 * np.sort(np.asarray(ms, np.float64))
    q = np.percentile(us, [25, 50, 75])
    return {"median_us": round(q[1], 2), "q25_us": round(q[0], 2), "q75_us": round(q[2], 2), "min_us": round(us[0], 2),
            "max_us": round(us[-1], 2), "n": len(us)}


def cost(args):
    from dynamic_direct_lidar_odometry_amd import odometry as OD
    import deskew_ref as DR
    n = 64 * 2048
    rng = np.random.default_rng(0)
    xyz = rng.uniform(-40, 40, (n, 3)).astype(np.float32)
    s = np.broadcast_to(np.arange(2048) / 2048, (64, 2048)).reshape(-1)
    rot, tr, zero = np.array([0.02, -0.01, 0.5]), np.array([0.2, 0.05, 0.0]), np.zeros(3)
    cases = {
        "f32_stride16_rotation": (DR.records(xyz, (0.1 * s).astype(np.float32), DR.F32_S, 16, 12), 12, DR.F32_S, 0.0, rot),
        "f32_stride16_translation": (DR.records(xyz, (0.1 * s).astype(np.float32), DR.F32_S, 16, 12), 12, DR.F32_S, 0.0, zero),
        "u32_stride16_rotation": (DR.records(xyz, np.round(1e8 * s).astype(np.uint32), DR.U32_NS, 16, 12), 12, DR.U32_NS, 0.0, rot),
        "f64_stride24_rotation": (DR.records(xyz, 1.7e9 + 0.1 * s, DR.F64_S, 24, 16), 16, DR.F64_S, 1.7e9, rot),
    }
    out = {}
    for name, (rec, off, tt, ref, omega) in cases.items():
        OD.deskew_time(rec, omega, tr, off, tt, ref, 0.1, reps=args.warmup)
        out[name] = stats(OD.deskew_time(rec, omega, tr, off, tt, ref, 0.1, reps=args.reps))
    return out


def trajectory(args):
    from dynamic_direct_lidar_odometry_amd import odometry as OD
    import deskew_ref as DR
    seq = DR.sequence(args.frames, 0.1)
    zero = np.zeros(3)
    runs = {}
    for mode in ("unskewed", "skewed_off", "skewed_predicted", "skewed_true_twist"):
        od = OD.Odometry(0, OD.default_odom_params(vf_scan_res=0.2, vf_submap_res=0.2))
        err_t, err_r, origin, sources = [], [], None, []
        for T, omega, t, ref in seq:
            if mode == "unskewed":
                xyz, s, _ = DR.room_scan(T, zero, zero)
            else:
                xyz, s, _ = DR.room_scan(T, omega, t)
            rec = DR.as_f32_rows(DR.records(xyz, (ref + 0.1 * s).astype(np.float32), DR.F32_S, 16, 12))
            if mode in ("skewed_predicted", "skewed_true_twist"):
                od.set_deskew(True, 12, OD.TIME_F32_S, ref, 0.1)
                if mode == "skewed_true_twist":
                    od.set_deskew_motion(omega, t)
                r = od.process(rec)
                sources.append(od.deskew_motion()[2])
            else:
                r = od.process(rec[:, :3])
            if r.status == OD.FIRST:
                origin = T
            if r.status in (OD.FIRST, OD.TRACKED):
                true = np.linalg.inv(origin) @ T
                got = np.array(r.T, np.float64).reshape(4, 4)
                err_t.append(float(np.linalg.norm(got[:3, 3] - true[:3, 3])))
                c = (np.trace(got[:3, :3].T @ true[:3, :3]) - 1) / 2
                err_r.append(float(np.degrees(np.arccos(np.clip(c, -1, 1)))))
        od.close()
        runs[mode] = {"poses": len(err_t), "trans_err_mean_m": round(float(np.mean(err_t)), 5),
                      "trans_err_max_m": round(float(np.max(err_t)), 5), "trans_err_final_m": round(err_t[-1], 5),
                      "rot_err_mean_deg": round(float(np.mean(err_r)), 5), "rot_err_max_deg": round(float(np.max(err_r)), 5)}
        if sources:
            runs[mode]["predicted_frames"] = int(np.sum(np.array(sources) == 1))
        if args.trace:
            runs[mode]["trans_err_m"] = [round(e, 4) for e in err_t]
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--trace", action="store_true", help="also the translation error of every pose")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-trajectory", action="store_true")
    args = ap.parse_args()
    out = {}
    if not args.skip_cost:
        out["cost_64x2048"] = cost(args)
    if not args.skip_trajectory:
        out["trajectory"] = {"frames": args.frames, **trajectory(args)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
