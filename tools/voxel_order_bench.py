#!/usr/bin/env python3
"""What the PCL summation order of the voxel filter (DDLO_VOXEL_ORDER_PCL) costs, host wall time
over synchronous calls; medians of --reps runs after warm-up, the variants alternated run by run.

  preprocess   ddlo_preprocess_ordered on frame 1 of the 64 x 2048 sequence (cfg 7), crop 1.0, at
               leaf 0.1 and 0.25: order INPUT against order PCL.  Every call builds and destroys a
               driver handle and uploads the scan, in both orders alike: the difference is the
               order's cost.  With --parent-lib PATH (a build of the parent commit) also that
               library's ddlo_preprocess on the same cloud, in the same process.
  sort         ddlo_debug_sort_order on the scan's voxel keys (upload, device sort, permutation
               back) and its path statistics.
  host         the alternative the device path has to beat: the keys read back from the device
               (blocking hipMemcpy into pageable memory), std::sort of the (key, index) pairs on
               the host (a few lines of C++ compiled here with g++), the permutation sent up again.
  chain        ddlo_odom_process over the first --frames frames of the 64 x 2048 loop with the
               yaml parameters (both voxel filters on), per frame, order INPUT against order PCL.

Prints one JSON line.  Usage: python tools/voxel_order_bench.py [--reps 30] [--frames 40]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOST_SORT = r"""
#include <algorithm>
#include <cstdint>
#include <vector>
struct Idx {
  uint32_t idx, pt;
  bool operator<(const Idx& o) const { return idx < o.idx; }
};
extern "C" void host_sort_order(const uint32_t* keys, int n, int32_t* perm) {
  std::vector<Idx> v(n);
  for (int i = 0; i < n; ++i) v[i] = {keys[i], (uint32_t)i};
  std::sort(v.begin(), v.end(), std::less<Idx>());
  for (int i = 0; i < n; ++i) perm[i] = (int32_t)v[i].pt;
}
"""


def ms(samples):
    return round(1e3 * statistics.median(samples), 4)


def spread(samples):
    s = sorted(samples)
    return [round(1e3 * s[len(s) // 10], 4), round(1e3 * s[-1 - len(s) // 10], 4)]    # 10th / 90th percentile


def hip_runtime():
    """The HIP runtime this process already runs on (the library's), for the host alternative's copies."""
    paths = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    for path in paths:
        H = C.CDLL(path)
        H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        H.hipFree.argtypes = [C.c_void_p]
        count = C.c_int()
        if H.hipGetDeviceCount(C.byref(count)) == 0 and count.value > 0 and H.hipSetDevice(0) == 0:
            return H
    raise RuntimeError(f"no usable HIP runtime among {paths}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    import dynamic_direct_lidar_odometry_amd as P
    from dynamic_direct_lidar_odometry_amd import odometry as OD
    from dynamic_direct_lidar_odometry_amd import scene
    import preprocess_ref as PR

    scan = np.ascontiguousarray(scene.odometry_sequence(64, 2048, 3, cfg_id=7)[0][1], np.float32)
    out = {"reps": args.reps, "points": len(scan), "preprocess": {}, "sort": {}, "host": {}}

    parent = None
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        parent.ddlo_preprocess.restype = C.c_int
        parent.ddlo_preprocess.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_double, C.c_double,
                                           C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    buf = np.zeros_like(scan)
    n = C.c_size_t()

    def parent_call(leaf):
        assert parent.ddlo_preprocess(0, P._ptr(scan), len(scan), 12, 1.0, leaf, P._ptr(buf), len(buf), C.byref(n)) == 0
        return buf[:n.value]

    for leaf in (0.1, 0.25):
        variants = {"input": lambda: OD.preprocess(scan, 1.0, leaf, order=OD.VOXEL_ORDER_INPUT),
                    "pcl": lambda: OD.preprocess(scan, 1.0, leaf, order=OD.VOXEL_ORDER_PCL)}
        if parent is not None:
            variants["parent"] = lambda: parent_call(leaf)
        t = {k: [] for k in variants}
        for f in variants.values():
            for _ in range(5):
                f()
        for _ in range(args.reps):
            for k, f in variants.items():
                t0 = time.perf_counter()
                r = f()
                t[k].append(time.perf_counter() - t0)
        if parent is not None:
            assert parent_call(leaf).tobytes() == variants["input"]().tobytes()
        out["preprocess"][f"leaf_{leaf}"] = {"centroids": len(r), **{f"{k}_ms": ms(v) for k, v in t.items()},
                                             **{f"{k}_p10_p90_ms": spread(v) for k, v in t.items()}}

    OD.sort_order(np.zeros(4, np.uint32))       # the library and its runtime are loaded
    hip = hip_runtime()
    lib_dir = tempfile.mkdtemp()
    src, so = os.path.join(lib_dir, "host_sort.cpp"), os.path.join(lib_dir, "libhost_sort.so")
    open(src, "w").write(HOST_SORT)
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", so, src], check=True)
    H = C.CDLL(so)
    H.host_sort_order.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    for leaf in (0.1, 0.25):
        keys = np.ascontiguousarray(PR.voxel_keys(scan[PR.crop_mask(scan, 1.0)], leaf)[0], np.uint32)
        nbytes = 4 * len(keys)
        dev_keys, dev_perm = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(dev_keys), nbytes) == 0 and hip.hipMalloc(C.byref(dev_perm), nbytes) == 0
        assert hip.hipMemcpy(dev_keys, keys.ctypes.data, nbytes, 1) == 0      # hipMemcpyHostToDevice
        hk = np.zeros(len(keys), np.uint32)
        perm = np.zeros(len(keys), np.int32)
        td, th, ts = [], [], []
        for rep in range(args.reps + 5):
            t0 = time.perf_counter()
            dperm, st = OD.sort_order(keys)
            t1 = time.perf_counter()
            assert hip.hipMemcpy(hk.ctypes.data, dev_keys, nbytes, 2) == 0     # hipMemcpyDeviceToHost (blocking)
            t2 = time.perf_counter()
            H.host_sort_order(hk.ctypes.data, len(hk), perm.ctypes.data)
            t3 = time.perf_counter()
            assert hip.hipMemcpy(dev_perm, perm.ctypes.data, nbytes, 1) == 0
            t4 = time.perf_counter()
            if rep >= 5:
                td.append(t1 - t0)
                th.append(t4 - t1)
                ts.append(t3 - t2)
        assert (dperm == perm).all() and (hk == keys).all()
        hip.hipFree(dev_keys)
        hip.hipFree(dev_perm)
        out["sort"][f"leaf_{leaf}"] = {"keys": len(keys), "device_call_ms": ms(td), "levels": st.levels,
                                       "global_levels": st.global_levels, "lds_segments": st.lds_segments,
                                       "heap_segments": st.heap_segments, "heap_longest": st.heap_longest,
                                       "threshold": st.threshold}
        out["host"][f"leaf_{leaf}"] = {"down_sort_up_ms": ms(th), "std_sort_alone_ms": ms(ts)}

    frames = scene.loop_sequence(64, 2048, 0, args.frames, device=0)[0]
    best = {}
    info = {}
    for _ in range(3):
        for name, order in (("input", OD.VOXEL_ORDER_INPUT), ("pcl", OD.VOXEL_ORDER_PCL)):
            od = OD.Odometry(0, OD.default_odom_params())
            od.set_voxel_order(order)
            t0 = time.perf_counter()
            for f in frames:
                r = od.process(f)
            el = time.perf_counter() - t0
            info[name] = {"keyframes": int(r.num_keyframes)}
            od.close()
            best[name] = min(best.get(name, el), el)
    out["chain_64x2048"] = {"frames": len(frames),
                            **{k: dict(ms_per_frame=round(1e3 * v / len(frames), 4), **info[k]) for k, v in best.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
