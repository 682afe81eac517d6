#!/usr/bin/env python3
"""Regenerate tests/golden/hungarian_ref.npz: cost matrices and the assignments
the reference's HungarianAlgorithm::Solve gives for them.

    python tests/golden/make_track_golden.py --reference <reference checkout>

A small driver of our own (DRIVER below) includes the reference's
``tracking/hungarian.h`` and is compiled with its ``src/tracking/hungarian.cpp``
by path, into a temporary directory; nothing of the reference is copied into
this repository, only the matrices and the assignments it printed.

The NaN cases (a cost that is 0 / 0) are probed one process each under a time
limit: the solver recurses step3 -> step5 -> step3 without end on them (a
stack overflow, or the time limit when the compiler turns the tail calls into
a loop).  ``nan_terminated`` records, per probe, whether it returned; the
tracker treats such a pair's IoU as 0 instead, so no NaN matrix is
part of the pinned set.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

DRIVER = r"""
#include <tracking/hungarian.h>
#include <cstdio>
#include <cstdint>
int main() {
  int32_t hdr[2];
  while (fread(hdr, sizeof(int32_t), 2, stdin) == 2) {
    const int r = hdr[0], c = hdr[1];
    std::vector<std::vector<double> > m(r, std::vector<double>(c));
    for (int i = 0; i < r; ++i)
      if (fread(m[i].data(), sizeof(double), c, stdin) != (size_t)c) return 2;
    std::vector<int> a;
    HungarianAlgorithm h;
    h.Solve(m, a);
    std::vector<int32_t> o(a.begin(), a.end());
    fwrite(o.data(), sizeof(int32_t), o.size(), stdout);
  }
  return 0;
}
"""


def matrices(rng):
    out = []

    def eighths(r, c, hi=9):
        return rng.integers(0, hi, (r, c)).astype(np.float64) / 8.0

    def plateau(r, c):
        # the tracker's usual matrix: IoU 0 almost everywhere, cost 0.8 + 0.1 * point_diff_rel, a few overlaps
        m = 0.8 + 0.1 * rng.integers(0, 5, (r, c)).astype(np.float64) / 4.0
        for _ in range(int(rng.integers(0, min(r, c) + 1))):
            m[rng.integers(0, r), rng.integers(0, c)] = float(np.float32(rng.uniform(0.0, 0.5)))
        return m

    shapes = [(1, 1), (1, 2), (1, 7), (2, 1), (7, 1), (2, 2), (3, 3), (4, 4), (5, 5), (8, 8), (12, 12), (2, 3), (3, 2),
              (3, 5), (5, 3), (4, 9), (9, 4), (6, 13), (13, 6), (1, 12), (12, 1), (7, 8), (8, 7)]
    for (r, c) in shapes:
        for _ in range(4):
            out.append(eighths(r, c))
        for _ in range(4):
            out.append(plateau(r, c))
        out.append(eighths(r, c, 2))                       # zeros and 1/8 only
        out.append(np.full((r, c), 0.875))                 # all equal
        out.append(np.zeros((r, c)))
        out.append(rng.uniform(0.0, 1.0, (r, c)))          # no ties
    for (r, c) in [(20, 20), (17, 25), (25, 17), (30, 30), (40, 40), (40, 33), (33, 40), (1, 40), (40, 1)]:
        out.append(eighths(r, c))
        out.append(plateau(r, c))
        out.append(np.full((r, c), 0.8))
    return out


def nan_cases():
    n = float("nan")
    return [np.array([[n]]), np.array([[n, 0.9], [0.9, n]]), np.array([[0.9, n], [0.85, 0.9]]),
            np.array([[n, n], [n, n]]), np.array([[0.5, n, 0.9]]), np.array([[0.5], [n], [0.9]])]


def blob(ms):
    b = bytearray()
    for m in ms:
        b += np.array(m.shape, np.int32).tobytes() + np.ascontiguousarray(m, np.float64).tobytes()
    return bytes(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DDLO_REFERENCE"), required="DDLO_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "hungarian_ref.npz"))
    a = ap.parse_args()
    root = os.path.join(a.reference, "dynamic_direct_lidar_odometry")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "driver.cpp")
        exe = os.path.join(tmp, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "include"), src,
                        os.path.join(root, "src", "tracking", "hungarian.cpp"), "-o", exe], check=True)
        ms = matrices(np.random.default_rng(20240607))
        p = subprocess.run([exe], input=blob(ms), stdout=subprocess.PIPE, check=True, timeout=120)
        flat = np.frombuffer(p.stdout, np.int32)
        assert flat.size == sum(m.shape[0] for m in ms)
        probes = nan_cases()
        terminated = []
        for m in probes:
            try:
                q = subprocess.run([exe], input=blob([m]), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=5)
                terminated.append(int(q.returncode == 0 and len(q.stdout) == 4 * m.shape[0]))
            except subprocess.TimeoutExpired:
                terminated.append(0)
    np.savez_compressed(a.out, shapes=np.array([m.shape for m in ms], np.int32),
                        costs=np.concatenate([m.reshape(-1) for m in ms]), assign=flat.copy(),
                        nan_shapes=np.array([m.shape for m in probes], np.int32),
                        nan_costs=np.concatenate([m.reshape(-1) for m in probes]),
                        nan_terminated=np.array(terminated, np.int32))
    print(f"{len(ms)} matrices, {os.path.getsize(a.out)} bytes; NaN probes terminated: {terminated}", file=sys.stderr)


if __name__ == "__main__":
    main()
