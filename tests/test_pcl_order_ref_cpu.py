"""CPU tests that pin tests/pcl_order_ref.py: its sort_order to std::sort itself (a small
stand-alone program compiled here with g++, the libstdc++ the oracle is built against), its
voxel_grid to the oracle's pcl::VoxelGrid restatement with assert_array_equal."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pcl_order_ref as PO
import preprocess_ref as PR
from oracle import oracle as O

STD_SORT_MAIN = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>
struct Idx {
  uint32_t idx, pt;
  bool operator<(const Idx& o) const { return idx < o.idx; }
};
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<uint32_t> keys;
  uint32_t k;
  while (std::fread(&k, 4, 1, f) == 1) keys.push_back(k);
  std::fclose(f);
  std::vector<Idx> v(keys.size());
  for (size_t i = 0; i < keys.size(); ++i) v[i] = {keys[i], (uint32_t)i};
  std::sort(v.begin(), v.end(), std::less<Idx>());
  f = std::fopen(argv[2], "wb");
  if (!f) return 4;
  for (const Idx& e : v) std::fwrite(&e.pt, 4, 1, f);
  std::fclose(f);
  return 0;
}
"""

S = 512      # the device's hand-over threshold (the lengths around it are sort lengths as any other here)
LENGTHS = (0, 1, 2, 16, 17, 18, 33, S - 1, S, S + 1, 2 * S + 3)


@pytest.fixture(scope="module")
def std_sort(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("std_sort")
    src, exe = d / "std_sort_main.cpp", d / "std_sort_main"
    src.write_text(STD_SORT_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", str(exe), str(src)], check=True)

    def run(keys):
        a = np.ascontiguousarray(keys, dtype=np.uint32)
        a.tofile(d / "keys.bin")
        subprocess.run([str(exe), str(d / "keys.bin"), str(d / "perm.bin")], check=True)
        return np.fromfile(d / "perm.bin", dtype=np.uint32).astype(np.int64)
    return run


def _check(std_sort, keys):
    perm, stats = PO.sort_order(keys)
    np.testing.assert_array_equal(perm, std_sort(keys))
    return stats


@pytest.mark.parametrize("n", LENGTHS)
def test_sort_order_patterns(std_sort, n):
    if n < 17:
        _check(std_sort, np.arange(n)[::-1] // 2)
        return
    for name, keys in PO.key_patterns(n).items():
        _check(std_sort, keys)


def test_sort_order_heap_path(std_sort):
    stats = _check(std_sort, PO.heap_keys())
    assert stats["heap_segments"] == 35 and stats["heap_longest"] == 340


def test_sort_order_scale(std_sort):
    keys = np.random.default_rng(5).integers(0, 40000, 131072)
    stats = _check(std_sort, keys)
    assert stats["heap_segments"] == 0 and stats["levels"] < 34
    _check(std_sort, np.full(4 * S, 3))


def _voxel_clouds():
    out = dict(PR.edge_clouds())
    s = PR.sites()
    for name, idx in PR.nonfinite_patterns(len(s)).items():
        out[f"sites_nan_{name}"] = PR.with_nonfinite(s, idx)
    out["line"] = PO.line_cloud()
    out["single_voxel_5000"] = PR.single_voxel(n=5000)
    return out


CLOUDS = _voxel_clouds()


@pytest.mark.parametrize("crop", (0.0, 1.0))
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_voxel_grid_equals_oracle(std_sort, name, crop):
    pts = CLOUDS[name]
    kept = PR.crop_keep(pts, crop) if crop > 0 else pts
    for leaf in PR.LEAVES:
        got = PO.voxel_grid(pts, leaf, crop)
        ref = O.voxel_grid(kept, leaf)
        assert got is not None
        np.testing.assert_array_equal(got[0], ref)
        x = pts[PR.crop_mask(pts, crop) if crop > 0 else PR.finite_mask(pts)]
        if len(x):       # the keys of a real cloud, against std::sort directly
            _check(std_sort, PR.voxel_keys(x, leaf)[0])


def test_voxel_grid_overflow():
    assert PO.voxel_grid(PR.wide(PR.OVERFLOW_HALF_Z), 0.05) is None
    w = PR.wide(PR.OVERFLOW_HALF_Z)
    np.testing.assert_array_equal(PO.voxel_grid(w, 0.1)[0], O.voxel_grid(w, 0.1))


def test_line_reaches_the_depth_limit():
    x = PO.line_cloud()
    for leaf in (0.1, 0.3):
        _, stats = PO.sort_order(PR.voxel_keys(x, leaf)[0])
        assert stats["heap_segments"] > 0, leaf
        ref = O.voxel_grid(x, leaf)
        differ = int((ref != PR.voxel_grid(x, leaf)[0]).any(axis=1).sum())
        print(f"line, leaf {leaf}: heap {stats}, {differ} of {len(ref)} centroids differ from input order")
        assert differ > 0
