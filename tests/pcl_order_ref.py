"""Plain numpy / Python restatement of the PCL summation order of the voxel filter
(csrc/voxel_order.hip): the permutation that libstdc++'s std::sort (introsort,
bits/stl_algo.h, bits/stl_heap.h) leaves on pairs (key_i, i) compared by key alone,
and the voxel filter that sums every voxel's points in that order.  It imports
neither the product nor the oracle: tests/test_pcl_order_ref_cpu.py pins it to
std::sort itself and to the oracle on the CPU; the GPU tests compare the kernels
with it bit for bit.

  sort_order(keys)   (perm, stats): perm[r] = the original index at sorted rank r
  voxel_grid(...)    preprocess_ref.voxel_grid with that permutation swapped in

The sort, as std::__sort runs it:
  * the depth limit is 2 * floor(log2(n)); every level of __introsort_loop takes one
    off it and splits each segment longer than 16 in two, which inherit what is left:
    all segments of one level share one counter and are independent of each other;
  * one split: __move_median_to_first on first + 1, mid, last - 1, then the Hoare
    scan of __unguarded_partition as ranks (L: the positions with key >= pivot,
    ascending; R: those with key <= pivot, descending; pair k swaps while L[k] < R[k]);
  * a segment still longer than 16 when the counter is 0 is heap-sorted
    (__partial_sort = __make_heap + __sort_heap, serial);
  * __final_insertion_sort compares strictly, so it is a stable sort by key of what
    the splits and heap sorts left.
"""
import numpy as np

import preprocess_ref as PR

THRESHOLD = 16           # _S_threshold


def _median_to_first(k, v, first, last):
    """std::__move_median_to_first(first, first + 1, mid, last - 1) on the keys k (values v follow)."""
    a, b, c = first + 1, first + (last - first) // 2, last - 1
    if k[a] < k[b]:
        m = b if k[b] < k[c] else (c if k[a] < k[c] else a)
    elif k[a] < k[c]:
        m = a
    elif k[b] < k[c]:
        m = c
    else:
        m = b
    k[first], k[m] = k[m], k[first]
    v[first], v[m] = v[m], v[first]


def _partition(k, v, first, last):
    """std::__unguarded_partition_pivot: returns the cut."""
    _median_to_first(k, v, first, last)
    p = k[first]
    seg = k[first + 1:last]
    L = first + 1 + np.flatnonzero(seg >= p)                 # ascending
    R = (first + 1 + np.flatnonzero(seg <= p))[::-1]         # descending
    m = min(len(L), len(R))
    ns = int(np.count_nonzero(L[:m] < R[:m]))                # a prefix: L rises, R falls
    i_prev, j_prev = (int(L[ns - 1]), int(R[ns - 1])) if ns else (first, last)
    i = min(int(L[ns]) if ns < len(L) else last, j_prev)
    j = max(int(R[ns]) if ns < len(R) else first, i_prev)
    assert not i < j
    a, b = L[:ns], R[:ns]
    k[a], k[b] = k[b].copy(), k[a].copy()
    v[a], v[b] = v[b].copy(), v[a].copy()
    return i


def _adjust_heap(k, v, first, hole, n, kv, vv):
    """std::__adjust_heap followed by its __push_heap."""
    top = hole
    child = hole
    while child < (n - 1) // 2:
        child = 2 * (child + 1)
        if k[first + child] < k[first + child - 1]:
            child -= 1
        k[first + hole], v[first + hole] = k[first + child], v[first + child]
        hole = child
    if (n & 1) == 0 and child == (n - 2) // 2:
        child = 2 * (child + 1)
        k[first + hole], v[first + hole] = k[first + child - 1], v[first + child - 1]
        hole = child - 1
    parent = (hole - 1) // 2
    while hole > top and k[first + parent] < kv:
        k[first + hole], v[first + hole] = k[first + parent], v[first + parent]
        hole = parent
        parent = (hole - 1) // 2
    k[first + hole], v[first + hole] = kv, vv


def _heap_sort(k, v, first, last):
    """std::__partial_sort(first, last, last): __make_heap, then __sort_heap."""
    n = last - first
    parent = (n - 2) // 2
    while True:
        _adjust_heap(k, v, first, parent, n, k[first + parent], v[first + parent])
        if parent == 0:
            break
        parent -= 1
    while last - first > 1:
        last -= 1
        kv, vv = k[last], v[last]
        k[last], v[last] = k[first], v[first]
        _adjust_heap(k, v, first, 0, last - first, kv, vv)


def sort_order(keys):
    """(perm, stats) of std::sort on the pairs (keys[i], i) compared by key.  stats: levels
    (partition levels run), heap_segments, heap_longest."""
    k = np.asarray(keys).astype(np.int64).copy()
    n = len(k)
    v = np.arange(n, dtype=np.int64)
    stats = {"levels": 0, "heap_segments": 0, "heap_longest": 0}
    if n > THRESHOLD:
        depth = 2 * (n.bit_length() - 1)
        segs = [(0, n)]
        while segs:
            if depth == 0:
                for first, last in segs:
                    _heap_sort(k, v, first, last)
                    stats["heap_segments"] += 1
                    stats["heap_longest"] = max(stats["heap_longest"], last - first)
                break
            depth -= 1
            stats["levels"] += 1
            nxt = []
            for first, last in segs:
                cut = _partition(k, v, first, last)
                nxt += [s for s in ((first, cut), (cut, last)) if s[1] - s[0] > THRESHOLD]
            segs = nxt
    return v[np.argsort(k, kind="stable")], stats


def voxel_grid(points, leaf, crop=0.0, centre=(0, 0, 0)):
    """preprocess_ref.voxel_grid with each voxel's float32 sum taken in the order std::sort leaves:
    (centroids float32, counts) in voxel-index order, or None when the grid overflows."""
    p = PR._xyz(points)
    x = p[PR.crop_mask(p, crop, centre) if crop > 0 else PR.finite_mask(p)]
    if len(x) == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int64)
    key, overflow = PR.voxel_keys(x, leaf)
    if overflow:
        return None
    order, _ = sort_order(key)
    _, start, cnt = np.unique(key[order], return_index=True, return_counts=True)
    xs = x[order]
    s32 = np.zeros((len(start), 3), np.float32)
    for k in range(int(cnt.max())):
        runs = np.flatnonzero(cnt > k)
        s32[runs] = s32[runs] + xs[start[runs] + k]
    return s32 / cnt.astype(np.float32)[:, None], cnt.astype(np.int64)


# ---- inputs both test files use -------------------------------------------------------------------
def key_patterns(n, seed=0):
    """name -> n keys (uint32), the patterns of the sort tests."""
    rng = np.random.default_rng(seed + n)
    h = (n + 1) // 2
    up = np.arange(h)
    return {
        "equal": np.full(n, 7),
        "alternating": np.arange(n) % 2 * 3 + 1,
        "ascending": np.arange(n),
        "descending": np.arange(n)[::-1],
        "organ_pipe": np.concatenate([up, up[::-1]])[:n],
        "few_values": rng.integers(0, max(n // 5, 1), n),
        "permutation": rng.permutation(n),
    }


def heap_keys():
    """Reaches the depth limit: 35 heap-sorted segments, the longest 340."""
    return np.concatenate([np.arange(3000) // 3, np.arange(3000)[::-1] // 3])


def line_cloud():
    """A line walked out and back, the return 3 mm off."""
    t = np.linspace(0, 30, 3000)
    line = np.stack([t, 0.3 * t, np.ones_like(t)], 1)
    return np.concatenate([line, line[::-1] + 0.003]).astype(np.float32)
