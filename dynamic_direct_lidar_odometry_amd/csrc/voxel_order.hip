// voxel_order.hip — the permutation libstdc++'s std::sort leaves on pairs
// (key_i, i) compared by key alone, on the device: the summation order of
// pcl::VoxelGrid (DDLO_VOXEL_ORDER_PCL; DESIGN.md "PCL-order voxel filter").
//
// std::__sort = __introsort_loop + __final_insertion_sort (bits/stl_algo.h).
// The final pass compares strictly, so it is a stable sort by key of the
// array the introsort loop left: the caller's radix sort.  This file does the
// loop, in place on (keys, idx)[0, ns):
//
//   k_order_setup    ns and the depth limit 2 * floor(log2(ns)) (device words)
//   k_order_level    one level of the recursion for the segments longer than
//                    kHandOver: a workgroup per segment, __move_median_to_first
//                    by one thread, then __unguarded_partition as two ranks
//                    (L: positions with key >= pivot ascending, R: key <= pivot
//                    descending), pair k swaps while L[k] < R[k], the cut is
//                    min(L[nswap], R[nswap - 1]); the children go to the next
//                    level's table or, once they fit, to the hand-over table
//   k_order_tail     the same for the levels past the launched ones, one
//                    workgroup looping over them (adversarial inputs only)
//   k_order_finish   a wavefront per handed-over segment, in LDS: the rest of
//                    its recursion level by level, one lane per sub-segment
//                    running libstdc++'s statements (Hoare scan; at depth 0
//                    __make_heap + __sort_heap), then the write-back
//
// All segments of one level share one depth counter (both halves of a split
// inherit what is left), so the level index is the counter.  Every loop is
// bounded by a segment length or the depth counter, never by the data alone.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <vector>

#include "../../include/ddlo_odom.h"
#include "launch.hpp"
#include "runtime.hpp"

namespace ddlo {

namespace {
constexpr int kInsertion = 16;                 // _S_threshold: a segment this short is left alone
constexpr int kHandOver = kVoxelOrderHandOver; // S: a segment this short finishes in LDS
constexpr int kLevelThreads = 1024;
constexpr int kLevelBlocks = 256;
constexpr int kFinishBlocks = 1024;
constexpr int kMaxTasks = kHandOver / (kInsertion + 1) + 2;   // disjoint sub-segments longer than 16
// control words
enum { C_NS = 0, C_DEPTH = 1, C_NFIN = 2, C_LEVELS = 3, C_GLEVELS = 4, C_LDS = 5, C_HEAPS = 6, C_HEAPMAX = 7,
       C_OVERFLOW = 8, C_LVL = 16 };
constexpr int kCtlInts = C_LVL + 80;           // per-level segment counts: levels 0 .. 2 * 31 + 1

inline int cdiv_i(long a, long b) { return (int)((a + b - 1) / b); }
inline int lg2(int n) { return 31 - __builtin_clz((unsigned)std::max(n, 1)); }

struct OrderBufs {
  int* ctl;
  int* lpos;      // [n]
  int* rpos;      // [n]
  int* lvl[2];    // [cap_l][2] each: (first, last) of the segments of an even / odd level
  int* fin;       // [cap_f][3]: (first, last, depth left)
  int cap_l, cap_f;
};
inline int cap_level(int n) { return n / kHandOver + 2; }
inline int cap_finish(int n) { return n / (kInsertion + 1) + 2; }
inline OrderBufs carve(int* scratch, int n) {
  OrderBufs b;
  b.cap_l = cap_level(n);
  b.cap_f = cap_finish(n);
  b.ctl = scratch;
  b.lpos = b.ctl + kCtlInts;
  b.rpos = b.lpos + n;
  b.lvl[0] = b.rpos + n;
  b.lvl[1] = b.lvl[0] + 2 * b.cap_l;
  b.fin = b.lvl[1] + 2 * b.cap_l;
  return b;
}

// ---- libstdc++'s statements on one lane (k, v: LDS or global) ----------------
__device__ __forceinline__ void swap_kv(unsigned* k, int* v, int a, int b) {
  const unsigned tk = k[a];
  const int tv = v[a];
  k[a] = k[b];
  v[a] = v[b];
  k[b] = tk;
  v[b] = tv;
}

// std::__move_median_to_first(first, first + 1, mid, last - 1), stl_algo.h:79-97
__device__ __forceinline__ void median_to_first(unsigned* k, int* v, int first, int last) {
  const int a = first + 1, b = first + (last - first) / 2, c = last - 1;
  const unsigned ka = k[a], kb = k[b], kc = k[c];
  int m;
  if (ka < kb) m = kb < kc ? b : (ka < kc ? c : a);
  else if (ka < kc) m = a;
  else if (kb < kc) m = c;
  else m = b;
  swap_kv(k, v, first, m);
}

// std::__unguarded_partition_pivot: the cut.  The scans stop at the segment's
// ends whatever the keys are; the outer loop runs at most once per element.
__device__ int partition_serial(unsigned* k, int* v, int first, int last) {
  median_to_first(k, v, first, last);
  const unsigned p = k[first];
  int i = first + 1, j = last;
  for (int it = first; it < last; ++it) {
    while (i < last && k[i] < p) ++i;
    --j;
    while (j > first && p < k[j]) --j;
    if (!(i < j)) break;
    swap_kv(k, v, i, j);
    ++i;
  }
  return min(max(i, first), last);
}

// std::__adjust_heap with its __push_heap, stl_heap.h:134-146, 223-248
__device__ void adjust_heap(unsigned* k, int* v, int hole, int n, unsigned kv, int vv) {
  const int top = hole;
  int child = hole;
  while (child < (n - 1) / 2) {          // child at least doubles: bounded by n
    child = 2 * (child + 1);
    if (k[child] < k[child - 1]) child--;
    k[hole] = k[child];
    v[hole] = v[child];
    hole = child;
  }
  if ((n & 1) == 0 && child == (n - 2) / 2) {
    child = 2 * (child + 1);
    k[hole] = k[child - 1];
    v[hole] = v[child - 1];
    hole = child - 1;
  }
  int parent = (hole - 1) / 2;
  while (hole > top && k[parent] < kv) {   // hole falls towards top
    k[hole] = k[parent];
    v[hole] = v[parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  k[hole] = kv;
  v[hole] = vv;
}

// std::__partial_sort(first, last, last): __make_heap, then __sort_heap (stl_heap.h:339-361, 418-428)
__device__ void heap_sort(unsigned* k, int* v, int n) {
  if (n < 2) return;
  for (int parent = (n - 2) / 2; parent >= 0; --parent) adjust_heap(k, v, parent, n, k[parent], v[parent]);
  for (int last = n - 1; last > 0; --last) {
    const unsigned kv = k[last];
    const int vv = v[last];
    k[last] = k[0];
    v[last] = v[0];
    adjust_heap(k, v, 0, last, kv, vv);
  }
}

// ---- setup ---------------------------------------------------------------------
// ns = n, or the compaction's count pos[n - 1] + keep[n - 1]; ctl arrives zeroed
__global__ void k_order_setup(int n, const int* __restrict__ pos, const int* __restrict__ keep, OrderBufs b) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int ns = pos ? pos[n - 1] + keep[n - 1] : n;
  const int depth = ns > 1 ? 2 * (31 - __clz(ns)) : 0;
  b.ctl[C_NS] = ns;
  b.ctl[C_DEPTH] = depth;
  if (ns <= kInsertion) return;
  if (ns > kHandOver) {
    b.lvl[0][0] = 0;
    b.lvl[0][1] = ns;
    b.ctl[C_LVL] = 1;
  } else {
    b.fin[0] = 0;
    b.fin[1] = ns;
    b.fin[2] = depth;
    b.ctl[C_NFIN] = 1;
    b.ctl[C_LDS] = 1;
  }
}

__global__ __launch_bounds__(256) void k_key_flags(const unsigned* __restrict__ key, int n, int* __restrict__ keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keep[i] = key[i] != 0xffffffffu ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_compact_pairs(const unsigned* __restrict__ key, const int* __restrict__ idx, int n,
                                                       const int* __restrict__ keep, const int* __restrict__ pos,
                                                       unsigned* __restrict__ ck, int* __restrict__ ci) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !keep[i]) return;
  ck[pos[i]] = key[i];
  ci[pos[i]] = idx[i];
}
__global__ __launch_bounds__(256) void k_iota(int n, int* __restrict__ idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) idx[i] = i;
}

// ---- global levels ----------------------------------------------------------------
// a control or table word another thread of this kernel may have written (k_order_tail runs
// several levels in one launch): read past any cached copy
__device__ __forceinline__ int ld_fresh(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void push_finish(const OrderBufs& b, int first, int last, int depth) {
  const int slot = atomicAdd(&b.ctl[C_NFIN], 1);
  if (slot < b.cap_f) {
    b.fin[3 * slot] = first;
    b.fin[3 * slot + 1] = last;
    b.fin[3 * slot + 2] = depth;
  } else {
    b.ctl[C_OVERFLOW] = 1;
  }
}

// one child of a split at level lev (depth left after it: depth)
__device__ void publish(const OrderBufs& b, int first, int last, int lev, int depth) {
  const int len = last - first;
  if (len <= kInsertion) return;
  if (len <= kHandOver) {
    push_finish(b, first, last, depth);
    atomicAdd(&b.ctl[C_LDS], 1);
    return;
  }
  const int slot = atomicAdd(&b.ctl[C_LVL + lev + 1], 1);
  if (slot < b.cap_l) {
    b.lvl[(lev + 1) & 1][2 * slot] = first;
    b.lvl[(lev + 1) & 1][2 * slot + 1] = last;
  } else {
    b.ctl[C_OVERFLOW] = 1;
  }
}

// Level lev for the segments blk, blk + nblk, ... of its table, by one
// workgroup of kLevelThreads.  Returns the level's segment count.
__device__ int level_pass(unsigned* __restrict__ keys, int* __restrict__ idx, const OrderBufs& b, int lev, int blk,
                          int nblk) {
  __shared__ unsigned s_wave[kLevelThreads / 64];
  __shared__ unsigned s_pivot;
  __shared__ int s_nswap;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int nseg = min(ld_fresh(&b.ctl[C_LVL + lev]), b.cap_l);
  const int depth = b.ctl[C_DEPTH] - lev;          // what is left of the depth limit before this level
  const int* const tab = b.lvl[lev & 1];
  for (int seg = blk; seg < nseg; seg += nblk) {
    const int first = ld_fresh(&tab[2 * seg]), last = ld_fresh(&tab[2 * seg + 1]);
    if (depth <= 0) {   // the depth limit: the segment is heap-sorted as it stands (k_order_finish)
      if (t == 0) push_finish(b, first, last, 0);
      continue;
    }
    if (t == 0) {
      median_to_first(keys, idx, first, last);
      s_pivot = keys[first];
      s_nswap = 0;
    }
    __syncthreads();
    const unsigned p = s_pivot;
    const int m = last - first - 1;                // the elements of [first + 1, last)
    int nl = 0, nr = 0;
    for (int base = 0; base < m; base += kLevelThreads) {
      const int e = base + t;
      const bool fl = e < m && keys[first + 1 + e] >= p;
      const bool fr = e < m && keys[last - 1 - e] <= p;
      // both counts in one scan: a chunk holds at most 1024 of each
      unsigned incl = (fl ? 1u : 0u) | (fr ? 0x10000u : 0u);
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
      }
      if (lane == 63) s_wave[w] = incl;
      __syncthreads();
      unsigned before = 0, total = 0;
      for (int q = 0; q < kLevelThreads / 64; ++q) {
        const unsigned x = s_wave[q];
        if (q < w) before += x;
        total += x;
      }
      incl += before;
      if (fl) b.lpos[first + nl + (int)(incl & 0xffffu) - 1] = first + 1 + e;
      if (fr) b.rpos[first + nr + (int)(incl >> 16) - 1] = last - 1 - e;
      nl += (int)(total & 0xffffu);
      nr += (int)(total >> 16);
      __syncthreads();
    }
    // the pairs that swap: a prefix (L rises, R falls), all disjoint
    const int npair = min(nl, nr);
    int mine = 0;
    for (int k = t; k < npair; k += kLevelThreads) {
      const int a = b.lpos[first + k], c = b.rpos[first + k];
      if (a < c) {
        swap_kv(keys, idx, a, c);
        ++mine;
      }
    }
    if (mine) atomicAdd(&s_nswap, mine);
    __syncthreads();
    if (t == 0) {
      const int ns = s_nswap;
      const int j_prev = ns > 0 ? b.rpos[first + ns - 1] : last;
      const int i = ns < nl ? b.lpos[first + ns] : INT_MAX;
      const int cut = min(max(min(i, j_prev), first), last);
      publish(b, first, cut, lev, depth - 1);
      publish(b, cut, last, lev, depth - 1);
      atomicMax(&b.ctl[C_LEVELS], lev + 1);
      atomicMax(&b.ctl[C_GLEVELS], lev + 1);
    }
    __syncthreads();
  }
  return nseg;
}

__global__ __launch_bounds__(kLevelThreads) void k_order_level(unsigned* __restrict__ keys, int* __restrict__ idx,
                                                               OrderBufs b, int lev) {
  (void)level_pass(keys, idx, b, lev, blockIdx.x, gridDim.x);
}

// levels lev0 .. lev1 by one workgroup (its own writes are visible to it after the barrier)
__global__ __launch_bounds__(kLevelThreads) void k_order_tail(unsigned* __restrict__ keys, int* __restrict__ idx,
                                                              OrderBufs b, int lev0, int lev1) {
  for (int lev = lev0; lev <= lev1; ++lev) {
    __threadfence();
    __syncthreads();
    if (level_pass(keys, idx, b, lev, 0, 1) == 0) break;   // no segment here: none later either
  }
}

// ---- the finish in LDS ---------------------------------------------------------------
__global__ __launch_bounds__(64) void k_order_finish(unsigned* __restrict__ keys, int* __restrict__ idx, OrderBufs b) {
  __shared__ unsigned sk[kHandOver];
  __shared__ int sv[kHandOver];
  __shared__ int task[2][kMaxTasks][2];
  __shared__ int ntask[2];
  const int lane = threadIdx.x;
  const int nfin = min(b.ctl[C_NFIN], b.cap_f);
  const int limit = b.ctl[C_DEPTH];
  for (int s = blockIdx.x; s < nfin; s += gridDim.x) {
    const int first = b.fin[3 * s], last = b.fin[3 * s + 1], depth0 = b.fin[3 * s + 2];
    const int len = last - first;
    if (len > kHandOver) {   // only at the depth limit: heap-sorted where it lies
      if (lane == 0) {
        heap_sort(keys + first, idx + first, len);
        atomicAdd(&b.ctl[C_HEAPS], 1);
        atomicMax(&b.ctl[C_HEAPMAX], len);
      }
      continue;
    }
    for (int e = lane; e < len; e += 64) {
      sk[e] = keys[first + e];
      sv[e] = idx[first + e];
    }
    if (lane == 0) {
      task[0][0][0] = 0;
      task[0][0][1] = len;
      ntask[0] = 1;
      ntask[1] = 0;
    }
    __syncthreads();
    int cur = 0;
    for (int depth = depth0; depth >= 0; --depth) {   // the depth counter bounds the levels
      const int nt = min(ntask[cur], kMaxTasks);
      if (nt == 0) break;
      if (depth == 0) {
        for (int q = lane; q < nt; q += 64) {
          const int f = task[cur][q][0], l = task[cur][q][1];
          heap_sort(sk + f, sv + f, l - f);
          atomicAdd(&b.ctl[C_HEAPS], 1);
          atomicMax(&b.ctl[C_HEAPMAX], l - f);
        }
        break;
      }
      for (int q = lane; q < nt; q += 64) {
        const int f = task[cur][q][0], l = task[cur][q][1];
        const int cut = partition_serial(sk, sv, f, l);
        if (cut - f > kInsertion) {
          const int slot = atomicAdd(&ntask[cur ^ 1], 1);
          if (slot < kMaxTasks) {
            task[cur ^ 1][slot][0] = f;
            task[cur ^ 1][slot][1] = cut;
          }
        }
        if (l - cut > kInsertion) {
          const int slot = atomicAdd(&ntask[cur ^ 1], 1);
          if (slot < kMaxTasks) {
            task[cur ^ 1][slot][0] = cut;
            task[cur ^ 1][slot][1] = l;
          }
        }
      }
      if (lane == 0) atomicMax(&b.ctl[C_LEVELS], limit - depth + 1);
      __syncthreads();
      if (lane == 0) ntask[cur] = 0;
      cur ^= 1;
      __syncthreads();
    }
    __syncthreads();
    for (int e = lane; e < len; e += 64) {
      keys[first + e] = sk[e];
      idx[first + e] = sv[e];
    }
    __syncthreads();
  }
}

}  // namespace

size_t voxel_order_scratch_ints(int n) {
  const size_t m = (size_t)std::max(n, 1);
  // compacted keys and indices, then launch_sort_order's own
  return 2 * m + sort_order_scratch_ints(n);
}
size_t sort_order_scratch_ints(int n) {
  const int m = std::max(n, 1);
  return (size_t)kCtlInts + 2 * (size_t)m + 4 * (size_t)cap_level(m) + 3 * (size_t)cap_finish(m);
}

// The introsort loop of std::sort on (keys, idx)[0, ns), in place; ns = n, or
// with pos / keep (a compaction's exclusive sum and flags over n) their count,
// read on the device.  A stable sort by key afterwards completes std::sort.
// scratch: sort_order_scratch_ints(n); its first ints are the control words.
void launch_sort_order(hipStream_t s, unsigned* keys, int* idx, int n, const int* pos, const int* keep, int* scratch) {
  if (n <= 0) return;
  const OrderBufs b = carve(scratch, n);
  (void)hipMemsetAsync(b.ctl, 0, sizeof(int) * kCtlInts, s);
  k_order_setup<<<1, 64, 0, s>>>(n, pos, keep, b);
  if (n <= kInsertion) return;
  if (n > kHandOver) {
    // level lev exists for lev <= the depth limit <= 2 floor(log2 n) (the last one only hands over).
    // A median-of-three split of n halves about log2(n / S) times; the launches cover that and
    // eight levels more, one workgroup takes whatever an adversarial input has beyond them.
    const int lmax = 2 * lg2(n);
    const int launched = std::min(lmax + 1, lg2(cdiv_i(n, kHandOver)) + 1 + 8);
    const int blocks = std::min(b.cap_l, kLevelBlocks);
    for (int lev = 0; lev < launched; ++lev) k_order_level<<<blocks, kLevelThreads, 0, s>>>(keys, idx, b, lev);
    if (launched <= lmax) k_order_tail<<<1, kLevelThreads, 0, s>>>(keys, idx, b, launched, lmax);
  }
  k_order_finish<<<std::min(cap_finish(n), kFinishBlocks), 64, 0, s>>>(keys, idx, b);
}

// the voxel filter's part: the pairs whose key is not UINT_MAX (the points in
// the pass) compacted in input order into ck / ci, whose tails keep UINT_MAX /
// 0, and permuted.  oscratch: voxel_order_scratch_ints(n).
int voxel_order_pairs(hipStream_t s, const unsigned* keys, const int* idx, int n, int* oscratch, void* tmp,
                      size_t tmp_bytes, unsigned** ck_out, int** ci_out) {
  unsigned* ck = reinterpret_cast<unsigned*>(oscratch);
  int* ci = oscratch + n;
  int* rest = ci + n;
  const OrderBufs b = carve(rest, n);
  int* keep = b.lpos;   // free until the levels run
  int* pos = b.rpos;
  (void)hipMemsetAsync(ck, 0xff, sizeof(unsigned) * (size_t)n, s);
  (void)hipMemsetAsync(ci, 0, sizeof(int) * (size_t)n, s);
  k_key_flags<<<cdiv_i(n, 256), 256, 0, s>>>(keys, n, keep);
  size_t need = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, need, keep, pos, n, s);
  if (need > tmp_bytes) return -2;
  (void)hipcub::DeviceScan::ExclusiveSum(tmp, need, keep, pos, n, s);
  k_compact_pairs<<<cdiv_i(n, 256), 256, 0, s>>>(keys, idx, n, keep, pos, ck, ci);
  launch_sort_order(s, ck, ci, n, pos, keep, rest);
  *ck_out = ck;
  *ci_out = ci;
  return 0;
}

}  // namespace ddlo

extern "C" gicp_status ddlo_debug_sort_order(int device, const uint32_t* keys, size_t n, int32_t* perm_out,
                                             ddlo_sort_order_stats* stats_out) {
  if ((!keys && n) || (!perm_out && n) || n > (size_t)INT32_MAX / 2) return fail(GICP_EINVAL, "invalid argument");
  HIP_TRY(hipSetDevice(device));
  if (stats_out) {
    *stats_out = ddlo_sort_order_stats{};
    stats_out->threshold = kHandOver;
  }
  if (n == 0) return GICP_OK;
  const int N = (int)n;
  DevBuf k, v, ks, vs, scratch, tmp;
  HIP_TRY(k.ensure(sizeof(unsigned) * n));
  HIP_TRY(v.ensure(sizeof(int) * n));
  HIP_TRY(ks.ensure(sizeof(unsigned) * n));
  HIP_TRY(vs.ensure(sizeof(int) * n));
  HIP_TRY(scratch.ensure(sizeof(int) * sort_order_scratch_ints(N)));
  size_t need = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, k.as<unsigned>(), ks.as<unsigned>(), v.as<int>(), vs.as<int>(),
                                             N, 0, 32, (hipStream_t)0));
  HIP_TRY(tmp.ensure(std::max<size_t>(need, 16)));
  hipStream_t s = nullptr;
  HIP_TRY(hipMemcpyAsync(k.p, keys, sizeof(unsigned) * n, hipMemcpyHostToDevice, s));
  k_iota<<<cdiv_i(N, 256), 256, 0, s>>>(N, v.as<int>());
  launch_sort_order(s, k.as<unsigned>(), v.as<int>(), N, nullptr, nullptr, scratch.as<int>());
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, need, k.as<unsigned>(), ks.as<unsigned>(), v.as<int>(), vs.as<int>(), N,
                                             0, 32, s));
  HIP_TRY(hipGetLastError());
  int ctl[kCtlInts];
  HIP_TRY(hipMemcpyAsync(perm_out, vs.p, sizeof(int) * n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(ctl, scratch.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (ctl[C_OVERFLOW]) return fail(GICP_EHIP, "sort order: a segment table overflowed");
  if (stats_out) {
    stats_out->levels = ctl[C_LEVELS];
    stats_out->global_levels = ctl[C_GLEVELS];
    stats_out->lds_segments = ctl[C_LDS];
    stats_out->heap_segments = ctl[C_HEAPS];
    stats_out->heap_longest = ctl[C_HEAPMAX];
  }
  return GICP_OK;
}
