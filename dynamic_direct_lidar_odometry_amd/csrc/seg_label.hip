// seg_label.hip — the labelling of the range image (cloudSegmentation /
// labelComponents, detection.cpp:510-724) on the device, exact to the host
// breadth-first search (Labeller, segment.hip) in labels and segment count
// (DESIGN.md §11).
//
// The search pushes t from f iff t is a 4-neighbour of f inside the window,
// still unlabelled, and the angle test on their two ranges passes.  The test
// is symmetric in f and t, so while no column wraps (label_device_window_ok)
// the segments are the connected components of an undirected graph on the
// eligible pixels E (label-init 0, inside the window), and:
//   seed       the component's smallest row-major index; feasible components
//              are numbered 1, 2, ... in seed order, the others become 999999;
//   pushed     the component's size n;
//   lines      the distinct rows among the non-seed pixels;
//   max_dist   the largest range in the component (n >= 2; else -1e6);
//   min_z      the minimum over the non-seed pixels of z with z != 0, not NaN,
//              z < 1e6 (else 1e6);
//   max_z      the maximum over the pushes that did not take the minimum (the
//              reference's if / else-if).  Let p be the first push whose z is
//              non-zero, not NaN and not a new strict minimum: from p on max_z
//              is at least every later minimum, so the rest contributes the
//              plain maximum of its non-NaN z.  Only the pushes up to p are
//              replayed in the search's order (k_lbl_replay);
//   residual   the reference's float sum in push order is not reproduced: here
//              the positive residuals of the non-seed pixels are summed in
//              double in row-major order and divided by their count.
// Stages, each one launch over the window (M pixels) unless noted:
//   k_lbl_init     (whole image) E, per-seed statistics reset, the horizontal
//                  runs joined within each wavefront
//   k_lbl_merge    union-find over the remaining left edges and the down edges
//   k_lbl_flatten  key = root (the seed) per window pixel
//   radix sort     (key, pixel): the components' pixels as lists in (seed,
//                  row-major pixel) order -- the sort is stable
//   k_lbl_stats    n, lines, max range, min_z, residual count per component
//   k_lbl_replay   one lane per component that passes the order-free tests
//   k_lbl_fold     the unmarked pixels' z into max_z
//   k_lbl_verdict  feasibility per list entry -> exclusive scan: the segment
//                  number (high word) and the feasible pixels' CSR slot (low)
//   k_lbl_write    labels, CSR, segment count
//   k_lbl_avg      the residual averages, one workgroup per segment; the counts
// Only integer and min / max atomics: the result is bit-identical run to run.
// No workgroup waits for another; every loop's termination is argued where it
// stands.  -ffp-contract=off as the rest.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <vector>

#include "seg_label.hpp"

namespace ddlo {
namespace {

using rt::fail;

constexpr int kRejected = DDLO_SEG_REJECTED;
constexpr int kLblThreads = 256;
constexpr int kAvgBlocks = 64;

// per component, at its seed's pixel index
struct CompStat {
  int start;   // the list position of the seed
  int n, lines, res;
  int maxr, minz, maxz;   // floats in the order-preserving integer code below
  int cand;    // passed the order-free tests: replayed, maxz valid
};

struct LblArgs {
  int H, W, N;
  int r0, r1, c0, c1, ww, M;   // the window (inclusive), its width and pixel count
  EdgeTrig t;
  float theta;
  int valid_point_num, min_line_num, valid_line_num;
  float min_delta_z, max_delta_z, max_distance, max_elevation, sensor_z;
  const float* range;
  const unsigned char* z;
  size_t zs;
  const float* resid;
  const signed char* ground;
  int* label;
  int* parent;            // N: -1 outside E
  CompStat* comp;         // N, valid at seeds
  unsigned char* mark;    // N: pushed by the replay
  int *keys_in, *vals_in; // M: by window pixel
  int *keys, *pix;        // M: sorted; keys[k] == N past the eligible pixels
  int* queue;             // M: a component's replay queue is its own list range
  unsigned long long *scan_in, *scan_out;   // M
  int *seg_off, *seg_pix;
  int* rec;
  double* avg;
  int* partial;           // 2 per workgroup of k_lbl_init: ground, range pixel counts
  int nblocks;            // of k_lbl_init
};

// float <-> int with the floats' order (no NaN): integer atomicMin / atomicMax on the code
__device__ __forceinline__ int enc(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float dec(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__device__ __forceinline__ float z_of(const LblArgs& a, int i) {
  return *reinterpret_cast<const float*>(a.z + (size_t)i * a.zs);
}

__device__ __forceinline__ int window_pixel(const LblArgs& a, int w) {
  const int r = w / a.ww;
  return (a.r0 + r) * a.W + a.c0 + (w - r * a.ww);
}

// Labeller::component's edge test on the ranges of two neighbours
__device__ __forceinline__ bool edge_pass(const LblArgs& a, float rf, float rt, bool vertical) {
  const float d1 = rf < rt ? rt : rf;   // std::max(rf, rt)
  const float d2 = rt < rf ? rt : rf;   // std::min(rf, rt)
  const float sa = vertical ? a.t.sin_y : a.t.sin_x, ca = vertical ? a.t.cos_y : a.t.cos_x;
  const float y = d2 * sa, x = d1 - d2 * ca;
  if (a.t.tan_ok && x > 0.f) {
    const double ratio = (double)y / (double)x;
    if (ratio > a.t.tan_hi) return true;
    if (ratio < a.t.tan_lo) return false;
  }
  // atan2f taken as the rounded double result, as k_seg_pixels' ground test does
  return (float)atan2((double)y, (double)x) > a.theta;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}

// E, the per-seed statistics' reset, and the horizontal runs: a pixel joined
// to its left neighbour starts as a child of its run's first pixel within the
// wavefront (a ballot and a bit scan), so the merge kernel is left with the
// runs' joins across wavefront boundaries and the vertical edges, and no tree
// starts deeper than one level.  Also the ground / range pixel counts, as one
// partial per workgroup (k_lbl_avg adds them up in order: no atomics).
__global__ __launch_bounds__(kLblThreads) void k_lbl_init(LblArgs a) {
  __shared__ int sh[2][kLblThreads / 64];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int ground = 0, ranged = 0;
  bool e = false, left = false;
  if (i < a.N) {
    const int r = i / a.W, c = i - r * a.W;
    e = r >= a.r0 && r <= a.r1 && c >= a.c0 && c <= a.c1 && a.label[i] == DDLO_SEG_UNLABELLED;
    const float ri = a.range[i];
    left = e && c > a.c0 && a.label[i - 1] == DDLO_SEG_UNLABELLED && edge_pass(a, a.range[i - 1], ri, false);
    a.mark[i] = 0;
    if (e) a.comp[i] = CompStat{0, 0, 0, 0, enc(-1e6f), enc(1e6f), enc(-1e6f), 0};
    if (a.ground) {
      ground = a.ground[i] == 1;
      ranged = ri > 0.f;
    }
  }
  // the nearest lane at or below mine that is not joined to its left (lane 0 if the run began in the wavefront before)
  const unsigned long long open = ~__ballot(left) & ((2ull << lane) - 1ull);
  const int first = open ? 63 - __clzll((long long)open) : 0;
  if (i < a.N) a.parent[i] = e ? i - (lane - first) : -1;
  if (!a.ground) return;   // (uniform)
  ground = wave_sum(ground);
  ranged = wave_sum(ranged);
  if (lane == 0) {
    sh[0][threadIdx.x >> 6] = ground;
    sh[1][threadIdx.x >> 6] = ranged;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 1; j < kLblThreads / 64; ++j) {
      ground += sh[0][j];
      ranged += sh[1][j];
    }
    a.partial[2 * blockIdx.x] = ground;
    a.partial[2 * blockIdx.x + 1] = ranged;
  }
}

// Union-find.  parent[x] <= x always (a root is only ever hooked under a
// smaller one, and a shortcut points to an ancestor), so a component's final
// root is its smallest index.  Every access to parent inside the merge kernel
// is a relaxed agent-scope atomic: a plain store is not seen across XCDs
// within a kernel.
__device__ __forceinline__ int lbl_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x, halving the path on the way (x's parent becomes its grandparent: still an
// ancestor, and only entries that are not roots are rewritten, so no hook is undone)
__device__ __forceinline__ int lbl_find(int* parent, int x) {
  int p = lbl_load(parent + x);
  while (p != x) {   // terminates: parent[x] < x unless x is a root, so x strictly decreases
    const int gp = lbl_load(parent + p);
    if (gp == p) return p;
    (void)__hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
    p = lbl_load(parent + x);
  }
  return x;
}

__device__ __forceinline__ void lbl_union(int* parent, int a, int b) {
  for (;;) {   // terminates: a failed exchange means another thread hooked a root, which happens fewer than |E| times in all
    a = lbl_find(parent, a);
    b = lbl_find(parent, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    int expect = b;   // hook b under a while b is still a root
    if (__hip_atomic_compare_exchange_strong(parent + b, &expect, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
  }
}

// Each undirected edge once: the left edge of a pixel (k_lbl_init joined it
// already unless the pixel is the first of a wavefront there) and its down
// edge.  A down edge is skipped when the square to its left has its other
// three edges (i-1 ~ i, i-1+W ~ i+W, i-1 ~ i-1+W): the two rows are then
// joined through that square's own down edge.
__global__ __launch_bounds__(kLblThreads) void k_lbl_merge(LblArgs a) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.M) return;
  const int i = window_pixel(a, w);
  // (parent[j] >= 0 is "j is in E": an entry never changes sign)
  if (lbl_load(a.parent + i) < 0) return;
  const int r = i / a.W, c = i - r * a.W;
  const float ri = a.range[i];
  const bool has_left = c > a.c0 && lbl_load(a.parent + i - 1) >= 0;
  const float rl = has_left ? a.range[i - 1] : 0.f;
  const bool left = has_left && edge_pass(a, rl, ri, false);
  if (left && (i & 63) == 0) lbl_union(a.parent, i - 1, i);   // (k_lbl_init's wavefronts start at multiples of 64)
  if (r + 1 <= a.r1 && lbl_load(a.parent + i + a.W) >= 0) {
    const float rd = a.range[i + a.W];
    if (edge_pass(a, ri, rd, true)) {
      bool implied = false;
      if (left && lbl_load(a.parent + i + a.W - 1) >= 0) {
        const float rdl = a.range[i + a.W - 1];
        implied = edge_pass(a, rdl, rd, false) && edge_pass(a, rl, rdl, true);
      }
      if (!implied) lbl_union(a.parent, i, i + a.W);
    }
  }
}

// sort input: (root, pixel) per window pixel in row-major order; pixels outside E get key N and sort last
__global__ __launch_bounds__(kLblThreads) void k_lbl_flatten(LblArgs a) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.M) return;
  const int i = window_pixel(a, w);
  a.keys_in[w] = a.parent[i] < 0 ? a.N : lbl_find(a.parent, i);
  a.vals_in[w] = i;
}

// list entry k: on (in E), its component's seed, its pixel, head (the seed's own entry: the
// smallest pixel of the component comes first)
struct Entry {
  bool on, head;
  int root, pix;
};
__device__ __forceinline__ Entry entry(const LblArgs& a, int k) {
  Entry e{false, false, -1, 0};
  if (k >= a.M) return e;
  const int key = a.keys[k];
  if (key >= a.N) return e;
  e.on = true;
  e.root = key;
  e.pix = a.pix[k];
  e.head = k == 0 || a.keys[k - 1] != key;
  return e;
}
// the wavefront's entries all belong to one component (the common case: the list is sorted by it)
__device__ __forceinline__ bool wave_one_root(int root) { return __all(root == __shfl(root, 0, 64)); }

__global__ __launch_bounds__(kLblThreads) void k_lbl_stats(LblArgs a) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const Entry e = entry(a, k);
  int one = 0, line = 0, res = 0, r = INT_MIN, zmin = INT_MAX;
  if (e.on) {
    one = 1;
    r = enc(a.range[e.pix]);
    if (e.head) {
      a.comp[e.root].start = k;
    } else {
      // the first non-seed pixel of its row (the list is row-major within the component)
      line = (k >= 2 && a.keys[k - 2] == e.root) ? (a.pix[k - 1] / a.W != e.pix / a.W) : 1;
      const float z = z_of(a, e.pix);
      if (z != 0.f && z < 1e6f) zmin = enc(z);   // (a NaN fails z < 1e6)
      res = a.resid && a.resid[e.pix] > 0.f;
    }
  }
  CompStat* c = a.comp + (e.on ? e.root : 0);
  if (wave_one_root(e.root)) {
    if (!e.on) return;   // (uniform)
    one = wave_sum(one);
    line = wave_sum(line);
    res = wave_sum(res);
    r = wave_max(r);
    zmin = wave_min(zmin);
    if ((threadIdx.x & 63) != 0) return;
  } else if (!e.on) {
    return;
  }
  atomicAdd(&c->n, one);
  if (line) atomicAdd(&c->lines, line);
  if (res) atomicAdd(&c->res, res);
  atomicMax(&c->maxr, r);
  if (zmin != INT_MAX) atomicMin(&c->minz, zmin);
}

// the feasibility tests that do not need max_z (the reference evaluates the
// elevation after delta-z, but the conjunction is the same)
__device__ __forceinline__ bool lbl_candidate(const LblArgs& a, const CompStat& c) {
  bool f = false;
  if (c.n >= 50 && c.lines >= a.min_line_num) f = true;
  else if (c.n >= a.valid_point_num && c.lines >= a.valid_line_num) f = true;
  const float max_dist = c.n >= 2 ? dec(c.maxr) : -1e6f;
  if (f) f = max_dist <= a.max_distance;
  if (f) f = dec(c.minz) - a.sensor_z <= a.max_elevation;
  return f;
}

__device__ __forceinline__ bool lbl_feasible(const LblArgs& a, const CompStat& c) {
  if (!c.cand) return false;
  const float dz = dec(c.maxz) - dec(c.minz);
  return a.min_delta_z <= dz && dz <= a.max_delta_z;
}

// The search from the seed, literally (neighbour order (-1,0),(0,1),(0,-1),
// (1,0), the same edge test, "already pushed" marks), until the first push
// whose z is non-zero, not NaN and did not take the minimum -- or the end of
// the component.  One lane per candidate component.
__global__ __launch_bounds__(kLblThreads) void k_lbl_replay(LblArgs a) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const Entry e = entry(a, k);
  if (!e.on || !e.head) return;
  const CompStat c = a.comp[e.root];
  if (!lbl_candidate(a, c)) return;
  int* const q = a.queue + k;   // n slots: entries k .. k + n - 1 are this component's
  int head = 0, tail = 1;
  q[0] = e.root;
  a.mark[e.root] = 1;
  float lit_min = 1e6f, max_z = -1e6f;
  bool stop = false, overflow = false;
  const int dr[4] = {-1, 0, 0, 1}, dc[4] = {0, 1, -1, 0};
  while (head < tail && !stop) {   // terminates: each pass pops one entry and at most n are pushed (a pushed pixel is marked)
    const int f = q[head++];
    const int fy = f / a.W, fx = f - fy * a.W;
    const float rf = a.range[f];
    // the four neighbours' loads are independent: issued together
    int t[4], par[4];
    unsigned char mk[4];
    float rt[4], zt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ty = fy + dr[j], tx = fx + dc[j];
      const bool in = ty >= a.r0 && ty <= a.r1 && tx >= a.c0 && tx <= a.c1;
      t[j] = in ? ty * a.W + tx : f;   // (f itself is marked: skipped below)
      par[j] = a.parent[t[j]];
      mk[j] = a.mark[t[j]];
      rt[j] = a.range[t[j]];
      zt[j] = z_of(a, t[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (stop || par[j] < 0 || mk[j] || !edge_pass(a, rf, rt[j], dr[j] != 0)) continue;
      if (tail >= c.n) {   // cannot happen (a pushed pixel belongs to the component); never write past the range
        overflow = stop = true;
        continue;
      }
      a.mark[t[j]] = 1;
      q[tail++] = t[j];
      const float zz = zt[j];
      if (zz < lit_min && zz != 0.f) {
        lit_min = zz;
      } else {
        if (zz > max_z) max_z = zz;
        if (zz != 0.f && zz == zz) stop = true;
      }
    }
  }
  a.comp[e.root].maxz = enc(max_z);
  a.comp[e.root].cand = 1;
  atomicAdd(a.rec + kRecReplayed, 1);
  atomicMax(a.rec + kRecLongestPrefix, tail - 1);
  if (overflow) atomicOr(a.rec + kRecError, 1);
}

__global__ __launch_bounds__(kLblThreads) void k_lbl_fold(LblArgs a) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const Entry e = entry(a, k);
  int zmax = INT_MIN;
  bool cand = false;
  if (e.on) {
    cand = a.comp[e.root].cand != 0;
    if (cand && !e.head && !a.mark[e.pix]) {
      const float z = z_of(a, e.pix);
      if (z == z) zmax = enc(z);
    }
  }
  if (wave_one_root(e.root)) {
    if (!cand) return;   // (uniform)
    zmax = wave_max(zmax);
    if ((threadIdx.x & 63) != 0) return;
  }
  if (zmax != INT_MIN) atomicMax(&a.comp[e.root].maxz, zmax);
}

// scan input: a feasible component's entries count one pixel each (low word), its head one segment (high word)
__global__ __launch_bounds__(kLblThreads) void k_lbl_verdict(LblArgs a) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.M) return;
  const Entry e = entry(a, k);
  unsigned long long v = 0;
  if (e.on && lbl_feasible(a, a.comp[e.root])) v = (e.head ? 1ull << 32 : 0ull) | 1ull;
  a.scan_in[k] = v;
}

__global__ __launch_bounds__(kLblThreads) void k_lbl_write(LblArgs a) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const Entry e = entry(a, k);
  if (e.on) {
    if (a.scan_in[k]) {
      const unsigned slot = (unsigned)a.scan_out[k];
      const int l = (int)(a.scan_out[a.comp[e.root].start] >> 32) + 1;
      a.label[e.pix] = l;
      a.seg_pix[slot] = e.pix;
      if (e.head) a.seg_off[l] = (int)slot;
    } else {
      a.label[e.pix] = kRejected;
    }
    if (k == a.M - 1 || a.keys[k + 1] >= a.N) a.rec[kRecEligible] = k + 1;   // the last entry in E
  }
  if (k == a.M - 1) {   // the totals
    const unsigned long long tot = a.scan_out[k] + a.scan_in[k];
    const int L = (int)(tot >> 32);
    a.rec[kRecSegments] = L;
    a.seg_off[0] = 0;
    a.seg_off[L + 1] = (int)(unsigned)tot;   // (L == 0: seg_off[1] = 0)
  }
}

// avg[l]: the positive residuals of segment l's pixels without its seed (the
// list's first entry), summed in double in a fixed order -- each thread its
// entries in list order, the wavefront by shuffles, the wavefronts 0..3 from
// LDS, as k_seg_objects sums -- over their count
__global__ __launch_bounds__(kLblThreads) void k_lbl_avg(LblArgs a) {
  __shared__ double sh_s[kLblThreads / 64];
  __shared__ int sh_m[kLblThreads / 64], sh_c[2][kLblThreads / 64];
  const int L = a.rec[kRecSegments];
  if (blockIdx.x == 0) {   // the counts: rejected = |E| - the feasible segments' pixels; k_lbl_init's partials in order
    int ground = 0, ranged = 0;
    if (a.ground)
      for (int j = threadIdx.x; j < a.nblocks; j += kLblThreads) {
        ground += a.partial[2 * j];
        ranged += a.partial[2 * j + 1];
      }
    ground = wave_sum(ground);
    ranged = wave_sum(ranged);
    if ((threadIdx.x & 63) == 0) {
      sh_c[0][threadIdx.x >> 6] = ground;
      sh_c[1][threadIdx.x >> 6] = ranged;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int j = 1; j < kLblThreads / 64; ++j) {
        ground += sh_c[0][j];
        ranged += sh_c[1][j];
      }
      a.rec[kRecGround] = ground;
      a.rec[kRecRange] = ranged;
      a.rec[kRecRejected] = a.rec[kRecEligible] - a.seg_off[L + 1];
      a.avg[0] = 0.0;
    }
  }
  for (int l = blockIdx.x + 1; l <= L; l += gridDim.x) {   // (uniform per workgroup)
    double s = 0.0;
    int m = 0;
    if (a.resid)
      for (int i = a.seg_off[l] + 1 + (int)threadIdx.x; i < a.seg_off[l + 1]; i += kLblThreads) {
        const float r = a.resid[a.seg_pix[i]];
        if (r > 0.f) {
          s += (double)r;
          ++m;
        }
      }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      s += __shfl_down(s, d, 64);
      m += __shfl_down(m, d, 64);
    }
    __syncthreads();   // the previous segment's reader is done with sh
    if ((threadIdx.x & 63) == 0) {
      sh_s[threadIdx.x >> 6] = s;
      sh_m[threadIdx.x >> 6] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int j = 1; j < kLblThreads / 64; ++j) {
        s += sh_s[j];
        m += sh_m[j];
      }
      a.avg[l] = m > 0 ? s / (double)m : 0.0;
    }
  }
}

template <bool FLAGS>
__global__ __launch_bounds__(kLblThreads) void k_lbl_drop(const int* __restrict__ ids, const int* __restrict__ off,
                                                          const int* __restrict__ pix, float4* __restrict__ pts,
                                                          unsigned char* __restrict__ flags) {
  const int l = ids[blockIdx.y];
  for (int i = off[l] + blockIdx.x * blockDim.x + threadIdx.x; i < off[l + 1]; i += gridDim.x * blockDim.x) {
    pts[pix[i]] = make_float4(NAN, NAN, NAN, FLAGS ? 0.f : kRemovedW);   // (a pixel named twice: the same bits)
    if (FLAGS) flags[pix[i]] = 1;
  }
}

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

}  // namespace

bool label_device_window_ok(const ddlo_seg_params& p) { return p.win_col0 >= 0 && p.win_col1 <= p.cols - 1; }

gicp_status label_device_run(hipStream_t s, const ddlo_seg_params& p, LabelDev& w, const LabelDevIn& in) {
  if (!label_device_window_ok(p))
    return fail(GICP_EINVAL, "device labelling needs 0 <= win_col0 and win_col1 <= cols - 1");
  LblArgs a{};
  a.H = p.rows;
  a.W = p.cols;
  a.N = p.rows * p.cols;
  a.r0 = std::max(0, p.win_row0);
  a.r1 = std::min(p.rows - 1, p.win_row1);
  a.c0 = p.win_col0;
  a.c1 = p.win_col1;
  a.ww = std::max(0, a.c1 - a.c0 + 1);
  a.M = a.ww * std::max(0, a.r1 - a.r0 + 1);
  a.t = edge_trig(p);
  a.theta = p.theta;
  a.valid_point_num = p.valid_point_num;
  a.min_line_num = p.min_line_num;
  a.valid_line_num = p.valid_line_num;
  a.min_delta_z = p.min_delta_z;
  a.max_delta_z = p.max_delta_z;
  a.max_distance = p.max_distance;
  a.max_elevation = p.max_elevation;
  a.sensor_z = in.sensor_z;
  a.range = in.range;
  a.z = in.z;
  a.zs = in.z_stride;
  a.resid = in.resid;
  a.ground = in.ground;
  a.label = in.label;
  const size_t N = (size_t)a.N, M = std::max<size_t>((size_t)a.M, 1);
  int bits = 1;   // of the keys 0 .. N
  while ((1ll << bits) <= (long long)N) ++bits;
  size_t sort_b = 0, scan_b = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, (const unsigned*)nullptr, (unsigned*)nullptr,
                                             (const int*)nullptr, (int*)nullptr, (int)M, 0, bits, s));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, (const unsigned long long*)nullptr,
                                           (unsigned long long*)nullptr, (int)M, s));
  // (grown once per image / window size: later frames find every buffer large enough)
  HIP_TRY(rt::grow(w.parent, sizeof(int) * N, s));
  HIP_TRY(rt::grow(w.comp, sizeof(CompStat) * N, s));
  HIP_TRY(rt::grow(w.mark, N, s));
  HIP_TRY(rt::grow(w.keys_in, sizeof(int) * M, s));
  HIP_TRY(rt::grow(w.vals_in, sizeof(int) * M, s));
  HIP_TRY(rt::grow(w.keys, sizeof(int) * M, s));
  HIP_TRY(rt::grow(w.pix, sizeof(int) * M, s));
  HIP_TRY(rt::grow(w.queue, sizeof(int) * M, s));
  HIP_TRY(rt::grow(w.scan_in, sizeof(unsigned long long) * M, s));
  HIP_TRY(rt::grow(w.scan_out, sizeof(unsigned long long) * M, s));
  HIP_TRY(rt::grow(w.cubtmp, std::max<size_t>(std::max(sort_b, scan_b), 256), s));
  HIP_TRY(rt::grow(w.seg_off, sizeof(int) * (M + 2), s));
  HIP_TRY(rt::grow(w.seg_pix, sizeof(int) * M, s));
  // (at least kLabelRecMinBytes: the caller reads the head of the record with one fixed-size copy)
  HIP_TRY(rt::grow(w.rec, std::max<size_t>(sizeof(int) * kLabelRecInts + sizeof(double) * (M + 1), kLabelRecMinBytes), s));
  a.parent = w.parent.as<int>();
  a.comp = w.comp.as<CompStat>();
  a.mark = w.mark.as<unsigned char>();
  a.keys_in = w.keys_in.as<int>();
  a.vals_in = w.vals_in.as<int>();
  a.keys = w.keys.as<int>();
  a.pix = w.pix.as<int>();
  a.queue = w.queue.as<int>();
  a.scan_in = w.scan_in.as<unsigned long long>();
  a.scan_out = w.scan_out.as<unsigned long long>();
  a.seg_off = w.off();
  a.seg_pix = w.pixels();
  a.rec = w.ints();
  a.avg = w.avg();
  a.nblocks = cdiv((long)N, kLblThreads);
  HIP_TRY(rt::grow(w.partial, sizeof(int) * 2 * (size_t)a.nblocks, s));
  a.partial = w.partial.as<int>();
  // the record's ints, avg[0], seg_off[0 .. 1]: all zero for an empty window
  HIP_TRY(hipMemsetAsync(w.rec.p, 0, sizeof(int) * kLabelRecInts + sizeof(double), s));
  HIP_TRY(hipMemsetAsync(w.seg_off.p, 0, 2 * sizeof(int), s));
  k_lbl_init<<<a.nblocks, kLblThreads, 0, s>>>(a);
  if (a.M > 0) {
    const int g = cdiv(a.M, kLblThreads);
    k_lbl_merge<<<g, kLblThreads, 0, s>>>(a);
    k_lbl_flatten<<<g, kLblThreads, 0, s>>>(a);
    size_t tmp = w.cubtmp.bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(w.cubtmp.p, tmp, (const unsigned*)a.keys_in, (unsigned*)a.keys,
                                               (const int*)a.vals_in, a.pix, a.M, 0, bits, s));
    k_lbl_stats<<<g, kLblThreads, 0, s>>>(a);
    k_lbl_replay<<<g, kLblThreads, 0, s>>>(a);
    k_lbl_fold<<<g, kLblThreads, 0, s>>>(a);
    k_lbl_verdict<<<g, kLblThreads, 0, s>>>(a);
    tmp = w.cubtmp.bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(w.cubtmp.p, tmp, (const unsigned long long*)a.scan_in, a.scan_out, a.M, s));
    k_lbl_write<<<g, kLblThreads, 0, s>>>(a);
  }
  k_lbl_avg<<<kAvgBlocks, kLblThreads, 0, s>>>(a);   // (an empty window: the counts alone)
  HIP_TRY(hipGetLastError());
  return GICP_OK;
}

gicp_status label_device_drop(hipStream_t s, const LabelDev& w, const int* ids, int nids, float4* pts,
                              unsigned char* flags) {
  if (nids <= 0) return GICP_OK;
  if (flags) k_lbl_drop<true><<<dim3(8, nids), kLblThreads, 0, s>>>(ids, w.off(), w.pixels(), pts, flags);
  else k_lbl_drop<false><<<dim3(8, nids), kLblThreads, 0, s>>>(ids, w.off(), w.pixels(), pts, nullptr);
  HIP_TRY(hipGetLastError());
  return GICP_OK;
}

}  // namespace ddlo

using namespace ddlo;

extern "C" gicp_status ddlo_seg_label_device(int device, const ddlo_seg_params* p, const float* range, const float* z,
                                             const float* residual, float sensor_z, int32_t* label,
                                             double* avg_residual, size_t avg_cap, int32_t* segments) {
  if (gicp_status st = seg_check_params(p)) return st;
  if (!range || !z || !label || (!avg_residual && avg_cap)) return fail(GICP_EINVAL, "invalid argument");
  if (!label_device_window_ok(*p))
    return fail(GICP_EINVAL, "device labelling needs 0 <= win_col0 and win_col1 <= cols - 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(GICP_EHIP, "no HIP device " + std::to_string(device) + " (HIP library present, device not visible)");
  HIP_TRY(hipSetDevice(device));
  const size_t n = (size_t)p->rows * p->cols;
  rt::DevBuf drange, dz, dres, dlabel;
  HIP_TRY(drange.ensure(sizeof(float) * n));
  HIP_TRY(dz.ensure(sizeof(float) * n));
  HIP_TRY(dlabel.ensure(sizeof(int) * n));
  if (residual) HIP_TRY(dres.ensure(sizeof(float) * n));
  hipStream_t s = nullptr;   // the null stream: the copies below are synchronous with it
  HIP_TRY(hipMemcpy(drange.p, range, sizeof(float) * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dz.p, z, sizeof(float) * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dlabel.p, label, sizeof(int) * n, hipMemcpyHostToDevice));
  if (residual) HIP_TRY(hipMemcpy(dres.p, residual, sizeof(float) * n, hipMemcpyHostToDevice));
  LabelDev w;
  LabelDevIn in{drange.as<float>(), dz.as<unsigned char>(), sizeof(float), residual ? dres.as<float>() : nullptr,
                nullptr,            dlabel.as<int>(),       sensor_z};
  if (gicp_status st = label_device_run(s, *p, w, in)) return st;
  int rec[kLabelRecInts];
  HIP_TRY(hipMemcpy(rec, w.rec.p, sizeof(rec), hipMemcpyDeviceToHost));
  if (rec[kRecError]) return fail(GICP_EHIP, "device labelling: a replay queue left its component's range");
  HIP_TRY(hipMemcpy(label, dlabel.p, sizeof(int) * n, hipMemcpyDeviceToHost));
  const size_t navg = (size_t)rec[kRecSegments] + 1;
  std::vector<double> avg(navg);
  HIP_TRY(hipMemcpy(avg.data(), w.avg(), sizeof(double) * navg, hipMemcpyDeviceToHost));
  for (size_t l = 0; l < avg_cap; ++l) avg_residual[l] = l < navg ? avg[l] : 0.0;
  if (segments) *segments = rec[kRecSegments];
  return GICP_OK;
}
