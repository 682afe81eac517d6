// covariance.hip — K2 of the GICP hot path: exact kNN-k and the regularised
// neighbourhood covariances.
//
//   K2 kNN-k covariance k_covariances<KCAP,EXACT>,      calculate_covariances
//                       k_covariances2 (two lanes per   nano_gicp_impl.hpp:373-441
//                       query, k = 10 / 20),
//                       k_knn_query (external queries),
//                       k_cov_import / export / remap
// Compiled with -ffp-contract=off (see index_build.hip).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gicp_types.hpp"
#include "search.hpp"
#include "cov_math.hpp"
#include "launch.hpp"
#include "launch_util.hpp"

namespace ddlo {

// ============================================================================
// K2: exact kNN-k (self queries) + covariance
// ============================================================================
// Kept-neighbour list storage: registers, or (KLDS: k up to 64, where a
// register list of 64 u64 keys spilled 213 VGPRs) a lane-interleaved LDS
// array, slot s of a lane at p[64 s].
template <int KCAP, bool KLDS>
struct KeyList {
  unsigned long long v[KCAP];
  __device__ __forceinline__ unsigned long long& operator[](int s) { return v[s]; }
  __device__ __forceinline__ const unsigned long long& operator[](int s) const { return v[s]; }
};
template <int KCAP>
struct KeyList<KCAP, true> {
  unsigned long long* p;   // the lane's slot 0 (LDS)
  __device__ __forceinline__ unsigned long long& operator[](int s) { return p[64 * s]; }
  __device__ __forceinline__ const unsigned long long& operator[](int s) const { return p[64 * s]; }
};

// Compare-exchange of two 64-bit keys: slot = min(key, slot), key = the
// larger, from ONE compare.  Written out because the compiler turns the two
// selects of one predicate into umin + umax and lowers each with its own
// 64-bit compare (9 instructions and a twice as long dependent chain per slot
// of the insertion network that bounds a kNN leaf scan).  The s_nop covers the
// VALU-writes-VCC -> v_cndmask hazard, as the compiler's own code does.
__device__ __forceinline__ void cmp_exchange_u64(unsigned long long& key, unsigned long long& slot) {
  const unsigned long long a = key, b = slot;
  unsigned lo0, lo1, hi0, hi1;
  asm volatile(
      "v_cmp_lt_u64_e32 vcc, %[a], %[b]\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e32 %[lo0], %[b0], %[a0], vcc\n\t"
      "v_cndmask_b32_e32 %[lo1], %[b1], %[a1], vcc\n\t"
      "v_cndmask_b32_e32 %[hi0], %[a0], %[b0], vcc\n\t"
      "v_cndmask_b32_e32 %[hi1], %[a1], %[b1], vcc"
      : [lo0] "=&v"(lo0), [lo1] "=&v"(lo1), [hi0] "=&v"(hi0), [hi1] "=&v"(hi1)
      : [a] "v"(a), [b] "v"(b), [a0] "v"((unsigned)a), [a1] "v"((unsigned)(a >> 32)), [b0] "v"((unsigned)b),
        [b1] "v"((unsigned)(b >> 32))
      : "vcc");
  slot = ((unsigned long long)lo1 << 32) | lo0;
  key = ((unsigned long long)hi1 << 32) | hi0;
}

template <int KCAP, bool EXACT, bool KLDS = false>
struct KnnVisitor : VisitStats {
  WaveBox box;
  float qx, qy, qz;
  bool active;
  int k;
  // kept neighbours as order-preserving (squared distance, sorted position)
  // keys, ascending: the exact rule (d < D) || (d == D && j < J) of
  // KNNResultSet + the position tie-break is one u64 compare per slot
  KeyList<KCAP, KLDS> K;
  unsigned long long wk;   // worst kept key (bound)
  float wd;                // its distance
  float tight;             // min over the tested full leaves of the farthest-corner distance (squared)
  float td;                // smallest distance of an examined point that is not kept (tie detection:
                           // the k-th distance is tied iff it equals td at the end)
  int nfull;               // leaves < nfull hold 32 real points (>= k: each such box bounds the k-th neighbour)
  int skip_lo, skip_hi;

  __device__ __forceinline__ float dist(int s) const { return __uint_as_float((unsigned)(K[s] >> 32)); }
  __device__ __forceinline__ int idx(int s) const { return (int)(unsigned)K[s]; }
  __device__ __forceinline__ void init(int kk) {
    k = kk;
#pragma unroll
    for (int s = 0; s < KCAP; ++s) K[s] = dkey(INFINITY, -1);
    wk = K[0];
    wd = INFINITY;
    tight = INFINITY;
    td = INFINITY;
    nfull = 0;
    skip_lo = 1;
    skip_hi = 0;
  }
  // k-th distance (slot k - 1) and whether an examined point outside the
  // kept k lies at exactly that distance (nanoflann then keeps the one its
  // walk met first)
  __device__ __forceinline__ float kth_dist() const {
    float d = INFINITY;
#pragma unroll
    for (int s = 0; s < KCAP; ++s)
      if (s == k - 1) d = dist(s);
    return d;
  }
  __device__ __forceinline__ float outside_min() const {   // td, plus slot k of an oversized list
    float t = td;
    if constexpr (!EXACT) {
#pragma unroll
      for (int s = 0; s < KCAP; ++s)
        if (s == k) t = fminf(t, dist(s));
    }
    return t;
  }
  // any two of the kept k at the same distance (their order is nanoflann's walk order)
  __device__ __forceinline__ bool inner_tie() const {
    bool t = false;
#pragma unroll
    for (int s = 1; s < KCAP; ++s)
      if (s < k) t |= dist(s) == dist(s - 1);
    return t;
  }
  // the slot j of the one equal-distance pair (j, j + 1) among the kept k, -1
  // if there are more (or three at one distance)
  __device__ __forceinline__ int single_pair() const {
    int cnt = 0, j = -1;
#pragma unroll
    for (int s = 1; s < KCAP; ++s)
      if (s < k && dist(s) == dist(s - 1)) {
        ++cnt;
        j = s - 1;
      }
    return cnt == 1 ? j : -1;
  }
  __device__ __forceinline__ void update_worst() {
    if constexpr (EXACT) {
      wk = K[KCAP - 1];
    } else {
#pragma unroll
      for (int s = 0; s < KCAP; ++s)
        if (s == k - 1) wk = K[s];
    }
    wd = __uint_as_float((unsigned)(wk >> 32));
  }
  __device__ __forceinline__ void insert(unsigned long long key) {
    if constexpr (KLDS) {   // sorted shift from the end (the list lives in LDS)
      const unsigned long long out = K[KCAP - 1];
      if (key >= out) {
        td = fminf(td, key_dist(key));
        return;
      }
      int s = KCAP - 1;
      for (; s > 0; --s) {
        const unsigned long long prev = K[s - 1];
        if (prev <= key) break;
        K[s] = prev;
      }
      K[s] = key;
      td = fminf(td, key_dist(out));   // the key pushed out of the list
    } else {
#pragma unroll
      for (int s = 0; s < KCAP; ++s) cmp_exchange_u64(key, K[s]);
      td = fminf(td, key_dist(key));   // the key pushed out of the list
    }
    update_worst();
  }
  // the k-th neighbour is no farther than the kept k-th key, nor than the
  // farthest corner of any full leaf (32 >= k real points inside)
  __device__ __forceinline__ float bound() const { return fminf(wd, tight); }
  __device__ __forceinline__ bool need(float4 lo, float4 hi) const { return box_dist2(qx, qy, qz, lo, hi) <= bound(); }
  __device__ __forceinline__ void note_leaf(f4v lo, f4v hi, int leaf) {
    if (leaf < nfull && active) tight = fminf(tight, box_maxdist2(qx, qy, qz, lo, hi));
  }
  __device__ __forceinline__ void process(const WaveLds* L, int start) {
    for (int j = 0; j < kLeafSize; ++j) {
      const float d = dist2(qx, qy, qz, L->px[j], L->py[j], L->pz[j]);
      const unsigned long long key = dkey(d, start + j);
      // d > tight: not among the k nearest.  Only an active lane's examined
      // points count for td: an inactive lane (another sub-range of a split
      // group) re-scans leaves whose points it may already keep.
      if (active && key < wk && d <= tight) insert(key);
      else td = fminf(td, active ? d : INFINITY);   // (a select: a second branch cost 24 VGPRs in k_covariances2)
    }
  }
  __device__ __forceinline__ void scan_leaf(const CloudDev& c, int leaf, WaveLds* L) {
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane_id() < kLeafSize) p = ldg4(c.pts, leaf * kLeafSize + lane_id());
    stage_points<KnnVisitor>(L, p);
    process(L, leaf * kLeafSize);
  }
  __device__ __forceinline__ bool scan_leaves(const CloudDev& c, int base, unsigned long long ex, WaveLds* L) {
    return scan_leaves_lds(c, base, ex, *this, L);
  }
};

// Mean and biased covariance of the kept neighbours in their order
// (nano_gicp_impl.hpp:392-399), regularised.  The neighbour points are loaded
// four at a time (compiler barriers between the groups): with all KCAP loads
// hoisted, k = 20 held 20 float4s live and spilled.  swap >= 0: slots swap and
// swap + 1 exchanged (cov_order_free).
template <int KCAP, class KL>
__device__ __forceinline__ void cov_compute(const CloudDev& c, const KL& K, int k, int method, int swap, double* out) {
  unsigned long long ka = 0, kb = 0;   // the swapped pair's keys (slot selects, no runtime index into the list)
  if (swap >= 0) {
#pragma unroll
    for (int s = 0; s < KCAP; ++s) {
      if (s == swap) ka = K[s];
      if (s == swap + 1) kb = K[s];
    }
  }
  auto slot_pos = [&](int s) -> int {
    const unsigned long long v = swap < 0 ? K[s] : (s == swap ? kb : (s == swap + 1 ? ka : K[s]));
    return (int)(unsigned)v;
  };
  double mx = 0, my = 0, mz = 0;
#pragma unroll
  for (int s = 0; s < KCAP; ++s) {
    if (s < k) {
      const float4 p = ldg4(c.pts, slot_pos(s));
      mx += (double)p.x;
      my += (double)p.y;
      mz += (double)p.z;
    }
    if ((s & 3) == 3) asm volatile("" ::: "memory");
  }
  mx /= k;
  my /= k;
  mz /= k;
  double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < KCAP; ++s) {
    if (s < k) {
      const float4 p = ldg4(c.pts, slot_pos(s));
      const double d0 = (double)p.x - mx, d1 = (double)p.y - my, d2 = (double)p.z - mz;
      C[0] += d0 * d0; C[1] += d0 * d1; C[2] += d0 * d2;
      C[3] += d1 * d0; C[4] += d1 * d1; C[5] += d1 * d2;
      C[6] += d2 * d0; C[7] += d2 * d1; C[8] += d2 * d2;
    }
    if ((s & 3) == 3) asm volatile("" ::: "memory");
  }
  for (int e = 0; e < 9; ++e) C[e] /= k;
  regularize(C, method, out);
}
template <int KCAP, class KL>
__device__ __forceinline__ void cov_from_keys(const CloudDev& c, const KL& K, int k, int method, double* o) {
  double out[6];
  cov_compute<KCAP>(c, K, k, method, -1, out);
  for (int e = 0; e < 6; ++e) o[e] = out[e];
}

// An inner tie whose order cannot change the result: the covariance with the
// tied neighbours j and j + 1 exchanged (the other order nanoflann's walk may
// have met them in) equals the one stored from the Morton order, bit for bit
// after the regularisation.  Then the stored result is nanoflann's whatever
// its order, and the query needs no re-run.
template <int KCAP, class KL>
__device__ __forceinline__ bool cov_order_free(const CloudDev& c, const KL& K, int k, int method, int j, const double* stored) {
  double out[6];
  cov_compute<KCAP>(c, K, k, method, j, out);
  bool same = true;
  for (int e = 0; e < 6; ++e) same = same && __double_as_longlong(out[e]) == __double_as_longlong(stored[e]);
  return same;
}

// Seed a kNN visitor with the leaves [s0, s1] and then run the full traversal.
template <int KCAP, bool EXACT, bool KLDS>
__device__ __forceinline__ void knn_search(const CloudDev& c, KnnVisitor<KCAP, EXACT, KLDS>& vis, int s0, int s1,
                                           WaveLds* L) {
  s0 = max(s0, 0);
  s1 = min(s1, c.cnt0 - 1);
  for (int l = s0; l <= s1; ++l) vis.scan_leaf(c, l, L);
  vis.skip_lo = s0;
  vis.skip_hi = s1;
  vis.box = make_wave_box(vis.active, vis.qx, vis.qy, vis.qz, vis.wd);
  traverse(c, vis, L);
}

// kNN-k of the cloud's own points: seed with the group's own leaves, then a
// split search (keys = the cloud's sorted Morton keys)
template <int KCAP, bool EXACT, bool KLDS>
__device__ __forceinline__ void knn_self_search(const CloudDev& c, KnnVisitor<KCAP, EXACT, KLDS>& vis, int s0, int s1,
                                                unsigned long long key, WaveLds* L) {
  s0 = max(s0, 0);
  s1 = min(s1, c.cnt0 - 1);
  for (int l = s0; l <= s1; ++l) {
    vis.scan_leaf(c, l, L);
    const float4 lo = ldg4(c.box_lo, l), hi = ldg4(c.box_hi, l);   // the seed leaves' boxes bound the k-th too
    vis.note_leaf(f4v{lo.x, lo.y, lo.z, 0.f}, f4v{hi.x, hi.y, hi.z, 0.f}, l);
  }
  vis.skip_lo = s0;
  vis.skip_hi = s1;
  split_search(c, vis, key, L);
}

// covariances of a cloud: wave w handles sorted points [64w, 64w+64) (leaves 2w, 2w+1)
template <int KCAP, bool EXACT>
__global__ __launch_bounds__(256) void k_covariances(CloudDev c, int k, int method, double* __restrict__ cov6,
                                                     const unsigned char* __restrict__ redo, TieList ties) {
  constexpr bool KLDS = KCAP > 32;
  __shared__ WaveLds lds[4];
  __shared__ unsigned long long klist[KLDS ? 4 * 64 * KCAP : 1];   // KLDS: the kept lists (128 KB at k <= 64)
  WaveLds* L = &lds[threadIdx.x >> 6];
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves_total = (gridDim.x * blockDim.x) >> 6;
  const int ngroups = (c.n + 63) >> 6;
  for (int g = wave; g < ngroups; g += nwaves_total) {
    if (redo && !redo[g]) continue;   // only the groups the task path could not finish
    const int i = g * 64 + lane_id();
    KnnVisitor<KCAP, EXACT, KLDS> vis;
    if constexpr (KLDS) vis.K.p = klist + (size_t)(threadIdx.x >> 6) * 64 * KCAP + lane_id();
    vis.init(k);
    vis.nfull = k <= kLeafSize ? c.n / kLeafSize : 0;   // a full leaf holds >= k points only if k <= 32
    vis.active = i < c.n;
    const float4 q = ldg4(c.pts, min(i, c.n - 1));
    vis.qx = q.x;
    vis.qy = q.y;
    vis.qz = q.z;
    knn_self_search(c, vis, 2 * g - 1, 2 * g + 2, gp(c.keys)[min(i, c.n - 1)], L);
    if (!vis.active) continue;
    // a tie at the k-th distance changes the set; one inside the k changes the
    // summation order, which the eigen-decomposition of a degenerate
    // (isotropic) neighbourhood turns into a different regularized covariance
    const bool kth_tie = vis.outside_min() == vis.kth_dist(), inner = vis.inner_tie();
    cov_from_keys<KCAP>(c, vis.K, k, method, cov6 + 6 * (size_t)i);
    if (ties.list && (kth_tie || inner)) {
      const int j = kth_tie ? -1 : vis.single_pair();
      if (j < 0 || !cov_order_free<KCAP>(c, vis.K, k, method, j, cov6 + 6 * (size_t)i)) ties.push(i);
    }
  }
}

// Two lanes per query (lanes l and l + 32, 32 queries per wave): twice the
// wavefronts of k_covariances for the same cloud, and half the serial scan
// per lane.  Each half keeps the exact top-k of its half of every leaf's
// points (positions 0-15 / 16-31); the k-th key of either half bounds the
// k-th of the union (k real points lie within it), so a point is inserted
// only below BOTH halves' k-th keys and a leaf is tested against the smaller
// bound.  At the end the two lists are merged: the union's exact top-k.
// The partner lane's word from a permlane32 swap of (v, v): one of the two
// results is the lane's own word, the other the partner's (equal words make
// the choice immaterial), whatever order the builtin returns them in.
template <class R>
__device__ __forceinline__ unsigned swap_partner(const R& r, unsigned own) { return r[0] == own ? r[1] : r[0]; }

template <int KCAP, bool EXACT>
struct KnnVisitor2 : KnnVisitor<KCAP, EXACT> {
  using Base = KnnVisitor<KCAP, EXACT>;
  unsigned long long wk_other = ~0ull;   // the other half's k-th key
#ifdef DDLO_COV_PROF
  // s_memtime cycles: waiting for a leaf's points, scanning them, a leaf block's box tests
  unsigned long long pt_last = 0, pt_wait = 0, pt_proc = 0, pt_box = 0;
  __device__ __forceinline__ void prof_mark(int k) {
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    if (k == 1) pt_wait += t - pt_last;
    else if (k == 2) pt_proc += t - pt_last;
    else if (k == 4) pt_box += t - pt_last;
    pt_last = t;
  }
#endif
  __device__ __forceinline__ unsigned long long wk_both() const { return umin64(this->wk, wk_other); }
  __device__ __forceinline__ float bound() const {
    return fminf(__uint_as_float((unsigned)(wk_both() >> 32)), this->tight);
  }
  __device__ __forceinline__ bool need(float4 lo, float4 hi) const {
    return box_dist2(this->qx, this->qy, this->qz, lo, hi) <= bound();
  }
  __device__ __forceinline__ void exchange() {   // whole wave: wk of lane l ^ 32
    const unsigned lo = (unsigned)this->wk, hi = (unsigned)(this->wk >> 32);
    const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    wk_other = ((unsigned long long)swap_partner(rh, hi) << 32) | swap_partner(rl, lo);
  }
  // The staged points are read four at a time (one 16-byte LDS read per
  // axis): a per-point loop waited for one LDS round trip per point.  For
  // k = 20 the insertion test is also evaluated without short-circuit
  // branches, with the halves' bound (wk_both) kept in registers and
  // refreshed only after an insertion: k = 20 0.59 -> 0.53 ms per 131k-point
  // scan, while k = 10 measured 3 % slower that way (tools/gpu_r6_x.sh).
  __device__ __forceinline__ void process(const WaveLds* L, int start) {
    const int h0 = (lane_id() >> 5) * (kLeafSize / 2);
    const bool act = this->active;
    unsigned long long wkb = wk_both();
    for (int j0 = 0; j0 < kLeafSize / 2; j0 += 4) {
      const f4v X = *reinterpret_cast<const f4v*>(&L->px[h0 + j0]);
      const f4v Y = *reinterpret_cast<const f4v*>(&L->py[h0 + j0]);
      const f4v Z = *reinterpret_cast<const f4v*>(&L->pz[h0 + j0]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float d = dist2(this->qx, this->qy, this->qz, X[u], Y[u], Z[u]);
        const unsigned long long key = dkey(d, start + h0 + j0 + u);
        if constexpr (KCAP > 16) {
          const bool ins = act & (key < wkb) & (d <= this->tight);
          if (ins) {
            this->insert(key);
            wkb = wk_both();
          }
          this->td = fminf(this->td, (act & !ins) ? d : INFINITY);   // active lanes only (see KnnVisitor::process)
        } else {
          if (act && key < wk_both() && d <= this->tight) this->insert(key);
          else this->td = fminf(this->td, act ? d : INFINITY);   // active lanes only (see KnnVisitor::process)
        }
      }
    }
    exchange();
  }
  __device__ __forceinline__ void scan_leaf(const CloudDev& c, int leaf, WaveLds* L) {
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane_id() < kLeafSize) p = ldg4(c.pts, leaf * kLeafSize + lane_id());
    stage_points<KnnVisitor2>(L, p);
    process(L, leaf * kLeafSize);
  }
  __device__ __forceinline__ bool scan_leaves(const CloudDev& c, int base, unsigned long long ex, WaveLds* L) {
    return scan_leaves_lds(c, base, ex, *this, L);
  }
  // whole wave: lanes 0-31 merge their partner's list (lane + 32) into their
  // own; lanes 32-63 keep theirs unchanged, so the partner word each swap
  // returns is still the partner's original list entry (no copy of the list)
  __device__ __forceinline__ void merge_halves() {
    const bool low = lane_id() < 32;
#pragma unroll
    for (int s = 0; s < KCAP; ++s) {
      const unsigned lo = (unsigned)this->K[s], hi = (unsigned)(this->K[s] >> 32);
      const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
      const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
      const unsigned long long other = ((unsigned long long)swap_partner(rh, hi) << 32) | swap_partner(rl, lo);
      if (low) {
        if (other < this->wk) this->insert(other);
        else this->td = fminf(this->td, key_dist(other));
      }
    }
    // both halves' discarded points: the union's
    const unsigned tb = __float_as_uint(this->td);
    const auto rt = __builtin_amdgcn_permlane32_swap(tb, tb, false, false);
    this->td = fminf(__uint_as_float(rt[0]), __uint_as_float(rt[1]));
  }
};

// developer build (-DDDLO_COV_PROF): per 32-query group of k_covariances2,
// (start, end) s_memrealtime stamps (100 MHz), leaves scanned / exact-tested,
// splits, the hardware wave slot and the group's largest k-th distance
// (tools/cov_timeline.py reads them through ddlo_dev_cov_prof)
#ifdef DDLO_COV_PROF
constexpr int kCovProfGroups = 8192;
__device__ unsigned long long g_cov_prof[kCovProfGroups * 4];
__device__ unsigned long long g_cov_prof2[kCovProfGroups * 4];   // cycles: point wait, scan, box tests; blocks
#endif

// covariances with two lanes per query: wave w handles sorted points
// [32w, 32w+32) (leaf w); seeds leaves w-1 .. w+1.  Waves per SIMD: k = 10
// fits 3 (128 VGPRs); k = 20 runs at 2 (158 VGPRs, no spills; at 3 it spilled)
template <int KCAP>
constexpr int kCov2Waves = KCAP <= 10 ? 3 : 2;
template <int KCAP, bool EXACT>
__global__ __launch_bounds__(256, kCov2Waves<KCAP>) void k_covariances2(CloudDev c, int k, int method, double* __restrict__ cov6,
                                                            TieList ties) {
  __shared__ WaveLds lds[4];
  WaveLds* L = &lds[threadIdx.x >> 6];
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves_total = (gridDim.x * blockDim.x) >> 6;
  const int ngroups = (c.n + 31) >> 5;
  for (int g = wave; g < ngroups; g += nwaves_total) {
#ifdef DDLO_COV_PROF
    const unsigned long long cp_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    const int i = g * 32 + (lane_id() & 31);
    KnnVisitor2<KCAP, EXACT> vis;
    vis.init(k);
    vis.wk_other = ~0ull;
    vis.nfull = k <= kLeafSize ? c.n / kLeafSize : 0;
    vis.active = i < c.n;
    const float4 q = ldg4(c.pts, min(i, c.n - 1));
    vis.qx = q.x;
    vis.qy = q.y;
    vis.qz = q.z;
    {
      // the seed leaves with the next one's points in flight (as scan_leaves_lds)
      const int s0 = max(g - 1, 0), s1 = min(g + 1, c.cnt0 - 1);
      float4 pn = lane_id() < kLeafSize ? ldg4(c.pts, s0 * kLeafSize + lane_id()) : make_float4(0.f, 0.f, 0.f, 0.f);
      for (int l = s0; l <= s1; ++l) {
        const float4 p = pn;
        if (l < s1 && lane_id() < kLeafSize) pn = ldg4(c.pts, (l + 1) * kLeafSize + lane_id());
        const float4 lo = ldg4(c.box_lo, l), hi = ldg4(c.box_hi, l);
        stage_points<KnnVisitor2<KCAP, EXACT>>(L, p);
        vis.process(L, l * kLeafSize);
        vis.note_leaf(f4v{lo.x, lo.y, lo.z, 0.f}, f4v{hi.x, hi.y, hi.z, 0.f}, l);
      }
      vis.skip_lo = s0;
      vis.skip_hi = s1;
      split_search<KnnVisitor2<KCAP, EXACT>, 32>(c, vis, gp(c.keys)[min(i, c.n - 1)], L);
    }
    vis.merge_halves();
#ifdef DDLO_COV_PROF
    {
      const float kd = wave_max(vis.active && lane_id() < 32 ? vis.kth_dist() : 0.f);
      const unsigned long long cp_t1 = __builtin_amdgcn_s_memrealtime();
      if (lane_id() == 0 && g < kCovProfGroups) {
        unsigned long long* o2 = g_cov_prof2 + (size_t)g * 4;
        o2[0] = vis.pt_wait;
        o2[1] = vis.pt_proc;
        o2[2] = vis.pt_box;
        o2[3] = vis.st_blocks;
        unsigned long long* o = g_cov_prof + (size_t)g * 4;
        o[0] = cp_t0;
        o[1] = cp_t1;
        o[2] = (unsigned long long)vis.st_scan | ((unsigned long long)vis.st_exact << 32);
        o[3] = (unsigned long long)__float_as_uint(kd) | ((unsigned long long)vis.st_splits << 32) |
               ((unsigned long long)(__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) & 0xffff) << 40);
      }
    }
#endif
    if (!vis.active || lane_id() >= 32) continue;
    const bool kth_tie = vis.td == vis.kth_dist(), inner = vis.inner_tie();
    cov_from_keys<KCAP>(c, vis.K, k, method, cov6 + 6 * (size_t)i);
    if (ties.list && (kth_tie || inner)) {   // rare: a tie whose order matters is re-run (nftree.hip)
      bool push = true;
      if constexpr (KCAP <= 16) {   // (k = 20: a second covariance spills at the 3-wave budget; re-run them all)
        const int j = kth_tie ? -1 : vis.single_pair();
        if (j >= 0) push = !cov_order_free<KCAP>(c, vis.K, k, method, j, cov6 + 6 * (size_t)i);
      }
      if (push) ties.push(i);
    }
  }
}
template __global__ void k_covariances2<10, true>(CloudDev, int, int, double*, TieList);
template __global__ void k_covariances2<20, true>(CloudDev, int, int, double*, TieList);

// kNN of external queries (any order) against a cloud; outputs original indices.
template <int KCAP, bool EXACT>
__global__ __launch_bounds__(256) void k_knn_query(CloudDev c, const float4* __restrict__ q, int nq, int k,
                                                   int* __restrict__ out_idx, float* __restrict__ out_d, TieList ties) {
  constexpr bool KLDS = KCAP >= 32;   // a register list of 32 keys spilled here (156 VGPRs)
  __shared__ WaveLds lds[4];
  __shared__ unsigned long long klist[KLDS ? 4 * 64 * KCAP : 1];
  WaveLds* L = &lds[threadIdx.x >> 6];
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves_total = (gridDim.x * blockDim.x) >> 6;
  const int ngroups = (nq + 63) >> 6;
  for (int g = wave; g < ngroups; g += nwaves_total) {
    const int i = g * 64 + lane_id();
    KnnVisitor<KCAP, EXACT, KLDS> vis;
    if constexpr (KLDS) vis.K.p = klist + (size_t)(threadIdx.x >> 6) * 64 * KCAP + lane_id();
    vis.init(k);
    vis.nfull = k <= kLeafSize ? c.n / kLeafSize : 0;   // a full leaf holds >= k points only if k <= 32
    vis.active = i < nq;
    const float4 p = ldg4(q, min(i, nq - 1));
    vis.qx = p.x;
    vis.qy = p.y;
    vis.qz = p.z;
    // seed around the Morton position of the first lane's query
    const float sx = uniform_f(p.x), sy = uniform_f(p.y), sz = uniform_f(p.z);
    const int pos = wave_lower_bound(c.keys, c.n, morton_key(sx, sy, sz, c.quant));
    const int leaf = min(pos, c.n - 1) / kLeafSize;
    knn_search(c, vis, leaf - 1, leaf + 1, L);
    if (!vis.active) continue;
    if (ties.list && (vis.outside_min() == vis.kth_dist() || vis.inner_tie())) ties.push(i);
#pragma unroll
    for (int s = 0; s < KCAP; ++s) {
      if (s < k) {
        const int j = vis.idx(s);
        out_idx[(size_t)i * k + s] = j >= 0 ? c.perm[j] : -1;
        out_d[(size_t)i * k + s] = vis.dist(s);
      }
    }
  }
}


template __global__ void k_covariances<10, true>(CloudDev, int, int, double*, const unsigned char*, TieList);
template __global__ void k_covariances<20, true>(CloudDev, int, int, double*, const unsigned char*, TieList);
template __global__ void k_covariances<16, false>(CloudDev, int, int, double*, const unsigned char*, TieList);
template __global__ void k_covariances<32, false>(CloudDev, int, int, double*, const unsigned char*, TieList);
template __global__ void k_covariances<64, false>(CloudDev, int, int, double*, const unsigned char*, TieList);
template __global__ void k_knn_query<1, true>(CloudDev, const float4*, int, int, int*, float*, TieList);
template __global__ void k_knn_query<10, true>(CloudDev, const float4*, int, int, int*, float*, TieList);
template __global__ void k_knn_query<20, true>(CloudDev, const float4*, int, int, int*, float*, TieList);
template __global__ void k_knn_query<16, false>(CloudDev, const float4*, int, int, int*, float*, TieList);
template __global__ void k_knn_query<32, false>(CloudDev, const float4*, int, int, int*, float*, TieList);
template __global__ void k_knn_query<64, false>(CloudDev, const float4*, int, int, int*, float*, TieList);

// covariance import/export between original order (host layout) and sorted sym6
__global__ __launch_bounds__(256) void k_cov_import(const double* __restrict__ in, int layout, int n,
                                                    const int* __restrict__ inv_perm, double* __restrict__ cov6) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // original index
  if (i >= n) return;
  double* o = cov6 + 6 * (size_t)inv_perm[i];
  if (layout == 0) {  // MAT4D row-major
    const double* m = in + 16 * (size_t)i;
    o[0] = m[0]; o[1] = m[1]; o[2] = m[2]; o[3] = m[5]; o[4] = m[6]; o[5] = m[10];
  } else {
    const double* m = in + 6 * (size_t)i;
    for (int e = 0; e < 6; ++e) o[e] = m[e];
  }
}
__global__ __launch_bounds__(256) void k_cov_export(const double* __restrict__ cov6, int layout, int n,
                                                    const int* __restrict__ perm, double* __restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;  // sorted index
  if (s >= n) return;
  const double* c = cov6 + 6 * (size_t)s;
  const int i = perm[s];
  if (layout == 0) {
    double* m = out + 16 * (size_t)i;
    m[0] = c[0]; m[1] = c[1]; m[2] = c[2]; m[3] = 0;
    m[4] = c[1]; m[5] = c[3]; m[6] = c[4]; m[7] = 0;
    m[8] = c[2]; m[9] = c[4]; m[10] = c[5]; m[11] = 0;
    m[12] = 0; m[13] = 0; m[14] = 0; m[15] = 0;
  } else {
    double* m = out + 6 * (size_t)i;
    for (int e = 0; e < 6; ++e) m[e] = c[e];
  }
}

// registerInputSource keeps source_covs_ (nano_gicp_impl.hpp:122-130): the
// covariance of original index o moves from the old cloud's sorted position
// to the new one's
__global__ __launch_bounds__(256) void k_cov_remap(const double* __restrict__ old_cov6,
                                                   const int* __restrict__ old_inv_perm,
                                                   const int* __restrict__ new_perm, int n, double* __restrict__ cov6) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;   // new sorted index
  if (s >= n) return;
  const double* src = old_cov6 + 6 * (size_t)old_inv_perm[new_perm[s]];
  double* o = cov6 + 6 * (size_t)s;
  for (int e = 0; e < 6; ++e) o[e] = src[e];
}

bool launch_covariances(hipStream_t s, const CloudDev& c, int k, int method, double* cov6, const unsigned char* redo,
                        TieList ties) {
  const int nb = group_blocks(c.n);
  static const int two_lanes = env_knob("DDLO_COV_2LANE", 1);   // two lanes per query (A/B)
  if (two_lanes && !redo && (k == 10 || k == 20)) {
    const int nb2 = std::max(1, std::min(cdiv(cdiv(c.n, 32), 4), 8192));
    if (k == 10) k_covariances2<10, true><<<nb2, 256, 0, s>>>(c, k, method, cov6, ties);
    else k_covariances2<20, true><<<nb2, 256, 0, s>>>(c, k, method, cov6, ties);
    return true;
  }
  if (k == 10) k_covariances<10, true><<<nb, 256, 0, s>>>(c, k, method, cov6, redo, ties);
  else if (k == 20) k_covariances<20, true><<<nb, 256, 0, s>>>(c, k, method, cov6, redo, ties);
  else if (k <= 16) k_covariances<16, false><<<nb, 256, 0, s>>>(c, k, method, cov6, redo, ties);
  else if (k <= 32) k_covariances<32, false><<<nb, 256, 0, s>>>(c, k, method, cov6, redo, ties);
  else if (k <= 64) k_covariances<64, false><<<nb, 256, 0, s>>>(c, k, method, cov6, redo, ties);
  else return false;
  return true;
}
bool launch_knn_query(hipStream_t s, const CloudDev& c, const float4* q, int nq, int k, int* out_idx, float* out_d,
                      TieList ties) {
  const int nb = group_blocks(nq);
  if (k == 1) k_knn_query<1, true><<<nb, 256, 0, s>>>(c, q, nq, k, out_idx, out_d, ties);
  else if (k == 10) k_knn_query<10, true><<<nb, 256, 0, s>>>(c, q, nq, k, out_idx, out_d, ties);
  else if (k == 20) k_knn_query<20, true><<<nb, 256, 0, s>>>(c, q, nq, k, out_idx, out_d, ties);
  else if (k <= 16) k_knn_query<16, false><<<nb, 256, 0, s>>>(c, q, nq, k, out_idx, out_d, ties);
  else if (k <= 32) k_knn_query<32, false><<<nb, 256, 0, s>>>(c, q, nq, k, out_idx, out_d, ties);
  else if (k <= 64) k_knn_query<64, false><<<nb, 256, 0, s>>>(c, q, nq, k, out_idx, out_d, ties);
  else return false;
  return true;
}
void launch_cov_import(hipStream_t s, const double* in, int layout, int n, const int* inv_perm, double* cov6) {
  k_cov_import<<<cdiv(n, 256), 256, 0, s>>>(in, layout, n, inv_perm, cov6);
}
void launch_cov_export(hipStream_t s, const double* cov6, int layout, int n, const int* perm, double* out) {
  k_cov_export<<<cdiv(n, 256), 256, 0, s>>>(cov6, layout, n, perm, out);
}
void launch_cov_remap(hipStream_t s, const double* old_cov6, const int* old_inv_perm, const int* new_perm, int n,
                      double* cov6) {
  k_cov_remap<<<cdiv(n, 256), 256, 0, s>>>(old_cov6, old_inv_perm, new_perm, n, cov6);
}

}  // namespace ddlo

#ifdef DDLO_COV_PROF
// developer build: k_covariances2's per-group records of the last launch, [group][4]
extern "C" int ddlo_dev_cov_prof2(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ddlo::g_cov_prof2), sizeof(ddlo::g_cov_prof2));
}
extern "C" int ddlo_dev_cov_prof(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ddlo::g_cov_prof), sizeof(ddlo::g_cov_prof));
}
#endif
