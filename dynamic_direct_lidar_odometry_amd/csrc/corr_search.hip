// corr_search.hip — K3 of the GICP hot path: the correspondence search of one
// outer iteration (its traversal and task helpers: search.hpp, nn_tasks.hpp).
//
//   K3 correspondences  k_align_init (per align),       update_correspondences
//                       k_cell_lookup (candidate cells, nano_gicp_impl.hpp:234-275
//                       cellgrid.hip), k_nn_seed +      (1-NN part)
//                       k_nn_scan (the walk)
// launch_linearize (moments.hip) issues these through linearize_internal.hpp.
// Compiled with -ffp-contract=off (see index_build.hip).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gicp_types.hpp"
#include "search.hpp"
#include "nn_tasks.hpp"
#include "launch.hpp"
#include "launch_util.hpp"
#include "linearize_internal.hpp"

namespace ddlo {

constexpr int kLinWaves = 4;        // waves per block of the lookup and seed kernels
constexpr int kSearchQ = 16;        // queries per wavefront in the correspondence search
constexpr int kSeedW = 8;           // Morton-window seed points per slice lane

// job_src (optional): the host's pinned AlignJob.  The block copies it to the
// device job (8-byte words) and initialises from its LDS copy, so an align
// needs no separate host-to-device copy before its first kernel.
__global__ __launch_bounds__(256) void k_align_init(AlignJob* __restrict__ job_dev,
                                                    const AlignJob* __restrict__ job_src) {
  static_assert(sizeof(AlignJob) % 8 == 0, "AlignJob is copied in 8-byte words");
  static_assert(offsetof(AlignJob, guess_R) % 8 == 0 && offsetof(AlignJob, guess_t) == offsetof(AlignJob, guess_R) + 72 &&
                    offsetof(AlignJob, job_full) == offsetof(AlignJob, guess_R) + 96 &&
                    offsetof(AlignJob, ticket) == offsetof(AlignJob, guess_R) + 104,
                "guess_R, guess_t, job_full, ticket: 14 consecutive 8-byte words");
  constexpr int kHdr0 = (int)(offsetof(AlignJob, guess_R) / 8), kHdrN = 14, kHdrFull = 12;
  __shared__ unsigned long long job_lds[sizeof(AlignJob) / 8];
  __shared__ int full_s;
  const AlignJob* job = job_dev;
  double gR[9], gt[3];
  // The device job's words this kernel needs, loaded before the host job's
  // header arrives (values only: they are used, and dereferenced, only when
  // the header says the device job is still the one of the last align, i.e.
  // job_full = 0; the device job buffer itself lives as long as the ctx).
  AlignState* const st_dev = job_dev->state;
  unsigned* const ctr_dev = job_dev->task_ctr;
  unsigned* const fb_dev = job_dev->fb_count;
  const int grid_dev = job_dev->grid_on;
  const int maxit_dev = job_dev->max_iterations;
  const int rec0_dev = job_dev->reuse && job_dev->reuse_rec0;
  bool full = true;
  if (job_src) {
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(job_src);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(job_dev);
    // system scope: read past every GPU cache (the host rewrites this buffer per align).
    // First the guess, the full-copy flag and the ticket (one round trip); the rest of the
    // job only when the host changed more than the guess since the last align.
    if ((int)threadIdx.x < kHdrN) {
      const unsigned long long v = __hip_atomic_load(src + kHdr0 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      job_lds[kHdr0 + threadIdx.x] = v;
      dst[kHdr0 + threadIdx.x] = v;
      if (threadIdx.x == kHdrFull) full_s = v != 0ull;
    }
    __syncthreads();
    full = full_s != 0;
    if (full) {
      for (int w = threadIdx.x; w < (int)(sizeof(AlignJob) / 8); w += blockDim.x) {
        if (w >= kHdr0 && w < kHdr0 + kHdrN) continue;
        const unsigned long long v = __hip_atomic_load(src + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        job_lds[w] = v;
        dst[w] = v;
      }
      __syncthreads();
      job = reinterpret_cast<const AlignJob*>(job_lds);
    }
    const AlignJob* jh = reinterpret_cast<const AlignJob*>(job_lds);
    for (int i = 0; i < 9; ++i) gR[i] = jh->guess_R[i];
    for (int i = 0; i < 3; ++i) gt[i] = jh->guess_t[i];
  } else {
    for (int i = 0; i < 9; ++i) gR[i] = job->guess_R[i];
    for (int i = 0; i < 3; ++i) gt[i] = job->guess_t[i];
  }
  AlignState* st = full ? job->state : st_dev;
  unsigned* const task_ctr = full ? job->task_ctr : ctr_dev;
  const int grid_on = full ? job->grid_on : grid_dev;
  unsigned* const fb_count = full ? job->fb_count : fb_dev;
  const int max_iterations = full ? job->max_iterations : maxit_dev;
  const int rec0 = full ? (job->reuse && job->reuse_rec0) : rec0_dev;
  if (threadIdx.x <= kTaskRegions) task_ctr[threadIdx.x * kCtrStride] = 0u;   // + the moment kernel's arrival counter
  if (grid_on && threadIdx.x <= kFbSegs) fb_count[threadIdx.x * 32] = 0u;   // the lookup's walk list (+ total)
  // source radius from the top-level boxes (<= 64 of them); an unchanged job
  // (same source cloud) keeps the last align's st->src_radius
  if (full && threadIdx.x < 64) {
    const CloudDev& c = job->src;
    const int top = c.nlevels - 1;
    const int off = lvl_off(c, top), cnt = lvl_cnt(c, top);
    float r = 0.f;
    if ((int)threadIdx.x < cnt) {
      const float4 lo = c.box_lo[off + threadIdx.x], hi = c.box_hi[off + threadIdx.x];
      const float mx = fmaxf(fabsf(lo.x), fabsf(hi.x)), my = fmaxf(fabsf(lo.y), fabsf(hi.y)),
                  mz = fmaxf(fabsf(lo.z), fabsf(hi.z));
      r = sqrtf(mx * mx + my * my + mz * mz) * 1.0001f;
    }
    for (int m = 32; m >= 1; m >>= 1) r = fmaxf(r, __shfl_xor(r, m));
    if (threadIdx.x == 0) st->src_radius = r;
  }
  if (threadIdx.x == 0) {
    st->rec = rec0;
    st->any_rec = 0;
    for (int i = 0; i < 9; ++i) st->R[i] = gR[i];
    for (int i = 0; i < 3; ++i) st->t[i] = gt[i];
    st->lambda = -1.0;
    st->iter = 0;
    st->done = max_iterations <= 0 ? 1 : 0;
    st->converged = 0;
    st->nr_iterations = 0;
    st->lm_failed = 0;
    st->lm_trials = 0;
    st->num_corr = 0;
    st->have_prev = 0;
    st->final_cost = 0.0;
    st->tie_pending = 0;
    st->ties_resolved = 0;
    st->tie_err = 0;
  }
}

// K3g: candidate-cell lookup (cellgrid.hip), one query per lane, before the
// walk.  The fp32 query transform of update_correspondences
// (nano_gicp_impl.hpp:240,253; k_nn_seed's operations), the query's cell, and
// the (squared distance, sorted position) minimum over the cell's list: the
// key the full search returns, because every point that can be the fp32
// nearest point of a query of the cell, or tie with it, is on the list.  The
// tie test of k_moments gets sec = the key's distance when a second list
// point has it (nanoflann's order then re-runs the query), else all ones (no
// test).  A query without a list (its cell was not built, or its list
// exceeded the cap) marks its 16-query sub-group for the walk (fb_mask bit,
// fb_list entry); the walk then searches only those queries.
__global__ __launch_bounds__(256) void k_cell_lookup(const AlignJob* __restrict__ job) {
  constexpr int Q = kTaskQ;   // queries per wavefront; 64 / Q lanes (slices) scan each list
  AlignState* st = job->state;
  if (__builtin_amdgcn_readfirstlane(st->done)) return;
  const CloudDev src = job->src;
  const CellGridDev G = job->grid;
  const float cap2 = job->cap2;
  const int lane = lane_id();
  const int qi = lane % Q, sl = lane / Q;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
  const int ngroups = (src.n + Q - 1) / Q;
  const int own_axis = job->own_axis;
  const float own_lo = job->own_lo, own_hi = job->own_hi;
  const int own_mod = job->own_mod, own_rem = job->own_rem;
  const int tie_detect = job->tie_detect;
  float Rf[9], tf[3];
  for (int e = 0; e < 9; ++e) Rf[e] = (float)st->R[e];
  for (int e = 0; e < 3; ++e) tf[e] = (float)st->t[e];
  for (int g = wave; g < ngroups; g += nwaves) {
    const int i = g * Q + qi;
    const bool inrange = i < src.n;
    const float4 a = ldg4(src.pts, inrange ? i : src.n - 1);
    const float qx = (Rf[0] * a.x + Rf[1] * a.y) + (Rf[2] * a.z + tf[0]);
    const float qy = (Rf[3] * a.x + Rf[4] * a.y) + (Rf[5] * a.z + tf[1]);
    const float qz = (Rf[6] * a.x + Rf[7] * a.y) + (Rf[8] * a.z + tf[2]);
    const float qa = own_axis == 0 ? qx : own_axis == 1 ? qy : qz;
    const bool owned = inrange && (own_axis < 0 || (qa >= own_lo && qa < own_hi)) &&
                       (own_mod == 0 || (g % own_mod) == own_rem);
    bool walk = false;
    unsigned off = 0, cnt = 0;
    if (owned) {
      const float tx = (qx - G.ox) * G.inv_s, ty = (qy - G.oy) * G.inv_s, tz = (qz - G.oz) * G.inv_s;
      if (!(tx >= 0.f && tx < (float)G.nx && ty >= 0.f && ty < (float)G.ny && tz >= 0.f && tz < (float)G.nz)) {
        walk = !G.outside_nomatch;   // beyond every target point's reach (or outside the built box)
      } else {
        walk = cg_cell_list(G, tx, ty, tz, off, cnt) == 2;
      }
    }
    // this slice's part of the list: the (distance, position) minimum and the
    // smallest distance of its other points
    unsigned long long bk = ~0ull;
    float d2 = INFINITY;
    constexpr int kU = 4;   // loads in flight per lane
    for (unsigned k = sl; k < cnt; k += kU * (64 / Q)) {
      float4 pp[kU];
#pragma unroll
      for (int j = 0; j < kU; ++j) pp[j] = ldg4(G.ent, off + min(k + j * (64 / Q), cnt - 1));
#pragma unroll
      for (int j = 0; j < kU; ++j) {
        const float4 p = pp[j];
        if (k + j * (64 / Q) < cnt) {
          const float dd = dist2(qx, qy, qz, p.x, p.y, p.z);
          const unsigned long long kk = dkey(dd, __float_as_int(p.w));
          if (kk < bk) {
            if (bk != ~0ull) d2 = fminf(d2, __uint_as_float((unsigned)(bk >> 32)));
            bk = kk;
          } else {
            d2 = fminf(d2, dd);
          }
        }
      }
    }
    // merge the slices: the loser's distance joins the others'
    static_assert(Q == 16, "slice merge over lanes l ^ 16, l ^ 32");
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned long long ob = h == 0 ? xor_min64<16>(bk) : xor_min64<32>(bk);   // min of the pair
      const unsigned long long other = h == 0 ? __shfl_xor(bk, 16) : __shfl_xor(bk, 32);
      const float od2 = h == 0 ? __shfl_xor(d2, 16) : __shfl_xor(d2, 32);
      const unsigned long long lose = bk < other ? other : bk;
      d2 = fminf(d2, od2);
      if (lose != ~0ull) d2 = fminf(d2, __uint_as_float((unsigned)(lose >> 32)));
      bk = ob;
    }
    if (sl == 0 && inrange && !walk) {
      job->qstate[i] = make_float4(qx, qy, qz, -1.f);
      const unsigned long long key = owned ? umin64(bk, dkey(cap2, -1)) : dkey(INFINITY, -1);
      job->key[i] = key;
      if (tie_detect) {
        const float kd = __uint_as_float((unsigned)(key >> 32));
        const bool tied = owned && (unsigned)key != 0xffffffffu && d2 == kd;
        job->sec[i] = tied ? (unsigned)(key >> 32) : 0xffffffffu;
      }
      if (job->tie_scan == 3) job->key2[i] = mirror_key(key);
    }
    // a sub-group with a query for the walk
    const unsigned m16 = (unsigned)__ballot(walk && sl == 0) & 0xffffu;
    if (m16 && lane == 0) {
      const int seg = g & (kFbSegs - 1);
      const int slot = (int)atomicAdd(job->fb_count + seg * 32, 1u);
      job->fb_list[seg * job->fb_seg_cap + slot] = g;
      job->fb_mask[g] = (unsigned short)m16;
    }
  }
}

// K3a (+ the former K3b): seed and walk of the exact bounded 1-NN correspondence search
// (nn_tasks.hpp; update_correspondences, nano_gicp_impl.hpp:249-258),
// Q = 16 queries (a sub-group) per wavefront: the fp32 query transform,
// then an exact upper bound — the triangle bound from the previous
// correspondence for a small pose step (no load), the Morton window around
// the previous match after a large step, else the Morton window around the
// query's own key — then probe seeds and group sharing.  The same wavefront
// then walks its sub-group from the seed in registers (TaskCollector: the
// LDS-cached upper levels with the union box of the 16 balls, the exact
// (leaf, query) box tests, tasks appended to the list for k_nn_scan) and
// writes the per-query search state (qstate), the key and the second
// distance.  4 waves/SIMD: the kernel fits 128 VGPRs.
__global__ __launch_bounds__(256, 4) void k_nn_seed(const AlignJob* __restrict__ job) {
  constexpr int Q = kTaskQ;
  AlignState* st = job->state;
  if (__builtin_amdgcn_readfirstlane(st->done)) return;
  const CloudDev src = job->src;
  const CloudDev tgt = job->tgt;
  const auto corr = gpw(job->corr);
  const auto sqd = gpw(job->sqd);
#ifdef DDLO_SEARCH_STATS
  unsigned int* const stats = job->stats;
#else
  // per-sub-group counters only in the developer build (make statsprof): the
  // production kernel then fits 128 VGPRs (4 waves/SIMD, no hot-loop spills)
  unsigned int* const stats = nullptr;
#endif
  const float cap2 = job->cap2;
  const int have_prev = st->have_prev;
  const int prev_window = job->prev_window;
  const double tri_mv = job->tri_mv_d;
  // walk-radius inflation of this search, wave-uniform (scalar registers for the whole kernel)
  const double gap_sel = have_prev ? job->reuse_gap_d : job->reuse_gap0_d;
  const long long gap_bits = __double_as_longlong(gap_sel);
  const double gap_u = __longlong_as_double(
      ((long long)__builtin_amdgcn_readfirstlane((int)(gap_bits >> 32)) << 32) |
      (unsigned)__builtin_amdgcn_readfirstlane((int)gap_bits));
  const int own_axis = job->own_axis;
  const float own_lo = job->own_lo, own_hi = job->own_hi;
  const int own_mod = job->own_mod, own_rem = job->own_rem;
  const int lane = lane_id();
  const int qi = lane % Q;
  const int wib = threadIdx.x >> 6;
  float4* const qstate = job->qstate;
  unsigned long long* const keyout = job->key;
  const int wave = (int)blockIdx.x * kLinWaves + wib;
  const int nwaves_total = gridDim.x * kLinWaves;
  const int ngroups = (src.n + Q - 1) / Q;
  const int reuse = job->reuse;
  const bool check_ref = reuse && have_prev && st->any_rec;   // references exist only after a recording iteration
  const int rec = st->rec;   // this search records references
  // fused walk: dynamic LDS = [kLinWaves x TaskLds][upper-level box cache]
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  TaskLds* const TL = reinterpret_cast<TaskLds*>(dsm) + __builtin_amdgcn_readfirstlane(wib);   // scalar base
  f4v* const upper = reinterpret_cast<f4v*>(dsm + kLinWaves * kTaskLdsBytes);
  // candidate cells (k_cell_lookup): only the listed sub-groups, only their
  // unanswered queries; the answered ones keep the lookup's outputs.  Their
  // tasks are scanned inline (task_cap_r = 0: no k_nn_scan launch).
  const int grid_on = job->grid_on;
  int seg_end[kFbSegs];
  int nitems = ngroups;
  if (grid_on) {
    nitems = 0;
#pragma unroll
    for (int sg = 0; sg < kFbSegs; ++sg) {
      nitems += (int)job->fb_count[sg * 32];
      seg_end[sg] = nitems;
    }
    if ((int)blockIdx.x * kLinWaves >= nitems) return;   // the whole block (uniform): before the LDS prologue
  }
  fill_upper(tgt, upper);
  __syncthreads();
  for (int item = wave; item < nitems; item += nwaves_total) {
    int g = item;
    unsigned gmask = 0xffffu;
    if (grid_on) {
      int sg = 0, s0 = 0;
#pragma unroll
      for (int t = 0; t < kFbSegs - 1; ++t)
        if (item >= seg_end[t]) {
          sg = t + 1;
          s0 = seg_end[t];
        }
      g = job->fb_list[sg * job->fb_seg_cap + (item - s0)];
      gmask = job->fb_mask[g];
    }
    const bool mine = (gmask >> qi) & 1u;   // this search writes the query's outputs
    const unsigned long long tm0 = stats ? __builtin_amdgcn_s_memtime() : 0ull;
    const int i = g * Q + qi;
    const bool inrange = i < src.n && mine;
    const int ic = i < src.n ? i : src.n - 1;
    // every independent per-query load of the prologue in one round trip
    const float4 a = ldg4(src.pts, ic);
    const int jprev = have_prev ? corr[ic] : -1;
    const float sqprev = have_prev ? sqd[ic] : 0.f;
    const float4 rf = check_ref ? ldg4(job->ref, ic) : make_float4(0.f, 0.f, 0.f, -1.f);
    const float4 rp = check_ref ? ldg4(job->ref_p, ic) : make_float4(0.f, 0.f, 0.f, 0.f);
    // the pose is read per sub-group, so that it is not held in 12 VGPRs
    // (the fp64 -> fp32 conversions are vector ops) across the walk
    float Rf[9], tf[3];
    for (int e = 0; e < 9; ++e) Rf[e] = (float)st->R[e];
    for (int e = 0; e < 3; ++e) tf[e] = (float)st->t[e];
    // fp32 query transform, Eigen lazy-product order (see oracle/cpu_ref.cpp)
    const float qx = (Rf[0] * a.x + Rf[1] * a.y) + (Rf[2] * a.z + tf[0]);
    const float qy = (Rf[3] * a.x + Rf[4] * a.y) + (Rf[5] * a.z + tf[1]);
    const float qz = (Rf[6] * a.x + Rf[7] * a.y) + (Rf[8] * a.z + tf[2]);
    // spatial sharding: search only the queries this rank owns
    const float qa = own_axis == 0 ? qx : own_axis == 1 ? qy : qz;
    static_assert(Q == 16, "interleaved ownership is per 16-point group: i >> 4 == g");
    const bool owned = inrange && (own_axis < 0 || (qa >= own_lo && qa < own_hi)) &&
                       (own_mod == 0 || (g % own_mod) == own_rem);   // scalar: g is wave-uniform
    // Verified reuse (AlignJob::ref): every target point other than p1 was
    // at fp32 squared distance >= B^2 from q_ref, so (relative 1e-6 covers
    // the fp32 rounding of a squared distance) its true distance from q is
    // >= sqrt(B^2 / (1 + 1e-6)) - eps, eps = |q - q_ref|, and its fp32
    // squared distance >= lb2.  p1 at dn < lb2 is then the exact minimum
    // (no tie possible); with no p1, lb2 > cap2 means no point within the
    // bound.  The key is what the full search returns: min((cap2, none),
    // (dn, p1)).
    bool passed = false;
    unsigned long long pass_key = dkey(cap2, -1);
    int rj = -1;
    float dn = INFINITY;
    if (owned && rf.w >= 0.f) {
      rj = __float_as_int(rp.w);
      const double ex = (double)qx - rf.x, ey = (double)qy - rf.y, ez = (double)qz - rf.z;
      const double eps = sqrt(ex * ex + ey * ey + ez * ez) * (1.0 + 1e-9) + 1e-12;
      const double b = sqrt((double)rf.w / (1.0 + 1e-6));
      const double lb2 = b > eps ? (b - eps) * (b - eps) * (1.0 - 1e-6) : -1.0;
      if (rj >= 0) {
        dn = dist2(qx, qy, qz, rp.x, rp.y, rp.z);
        if ((double)dn < lb2) {
          passed = true;
          pass_key = umin64(pass_key, dkey(dn, rj));
        }
      } else if (lb2 > job->cap2_d) {
        passed = true;
      }
    }
    const bool active = owned && !passed;
    if (!__any(active)) {
      if (inrange && lane < Q) {
        keyout[i] = passed ? pass_key : dkey(INFINITY, -1);
        qstate[i] = make_float4(qx, qy, qz, -1.f);
        if (job->tie_detect) job->sec[i] = 0xffffffffu;   // not searched (proven strict or not owned): no tie test
        if (job->tie_scan == 3) job->key2[i] = mirror_key(passed ? pass_key : dkey(INFINITY, -1));
      }
      if (stats) {
        const unsigned npass = (unsigned)__popcll(__ballot(passed && lane < Q));
        if (lane == 0) {
          unsigned int* o = stats + (size_t)g * kStatFields;
          for (int f = 0; f < kStatFields; ++f) o[f] = 0;
          o[6] = npass << 8;
          o[7] = 1;
        }
      }
      continue;
    }
    NNVisitor<Q> vis;
    vis.qx = qx;
    vis.qy = qy;
    vis.qz = qz;
    vis.active = active;
    vis.best = active ? cap2 : -1.f;
    vis.bestj = -1;
    vis.skip_lo = 1;
    vis.skip_hi = 0;
    bool seeded = false;
    bool large_step = false;   // previous match exists but the pose moved >= 2 cm since
    bool rewindow = false;     // mode 2: previous match's distance AND the Morton window at the new position
    // coordinates of the point behind vis.bestj (every seed step carries them)
    float bpx = 0.f, bpy = 0.f, bpz = 0.f;
    if (have_prev && active) {
      const int j = jprev;
      if (j >= 0) {
        // NN(q) <= |q - p_prev| <= sqrt(sqd_prev) + |q - q_prev| (triangle
        // inequality; fp64 with an upward margin covers fp32 rounding), so
        // the bound needs no load of the previous match.
        // previous linearization pose (for the triangle-inequality bound)
        float Rp[9], tp[3];
        for (int e = 0; e < 9; ++e) Rp[e] = (float)st->last_lin_R[e];
        for (int e = 0; e < 3; ++e) tp[e] = (float)st->last_lin_t[e];
        const float qpx = (Rp[0] * a.x + Rp[1] * a.y) + (Rp[2] * a.z + tp[0]);
        const float qpy = (Rp[3] * a.x + Rp[4] * a.y) + (Rp[5] * a.z + tp[1]);
        const float qpz = (Rp[6] * a.x + Rp[7] * a.y) + (Rp[8] * a.z + tp[2]);
        const double ddx = (double)qx - qpx, ddy = (double)qy - qpy, ddz = (double)qz - qpz;
        const double mv = sqrt(ddx * ddx + ddy * ddy + ddz * ddz);
        if (mv < tri_mv) {
          const double r = sqrt((double)sqprev) + mv;
          const double b2 = r * r * (1.0 + 1e-5) + 1e-12;
          if (b2 < job->cap2_d) {
            vis.best = __uint_as_float(__float_as_uint((float)b2) + 1);  // round up
            seeded = true;
          }
        } else if (prev_window == 1) {
          large_step = true;   // exact distances to the Morton window around p_prev (below)
        } else {  // large pose step: the exact distance to the previous match (+ mode 2: the Morton window below)
          rewindow = prev_window == 2;
          const float4 p = ldg4(tgt.pts, j);
          const float d = dist2(qx, qy, qz, p.x, p.y, p.z);
          if (d < cap2) {
            vis.best = d;
            vis.bestj = j;
            bpx = p.x;
            bpy = p.y;
            bpz = p.z;
            seeded = true;
          }
        }
      }
    }
    // the reference's match at the new position is a real candidate
    if (active && rj >= 0 && dn < vis.best) {
      vis.best = dn;
      vis.bestj = rj;
      bpx = rp.x;
      bpy = rp.y;
      bpz = rp.z;
      seeded = true;
    }
    // Exact seeding for queries without a usable previous correspondence:
    // the real target points around the query's Morton position give an
    // upper bound, so the single search below stays exact.  After a large
    // pose step the window is centred on the previous match instead (its
    // sorted position IS a Morton position next to the new nearest point,
    // and no key search is needed); the window contains the previous match.
    const bool need_seed = active && ((!seeded && !large_step) || rewindow);
    const bool use_window = need_seed || large_step;
    if (__any(use_window)) {
      // Morton window of kSeedW points per slice lane (64/Q * kSeedW per query)
      int pos = large_step ? jprev : 0;
      if (__any(need_seed)) {
        const unsigned long long qk = morton_key(qx, qy, qz, tgt.quant);
        int dlo, dhi, sp;
        const bool found = seed_pos(tgt.dir, qk, sp, dlo, dhi);   // directory + fine directory: <= 2 loads
        if (__any(!found)) {   // a bucket of >= 2^16 keys: searched
          const bool srch = need_seed && !found;
          sp = group_lower_bound<Q>(tgt.keys, tgt.n, qk, srch ? dlo : sp, srch ? dhi : sp);
        }
        if (need_seed) pos = sp;
      }
      const int s = lane / Q;
      const int w0 = pos - (64 / Q) * kSeedW / 2 + s * kSeedW;
      unsigned long long bk = dkey(vis.best, vis.bestj);
      float4 p[kSeedW];
#pragma unroll
      for (int k = 0; k < kSeedW; ++k) p[k] = ldg4(tgt.pts, min(max(w0 + k, 0), tgt.n - 1));
      // the winner's coordinates travel with its key (group sharing below needs no load)
      float cx = bpx, cy = bpy, cz = bpz;
      if (use_window) {
#pragma unroll
        for (int k = 0; k < kSeedW; ++k) {
          const int cand = min(max(w0 + k, 0), tgt.n - 1);
          const unsigned long long kk = dkey(dist2(qx, qy, qz, p[k].x, p[k].y, p[k].z), cand);
          if (kk < bk) {
            bk = kk;
            cx = p[k].x;
            cy = p[k].y;
            cz = p[k].z;
          }
        }
      }
      static_assert(Q == 16, "slice merge over lanes l ^ 16, l ^ 32");
      xor_min64_xyz<16>(bk, cx, cy, cz);
      xor_min64_xyz<32>(bk, cx, cy, cz);
      if (use_window) {
        const float bd = __uint_as_float((unsigned)(bk >> 32));
        if (bd < cap2) {
          vis.best = bd;
          vis.bestj = (int)(unsigned)bk;
          bpx = cx;
          bpy = cy;
          bpz = cz;
        }
      }
    }
    // Probe seeds: a sub-group whose Morton windows found nothing near (its
    // queries sit off every surface near their own Morton positions, e.g.
    // 0.4-0.5 m off a wall under the guess pose, and keep a bound near the
    // cap) takes the Morton windows of 8 points around its centre, offset by
    // probe_d along +-x, +-y, +-z and the two xy diagonals: 8 points each,
    // staged in LDS, every query their exact distances (real candidates, so
    // exactness is kept; group sharing below spreads them).
    {
      const float pt2 = job->probe2;
      if (pt2 > 0.f && pt2 < 0.5f * cap2 && __any(need_seed && vis.best > pt2)) {   // radius < 0.71 x the cap
        // centre: the first active query (the sub-group is Morton-compact)
        const unsigned long long am = __ballot(active);
        const int c0 = am ? __builtin_ctzll(am) : 0;
        const float cx = readlane_f(qx, c0), cy = readlane_f(qy, c0), cz = readlane_f(qz, c0);
        const float d = job->probe_d, dd = d * 0.70710678f;
        const int pr = lane & 7;
        const float ox = pr == 0 ? d : pr == 1 ? -d : pr == 6 ? dd : pr == 7 ? -dd : 0.f;
        const float oy = pr == 2 ? d : pr == 3 ? -d : pr == 6 ? dd : pr == 7 ? -dd : 0.f;
        const float oz = pr == 4 ? d : pr == 5 ? -d : 0.f;
        const unsigned long long pk = morton_key(cx + ox, cy + oy, cz + oz, tgt.quant);
        int plo, phi, plb;
        const bool pfound = seed_pos(tgt.dir, pk, plb, plo, phi);
        if (__any(!pfound)) plb = group_lower_bound<8>(tgt.keys, tgt.n, pk, pfound ? plb : plo, pfound ? plb : phi);
        const int cand = min(max(plb - 4 + (lane >> 3), 0), tgt.n - 1);
        const float4 p = ldg4(tgt.pts, cand);
        f4v* const CP = TL->sb_lo;   // 64 staged candidates (the walk's box stage, free until the walk)
        CP[lane] = f4v{p.x, p.y, p.z, __int_as_float(cand)};
        __builtin_amdgcn_wave_barrier();
        unsigned long long bk = dkey(vis.best, vis.bestj);
        float ux = bpx, uy = bpy, uz = bpz;
        const int s4 = lane / Q;
#pragma unroll 4
        for (int k = 0; k < 64 / (64 / Q); ++k) {
          const f4v c = CP[s4 * (64 / (64 / Q)) + k];
          const unsigned long long kk = dkey(dist2(qx, qy, qz, c.x, c.y, c.z), __float_as_int(c.w));
          if (kk < bk) {
            bk = kk;
            ux = c.x;
            uy = c.y;
            uz = c.z;
          }
        }
        xor_min64_xyz<16>(bk, ux, uy, uz);
        xor_min64_xyz<32>(bk, ux, uy, uz);
        __builtin_amdgcn_wave_barrier();
        if (active && bk < dkey(vis.best, vis.bestj)) {
          vis.best = __uint_as_float((unsigned)(bk >> 32));
          vis.bestj = (int)(unsigned)bk;
          bpx = ux;
          bpy = uy;
          bpz = uz;
          seeded = true;
        }
      }
    }
    // Group sharing: every query also takes the exact distance to the other
    // queries' candidate points (Morton-adjacent queries are spatially
    // adjacent, so a neighbour's candidate is often far closer than the
    // query's own).  Valid (distance, position) pairs only: exactness kept.
    {
      const unsigned long long donors = __ballot(lane < Q && active && vis.bestj >= 0);
      if (donors && __any(active)) {
        // lane (query qi, slice s) takes donors 4s .. 4s + 3 (read from their
        // slice-0 lanes), then the four slices merge: 4 distance steps per
        // lane instead of one per donor
        unsigned long long bk = dkey(vis.best, vis.bestj);
        const int s = lane / Q;
#pragma unroll 1
        for (int t = 0; t < 4; ++t) {
          const int d = s * 4 + t;
          const float sx = __shfl(bpx, d), sy = __shfl(bpy, d), sz = __shfl(bpz, d);
          const int sj = __shfl(vis.bestj, d);
          if ((donors >> d) & 1ull) bk = umin64(bk, dkey(dist2(qx, qy, qz, sx, sy, sz), sj));
        }
        bk = xor_min64<16>(bk);
        bk = xor_min64<32>(bk);
        if (active) {
          vis.best = __uint_as_float((unsigned)(bk >> 32));
          vis.bestj = (int)(unsigned)bk;
        }
      }
    }
    // walk radius: the seed bound, widened by the reuse gap so that the
    // reference recorded from this search has B well above d1
    float wr = vis.best;
    const double gap = gap_u;
    if (rec && active && gap > 0.0) {
      const double r = sqrt((double)vis.best) + gap;
      wr = __uint_as_float(__float_as_uint((float)(r * r)) + 1);   // rounded up
    }
    // The walk, from the seed in registers.  The query state and key are
    // stored after it -- a store ahead of the walk's first box loads would be
    // waited for with them (vmcnt counts loads and stores in issue order)
    {
      const unsigned long long k0 = dkey(vis.best, vis.bestj);
      TaskList tl;
      tl.tasks = job->tasks;
      tl.ctr = job->task_ctr;
      tl.cap_r = job->task_cap_r;
      TaskCollector col;
      col.L = TL;
      col.U = upper;
      col.nup = upper_count(tgt);
      col.qx = qx;
      col.qy = qy;
      col.qz = qz;
      col.active = active;
      col.bk = k0;
      col.wr = active ? wr : -1.f;
      col.sg = g;
      col.pf_ratio = job->pf_ratio;
      const unsigned tm1 = stats ? (unsigned)__builtin_amdgcn_s_memtime() : 0u;
      col.run(tgt, tl, gp(src.keys)[ic], job->split_extent);
      if (inrange && lane < Q) {
        qstate[i] = make_float4(qx, qy, qz, active ? wr : -1.f);
        const unsigned long long k_out = active ? col.bk : passed ? pass_key : dkey(INFINITY, -1);
        keyout[i] = k_out;   // col.bk: the seed, lowered by inline scans
        if (job->tie_scan == 3) job->key2[i] = mirror_key(k_out);
      }
      // the examined points' second distance: the reuse bound (rec) and the
      // tie test of k_moments (sec == the key's distance); k_nn_scan lowers it
      if ((rec || job->tie_detect) && inrange && lane < Q)
        job->sec[i] = active ? __float_as_uint(col.sec) : 0xffffffffu;   // all ones: not searched, no tie test
      if (stats) {
        const unsigned npass = (unsigned)__popcll(__ballot(passed && lane < Q));
        if (lane == 0) {
          unsigned int* o = stats + (size_t)g * kStatFields;
          o[0] = col.st_blocks;
          o[1] = min((tm1 - (unsigned)tm0) >> 4, 65535u);
          o[2] = col.st_tasks | (min(col.st_iters, 65535u) << 16);
          o[3] = col.st_inline;
          o[4] = (unsigned)__builtin_amdgcn_s_memtime() - (unsigned)tm0;
          o[5] = min((col.tm_walk - (unsigned)tm0) >> 4, 65535u);
          o[6] = npass << 8;   // queries proven by their reuse reference (bit 0, "hard", is always 0)
          o[7] = 1;
        }
      }
    }
  }
}

// K3c: leaf scans of the task list.  The waves of region r split its tasks
// into contiguous chunks (XCD-aware, see below).  A wave loads up to 64
// task words at once and stages batches of kScanBatch tasks in LDS with
// LDS-DMA — per task the leaf's 32 SoA points (384 B) and the sub-group's 16
// query states (256 B) — double-buffered: batch k + 1 is in flight while
// batch k is scanned from LDS (lane = query qi x quarter s of the leaf).  A
// sub-group's tasks sit next to each other in the list (one collect flush),
// so the per-query minimum is kept in registers across a run of the same
// sub-group and merged into the result with one 64-bit atomicMin per query.
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

constexpr int kScanBatch = 6;                         // tasks per LDS batch (two batches in flight: 7.5 KB of LDS per wave)
constexpr int kScanTaskBytes = 3 * kLeafSize * 4 + kTaskQ * 16;   // 384 B points + 256 B queries
constexpr int kScanWaves = 4;                         // waves per block

// 5 waves/SIMD: 96 VGPRs, and 5 x 4 waves x 7.5 KB = 150 KB of the CU's 160 KB of LDS
__global__ __launch_bounds__(64 * kScanWaves, 5) void k_nn_scan(const AlignJob* __restrict__ job) {
  constexpr int BATCH = kScanBatch;
  const AlignState* st = job->state;
  if (__builtin_amdgcn_readfirstlane(st->done)) return;
  const CloudDev tgt = job->tgt;
  const float4* const qstate = job->qstate;
  unsigned long long* const key = job->key;
  const int cap_r = job->task_cap_r;
  const int lane = lane_id();
  const int qi = lane & 15, s = lane >> 4;
  constexpr int kBatchBytes = BATCH * kScanTaskBytes;   // 6 tasks: 3.75 KB, the last of 4 LDS-DMA wave-instructions partial
  constexpr int kDma = (kBatchBytes + 1023) / 1024;     // LDS-DMA wave-instructions per batch
  static_assert(kDma <= 15, "vmcnt immediate");
  __shared__ __attribute__((aligned(16))) unsigned char lds_all[kScanWaves][2][kBatchBytes];
  unsigned char* const L0 = lds_all[threadIdx.x >> 6][0];
  unsigned char* const L1 = lds_all[threadIdx.x >> 6][1];
  const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
  const int wpr = nwaves / kTaskRegions;   // the grid is a multiple of 8 * kTaskRegions waves
  // (region, chunk) of this wave.  A region's tasks were appended roughly in
  // sub-group (= Morton) order, so chunk c of every region covers about the
  // same c-th slice of the scene; blocks b and b + 8 share an XCD and its
  // L2, so XCD x = b % 8 gets chunks [x wpr / 8, (x + 1) wpr / 8) of all
  // regions: one spatial eighth of the target per L2.  Speed only: any
  // bijection of waves onto (region, chunk) is exact.
  int r, c;
  if (job->xcd_scan && wpr % 8 == 0) {
    const int x = blockIdx.x % 8, u = (int)(blockIdx.x / 8) * kScanWaves + (int)(threadIdx.x >> 6);
    r = u % kTaskRegions;
    c = x * (wpr / 8) + u / kTaskRegions;
  } else {
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    r = wave % kTaskRegions;
    c = wave / kTaskRegions;
  }
  const int n = min((int)__builtin_amdgcn_readfirstlane(job->task_ctr[r * kCtrStride]), cap_r);
  const int chunk = (n + wpr - 1) / wpr;
  const int lo = c * chunk, hi = min(n, lo + chunk);
  const unsigned long long* rt = job->tasks + (size_t)r * cap_r;
  unsigned* const sec = job->sec;
  const bool rec = st->rec != 0;     // this search records reuse references
  // the second distance of the examined points is tracked for the reuse
  // bound (rec) and for k_moments' tie test (tie_detect): every point at the
  // final nearest distance is examined (its leaf is within the walk radius),
  // so the query is tied iff another examined point has that distance
  const bool reuse = rec || (job->tie_scan == 1 || job->tie_scan == 2);
  const bool lane_sd = rec || job->tie_scan == 1;   // second distance over every point of a slice
  // tie_scan 3 (not recording): the Morton-order scan plus equal-distance
  // flags at its merges (slices, tasks of a run) and the mirrored key pushed
  // beside the key (runs): no atomic return is waited for
  // tie_scan 4: the same, but the runs' ties come from the key's atomicMin
  // return (consumed at the next run's merge) and a run's own merges instead
  // of a mirrored key: one atomic per run, no key2 traffic
  const bool tie3 = !rec && (job->tie_scan == 3 || job->tie_scan == 4);
  const bool mirror = job->tie_scan == 3;
  const bool tie_xor = !(job->tie_ab & 2);
  unsigned long long* const key2 = job->key2;
  unsigned td = 0xffffffffu;   // smallest distance (bits) met twice at a slice merge of this run (any slice lane)
  unsigned long long accm = ~0ull;   // the run's minimum of mirrored keys (its tasks' bests, highest position first)
  int run_sg = -1;
  unsigned long long acc = ~0ull;   // lane's query minimum over the current run
  float acc2 = INFINITY;            // smallest distance of the run's other points (reuse)
  float run_bound = -1.f;
  // A run's merge into the result: the key's atomicMin, then (reuse) the
  // smallest distance of every examined point except the final best — the
  // run's other points and whichever of (old key, run minimum) lost.  The
  // second push needs the atomicMin's return value: it is issued at the
  // NEXT run's merge, so the return trip overlaps the scan of that run.
  bool pend = false;
  size_t pend_q = 0;
  unsigned long long pend_acc = 0ull, pend_old = 0ull;
  float pend_acc2 = 0.f, pend_bound = 0.f;
  auto resolve = [&]() {
    if (pend) {
      float push = pend_acc2;
      if (pend_old != pend_acc) {
        const unsigned long long lost = pend_old < pend_acc ? pend_acc : pend_old;
        if (key_real(lost)) push = fminf(push, key_dist(lost));
      }
      // rec: everything below the walk radius (B^2 = min(sec, radius));
      // tie test only: a push can matter only if it equals the query's
      // current minimum (the final one is <= it), so almost none is issued
      if (rec ? push <= pend_bound : push == key_dist(umin64(pend_old, pend_acc)))
        atomicMin(sec + pend_q, __float_as_uint(push));
      pend = false;
    }
  };
  // tie_scan 4 (the same pending slot, reuse is off): the previous run's key
  // atomicMin return at the same distance and another position is a tie
  auto resolve4 = [&]() {
    if (pend) {
      if (key_real(pend_old) && pend_old != pend_acc && (pend_old >> 32) == (pend_acc >> 32))
        atomicMin(sec + pend_q, (unsigned)(pend_acc >> 32));
      pend = false;
    }
  };
  auto flush_run = [&]() {
    if (tie3 && !mirror) resolve4();
    if (run_sg >= 0 && lane < 16 && (unsigned)(acc >> 32) <= __float_as_uint(run_bound)) {
      const size_t qidx = (size_t)run_sg * kTaskQ + qi;
      if (reuse) {
        resolve();
        pend_old = atomicMin(key + qidx, acc);
        pend = true;
        pend_q = qidx;
        pend_acc = acc;
        pend_acc2 = acc2;
        pend_bound = run_bound;
      } else if (tie3 && !mirror) {
        pend_old = atomicMin(key + qidx, acc);
        pend = true;
        pend_q = qidx;
        pend_acc = acc;
      } else {
        atomicMin(key + qidx, acc);
        if (tie3 && !(job->tie_ab & 1)) atomicMin(key2 + qidx, accm);   // with key: two of the run's tasks at the distance = a tie
      }
    }
    if (tie3 && run_sg >= 0) {   // the run's tie distances of the query's four slice lanes -> its lane qi
      unsigned t = min(td, (unsigned)__shfl_xor((int)td, 16));
      t = min(t, (unsigned)__shfl_xor((int)t, 32));
      if (lane < 16 && t <= __float_as_uint(run_bound))   // rare: a real equal-distance pair
        atomicMin(sec + (size_t)run_sg * kTaskQ + qi, t);   // k_moments: tied iff it is the final distance
    }
  };
  for (int wbase = lo; wbase < hi; wbase += 64) {
    const int wcnt = min(64, hi - wbase);
    const unsigned long long tl = lane < wcnt ? rt[wbase + lane] : 0ull;   // up to 64 task words at once
    // LDS-DMA tasks [b0, b0 + kScanBatch) of the window: 16 B per lane per
    // instruction, 1 KB per wave-instruction (past the window: the last task
    // again, never read)
    auto issue = [&](int b0, unsigned char* buf) {
#pragma unroll
      for (int i = 0; i < kDma; ++i) {
        const int o = i * 1024 + lane * 16;
        const int k = min(b0 + o / kScanTaskBytes, wcnt - 1), w = o % kScanTaskBytes;
        const unsigned long long tk = __shfl(tl, k);   // every lane takes part in the permute
        const char* src = w < 3 * kLeafSize * 4
                              ? (const char*)(tgt.soa + (size_t)(tk >> 40) * (3 * kLeafSize)) + w
                              : (const char*)(qstate + (size_t)((tk >> 16) & 0xffffffull) * kTaskQ) + (w - 3 * kLeafSize * 4);
        if (kBatchBytes % 1024 == 0 || o < kBatchBytes)   // a partial last instruction: lanes past the batch idle
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                           (__attribute__((address_space(3))) void*)(buf + i * 1024), 16, 0, 0);
      }
    };
    issue(0, L0);
    for (int b0 = 0; b0 < wcnt; b0 += BATCH) {
      unsigned char* const cur = ((b0 / BATCH) & 1) ? L1 : L0;
      if (b0 + BATCH < wcnt) {
        issue(b0 + BATCH, ((b0 / BATCH) & 1) ? L0 : L1);
        __builtin_amdgcn_s_waitcnt(0x0F70 | kDma);  // vmcnt(kDma): all but the batch just issued -> the current batch landed
      } else {
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      }
      __builtin_amdgcn_wave_barrier();
      const int nb = min(BATCH, wcnt - b0);
      for (int k = 0; k < nb; ++k) {
        const unsigned long long t = readlane_u64(tl, b0 + k);
        const int sg = (int)((t >> 16) & 0xffffffull);
        if (sg != run_sg) {   // uniform: a new sub-group's run starts
          flush_run();
          run_sg = sg;
          acc = ~0ull;
          acc2 = INFINITY;
          run_bound = -1.f;
          td = 0xffffffffu;
          accm = ~0ull;
        }
        const unsigned char* T = cur + k * kScanTaskBytes;
        const f4v x0 = *(const f4v*)(T + s * 32), x1 = *(const f4v*)(T + s * 32 + 16);
        const f4v y0 = *(const f4v*)(T + 128 + s * 32), y1 = *(const f4v*)(T + 128 + s * 32 + 16);
        const f4v z0 = *(const f4v*)(T + 256 + s * 32), z1 = *(const f4v*)(T + 256 + s * 32 + 16);
        const f4v q = *(const f4v*)(T + 384 + qi * 16);
        const float X[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        const float Y[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
        const float Z[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
        // same IEEE ops as dist2(), two points per packed instruction; the
        // lane's points come in increasing position, so strict < keeps the
        // lowest position among equal distances
        const f2v qx2 = {q.x, q.x}, qy2 = {q.y, q.y}, qz2 = {q.z, q.z};
        f2v d[4];
#pragma unroll
        for (int h = 0; h < 8; h += 2) {
          const f2v dx = qx2 - f2v{X[h], X[h + 1]};
          const f2v dy = qy2 - f2v{Y[h], Y[h + 1]};
          const f2v dz = qz2 - f2v{Z[h], Z[h + 1]};
          d[h / 2] = (dx * dx + dy * dy) + dz * dz;
        }
        const bool on = ((t >> qi) & 1ull) != 0ull;
        const int pos0 = (int)(t >> 40) * kLeafSize + s * 8;
        if (reuse) {   // recording search / tie test: the leaf's best key and a second distance (uniform branch)
          float bd = INFINITY, sd = INFINITY;
          int bh = 0;
          if (lane_sd) {   // every examined point: the reuse bound (and the full tie test)
#pragma unroll
            for (int h = 0; h < 8; ++h) {
              const float dh = (h & 1) ? d[h / 2].y : d[h / 2].x;
              if (dh < bd) { sd = bd; bd = dh; bh = h; } else { sd = fminf(sd, dh); }
            }
          } else {   // tie test only: the slices' losing bests; a tie inside the winner's 8-point slice is
                     // k_moments' own check
#pragma unroll
            for (int h = 0; h < 8; ++h) {
              const float dh = (h & 1) ? d[h / 2].y : d[h / 2].x;
              if (dh < bd) { bd = dh; bh = h; }
            }
          }
          unsigned long long bk = dkey(bd, pos0 + bh);
          xor_top2<16>(bk, sd);
          xor_top2<32>(bk, sd);
          if (on) fold_top2(acc, acc2, bk, sd);
        } else {
          float bd = INFINITY;
          int bh = 0;
#pragma unroll
          for (int h = 0; h < 8; ++h) {
            const float dh = (h & 1) ? d[h / 2].y : d[h / 2].x;
            if (dh < bd) { bd = dh; bh = h; }
          }
          unsigned long long bk = dkey(bd, pos0 + bh);
          if (tie3) {   // equal distances meeting at a merge: a tie (two points of one slice: k_moments' check)
            unsigned tt = 0xffffffffu;
            if (tie_xor) {
              bk = xor_min64_eq<16>(bk, tt);
              bk = xor_min64_eq<32>(bk, tt);
            } else {
              bk = xor_min64<16>(bk);
              bk = xor_min64<32>(bk);
            }
            if (on) {
              td = min(td, tt);
              // two of the run's tasks at one distance (tie_scan 4; a leaf met twice in a run is one key)
              if (!mirror && acc != bk && (acc >> 32) == (bk >> 32)) td = min(td, (unsigned)(bk >> 32));
              acc = umin64(acc, bk);
              if (mirror) accm = umin64(accm, mirror_key(bk));   // (a leaf met twice in a run is one key: no false tie)
            }
          } else {
            bk = xor_min64<16>(bk);
            bk = xor_min64<32>(bk);
            if (on) acc = umin64(acc, bk);
          }
        }
        if (on) run_bound = q.w;
      }
      __builtin_amdgcn_wave_barrier();   // reads of `cur` done before it is refilled
    }
  }
  flush_run();
  if (tie3 && !mirror) resolve4();
  else resolve();
}

void launch_align_init(hipStream_t s, AlignJob* job, const AlignJob* job_src) {
  k_align_init<<<1, 128, 0, s>>>(job, job_src);
}
// dynamic LDS of k_nn_seed: [kLinWaves x TaskLds][upper-level box cache]
static size_t collect_lds_bytes(int upper_count) {
  return (size_t)kLinWaves * kTaskLdsBytes + 2 * sizeof(f4v) * (size_t)upper_count;
}
// kTaskRegions-multiple grid of the scan kernel (4 waves per block)
static int scan_blocks(int nsrc) {
  const int groups = (nsrc + kTaskQ - 1) / kTaskQ;
  static const int cap = [] {   // development knob
    const char* v = dev_getenv("DDLO_SCAN_WAVES");
    return v && *v ? std::max(kTaskRegions, std::atoi(v)) : 8192;
  }();
  int waves = std::min(std::max(groups, kTaskRegions), cap);
  waves = (waves + 8 * kTaskRegions - 1) / (8 * kTaskRegions) * (8 * kTaskRegions);
  return waves / kScanWaves;
}
// Bucketed launch geometry: scans of similar size (cfg 5: +-1k points per
// frame) share one captured chunk graph, and a graph never runs with a grid
// or LDS size smaller than the clouds need (all of it is in the graph key).
LinGeom linearize_geometry(int nsrc, int tgt_upper) {
  LinGeom g;
  const int groups = cdiv(std::max(nsrc, 1), kSearchQ);
  const int gcap = cdiv(groups, 1024) * 1024;                    // 16k-point steps
  g.seed_blocks = gcap / kLinWaves;                               // grid-stride kernel: any grid is exact
  g.scan_blocks = scan_blocks(gcap * kSearchQ);                   // any grid is exact
  g.mom_blocks = moment_blocks(cdiv(std::max(nsrc, 1), 32768) * 32768);   // grid-stride; = the slab rows
  g.lds_boxes = std::min(2048, cdiv(std::max(tgt_upper, 1), 128) * 128);   // >= the target's upper boxes
  g.lookup_blocks = gcap / kLinWaves;                                      // one 16-query sub-group per wave
  return g;
}

void launch_cell_lookup(hipStream_t s, const AlignJob* job, const LinGeom& g) {
  k_cell_lookup<<<g.lookup_blocks, 256, 0, s>>>(job);
}
void launch_nn_walk(hipStream_t s, const AlignJob* job, const LinGeom& g) {
  const size_t lds = collect_lds_bytes(g.lds_boxes);
  // with candidate cells the walk gets the few sub-groups without a list:
  // small grids (the kernels are grid-stride loops), so that the usual
  // empty launches cost little
  const int seed_blocks = g.grid ? std::min(g.seed_blocks, 256) : g.seed_blocks;
  k_nn_seed<<<seed_blocks, 64 * kLinWaves, lds, s>>>(job);
  // with candidate cells the walk scanned its (few) sub-groups' tasks inline (AlignJob::task_cap_r = 0)
  if (!g.grid) k_nn_scan<<<g.scan_blocks, 64 * kScanWaves, 0, s>>>(job);
}
int search_queries_per_wave() { return kSearchQ; }
int task_cap_per_region(int nsrc) {
  const long groups = (nsrc + kTaskQ - 1) / kTaskQ;
  return (int)std::max<long>(1024, (groups * kTasksPerGroup + kTaskRegions - 1) / kTaskRegions);
}

}  // namespace ddlo
