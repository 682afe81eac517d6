// moments.hip — K4 and K5 of the GICP hot path: the normal-equation moments
// of the matched pairs and the LM / GN step.
//
//   K4 moments          k_moments                       update_correspondences
//                                                       (M) + linearize :277-336
//   K5 LM / GN step     k_lm_step, k_mom_reduce         lsq_registration_impl.hpp:95-232
//                       (the step itself: lm_step.hpp)  (+ compute_error :339-383
//                                                       evaluated from the moments)
// launch_linearize is one outer iteration up to the moments: the search
// kernels of corr_search.hip (linearize_internal.hpp), then k_moments.
// Compiled with -ffp-contract=off (see index_build.hip).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gicp_types.hpp"
#include "search.hpp"
#include "nftree.hpp"
#include "cov_math.hpp"
#include "launch.hpp"
#include "launch_util.hpp"
#include "linearize_internal.hpp"
#include "lm_step.hpp"

namespace ddlo {

// one matched pair's terms of the moment sums (gicp_types.hpp: the moment slots)
struct Contrib {
  double M[6];   // Mahalanobis (xx xy xz yy yz zz)
  double q[3];   // transformed source point (double)
  double qq[6];  // q_k q_l (00 01 02 11 12 22)
  double v[3];   // M e
  double y;      // e^T M e
  double c;      // 1 if matched
};

template <int S>
__device__ __forceinline__ double moment_val(const Contrib& C) {
  if constexpr (S < 6) {
    return C.M[S];
  } else if constexpr (S < 24) {
    return C.q[(S - 6) / 6] * C.M[(S - 6) % 6];
  } else if constexpr (S < 60) {
    return C.qq[(S - 24) / 6] * C.M[(S - 24) % 6];
  } else if constexpr (S < 72) {
    constexpr int m = (S - 60) / 4, kk = (S - 60) % 4;
    if constexpr (kk == 3)
      return C.v[m];
    else
      return C.v[m] * C.q[kk];
  } else if constexpr (S == 72) {
    return C.y;
  } else if constexpr (S == 73) {
    return C.c;
  } else {
    return 0.0;
  }
}

// In-register transpose reduction step L (L = 1..5): the lane whose bit
// (6 - L) is 0 keeps the lower-half slot a, the other keeps b; each receives
// its partner's copy of the kept slot.  Steps 1 and 2 use the gfx950
// v_permlane32_swap / v_permlane16_swap (no LDS, no selects), steps 3..5 DPP
// row_mirror / row_half_mirror / quad_perm pairings.
__device__ __forceinline__ double dpp_f64(double x, int ctrl_sel) {
  const int lo = __double2loint(x), hi = __double2hiint(x);
  int rlo, rhi;
  switch (ctrl_sel) {
    case 0:  // row_mirror: l <-> 15 - l (bit 3 differs)
      rlo = __builtin_amdgcn_update_dpp(0, lo, 0x140, 0xf, 0xf, false);
      rhi = __builtin_amdgcn_update_dpp(0, hi, 0x140, 0xf, 0xf, false);
      break;
    case 1:  // row_half_mirror: l <-> 7 - l (bit 2 differs)
      rlo = __builtin_amdgcn_update_dpp(0, lo, 0x141, 0xf, 0xf, false);
      rhi = __builtin_amdgcn_update_dpp(0, hi, 0x141, 0xf, 0xf, false);
      break;
    case 2:  // quad_perm [2,3,0,1]: xor 2
      rlo = __builtin_amdgcn_update_dpp(0, lo, 0x4e, 0xf, 0xf, false);
      rhi = __builtin_amdgcn_update_dpp(0, hi, 0x4e, 0xf, 0xf, false);
      break;
    default:  // quad_perm [1,0,3,2]: xor 1
      rlo = __builtin_amdgcn_update_dpp(0, lo, 0xb1, 0xf, 0xf, false);
      rhi = __builtin_amdgcn_update_dpp(0, hi, 0xb1, 0xf, 0xf, false);
      break;
  }
  return __hiloint2double(rhi, rlo);
}

template <int L>
__device__ __forceinline__ double xchg(double a, double b) {
  if constexpr (L == 1 || L == 2) {
    const unsigned alo = __double2loint(a), ahi = __double2hiint(a);
    const unsigned blo = __double2loint(b), bhi = __double2hiint(b);
    unsigned x0, x1, y0, y1;
    if constexpr (L == 1) {
      const auto rl = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
      const auto rh = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
      x0 = rl[0]; y0 = rl[1]; x1 = rh[0]; y1 = rh[1];
    } else {
      const auto rl = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
      const auto rh = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
      x0 = rl[0]; y0 = rl[1]; x1 = rh[0]; y1 = rh[1];
    }
    return __hiloint2double(x1, x0) + __hiloint2double(y1, y0);
  } else {
    const int bit = 1 << (6 - L);
    const bool hi = (lane_id() & bit) != 0;
    const double keep = hi ? b : a;
    const double send = hi ? a : b;
    return keep + dpp_f64(send, L - 3);
  }
}

template <int L, int S>
__device__ __forceinline__ double treduce(const Contrib& C) {
  if constexpr (L == 0) {
    return moment_val<S>(C);
  } else {
    constexpr int half = kMomentSlots >> L;
    const double a = treduce<L - 1, S>(C);
    const double b = treduce<L - 1, S + half>(C);
    return xchg<L>(a, b);
  }
}

__device__ __forceinline__ double final_pair(double x) { return x + dpp_f64(x, 3); }

// slot base of the 3 moments a lane owns after the 5 pairing steps
__device__ __forceinline__ int moment_base(int lane) {
  return 48 * ((lane >> 5) & 1) + 24 * ((lane >> 4) & 1) + 12 * ((lane >> 3) & 1) + 6 * ((lane >> 2) & 1) +
         3 * ((lane >> 1) & 1);
}

__device__ __forceinline__ void load_sym6(const __attribute__((address_space(1))) double* p, double c[6]) {
  const auto q = (const __attribute__((address_space(1))) d2v*)p;
  const d2v a = q[0];
  const d2v b = q[1];
  const d2v d = q[2];
  c[0] = a.x; c[1] = a.y; c[2] = b.x; c[3] = b.y; c[4] = d.x; c[5] = d.y;
}

// K4: Mahalanobis + normal-equation moments of the matched pairs
// (update_correspondences :265-273 + linearize :292-328), 64 points per
// wavefront, in-register transpose reduction, one slab row per block.
constexpr int kMomWaves = 8;    // waves per moment block (512 threads: 256 blocks fill the chip at 131k points)

// Exact ties of update_correspondences' 1-NN (nano_gicp_impl.hpp:255): the
// reference keeps the equidistant point nanoflann's walk meets first
// (KNNResultSet adds only below the worst distance, nanoflann_impl.hpp:1509),
// the search here the lower Morton position.  The lanes in `tied` are re-run,
// one at a time by the whole wavefront, through the target's nanoflann tree
// (nf_search_wave, k = 1), from the same fp32 query; the result must have the
// same distance.  Without a tree the align is flagged (tie_pending): the host
// builds it and runs the align again.  Not inlined: the rare path keeps its
// registers out of the moment loop.
__device__ __forceinline__ void resolve_tied_corr(const AlignJob* __restrict__ job, AlignState* st, const CloudDev& tgt,
                                               bool tied, int i, float kd, int& j, NfWaveStack* S,
                                               bool q_in_regs = false, float qx = 0.f, float qy = 0.f, float qz = 0.f) {
  unsigned long long tm = __ballot(tied);
  const int lane = lane_id();
  const NfTreeDev t = job->tgt_nf;
  if (t.nodes == nullptr) {
    if (lane == __builtin_ctzll(tm)) atomicOr(&st->tie_pending, 1);   // (an atomic: the last block may publish it in this launch)
    return;
  }
  if (*job->tgt_nf_status) {   // the tree build failed: keep the Morton-order answers, report
    if (lane == __builtin_ctzll(tm)) atomicOr(&st->tie_err, 2);
    return;
  }
  int nres = 0;
  while (tm) {
    const int l = __builtin_ctzll(tm);
    tm &= tm - 1;
    const int il = __builtin_amdgcn_readlane(i, l);
    const float dl = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(kd), l));
    // the search's fp32 query (trans_f * a_i, :240,253)
    const float4 q = q_in_regs ? make_float4(readlane_f(qx, l), readlane_f(qy, l), readlane_f(qz, l), 0.f)
                               : ldg4(job->qstate, il);
    float rd;
    int rix;
    int err = 0, jn = -1;
    const bool ok = nf_search_wave(t, q.x, q.y, q.z, 1, S, &rd, &rix);
    // lane 0 holds the (k = 1) result
    rd = __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(rd)));
    rix = __builtin_amdgcn_readfirstlane(rix);
    if (!ok) err = 1;
    else if (__float_as_uint(rd) != __float_as_uint(dl) || rix < 0 || rix >= t.n) err = 16;
    else if ((jn = tgt.inv_perm[rix]) < 0) err = 32;
    if (lane == l) {
      if (jn >= 0) j = jn;
      else atomicOr(&st->tie_err, err);
    }
    ++nres;
  }
  if (lane == 0) atomicAdd(&st->ties_resolved, nres);
}

// FUSE_LM: the LM step runs in the last block to finish (one block per CU:
// 256 blocks), handed off without a release fence -- each block stores its
// slab row write-through (sc1), drains it (vmcnt(0)), and one lane adds to
// an arrival counter (memory-side atomic); the block that arrives last takes
// one agent-scope acquire and reads the slab with plain loads
// (MI355X_MICROARCH.md "visibility", the split-K form of Guideline 16).
// Measured and not kept (DESIGN.md §4 "LM step", round 7): sc1 buffer loads
// of the slab in place of the acquire, with a counter that is never re-armed
// -- no gain on its own or on top of the fence-free publication below.
// The last block then publishes the state itself (publish_state).
// LOOKUP (candidate cells without any fallback cell): the correspondence
// lookup of k_cell_lookup is done here, one query per lane, and the match's
// coordinates are loaded once the scan has named it (tgt.pts[position]: the
// bits of its list entry) -- no lookup kernel, no key / sec round trip.  Same
// keys, ties and moments as k_cell_lookup + k_moments.
// Fused lookup: list entries loaded per round, all of a round's loads issued
// before its first entry is consumed, and scanned by the key alone without a
// branch: about 16 instructions an entry where the branching scan that also
// carried the coordinates took 43, and the scan's instruction issue, not the
// memory system, was what the phase waited for
// (profiles/lookup_scan_summary.md).  Round size: 16 measured 2-4 % faster on
// cfg 3 than 8 (the waves are 2 per SIMD, so the registers are free); 12, 32
// (again with the key-only scan), exec-masked loads, two rounds in flight (8
// or 12 per round) and a flat wavefront-wide scan of all 64 lists (LDS atomic
// min per owner) all slower (tools/mom_timeline.py; -DDDLO_LOOKUP_U for A/B
// builds).
#ifndef DDLO_LOOKUP_U
#define DDLO_LOOKUP_U 16
#endif
constexpr int kLookupU = DDLO_LOOKUP_U;
// Remainder phase of the fused lookup.  Every lane scans entries [0, kTailE0)
// of its own list as above.  A wavefront in which H > 0 lanes then have
// entries left (a ballot) shares them: the heavy lane of rank r (in lane
// order) is served by the aligned team of F lanes r F .. r F + F - 1, F the
// largest power of two with H F <= 64 (at most kTailFCap); member m scans the
// kLookupU-entry chunks c = m (mod F) of [kTailE0, cnt) against the owner's
// query, and the members' partial results are merged by a butterfly over the
// team and moved back to the owner.  The merge (tail_merge) is the second
// order statistic of a union of disjoint entry sets, which is what the
// sequential scan computes, so key and second distance are the sequential
// scan's bit for bit whatever the partition.  H > 32: F = 1, every
// lane goes on alone.  No LDS, no barrier; a wavefront without a long list
// pays one ballot and one branch.  Measured (profiles/lookup_tail_summary.md):
// kTailE0 16 and 48 and a cap of 8 on F slower, a cap of 16 the same; a member
// that loads its next chunk before it consumes the current one more than
// twice as slow (not kept).  (-DDDLO_TAIL_E0 / -DDDLO_TAIL_FCAP: A/B builds.)
#ifndef DDLO_TAIL_E0
#define DDLO_TAIL_E0 32
#endif
#ifndef DDLO_TAIL_FCAP
#define DDLO_TAIL_FCAP 64
#endif
constexpr unsigned kTailE0 = DDLO_TAIL_E0;
constexpr int kTailFCap = DDLO_TAIL_FCAP;
static_assert(kTailE0 > 0 && kTailE0 % kLookupU == 0, "the common rounds end on a round boundary");
static_assert(kTailFCap >= 1 && kTailFCap <= 64 && (kTailFCap & (kTailFCap - 1)) == 0, "team size: a power of two");

// One lane's lookup result over the entries it has seen: the smallest
// (distance, position) key, and the smallest distance of any other entry
// (the second order statistic: it feeds the tie test only).
// The key alone names the match: its coordinates are tgt.pts[position], the
// bits k_cg_emit_* copied into the entry, loaded once after the scan.
// d2 is kept as the distance's bit pattern and folded with the unsigned
// minimum: on the non-negative distances of dist2 that is fminf bit for bit,
// a NaN (any sign) is above +inf and is dropped as fminf drops it, and so is
// the all-ones high word of the empty key ~0 -- no test for it, and none of
// the canonicalising v_max that a float minimum of a selected word costs.
constexpr unsigned kLookupInf = 0x7f800000u;   // +inf: no second distance yet
struct LookupBest {
  unsigned long long bk;
  unsigned d2;
};
// a <- the result over the union of a's and o's (disjoint) entry sets
__device__ __forceinline__ void tail_merge(LookupBest& a, const LookupBest& o) {
  const bool take = o.bk < a.bk;
  const unsigned long long loser = take ? a.bk : o.bk;
  if (take) a.bk = o.bk;
  a.d2 = min(min(a.d2, o.d2), (unsigned)(loser >> 32));
}
__device__ __forceinline__ LookupBest tail_shfl(const LookupBest& s, int src) {
  LookupBest r;
  r.bk = ((unsigned long long)(unsigned)__shfl((int)(unsigned)(s.bk >> 32), src) << 32) |
         (unsigned)__shfl((int)(unsigned)s.bk, src);
  r.d2 = (unsigned)__shfl((int)s.d2, src);
  return r;
}

// developer build (-DDDLO_MOM_PROF): a wave timeline of the fused-lookup
// moment kernel, s_memrealtime stamps (100 MHz, one clock for the device)
// printed by every 16th wavefront
#ifdef DDLO_MOM_PROF
#define MOM_PROF(i) if (LOOKUP) mp_t[i] = __builtin_amdgcn_s_memrealtime()
constexpr int kMomProfIters = 8, kMomProfWaves = 2048;
constexpr int kMomProfWords = 7;   // six stamps, then the remainder phase's word: H | rounds << 8
__device__ unsigned long long g_mom_prof[kMomProfIters * kMomProfWaves * kMomProfWords];   // [iteration][wave][word]
#else
#define MOM_PROF(i)
#endif
// The three tie words of the state are written by whichever block meets a
// tie (resolve_tied_corr: agent-scope atomics), possibly in the launch that
// publishes them: the publishing block's one lane kTieThread fetches them
// with returning agent-scope atomics, which are performed where the other
// blocks' were.  In the fused kernel only after the arrival count has shown
// every block done (each block's waves drain vmcnt before the add).
struct TieWords {
  int pending, resolved, err;
};
constexpr int kTieThread = 64 * (kMomWaves - 1);   // lane 0 of the last wave: idle through the LM step's serial part
__device__ __forceinline__ TieWords fetch_tie_words(AlignState* st) {
  // compare-and-swap of 0 for 0: changes nothing and returns the word.  (An
  // or / add of a constant 0 is compiled to a load, and of an opaque 0 to
  // three wave-reduced atomics, each waited for in turn; these three are
  // issued back to back and waited for with the caller's next loads.)
  TieWords tw{0, 0, 0};
  __hip_atomic_compare_exchange_strong(&st->tie_pending, &tw.pending, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_compare_exchange_strong(&st->ties_resolved, &tw.resolved, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_compare_exchange_strong(&st->tie_err, &tw.err, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  return tw;
}

// Copy the state to the host-mapped slot, then its publication word
// (AlignState::pub: ticket, done, iter), so the host that sees the word reads
// a complete state.  Whole block (64 * kMomWaves threads); tw: thread
// kTieThread's fetch_tie_words.  No thread takes a full fence:
//   1. every wave drains its own stores to st (they are then in this XCD's
//      L2: the L1 is write-through), one barrier;
//   2. the copy reads st with 8-byte sc1 loads, which bypass this CU's L1 and
//      are served by that L2 (a no-op iteration's or k_lm_step's unchanged
//      words come from behind a kernel boundary either way);
//   3. every storing wave drains its pinned stores, one barrier;
//   4. thread 0's system-scope release store of the word, ordered behind the
//      barrier, covers the block's stores.
// ticket: the align's ticket where the device job does not hold it yet
// (k_moments_fresh stores it in this same launch), else nullptr.
__device__ __forceinline__ void publish_state(const AlignJob* __restrict__ job, AlignState* __restrict__ st,
                                              AlignState* __restrict__ publish, const TieWords& tw,
                                              const unsigned long long* ticket = nullptr) {
  static_assert(sizeof(AlignState) % 8 == 0, "AlignState is copied in 8-byte words");
  static_assert(offsetof(AlignState, pub) == sizeof(AlignState) - 8, "the publication word is the last 8 bytes");
  static_assert(offsetof(AlignState, iter) % 8 == 0 && offsetof(AlignState, done) == offsetof(AlignState, iter) + 4,
                "iter and done are one 8-byte word");
  __shared__ int tie_s[3];
  if (threadIdx.x == kTieThread) {
    tie_s[0] = tw.pending;
    tie_s[1] = tw.resolved;
    tie_s[2] = tw.err;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const auto src = gpw(reinterpret_cast<unsigned long long*>(st));
  const auto dst = gpw(reinterpret_cast<unsigned long long*>(publish));
  constexpr int kWords = (int)(sizeof(AlignState) / 8);
  static_assert(kWords <= 64 * kMomWaves && kLmThreads == 64 * kMomWaves, "one 8-byte word per thread");
  // an int of the state at byte offset off, within the 8-byte word w
  auto patch = [](unsigned long long v, int w, size_t off, int val) {
    if ((size_t)w != off / 8) return v;
    const int sh = (int)(off & 4) * 8;
    return (v & ~(0xffffffffull << sh)) | ((unsigned long long)(unsigned)val << sh);
  };
  // (iter, done) for the publication word, from the thread that copies them
  __shared__ unsigned long long iter_s;
  const int w = threadIdx.x;
  if (w < kWords) {
    unsigned long long v = __hip_atomic_load(src + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v = patch(v, w, offsetof(AlignState, tie_pending), tie_s[0]);
    v = patch(v, w, offsetof(AlignState, ties_resolved), tie_s[1]);
    v = patch(v, w, offsetof(AlignState, tie_err), tie_s[2]);
    dst[w] = v;
    if (w == (int)(offsetof(AlignState, iter) / 8)) iter_s = v;
  }
  const unsigned long long tk = ticket ? *ticket : job->ticket;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long id = iter_s;
    const unsigned long long w = (tk << 17) | ((unsigned long long)((unsigned)(id >> 32) != 0u) << 16) | (id & 0xffffu);
    __hip_atomic_store(&publish->pub, w, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// FRESH (k_moments_fresh, below): the first iteration of an align whose job is
// the previous align's but for the guess and the ticket, with no k_align_init
// in front of it.  The state still holds the previous align's words (done
// set), so nothing of it is read at the start: the pose is the guess in fs
// (kernel arguments: uniform, in scalar registers, no load), rec is fs->rec0
// and no earlier iteration recorded; block 0 stores the device job's header
// words and zeroes the walk list's total as the init kernel does, and the
// last block's LM step and publication take their start values and the
// ticket from fs (lm_step_body<.., FRESH>).  What only the host can
// guarantee is its rule for this form (run_align_graph): the three tie words
// are 0 -- any block may add to them in this launch, so no block can reset
// them -- and the arrival word is 0, as every completed fused launch leaves it.
template <bool FUSE_LM, bool LOOKUP, bool FRESH>
__device__ __forceinline__ void moments_body(const AlignJob* __restrict__ job, AlignState* __restrict__ st,
                                             AlignState* __restrict__ publish, const FreshStart* fs) {
  static_assert(!FRESH || (FUSE_LM && LOOKUP), "the fresh start exists for the fused one-kernel lookup iteration only");
#ifdef DDLO_MOM_PROF
  unsigned long long mp_t[kMomProfWords] = {0, 0, 0, 0, 0, 0, 0};
#endif
  MOM_PROF(0);
  double R[9], t[3];
  int st_rec, st_any_rec;
  if constexpr (FRESH) {
    for (int e = 0; e < 9; ++e) R[e] = fs->R[e];
    for (int e = 0; e < 3; ++e) t[e] = fs->t[e];
    st_rec = fs->rec0;
    st_any_rec = 0;
    if (blockIdx.x == 0 && threadIdx.x == 64) {
      // the words k_align_init copies for such an align: the later kernels of
      // the align read the ticket (publish_state) behind a kernel boundary
      static_assert(offsetof(AlignJob, guess_t) == offsetof(AlignJob, guess_R) + 72 &&
                        offsetof(AlignJob, job_full) == offsetof(AlignJob, guess_R) + 96 &&
                        offsetof(AlignJob, ticket) == offsetof(AlignJob, guess_R) + 104,
                    "guess_R, guess_t, job_full, ticket: the job's 14 header words");
      AlignJob* const jw = fs->job_w;
      for (int e = 0; e < 9; ++e) jw->guess_R[e] = fs->R[e];
      for (int e = 0; e < 3; ++e) jw->guess_t[e] = fs->t[e];
      jw->job_full = 0;
      jw->ticket = fs->ticket;
    }
  } else {
    // st (= job->state) is a kernel argument and the pose is loaded with the
    // done flag, before the test: the state words are one load from the
    // arguments, not three dependent ones (job -> state -> done -> pose)
    const auto sg = gp(st);
    for (int e = 0; e < 9; ++e) R[e] = sg->R[e];
    for (int e = 0; e < 3; ++e) t[e] = sg->t[e];
    st_rec = sg->rec;
    st_any_rec = sg->any_rec;
    if (__builtin_amdgcn_readfirstlane(sg->done)) {
      // a no-op iteration after convergence: the chunk's publication still
      // happens (as k_lm_step's after an early exit), by block 0
      if (FUSE_LM && publish && blockIdx.x == 0) {
        TieWords tw{};
        if (threadIdx.x == kTieThread) tw = fetch_tie_words(st);
        publish_state(job, st, publish, tw);
      }
      return;
    }
  }
  const CloudDev src = job->src;
  const CloudDev tgt = job->tgt;
  const auto src_cov = gp(job->src_cov);
  const auto tgt_cov = gp(job->tgt_cov);
  const auto key = gp((const unsigned long long*)job->key);
  const auto corr = gpw(job->corr);
  const auto sqd = gpw(job->sqd);
  const auto slab = gpw(job->slab);
  const double max_corr2 = job->max_corr2;
  const int rec = st_rec;   // this iteration records reuse references
  const int first_rec_done = st_any_rec;   // an earlier iteration of this align recorded
  const int tie_detect = job->tie_detect;
  const bool slice_check = tie_detect && job->tie_scan >= 2 && !(job->tie_ab & 4);
  const bool tie3m = tie_detect && job->tie_scan == 3 && !rec;   // the mirrored key of a non-recording search
  __shared__ NfWaveStack tie_stk[kMomWaves];   // nanoflann search frames of a tied query (per wave)
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
#ifdef DDLO_MOM_PROF
  __builtin_amdgcn_s_waitcnt(0);
#endif
  MOM_PROF(1);
  const int wave = blockIdx.x * kMomWaves + wib;
  const int nwaves_total = gridDim.x * kMomWaves;
  const int ngroups = (src.n + 63) >> 6;
  // the search's task counters are free again: zero them for the next one
  if (blockIdx.x == 0 && threadIdx.x < kTaskRegions) job->task_ctr[threadIdx.x * kCtrStride] = 0u;
  if (blockIdx.x == 0 && job->grid_on && threadIdx.x == 0) {   // the walk list is consumed: its total, then reset
    unsigned t = 0;
    for (int sg = 0; sg < kFbSegs; ++sg) t += job->fb_count[sg * 32];
    if constexpr (FRESH) job->fb_count[kFbSegs * 32] = 0u;   // the align's first iteration (no walk in front of it)
    else job->fb_count[kFbSegs * 32] += t;
    for (int sg = 0; sg < kFbSegs; ++sg) job->fb_count[sg * 32] = 0u;
  }
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  for (int g = wave; g < ngroups; g += nwaves_total) {
    const int i = g * 64 + lane;
    const bool active = i < src.n;
    // the search result key -> correspondences_ / sq_distances_
    // (nano_gicp_impl.hpp:257-258): a match iff a point was found and its
    // squared distance, promoted to double, is below max_corr^2
    int j = -1;
    unsigned kj = 0xffffffffu;
    float kd = INFINITY;
    bool tied = false;
    // the moment operands (a, b, their covariances) are loaded before the tie
    // checks, so those loads overlap them; a re-run query reloads its b
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    double ca[6] = {0, 0, 0, 0, 0, 0}, cb[6] = {0, 0, 0, 0, 0, 0};
    float lqx = 0.f, lqy = 0.f, lqz = 0.f;   // LOOKUP: the fp32 query
    unsigned long long lkey = 0ull;
    unsigned lsec = 0xffffffffu;
    if constexpr (LOOKUP) {
      // k_cell_lookup's arithmetic, one lane per query
      const CellGridDev G = job->grid;
      a = ldg4(src.pts, active ? i : src.n - 1);
      const float Rf0 = (float)R[0], Rf1 = (float)R[1], Rf2 = (float)R[2], Rf3 = (float)R[3], Rf4 = (float)R[4],
                  Rf5 = (float)R[5], Rf6 = (float)R[6], Rf7 = (float)R[7], Rf8 = (float)R[8];
      const float tf0 = (float)t[0], tf1 = (float)t[1], tf2 = (float)t[2];
      lqx = (Rf0 * a.x + Rf1 * a.y) + (Rf2 * a.z + tf0);
      lqy = (Rf3 * a.x + Rf4 * a.y) + (Rf5 * a.z + tf1);
      lqz = (Rf6 * a.x + Rf7 * a.y) + (Rf8 * a.z + tf2);
      const int g16 = i >> 4;
      const float qa = job->own_axis == 0 ? lqx : job->own_axis == 1 ? lqy : lqz;
      const bool owned = active && (job->own_axis < 0 || (qa >= job->own_lo && qa < job->own_hi)) &&
                         (job->own_mod == 0 || (g16 % job->own_mod) == job->own_rem);
      unsigned off = 0, cnt = 0;
      if (owned) {
        const float tx = (lqx - G.ox) * G.inv_s, ty = (lqy - G.oy) * G.inv_s, tz = (lqz - G.oz) * G.inv_s;
        if (tx >= 0.f && tx < (float)G.nx && ty >= 0.f && ty < (float)G.ny && tz >= 0.f && tz < (float)G.nz) {
          cg_cell_list(G, tx, ty, tz, off, cnt);   // (no fallback cell in LOOKUP mode)
        }
      }
      // (the second distance feeds the tie test only: without tie_detect it is
      // computed all the same, one instruction an entry, and lsec is not read)
      LookupBest own{~0ull, kLookupInf};
      constexpr int kU = kLookupU;   // loads in flight
      // Entries [k, k + kU) of the list of n (k < n), against the query q, into
      // r: no branch, the key alone.  An entry past the list's end (what the
      // loads return there: the next list's entries, often this list's own
      // points again) takes the all-ones word for its distance: with a real
      // entry in front of it in every round its key is above r.bk, so it never
      // wins, and the word is above every distance, so it never reaches d2.
      // The loser's distance goes to d2; the empty key's high word is that
      // same word (the first entry adds nothing to d2).
      auto consume = [&](const float4 (&pp)[kU], unsigned k, unsigned n, float qx, float qy, float qz, LookupBest& r) {
        const unsigned left = n - k;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const float dd = dist2(qx, qy, qz, pp[u].x, pp[u].y, pp[u].z);
          const unsigned dw = (unsigned)u < left ? __float_as_uint(dd) : 0xffffffffu;
          const unsigned long long kk = ((unsigned long long)dw << 32) | (unsigned)__float_as_int(pp[u].w);
          const bool take = kk < r.bk;
          r.d2 = min(r.d2, take ? (unsigned)(r.bk >> 32) : dw);
          r.bk = take ? kk : r.bk;
        }
      };
      // One address per round, the loads at immediate offsets.  They run up to
      // kU - 1 entries past the list's end: inside the buffer, which
      // cellgrid_build pads by kCgEntPad entries.  (Clamped per-load addresses
      // cost 70 instructions a round more and measured the same or slower.)
      static_assert(kU <= kCgEntPad, "a round reads at most kCgEntPad entries past a list's end");
      auto fetch = [&](float4 (&pp)[kU], unsigned k, unsigned lo) {
        const float4* const p = G.ent + (size_t)(lo + k);
#pragma unroll
        for (int u = 0; u < kU; ++u) pp[u] = ldg4(p, u);
        // every load of the round is issued before the first entry is consumed
        // (without the branches the scheduler would sink the loads between them)
        __builtin_amdgcn_sched_barrier(0);
      };
      const unsigned c0 = min(cnt, kTailE0);
      for (unsigned k = 0; k < c0; k += kU) {
        float4 pp[kU];
        fetch(pp, k, off);
        consume(pp, k, cnt, lqx, lqy, lqz, own);
      }
      // the remainder phase (kTailE0): lists longer than the common rounds
      const bool heavy = cnt > kTailE0;
      const unsigned long long rem = __ballot(heavy);
      if (rem != 0ull) {
        const int H = __popcll(rem);
        int lf = 0;   // log2 of the team size
        while ((H << (lf + 1)) <= 64 && (2 << lf) <= kTailFCap) ++lf;
        const int F = 1 << lf;
        const int rank = __popcll(rem & ((1ull << lane) - 1ull));   // a heavy lane's rank
        // the lane this one serves: its own (F = 1), or the heavy lane whose rank is this lane's team
        int owner = lane;
        if (F > 1) {
          const int team = lane >> lf;
          owner = -1;   // (H F < 64: the teams from H on are idle)
          int r = 0;
          for (unsigned long long mm = rem; mm; mm &= mm - 1, ++r)
            if (team == r) owner = __builtin_ctzll(mm);
        }
        const int osrc = owner < 0 ? lane : owner;
        const unsigned ooff = (unsigned)__shfl((int)off, osrc);
        const unsigned ocnt0 = (unsigned)__shfl((int)cnt, osrc);   // (every lane takes part: a lane left out reads as 0)
        const unsigned ocnt = owner < 0 ? 0u : ocnt0;
        const float oqx = __shfl(lqx, osrc), oqy = __shfl(lqy, osrc), oqz = __shfl(lqz, osrc);
        LookupBest mine{~0ull, kLookupInf};
        const unsigned stride = (unsigned)kU << lf;
        unsigned k = kTailE0 + (unsigned)kU * (unsigned)(lane & (F - 1));
#ifdef DDLO_MOM_PROF
        int rounds = 0;
#define MOM_PROF_ROUND ++rounds
#else
#define MOM_PROF_ROUND
#endif
        for (; k < ocnt; k += stride) {
          float4 pp[kU];
          fetch(pp, k, ooff);
          consume(pp, k, ocnt, oqx, oqy, oqz, mine);
          MOM_PROF_ROUND;
        }
#undef MOM_PROF_ROUND
        // the team's result in every member, then in the owner
        for (int m = 1; m < F; m <<= 1) tail_merge(mine, tail_shfl(mine, lane ^ m));
        const LookupBest got = tail_shfl(mine, heavy && F > 1 ? rank << lf : lane);   // (F = 1: its own)
        if (heavy) tail_merge(own, got);
#ifdef DDLO_MOM_PROF
        mp_t[6] = (unsigned long long)H | ((unsigned long long)wave_max((float)rounds) << 8);
#endif
      }
      const unsigned long long bk = own.bk;
      const unsigned d2 = own.d2;
      lkey = owned ? umin64(bk, dkey(job->cap2, -1)) : dkey(INFINITY, -1);
      lsec = (owned && (unsigned)lkey != 0xffffffffu && d2 == (unsigned)(lkey >> 32)) ? (unsigned)(lkey >> 32) : 0xffffffffu;

      MOM_PROF(2);
    }
    if (active) {
      const unsigned long long k = LOOKUP ? lkey : key[i];
      // independent of the key: issued with it
      const unsigned sv = !tie_detect ? 0xffffffffu : LOOKUP ? lsec : job->sec[i];
      const unsigned k2lo = (tie3m && !LOOKUP) ? (unsigned)job->key2[i] : 0u;
      kj = (unsigned)k;
      kd = __uint_as_float((unsigned)(k >> 32));
      j = (kj != 0xffffffffu && (double)kd < max_corr2) ? (int)kj : -1;
      if (j >= 0) {
        if constexpr (!LOOKUP) a = ldg4(src.pts, i);   // (LOOKUP: a is in registers already)
        b = ldg4(tgt.pts, j);   // (LOOKUP: the bits of the winning entry, issued with the covariances)
        load_sym6(src_cov + 6 * (size_t)i, ca);
        load_sym6(tgt_cov + 6 * (size_t)j, cb);
      }
      // another examined point at the nearest distance: an exact tie.  sec:
      // all ones = not searched (a reuse reference proved the match), else
      // the smallest distance met twice / of a non-best point (never below
      // the key's); tie_scan 3 also: the mirrored key names another point
      const bool searched = tie_detect && j >= 0 && sv != 0xffffffffu;
      tied = searched && sv <= (unsigned)(k >> 32);
      if (tie3m && searched && !LOOKUP) tied = tied || k2lo != ((unsigned)k ^ 0xffffffffu);
      // tie_scan >= 2: the scan compares only the 8-point slices' bests, so a
      // second point at the distance inside the winner's own slice (the 8
      // aligned sorted positions one lane scanned; the same 128-B line as the
      // winner) is checked here, in the scan's fp32 arithmetic
      if (slice_check && searched && !tied) {
        // the search's fp32 query, recomputed (k_nn_seed's transform, same operations)
        const float qx = ((float)R[0] * a.x + (float)R[1] * a.y) + ((float)R[2] * a.z + (float)t[0]);
        const float qy = ((float)R[3] * a.x + (float)R[4] * a.y) + ((float)R[5] * a.z + (float)t[1]);
        const float qz = ((float)R[6] * a.x + (float)R[7] * a.y) + ((float)R[8] * a.z + (float)t[2]);
        const int b0 = j & ~7;
#pragma unroll
        for (int h = 0; h < 8; ++h) {
          const float4 p = ldg4(tgt.pts, b0 + h);
          tied = tied || (b0 + h != j && dist2(qx, qy, qz, p.x, p.y, p.z) == kd);
        }
      }
    }
    // nanoflann's choice among the tied points (wave-uniform, rare)
    if (tie_detect && __any(tied)) {
      const int j0 = j;
      resolve_tied_corr(job, st, tgt, tied, i, kd, j, &tie_stk[wib], LOOKUP, lqx, lqy, lqz);
      if (tied) kj = (unsigned)j;
      if (j != j0) {   // another point of the same distance: its coordinates and covariance
        b = ldg4(tgt.pts, j);
        load_sym6(tgt_cov + 6 * (size_t)j, cb);
      }
    }
    if (active) {
      corr[i] = j;
      sqd[i] = kj != 0xffffffffu ? kd : INFINITY;
      // reuse reference of a query searched in a recording iteration: its
      // position, B^2 = min(smallest distance of an examined non-best point,
      // walk radius) — every unexamined point lies in a leaf farther than the
      // walk radius — and its match.  A reference stays a valid proof for
      // the rest of the align (same target), so other iterations keep it.
      if (rec && !LOOKUP) {   // (LOOKUP: no walk, so no reference is ever checked)
        const float4 qs = ldg4(job->qstate, i);
        if (qs.w >= 0.f) {
          job->ref[i] = make_float4(qs.x, qs.y, qs.z, fminf(__uint_as_float(job->sec[i]), qs.w));
          float4 pp = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
          if (kj != 0xffffffffu) {
            const float4 p = ldg4(tgt.pts, (int)kj);
            pp = make_float4(p.x, p.y, p.z, __int_as_float((int)kj));
          }
          job->ref_p[i] = pp;
        } else if (!first_rec_done) {
          // the align's first recording iteration: a query it did not search
          // (another shard's) must not keep a previous align's reference
          job->ref[i] = make_float4(0.f, 0.f, 0.f, -1.f);
        }
      }
    }
    Contrib C;
    if (j >= 0) {
      const double A[9] = {ca[0], ca[1], ca[2], ca[1], ca[3], ca[4], ca[2], ca[4], ca[5]};
      // RC = R * CA ; S = RC * R^T ; RCR = CB + S
      double RC[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) RC[3 * r + cc] = R[3 * r] * A[cc] + R[3 * r + 1] * A[3 + cc] + R[3 * r + 2] * A[6 + cc];
      double S[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) S[3 * r + cc] = RC[3 * r] * R[3 * cc] + RC[3 * r + 1] * R[3 * cc + 1] + RC[3 * r + 2] * R[3 * cc + 2];
      const double Cm[9] = {cb[0] + S[0], cb[1] + S[1], cb[2] + S[2], cb[1] + S[3], cb[3] + S[4],
                            cb[4] + S[5], cb[2] + S[6], cb[4] + S[7], cb[5] + S[8]};
      double Mi[9];
      inv3(Cm, Mi);
      C.M[0] = Mi[0]; C.M[1] = 0.5 * (Mi[1] + Mi[3]); C.M[2] = 0.5 * (Mi[2] + Mi[6]);
      C.M[3] = Mi[4]; C.M[4] = 0.5 * (Mi[5] + Mi[7]); C.M[5] = Mi[8];
      const double ax = a.x, ay = a.y, az = a.z;
      C.q[0] = (R[0] * ax + R[1] * ay) + (R[2] * az + t[0]);
      C.q[1] = (R[3] * ax + R[4] * ay) + (R[5] * az + t[1]);
      C.q[2] = (R[6] * ax + R[7] * ay) + (R[8] * az + t[2]);
      const double e0 = (double)b.x - C.q[0], e1 = (double)b.y - C.q[1], e2 = (double)b.z - C.q[2];
      C.v[0] = C.M[0] * e0 + C.M[1] * e1 + C.M[2] * e2;
      C.v[1] = C.M[1] * e0 + C.M[3] * e1 + C.M[4] * e2;
      C.v[2] = C.M[2] * e0 + C.M[4] * e1 + C.M[5] * e2;
      C.y = e0 * C.v[0] + e1 * C.v[1] + e2 * C.v[2];
      C.c = 1.0;
    } else {
      for (int e = 0; e < 6; ++e) C.M[e] = 0.0;
      C.q[0] = C.q[1] = C.q[2] = 0.0;
      C.v[0] = C.v[1] = C.v[2] = 0.0;
      C.y = 0.0;
      C.c = 0.0;
    }
    C.qq[0] = C.q[0] * C.q[0]; C.qq[1] = C.q[0] * C.q[1]; C.qq[2] = C.q[0] * C.q[2];
    C.qq[3] = C.q[1] * C.q[1]; C.qq[4] = C.q[1] * C.q[2]; C.qq[5] = C.q[2] * C.q[2];
    MOM_PROF(3);
    acc0 += final_pair(treduce<5, 0>(C));
    acc1 += final_pair(treduce<5, 1>(C));
    acc2 += final_pair(treduce<5, 2>(C));
  }
  MOM_PROF(4);
  __shared__ double red[kMomWaves][kMomentSlots];
  if ((lane & 1) == 0) {
    const int base = moment_base(lane);
    red[wib][base + 0] = acc0;
    red[wib][base + 1] = acc1;
    red[wib][base + 2] = acc2;
  }
  __syncthreads();
  if (threadIdx.x < kSlabStride) {
    double sum = 0.0;
    if (threadIdx.x < kMoments)
      for (int w = 0; w < kMomWaves; ++w) sum += red[w][threadIdx.x];
    if constexpr (FUSE_LM)
      __hip_atomic_store((__attribute__((address_space(1))) unsigned long long*)(slab + (size_t)blockIdx.x * kSlabStride +
                                                                                 threadIdx.x),
                         (unsigned long long)__double_as_longlong(sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      slab[(size_t)blockIdx.x * kSlabStride + threadIdx.x] = sum;
  }
#ifdef DDLO_MOM_PROF
  MOM_PROF(5);
  if (LOOKUP && lane == 0 && wave < kMomProfWaves) {
    unsigned long long* o = g_mom_prof + ((size_t)min(st->iter, kMomProfIters - 1) * kMomProfWaves + wave) * kMomProfWords;
    for (int e = 0; e < kMomProfWords; ++e) o[e] = mp_t[e];
  }
#endif
  if constexpr (FUSE_LM) {
    __shared__ int last_s;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave: its sc1 slab stores are done
    __syncthreads();
    unsigned* const arrive = job->task_ctr + kTaskRegions * kCtrStride;   // the word after the regions' counters
    if (threadIdx.x == 0) last_s = atomicAdd(arrive, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!last_s) return;
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // re-armed for the next iteration, and for the next align's when that starts without
      // k_align_init, which zeroes it per align
      atomicExch(arrive, 0u);
    }
    __syncthreads();
    // every block has arrived, so the tie words are final: fetched in flight with the slab loads
    TieWords tw{};
    if (publish && threadIdx.x == kTieThread) tw = fetch_tie_words(st);
    lm_step_body<false, FRESH>(job, st, job->slab, job->nblocks, nullptr, fs);
    if (publish) publish_state(job, st, publish, tw, FRESH ? &fs->ticket : nullptr);
  }
}

template <bool FUSE_LM, bool LOOKUP = false>
__global__ __launch_bounds__(64 * kMomWaves) void k_moments(const AlignJob* __restrict__ job,
                                                            AlignState* __restrict__ st, AlignState* __restrict__ publish) {
  moments_body<FUSE_LM, LOOKUP, false>(job, st, publish, nullptr);
}
// The fused lookup iteration as an align's first kernel (moments_body<.., FRESH>).
__global__ __launch_bounds__(64 * kMomWaves) void k_moments_fresh(const AlignJob* __restrict__ job,
                                                                  AlignState* __restrict__ st,
                                                                  AlignState* __restrict__ publish, const FreshStart fs) {
  moments_body<true, true, true>(job, st, publish, &fs);
}
template __global__ void k_moments<false>(const AlignJob*, AlignState*, AlignState*);
template __global__ void k_moments<true>(const AlignJob*, AlignState*, AlignState*);
template __global__ void k_moments<false, true>(const AlignJob*, AlignState*, AlignState*);
template __global__ void k_moments<true, true>(const AlignJob*, AlignState*, AlignState*);

// K5a (sharded align only): this rank's reduced moments -> job->mom, which
// the host's all-reduce then sums across ranks before k_lm_step.
__global__ __launch_bounds__(kLmThreads) void k_mom_reduce(const AlignJob* __restrict__ job) {
  AlignState* st = job->state;
  if (__builtin_amdgcn_readfirstlane(st->done)) return;
  __shared__ double part[kLmParts][kSlabStride];
  __shared__ double mom[kSlabStride];
  reduce_slab(job->slab, job->nblocks, part, mom);
  __syncthreads();
  if (threadIdx.x < kSlabStride) gpw(job->mom)[threadIdx.x] = mom[threadIdx.x];
}

// publish (optional): a host-mapped AlignState the block copies the final
// state of this step to (also after an early exit), so the host reads a
// chunk's result from pinned memory without a device-to-host copy.
__global__ __launch_bounds__(kLmThreads) void k_lm_step(const AlignJob* __restrict__ job, AlignState* __restrict__ st,
                                                        const double* __restrict__ slab, int nblocks,
                                                        const double* __restrict__ premom,
                                                        AlignState* __restrict__ publish) {
  TieWords tw{};
  if (publish && threadIdx.x == kTieThread) tw = fetch_tie_words(st);
  if (!__builtin_amdgcn_readfirstlane(st->done)) {
    if (premom) lm_step_body<true>(job, st, slab, nblocks, premom);
    else lm_step_body<false>(job, st, slab, nblocks, nullptr);
  }
  if (publish) publish_state(job, st, publish, tw);
}

bool linearize_is_one_kernel(const LinGeom& g) {
  static const int fused_lookup = env_knob("DDLO_GRID_FUSED", 1);   // 0: separate lookup kernel (A/B)
  return g.grid && !g.grid_walk && fused_lookup;
}
void launch_linearize(hipStream_t s, const AlignJob* job, const LinGeom& g, AlignState* publish) {
  if (linearize_is_one_kernel(g)) {
    // every query is answered by its cell: the lookup runs inside the moment kernel
    if (g.fuse_lm) k_moments<true, true><<<g.mom_blocks, 64 * kMomWaves, 0, s>>>(job, g.state, publish);
    else k_moments<false, true><<<g.mom_blocks, 64 * kMomWaves, 0, s>>>(job, g.state, nullptr);
    return;
  }
  if (g.grid) launch_cell_lookup(s, job, g);
  // (no walk when every query is answered by its cell, or provably unmatched)
  if (!g.grid || g.grid_walk) launch_nn_walk(s, job, g);
  if (g.fuse_lm) k_moments<true><<<g.mom_blocks, 64 * kMomWaves, 0, s>>>(job, g.state, publish);
  else k_moments<false><<<g.mom_blocks, 64 * kMomWaves, 0, s>>>(job, g.state, nullptr);
}
void launch_linearize_fresh(hipStream_t s, const AlignJob* job, const LinGeom& g, const FreshStart& fs,
                            AlignState* publish) {
  // (the caller has checked the geometry: linearize_is_one_kernel(g) && g.fuse_lm)
  k_moments_fresh<<<g.mom_blocks, 64 * kMomWaves, 0, s>>>(job, g.state, publish, fs);
}
int moment_blocks(int nsrc) {
  const int groups = (nsrc + 63) / 64;
  return std::max(1, std::min((groups + kMomWaves - 1) / kMomWaves, kMomBlocksMax));
}
int lm_slab_rows_max() { return kMomBlocksMax; }
void launch_lm_step(hipStream_t s, const AlignJob* job, AlignState* st, const double* slab, int nblocks,
                    const double* premom, AlignState* publish) {
  k_lm_step<<<1, kLmThreads, 0, s>>>(job, st, slab, nblocks, premom, publish);
}
void launch_mom_reduce(hipStream_t s, const AlignJob* job) { k_mom_reduce<<<1, kLmThreads, 0, s>>>(job); }

}  // namespace ddlo

#ifdef DDLO_MOM_PROF
// developer build: the fused moment kernel's wave stamps of the last align, [iteration][wave][7]
extern "C" int ddlo_dev_mom_prof(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ddlo::g_mom_prof), sizeof(ddlo::g_mom_prof));
}
#endif
