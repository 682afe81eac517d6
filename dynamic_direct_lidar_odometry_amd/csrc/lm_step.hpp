// lm_step.hpp — the LM / GN step on one workgroup (K5): slab reduction, the
// normal equations from the moments, every LM trial in its own thread, the
// accept / reject decisions and the new state
// (lsq_registration_impl.hpp:95-232).  Device code inlined at both call
// sites in moments.hip: k_lm_step, and the last block of k_moments when the
// step is fused into the moment kernel (the default on the lookup path).
#pragma once
#include <hip/hip_runtime.h>

#include "gicp_types.hpp"
#include "search.hpp"

namespace ddlo {

// (so3_exp_d and ldlt_solve6_perm are not forced inline -- the compiler
// decides per call site -- so they are static: one definition per TU)
static __device__ void so3_exp_d(const double w[3], double R[9]) {  // gicp/so3.hpp:101-124
  const double theta_sq = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double imag, real;
  if (theta_sq < 1e-10) {
    const double theta_quad = theta_sq * theta_sq;
    imag = 0.5 - 1.0 / 48.0 * theta_sq + 1.0 / 3840.0 * theta_quad;
    real = 1.0 - 1.0 / 8.0 * theta_sq + 1.0 / 384.0 * theta_quad;
  } else {
    const double theta = sqrt(theta_sq);
    const double half = 0.5 * theta;
    double sh, ch;
    sincos(half, &sh, &ch);   // one argument reduction for both
    imag = sh / theta;
    real = ch;
  }
  const double qw = real, qx = imag * w[0], qy = imag * w[1], qz = imag * w[2];
  const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
  const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
  const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
  const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// Eigen::LDLT<Matrix6d>(H + lambda I).solve(rhs) (restated, see oracle).
// Eigen's pivoted LDLT (ldlt_inplace) is left-looking: step k updates only
// row / column k, so the diagonal entries k..5 its pivot search reads are
// still A's own and the transpositions follow from diag(A) alone.  They are
// found first; the factorization then runs unpivoted on the lower triangle of
// P A P^T, gathered from LDS — the same operations on the same values as
// swapping rows and columns in place (checked bit for bit against that form
// on 2M random, tied and rank-deficient systems), without its select chains.
// H, b: LDS (H's lower triangle is read, as Eigen's Lower LDLT); rhs = -b;
// xs: this thread's 6-double LDS row for the un-permuting scatter.  Every
// register-array index is a compile-time constant (no scratch).
static __device__ void ldlt_solve6_perm(const double* H, const double* b, double lambda, double* xs, double x[6]) {
  constexpr int n = 6;
  double v[6];
  int p[6];
#pragma unroll
  for (int i = 0; i < n; ++i) {
    v[i] = fabs(H[7 * i] + lambda);
    p[i] = i;
  }
#pragma unroll
  for (int k = 0; k < n - 1; ++k) {
    // the first largest of v[k..5] (Eigen's maxCoeff keeps the first), swapped to k
    double bv = v[k];
    int bp = p[k], big = k;
#pragma unroll
    for (int i = k + 1; i < n; ++i)
      if (v[i] > bv) { bv = v[i]; bp = p[i]; big = i; }
#pragma unroll
    for (int i = k + 1; i < n; ++i)
      if (big == i) { v[i] = v[k]; p[i] = p[k]; }
    v[k] = bv;
    p[k] = bp;
  }
  double m[36];
#pragma unroll
  for (int i = 0; i < n; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const int hi = max(p[i], p[j]), lo = min(p[i], p[j]);
      m[i * n + j] = i == j ? H[7 * p[i]] + lambda : H[hi * n + lo];
    }
#pragma unroll
  for (int k = 0; k < n; ++k) {
    if (k > 0) {
      double temp[6];
#pragma unroll
      for (int j = 0; j < k; ++j) temp[j] = m[j * n + j] * m[k * n + j];
      double s = 0;
#pragma unroll
      for (int j = 0; j < k; ++j) s += m[k * n + j] * temp[j];
      m[k * n + k] -= s;
#pragma unroll
      for (int i = k + 1; i < n; ++i) {
        double a = 0;
#pragma unroll
        for (int j = 0; j < k; ++j) a += m[i * n + j] * temp[j];
        m[i * n + k] -= a;
      }
    }
    const double akk = m[k * n + k];
    if (k < n - 1 && fabs(akk) > 0.0) {
#pragma unroll
      for (int i = k + 1; i < n; ++i) m[i * n + k] /= akk;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < n; ++i) y[i] = -b[p[i]];   // P rhs
#pragma unroll
  for (int i = 0; i < n; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) y[i] -= m[i * n + j] * y[j];
#pragma unroll
  for (int i = 0; i < n; ++i) y[i] = (fabs(m[i * n + i]) > 2.2250738585072014e-308) ? y[i] / m[i * n + i] : 0.0;
#pragma unroll
  for (int i = n - 1; i >= 0; --i)
#pragma unroll
    for (int j = i + 1; j < n; ++j) y[i] -= m[j * n + i] * y[j];
#pragma unroll
  for (int i = 0; i < n; ++i) xs[p[i]] = y[i];   // P^T y
#pragma unroll
  for (int i = 0; i < n; ++i) x[i] = xs[i];
}

// Moment slots.  W(k,l) = sum M qt_k qt_l (qt = [q;1]), G(m,k) = sum (Me)_m qt_k.
constexpr int mom_ab(int a, int b) {   // symmetric 3 x 3 (a, b) -> 0..5
  return a <= b ? (a == 0 ? b : (a == 1 ? 2 + b : 5)) : (b == 0 ? a : (b == 1 ? 2 + a : 5));
}
constexpr int mom_w(int k, int l, int a, int b) {   // (a, b) entry of W(k, l)
  return (k == 3 && l == 3) ? mom_ab(a, b)
         : k == 3           ? 6 + 6 * l + mom_ab(a, b)
         : l == 3           ? 6 + 6 * k + mom_ab(a, b)
                            : 24 + 6 * mom_ab(k, l) + mom_ab(a, b);
}
constexpr int mom_g(int mm, int k) { return 60 + 4 * mm + k; }
constexpr int kMomY0 = 72, kMomCount = 73;

// The LM step's inputs from the moments, one entry per thread through a
// compile-time table of signed moment slots summed in order:
//   [0, 36)  H = sum J^T M J, [36, 42) b = sum J^T M e, J = [skew(q) | -I]
//            (nano_gicp_impl.hpp:317-324);
//   [42, 186) W12[3k + a][3l + b] = W(k,l)[a][b], [186, 198) g12[3k + r] = G(r, k):
//            the trials' cost decrease y0 - y(delta) = 2 <g12, d> - d^T W12 d over
//            d = vec([Rd - I | td]) (e' = e - D qt for the frozen correspondences).
// Column i of the skew generators S_c has two non-zeros S_c[r][i] = +-1,
// ordered by c, so H_rr(i,j) = sum_{c,d,r,q} S_c[r][i] W(c,d)[r][q] S_d[q][j]
// is a 4-term signed sum (the same products in the same order as the full one).
constexpr int kNeqEntries = 198;
struct NeqTerm {       // packed into three registers: byte t of idx / sgn is term t
  unsigned idx;        // moment slots
  unsigned sgn;        // signs: 1 = +1, 0xff = -1
  unsigned ctl;        // bits 0-7: term count, bit 8: negate the sum
};
struct NeqTable {
  NeqTerm e[kNeqEntries];
};
constexpr void skew_nz_c(int i, int p, int& c, int& r, int& sg) {
  // i=0: S_1[2][0]=-1, S_2[1][0]=+1; i=1: S_0[2][1]=+1, S_2[0][1]=-1; i=2: S_0[1][2]=-1, S_1[0][2]=+1
  constexpr int cc[3][2] = {{1, 2}, {0, 2}, {0, 1}};
  constexpr int rr[3][2] = {{2, 1}, {2, 0}, {1, 0}};
  constexpr int ss[3][2] = {{-1, 1}, {1, -1}, {-1, 1}};
  c = cc[i][p];
  r = rr[i][p];
  sg = ss[i][p];
}
constexpr NeqTable make_neq_table() {
  NeqTable T{};
  auto add = [&](int e, int idx, int sg) {
    const unsigned t = T.e[e].ctl & 0xffu;
    T.e[e].idx |= (unsigned)idx << (8 * t);
    T.e[e].sgn |= (sg < 0 ? 0xffu : 1u) << (8 * t);
    T.e[e].ctl += 1u;
  };
  for (int e = 0; e < 42; ++e) {
    if (e >= 36) {
      const int i = e - 36;
      if (i >= 3) {
        add(e, mom_g(i - 3, 3), -1);   // b_t = -G(:,3)
      } else {                         // b_r(i) = sum_c sum_r S_c[r][i] G(r,c)
        for (int p = 0; p < 2; ++p) {
          int c = 0, r = 0, sg = 0;
          skew_nz_c(i, p, c, r, sg);
          add(e, mom_g(r, c), sg);
        }
      }
      continue;
    }
    const int i = e / 6, j = e % 6;
    if (i < 3 && j < 3) {
      for (int p = 0; p < 2; ++p) {
        int c = 0, r = 0, sr = 0;
        skew_nz_c(i, p, c, r, sr);
        for (int u = 0; u < 2; ++u) {
          int d = 0, q = 0, sq = 0;
          skew_nz_c(j, u, d, q, sq);
          add(e, mom_w(c, d, r, q), sr * sq);
        }
      }
    } else if (i >= 3 && j >= 3) {
      add(e, mom_w(3, 3, i - 3, j - 3), 1);   // H_tt = sum M
    } else {   // H_rt(a, t) = -sum_c sum_r S_c[r][a] W(c,3)[r][t]
      const int a = i < 3 ? i : j, t = i < 3 ? j - 3 : i - 3;
      for (int p = 0; p < 2; ++p) {
        int c = 0, r = 0, sr = 0;
        skew_nz_c(a, p, c, r, sr);
        add(e, mom_w(c, 3, r, t), sr);
      }
      T.e[e].ctl |= 0x100u;
    }
  }
  for (int e = 0; e < 144; ++e) add(42 + e, mom_w(e / 12 / 3, e % 12 / 3, e / 12 % 3, e % 12 % 3), 1);
  for (int e = 0; e < 12; ++e) add(186 + e, mom_g(e % 3, e / 3), 1);
  return T;
}
static __constant__ NeqTable kNeq = make_neq_table();
// One table entry: a single slot is taken as is (times +-1, exact); a sum
// starts from 0.0 and adds its terms in order (as the loops it restates).
__device__ __forceinline__ double neq_term(const NeqTerm& E, const double* mom, int t) {
  const double v = mom[(E.idx >> (8 * t)) & 0xffu];
  return ((E.sgn >> (8 * t)) & 0xffu) == 1u ? v : -v;
}
__device__ __forceinline__ double neq_value(const NeqTerm& E, const double* mom) {
  const unsigned n = E.ctl & 0xffu;
  double s = neq_term(E, mom, 0);
  if (n > 1) {
    s = 0.0 + s;
#pragma unroll
    for (int t = 1; t < 4; ++t)
      if (t < (int)n) s += neq_term(E, mom, t);
  }
  return (E.ctl & 0x100u) ? -s : s;
}

constexpr int kLmThreads = 512;
constexpr int kMaxTrials = 64;
constexpr int kMomBlocksMax = 256;                      // moment-kernel blocks (slab rows)
constexpr int kLmParts = 12;                                          // slab row partitions
// (1024 threads, 25 partitions of 11 rows: reduction 5.5k -> 5.8k cycles, no gain)
constexpr int kLmRowsPerPart = (kMomBlocksMax + kLmParts - 1) / kLmParts;  // slab rows per reducer thread

// Fixed-order reduction of the linearize slab (nblocks x kSlabStride) into
// mom[kSlabStride] by one workgroup: thread (p, v2) sums column pair v2 of
// rows p, p + 12, ... with 16-byte loads (kLmParts x 40 threads), then 80
// threads add the 12 partials in order (fixed order => deterministic).
// mom is complete after the caller's next barrier.
__device__ __forceinline__ void reduce_slab(const double* slab_in, int nb, double (*part)[kSlabStride], double* mom) {
  const int tid = threadIdx.x;
  const auto slab = (const __attribute__((address_space(1))) d2v*)gp(slab_in);
  constexpr int kPairs = kSlabStride / 2;
  if (tid < kLmParts * kPairs) {
    // unconditional (clamped) loads into registers, all issued before the
    // in-order adds consume them (one memory latency, not one per batch the
    // scheduler would otherwise interleave with the adds)
    const int v2 = tid % kPairs, p = tid / kPairs;
    d2v x[kLmRowsPerPart];
#pragma unroll
    for (int r = 0; r < kLmRowsPerPart; ++r) x[r] = slab[(size_t)min(p + kLmParts * r, nb - 1) * kPairs + v2];
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int r = 0; r < kLmRowsPerPart; ++r) {
      const bool in = p + kLmParts * r < nb;
      s0 += in ? x[r].x : 0.0;
      s1 += in ? x[r].y : 0.0;
    }
    part[p][2 * v2] = s0;
    part[p][2 * v2 + 1] = s1;
  }
  __syncthreads();
  if (tid < kSlabStride) {
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < kLmParts; ++p) s += part[p][tid];
    mom[tid] = s;
  }
}

// One workgroup: (1) fixed-order reduction of the linearize partials,
// (2) H, b and the cost-decrease form one entry per thread, (3) every LM
// trial in its own thread — the reference's trial sequence is fully
// determined up front (lambda_i = nu_{i-1} lambda_{i-1}, nu doubling:
// lsq_registration_impl.hpp:187-223), so trial i is evaluated with exactly
// the lambda the sequential loop would use, (4) wavefront 0 takes the
// sequential accept/reject decisions as one ballot and stores the new state
// while the other wavefronts store the per-linearize record.  Every state
// and job word is loaded at the start (its latency hides behind the slab).
#ifdef DDLO_LM_PROF   // developer build (make lmprof): per-phase cycle counts of one LM step, printed by thread 0
#define LM_PROF(i) if (threadIdx.x == 0) lm_t[i] = __builtin_amdgcn_s_memtime()
#define LM_PROF_TRIAL(i) if (threadIdx.x == 0) lm_tt[i] = __builtin_amdgcn_s_memtime()
#else
#define LM_PROF(i)
#define LM_PROF_TRIAL(i)
#endif
// st, slab, nblocks: job->state, job->slab, job->nblocks, passed as kernel
// arguments so the slab loads need no job load first; premom (PREMOM): the
// moments already reduced (and summed across shards: job->mom).
// FRESH (k_moments_fresh, an align's first step without k_align_init before
// it): the state still holds the previous align's words, so the step starts
// from the values the init kernel would have stored (iteration 0, no trials,
// lambda -1, the guess and rec0 from fs) and stores every word the init
// kernel resets whether this step sets it or not; the state it leaves is the
// one k_align_init + the plain step leave, word for word.
template <bool PREMOM, bool FRESH = false>
__device__ __forceinline__ void lm_step_body(const AlignJob* __restrict__ job, AlignState* __restrict__ st,
                                             const double* __restrict__ slab, int nblocks,
                                             const double* __restrict__ premom, const FreshStart* fs = nullptr) {
#ifdef DDLO_LM_PROF
  unsigned long long lm_t[6], lm_tt[4] = {0, 0, 0, 0};
#endif
  LM_PROF(0);
  __shared__ double part[kLmParts][kSlabStride];
  __shared__ double mom[kSlabStride];
  __shared__ double nq[kNeqEntries];   // H (36), b (6), W12 (144), g12 (12)
  double* const Hs = nq;
  double* const bs = nq + 36;
  double* const W12 = nq + 42;
  double* const g12 = nq + 186;
  __shared__ double tr_lambda[kMaxTrials], tr_cm[kMaxTrials], tr_fro[kMaxTrials];
  __shared__ double tr_R[kMaxTrials][9], tr_t[kMaxTrials][3];
  __shared__ double tr_d[kMaxTrials][12], tr_row[kMaxTrials][12], tr_den[kMaxTrials], tr_x[kMaxTrials][6];
  __shared__ double Rt_s[12];
  __shared__ int tr_conv[kMaxTrials];
  const int tid = threadIdx.x;
  // state words, loaded before the slab (their latency overlaps it)
  const int it_pre = FRESH ? 0 : st->iter;
  const int trials_pre = FRESH ? 0 : st->lm_trials;
  const int rec_pre = FRESH ? fs->rec0 : st->rec;
  const float src_radius = st->src_radius;   // (FRESH too: only a whole job changes it)
  const double lambda_pre = FRESH ? -1.0 : st->lambda;
  // the pose, held in a register until the slab loads are issued (an LDS
  // store here would wait for it first)
  double rt_v = 0.0;
  if constexpr (FRESH) {   // the guess: kernel arguments (scalar registers), one select per entry
#pragma unroll
    for (int e = 0; e < 12; ++e)
      if (tid == e) rt_v = e < 9 ? fs->R[e] : fs->t[e - 9];
  } else {
    if (tid < 12) rt_v = tid < 9 ? st->R[tid] : st->t[tid - 9];
  }
  // job words and this thread's table entry too (misses at their first use would each stall a phase)
  const int optimizer = job->optimizer, lm_max_iterations = job->lm_max_iterations;
  const int fixed_iterations = job->fixed_iterations, max_iterations = job->max_iterations;
  const double lm_init_lambda_factor = job->lm_init_lambda_factor;
  const double rotation_epsilon = job->rotation_epsilon, transformation_epsilon = job->transformation_epsilon;
  const int reuse = job->reuse;
  const float reuse_rec_eps = job->reuse_rec_eps, reuse_rec_conv = job->reuse_rec_conv;
  NeqTerm E{};
  if (tid < kNeqEntries) E = kNeq.e[tid];
  if constexpr (PREMOM) {  // moments already reduced (and summed across shards)
    if (tid < kSlabStride) mom[tid] = gp(premom)[tid];
  } else {
    reduce_slab(slab, nblocks, part, mom);
  }
  if (tid < 12) Rt_s[tid] = rt_v;
  __syncthreads();
  LM_PROF(1);
  if (tid < kNeqEntries) nq[tid] = neq_value(E, mom);
  __syncthreads();
  LM_PROF(2);
  const bool lm = optimizer != 0;
  const int ntr = lm ? min(lm_max_iterations, kMaxTrials) : 1;
  // one trial per thread (one wavefront issues them all: a trial per
  // wavefront with wave-uniform pivots measured 2x slower, the waves then
  // share the SIMDs' fp64 issue)
  if (tid < ntr) {
    const int trial = tid;
    double lambda = 0.0;
    if (lm) {
      lambda = lambda_pre;
      if (lambda < 0.0) {   // the first LM step: lm_init_lambda_factor * max |diag H| (:180-183)
        double mx = 0.0;
        for (int e = 0; e < 6; ++e) mx = fmax(mx, fabs(Hs[7 * e]));
        lambda = lm_init_lambda_factor * mx;
      }
      double nu = 2.0;
      for (int k = 0; k < trial; ++k) {
        lambda = nu * lambda;
        nu = 2 * nu;
      }
    }
    LM_PROF_TRIAL(0);
    double d[6];
    ldlt_solve6_perm(Hs, bs, lambda, tr_x[trial], d);   // GN: lambda 0 (H + 0 = H)
    LM_PROF_TRIAL(1);
    double Rd[9], td[3];
    so3_exp_d(d, Rd);
    LM_PROF_TRIAL(2);
    td[0] = d[3]; td[1] = d[4]; td[2] = d[5];
    double den = 0.0;
    for (int e = 0; e < 6; ++e) den += d[e] * (lambda * d[e] - bs[e]);
    tr_den[trial] = den;
    tr_lambda[trial] = lambda;
    // is_converged's measure max((1 / rot_eps) |Rd - I|, (1 / trans_eps) |td|)
    // (lsq_registration_impl.hpp:128-139); the product rounds monotonically,
    // so scaling each largest |x| gives the same maximum
    double mr = 0.0, mt = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) mr = fmax(mr, fabs(Rd[3 * i + j] - (i == j ? 1.0 : 0.0)));
    for (int i = 0; i < 3; ++i) mt = fmax(mt, fabs(td[i]));
    const double cm = fmax(1.0 / rotation_epsilon * mr, 1.0 / transformation_epsilon * mt);
    tr_cm[trial] = cm;
    tr_conv[trial] = fixed_iterations <= 0 && cm < 1;
    double fro = 0.0;
    for (int e = 0; e < 9; ++e) {
      const double dd = Rd[e] - ((e % 4 == 0) ? 1.0 : 0.0);
      fro += dd * dd;
    }
    tr_fro[trial] = fro;
    for (int e = 0; e < 9; ++e) tr_R[trial][e] = Rd[e];
    for (int e = 0; e < 3; ++e) tr_t[trial][e] = td[e];
    // d = vec([Rd - I | td]), d[3k + a] = D[a][k]
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int a = 0; a < 3; ++a) tr_d[trial][3 * k + a] = k < 3 ? Rd[3 * a + k] - (a == k ? 1.0 : 0.0) : td[a];
    LM_PROF_TRIAL(3);
  }
  __syncthreads();
  LM_PROF(3);
  // trial cost decrease, one row of the quadratic form per thread: (trial, row) = (x / 12, x % 12)
  for (int x = tid; lm && x < 12 * ntr; x += (int)blockDim.x) {
    const int tr = x / 12, i = x % 12;
    double srow = 0.0;
#pragma unroll
    for (int j = 0; j < 12; ++j) srow += W12[12 * i + j] * tr_d[tr][j];
    tr_row[tr][i] = tr_d[tr][i] * srow;
  }
  __syncthreads();
  LM_PROF(4);
  if (tid >= 64) {
    // the per-linearize record, stored by the other wavefronts while wavefront 0 decides
    const int u = tid - 64;
    if (u < kSlabStride) st->last_mom[u] = mom[u];
    else if (u < kSlabStride + 9) st->last_lin_R[u - kSlabStride] = Rt_s[u - kSlabStride];
    else if (u < kSlabStride + 12) st->last_lin_t[u - kSlabStride - 9] = Rt_s[u - kSlabStride];
    else if (u < kSlabStride + 18) st->last_b[u - kSlabStride - 12] = bs[u - kSlabStride - 12];
    return;
  }
  // wavefront 0: the trials' gain ratios, then step_lm's sequential decisions
  // (:188-231) as one ballot — the first trial that is accepted (rho >= 0, or
  // NaN) or, rejected, has converged; step_gn always takes its step (:155-173)
  const int lane = tid;
  double rho = 1.0;
  if (lm && lane < ntr) {
    double lin = 0.0, quad = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 4; ++k) lin += tr_d[lane][3 * k + r] * g12[3 * k + r];
#pragma unroll
    for (int i = 0; i < 12; ++i) quad += tr_row[lane][i];
    rho = (2.0 * lin - quad) / tr_den[lane];
  }
  bool ok = true, accept = true;
  int chosen = 0;
  if (lm) {
    const unsigned long long ball = __ballot(lane < ntr && (!(rho < 0) || tr_conv[lane]));
    ok = ball != 0ull;
    chosen = ok ? (int)__builtin_ctzll(ball) : ntr - 1;
    const double rho_c = __shfl(rho, chosen);
    accept = ok && !(rho_c < 0);
    if (lane == 0) {
      st->lm_trials = trials_pre + (ok ? chosen + 1 : ntr);
      if (accept) {
        const double c = 2 * rho_c - 1;
        st->lambda = tr_lambda[chosen] * fmax(1.0 / 3.0, 1 - c * c * c);
      } else if (ok) {
        st->lambda = tr_lambda[chosen];
      } else {
        st->lambda = tr_lambda[ntr - 1] * 2.0;  // not observable: the align ends
      }
    }
  } else if (FRESH && lane == 0) {   // GN leaves both as k_align_init set them
    st->lm_trials = 0;
    st->lambda = -1.0;
  }
  if (lane == 0) {
    st->nr_iterations = it_pre;
    st->final_cost = mom[kMomY0];
    st->num_corr = (int)mom[kMomCount];
    if (rec_pre) st->any_rec = 1;   // this iteration's search recorded references
    else if (FRESH) st->any_rec = 0;
    st->iter = it_pre + 1;
    st->have_prev = 1;
    int done = 0;
    if constexpr (FRESH) {
      const int failed = !ok, conv = ok && tr_conv[chosen];
      st->lm_failed = failed;
      st->converged = conv;
      done = failed | conv;
      if (it_pre + 1 >= max_iterations) done = 1;
      st->done = done;
    } else {
      if (!ok) {
        st->lm_failed = 1;
        done = 1;
      } else if (tr_conv[chosen]) {
        st->converged = 1;
        done = 1;
      }
      if (it_pre + 1 >= max_iterations) done = 1;
      if (done) st->done = 1;
    }
  }
  // accepted: x0 = delta * x0 (compose, lsq_registration_impl.hpp:193-197,225-228),
  // one entry of (Rn | tn) per lane
  double v = 0.0;
  if (accept) {
    const double* Rd = tr_R[chosen];
    if (lane < 9) {
      const int i = lane / 3, j = lane % 3;
      v = Rd[3 * i + 0] * Rt_s[0 + j] + Rd[3 * i + 1] * Rt_s[3 + j] + Rd[3 * i + 2] * Rt_s[6 + j];
      st->R[lane] = v;
    } else if (lane < 12) {
      const int i = lane - 9;
      v = (Rd[3 * i + 0] * Rt_s[9] + Rd[3 * i + 1] * Rt_s[10] + Rd[3 * i + 2] * Rt_s[11]) + tr_t[chosen][i];
      st->t[i] = v;
    } else if (lane >= 16 && lane < 16 + 36) {
      st->final_hessian[lane - 16] = Hs[lane - 16];
    }
  } else if (FRESH && lane < 12) {   // not accepted: the pose stays the guess (final_hessian: no kernel resets it)
    if (lane < 9) st->R[lane] = Rt_s[lane];
    else st->t[lane - 9] = Rt_s[lane];
  }
  int rec = reuse;
  if (accept) {
    // how far the step moved a source point: |dR q + dt - q| <= |dR - I|_F |q| + |dt|,
    // |q| <= src_radius + |t|; the next search records references only
    // after a small step (the one after it is expected to be smaller) ...
    const double tn0 = __shfl(v, 9), tn1 = __shfl(v, 10), tn2 = __shfl(v, 11);
    const double* dt = tr_t[chosen];
    const double mv = sqrt(tr_fro[chosen]) * ((double)src_radius + sqrt(tn0 * tn0 + tn1 * tn1 + tn2 * tn2)) +
                      sqrt(dt[0] * dt[0] + dt[1] * dt[1] + dt[2] * dt[2]);
    // ... and, with the reference's convergence test on, only while the step
    // is still far from converging (is_converged's measure > reuse_rec_conv):
    // references pay off only if two more iterations follow
    rec = rec && mv < (double)reuse_rec_eps && (fixed_iterations > 0 || tr_cm[chosen] > (double)reuse_rec_conv);
  }
  if (lane == 0) st->rec = rec;
  LM_PROF(5);
#ifdef DDLO_LM_PROF
  if (tid == 0)
    printf("lm_prof %d %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", it_pre, lm_t[1] - lm_t[0], lm_t[2] - lm_t[1],
           lm_t[3] - lm_t[2], lm_t[4] - lm_t[3], lm_t[5] - lm_t[4], lm_tt[0] - lm_t[2], lm_tt[1] - lm_tt[0],
           lm_tt[2] - lm_tt[1], lm_tt[3] - lm_tt[2]);
#endif
}

}  // namespace ddlo
