// capi_debug.hip — the diagnostic and test entry points of include/ddlo_gicp.h:
// the search pose by pose (gicp_debug_search_*), nanoflann's tree and its build
// stage by stage, one LM step on given moments, counters, statistics and the
// profiling switches.  None of it runs in an ordinary align.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "cellgrid.hpp"   // maybe_build_grid

extern "C" {

// The search pose by pose (tests): gicp_linearize's start, then one iteration
// per gicp_debug_search_step at the caller's pose and recording flag, on the
// state the previous one left.
gicp_status gicp_debug_search_begin(gicp_ctx* c) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  c->fresh_ok = false;   // (not an align on the graph path)
  c->dbg_search = false;
  begin_ties(c);
  gicp_status s = set_device(c);
  if (s) return s;
  s = maybe_build_grid(c);
  if (s) return s;
  s = prepare_align(c);
  if (s) return s;
  const int ns = c->src.cloud->n;
  s = fill_job(c, nullptr, linearize_blocks(ns));
  if (s) return s;
  c->job_host->optimizer = GICP_OPT_GAUSS_NEWTON;
  c->job_host->max_iterations = 1 << 30;     // never reached: no step ends the sequence
  c->job_host->fixed_iterations = 1 << 30;   // (and no step converges)
  c->job_last_valid = false;                 // the whole job, and the next align's too (the steps patch the device job)
  finalize_job(c);
  JobCommit commit(c);   // not completed: the device job is never taken for an align's
  launch_align_init(c->stream, c->job_dev.as<AlignJob>(), c->job_host_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->state_host, c->state_dev.p, sizeof(AlignState), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->state_slot = 0;
  c->tail_pending = false;
  c->have_align = false;   // no linearization yet
  c->last_nsrc = ns;
  std::memcpy(&c->dbg_job, c->job_host, sizeof(AlignJob));
  c->dbg_search = true;
  return GICP_OK;
}

// The ctx would still build the job gicp_debug_search_begin sent: same clouds,
// covariances, buffers, parameters, shard, tie tree and candidate cells.  A
// setter called since (gicp_set_covariances, gicp_set_params, ...) makes the
// device job stale; the step then refuses instead of running on it.
static gicp_status debug_search_job_current(gicp_ctx* c) {
  if (!c->src.cloud || !c->tgt.cloud || !c->src.has_cov() || !c->tgt.has_cov() || c->src.cloud->n != c->last_nsrc)
    return fail(GICP_ESTATE, "the clouds or covariances changed since gicp_debug_search_begin");
  const unsigned long long ticket = c->ticket;
  gicp_status s = fill_job(c, nullptr, linearize_blocks(c->src.cloud->n));
  c->ticket = ticket;
  if (s) return s;
  AlignJob& j = *c->job_host;
  j.optimizer = c->dbg_job.optimizer;
  j.max_iterations = c->dbg_job.max_iterations;
  j.fixed_iterations = c->dbg_job.fixed_iterations;
  j.job_full = c->dbg_job.job_full;
  j.ticket = c->dbg_job.ticket;
  const bool same = std::memcmp(&j, &c->dbg_job, sizeof(AlignJob)) == 0;
  std::memcpy(&j, &c->dbg_job, sizeof(AlignJob));
  if (!same) {
    c->dbg_search = false;
    return fail(GICP_ESTATE, "the ctx changed since gicp_debug_search_begin (parameters, covariances, shard, cells or tie tree): begin again");
  }
  return GICP_OK;
}

gicp_status gicp_debug_search_step(gicp_ctx* c, const double* pose16, int rec, double* H36, double* b6, double* cost,
                                   int32_t* ncorr) {
  if (!c || !pose16) return fail(GICP_EINVAL, "null argument");
  if (!c->dbg_search || !c->src.cloud || !c->tgt.cloud || c->src.cloud->n != c->last_nsrc)
    return fail(GICP_ESTATE, "gicp_debug_search_begin first");
  gicp_status s = set_device(c);
  if (s) return s;
  s = debug_search_job_current(c);
  if (s) return s;
  begin_ties(c);
  const int ns = c->src.cloud->n;
  const int nblocks = linearize_blocks(ns);
  AlignJob* jd = c->job_dev.as<AlignJob>();
  char* const sd = c->state_dev.as<char>();
  // the words k_lm_step would have left for this iteration: the pose, not done, the recording flag
  struct {
    double Rt[12];
    int done, rec;
  } w;
  for (int r = 0; r < 3; ++r) {
    for (int cc = 0; cc < 3; ++cc) w.Rt[3 * r + cc] = pose16[4 * r + cc];
    w.Rt[9 + r] = pose16[4 * r + 3];
  }
  w.done = 0;
  w.rec = rec ? 1 : 0;
  static_assert(offsetof(AlignState, t) == offsetof(AlignState, R) + 72, "R, t: 12 consecutive doubles");
  // Until the target has its tie tree a step may meet a tie it cannot resolve
  // (tie_pending): the state it found is kept, so that the tree is built and
  // the same step runs again on what the previous step left.
  const bool may_rerun = c->job_host->tie_detect && !c->job_host->tgt_nf.nodes;
  const SearchLayout sl(ns);
  const size_t nb_state = align256(sizeof(AlignState)), nb_corr = align256(sizeof(int) * (size_t)ns),
               nb_search = sl.tasks;   // every per-query array and the counters (the task list is consumed per iteration)
  if (may_rerun) HIP_TRY(c->dbg_snap.ensure(nb_state + 2 * nb_corr + nb_search));
  char* const snap = c->dbg_snap.as<char>();
  auto carry = [&](bool save) -> gicp_status {
    const struct {
      void* p;
      size_t off, n;
    } part[4] = {{c->state_dev.p, 0, sizeof(AlignState)},
                 {c->corr.p, nb_state, sizeof(int) * (size_t)ns},
                 {c->sqd.p, nb_state + nb_corr, sizeof(float) * (size_t)ns},
                 {c->search.p, nb_state + 2 * nb_corr, nb_search}};
    for (const auto& q : part)
      HIP_TRY(hipMemcpyAsync(save ? (void*)(snap + q.off) : q.p, save ? q.p : (void*)(snap + q.off), q.n,
                             hipMemcpyDeviceToDevice, c->stream));
    return GICP_OK;
  };
  for (int rerun = 0;; ++rerun) {
    if (may_rerun) {
      s = carry(rerun == 0);
      if (s) return s;
    }
    HIP_TRY(hipMemcpyAsync(sd + offsetof(AlignState, R), w.Rt, sizeof(w.Rt), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(sd + offsetof(AlignState, done), &w.done, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(sd + offsetof(AlignState, rec), &w.rec, sizeof(int), hipMemcpyHostToDevice, c->stream));
    s = enqueue_iteration(c, jd, nblocks, nullptr);
    if (s) return s;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->state_host, c->state_dev.p, sizeof(AlignState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->state_slot = 0;
    if (!final_state(c).tie_pending || rerun > 0 || !may_rerun) break;
    s = ensure_tie_tree(c);
    if (s) return s;
    // the device job learns of the tree (k_align_init would also reset the state)
    const NfTreeData* tt = c->tgt.cloud->nf.get();
    c->job_host->tgt_nf = tt->dev();
    c->job_host->tgt_nf_status = tt->status.as<int>();
    HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(jd) + offsetof(AlignJob, tgt_nf_status), &c->job_host->tgt_nf_status,
                           sizeof(c->job_host->tgt_nf_status), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(jd) + offsetof(AlignJob, tgt_nf), &c->job_host->tgt_nf,
                           sizeof(NfTreeDev), hipMemcpyHostToDevice, c->stream));
    std::memcpy(&c->dbg_job, c->job_host, sizeof(AlignJob));
  }
  const AlignState& st = final_state(c);
  s = check_ties(c);
  if (s) return s;
  if (st.tie_err || st.tie_pending)
    return fail(GICP_EHIP, "nanoflann tie order: a tied correspondence could not be re-run (bits " +
                               std::to_string(st.tie_err) + ")");
  if (H36) std::memcpy(H36, st.final_hessian, sizeof(double) * 36);
  if (cost) *cost = st.final_cost;
  if (ncorr) *ncorr = st.num_corr;
  if (b6) std::memcpy(b6, st.last_b, sizeof(double) * 6);
  c->have_align = true;
  return GICP_OK;
}

// The per-query search state of the last iteration, in the caller's order
// (tests).  Copies only: the permutation is applied on the host.
gicp_status gicp_debug_search_state(gicp_ctx* c, int32_t* corr, float* sqd, uint32_t* sec, float* ref4, float* refp4,
                                    float* wr, int32_t* any_rec_out, size_t n) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  if (!c->have_align || !c->src.cloud || !c->tgt.cloud) return fail(GICP_ESTATE, "no linearization");
  if ((int)n != c->src.cloud->n || c->last_nsrc != (int)n) return fail(GICP_EINVAL, "n != source size");
  gicp_status s = set_device(c);
  if (s) return s;
  const SearchLayout sl(c->src.cloud->n);
  if (c->search.bytes < sl.total) return fail(GICP_ESTATE, "no search state");
  const int nt = c->tgt.cloud->n;
  std::vector<int> sperm(n), tperm((size_t)nt), hcorr(n);
  std::vector<float> hsqd(n);
  std::vector<unsigned> hsec(n);
  std::vector<float4> href(n), hrefp(n), hq(n);
  const char* u = c->search.as<char>();
  HIP_TRY(hipStreamSynchronize(c->stream));   // (an align's queued no-op chunk)
  int any_rec = 0;
  HIP_TRY(hipMemcpy(&any_rec, c->state_dev.as<char>() + offsetof(AlignState, any_rec), sizeof(int), hipMemcpyDeviceToHost));
  if (any_rec_out) *any_rec_out = any_rec;
  HIP_TRY(hipMemcpy(sperm.data(), c->src.cloud->perm.p, sizeof(int) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tperm.data(), c->tgt.cloud->perm.p, sizeof(int) * (size_t)nt, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hcorr.data(), c->corr.p, sizeof(int) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hsqd.data(), c->sqd.p, sizeof(float) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hsec.data(), u + sl.sec, sizeof(unsigned) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(href.data(), u + sl.ref, sizeof(float4) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hrefp.data(), u + sl.ref_p, sizeof(float4) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hq.data(), u + sl.qstate, sizeof(float4) * n, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {
    const size_t o = (size_t)sperm[i];
    if (o >= n) return fail(GICP_EHIP, "source permutation out of range");
    if (corr) corr[o] = (hcorr[i] >= 0 && hcorr[i] < nt) ? tperm[(size_t)hcorr[i]] : -1;
    if (sqd) sqd[o] = hsqd[i];
    if (sec) sec[o] = hsec[i];
    if (ref4) std::memcpy(ref4 + 4 * o, &href[i], sizeof(float4));   // raw: the search reads it only with any_rec set
    if (refp4) {
      int j;
      std::memcpy(&j, &hrefp[i].w, sizeof(int));
      const int jo = (j >= 0 && j < nt) ? tperm[(size_t)j] : -1;   // int bits, as on the device
      refp4[4 * o] = hrefp[i].x;
      refp4[4 * o + 1] = hrefp[i].y;
      refp4[4 * o + 2] = hrefp[i].z;
      std::memcpy(refp4 + 4 * o + 3, &jo, sizeof(int));
    }
    if (wr) wr[o] = hq[i].w;
  }
  return GICP_OK;
}

gicp_status gicp_get_start_counts(gicp_ctx* c, int64_t* fresh_starts, int64_t* init_starts) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  if (fresh_starts) *fresh_starts = c->fresh_aligns;
  if (init_starts) *init_starts = c->init_aligns;
  return GICP_OK;
}

gicp_status gicp_get_lookup_stats(gicp_ctx* c, int64_t* walk_groups) {
  if (!c || !walk_groups) return fail(GICP_EINVAL, "null argument");
  *walk_groups = -1;
  if (!c->fb.p || !c->src.cloud) return GICP_OK;
  gicp_status s = set_device(c);
  if (s) return s;
  unsigned v = 0;
  const FbLayout fl(c->src.cloud->n);
  HIP_TRY(hipMemcpyAsync(&v, c->fb.as<char>() + fl.ctr + sizeof(unsigned) * kFbSegs * 32, sizeof(unsigned),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *walk_groups = v;
  return GICP_OK;
}

gicp_status gicp_debug_nftree(gicp_ctx* c, int side, int32_t* vind, int32_t* nodes4, float* div2, size_t cap,
                              size_t* nnodes) {
  if (!c || (side != 0 && side != 1) || !nnodes) return fail(GICP_EINVAL, "invalid argument");
  Side& sd = side == GICP_SIDE_SOURCE ? c->src : c->tgt;
  if (!sd.cloud) return fail(GICP_ESTATE, "no cloud on this side");
  gicp_status s = set_device(c);
  if (s) return s;
  s = ensure_nftree(c, *sd.cloud, c->stream);
  if (s) return s;
  const NfTreeData& t = *sd.cloud->nf;
  HIP_TRY(nftree_join(t, c->stream));
  int st[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(st, t.status.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (st[0]) return fail(GICP_EHIP, "nanoflann tree build failed (error bits " + std::to_string(st[0]) + ")");
  *nnodes = (size_t)st[1];
  if (!vind && !nodes4 && !div2) return GICP_OK;
  if (cap < (size_t)st[1]) return fail(GICP_EINVAL, "node capacity too small");
  const int n = t.n;
  DevBuf dv, dn, df;
  HIP_TRY(dv.ensure(sizeof(int) * (size_t)n));
  HIP_TRY(dn.ensure(sizeof(int) * 4 * (size_t)st[1]));
  HIP_TRY(df.ensure(sizeof(float) * 2 * (size_t)st[1]));
  launch_nf_export(c->stream, t.dev(), t.status.as<int>(), st[1], dv.as<int>(), dn.as<int>(), df.as<float>());
  HIP_TRY(hipGetLastError());
  if (vind) HIP_TRY(hipMemcpyAsync(vind, dv.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  if (nodes4) HIP_TRY(hipMemcpyAsync(nodes4, dn.p, sizeof(int) * 4 * (size_t)st[1], hipMemcpyDeviceToHost, c->stream));
  if (div2) HIP_TRY(hipMemcpyAsync(div2, df.p, sizeof(float) * 2 * (size_t)st[1], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GICP_OK;
}

gicp_status gicp_debug_nfbuild(gicp_ctx* c, int side, int stop, int32_t* vind, int64_t* info16, int32_t* status2,
                               void* scratch, size_t scratch_cap) {
  if (!c || (side != 0 && side != 1) || !vind || !info16 || !status2) return fail(GICP_EINVAL, "invalid argument");
  Side& sd = side == GICP_SIDE_SOURCE ? c->src : c->tgt;
  if (!sd.cloud) return fail(GICP_ESTATE, "no cloud on this side");
  gicp_status s = set_device(c);
  if (s) return s;
  NfTreeData t;
  long long off[16];
  s = nftree_build(c, *sd.cloud, c->stream, t, stop, off);
  if (s) return s;
  HIP_TRY(nftree_join(t, c->stream));
  for (int i = 0; i < 16; ++i) info16[i] = off[i];
  HIP_TRY(hipMemcpyAsync(status2, t.status.p, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  std::vector<float4> v((size_t)t.n);
  HIP_TRY(hipMemcpyAsync(v.data(), t.vpts.p, sizeof(float4) * (size_t)t.n, hipMemcpyDeviceToHost, c->stream));
  if (scratch && scratch_cap)
    HIP_TRY(hipMemcpyAsync(scratch, c->nf_scratch.p, std::min(scratch_cap, (size_t)off[13]), hipMemcpyDeviceToHost,
                           c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int i = 0; i < t.n; ++i) {
    int w;
    std::memcpy(&w, &v[(size_t)i].w, sizeof(int));
    vind[i] = w;
  }
  return GICP_OK;
}

gicp_status gicp_get_moments(const gicp_ctx* c, double* out80) {
  if (!c || !out80) return fail(GICP_EINVAL, "null argument");
  std::memcpy(out80, final_state(c).last_mom, sizeof(double) * kSlabStride);
  return GICP_OK;
}

// One k_lm_step launch on given moments, on buffers of its own (tests): the
// ctx lends its params, device and stream only.  The slab holds the step's
// full 256 rows, NaN beyond the caller's, so a sum that reads a row at or
// beyond nrows shows in the result; the step's clamped loads stay inside it.
gicp_status gicp_debug_lm_step(gicp_ctx* c, const gicp_lm_state* in, const double* slab, int nrows, const double* mom80,
                               gicp_lm_state* out) {
  if (!c || !in || !out || !slab == !mom80) return fail(GICP_EINVAL, "null argument (pass either slab or mom80)");
  const int max_rows = lm_slab_rows_max();
  if (slab && (nrows < 1 || nrows > max_rows)) return fail(GICP_EINVAL, "nrows must be in [1, 256]");
  gicp_status s = set_device(c);
  if (s) return s;
  AlignJob j{};
  j.fixed_iterations = c->params.fixed_iterations;
  j.max_iterations = c->params.fixed_iterations > 0 ? c->params.fixed_iterations : c->params.max_iterations;
  j.optimizer = c->params.optimizer;
  j.lm_max_iterations = c->params.lm_max_iterations;
  j.lm_init_lambda_factor = c->params.lm_init_lambda_factor;
  j.transformation_epsilon = c->params.transformation_epsilon;
  j.rotation_epsilon = c->params.rotation_epsilon;
  j.reuse = 0;
  AlignState st{};
  std::memcpy(st.R, in->R, sizeof(st.R));
  std::memcpy(st.t, in->t, sizeof(st.t));
  st.lambda = in->lambda;
  st.final_cost = in->final_cost;
  std::memcpy(st.final_hessian, in->final_hessian, sizeof(st.final_hessian));
  std::memcpy(st.last_b, in->last_b, sizeof(st.last_b));
  std::memcpy(st.last_mom, in->last_mom, sizeof(st.last_mom));
  st.iter = in->iter;
  st.lm_trials = in->lm_trials;
  st.converged = in->converged;
  st.lm_failed = in->lm_failed;
  st.done = 0;   // (a finished state would make the kernel a no-op)
  st.nr_iterations = in->nr_iterations;
  st.num_corr = in->num_corr;
  std::vector<double> rows;
  if (slab) {
    rows.assign((size_t)max_rows * kSlabStride, std::numeric_limits<double>::quiet_NaN());
    std::memcpy(rows.data(), slab, sizeof(double) * (size_t)nrows * kSlabStride);
  } else {
    rows.assign(mom80, mom80 + kSlabStride);
  }
  DevBuf djob, dstate, dmom;
  HIP_TRY(djob.ensure(sizeof(AlignJob)));
  HIP_TRY(dstate.ensure(sizeof(AlignState)));
  HIP_TRY(dmom.ensure(sizeof(double) * rows.size()));
  HIP_TRY(hipMemcpyAsync(djob.p, &j, sizeof(j), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(dstate.p, &st, sizeof(st), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(dmom.p, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice, c->stream));
  launch_lm_step(c->stream, djob.as<AlignJob>(), dstate.as<AlignState>(), slab ? dmom.as<double>() : nullptr,
                 slab ? nrows : 0, slab ? nullptr : dmom.as<double>(), nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&st, dstate.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::memcpy(out->R, st.R, sizeof(st.R));
  std::memcpy(out->t, st.t, sizeof(st.t));
  out->lambda = st.lambda;
  out->final_cost = st.final_cost;
  std::memcpy(out->final_hessian, st.final_hessian, sizeof(st.final_hessian));
  std::memcpy(out->last_b, st.last_b, sizeof(st.last_b));
  std::memcpy(out->last_mom, st.last_mom, sizeof(st.last_mom));
  out->iter = st.iter;
  out->lm_trials = st.lm_trials;
  out->converged = st.converged;
  out->lm_failed = st.lm_failed;
  out->done = st.done;
  out->nr_iterations = st.nr_iterations;
  out->num_corr = st.num_corr;
  out->reserved = 0;
  return GICP_OK;
}

// diagnostics: per 64-query group counters of the LAST linearize launch
gicp_status gicp_debug_stats(gicp_ctx* c, int enable, unsigned int* out, size_t max_words, size_t* nwords) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  c->stats_on = enable != 0;
  if (out && c->src.cloud && c->stats.p) {
    const int q = search_queries_per_wave();
    const size_t groups = (c->src.cloud->n + q - 1) / q;
    const size_t words = std::min(max_words, (size_t)kStatFields * (groups + (groups + 3) / 4));  // phase A + B rows
    HIP_TRY(hipMemcpyAsync(out, c->stats.p, sizeof(unsigned int) * words, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nwords) *nwords = words;
  }
  return GICP_OK;
}

gicp_status gicp_set_profiling(gicp_ctx* c, int enable) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  c->profiling = enable != 0;
  return GICP_OK;
}

gicp_status gicp_get_stage_times(gicp_ctx* c, gicp_stage_times* out) {
  if (!c || !out) return fail(GICP_EINVAL, "null argument");
  std::memset(out, 0, sizeof(*out));
  if (!c->st_ev[0]) return fail(GICP_ESTATE, "no profiled compute_covariances on this ctx");
  gicp_status s = set_device(c);
  if (s) return s;
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipStreamSynchronize(c->aux_stream));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->st_ev[0], c->st_ev[1]));
  out->cov_ms = ms;
  if (c->st_tree) {
    HIP_TRY(hipEventElapsedTime(&ms, c->st_ev[2], c->st_ev[3]));
    out->tree_ms = ms;
  }
  if (c->st_resolve) {
    HIP_TRY(hipEventElapsedTime(&ms, c->st_ev[4], c->st_ev[5]));
    out->resolve_ms = ms;
  }
  return GICP_OK;
}

}  // extern "C"
