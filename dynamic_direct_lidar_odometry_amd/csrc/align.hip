// align.hip — the align engine behind gicp_align, gicp_linearize and
// gicp_s2s_batch.
//
// An align runs as hipGraphs of chunks:
//   k_align_init, then max_iterations x {k_linearize, k_lm_step}
// whose kernels become no-ops once the on-device LM has converged or
// failed.  The host polls the published state once per chunk and reads the
// pose from it.  The whole per-align host path (gicp_align, prepare_align,
// fill_job, finalize_job, run_align_graph) is in this file: its time is part
// of every align's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "capi_internal.hpp"
#include "cellgrid.hpp"   // maybe_build_grid
#include "comm.hpp"

namespace {

// Tuning knob of the search (development; the default is the tuned value)
constexpr float kSplitExtentDefault = 5.0f;
float env_float(const char* name, float dflt) {
  const char* v = dev_getenv(name);
  if (!v || !*v) return dflt;
  char* end = nullptr;
  const float f = std::strtof(v, &end);
  return (end && end != v && f >= 0.f) ? f : dflt;
}

int env_int(const char* name, int dflt) {
  const char* v = dev_getenv(name);
  return (v && *v) ? std::atoi(v) : dflt;
}

// The search's development knobs, read from the environment once per
// process, not on every align (host time between aligns).
struct SearchKnobs {
  float split_extent, probe, probe_d, tri_mv, reuse_gap, reuse_gap0, reuse_rec_eps, reuse_rec_conv;
  int xcd_scan, pf_ratio, prev_window, reuse, reuse_rec0, tie_scan, tie_ab;
};
const SearchKnobs& search_knobs() {
  static const SearchKnobs k = [] {
    SearchKnobs v;
    v.split_extent = env_float("DDLO_SPLIT_EXTENT", kSplitExtentDefault);
    v.xcd_scan = env_int("DDLO_XCD_SCAN", 1);
    v.pf_ratio = env_int("DDLO_PF_RATIO", 2);
    v.prev_window = env_int("DDLO_PREV_WINDOW", 2);
    v.tri_mv = env_float("DDLO_TRI_MV", 0.2f);
    v.probe = env_float("DDLO_PROBE", 1.0f);
    v.probe_d = env_float("DDLO_PROBE_D", 0.5f);
    v.reuse = env_int("DDLO_REUSE", 1);
    v.reuse_gap = env_float("DDLO_REUSE_GAP", 0.05f);
    v.reuse_gap0 = env_float("DDLO_REUSE_GAP0", 0.f);
    v.reuse_rec0 = env_int("DDLO_REUSE_REC0", 0);
    v.reuse_rec_eps = env_float("DDLO_REUSE_REC_EPS", 0.05f);
    v.reuse_rec_conv = env_float("DDLO_REUSE_REC_CONV", 10.f);
    v.tie_ab = env_int("DDLO_TIE_AB", 0);
    v.tie_scan = env_int("DDLO_TIE_SCAN", 4);   // 1 / 2 / 3 / 4 (see AlignJob::tie_scan); 0 = A/B only
    return v;
  }();
  return k;
}

constexpr int kMaxFirstChunk = 8;  // largest predicted first chunk (iterations)
// With fixed_iterations the count is known, so the whole align is one graph
// (up to this many iterations): every later chunk is a separate graph launch
// and a host round trip (cfg 2: 20 iterations were 1 + 12 chunks)
constexpr int kMaxFixedChunk = 64;

}  // namespace

// the search bound of an align: nextafter(float(max_corr^2), +inf) (AlignJob::cap2)
float ddlo::rt::search_cap2(const gicp_params& p) {
  const double r = p.max_correspondence_distance;
  float f = (float)(r * r);
  if (!std::isfinite(f)) f = FLT_MAX;
  return std::nextafter(f, INFINITY);
}

// The target's candidate cells answer this ctx's searches (same bound)
bool ddlo::rt::grid_active(const gicp_ctx* c) {
  if (!c->grid_mode || !c->tgt.cloud) return false;
  const auto& g = c->tgt.cloud->grid;
  return g && g->ok && g->cap2 == search_cap2(c->params);
}

// Just before k_align_init reads the pinned job: whole (job_full = 1) unless
// only the guess changed since the job it last copied whole, whose device copy
// is still in place (k_align_init alone writes the device job).
// finalize_job records the job as the device's copy before anything is
// launched; an error return before the launch has happened must forget it,
// or the next align would send only its guess to a device job that never
// received this one (JobCommit: armed after finalize_job, done() once the
// launch succeeded).
void ddlo::rt::finalize_job(gicp_ctx* c) {
  AlignJob& j = *c->job_host;
  j.job_full = 0;
  AlignJob probe = j;
  std::memcpy(probe.guess_R, c->job_last.guess_R, sizeof(probe.guess_R));
  std::memcpy(probe.guess_t, c->job_last.guess_t, sizeof(probe.guess_t));
  probe.job_full = c->job_last.job_full;
  probe.ticket = c->job_last.ticket;
  if (!c->job_last_valid || std::memcmp(&probe, &c->job_last, sizeof(AlignJob)) != 0) {
    j.job_full = 1;
    c->job_last = j;
    c->job_last_valid = true;
  }
}

gicp_status ddlo::rt::fill_job(gicp_ctx* c, const float* guess16, int nblocks) {
  const SearchKnobs& kn = search_knobs();
  AlignJob& j = *c->job_host;
  std::memset(&j, 0, sizeof(j));
  j.src = c->src.cloud->dev();
  j.tgt = c->tgt.cloud->dev();
  j.src_cov = c->src.cov->cov6.as<double>();
  j.tgt_cov = c->tgt.cov->cov6.as<double>();
  j.corr = c->corr.as<int>();
  j.sqd = c->sqd.as<float>();
  j.slab = c->slab.as<double>();
  j.state = c->state_dev.as<AlignState>();
  j.ticket = (++c->ticket) & ((1ull << 47) - 1);
  j.stats = c->stats_on ? c->stats.as<unsigned int>() : nullptr;
  for (int r = 0; r < 3; ++r) {
    for (int cc = 0; cc < 3; ++cc) j.guess_R[3 * r + cc] = guess16 ? (double)guess16[4 * r + cc] : (r == cc ? 1.0 : 0.0);
    j.guess_t[r] = guess16 ? (double)guess16[4 * r + 3] : 0.0;
  }
  const double r = c->params.max_correspondence_distance;
  j.max_corr2 = r * r;
  j.cap2 = search_cap2(c->params);
  j.nblocks = nblocks;
  j.fixed_iterations = c->params.fixed_iterations;
  j.max_iterations = c->params.fixed_iterations > 0 ? c->params.fixed_iterations : c->params.max_iterations;
  j.optimizer = c->params.optimizer;
  j.lm_max_iterations = c->params.lm_max_iterations;
  j.lm_init_lambda_factor = c->params.lm_init_lambda_factor;
  j.transformation_epsilon = c->params.transformation_epsilon;
  j.rotation_epsilon = c->params.rotation_epsilon;
  j.own_axis = c->own_axis;
  j.own_lo = c->own_lo;
  j.own_hi = c->own_hi;
  j.own_mod = c->own_mod;
  j.own_rem = c->own_rem;
  j.split_extent = kn.split_extent;
  j.premom = c->comm ? 1 : 0;
  j.mom = c->mom.as<double>();
  {
    const SearchLayout sl(c->src.cloud->n);
    char* u = c->search.as<char>();
    j.qstate = reinterpret_cast<float4*>(u + sl.qstate);
    j.key = reinterpret_cast<unsigned long long*>(u + sl.key);
    j.task_ctr = reinterpret_cast<unsigned*>(u + sl.ctr);
    j.tasks = reinterpret_cast<unsigned long long*>(u + sl.tasks);
    j.task_cap_r = sl.cap_r;
    j.ref = reinterpret_cast<float4*>(u + sl.ref);
    j.ref_p = reinterpret_cast<float4*>(u + sl.ref_p);
    j.sec = reinterpret_cast<unsigned*>(u + sl.sec);
    j.key2 = reinterpret_cast<unsigned long long*>(u + sl.key2);
  }
  j.xcd_scan = kn.xcd_scan;
  j.pf_ratio = kn.pf_ratio;
  j.prev_window = kn.prev_window;
  j.tri_mv = kn.tri_mv;
  j.probe2 = kn.probe * kn.probe;
  j.probe_d = kn.probe_d;
  j.reuse = kn.reuse;
  j.reuse_gap = kn.reuse_gap;
  j.reuse_gap0 = kn.reuse_gap0;
  j.cap2_d = (double)j.cap2;
  j.tri_mv_d = (double)j.tri_mv;
  j.reuse_gap_d = (double)j.reuse_gap;
  j.reuse_gap0_d = (double)j.reuse_gap0;
  j.reuse_rec0 = kn.reuse_rec0;
  j.reuse_rec_eps = kn.reuse_rec_eps;
  j.reuse_rec_conv = kn.reuse_rec_conv;
  // exact correspondence ties in nanoflann's order (k_moments): the task
  // search tracks the examined points' second distance; the target's tree,
  // when it exists, re-runs the tied queries.  Slab shards hold a subset of
  // the target, whose tree orders ties differently: Morton order there.
  j.tie_detect = (c->tie_exact && (c->own_axis < 0 || c->tie_tree)) ? 1 : 0;
  j.tgt_nf = NfTreeDev{nullptr, nullptr, nullptr, 0};
  j.tgt_nf_status = nullptr;
  j.tie_scan = j.tie_detect ? kn.tie_scan : 0;
  j.tie_ab = kn.tie_ab;
  if (j.tie_detect) {
    const NfTreeData* tt = c->tie_tree ? c->tie_tree.get() : c->tgt.cloud->nf.get();
    if (tt) {
      j.tgt_nf = tt->dev();
      j.tgt_nf_status = tt->status.as<int>();
    }
  }
  // the target's candidate cells answer the search first (k_cell_lookup)
  j.grid_on = grid_active(c) ? 1 : 0;
  if (j.grid_on) {
    j.task_cap_r = 0;   // the walk's few sub-groups scan their leaves inline (no k_nn_scan launch)
    j.grid = c->tgt.cloud->grid->dev;
    const FbLayout fl(c->src.cloud->n);
    char* u = c->fb.as<char>();
    j.fb_count = reinterpret_cast<unsigned*>(u + fl.ctr);
    j.fb_list = reinterpret_cast<int*>(u + fl.list);
    j.fb_seg_cap = fl.seg_cap;
    j.fb_mask = reinterpret_cast<unsigned short*>(u + fl.mask);
  }
  // no copy here: k_align_init reads the pinned job and writes the device one
  return GICP_OK;
}

namespace {

LinGeom geometry(const gicp_ctx* c) {
  LinGeom g = linearize_geometry(c->src.cloud->n, c->tgt.cloud->upper_count());
  g.state = c->state_dev.as<AlignState>();
  g.grid = grid_active(c);
  g.grid_walk = !g.grid || c->tgt.cloud->grid->dev.has_fallback != 0;
  // the LM step in the moment kernel's last block: a sharded align all-reduces
  // between the two, so never there; on by default for the one-kernel lookup
  // linearize (DDLO_FUSE_LM: development A/B for every path)
  g.fuse_lm = !c->comm && lm_fusion_enabled(g.grid && !g.grid_walk);
  return g;
}

}  // namespace

gicp_status ddlo::rt::prepare_align(gicp_ctx* c) {
  if (!c->src.cloud) return fail(GICP_ENOSOURCE, "no source cloud");
  if (!c->tgt.cloud) return fail(GICP_ENOTARGET, "no target cloud");
  // NanoGICP::computeTransformation (:186-193): compute missing covariances
  if (!c->src.has_cov()) {
    gicp_status s = compute_cov(c, c->src);
    if (s) return s;
  }
  if (!c->tgt.has_cov()) {
    gicp_status s = compute_cov(c, c->tgt);
    if (s) return s;
  }
  const int ns = c->src.cloud->n;
  // a growing buffer goes back to the pool: the queued no-op chunk of the
  // previous align must not still reference it
  const size_t need_corr = sizeof(int) * ns, need_sqd = sizeof(float) * ns,
               need_slab = sizeof(double) * kSlabStride * linearize_blocks(ns),
               need_search = SearchLayout(ns).total, need_fb = grid_active(c) ? FbLayout(ns).total : 0;
  if (need_corr > c->corr.bytes || need_sqd > c->sqd.bytes || need_slab > c->slab.bytes ||
      need_search > c->search.bytes || need_fb > c->fb.bytes ||
      (c->stats_on && sizeof(unsigned int) * kStatFields * (ns + 15) > c->stats.bytes)) {
    gicp_status s = drain_tail(c);
    if (s) return s;
  }
  HIP_TRY(c->corr.ensure(sizeof(int) * ns));
  HIP_TRY(c->sqd.ensure(sizeof(float) * ns));
  HIP_TRY(c->slab.ensure(sizeof(double) * kSlabStride * linearize_blocks(ns)));
  HIP_TRY(c->mom.ensure(sizeof(double) * kSlabStride));
  HIP_TRY(c->search.ensure(need_search));
  if (need_fb) HIP_TRY(c->fb.ensure(need_fb));
  // the target's nanoflann tree (tie order): a sharded align builds it up
  // front (every rank the same tree, so no rank ever re-runs alone and the
  // collectives stay matched); otherwise it is built only when an align
  // meets a tie (gicp_align).  The stream waits once for a tree's build.
  if (c->tie_exact && (c->own_axis < 0 || c->tie_tree)) {
    CloudData& tc = *c->tgt.cloud;
    if (c->comm && !c->tie_tree && !tc.nf) {
      gicp_status s = ensure_nftree(c, tc, c->stream);
      if (s) return s;
    }
    const auto& nf = c->tie_tree ? c->tie_tree : tc.nf;
    if (nf && c->nf_joined.lock() != nf) {
      HIP_TRY(nftree_join(*nf, c->stream));
      c->nf_joined = nf;
    }
  }
  if (c->stats_on) {
    HIP_TRY(c->stats.ensure(sizeof(unsigned int) * kStatFields * (ns + 15)));
    HIP_TRY(hipMemsetAsync(c->stats.p, 0, c->stats.bytes, c->stream));
  }
  return GICP_OK;
}

// Build the target's nanoflann tree (the tie order of the correspondences)
// and make the ctx stream wait for it.
gicp_status ddlo::rt::ensure_tie_tree(gicp_ctx* c) {
  gicp_status s = drain_tail(c);
  if (s) return s;
  s = ensure_nftree(c, *c->tgt.cloud, c->stream);
  if (s) return s;
  HIP_TRY(nftree_join(*c->tgt.cloud->nf, c->stream));
  c->nf_joined = c->tgt.cloud->nf;
  return GICP_OK;
}

// One outer iteration: linearize (search + moments), then — on a sharded ctx —
// this rank's reduced moments all-reduced across ranks (80 doubles over
// RCCL: H, b, cost and the LM trial-cost moments in one collective), then
// the LM/GN step, replicated bit-identically on every rank.
// publish: host-mapped state slot the LM step copies the new state to (the
// last iteration of a chunk), or nullptr.
gicp_status ddlo::rt::enqueue_iteration(gicp_ctx* c, const AlignJob* jd, int nblocks, AlignState* publish) {
  (void)nblocks;   // = geometry(c).mom_blocks (fill_job)
  const LinGeom g = geometry(c);
  launch_linearize(c->stream, jd, g, publish);   // (fused LM step: the moment kernel's last block publishes)
  if (c->comm) {
    launch_mom_reduce(c->stream, jd);
    NCCL_TRY(rccl().all_reduce(c->mom.p, c->mom.p, kSlabStride, ncclFloat64, ncclSum, c->comm, c->stream));
  }
  if (!g.fuse_lm)
    launch_lm_step(c->stream, jd, c->state_dev.as<AlignState>(), c->slab.as<double>(), g.mom_blocks,
                   c->comm ? c->mom.as<double>() : nullptr, publish);
  return GICP_OK;
}

namespace {

gicp_status enqueue_chunk(gicp_ctx* c, bool with_init, int iters, int nblocks, int slot) {
  AlignJob* jd = c->job_dev.as<AlignJob>();
  if (with_init) launch_align_init(c->stream, jd, c->job_host_dev);
  // the chunk's last LM step publishes the whole state to pinned host
  // memory: the host polls {iter, done} from it, and once done it already
  // holds the final pose, so no read-back round trip (and no copy kernel)
  // follows convergence (a speculative no-op chunk behind it rewrites the
  // same bytes)
  for (int i = 0; i < iters; ++i) {
    gicp_status s = enqueue_iteration(c, jd, nblocks, i == iters - 1 ? c->state_host_dev + slot : nullptr);
    if (s) return s;
  }
  return GICP_OK;
}

gicp_status capture_chunk(gicp_ctx* c, bool with_init, int iters, int nblocks, int slot, hipExecGraphPair* out) {
  ++c->captures;
  HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  const gicp_status s = enqueue_chunk(c, with_init, iters, nblocks, slot);
  const hipError_t e = hipStreamEndCapture(c->stream, &out->g);  // always leave capture mode
  if (s) return s;
  HIP_TRY(e);
  HIP_TRY(hipGraphInstantiate(&out->ge, out->g, nullptr, nullptr, 0));
  return GICP_OK;
}

void drop_pair(hipExecGraphPair& p) {
  if (p.ge) (void)hipGraphExecDestroy(p.ge);
  if (p.g) (void)hipGraphDestroy(p.g);
  p.ge = nullptr;
  p.g = nullptr;
}

void drop_set(GraphSet& gs) {
  for (auto& p : gs.first) drop_pair(p);
  gs.first.clear();
  drop_pair(gs.rest[0]);
  drop_pair(gs.rest[1]);
  gs.key.fill(-1);
}

}  // namespace

void ddlo::rt::drop_graphs(gicp_ctx* c) {
  for (auto& gs : c->gsets) drop_set(gs);
  c->gsets.clear();
}

namespace {

// The graph set of a launch geometry: a cached one, else captured (its two
// single-iteration graphs now, first chunks on demand), evicting the least
// recently used set -- after the stream's queued chunk, which may be one of
// its graphs, has run.
gicp_status graph_set(gicp_ctx* c, const std::array<long long, 7>& key, int nblocks, GraphSet** out);

// DDLO_FRESH_START=0 (dev builds): every align starts with k_align_init (A/B).
bool fresh_start_enabled() {
  static const bool on = [] {
    const char* v = dev_getenv("DDLO_FRESH_START");
    return !(v && *v == '0');
  }();
  return on;
}

// An align may start without k_align_init when the device job and state are
// provably what the init kernel would find and leave but for the words
// k_moments_fresh writes itself:
//   - the job is the device's copy but for the guess and the ticket
//     (finalize_job left job_full = 0), so the state's src_radius holds too;
//   - the linearize is the fused one-kernel lookup with the LM step in its
//     last block, unsharded, with no profiling and no per-wave statistics;
//   - at least one iteration runs;
//   - prev_ok: the ctx's last align completed on the graph path without an
//     error -- the state is a completed align's, the arrival word is re-armed
//     -- and published tie words that were all 0 (no kernel can zero them at
//     the start of a launch whose blocks add to them).
bool fresh_start_allowed(const gicp_ctx* c, bool prev_ok, int max_it) {
  if (!prev_ok || !fresh_start_enabled() || c->job_host->job_full != 0 || max_it <= 0) return false;
  if (c->comm || c->profiling || c->stats_on) return false;
  const LinGeom g = geometry(c);
  return linearize_is_one_kernel(g) && g.fuse_lm;
}

// Launch the align as a first chunk of n outer iterations (n = the previous
// align's iteration count on this ctx: aligns of consecutive scans converge
// in similar counts) followed by single-iteration chunks, keeping one
// speculative single-iteration chunk queued ahead while the host checks the
// previous chunk's done flag (from the first chunk on only when the previous
// align needed more than its first chunk).  After convergence at most that
// one no-op iteration (three early-exiting kernels) runs.  Returns the index
// of the chunk after which the state is final.
// fresh (fresh_start_allowed): the first chunk starts without k_align_init
// and is not a graph.  Its first iteration is k_moments_fresh -- the guess,
// the ticket and rec0 are its arguments, which the runtime pushes with the
// dispatch -- and its other first - 1 iterations are launched one by one
// behind it while it runs.  Of the three ways to deliver the arguments that
// was the fastest (profiles/fresh_start_summary.md: a graph of the other
// iterations behind the kernel, and one graph whose first node's arguments
// are updated per launch, both cost a graph launch the plain launches do
// not).  The chunk publishes to slot 0 as the graph it stands for, so slots,
// events, speculation and the prediction are unchanged.
gicp_status run_align_graph(gicp_ctx* c, int max_it, int nblocks, bool fresh, int* final_chunk) {
  const void* jd = c->job_dev.p;
  // key: whether RCCL is in the chunk, the job buffer and the launch geometry
  const LinGeom g = geometry(c);
  (void)nblocks;   // = g.mom_blocks
  // (the slab buffer: k_lm_step takes it as an argument; pool blocks are 256-B aligned, bit 0 = RCCL)
  const std::array<long long, 7> key{{(long long)(uintptr_t)c->slab.p | (c->comm ? 1 : 0), (long long)(uintptr_t)jd,
                                      g.seed_blocks, g.scan_blocks, g.mom_blocks, g.lds_boxes,
                                      g.grid ? (g.grid_walk ? 2L : 1L) * g.lookup_blocks : 0}};
  const bool use_graph = !c->comm || c->comm_graphs;
  const int first = c->params.fixed_iterations > 0
                        ? std::max(1, std::min(max_it, kMaxFixedChunk))
                        : std::max(1, std::min({c->predicted_iters, max_it, kMaxFirstChunk}));
  GraphSet* gs = nullptr;
  if (use_graph) {
    gicp_status s = graph_set(c, key, nblocks, &gs);
    if (s) {
      drop_graphs(c);
      (void)hipGetLastError();
      if (!c->comm) return s;
      c->comm_graphs = false;  // RCCL refused stream capture: launch chunks eagerly
      return run_align_graph(c, max_it, nblocks, fresh, final_chunk);
    }
  }
  if (use_graph && !fresh && !gs->first[first - 1].ge) {
    gicp_status s = capture_chunk(c, true, first, nblocks, 0, &gs->first[first - 1]);
    if (s) {
      drop_graphs(c);
      return s;
    }
  }
  // chunk k publishes to slot k % 2 (chunk 0: the first-chunk graph, slot 0)
  auto launch_chunk = [&](int k) -> gicp_status {
    const bool is_first = k == 0;
    if (is_first && fresh) {
      const AlignJob& jh = *c->job_host;
      FreshStart fs{};
      std::memcpy(fs.R, jh.guess_R, sizeof(fs.R));
      std::memcpy(fs.t, jh.guess_t, sizeof(fs.t));
      fs.ticket = jh.ticket;
      fs.job_w = c->job_dev.as<AlignJob>();
      fs.rec0 = jh.reuse && jh.reuse_rec0;
      launch_linearize_fresh(c->stream, c->job_dev.as<AlignJob>(), g, fs, first == 1 ? c->state_host_dev : nullptr);
      HIP_TRY(hipGetLastError());
      return first > 1 ? enqueue_chunk(c, false, first - 1, nblocks, 0) : GICP_OK;
    }
    if (use_graph) {
      HIP_TRY(hipGraphLaunch(is_first ? gs->first[first - 1].ge : gs->rest[k & 1].ge, c->stream));
      return GICP_OK;
    }
    return enqueue_chunk(c, is_first, is_first ? first : 1, nblocks, k & 1);
  };
  const int nchunks = 1 + (max_it - first);
  while ((int)c->chunk_ev.size() < nchunks) {
    hipEvent_t e;
    // (untimed: only profiled aligns take a device time, from events of their own)
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->chunk_ev.push_back(e);
  }
  gicp_status s = launch_chunk(0);
  if (s) return s;
  HIP_TRY(hipEventRecord(c->chunk_ev[0], c->stream));
  int launched = 1;
  if (nchunks > 1 && c->speculate) {
    s = launch_chunk(1);
    if (s) return s;
    HIP_TRY(hipEventRecord(c->chunk_ev[1], c->stream));
    launched = 2;
  }
  // The number of chunks launched depends only on the done flags, which the
  // replicated LM step makes identical on every rank of a sharded align, so
  // every rank issues the same sequence of collectives.  When chunk k is
  // read, at most chunk k + 1 (the other slot) is queued behind it; chunk
  // k + 2 (same slot as k) is launched only after the read.
  int k = 0;
  // the host polls the chunk's event (hipEventQuery) instead of blocking in
  // hipEventSynchronize: 2 us less per align at cfg 3 (DDLO_SPIN_WAIT=0: block)
  static const bool spin = [] {
    const char* v = dev_getenv("DDLO_SPIN_WAIT");
    return !(v && *v == '0');
  }();
  const unsigned long long ticket = c->job_host->ticket;
  for (;;) {
    if (spin) {
      // chunk k's last LM step writes its publication word (ticket, done,
      // iter) after the state (AlignState::pub): the host polls that word in
      // pinned memory, which lands as the kernel stores it, instead of the
      // chunk's event, which completes only after the command processor has
      // retired the kernel.  The event is still queried every 64 polls (an
      // error, or a word that never comes, ends the wait).
      static std::atomic<int> waiters{0};
      waiters.fetch_add(1, std::memory_order_relaxed);
      const volatile unsigned long long* pw = &(c->state_host + (k & 1))->pub;
      const int expect = first + k;   // iterations after chunk k unless done earlier
      hipError_t q = hipErrorNotReady;
      for (unsigned n = 1;; ++n) {
        const unsigned long long w = *pw;
        if ((w >> 17) == ticket && (((w >> 16) & 1ull) || (int)(w & 0xffffu) >= expect)) {
          q = hipSuccess;
          break;
        }
        if ((n & 63) == 0) {
          q = hipEventQuery(c->chunk_ev[k]);
          if (q != hipErrorNotReady) {
            const unsigned long long w2 = *pw;   // the event completed: the word has landed
            if (q == hipSuccess && !((w2 >> 17) == ticket && (((w2 >> 16) & 1ull) || (int)(w2 & 0xffffu) >= expect)))
              q = hipErrorUnknown;
            break;
          }
        }
        if (waiters.load(std::memory_order_relaxed) > 1) std::this_thread::yield();
      }
      waiters.fetch_sub(1, std::memory_order_relaxed);
      if (q == hipErrorUnknown) return fail(GICP_EHIP, "align chunk completed without its state publication");
      HIP_TRY(q);
    } else {
      HIP_TRY(hipEventSynchronize(c->chunk_ev[k]));
    }
    const volatile AlignState* st = c->state_host + (k & 1);
    if (st->done || k == nchunks - 1) break;
    while (launched < nchunks && launched <= k + 2) {  // keep one chunk queued ahead of k+1
      s = launch_chunk(launched);
      if (s) return s;
      HIP_TRY(hipEventRecord(c->chunk_ev[launched], c->stream));
      ++launched;
    }
    ++k;
  }
  *final_chunk = k;
  c->state_slot = k & 1;
  c->tail_ev = c->chunk_ev[launched - 1];
  // (a published chunk may still be retiring its last kernel: the tail covers it too)
  c->tail_pending = launched - 1 > k || spin;
  // Speculate next time only if this align outran its predicted first chunk:
  // when the prediction held, the queued no-op chunk only delays the next
  // align (A/B at cfg 3: 0.466 -> 0.459 ms/scan without it).
  c->speculate = k > 0;
  c->predicted_iters = std::max(1, (int)((const volatile AlignState*)(c->state_host + (k & 1)))->iter);
  return GICP_OK;
}

gicp_status graph_set(gicp_ctx* c, const std::array<long long, 7>& key, int nblocks, GraphSet** out) {
  ++c->graph_clock;
  for (auto& gs : c->gsets)
    if (gs.key == key) {
      gs.last_use = c->graph_clock;
      *out = &gs;
      return GICP_OK;
    }
  GraphSet* slot = nullptr;
  if ((int)c->gsets.size() < kGraphSets) {
    c->gsets.reserve(kGraphSets);   // no reallocation: the sets stay where their pointers point
    c->gsets.emplace_back();
    slot = &c->gsets.back();
  } else {
    slot = &c->gsets[0];
    for (auto& gs : c->gsets)
      if (gs.last_use < slot->last_use) slot = &gs;
    gicp_status s = drain_tail(c);   // the queued speculative chunk may be one of its graphs
    if (s) return s;
    drop_set(*slot);
  }
  slot->first.resize(kMaxFixedChunk);
  gicp_status s = capture_chunk(c, false, 1, nblocks, 0, &slot->rest[0]);
  if (!s) s = capture_chunk(c, false, 1, nblocks, 1, &slot->rest[1]);
  if (s) return s;
  slot->key = key;
  slot->last_use = c->graph_clock;
  *out = slot;
  return GICP_OK;
}

gicp_status run_align_eager_profiled(gicp_ctx* c, int max_it, int nblocks) {
  AlignJob* jd = c->job_dev.as<AlignJob>();
  const size_t need = 2 * (size_t)max_it;
  while (c->prof_ev.size() < need) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    c->prof_ev.push_back(e);
  }
  launch_align_init(c->stream, jd, c->job_host_dev);
  for (int i = 0; i < max_it; ++i) {
    HIP_TRY(hipEventRecord(c->prof_ev[2 * i], c->stream));
    LinGeom g = geometry(c);
    g.fuse_lm = false;   // profiled aligns time the linearize on its own
    launch_linearize(c->stream, jd, g);
    HIP_TRY(hipEventRecord(c->prof_ev[2 * i + 1], c->stream));
    if (c->comm) {
      launch_mom_reduce(c->stream, jd);
      NCCL_TRY(rccl().all_reduce(c->mom.p, c->mom.p, kSlabStride, ncclFloat64, ncclSum, c->comm, c->stream));
    }
    launch_lm_step(c->stream, jd, c->state_dev.as<AlignState>(), c->slab.as<double>(), g.mom_blocks,
                   c->comm ? c->mom.as<double>() : nullptr, nullptr);
  }
  HIP_TRY(hipGetLastError());
  return GICP_OK;
}

}  // namespace

namespace ddlo {
bool lm_fusion_enabled(bool lookup) {
  static const int on = [] {   // -1: the default (fused on the lookup path only)
    const char* v = dev_getenv("DDLO_FUSE_LM");
    return v && *v ? std::atoi(v) : -1;
  }();
  return on < 0 ? lookup : on != 0;
}
}  // namespace ddlo

extern "C" {

gicp_status gicp_align(gicp_ctx* c, const float* guess16, float* out16, gicp_result* res) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  // (cleared while the align is under way: an error return leaves it cleared)
  bool prev_ok = c->fresh_ok;
  c->fresh_ok = false;
  c->dbg_search = false;
  bool graph_path = false;
  begin_ties(c);
  gicp_status s = set_device(c);
  if (s) return s;
  s = maybe_build_grid(c);
  if (s) return s;
  s = prepare_align(c);
  if (s) return s;
  const int ns = c->src.cloud->n;
  const int nblocks = linearize_blocks(ns);
  hipEvent_t end_ev = c->ev1;
  int reruns = 0;
  for (;;) {
    s = fill_job(c, guess16, nblocks);
    if (s) return s;
    finalize_job(c);
    JobCommit commit(c);
    const int max_it = c->job_host->max_iterations;
    const bool fresh = fresh_start_allowed(c, prev_ok, max_it);
    prev_ok = false;   // (a tie re-run changes the job: k_align_init)
    ++(fresh ? c->fresh_aligns : c->init_aligns);
    end_ev = c->ev1;
    if (c->profiling) HIP_TRY(hipEventRecord(c->ev0, c->stream));   // (read only by the profiled path below)
    if (c->profiling || max_it <= 0) {
      s = max_it > 0 ? run_align_eager_profiled(c, max_it, nblocks) : GICP_OK;
      if (s) return s;
      if (max_it <= 0) launch_align_init(c->stream, c->job_dev.as<AlignJob>(), c->job_host_dev);
      HIP_TRY(hipGetLastError());
      commit.done();
      HIP_TRY(hipEventRecord(c->ev1, c->stream));
      HIP_TRY(hipMemcpyAsync(c->state_host, c->state_dev.p, sizeof(AlignState), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      c->state_slot = 0;
      c->tail_pending = false;
      graph_path = false;
    } else {
      int fc = 0;
      s = run_align_graph(c, max_it, nblocks, fresh, &fc);
      if (s) return s;
      commit.done();
      graph_path = true;
      // chunk fc's end-of-chunk copy already put the final state in its
      // slot; the (at most one) speculative no-op chunk still queued writes
      // the other slot and does not delay the return
      end_ev = c->chunk_ev[fc];
    }
    // a correspondence met an exact tie before the target had nanoflann's
    // tree: build it and run the align again, so every correspondence is
    // nanoflann's (the tree stays with the target cloud for later aligns)
    if (!final_state(c).tie_pending || reruns > 0) break;
    s = ensure_tie_tree(c);
    if (s) return s;
    ++reruns;
  }
  const AlignState& st = final_state(c);
  c->have_align = st.iter > 0;
  c->last_nsrc = ns;
  if (out16) {
    for (int r = 0; r < 3; ++r) {
      for (int cc = 0; cc < 3; ++cc) out16[4 * r + cc] = (float)st.R[3 * r + cc];
      out16[4 * r + 3] = (float)st.t[r];
    }
    out16[12] = out16[13] = out16[14] = 0.f;
    out16[15] = 1.f;
  }
  if (res) {
    std::memset(res, 0, sizeof(*res));
    res->converged = st.converged;
    res->nr_iterations = st.nr_iterations;
    res->iterations_run = st.iter;
    res->lm_failed = st.lm_failed;
    res->lm_trials = st.lm_trials;
    res->num_correspondences = st.num_corr;
    res->final_cost = st.final_cost;
    std::memcpy(res->final_hessian, st.final_hessian, sizeof(res->final_hessian));
    res->lm_lambda = st.lambda;
    res->ties_resolved = st.ties_resolved;
    res->tie_reruns = reruns;
    if (c->profiling) {
      // (profiled aligns only: a graph align returns as soon as its state is
      // published, before its end event has completed)
      float ms = 0.f;
      HIP_TRY(hipEventSynchronize(end_ev));
      HIP_TRY(hipEventElapsedTime(&ms, c->ev0, end_ev));
      res->device_ms = ms;
      double tot = 0.0;
      for (int i = 0; i < st.iter; ++i) {
        float m = 0.f;
        HIP_TRY(hipEventElapsedTime(&m, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
        tot += m;
      }
      res->linearize_ms = tot;
    }
  }
  s = check_ties(c);
  if (s) return s;
  if (st.tie_err || st.tie_pending)
    return fail(GICP_EHIP, "nanoflann tie order: a tied correspondence could not be re-run (bits " +
                               std::to_string(st.tie_err) + (st.tie_pending ? ", no tree" : "") + ")");
  if (st.lm_failed) g_last_error = "lm not converged!!";
  // the next align may start without k_align_init (fresh_start_allowed): the state this one
  // published holds every tie the align met, and a queued no-op chunk adds none
  c->fresh_ok = graph_path && !st.tie_pending && !st.ties_resolved && !st.tie_err;
  return GICP_OK;
}

gicp_status gicp_linearize(gicp_ctx* c, const double* pose16, double* H36, double* b6, double* cost, int32_t* ncorr) {
  if (!c || !pose16) return fail(GICP_EINVAL, "null argument");
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
  const int nblocks = linearize_blocks(ns);
  for (int rerun = 0;; ++rerun) {
    float g[16];
    for (int i = 0; i < 16; ++i) g[i] = 0.f;
    s = fill_job(c, g, nblocks);
    if (s) return s;
    // exact double pose (not the float guess path)
    for (int r = 0; r < 3; ++r) {
      for (int cc = 0; cc < 3; ++cc) c->job_host->guess_R[3 * r + cc] = pose16[4 * r + cc];
      c->job_host->guess_t[r] = pose16[4 * r + 3];
    }
    c->job_host->optimizer = GICP_OPT_GAUSS_NEWTON;
    c->job_host->max_iterations = 1;
    c->job_host->fixed_iterations = 1;
    finalize_job(c);
    JobCommit commit(c);
    AlignJob* jd = c->job_dev.as<AlignJob>();
    launch_align_init(c->stream, jd, c->job_host_dev);
    s = enqueue_iteration(c, jd, nblocks, nullptr);
    if (s) return s;
    HIP_TRY(hipGetLastError());
    commit.done();
    HIP_TRY(hipMemcpyAsync(c->state_host, c->state_dev.p, sizeof(AlignState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->state_slot = 0;
    c->tail_pending = false;
    if (!final_state(c).tie_pending || rerun > 0) break;
    s = ensure_tie_tree(c);   // a tie met before the target had its nanoflann tree (see gicp_align)
    if (s) return s;
  }
  const AlignState& st = final_state(c);
  if (st.tie_err || st.tie_pending)
    return fail(GICP_EHIP, "nanoflann tie order: a tied correspondence could not be re-run (bits " +
                               std::to_string(st.tie_err) + ")");
  if (H36) std::memcpy(H36, st.final_hessian, sizeof(double) * 36);
  if (cost) *cost = st.final_cost;
  if (ncorr) *ncorr = st.num_corr;
  if (b6) std::memcpy(b6, st.last_b, sizeof(double) * 6);
  c->have_align = true;
  c->last_nsrc = ns;
  return GICP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Frame-parallel S2S batch (ddlo_gicp.h): nstreams chained chunks, one ctx,
// HIP stream and host thread each.
gicp_status gicp_s2s_batch(int device, const gicp_params* p, const float* const* clouds, const size_t* sizes,
                           size_t stride_bytes, int nframes, int nstreams, float* out16, gicp_result* res) {
  if (!p || !clouds || !sizes || !out16 || nframes < 1 || nstreams < 1)
    return fail(GICP_EINVAL, "invalid batch arguments");
  for (int t = 0; t < nframes; ++t)
    if (!clouds[t] || sizes[t] == 0) return fail(GICP_EINVAL, "null or empty frame");
  for (int e = 0; e < 16; ++e) out16[e] = (e % 5 == 0) ? 1.f : 0.f;
  if (res) std::memset(&res[0], 0, sizeof(gicp_result));
  const int npairs = nframes - 1;
  if (npairs == 0) return GICP_OK;
  const int nthreads = std::min(nstreams, npairs);
  std::vector<gicp_status> status(nthreads, GICP_OK);
  std::vector<std::string> errors(nthreads);
  // contexts are made (and destroyed) on this thread, outside any worker's
  // graph capture
  std::vector<gicp_ctx*> ctxs(nthreads, nullptr);
  for (int w = 0; w < nthreads; ++w) {
    gicp_status s = gicp_ctx_create(device, &ctxs[w]);
    if (!s) s = gicp_set_params(ctxs[w], p);
    if (!s) {
      const char* os = dev_getenv("DDLO_NF_OWN_STREAM");   // 0: the second stream (A/B)
      ctxs[w]->nf_same_stream = !(os && *os == '0');
    }
    if (s) {
      const std::string why = g_last_error;
      for (auto* c : ctxs)
        if (c) (void)gicp_ctx_destroy(c);
      return fail(s, why);
    }
  }
  auto worker = [&](int w) {
    // pairs (t-1, t) for t in [t0, t1)
    const int t0 = 1 + (int)((long)npairs * w / nthreads);
    const int t1 = 1 + (int)((long)npairs * (w + 1) / nthreads);
    gicp_ctx* c = ctxs[w];
    gicp_status s = gicp_set_target(c, clouds[t0 - 1], sizes[t0 - 1], stride_bytes);
    for (int t = t0; t < t1 && !s; ++t) {
      s = set_source_impl(c, clouds[t], sizes[t], stride_bytes, 1, true);
      if (!s) s = gicp_align(c, nullptr, out16 + 16 * (size_t)t, res ? &res[t] : nullptr);
      if (!s) s = gicp_swap_source_target(c);  // scan t becomes the next target (odom.cc:768)
    }
    if (s) {
      status[w] = s;
      errors[w] = g_last_error;
    }
  };
  std::vector<std::thread> pool;
  for (int w = 1; w < nthreads; ++w) pool.emplace_back(worker, w);
  worker(0);
  for (auto& th : pool) th.join();
  for (auto* c : ctxs) (void)gicp_ctx_destroy(c);
  for (int w = 0; w < nthreads; ++w)
    if (status[w]) return fail(status[w], "s2s batch chunk " + std::to_string(w) + ": " + errors[w]);
  return GICP_OK;
}
