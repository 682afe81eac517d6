// cloud.hip — the device cloud behind a Side: its Morton-sorted points and
// search hierarchy (build_cloud, K1; the radix sort is hipcub's), nanoflann's
// own tree of it for the tie order (nftree_build and the ensure_* wrappers,
// kernels in nftree.hip) and its covariances (compute_cov, K2).  Declared in
// runtime.hpp; called by the C-ABI files and the odometry driver (odom.hip).
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "runtime.hpp"

namespace ddlo {
namespace rt {

gicp_status build_cloud(gicp_ctx* c, const float* xyz, size_t n, size_t stride, std::shared_ptr<CloudData>* out,
                        bool on_device, bool check_finite, bool nf_early) {
  if (!xyz || n == 0 || stride < 12 || (stride % 4) != 0) return fail(GICP_EINVAL, "invalid cloud (null, empty or bad stride)");
  if (n > (size_t)INT32_MAX / 2) return fail(GICP_EINVAL, "cloud too large");
  auto cd = std::make_shared<CloudData>();
  // nf_early starts nanoflann's tree of cd on the aux stream; if this call
  // then fails (non-finite input, a HIP error), cd and its buffers go back
  // to the device pool: wait for the build first, so that no other ctx gets
  // a block the aux stream still writes (DevicePool: idle when released)
  struct AuxDrain {
    gicp_ctx* c;
    bool armed = false;
    ~AuxDrain() {
      if (armed) (void)hipStreamSynchronize(c->aux_stream);
    }
  } drain{c};
  const int N = (int)n;
  cd->n = N;
  cd->nlevels = levels_for(N, cd->lvl_cnt, cd->lvl_off);
  if (cd->nlevels < 0) return fail(GICP_EINVAL, "cloud too large for the search hierarchy");
  if (cd->upper_count() > 2048)  // LDS cache of levels >= 1 (64 KB): <= 4.2M points
    return fail(GICP_EINVAL, "cloud too large for the search hierarchy's LDS cache (max ~4.2M points)");
  const int total_boxes = cd->lvl_off[cd->nlevels - 1] + cd->lvl_cnt[cd->nlevels - 1];
  hipStream_t s = c->stream;
  const size_t raw_sz = (n - 1) * stride + 12;
  const unsigned char* raw = reinterpret_cast<const unsigned char*>(xyz);
  if (!on_device) {
    HIP_TRY(grow(c->raw_bytes, raw_sz, s));
    HIP_TRY(hipMemcpyAsync(c->raw_bytes.p, xyz, raw_sz, hipMemcpyHostToDevice, s));
    raw = c->raw_bytes.as<unsigned char>();
  }
  const int nb = (N + 255) / 256;
  HIP_TRY(grow(c->raw_pts, sizeof(float4) * n, s));
  HIP_TRY(grow(c->partial, sizeof(float) * 6 * nb, s));
  HIP_TRY(grow(c->nonfinite, sizeof(int), s));
  if (check_finite) HIP_TRY(hipMemsetAsync(c->nonfinite.p, 0, sizeof(int), s));   // (else never read)
  HIP_TRY(cd->quant.ensure(sizeof(float) * 8));
  launch_pack_bbox(s, raw, stride, N, c->raw_pts.as<float4>(), c->partial.as<float>(),
                   c->nonfinite.as<int>(), nb);
  launch_bbox_final(s, c->partial.as<float>(), nb, cd->quant.as<float>());
  HIP_TRY(grow(c->keys_tmp, sizeof(unsigned long long) * n, s));
  HIP_TRY(grow(c->vals_tmp, sizeof(int) * n, s));
  HIP_TRY(cd->keys.ensure(sizeof(unsigned long long) * n));
  HIP_TRY(cd->perm.ensure(sizeof(int) * n));
  launch_morton(s, c->raw_pts.as<float4>(), N, cd->quant.as<float>(), c->keys_tmp.as<unsigned long long>(),
                c->vals_tmp.as<int>());
  size_t tmp_bytes = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, c->keys_tmp.as<unsigned long long>(),
                                             cd->keys.as<unsigned long long>(), c->vals_tmp.as<int>(),
                                             cd->perm.as<int>(), N, 0, 63, s));
  HIP_TRY(grow(c->sort_tmp, tmp_bytes, s));
  tmp_bytes = c->sort_tmp.bytes;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(c->sort_tmp.p, tmp_bytes, c->keys_tmp.as<unsigned long long>(),
                                             cd->keys.as<unsigned long long>(), c->vals_tmp.as<int>(),
                                             cd->perm.as<int>(), N, 0, 63, s));
  const int npad = cd->lvl_cnt[0] * kLeafSize;  // whole leaves, sentinel-padded
  HIP_TRY(cd->pts.ensure(sizeof(float4) * npad));
  HIP_TRY(cd->inv_perm.ensure(sizeof(int) * n));
  launch_gather(s, c->raw_pts.as<float4>(), cd->perm.as<int>(), N, npad, cd->pts.as<float4>(), cd->inv_perm.as<int>());
  // (a ctx building its trees on its own stream gates the partial tree on the
  // covariance pass's tie count instead: compute_cov)
  if (nf_early && c->tie_exact && !(c->nf_same_stream && c->tie_lazy && !c->lazy_heavy)) {
    drain.armed = true;
    gicp_status st = (c->tie_lazy && !c->lazy_heavy) ? ensure_nftree_partial(c, *cd, s) : ensure_nftree(c, *cd, s);
    if (st) return st;
  }
  HIP_TRY(cd->dir.ensure(sizeof(int) * (size_t)fine_dir_ints(N)));
  launch_key_dir(s, cd->keys.as<unsigned long long>(), N, cd->dir.as<int>());
  HIP_TRY(cd->soa.ensure(sizeof(float) * 3 * (size_t)npad));
  HIP_TRY(cd->box_lo.ensure(sizeof(float4) * total_boxes));
  HIP_TRY(cd->box_hi.ensure(sizeof(float4) * total_boxes));
  launch_leaf_soa_boxes(s, cd->pts.as<float4>(), N, cd->lvl_cnt[0], cd->soa.as<float>(), cd->box_lo.as<float4>(),
                        cd->box_hi.as<float4>());
  for (int l = 1; l < cd->nlevels; ++l)
    launch_level_boxes(s, cd->box_lo.as<float4>() + cd->lvl_off[l - 1], cd->box_hi.as<float4>() + cd->lvl_off[l - 1],
                       cd->lvl_cnt[l - 1], cd->lvl_cnt[l], cd->box_lo.as<float4>() + cd->lvl_off[l],
                       cd->box_hi.as<float4>() + cd->lvl_off[l]);
  HIP_TRY(hipGetLastError());
  if (check_finite) {
    HIP_TRY(hipMemcpyAsync(c->flag_host, c->nonfinite.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (*c->flag_host) return fail(GICP_ENONFINITE, "cloud contains non-finite coordinates");
  }
  *out = cd;
  drain.armed = false;   // the tree's owner (cd) lives on: its users wait on nf->ready
  return GICP_OK;
}

gicp_status nftree_build(gicp_ctx* c, CloudData& cd, hipStream_t s_in, NfTreeData& tr, int stop, long long* off,
                         int partial_levels, const int* gate, bool zero_nodes) {
  NfTreeData* t = &tr;
  const int n = cd.n;
  // the cloud is ready on s_in; the build runs on the aux stream
  static const bool same_env = dev_getenv("DDLO_NF_SAME_STREAM") != nullptr;   // A/B, diagnostics
  const bool same_stream = same_env || c->nf_same_stream;
  const hipStream_t s = same_stream ? s_in : c->aux_stream;
  if (!same_stream) {
    HIP_TRY(hipEventRecord(c->aux_ev, s_in));
    HIP_TRY(hipStreamWaitEvent(s, c->aux_ev, 0));
  }
  if (!t->ready) HIP_TRY(hipEventCreateWithFlags(&t->ready, hipEventDisableTiming));
  t->n = n;
  const bool timed = c->profiling && c->st_in_cov && c->st_ev[2] && stop < 0 && !off;
  if (timed) HIP_TRY(hipEventRecord(c->st_ev[2], s));
  // grids sized for a bucket of 16k points: one captured build graph serves
  // every cloud of the bucket (the kernels read the descriptor, and n, from
  // device memory), so a build is one graph launch, not ~80 kernel launches
  const int nbucket = (int)(((long)n + 16383) / 16384 * 16384);
  const NfSizes z = nf_sizes(nbucket);
  // the level count: the full margin for diagnostics builds, else from the
  // last completed build of this bucket on this ctx
  if (c->nf_ntask_pending_check()) {
    int used = 0;
    while (used < c->nf_ntask_lmax && c->nf_ntask_host[used] > 0) ++used;
    auto& h = c->nf_hints[c->nf_ntask_bucket];
    if (used >= c->nf_ntask_lmax) {
      h.hint = 0;   // every level had nodes to split: measure again with the full margin
    } else {
      h.used_max = std::max(h.used_max, used);
      h.hint = h.used_max + kNfLevelSpare;
    }
    c->nf_ntask_bucket = -1;
  }
  int Lmax = z.Lmax;
  const bool partial = partial_levels >= 0 && stop < 0 && !off;
  if (partial) Lmax = std::min(z.Lmax, partial_levels);
  if (stop < 0 && !off && !partial) {
    const auto it = c->nf_hints.find(nbucket);
    if (it != c->nf_hints.end() && it->second.hint > 0) Lmax = std::min(z.Lmax, it->second.hint);
  }
  t->cap = z.big_ids + 2 * n;   // big-level ids, then 2 per point for the small subtrees' ranges
  HIP_TRY(t->vpts.ensure(sizeof(float4) * (size_t)n));
  HIP_TRY(t->nodes.ensure(sizeof(NfNode) * (size_t)t->cap));
  if (zero_nodes) HIP_TRY(hipMemsetAsync(t->nodes.p, 0, t->nodes.bytes, s));   // unwritten slots read as non-nodes (tietree.hip)
  HIP_TRY(t->box.ensure(2 * sizeof(float4)));   // root_bbox
  HIP_TRY(t->status.ensure(2 * sizeof(int)));
  t->partial = partial;
  if (partial) HIP_TRY(t->sbox.ensure(2 * sizeof(float4) * (size_t)z.big_ids));
  const size_t o_ctl = 0, o_tasks = o_ctl + align256(sizeof(NfCtl)),
               o_pend = o_tasks + align256(sizeof(NfTask) * (size_t)(z.Lmax + 1) * z.max_task),
               o_small = o_pend + align256(sizeof(NfTask) * (size_t)(z.Lmax + 1) * z.max_pend),
               o_cmap = o_small + align256(sizeof(NfTask) * (size_t)z.max_small),
               o_cA = o_cmap + align256(sizeof(int) * 2 * (size_t)z.max_chunks),
               o_cAE = o_cA + align256(sizeof(int) * (size_t)z.max_chunks),
               o_cE2 = o_cAE + align256(sizeof(int) * (size_t)z.max_chunks),
               o_tblL = o_cE2 + align256(sizeof(int) * (size_t)z.max_chunks),
               o_tblR = o_tblL + align256(sizeof(float4) * (size_t)nbucket),
               o_ctask = o_tblR + align256(sizeof(float4) * (size_t)nbucket),
               total = o_ctask + align256(sizeof(NfTask) * 2 * (size_t)z.max_chunks);
  HIP_TRY(grow(c->nf_scratch, total, s));
  char* u = c->nf_scratch.as<char>();
  NfBuild b;
  b.vpts = t->vpts.as<float4>();
  b.nodes = t->nodes.as<NfNode>();
  b.box = t->box.as<float4>();
  b.cap = t->cap;
  b.ctl = reinterpret_cast<NfCtl*>(u + o_ctl);
  b.tasks = reinterpret_cast<NfTask*>(u + o_tasks);
  b.pend = reinterpret_cast<NfTask*>(u + o_pend);
  b.small = reinterpret_cast<NfTask*>(u + o_small);
  b.chunk_task = reinterpret_cast<int*>(u + o_cmap);
  b.ctask = reinterpret_cast<NfTask*>(u + o_ctask);
  b.cA = reinterpret_cast<int*>(u + o_cA);
  b.cAE = reinterpret_cast<int*>(u + o_cAE);
  b.cE2 = reinterpret_cast<int*>(u + o_cE2);
  b.tblL = reinterpret_cast<float4*>(u + o_tblL);
  b.tblR = reinterpret_cast<float4*>(u + o_tblR);
  b.quant = cd.quant.as<float>();
  b.sbox = partial ? t->sbox.as<float4>() : nullptr;
  b.sorted = cd.pts.as<float4>();
  b.gate = gate;
  b.n = n;
  b.nbucket = nbucket;
  b.Lmax = Lmax;
  b.max_task = z.max_task;
  b.max_pend = z.max_pend;
  b.max_small = z.max_small;
  b.max_chunks = z.max_chunks;
  b.big_ids = z.big_ids;
  if (off) {
    const long long v[16] = {Lmax, z.max_task, z.max_pend, z.max_small, z.max_chunks, (long long)o_tasks,
                             (long long)o_pend, (long long)o_small, (long long)o_cmap, (long long)o_cA,
                             (long long)o_cAE, (long long)o_cE2, (long long)o_tblL, (long long)total, n, t->cap};
    for (int i = 0; i < 16; ++i) off[i] = v[i];
  }
  HIP_TRY(c->nf_desc.ensure(sizeof(NfBuild)));
  NfBuild* db = c->nf_desc.as<NfBuild>();
  launch_nf_set_desc(s, b, db);   // by value as a kernel argument: no host buffer has to outlive the call
  static const bool no_graph = dev_getenv("DDLO_NF_NO_GRAPH") != nullptr;   // A/B, diagnostics
  if (stop >= 0 || no_graph || same_env) {
    launch_nf_build(s, b, db, stop);
    HIP_TRY(hipGetLastError());
  } else {
    const long long gkey = ((long long)nbucket * 64 + Lmax) * 2 + (partial ? 1 : 0);
    ++c->nf_clock;
    gicp_ctx::NfGraph* ng = nullptr;
    for (auto& e : c->nf_graphs)
      if (e.key == gkey) ng = &e;
    if (!ng) {
      if ((int)c->nf_graphs.size() < kNfGraphs) {
        c->nf_graphs.reserve(kNfGraphs);
        c->nf_graphs.emplace_back();
        ng = &c->nf_graphs.back();
      } else {   // evict the least recently used, after the builds queued on the stream
        ng = &c->nf_graphs[0];
        for (auto& e : c->nf_graphs)
          if (e.last_use < ng->last_use) ng = &e;
        HIP_TRY(hipStreamSynchronize(s));
        if (ng->ge) HIP_TRY(hipGraphExecDestroy(ng->ge));
        ng->ge = nullptr;
        ng->key = -1;
      }
      hipGraph_t g = nullptr;
      HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      launch_nf_build(s, b, db, -1);   // (b.sbox set: the partial build)
      const hipError_t e1 = hipGetLastError();
      const hipError_t e2 = hipStreamEndCapture(s, &g);
      HIP_TRY(e1);
      HIP_TRY(e2);
      const hipError_t e3 = hipGraphInstantiate(&ng->ge, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      HIP_TRY(e3);
      ng->key = gkey;
    }
    ng->last_use = c->nf_clock;
    HIP_TRY(hipGraphLaunch(ng->ge, s));
  }
  if (stop < 0 && !off && !partial) {   // the level counts of this build, for the next one
    if (!c->nf_ntask_host) {
      HIP_TRY(pinned_pool().alloc((void**)&c->nf_ntask_host, sizeof(int) * (kNfMaxLevels + 1), hipHostMallocDefault));
      HIP_TRY(hipEventCreateWithFlags(&c->nf_ntask_ev, hipEventDisableTiming));
    }
    HIP_TRY(hipMemcpyAsync(c->nf_ntask_host, b.ctl->ntask, sizeof(int) * (kNfMaxLevels + 1), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(c->nf_ntask_ev, s));
    c->nf_ntask_bucket = nbucket;
    c->nf_ntask_lmax = Lmax;
  }
  HIP_TRY(hipMemcpyAsync(t->status.p, &b.ctl->err, sizeof(int), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(t->status.as<int>() + 1, &b.ctl->nnodes, sizeof(int), hipMemcpyDeviceToDevice, s));
  if (timed) {
    HIP_TRY(hipEventRecord(c->st_ev[3], s));
    c->st_tree = true;
  }
  HIP_TRY(hipEventRecord(t->ready, s));
  return GICP_OK;
}

gicp_status ensure_nftree(gicp_ctx* c, CloudData& cd, hipStream_t s) {
  if (cd.nf) return GICP_OK;
  auto t = std::make_shared<NfTreeData>();
  gicp_status st = nftree_build(c, cd, s, *t);
  if (st) return st;
  cd.nf = t;
  return GICP_OK;
}

gicp_status ensure_nftree_partial(gicp_ctx* c, CloudData& cd, hipStream_t s) {
  if (cd.nfp || cd.nf) return GICP_OK;
  auto t = std::make_shared<NfTreeData>();
  gicp_status st = nftree_build(c, cd, s, *t, -1, nullptr, c->partial_levels);
  if (st) return st;
  cd.nfp = t;
  return GICP_OK;
}

gicp_status tie_scratch(gicp_ctx* c, int n, hipStream_t s, TieList* tl) {
  // a point is listed at most twice (the task-based kNN, then the lane-per-query kernel for its group)
  HIP_TRY(grow(c->tie_buf, sizeof(int) * (2 * (size_t)n + 64), s));
  HIP_TRY(c->nf_err.ensure(sizeof(int)));
  if (!c->nf_err_host) HIP_TRY(pinned_pool().alloc((void**)&c->nf_err_host, 2 * sizeof(int), hipHostMallocDefault));
  if (!c->nf_err_pending) {
    HIP_TRY(hipMemsetAsync(c->nf_err.p, 0, sizeof(int), s));
    c->nf_err_pending = true;
  }
  HIP_TRY(hipMemsetAsync(c->tie_buf.p, 0, sizeof(int), s));
  tl->count = c->tie_buf.as<int>();
  tl->list = c->tie_buf.as<int>() + 64;
  tl->cap = 2 * n;
  return GICP_OK;
}

gicp_status check_ties(gicp_ctx* c) {
  if (!c->nf_err_pending) return GICP_OK;
  c->nf_err_pending = false;
  const int e = *(volatile int*)c->nf_err_host;
  if (e)
    return fail(GICP_EHIP, "nanoflann tie order: the device kd-tree build or search failed (resolver bits " +
                               std::to_string(e & 255) + ", build bits " + std::to_string(e >> 8) + ")");
  return GICP_OK;
}

gicp_status publish_ties(gicp_ctx* c, hipStream_t s) {
  if (c->nf_err_pending) HIP_TRY(hipMemcpyAsync(c->nf_err_host, c->nf_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
  return GICP_OK;
}

// workgroups of the lazy tie search: one tied query each at a time, a
// private copy of the cloud each (scratch bounded by ~256 MB)
int lazy_workgroups(int n) {
  const size_t per = nf_lazy_bytes(n, 1) - nf_lazy_bytes(n, 0);
  return (int)std::max<size_t>(1, std::min<size_t>(64, (size_t(256) << 20) / std::max<size_t>(per, 1)));
}

gicp_status compute_cov(gicp_ctx* c, Side& side, int k_use) {
  if (!side.cloud) return fail(GICP_ESTATE, "no cloud on this side");
  const int k = k_use > 0 ? k_use : c->params.k_correspondences;
  if (k <= 0 || k > 64) return fail(GICP_EINVAL, "k_correspondences must be in [1, 64]");
  if (side.cloud->n < k) return fail(GICP_ETOOFEW, "cloud has fewer points than k_correspondences");
  auto cv = std::make_shared<CovData>();
  cv->n = side.cloud->n;
  HIP_TRY(cv->cov6.ensure(sizeof(double) * 6 * (size_t)cv->n));
  if (c->profiling && !c->st_ev[0])
    for (auto& e : c->st_ev) HIP_TRY(hipEventCreate(&e));
  // stage times: only what this pass records (a tree built earlier, e.g. with
  // the index, is not this pass's; nothing is reported from an older pass)
  c->st_tree = false;
  c->st_resolve = false;
  struct InCov {
    gicp_ctx* c;
    ~InCov() { c->st_in_cov = false; }
  } in_cov{c};
  c->st_in_cov = c->profiling;
  // GICP_OPT_COV_TASKS: the task-based kNN (knn_tasks.hip) — exact, but not
  // faster than the lane-per-query kernel on the cfg 5 clouds
  const bool tasks = c->cov_tasks;
  const CloudDev cd = side.cloud->dev();
  // exact ties: the points whose k-th neighbour distance is tied get their
  // neighbourhood from nanoflann's own search (nftree.hip)
  TieList tl{nullptr, nullptr};
  // the previous pass's tie count (once its copy has landed): many ties make
  // the whole tree cheaper than one lazy search per tied query
  if (c->tie_cnt_pending && hipEventQuery(c->tie_cnt_ev) == hipSuccess) {
    c->lazy_heavy = c->nf_err_host[1] > 2 * std::max(c->lazy_wgs_last, 1);
    c->tie_cnt_pending = false;
  }
  const bool lazy = c->tie_exact && c->tie_lazy && !c->lazy_heavy && !side.cloud->nf;
  const bool gated = lazy && c->nf_same_stream && !side.cloud->nfp;
  if (c->tie_exact) {
    gicp_status st = gated ? GICP_OK
                     : lazy ? ensure_nftree_partial(c, *side.cloud, c->stream)
                            : ensure_nftree(c, *side.cloud, c->stream);
    if (!st) st = tie_scratch(c, side.cloud->n, c->stream, &tl);
    if (st) return st;
  }
  if (c->profiling) HIP_TRY(hipEventRecord(c->st_ev[0], c->stream));
  if (tasks && k <= 32) {
    // scratch of the task-based kNN; a queued covariance launch may still
    // read the old block, so growing it waits for the stream
    const int n = cv->n;
    const int cap = std::max(64, 6 * k);
    const int cap2 = 8 * cap, max2 = std::max(256, n / 64);   // second round: ~1 % of the points, longer lists
    const int cap_r = knn_task_cap_per_region(n);
    const size_t o_q = 0, o_cnt = o_q + align256(sizeof(float4) * ((size_t)(n + 15) / 16 * 16)),
                 o_redo = o_cnt + align256(sizeof(unsigned) * (size_t)n), o_again = o_redo + align256((size_t)(n + 63) / 64),
                 o_slot2 = o_again + align256((size_t)n), o_n2 = o_slot2 + align256(sizeof(int) * (size_t)n),
                 o_ctr = o_n2 + 256,
                 o_tasks = o_ctr + align256(sizeof(unsigned) * kTaskRegions * kCtrStride),
                 o_cand = o_tasks + align256(sizeof(unsigned long long) * (size_t)kTaskRegions * cap_r),
                 o_cand2 = o_cand + align256(sizeof(unsigned long long) * (size_t)n * cap),
                 total = o_cand2 + sizeof(unsigned long long) * (size_t)max2 * cap2;
    if (total > c->knn.bytes) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      HIP_TRY(c->knn.ensure(total));
    }
    char* u = c->knn.as<char>();
    KnnJob j;
    j.c = cd;
    j.k = k;
    j.method = c->params.regularization;
    j.cov6 = cv->cov6.as<double>();
    j.qstate = reinterpret_cast<float4*>(u + o_q);
    j.cnt = reinterpret_cast<unsigned*>(u + o_cnt);
    j.redo = reinterpret_cast<unsigned char*>(u + o_redo);
    j.again = reinterpret_cast<unsigned char*>(u + o_again);
    j.round = 1;
    j.slot2 = reinterpret_cast<int*>(u + o_slot2);
    j.n2 = reinterpret_cast<unsigned*>(u + o_n2);
    j.cand2 = reinterpret_cast<unsigned long long*>(u + o_cand2);
    j.cap2 = cap2;
    j.max2 = max2;
    j.task_ctr = reinterpret_cast<unsigned*>(u + o_ctr);
    j.tasks = reinterpret_cast<unsigned long long*>(u + o_tasks);
    j.cand = reinterpret_cast<unsigned long long*>(u + o_cand);
    j.cap = cap;
    j.task_cap_r = cap_r;
    j.split_extent = 5.0f;
    j.tie_list = tl.list;
    j.tie_count = tl.count;
    j.tie_cap = tl.cap;
    if (!launch_knn_covariances(c->stream, j, side.cloud->upper_count()))
      return fail(GICP_EINVAL, "unsupported k");
    launch_covariances(c->stream, cd, k, c->params.regularization, cv->cov6.as<double>(), j.redo, tl);
    if (dev_getenv("DDLO_COV_DEBUG")) {   // development: how many groups needed the fallback
      std::vector<unsigned char> r((n + 63) / 64);
      std::vector<unsigned> cn(n);
      HIP_TRY(hipMemcpyAsync(r.data(), j.redo, r.size(), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipMemcpyAsync(cn.data(), j.cnt, sizeof(unsigned) * n, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      size_t nr = 0, over = 0, sum = 0, mx = 0;
      for (auto v : r) nr += v;
      for (auto v : cn) { over += v > (unsigned)cap; sum += v; mx = std::max<size_t>(mx, v); }
      std::fprintf(stderr, "[cov] n %d k %d redo groups %zu / %zu, points over cap %zu, mean cand %.1f max %zu\n", n, k,
                   nr, r.size(), over, (double)sum / n, mx);
    }
  } else if (!launch_covariances(c->stream, cd, k, c->params.regularization, cv->cov6.as<double>(), nullptr, tl)) {
    return fail(GICP_EINVAL, "unsupported k");
  }
  if (c->profiling) HIP_TRY(hipEventRecord(c->st_ev[1], c->stream));
  c->st_resolve = c->tie_exact && c->profiling;
  if (c->tie_exact) {
    if (lazy) {
      const int n = side.cloud->n;
      const int wgs = lazy_workgroups(n);
      HIP_TRY(grow(c->lazy_buf, nf_lazy_bytes(n, wgs), c->stream));
      if (gated) {   // after the covariance kernel, on the stream: no work when no query is tied
        if (!c->nf_gated) c->nf_gated = std::make_unique<NfTreeData>();
        gicp_status st = nftree_build(c, *side.cloud, c->stream, *c->nf_gated, -1, nullptr, c->partial_levels, tl.count);
        if (st) return st;
      }
      const NfTreeData& tp = gated ? *c->nf_gated : *side.cloud->nfp;
      HIP_TRY(nftree_join(tp, c->stream));
      if (c->profiling) HIP_TRY(hipEventRecord(c->st_ev[4], c->stream));
      if (!launch_nf_lazy(c->stream, tp.dev(), cd, nullptr, tl, k, c->params.regularization, cv->cov6.as<double>(),
                          nullptr, nullptr, c->lazy_buf.p, wgs, tp.status.as<int>(), c->nf_err.as<int>()))
        return fail(GICP_EINVAL, "nanoflann tie order: the lazy tie search cannot run (k > 64 or no partial tree)");
      if (c->profiling) HIP_TRY(hipEventRecord(c->st_ev[5], c->stream));
      c->lazy_wgs_last = wgs;
    } else {
      HIP_TRY(nftree_join(*side.cloud->nf, c->stream));
      if (c->profiling) HIP_TRY(hipEventRecord(c->st_ev[4], c->stream));
      launch_nf_resolve_cov(c->stream, side.cloud->nf->dev(), cd, tl, k, c->params.regularization,
                            cv->cov6.as<double>(), side.cloud->nf->status.as<int>(), c->nf_err.as<int>());
      if (c->profiling) HIP_TRY(hipEventRecord(c->st_ev[5], c->stream));
      c->lazy_wgs_last = lazy_workgroups(side.cloud->n);
    }
    if (c->tie_lazy) {   // the count for the next pass's choice
      if (!c->tie_cnt_ev) HIP_TRY(hipEventCreateWithFlags(&c->tie_cnt_ev, hipEventDisableTiming));
      HIP_TRY(hipMemcpyAsync(c->nf_err_host + 1, tl.count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipEventRecord(c->tie_cnt_ev, c->stream));
      c->tie_cnt_pending = true;
    }
    gicp_status st = publish_ties(c, c->stream);
    if (st) return st;
    static const bool dbg = dev_getenv("DDLO_TIE_DEBUG") != nullptr;   // development: tied queries per cloud
    if (dbg) {
      int cnt = 0;
      HIP_TRY(hipMemcpyAsync(&cnt, tl.count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      std::fprintf(stderr, "[ties] n %d k %d tied %d\n", side.cloud->n, k, cnt);
      if (const char* path = dev_getenv("DDLO_TIE_DUMP")) {   // the tied queries' original indices, one line per cloud
        const int m = std::min(cnt, tl.cap);
        std::vector<int> pos(m), perm(side.cloud->n);
        HIP_TRY(hipMemcpyAsync(pos.data(), tl.list, sizeof(int) * m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(perm.data(), side.cloud->perm.p, sizeof(int) * perm.size(), hipMemcpyDeviceToHost,
                               c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (FILE* f = std::fopen(path, "a")) {
          std::fprintf(f, "%d %d", side.cloud->n, k);
          for (int p : pos) std::fprintf(f, " %d", p < side.cloud->n ? perm[p] : -1);
          std::fprintf(f, "\n");
          std::fclose(f);
        }
      }
    }
  }
  HIP_TRY(hipGetLastError());
  side.cov = cv;
  return GICP_OK;
}

}  // namespace rt
}  // namespace ddlo
