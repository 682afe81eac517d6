// capi.hip — the plain C-ABI of include/ddlo_gicp.h: contexts, parameters and
// options, the clouds of the two sides (ref-counted, so swap/share are O(1))
// and their covariances, and the read-backs of an align's results.  The align
// itself is align.hip; the device cloud and its covariances are cloud.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "capi_internal.hpp"
#include "comm.hpp"

namespace {

// Options (gicp_set_option): the values new contexts take.  A -DDDLO_DEV
// build still reads the old A/B environment variables as the initial values.
static std::atomic<int> g_opt_default[GICP_OPT_COUNT] = {{0}, {1}, {1}, {3}, {0}, {0}};
static const bool g_opt_env_read = [] {
  auto rd = [](const char* name, int opt, bool flag) {
    const char* v = dev_getenv(name);
    if (v && *v) g_opt_default[opt].store(flag ? (*v != '0') : std::max(0, std::atoi(v)));
  };
  rd("DDLO_TIE_EXACT", GICP_OPT_TIE_ORDER, true);
  rd("DDLO_TIE_LAZY", GICP_OPT_TIE_LAZY, true);
  rd("DDLO_TIE_PARTIAL_LEVELS", GICP_OPT_TIE_PARTIAL_LEVELS, false);
  rd("DDLO_COV_TASKS", GICP_OPT_COV_TASKS, true);
  return true;
}();

static gicp_status check_option(int option, int value) {
  if (option <= 0 || option >= GICP_OPT_COUNT) return fail(GICP_EINVAL, "unknown option");
  const bool ok = option == GICP_OPT_TIE_PARTIAL_LEVELS ? (value >= 0 && value <= 24)
                  : option == GICP_OPT_GRID_MAX_MB        ? value >= 0
                                                          : (value == 0 || value == 1);
  if (!ok) return fail(GICP_EINVAL, "option value out of range");
  return GICP_OK;
}

}  // namespace

gicp_status ddlo::rt::set_source_impl(gicp_ctx* c, const float* xyz, size_t n, size_t stride, int build_index,
                                      bool nf_early) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  gicp_status s = set_device(c);
  if (s) return s;
  std::shared_ptr<CloudData> cd;
  s = build_cloud(c, xyz, n, stride, &cd, false, true, nf_early);   // the device cloud is always sorted + indexed (cheap)
  if (s) return s;
  const Side old = c->src;
  c->src.cloud = cd;
  c->src.cov.reset();  // setInputSource clears source covariances (:142)
  if (!build_index && old.has_cov() && old.cloud->n == (int)n) {
    // registerInputSource (:122-130) keeps source_covs_: covariance i stays
    // with point i of the new cloud (a size mismatch is recomputed at align,
    // :186-189, so it is dropped here)
    auto cv = std::make_shared<CovData>();
    cv->n = (int)n;
    HIP_TRY(cv->cov6.ensure(sizeof(double) * 6 * n));
    launch_cov_remap(c->stream, old.cov->cov6.as<double>(), old.cloud->inv_perm.as<int>(), cd->perm.as<int>(), (int)n,
                     cv->cov6.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->src.cov = cv;
  }
  invalidate_align(c);
  return GICP_OK;
}

extern "C" {

int32_t gicp_abi_version(void) { return DDLO_GICP_ABI_VERSION; }
const char* gicp_last_error(void) { return g_last_error.c_str(); }

gicp_status gicp_default_params(gicp_params* p) {
  if (!p) return fail(GICP_EINVAL, "null params");
  p->k_correspondences = 20;
  p->max_iterations = 64;
  p->max_correspondence_distance = FLT_MAX;
  p->transformation_epsilon = 5e-4;
  p->rotation_epsilon = 2e-3;
  p->lm_init_lambda_factor = 1e-9;
  p->regularization = GICP_REG_PLANE;
  p->optimizer = GICP_OPT_LEVENBERG_MARQUARDT;
  p->lm_max_iterations = 10;
  p->fixed_iterations = 0;
  return GICP_OK;
}

gicp_status gicp_ctx_create(int device, gicp_ctx** out) {
  if (!out) return fail(GICP_EINVAL, "null out");
  *out = nullptr;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(GICP_EINVAL, "invalid device ordinal");
  HIP_TRY(hipSetDevice(device));
  auto c = std::make_unique<gicp_ctx>();
  c->device = device;
  gicp_default_params(&c->params);
  HIP_TRY(stream_pool().acquire(&c->stream));
  HIP_TRY(stream_pool().acquire(&c->aux_stream));
  HIP_TRY(hipEventCreateWithFlags(&c->aux_ev, hipEventDisableTiming));
  HIP_TRY(pinned_pool().alloc((void**)&c->job_host, sizeof(AlignJob), hipHostMallocMapped));
  HIP_TRY(pinned_pool().alloc((void**)&c->state_host, 2 * sizeof(AlignState), hipHostMallocMapped));
  HIP_TRY(hipHostGetDevicePointer((void**)&c->job_host_dev, c->job_host, 0));
  HIP_TRY(hipHostGetDevicePointer((void**)&c->state_host_dev, c->state_host, 0));
  HIP_TRY(pinned_pool().alloc((void**)&c->flag_host, sizeof(int) * 4, hipHostMallocDefault));
  HIP_TRY(c->job_dev.ensure(sizeof(AlignJob)));
  HIP_TRY(c->state_dev.ensure(sizeof(AlignState)));
  std::memset(c->state_host, 0, 2 * sizeof(AlignState));
  for (int i = 0; i < 6; ++i) c->state_host->final_hessian[7 * i] = 1.0;  // final_hessian_.setIdentity()
  // stream-ordered (never the legacy stream: another ctx's thread may be
  // capturing its align graph at this moment)
  HIP_TRY(hipMemcpyAsync(c->state_dev.p, c->state_host, sizeof(AlignState), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipEventCreate(&c->ev0));
  HIP_TRY(hipEventCreate(&c->ev1));
  // options (gicp_set_default_option: the process-wide values new contexts take)
  c->tie_exact = g_opt_default[GICP_OPT_TIE_ORDER].load() != 0;
  c->tie_lazy = g_opt_default[GICP_OPT_TIE_LAZY].load() != 0;
  c->partial_levels = g_opt_default[GICP_OPT_TIE_PARTIAL_LEVELS].load();
  c->cov_tasks = g_opt_default[GICP_OPT_COV_TASKS].load() != 0;
  c->grid_max_mb = g_opt_default[GICP_OPT_GRID_MAX_MB].load();
  {
    // DDLO_NF_OWN_STREAM=1 (development): every ctx builds its trees on its
    // own stream, the partial tree gated on the tie count (the S2S batch's
    // workers always do)
    const char* os = dev_getenv("DDLO_NF_OWN_STREAM");
    c->nf_same_stream = os && *os == '1';
  }
  *out = c.release();
  return GICP_OK;
}

gicp_status gicp_ctx_destroy(gicp_ctx* c) {
  if (!c) return GICP_OK;
  if (dev_getenv("DDLO_GRAPH_DEBUG")) std::fprintf(stderr, "[graphs] ctx %p: %ld chunk captures\n", (void*)c, c->captures);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(c->aux_stream);
  drop_graphs(c);
  if (c->comm) (void)rccl().comm_destroy(c->comm);
  for (auto e : c->prof_ev) (void)hipEventDestroy(e);
  for (auto e : c->st_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto e : c->chunk_ev) (void)hipEventDestroy(e);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  pinned_pool().release(c->job_host, sizeof(AlignJob), hipHostMallocMapped);
  pinned_pool().release(c->state_host, 2 * sizeof(AlignState), hipHostMallocMapped);
  pinned_pool().release(c->flag_host, sizeof(int) * 4, hipHostMallocDefault);
  pinned_pool().release(c->nf_err_host, 2 * sizeof(int), hipHostMallocDefault);
  if (c->tie_cnt_ev) (void)hipEventDestroy(c->tie_cnt_ev);
  c->src = Side();
  c->tgt = Side();
  (void)hipStreamSynchronize(c->aux_stream);
  for (auto& e : c->nf_graphs)
    if (e.ge) (void)hipGraphExecDestroy(e.ge);
  pinned_pool().release(c->nf_ntask_host, sizeof(int) * (kNfMaxLevels + 1), hipHostMallocDefault);
  if (c->nf_ntask_ev) (void)hipEventDestroy(c->nf_ntask_ev);
  stream_pool().release(c->device, c->aux_stream);   // (both synchronized above)
  stream_pool().release(c->device, c->stream);
  (void)hipEventDestroy(c->aux_ev);
  delete c;
  return GICP_OK;
}

gicp_status gicp_set_params(gicp_ctx* c, const gicp_params* p) {
  if (!c || !p) return fail(GICP_EINVAL, "null argument");
  if (p->regularization < 0 || p->regularization > 4) return fail(GICP_EINVAL, "invalid regularization method");
  if (p->optimizer < 0 || p->optimizer > 1) return fail(GICP_EINVAL, "invalid optimizer");
  if (p->k_correspondences < 1 || p->k_correspondences > 64) return fail(GICP_EINVAL, "k_correspondences must be in [1, 64]");
  if (p->lm_max_iterations < 1 || p->max_iterations < 0 || p->fixed_iterations < 0)
    return fail(GICP_EINVAL, "invalid iteration limits");
  if (!(p->max_correspondence_distance > 0) || !(p->transformation_epsilon > 0) || !(p->rotation_epsilon > 0))
    return fail(GICP_EINVAL, "distances/epsilons must be positive");
  c->params = *p;
  // per-ctx launch history restarts with the parameters: every rank of a
  // sharded align then derives the same chunk sequence (same collectives)
  c->speculate = true;
  c->predicted_iters = kDefaultPredictedIters;
  return GICP_OK;
}

gicp_status gicp_get_params(const gicp_ctx* c, gicp_params* out) {
  if (!c || !out) return fail(GICP_EINVAL, "null argument");
  *out = c->params;
  return GICP_OK;
}

gicp_status gicp_set_source(gicp_ctx* c, const float* xyz, size_t n, size_t stride, int build_index) {
  return set_source_impl(c, xyz, n, stride, build_index, false);
}

gicp_status gicp_set_target(gicp_ctx* c, const float* xyz, size_t n, size_t stride) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  gicp_status s = set_device(c);
  if (s) return s;
  std::shared_ptr<CloudData> cd;
  s = build_cloud(c, xyz, n, stride, &cd);
  if (s) return s;
  c->tgt.cloud = cd;
  c->tgt.cov.reset();  // (:154)
  c->tie_tree.reset();  // a slab's tie order belongs to the previous target
  invalidate_align(c);
  return GICP_OK;
}

gicp_status gicp_clear_source(gicp_ctx* c) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  c->src = Side();
  invalidate_align(c);
  return GICP_OK;
}
gicp_status gicp_clear_target(gicp_ctx* c) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  c->tgt = Side();
  c->tie_tree.reset();   // a slab's tie order belongs to the cleared target
  invalidate_align(c);
  return GICP_OK;
}

gicp_status gicp_get_size(const gicp_ctx* c, int side, size_t* n) {
  if (!c || !n) return fail(GICP_EINVAL, "null argument");
  const Side& sd = side == GICP_SIDE_SOURCE ? c->src : c->tgt;
  *n = sd.cloud ? (size_t)sd.cloud->n : 0;
  return GICP_OK;
}

gicp_status gicp_compute_covariances(gicp_ctx* c, int side) {
  if (!c || (side != 0 && side != 1)) return fail(GICP_EINVAL, "invalid argument");
  begin_ties(c);
  gicp_status s = set_device(c);
  if (s) return s;
  s = compute_cov(c, side == GICP_SIDE_SOURCE ? c->src : c->tgt);
  if (s) return s;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return check_ties(c);
}

gicp_status gicp_set_covariances(gicp_ctx* c, int side, const double* cov, size_t n, int layout) {
  if (!c || !cov || (side != 0 && side != 1) || (layout != 0 && layout != 1)) return fail(GICP_EINVAL, "invalid argument");
  Side& sd = side == GICP_SIDE_SOURCE ? c->src : c->tgt;
  if (!sd.cloud) return fail(GICP_ESTATE, "set the cloud before its covariances");
  if ((int)n != sd.cloud->n) return fail(GICP_EINVAL, "covariance count != cloud size");
  gicp_status s = set_device(c);
  if (s) return s;
  const size_t w = layout == GICP_COV_MAT4D ? 16 : 6;
  HIP_TRY(c->tmp_out.ensure(sizeof(double) * w * n));
  HIP_TRY(hipMemcpyAsync(c->tmp_out.p, cov, sizeof(double) * w * n, hipMemcpyHostToDevice, c->stream));
  auto cv = std::make_shared<CovData>();  // copy semantics (:161,168): never mutate a shared CovData
  cv->n = (int)n;
  HIP_TRY(cv->cov6.ensure(sizeof(double) * 6 * n));
  launch_cov_import(c->stream, c->tmp_out.as<double>(), layout, (int)n, sd.cloud->inv_perm.as<int>(), cv->cov6.as<double>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  sd.cov = cv;
  return GICP_OK;
}

gicp_status gicp_get_covariances(const gicp_ctx* cc, int side, double* cov, size_t n, int layout) {
  gicp_ctx* c = const_cast<gicp_ctx*>(cc);
  if (!c || !cov || (side != 0 && side != 1) || (layout != 0 && layout != 1)) return fail(GICP_EINVAL, "invalid argument");
  Side& sd = side == GICP_SIDE_SOURCE ? c->src : c->tgt;
  if (!sd.has_cov()) return fail(GICP_ESTATE, "no covariances on this side");
  if ((int)n != sd.cloud->n) return fail(GICP_EINVAL, "n != cloud size");
  gicp_status s = set_device(c);
  if (s) return s;
  const size_t w = layout == GICP_COV_MAT4D ? 16 : 6;
  HIP_TRY(c->tmp_out.ensure(sizeof(double) * w * n));
  launch_cov_export(c->stream, sd.cov->cov6.as<double>(), layout, (int)n, sd.cloud->perm.as<int>(), c->tmp_out.as<double>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(cov, c->tmp_out.p, sizeof(double) * w * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GICP_OK;
}

gicp_status gicp_has_covariances(const gicp_ctx* c, int side, int* has) {
  if (!c || !has || (side != 0 && side != 1)) return fail(GICP_EINVAL, "invalid argument");
  *has = (side == GICP_SIDE_SOURCE ? c->src : c->tgt).has_cov() ? 1 : 0;
  return GICP_OK;
}

gicp_status gicp_swap_source_target(gicp_ctx* c) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  std::swap(c->src, c->tgt);  // clouds, indices and covariances (:100-102)
  c->tie_tree.reset();        // a slab's tie order belonged to the old target
  invalidate_align(c);        // correspondences_.clear() (:104-105)
  return GICP_OK;
}

gicp_status gicp_share_source(gicp_ctx* dst, const gicp_ctx* src) {
  if (!dst || !src) return fail(GICP_EINVAL, "null ctx");
  if (dst->device != src->device) return fail(GICP_EINVAL, "contexts live on different devices");
  dst->src = src->src;
  invalidate_align(dst);
  return GICP_OK;
}

gicp_status gicp_get_residuals(gicp_ctx* c, double* out, size_t n) {
  if (!c || !out) return fail(GICP_EINVAL, "null argument");
  if (!c->have_align || !c->src.cloud || !c->tgt.cloud) return fail(GICP_ESTATE, "no linearization to report residuals of");
  if ((int)n != c->src.cloud->n) return fail(GICP_EINVAL, "n != source size");
  gicp_status s = set_device(c);
  if (s) return s;
  HIP_TRY(c->tmp_out.ensure(sizeof(double) * n));
  launch_residuals(c->stream, c->job_dev.as<AlignJob>(), (int)n, c->tmp_out.as<double>());
  HIP_TRY(hipGetLastError());
  // sharded: every rank holds the exact nearest distance within its tile +
  // halo for every source point (owned matches, unbounded search otherwise);
  // the tiles cover the whole target, so the minimum over ranks is the
  // global 1-NN distance (nano_gicp_impl.hpp:255-257,225-232)
  if (c->comm)
    NCCL_TRY(rccl().all_reduce(c->tmp_out.p, c->tmp_out.p, n, ncclFloat64, ncclMin, c->comm, c->stream));
  HIP_TRY(hipMemcpyAsync(out, c->tmp_out.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GICP_OK;
}

gicp_status gicp_residual_image(gicp_ctx* c, double theta_min, double theta_max, int width, int height, float* img,
                                float* xyz) {
  if (!c || !img) return fail(GICP_EINVAL, "null argument");
  if (width <= 0 || height <= 0 || (long)width * height > (1L << 28) || !(theta_max > theta_min))
    return fail(GICP_EINVAL, "invalid image geometry");
  if (!c->have_align || !c->src.cloud || !c->tgt.cloud) return fail(GICP_ESTATE, "no linearization to report residuals of");
  gicp_status s = set_device(c);
  if (s) return s;
  const int n = c->src.cloud->n;
  const size_t npix = (size_t)width * height;
  HIP_TRY(c->tmp_out.ensure(sizeof(double) * n));
  launch_residuals(c->stream, c->job_dev.as<AlignJob>(), n, c->tmp_out.as<double>());
  if (c->comm)  // sharded: global residual = min over ranks (see gicp_get_residuals)
    NCCL_TRY(rccl().all_reduce(c->tmp_out.p, c->tmp_out.p, n, ncclFloat64, ncclMin, c->comm, c->stream));
  DevBuf winner, dimg, dxyz;
  HIP_TRY(winner.ensure(sizeof(int) * npix));
  HIP_TRY(dimg.ensure(sizeof(float) * npix));
  if (xyz) HIP_TRY(dxyz.ensure(sizeof(float) * 3 * npix));
  HIP_TRY(hipMemsetAsync(winner.p, 0xff, sizeof(int) * npix, c->stream));  // -1: no point
  const CloudData& cd = *c->src.cloud;
  launch_residual_image(c->stream, cd.pts.as<float4>(), cd.perm.as<int>(), cd.inv_perm.as<int>(), n,
                        c->tmp_out.as<double>(), theta_min, theta_max, width, height, winner.as<int>(),
                        dimg.as<float>(), xyz ? dxyz.as<float>() : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(img, dimg.p, sizeof(float) * npix, hipMemcpyDeviceToHost, c->stream));
  if (xyz) HIP_TRY(hipMemcpyAsync(xyz, dxyz.p, sizeof(float) * 3 * npix, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GICP_OK;
}

gicp_status gicp_get_correspondences(gicp_ctx* c, int32_t* corr, float* sq_dist, size_t n) {
  if (!c || (!corr && !sq_dist)) return fail(GICP_EINVAL, "null argument");
  if (!c->have_align || !c->src.cloud) return fail(GICP_ESTATE, "no linearization");
  if ((int)n != c->src.cloud->n) return fail(GICP_EINVAL, "n != source size");
  gicp_status s = set_device(c);
  if (s) return s;
  HIP_TRY(c->tmp_out.ensure((sizeof(int) + sizeof(float)) * n + 64));
  int* dcorr = c->tmp_out.as<int>();
  float* dsqd = reinterpret_cast<float*>(c->tmp_out.as<char>() + ((sizeof(int) * n + 63) / 64) * 64);
  // sq_distances_ holds the unbounded 1-NN distance of EVERY point
  // (nano_gicp_impl.hpp:255-257); the bounded search left +inf for points
  // without a match, so complete those first (same kernel as getResiduals)
  if (sq_dist && c->tgt.cloud) launch_residuals(c->stream, c->job_dev.as<AlignJob>(), (int)n, nullptr);
  launch_export_corr(c->stream, c->job_dev.as<AlignJob>(), (int)n, dcorr, dsqd);
  HIP_TRY(hipGetLastError());
  if (corr) HIP_TRY(hipMemcpyAsync(corr, dcorr, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  if (sq_dist) HIP_TRY(hipMemcpyAsync(sq_dist, dsqd, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GICP_OK;
}

gicp_status gicp_transform_source(gicp_ctx* c, float* out_xyz, size_t n, size_t stride) {
  if (!c || !out_xyz || stride < 12 || stride % 4) return fail(GICP_EINVAL, "invalid argument");
  if (!c->src.cloud) return fail(GICP_ENOSOURCE, "no source");
  if ((int)n != c->src.cloud->n) return fail(GICP_EINVAL, "n != source size");
  gicp_status s = set_device(c);
  if (s) return s;
  // final_transformation_ = x0.cast<float>() of the last align
  float T[16];
  const AlignState& st = final_state(c);
  for (int r = 0; r < 3; ++r) {
    for (int cc = 0; cc < 3; ++cc) T[4 * r + cc] = (float)st.R[3 * r + cc];
    T[4 * r + 3] = (float)st.t[r];
  }
  T[12] = T[13] = T[14] = 0.f;
  T[15] = 1.f;
  const size_t bytes = (n - 1) * stride + 12;
  HIP_TRY(c->tmp_out.ensure(bytes + 256));
  float* dT = reinterpret_cast<float*>(c->tmp_out.as<char>() + ((bytes + 63) / 64) * 64);
  HIP_TRY(hipMemcpyAsync(dT, T, sizeof(T), hipMemcpyHostToDevice, c->stream));
  // keep the caller's other fields (e.g. intensity): start from their buffer
  HIP_TRY(hipMemcpyAsync(c->tmp_out.p, out_xyz, bytes, hipMemcpyHostToDevice, c->stream));
  launch_transform(c->stream, c->src.cloud->pts.as<float4>(), (int)n, c->src.cloud->perm.as<int>(), dT,
                   c->tmp_out.as<float>(), stride / 4);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_xyz, c->tmp_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GICP_OK;
}

gicp_status gicp_knn_target(gicp_ctx* c, const float* q, size_t nq, size_t stride, int k, int32_t* idx, float* sqd) {
  if (!c || !q || !idx || !sqd || nq == 0 || stride < 12 || stride % 4) return fail(GICP_EINVAL, "invalid argument");
  if (!c->tgt.cloud) return fail(GICP_ENOTARGET, "no target");
  if (k < 1 || k > 64) return fail(GICP_EINVAL, "k must be in [1, 64]");
  if (c->tgt.cloud->n < k) return fail(GICP_ETOOFEW, "target has fewer than k points");
  begin_ties(c);
  gicp_status s = set_device(c);
  if (s) return s;
  const size_t raw = (nq - 1) * stride + 12;
  HIP_TRY(c->raw_bytes.ensure(raw));
  HIP_TRY(hipMemcpyAsync(c->raw_bytes.p, q, raw, hipMemcpyHostToDevice, c->stream));
  const int nb = (int)((nq + 255) / 256);
  HIP_TRY(c->raw_pts.ensure(sizeof(float4) * nq));
  HIP_TRY(c->partial.ensure(sizeof(float) * 6 * nb));
  HIP_TRY(c->nonfinite.ensure(sizeof(int)));
  launch_pack_bbox(c->stream, c->raw_bytes.as<unsigned char>(), stride, (int)nq, c->raw_pts.as<float4>(),
                   c->partial.as<float>(), c->nonfinite.as<int>(), nb);
  HIP_TRY(c->tmp_out.ensure((sizeof(int) + sizeof(float)) * nq * k + 64));
  int* didx = c->tmp_out.as<int>();
  float* dd = reinterpret_cast<float*>(c->tmp_out.as<char>() + ((sizeof(int) * nq * k + 63) / 64) * 64);
  TieList tl{nullptr, nullptr};
  if (c->tie_exact) {   // tied answers are re-run in nanoflann's order (nftree.hip)
    s = ensure_nftree(c, *c->tgt.cloud, c->stream);
    if (!s) s = tie_scratch(c, (int)nq, c->stream, &tl);
    if (s) return s;
  }
  if (!launch_knn_query(c->stream, c->tgt.cloud->dev(), c->raw_pts.as<float4>(), (int)nq, k, didx, dd, tl))
    return fail(GICP_EINVAL, "unsupported k");
  if (c->tie_exact) {
    HIP_TRY(nftree_join(*c->tgt.cloud->nf, c->stream));
    launch_nf_resolve_knn(c->stream, c->tgt.cloud->nf->dev(), c->raw_pts.as<float4>(), tl, k, didx, dd,
                          c->tgt.cloud->nf->status.as<int>(), c->nf_err.as<int>());
    s = publish_ties(c, c->stream);
    if (s) return s;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(idx, didx, sizeof(int) * nq * k, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(sqd, dd, sizeof(float) * nq * k, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return check_ties(c);
}

gicp_status gicp_set_tie_order(gicp_ctx* c, int nanoflann_order) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  c->tie_exact = nanoflann_order != 0;
  return GICP_OK;
}

gicp_status gicp_set_option(gicp_ctx* c, int option, int value) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  gicp_status s = check_option(option, value);
  if (s) return s;
  switch (option) {
    case GICP_OPT_TIE_ORDER: c->tie_exact = value != 0; break;
    case GICP_OPT_TIE_LAZY: c->tie_lazy = value != 0; break;
    case GICP_OPT_TIE_PARTIAL_LEVELS: c->partial_levels = value; break;
    case GICP_OPT_COV_TASKS: c->cov_tasks = value != 0; break;
    case GICP_OPT_GRID_MAX_MB: c->grid_max_mb = value; break;
  }
  return GICP_OK;
}

gicp_status gicp_get_option(const gicp_ctx* c, int option, int* value) {
  if (!c || !value) return fail(GICP_EINVAL, "null argument");
  gicp_status s = check_option(option, 0);
  if (s) return s;
  switch (option) {
    case GICP_OPT_TIE_ORDER: *value = c->tie_exact ? 1 : 0; break;
    case GICP_OPT_TIE_LAZY: *value = c->tie_lazy ? 1 : 0; break;
    case GICP_OPT_TIE_PARTIAL_LEVELS: *value = c->partial_levels; break;
    case GICP_OPT_COV_TASKS: *value = c->cov_tasks ? 1 : 0; break;
    case GICP_OPT_GRID_MAX_MB: *value = c->grid_max_mb; break;
  }
  return GICP_OK;
}

gicp_status gicp_set_default_option(int option, int value) {
  gicp_status s = check_option(option, value);
  if (s) return s;
  g_opt_default[option].store(value);
  return GICP_OK;
}

gicp_status gicp_get_default_option(int option, int* value) {
  if (!value) return fail(GICP_EINVAL, "null argument");
  gicp_status s = check_option(option, 0);
  if (s) return s;
  *value = g_opt_default[option].load();
  return GICP_OK;
}

gicp_status gicp_get_tie_order(const gicp_ctx* c, int* nanoflann_order) {
  if (!c || !nanoflann_order) return fail(GICP_EINVAL, "null argument");
  *nanoflann_order = c->tie_exact ? 1 : 0;
  return GICP_OK;
}

namespace {
int64_t tree_bytes(const std::shared_ptr<NfTreeData>& t) {
  return t ? (int64_t)(t->vpts.bytes + t->nodes.bytes + t->box.bytes + t->status.bytes + t->sbox.bytes) : 0;
}
int64_t cloud_bytes(const std::shared_ptr<CloudData>& cd) {
  if (!cd) return 0;
  const CloudData& d = *cd;
  int64_t b = (int64_t)(d.pts.bytes + d.keys.bytes + d.perm.bytes + d.inv_perm.bytes + d.box_lo.bytes +
                        d.box_hi.bytes + d.quant.bytes + d.soa.bytes + d.dir.bytes);
  b += tree_bytes(d.nf) + tree_bytes(d.nfp);
  if (d.grid) b += (int64_t)(d.grid->dir.bytes + d.grid->fine.bytes + d.grid->ent.bytes);
  return b;
}
}  // namespace

gicp_status gicp_get_device_bytes(const gicp_ctx* c, int64_t* out, int nout) {
  if (!c || !out || nout < 1) return fail(GICP_EINVAL, "null argument");
  int64_t v[7] = {0, 0, 0, 0, 0, 0, 0};
  v[1] = cloud_bytes(c->tgt.cloud);
  v[2] = c->src.cloud == c->tgt.cloud ? 0 : cloud_bytes(c->src.cloud);
  v[3] = (c->tgt.cov ? (int64_t)c->tgt.cov->cov6.bytes : 0) + (c->src.cov && c->src.cov != c->tgt.cov ? (int64_t)c->src.cov->cov6.bytes : 0);
  v[4] = tree_bytes(c->tie_tree);
  v[5] = cloud_bytes(c->tie_whole) + (int64_t)(c->tie_scratch.bytes + c->tie_lidx.bytes + c->tie_out_nodes.bytes +
                                               c->tie_out_pts.bytes + c->tie_counts.bytes);
  const DevBuf* scratch[] = {&c->raw_bytes, &c->raw_pts, &c->partial, &c->nonfinite, &c->keys_tmp, &c->vals_tmp,
                             &c->sort_tmp, &c->knn, &c->corr, &c->sqd, &c->slab, &c->job_dev, &c->state_dev,
                             &c->tmp_out, &c->stats, &c->nf_desc, &c->mom, &c->search, &c->nf_scratch, &c->tie_buf,
                             &c->nf_err, &c->lazy_buf, &c->fb};
  for (const DevBuf* b : scratch) v[6] += (int64_t)b->bytes;
  if (c->nf_gated) v[6] += (int64_t)(c->nf_gated->vpts.bytes + c->nf_gated->nodes.bytes + c->nf_gated->box.bytes +
                                     c->nf_gated->status.bytes + c->nf_gated->sbox.bytes);
  v[0] = v[1] + v[2] + v[3] + v[4] + v[5] + v[6];
  for (int i = 0; i < nout && i < 7; ++i) out[i] = v[i];
  for (int i = 7; i < nout; ++i) out[i] = 0;
  return GICP_OK;
}

gicp_status gicp_synchronize(gicp_ctx* c) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  gicp_status s = set_device(c);
  if (s) return s;
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipStreamSynchronize(c->aux_stream));
  return GICP_OK;
}

gicp_status gicp_get_stream(const gicp_ctx* c, void** stream) {
  if (!c || !stream) return fail(GICP_EINVAL, "null argument");
  *stream = (void*)c->stream;
  return GICP_OK;
}

}  // extern "C"
