// capi_internal.hpp — what the translation units behind include/ddlo_gicp.h
// (capi, align, capi_debug, comm, cellgrid_host .hip) need of one another.
// Only names a second file uses; everything else stays local to its file.
#pragma once
#include "runtime.hpp"

namespace ddlo {
namespace rt {

// byte layout of ctx->search for ns source points
struct SearchLayout {
  size_t qstate, key, ctr, ref, ref_p, sec, key2, tasks, total;
  int cap_r;
  explicit SearchLayout(int ns) {
    cap_r = task_cap_per_region(ns);
    qstate = 0;
    key = align256(sizeof(float4) * (size_t)ns);
    ctr = key + align256(sizeof(unsigned long long) * (size_t)ns);
    ref = ctr + align256(sizeof(unsigned) * (kTaskRegions + 1) * kCtrStride);   // + the moment kernel's arrival counter
    ref_p = ref + align256(sizeof(float4) * (size_t)ns);
    sec = ref_p + align256(sizeof(float4) * (size_t)ns);
    key2 = sec + align256(sizeof(unsigned) * (size_t)ns);
    tasks = key2 + align256(sizeof(unsigned long long) * (size_t)ns);
    total = tasks + sizeof(unsigned long long) * (size_t)kTaskRegions * cap_r;
  }
};

// byte layout of ctx->fb (the lookup's walk list) for ns source points
struct FbLayout {
  size_t ctr, list, mask, total;
  int seg_cap;
  explicit FbLayout(int ns) {
    seg_cap = (ns + 15) / 16 + 1;
    ctr = 0;
    list = align256(sizeof(unsigned) * (kFbSegs + 1) * 32);   // + the align's total
    mask = list + align256(sizeof(int) * (size_t)kFbSegs * seg_cap);
    total = mask + align256(sizeof(unsigned short) * (size_t)seg_cap);
  }
};

// ---- align.hip: the align engine ----

// the search bound of an align: nextafter(float(max_corr^2), +inf) (AlignJob::cap2)
float search_cap2(const gicp_params& p);
// The target's candidate cells answer this ctx's searches (same bound)
bool grid_active(const gicp_ctx* c);

inline int linearize_blocks(int nsrc) { return linearize_geometry(nsrc, 0).mom_blocks; }   // slab rows

// Arms finalize_job's record of the device job: an error return before the
// launch forgets it (see finalize_job in align.hip); done() once the launch succeeded.
struct JobCommit {
  gicp_ctx* c;
  bool ok = false;
  explicit JobCommit(gicp_ctx* ctx) : c(ctx) {}
  void done() { ok = true; }
  ~JobCommit() {
    if (!ok) c->job_last_valid = c->fresh_ok = false;
  }
};
void finalize_job(gicp_ctx* c);
gicp_status fill_job(gicp_ctx* c, const float* guess16, int nblocks);
gicp_status prepare_align(gicp_ctx* c);
gicp_status ensure_tie_tree(gicp_ctx* c);
gicp_status enqueue_iteration(gicp_ctx* c, const AlignJob* jd, int nblocks, AlignState* publish);
void drop_graphs(gicp_ctx* c);

// ---- capi.hip ----

// gicp_set_source; nf_early: the caller computes the source covariances next
// (gicp_s2s_batch), so nanoflann's tree starts with the index build
gicp_status set_source_impl(gicp_ctx* c, const float* xyz, size_t n, size_t stride, int build_index, bool nf_early);

}  // namespace rt
}  // namespace ddlo
