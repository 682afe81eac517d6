// launch.hpp — host-callable launchers of the kernels in the stage files
// (index_build, covariance, corr_search, moments, outputs .hip) and the other
// translation units.  The host runtime (cloud.hip, align.hip and the other host-only
// files) only sees these plain functions.
#pragma once
#include <hip/hip_runtime.h>

#include "gicp_types.hpp"

namespace ddlo {

void launch_pack_bbox(hipStream_t s, const unsigned char* raw, size_t stride, int n, float4* out, float* partial,
                      int* nonfinite, int nblocks);
void launch_bbox_final(hipStream_t s, const float* partial, int nparts, float* quant);
void launch_morton(hipStream_t s, const float4* pts, int n, const float* quant, unsigned long long* keys, int* vals);
void launch_gather(hipStream_t s, const float4* raw, const int* perm, int n, int npad, float4* sorted, int* inv_perm);
void launch_key_dir(hipStream_t s, const unsigned long long* keys, int n, int* dir);
// the sorted points' per-leaf SoA copy (nleaves whole leaves) and the leaves' boxes (real points only)
void launch_leaf_soa_boxes(hipStream_t s, const float4* pts, int n, int nleaves, float* soa, float4* lo, float4* hi);
void launch_level_boxes(hipStream_t s, const float4* clo, const float4* chi, int nchild, int nparent, float4* plo,
                        float4* phi);
// returns false if k is unsupported (> 64)
// redo: nullptr = every point, else only the 64-point groups flagged 1
// ties (optional): sorted positions whose k-neighbourhood has an exact
// distance tie at its boundary are appended to ties->list (nftree.hip
// resolves them in nanoflann's order)
struct TieList {
  int* list;
  int* count;
  int cap = 0;   // list capacity: an append beyond it is dropped and the resolver reports the overflow
  __device__ __forceinline__ void push(int i) const {
    const int slot = atomicAdd(count, 1);
    if (slot < cap) list[slot] = i;
  }
};
bool launch_covariances(hipStream_t s, const CloudDev& c, int k, int method, double* cov6, const unsigned char* redo,
                        TieList ties = TieList{nullptr, nullptr});
// task-based kNN-k covariances (knn_tasks.hip), k <= 32; groups it flags in
// j.redo must then be recomputed with launch_covariances(..., j.redo)
bool launch_knn_covariances(hipStream_t s, const KnnJob& j, int tgt_upper);
int knn_task_cap_per_region(int n);
// ties: query rows whose answer holds an exact distance tie (inside the k or
// at its boundary) are listed for the nanoflann-order resolver
bool launch_knn_query(hipStream_t s, const CloudDev& c, const float4* q, int nq, int k, int* out_idx, float* out_d,
                      TieList ties = TieList{nullptr, nullptr});
void launch_cov_import(hipStream_t s, const double* in, int layout, int n, const int* inv_perm, double* cov6);
void launch_cov_export(hipStream_t s, const double* cov6, int layout, int n, const int* perm, double* out);
// tietree.hip: a slab shard's restriction of the whole submap's nanoflann tree
size_t tie_prune_scratch_bytes(int n, int cap);
hipError_t launch_tie_prune(hipStream_t s, const NfTreeDev& t, int cap, const int* local_index, int n_local,
                            void* scratch, NfNode* out_nodes, float4* out_pts, unsigned* counts);
void launch_align_init(hipStream_t s, AlignJob* job, const AlignJob* job_src);
// tgt_upper: number of upper-level (>= 1) boxes of the target (LDS cache size)
// Launch geometry of one linearize (grids, upper-box LDS cache), bucketed by
// cloud size; part of the chunk-graph key.
struct LinGeom {
  int seed_blocks, scan_blocks, mom_blocks, lds_boxes, lookup_blocks;
  bool fuse_lm = false;   // the LM step runs in the moment kernel's last block (no k_lm_step launch)
  AlignState* state = nullptr;   // the job's state (job->state), a kernel argument of the moment kernel
  bool grid = false;      // the target's candidate cells answer the search first (k_cell_lookup)
  bool grid_walk = true;  // ... and some of its cells have no list: the walk kernel follows the lookup
};
bool lm_fusion_enabled(bool lookup);   // unsharded aligns on the one-kernel lookup path (DDLO_FUSE_LM: dev A/B)
LinGeom linearize_geometry(int nsrc, int tgt_upper);
// publish: with g.fuse_lm, the host-mapped state slot the fused LM step publishes to (or nullptr)
void launch_linearize(hipStream_t s, const AlignJob* job, const LinGeom& g, AlignState* publish = nullptr);
bool linearize_is_one_kernel(const LinGeom& g);   // every query is answered by its cell: the lookup runs in k_moments
// An align's first iteration without k_align_init in front of it (k_moments_fresh): only where
// linearize_is_one_kernel(g) && g.fuse_lm, for a device job that is this align's but for the guess and
// the ticket and a state whose tie words are 0.
void launch_linearize_fresh(hipStream_t s, const AlignJob* job, const LinGeom& g, const FreshStart& fs,
                            AlignState* publish = nullptr);
int search_queries_per_wave();
int task_cap_per_region(int nsrc);   // task-list slots per region for nsrc source points
int moment_blocks(int nsrc);  // slab rows written by the moment kernel
int lm_slab_rows_max();       // the most slab rows one LM step reduces (kMomBlocksMax)
// st / slab / nblocks / premom: the job's state, slab rows and (sharded) all-reduced moments, as
// kernel arguments (the state and slab loads then need no job load first)
void launch_lm_step(hipStream_t s, const AlignJob* job, AlignState* st, const double* slab, int nblocks,
                    const double* premom, AlignState* publish);
void launch_mom_reduce(hipStream_t s, const AlignJob* job);  // sharded align: slab -> job->mom
void launch_residuals(hipStream_t s, const AlignJob* job, int nsrc, double* out);
void launch_residual_image(hipStream_t s, const float4* pts, const int* perm, const int* inv_perm, int n,
                           const double* residual, double tmin, double tmax, int W, int H, int* winner, float* img,
                           float* xyz);
void launch_transform(hipStream_t s, const float4* pts, int n, const int* perm, const float* T16, float* out,
                      size_t stride_floats);
void launch_export_corr(hipStream_t s, const AlignJob* job, int nsrc, int* corr, float* sqd);

// nftree.hip: nanoflann's kd-tree on the device (tie order) and the tie resolvers
NfSizes nf_sizes(int n);
// sorted_pts: the cloud's Morton-sorted points (w = original index)
// stop >= 0: run only that many big levels (diagnostics)
void launch_nf_build(hipStream_t s, const NfBuild& hb, const NfBuild* db, int stop = -1);
// *db = b on the stream (the descriptor the build kernels read)
void launch_nf_set_desc(hipStream_t s, const NfBuild& b, NfBuild* db);
// status = {build error bits, node count}; nodes: 4 ints per node (c1, c2, feat, parent), f: divlow, divhigh
void launch_nf_export(hipStream_t s, const NfTreeDev& t, const int* status, int cap, int* vind, int* nodes, float* f);
// re-run the listed (tied) queries with nanoflann's search; status: the
// tree build's error bits (nonzero: nothing resolved, *err |= 2); *err |= 1
// on a failed search
bool launch_nf_resolve_cov(hipStream_t s, const NfTreeDev& t, const CloudDev& c, TieList ties, int k, int method,
                           double* cov6, const int* status, int* err);
bool launch_nf_resolve_knn(hipStream_t s, const NfTreeDev& t, const float4* q, TieList ties, int k, int* out_idx,
                           float* out_d, const int* status, int* err);
// the same re-run on the cloud's partial tree (nftree_build partial_levels):
// each listed query's nanoflann search walks the built top levels and splits
// the stubs it enters lazily, on a private copy of their vind ranges (one
// workgroup per query, wgs workgroups; scratch: nf_lazy_bytes(c.n, wgs)).
// cov6 != nullptr: the cloud's own tied points get their covariances; else
// rows of q their (out_idx, out_d).  *err |= 1 depth, 2 build, 4 fewer than k,
// 16 pairing check.
size_t nf_lazy_bytes(int n, int wgs);
bool launch_nf_lazy(hipStream_t s, const NfTreeDev& t, const CloudDev& c, const float4* q, TieList ties, int k,
                    int method, double* cov6, int* out_idx, float* out_d, void* scratch, int wgs, const int* status,
                    int* err);
void launch_cov_remap(hipStream_t s, const double* old_cov6, const int* old_inv_perm, const int* new_perm, int n,
                      double* cov6);

// preprocess.hip (odometry driver): see the kernels there for the reference
// filters they restate.  Scratch sizes: *_tmp_bytes (hipcub temporaries).
// ioff (ddlo_intensity.h): 0 = w is 0; else w = the float ioff (>= 12) bytes into each record
void launch_pack4(hipStream_t s, const unsigned char* raw, size_t stride, int n, float4* out, size_t ioff = 0);
// the row/column filter's registration pass (ddlo_downsample.h): |S| of a rows x cols image, the
// number of S's pixels below n, and the pack of exactly those, ascending, into out (returns that number)
long long rowcol_size(int rows, int cols, int row_step, int col_step);
int rowcol_count(int n, int rows, int cols, int row_step, int col_step);
int launch_pack4_rowcol(hipStream_t s, const unsigned char* raw, size_t stride, int n, int rows, int cols, int row_step,
                        int col_step, float4* out, size_t ioff = 0);
// centre of the crop box (CropBox::setTranslation); the origin by default
struct CropCentre {
  float x = 0.f, y = 0.f, z = 0.f;
};
// pin: pinned host ints for the count read-back (crop_box 2, voxel_grid 16)
// box = false: no box, only the non-finite points are dropped
int crop_box(hipStream_t s, const float4* in, int n, float size, float4* out, int* keep, int* pos, void* tmp,
             size_t tmp_bytes, int* count_host, int* pin, CropCentre centre = CropCentre(), bool box = true);
size_t crop_box_tmp_bytes(int n);
// crop_box's second half on flags of the caller's (keep[i] = 0 / 1): the
// flagged points to out in input order; scratch and pin as for crop_box
int compact_flagged(hipStream_t s, const float4* in, int n, float4* out, const int* keep, int* pos, void* tmp,
                    size_t tmp_bytes, int* count_host, int* pin);
// crop > 0: the crop box (points inside [-crop, crop]^3 removed) folded into the same pass
// order: ddlo_voxel_order.  0 (input order) launches what it always did and reads neither
// oscratch nor anything of voxel_order.hip; 1 (PCL order) sums every voxel's points in the order
// std::sort leaves them and needs oscratch = voxel_order_scratch_ints(n) ints of its own.
// intensity: w is a channel, averaged as x, y, z are (same points, order and count); false
// launches the kernel it always did, and the centroids' w is 0.
int voxel_grid(hipStream_t s, const float4* in, int n, float leaf, float4* out, int* scratch, void* tmp, size_t tmp_bytes,
               int* count_host, float crop, int* pin, CropCentre centre = CropCentre(), int order = 0,
               int* oscratch = nullptr, bool intensity = false);
size_t voxel_tmp_bytes(int n);
constexpr size_t voxel_scratch_ints(int n) { return 7 * (size_t)n + 16 + 6 * 64; }

// voxel_order.hip: std::sort's permutation of (key, index) pairs on the device.
// A segment of at most this many pairs finishes its recursion in LDS.
constexpr int kVoxelOrderHandOver = 512;
size_t sort_order_scratch_ints(int n);
size_t voxel_order_scratch_ints(int n);
// the introsort loop (partition levels, depth-limit heap sorts) in place on (keys, idx)[0, ns): ns = n,
// or the count of a compaction (pos = exclusive sum of keep over n), read on the device.  The caller's
// stable sort by key completes std::sort.  No host synchronisation.
void launch_sort_order(hipStream_t s, unsigned* keys, int* idx, int n, const int* pos, const int* keep, int* scratch);
// the voxel pass's pairs with key != UINT_MAX compacted in input order and permuted; the tails of
// *ck_out / *ci_out (in oscratch) keep UINT_MAX / 0.  -2: tmp too small (an exclusive sum over n).
int voxel_order_pairs(hipStream_t s, const unsigned* keys, const int* idx, int n, int* oscratch, void* tmp,
                      size_t tmp_bytes, unsigned** ck_out, int** ci_out);
void median_range_async(hipStream_t s, const float4* in, int n, float* d, float* result, void* tmp, size_t tmp_bytes,
                        float* out);
size_t median_tmp_bytes(int n);
// w_orig: the intensities of the outputs (original order), or nullptr: w = 0
void launch_transform4(hipStream_t s, const float4* pts, const int* perm, int n, const float* T12, float4* out,
                       const float* w_orig = nullptr);
void launch_take_w(hipStream_t s, const float4* in, int n, float* w);
// organized raw scan -> world frame float4, pixel order kept (non-finite pixels: NaN)
// ioff: as launch_pack4's
void launch_transform_raw(hipStream_t s, const unsigned char* raw, size_t stride, int n, const float* T12, float4* out,
                          size_t ioff = 0);
void launch_gather_cov6(hipStream_t s, const double* cov_sorted, const int* perm, int n, double* out);

// deskew.hip (ddlo_deskew.h): a scan's twist as the kernel takes it, by value
struct DeskewTwist {
  double theta, k[3], t[3], ref_time, period;
};
// theta, k = omega / theta (0 when theta == 0) and the rest into *w; false for the identity twist (launch nothing)
bool deskew_twist(const double* omega, const double* t, double ref_time, double period, DeskewTwist* w);
// the header's rules for the time field's place in a record; nullptr when they hold.  inten: the
// intensity channel is on, at ioff
const char* deskew_field_error(int time_type, size_t toff, size_t stride, bool inten, size_t ioff);
// the split log of inv(T_a) * T_b (row-major float poses, taken in double): the constant-velocity prediction
void deskew_between(const float* Ta, const float* Tb, double* omega, double* t);
// the in-place pass over n uploaded records: x, y, z of every point with finite coordinates and time
void launch_deskew(hipStream_t s, unsigned char* raw, size_t stride, int n, int time_type, size_t toff,
                   const DeskewTwist& w);

}  // namespace ddlo
