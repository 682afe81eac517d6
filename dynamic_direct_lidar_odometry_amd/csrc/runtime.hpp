// runtime.hpp — device-side objects of the GICP runtime shared by the C-ABI
// (capi, align, capi_debug, comm, cellgrid_host .hip) and the odometry driver
// (odom.hip): the caching device allocator, ref-counted device clouds
// (Morton-sorted points + search hierarchy) and covariance sets, and the
// per-ctx state behind gicp_ctx.  Types and one-line accessors only: what
// builds a cloud, its nanoflann tree and its covariances is declared here and
// defined in cloud.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <rccl/rccl.h>  // types only (ncclComm_t)

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/ddlo_gicp.h"
#include "gicp_types.hpp"
#include "launch.hpp"
#include "devknobs.hpp"

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return ::ddlo::rt::fail(_e == hipErrorOutOfMemory ? GICP_ENOMEM : GICP_EHIP,          \
                              std::string(#expr) + ": " + hipGetErrorString(_e));           \
  } while (0)

namespace ddlo {
namespace rt {


inline thread_local std::string g_last_error;

inline gicp_status fail(gicp_status s, const std::string& msg) {
  g_last_error = msg;
  return s;
}

// a byte count rounded up to 256: the sub-buffers laid out in one DevBuf start on such offsets
constexpr size_t align256(size_t b) { return (b + 255) / 256 * 256; }


// Caching device allocator.  hipFree synchronizes the whole device, which
// would serialize every ctx of a multi-stream batch (a new cloud index and
// covariance set per scan); released blocks go to a per-(device, size class)
// free list instead and are handed out again.  Safe because every entry
// point that enqueues work on a buffer waits for it before returning, so a
// buffer is idle whenever its owner releases it (the speculative no-op
// iteration of an align touches only ctx-owned state, freed at ctx
// destruction after a stream synchronize).
struct DevicePool {
  std::mutex m;
  std::multimap<std::pair<int, size_t>, void*> free_blocks;
  static size_t size_class(size_t b) {  // <= 12.5 % rounding, so same-shape clouds share a class
    b = std::max<size_t>(b, 256);
    size_t top = 1;
    while ((top << 1) <= b) top <<= 1;
    const size_t g = std::max<size_t>(top / 8, 256);
    return (b + g - 1) / g * g;
  }
  hipError_t alloc(size_t cls, void** p) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    {
      std::lock_guard<std::mutex> lk(m);
      auto it = free_blocks.find({dev, cls});
      if (it != free_blocks.end()) {
        *p = it->second;
        free_blocks.erase(it);
        return hipSuccess;
      }
    }
    e = hipMalloc(p, cls);
    if (e == hipErrorOutOfMemory) {  // give the cached blocks back and retry once
      trim();
      e = hipMalloc(p, cls);
    }
    return e;
  }
  void release(int dev, size_t cls, void* p) {
    std::lock_guard<std::mutex> lk(m);
    free_blocks.insert({{dev, cls}, p});
  }
  void trim() {
    std::lock_guard<std::mutex> lk(m);
    for (auto& kv : free_blocks) (void)hipFree(kv.second);
    free_blocks.clear();
  }
};
inline DevicePool& device_pool() {
  static DevicePool* pool = new DevicePool();  // never destroyed: blocks live until exit
  return *pool;
}

// HIP streams are recycled, not destroyed: a context made after others were
// destroyed gets their streams (and hardware queues) back instead of new
// ones.  The S2S batch in a fresh process: 0.42 ms per pair with recycling,
// 0.46-0.47 without; after 10 contexts made and destroyed it still runs at
// ~0.59-0.64 either way (cause not found: not the streams, not the pinned
// blocks; tools/batch_leg_alone.py).  A released stream is idle (its owner
// synchronized it); the last released is handed out first.
struct StreamPool {
  std::mutex m;
  std::vector<std::pair<int, hipStream_t>> free_streams;
  hipError_t acquire(hipStream_t* s) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    {
      std::lock_guard<std::mutex> lk(m);
      for (size_t i = free_streams.size(); i-- > 0;)
        if (free_streams[i].first == dev) {
          *s = free_streams[i].second;
          free_streams.erase(free_streams.begin() + (long)i);
          return hipSuccess;
        }
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  }
  void release(int dev, hipStream_t s) {
    std::lock_guard<std::mutex> lk(m);
    free_streams.emplace_back(dev, s);
  }
};
inline StreamPool& stream_pool() {
  static StreamPool* pool = new StreamPool();  // never destroyed: streams live until exit
  return *pool;
}

// Pinned host blocks of the contexts (job / state descriptors the device
// reads, read-back flags), recycled like the streams: freed to this list at
// context destruction and handed out again by (size, flags)
struct PinnedPool {
  std::mutex m;
  std::multimap<std::pair<size_t, unsigned>, void*> free_blocks;
  hipError_t alloc(void** p, size_t bytes, unsigned flags) {
    {
      std::lock_guard<std::mutex> lk(m);
      auto it = free_blocks.find({bytes, flags});
      if (it != free_blocks.end()) {
        *p = it->second;
        free_blocks.erase(it);
        std::memset(*p, 0, bytes);   // no state of the previous owner
        return hipSuccess;
      }
    }
    return hipHostMalloc(p, bytes, flags);
  }
  void release(void* p, size_t bytes, unsigned flags) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(m);
    free_blocks.insert({{bytes, flags}, p});
  }
};
inline PinnedPool& pinned_pool() {
  static PinnedPool* pool = new PinnedPool();  // never destroyed: blocks live until exit
  return *pool;
}

// A pinned host block owned by one handle (staging of small transfers, count
// and record read-backs), grown on demand: its contents are dropped when it
// grows.  Not from PinnedPool: nothing recycles or zero-fills these.
struct PinBuf {
  void* p = nullptr;
  size_t bytes = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() {
    if (p) (void)hipHostFree(p);
  }
  // a new block of exactly b bytes (the fixed-size blocks, or a growth rule of the caller's own)
  hipError_t reset(size_t b) {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    const hipError_t e = hipHostMalloc(&p, b, hipHostMallocDefault);
    if (e != hipSuccess) p = nullptr;
    else bytes = b;
    return e;
  }
  // at least b bytes: twice what is asked for, so that a slowly growing need does not reallocate every time
  hipError_t ensure(size_t b) { return b <= bytes ? hipSuccess : reset(std::max<size_t>(2 * b, 4096)); }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int dev = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  void reset() {
    if (p) device_pool().release(dev, bytes, p);
    p = nullptr;
    bytes = 0;
  }
  hipError_t ensure(size_t b) {
    if (b <= bytes && p) return hipSuccess;
    reset();
    const size_t cls = DevicePool::size_class(b);
    hipError_t e = device_pool().alloc(cls, &p);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    (void)hipGetDevice(&dev);
    bytes = cls;
    return e;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

// m float4 points of device memory as xyz triples in out: read back on the
// stream into a pageable temporary, waited for, then unpacked
inline gicp_status read_xyz(hipStream_t s, const float4* dev, size_t m, float* out) {
  std::vector<float4> h(m);
  HIP_TRY(hipMemcpyAsync(h.data(), dev, sizeof(float4) * m, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (size_t i = 0; i < m; ++i) {
    out[3 * i] = h[i].x;
    out[3 * i + 1] = h[i].y;
    out[3 * i + 2] = h[i].z;
  }
  return GICP_OK;
}

// nanoflann's own kd-tree of a cloud (nftree.hip), built on first need: the
// order in which the reference's search meets equidistant points.
struct NfTreeData {
  int n = 0, cap = 0;
  DevBuf vpts, nodes, box, status;   // status: {the build's error bits, node count} (device ints)
  bool partial = false;              // the top levels only (nftree_build partial_levels): stubs below
  DevBuf sbox;                       // partial: the stubs' passed-down boxes
  hipEvent_t ready = nullptr;        // recorded after the build on the ctx's aux stream; users wait on it
  NfTreeData() = default;
  NfTreeData(const NfTreeData&) = delete;
  NfTreeData& operator=(const NfTreeData&) = delete;
  ~NfTreeData() {
    if (ready) (void)hipEventDestroy(ready);
  }
  NfTreeDev dev() const {
    NfTreeDev t;
    t.vpts = vpts.as<float4>();
    t.nodes = nodes.as<NfNode>();
    t.box = box.as<float4>();
    t.n = n;
    t.partial = partial ? 1 : 0;
    t.sbox = partial ? sbox.as<float4>() : nullptr;
    return t;
  }
};

// Candidate cells of a target cloud for one correspondence bound
// (cellgrid.hip; built by cellgrid_build in cellgrid_host.hip).
struct CellGridData {
  float cap2 = 0.f;            // the bound (AlignJob::cap2) the lists were built for
  bool ok = false;             // built (else the walk answers every query)
  DevBuf dir, fine, ent;
  CellGridDev dev{};
  gicp_grid_info info{};
};

// Immutable device cloud + search hierarchy (shared between ctxs/sides).
struct CloudData {
  int n = 0;
  DevBuf pts, keys, perm, inv_perm, box_lo, box_hi, quant, soa, dir;
  std::shared_ptr<NfTreeData> nf;   // nanoflann's tree (tie order), built on first need
  std::shared_ptr<NfTreeData> nfp;  // its top levels only (the lazy covariance tie search)
  std::shared_ptr<CellGridData> grid;   // candidate cells (S2M targets), built on demand
  float grid_aligns_cap2 = -1.f;        // the bound of the aligns counted in grid_aligns
  int grid_aligns = 0;                  // aligns against this cloud as the target with that bound
  int nlevels = 0;
  int lvl_off[kMaxLevels] = {0};
  int lvl_cnt[kMaxLevels] = {0};
  int upper_count() const {
    return nlevels <= 1 ? 0 : lvl_off[nlevels - 1] + lvl_cnt[nlevels - 1] - lvl_off[1];
  }
  CloudDev dev() const {
    CloudDev c;
    c.pts = pts.as<float4>();
    c.keys = keys.as<unsigned long long>();
    c.perm = perm.as<int>();
    c.inv_perm = inv_perm.as<int>();
    c.box_lo = box_lo.as<float4>();
    c.box_hi = box_hi.as<float4>();
    c.quant = quant.as<float>();
    c.soa = soa.as<float>();
    c.dir = dir.as<int>();
    c.n = n;
    c.nlevels = nlevels;
    c.off0 = lvl_off[0]; c.off1 = lvl_off[1]; c.off2 = lvl_off[2]; c.off3 = lvl_off[3]; c.off4 = lvl_off[4];
    c.cnt0 = lvl_cnt[0]; c.cnt1 = lvl_cnt[1]; c.cnt2 = lvl_cnt[2]; c.cnt3 = lvl_cnt[3]; c.cnt4 = lvl_cnt[4];
    return c;
  }
};

struct CovData {
  int n = 0;
  DevBuf cov6;  // sym6 per SORTED point
};

struct Side {
  std::shared_ptr<CloudData> cloud;
  std::shared_ptr<CovData> cov;
  bool has_cov() const { return cloud && cov && cov->n == cloud->n; }
};

inline int levels_for(int n, int* cnt, int* off) {
  int c = (n + kLeafSize - 1) / kLeafSize;
  int L = 0, o = 0;
  for (;;) {
    if (L >= kMaxLevels) return -1;
    cnt[L] = c;
    off[L] = o;
    o += c;
    ++L;
    if (c <= kFanout) break;
    c = (c + kFanout - 1) / kFanout;
  }
  return L;
}

}  // namespace rt
}  // namespace ddlo

using namespace ddlo;
using namespace ddlo::rt;

// one captured chunk: the graph and its executable instance
struct hipExecGraphPair {
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
};

// The chunk graphs of one launch geometry: [init + n iterations] for the
// predicted iteration count n (one per n, index n - 1) and [1 iteration]
// publishing to state slot s = 0, 1; captured for: RCCL in the chunk, job
// buffer, launch geometry (LinGeom).
struct GraphSet {
  std::array<long long, 7> key{{-1, -1, -1, -1, -1, -1, -1}};
  std::vector<hipExecGraphPair> first;
  hipExecGraphPair rest[2];
  long long last_use = 0;
};
constexpr int kGraphSets = 4;   // geometries a ctx keeps captured (scans straddling a size bucket alternate)
constexpr int kNfGraphs = 4;    // tree-build graphs a ctx keeps captured

constexpr int kDefaultPredictedIters = 4;

struct gicp_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  gicp_params params{};
  Side src, tgt;
  // build scratch
  DevBuf raw_bytes, raw_pts, partial, nonfinite, keys_tmp, vals_tmp, sort_tmp, knn;
  // align buffers
  DevBuf corr, sqd, slab, job_dev, state_dev, tmp_out, stats;
  bool stats_on = false;
  AlignJob* job_host = nullptr;   // pinned
  AlignJob job_last{};            // the job k_align_init last copied whole (AlignJob::job_full)
  bool job_last_valid = false;
  // The next align may start without k_align_init (run_align_graph, k_moments_fresh): the last align
  // on this ctx completed on the graph path without an error and published tie words that are all 0.
  // Cleared with job_last_valid, by every other route that writes the device state and while an
  // align is under way (so an error return leaves it cleared).
  bool fresh_ok = false;
  long long fresh_aligns = 0, init_aligns = 0;   // aligns started by k_moments_fresh / by k_align_init (gicp_get_start_counts)
  AlignJob* job_host_dev = nullptr;     // its device-side address (read by k_align_init)
  AlignState* state_host_dev = nullptr; // state_host's device-side address (written by k_lm_step)
  // pinned, two slots: chunk k publishes its end state to slot k % 2, so the
  // (at most one) chunk queued behind the one the host is reading never
  // writes the bytes being read (no torn pose / done / iter)
  AlignState* state_host = nullptr;
  int state_slot = 0;              // slot holding the state of the last align / linearize
  hipEvent_t tail_ev = nullptr;    // last chunk launched by the last align (may still be queued)
  bool tail_pending = false;
  int grid_max_mb = 0;             // GICP_OPT_GRID_MAX_MB (0: no cap)
  unsigned long long ticket = 0;   // aligns launched (AlignJob::ticket)
  int* flag_host = nullptr;       // pinned
  bool have_align = false;        // a linearize ran against the current src/tgt
  bool dbg_search = false;        // gicp_debug_search_begin's job and state are on the device (gicp_debug_search_step)
  DevBuf dbg_snap;                // a step's carried state, kept until the target has its tie tree
  AlignJob dbg_job{};             // the job gicp_debug_search_begin sent (+ the tie tree a step added): a step runs only while
                                  // the ctx would still build the same one
  int last_nsrc = 0;
  // chunk graphs of the last kGraphSets launch geometries (least recently
  // used evicted)
  std::vector<GraphSet> gsets;
  long long graph_clock = 0;
  int predicted_iters = kDefaultPredictedIters;   // iterations of the previous align on this ctx
  std::vector<hipEvent_t> chunk_ev;
  // second stream: nanoflann's tree (tie order) is built here while the
  // covariance / kNN kernels run on `stream`; the resolvers wait for it
  hipStream_t aux_stream = nullptr;
  hipEvent_t aux_ev = nullptr;
  DevBuf nf_desc;                    // the build descriptor the tree kernels read
  // the build, captured per (size bucket, level count); the last kNfGraphs
  // kept (a scan size straddling a bucket boundary alternates two)
  struct NfGraph {
    long long key = -1;
    hipGraphExec_t ge = nullptr;
    long long last_use = 0;
  };
  std::vector<NfGraph> nf_graphs;
  long long nf_clock = 0;
  // Big levels the builds of this ctx need: the level counts of each build
  // (ctl->ntask, copied to pinned memory after it) set later builds of the
  // size bucket to the most levels any of them used + kNfLevelSpare, so
  // that the graph does not carry ~6 kernels per level that finds no node to
  // split.  A cloud that needs more levels is still exact (its larger nodes
  // go to k_nf_small_global, slowly) and sends the next build back to the
  // full margin.
  int* nf_ntask_host = nullptr;       // pinned [kNfMaxLevels + 1]
  hipEvent_t nf_ntask_ev = nullptr;   // the copy's completion
  int nf_ntask_bucket = -1, nf_ntask_lmax = 0;   // the build the copy belongs to
  struct NfHint {
    int used_max = 0, hint = 0;   // hint 0: the full margin
  };
  std::map<int, NfHint> nf_hints;   // per size bucket: the next build's level count
  // a copied level count is ready to read (its build completed)
  bool nf_ntask_pending_check() const {
    return nf_ntask_bucket >= 0 && nf_ntask_ev && hipEventQuery(nf_ntask_ev) == hipSuccess;
  }
  bool profiling = false;
  std::vector<hipEvent_t> prof_ev;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // spatial sharding: ownership slab + RCCL communicator
  int own_axis = -1;
  float own_lo = -INFINITY, own_hi = INFINITY;
  int own_mod = 0, own_rem = 0;   // interleaved sharding (gicp_set_shard_groups)
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  DevBuf mom;          // [kSlabStride] reduced moments, all-reduced in place
  DevBuf search;       // correspondence search: [qstate f4 x n][key u64 x n][counters][tasks]
  bool speculate = true;    // queue a follow-on chunk before the first one's flag is seen
  bool comm_graphs = true;  // RCCL captured into the chunk graphs (else eager chunks)
  long captures = 0;        // chunk graphs captured (diagnostics: DDLO_GRAPH_DEBUG)
  // exact distance ties in nanoflann's order (gicp_set_tie_order): the tree
  // build scratch, the tied-query list and the resolvers' error word
  bool tie_exact = true;
  DevBuf nf_scratch, tie_buf, nf_err;
  int* nf_err_host = nullptr;   // pinned: [0] copy of nf_err, read after the entry point's final wait;
                                // [1] the last covariance pass's tied-query count
  // covariance ties without a tree (k_nf_lazy): each tied query's search
  // splits only the nodes it walks; a cloud with many ties gets the whole
  // tree instead (lazy_heavy: the previous pass listed more than 2 x the
  // lazy kernel's workgroups)
  bool tie_lazy = true;    // GICP_OPT_TIE_LAZY 0: the whole tree for covariance ties too
  int partial_levels = 3;  // big levels of the partial tree the lazy search starts from (GICP_OPT_TIE_PARTIAL_LEVELS)
  bool cov_tasks = false;  // GICP_OPT_COV_TASKS: the task-based kNN for covariances
  bool lazy_heavy = false;
  // nanoflann's tree on the ctx's own stream, not beside it (gicp_s2s_batch's
  // workers: the other workers fill the device, and a second stream per
  // worker shares the 4 hardware queues with them -- 0.44 against 0.55 ms per
  // pair at 4 workers, tools/batch_streams.py)
  bool nf_same_stream = false;
  // ... and then builds the partial tree after the covariance kernel, into
  // this ctx-owned tree, gated on the tie count (no work for a scan without
  // ties, about half of cfg 5's)
  std::unique_ptr<NfTreeData> nf_gated;
  DevBuf lazy_buf;
  hipEvent_t tie_cnt_ev = nullptr;   // recorded after the count's copy
  bool tie_cnt_pending = false;
  int lazy_wgs_last = 0;
  bool nf_err_pending = false;
  long ties_resolved = 0;       // diagnostics
  std::weak_ptr<NfTreeData> nf_joined;   // the target tree c->stream last waited for
  // slab shard: its restriction of the whole submap's nanoflann tree
  // (tietree.hip; gicp_set_tie_tree), which orders the in-align ties
  std::shared_ptr<NfTreeData> tie_tree;
  // tie builder (gicp_tie_builder_set): the whole submap, its tree, and the
  // buffers of the restrictions exported from it
  std::shared_ptr<CloudData> tie_whole;
  DevBuf tie_scratch, tie_lidx, tie_out_nodes, tie_out_pts, tie_counts;
  std::vector<unsigned char> tie_blob;   // the last exported restriction (gicp_tie_builder_export)
  // candidate cells of the target (gicp_set_target_grid): 0 off, 1 auto, 2 on
  int grid_mode = GICP_GRID_AUTO;
  DevBuf fb;                      // the lookup's walk list: [counters][list segments][masks]
  // stage timing of compute_cov (profiling on): covariance kernel, tree build, resolvers
  hipEvent_t st_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool st_tree = false;          // the last compute_cov built a tree (events 2, 3 recorded)
  bool st_resolve = false;       // ... and ran the tie resolvers (events 4, 5)
  bool st_in_cov = false;        // a profiled compute_cov is running: only its own tree build is timed
};

namespace ddlo {
namespace rt {


inline const AlignState& final_state(const gicp_ctx* c) { return c->state_host[c->state_slot]; }

// Wait for the align's trailing no-op chunk (if one is still queued) before
// a ctx-owned buffer it touches may be released to the device pool.
inline gicp_status drain_tail(gicp_ctx* c) {
  if (c->tail_pending) {
    HIP_TRY(hipEventSynchronize(c->tail_ev));
    c->tail_pending = false;
  }
  return GICP_OK;
}

inline gicp_status set_device(const gicp_ctx* c) {
  HIP_TRY(hipSetDevice(c->device));
  return GICP_OK;
}

// Grow a ctx scratch buffer; work still queued on the stream may read the
// old block, so the stream is drained before it goes back to the pool.
inline hipError_t grow(DevBuf& b, size_t bytes, hipStream_t s) {
  if (bytes <= b.bytes && b.p) return hipSuccess;
  if (b.p) {
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
  }
  return b.ensure(bytes);
}

// ---- cloud.hip: the device cloud, its nanoflann tree, its covariances ----

// xyz: host memory (copied to the device first), or device memory when
// on_device (e.g. a preprocessed scan or a keyframe of the odometry driver).
// check_finite = false (device clouds known finite): no read-back, and the
// call returns without waiting for the build.
// nf_early: start nanoflann's tree of the cloud (ctx's aux stream) as soon
// as its sorted points exist, beside the rest of the index build -- for a
// cloud whose covariances follow (the odometry driver's scans and keyframes)
gicp_status build_cloud(gicp_ctx* c, const float* xyz, size_t n, size_t stride, std::shared_ptr<CloudData>* out,
                        bool on_device = false, bool check_finite = true, bool nf_early = false);

// Build nanoflann's tree of cd into t on the given stream.  stop >= 0 (the
// diagnostics entry only) runs that many big levels and nothing after;
// off (optional, 16 entries) receives the sizes and the scratch offsets.
// partial_levels >= 0: only that many big levels, then stubs (k_nf_stub).
gicp_status nftree_build(gicp_ctx* c, CloudData& cd, hipStream_t s_in, NfTreeData& tr, int stop = -1,
                         long long* off = nullptr, int partial_levels = -1, const int* gate = nullptr,
                         bool zero_nodes = false);
// nanoflann's tree of a cloud (once per cloud, on the given stream)
gicp_status ensure_nftree(gicp_ctx* c, CloudData& cd, hipStream_t s);
// the top levels of nanoflann's tree (the lazy covariance tie search), once per cloud
gicp_status ensure_nftree_partial(gicp_ctx* c, CloudData& cd, hipStream_t s);

// the tied-query list ([count][list n]) and the resolvers' error word, reset on the stream
gicp_status tie_scratch(gicp_ctx* c, int n, hipStream_t s, TieList* tl);
// after the entry point's final wait: a failed tie resolution is an error
// (the answers would silently carry the Morton tie order instead of nanoflann's)
gicp_status check_ties(gicp_ctx* c);
// enqueue the copy of the resolvers' error word that check_ties reads
gicp_status publish_ties(gicp_ctx* c, hipStream_t s);
// workgroups of the lazy tie search
int lazy_workgroups(int n);

// k_use > 0 overrides the ctx's k (a keyframe smaller than k, odom.hip)
gicp_status compute_cov(gicp_ctx* c, Side& side, int k_use = 0);

// stream s waits for the tree's build (enqueued, no host wait)
inline hipError_t nftree_join(const NfTreeData& t, hipStream_t s) { return hipStreamWaitEvent(s, t.ready, 0); }

// at the start of an entry point: a tie error word left pending by an
// earlier call that failed before its check belongs to that call (already
// reported as its failure), not to this one
inline void begin_ties(gicp_ctx* c) { c->nf_err_pending = false; }

// A cloud, covariance or tie-tree change: no linearization to report, and the
// next align sends its whole job (k_align_init keeps per-source values such as
// st->src_radius only across aligns whose job is unchanged; a new cloud may
// reuse the old one's pool blocks, so equal pointers do not prove the same cloud)
inline void invalidate_align(gicp_ctx* c) {
  c->have_align = false;
  c->job_last_valid = false;
  c->fresh_ok = false;
  c->dbg_search = false;
}

}  // namespace rt
}  // namespace ddlo
