// comm.hip — spatial shards and their collectives: the RCCL
// dlopen table, the communicator and ownership slab of a ctx, and the slab
// shards' tie order (tie-tree blobs built from the whole submap, tietree.hip,
// and sent from the root rank).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "capi_internal.hpp"
#include "comm.hpp"
#include "nftree.hpp"   // kNfStack: the search depth a tie tree must fit

const Rccl& ddlo::rt::rccl() {
  static Rccl r = [] {
    Rccl x;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
      const char* e = dlerror();
      x.why = std::string("cannot load RCCL: ") + (e ? e : "?");
      return x;
    }
    x.get_unique_id = (decltype(x.get_unique_id))dlsym(h, "ncclGetUniqueId");
    x.comm_init_rank = (decltype(x.comm_init_rank))dlsym(h, "ncclCommInitRank");
    x.comm_destroy = (decltype(x.comm_destroy))dlsym(h, "ncclCommDestroy");
    x.all_reduce = (decltype(x.all_reduce))dlsym(h, "ncclAllReduce");
    x.error_string = (decltype(x.error_string))dlsym(h, "ncclGetErrorString");
    x.broadcast = (decltype(x.broadcast))dlsym(h, "ncclBroadcast");
    x.send = (decltype(x.send))dlsym(h, "ncclSend");
    x.recv = (decltype(x.recv))dlsym(h, "ncclRecv");
    x.group_start = (decltype(x.group_start))dlsym(h, "ncclGroupStart");
    x.group_end = (decltype(x.group_end))dlsym(h, "ncclGroupEnd");
    x.ok = x.get_unique_id && x.comm_init_rank && x.comm_destroy && x.all_reduce && x.error_string;
    if (!x.ok) x.why = "RCCL is missing an entry point";
    return x;
  }();
  return r;
}

extern "C" {

gicp_status gicp_comm_unique_id(uint8_t* out, size_t nbytes) {
  if (!out || nbytes < sizeof(ncclUniqueId)) return fail(GICP_EINVAL, "unique id buffer must hold 128 bytes");
  const Rccl& r = rccl();
  if (!r.ok) return fail(GICP_ECOMM, r.why);
  ncclUniqueId id;
  NCCL_TRY(r.get_unique_id(&id));
  std::memcpy(out, &id, sizeof(id));
  return GICP_OK;
}

gicp_status gicp_set_comm(gicp_ctx* c, const uint8_t* id, size_t nbytes, int nranks, int rank) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  gicp_status s = set_device(c);
  if (s) return s;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->comm) {
    (void)rccl().comm_destroy(c->comm);
    c->comm = nullptr;
  }
  drop_graphs(c);
  c->nranks = 1;
  c->rank = 0;
  c->comm_graphs = true;
  c->tail_pending = false;  // the stream was synchronized above
  c->speculate = true;      // identical launch history on every rank
  c->predicted_iters = kDefaultPredictedIters;
  if (nranks == 0) return GICP_OK;  // detach
  if (!id || nbytes < sizeof(ncclUniqueId) || nranks < 1 || rank < 0 || rank >= nranks)
    return fail(GICP_EINVAL, "invalid communicator arguments");
  const Rccl& r = rccl();
  if (!r.ok) return fail(GICP_ECOMM, r.why);
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  NCCL_TRY(r.comm_init_rank(&c->comm, nranks, uid, rank));
  HIP_TRY(c->mom.ensure(sizeof(double) * kSlabStride));
  c->nranks = nranks;
  c->rank = rank;
  invalidate_align(c);
  return GICP_OK;
}

gicp_status gicp_get_comm_info(const gicp_ctx* c, int* nranks, int* rank, int* graphs) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  if (nranks) *nranks = c->comm ? c->nranks : 0;
  if (rank) *rank = c->rank;
  if (graphs) *graphs = (!c->comm || c->comm_graphs) ? 1 : 0;
  return GICP_OK;
}

gicp_status gicp_set_shard(gicp_ctx* c, int axis, float lo, float hi) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  if (axis < -1 || axis > 2) return fail(GICP_EINVAL, "shard axis must be -1 (none), 0, 1 or 2");
  if (axis >= 0 && !(lo < hi)) return fail(GICP_EINVAL, "empty shard range");
  c->own_axis = axis;
  c->own_lo = axis >= 0 ? lo : -INFINITY;
  c->own_hi = axis >= 0 ? hi : INFINITY;
  invalidate_align(c);
  return GICP_OK;
}

gicp_status gicp_set_shard_groups(gicp_ctx* c, int nparts, int part) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  if (nparts < 0 || (nparts > 0 && (part < 0 || part >= nparts))) return fail(GICP_EINVAL, "invalid shard part");
  c->own_mod = nparts <= 1 ? 0 : nparts;
  c->own_rem = nparts <= 1 ? 0 : part;
  invalidate_align(c);
  return GICP_OK;
}

// ---- slab shards' tie order (tietree.hip, DESIGN.md §5 "Slab shards") ----
// Blob: header, the restricted tree's nodes, its points (x, y, z, local index).
struct TieBlobHeader {
  uint32_t magic, version;
  int32_t n_local, nnodes;
  float box[8];   // root_bbox lo (x, y, z, 0), hi (x, y, z, 0): the whole submap's
};
constexpr uint32_t kTieBlobMagic = 0x31545444u;   // "DTT1"

namespace {
gicp_status check_local_index(const int32_t* local_index, size_t n_local, size_t n) {
  std::vector<unsigned char> seen(n, 0);
  for (size_t i = 0; i < n_local; ++i) {
    if (local_index[i] < 0 || (size_t)local_index[i] >= n) return fail(GICP_EINVAL, "local_index out of range");
    if (seen[(size_t)local_index[i]]++) return fail(GICP_EINVAL, "local_index is not one-to-one");
  }
  return GICP_OK;
}
}  // namespace

gicp_status gicp_tie_builder_set(gicp_ctx* c, const float* xyz, size_t n, size_t stride) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  gicp_status s = set_device(c);
  if (s) return s;
  if (n == 0) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->tie_whole.reset();
    c->tie_scratch.reset();
    c->tie_lidx.reset();
    c->tie_out_nodes.reset();
    c->tie_out_pts.reset();
    c->tie_counts.reset();
    std::vector<unsigned char>().swap(c->tie_blob);
    return GICP_OK;
  }
  if (!xyz) return fail(GICP_EINVAL, "null argument");
  std::shared_ptr<CloudData> cd;
  s = build_cloud(c, xyz, n, stride, &cd);
  if (s) return s;
  auto t = std::make_shared<NfTreeData>();
  s = nftree_build(c, *cd, c->stream, *t, -1, nullptr, -1, nullptr, /*zero_nodes=*/true);
  if (s) return s;
  HIP_TRY(nftree_join(*t, c->stream));
  cd->nf = t;
  c->tie_whole = cd;
  return GICP_OK;
}

gicp_status gicp_tie_builder_export(gicp_ctx* c, const int32_t* local_index, size_t n_local, const void** blob,
                                    size_t* bytes) {
  if (!c || !blob || !bytes) return fail(GICP_EINVAL, "null argument");
  *blob = nullptr;
  *bytes = 0;
  if (!c->tie_whole || !c->tie_whole->nf) return fail(GICP_ESTATE, "no whole cloud: gicp_tie_builder_set first");
  if (n_local == 0 || !local_index) return fail(GICP_EINVAL, "empty local_index");
  const CloudData& W = *c->tie_whole;
  const NfTreeData& T = *W.nf;
  gicp_status s = check_local_index(local_index, n_local, (size_t)W.n);
  if (s) return s;
  s = set_device(c);
  if (s) return s;
  HIP_TRY(c->tie_scratch.ensure(tie_prune_scratch_bytes(T.n, T.cap)));
  HIP_TRY(c->tie_lidx.ensure(sizeof(int) * n_local));
  HIP_TRY(c->tie_out_nodes.ensure(sizeof(NfNode) * (size_t)T.cap));
  HIP_TRY(c->tie_out_pts.ensure(sizeof(float4) * n_local));
  HIP_TRY(c->tie_counts.ensure(sizeof(unsigned) * 4 + 2 * sizeof(float4)));
  HIP_TRY(hipMemcpyAsync(c->tie_lidx.p, local_index, sizeof(int) * n_local, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(launch_tie_prune(c->stream, T.dev(), T.cap, c->tie_lidx.as<int>(), (int)n_local, c->tie_scratch.p,
                           c->tie_out_nodes.as<NfNode>(), c->tie_out_pts.as<float4>(), c->tie_counts.as<unsigned>()));
  unsigned cnt[4];
  float4 box[2];
  int bstat = 0;
  HIP_TRY(hipMemcpyAsync(cnt, c->tie_counts.p, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(box, T.box.p, sizeof(box), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(&bstat, T.status.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (bstat) return fail(GICP_EHIP, "the whole cloud's tree build failed");
  if (cnt[2] || cnt[0] != (unsigned)n_local || cnt[1] == 0 || cnt[1] > (unsigned)T.cap)
    return fail(GICP_EHIP, "tie tree restriction failed");
  const size_t nb = sizeof(TieBlobHeader) + sizeof(NfNode) * cnt[1] + sizeof(float4) * n_local;
  c->tie_blob.resize(nb);
  TieBlobHeader h{};
  h.magic = kTieBlobMagic;
  h.version = 1;
  h.n_local = (int32_t)n_local;
  h.nnodes = (int32_t)cnt[1];
  std::memcpy(h.box, box, sizeof(h.box));
  std::memcpy(c->tie_blob.data(), &h, sizeof(h));
  unsigned char* q = c->tie_blob.data() + sizeof(h);
  HIP_TRY(hipMemcpyAsync(q, c->tie_out_nodes.p, sizeof(NfNode) * cnt[1], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(q + sizeof(NfNode) * cnt[1], c->tie_out_pts.p, sizeof(float4) * n_local,
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *blob = c->tie_blob.data();
  *bytes = nb;
  return GICP_OK;
}

gicp_status gicp_set_tie_tree(gicp_ctx* c, const void* blob, size_t bytes) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  if (bytes == 0) {
    c->tie_tree.reset();
    invalidate_align(c);
    return GICP_OK;
  }
  if (!blob || bytes < sizeof(TieBlobHeader)) return fail(GICP_EINVAL, "tie tree blob too short");
  TieBlobHeader h;
  std::memcpy(&h, blob, sizeof(h));
  if (h.magic != kTieBlobMagic || h.version != 1) return fail(GICP_EINVAL, "not a tie tree blob");
  if (!c->tgt.cloud) return fail(GICP_ESTATE, "set the local target first");
  const int nl = c->tgt.cloud->n;
  if (h.n_local != nl) return fail(GICP_EINVAL, "tie tree is not for a target of this size");
  if (h.nnodes < 1 || bytes != sizeof(h) + sizeof(NfNode) * (size_t)h.nnodes + sizeof(float4) * (size_t)nl)
    return fail(GICP_EINVAL, "tie tree blob size mismatch");
  const unsigned char* q = static_cast<const unsigned char*>(blob) + sizeof(h);
  std::vector<NfNode> nodes((size_t)h.nnodes);
  std::vector<float4> pts((size_t)nl);
  std::memcpy(nodes.data(), q, sizeof(NfNode) * nodes.size());
  std::memcpy(pts.data(), q + sizeof(NfNode) * nodes.size(), sizeof(float4) * pts.size());
  // a tree: every node reached once from the root, within the search's depth;
  // the leaves' point ranges partition [0, n_local)
  {
    std::vector<unsigned char> seen(nodes.size(), 0);
    std::vector<std::pair<int, int>> st{{0, 0}};
    long covered = 0;
    std::vector<int> cover((size_t)nl + 1, 0);
    while (!st.empty()) {
      const auto [v, d] = st.back();
      st.pop_back();
      if (v < 0 || v >= h.nnodes || seen[(size_t)v]++ || d >= kNfStack) return fail(GICP_EINVAL, "tie tree is not a tree");
      const NfNode& nd = nodes[(size_t)v];
      if (nd.feat == -1) {
        if (nd.c1 < 0 || nd.c2 > nl || nd.c1 > nd.c2) return fail(GICP_EINVAL, "tie tree leaf range out of bounds");
        covered += nd.c2 - nd.c1;
        cover[(size_t)nd.c1] += 1;
        cover[(size_t)nd.c2] -= 1;
      } else {
        if (nd.feat < 0 || nd.feat > 2) return fail(GICP_EINVAL, "tie tree node has no cut dimension");
        st.push_back({nd.c2, d + 1});
        st.push_back({nd.c1, d + 1});
      }
    }
    int run = 0;
    for (int i = 0; i < nl; ++i)
      if ((run += cover[(size_t)i]) != 1) return fail(GICP_EINVAL, "tie tree leaves do not partition the points");
    if (covered != nl) return fail(GICP_EINVAL, "tie tree leaves do not partition the points");
  }
  gicp_status s = set_device(c);
  if (s) return s;
  {
    // its points are the local target's, each once (point ids = local indices)
    std::vector<float4> lp((size_t)nl);
    HIP_TRY(hipMemcpyAsync(lp.data(), c->tgt.cloud->pts.p, sizeof(float4) * nl, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<float4> by_orig((size_t)nl);
    for (const float4& p : lp) {
      int o;
      std::memcpy(&o, &p.w, sizeof(int));
      by_orig[(size_t)o] = p;
    }
    std::vector<unsigned char> seen((size_t)nl, 0);
    for (const float4& p : pts) {
      int w;
      std::memcpy(&w, &p.w, sizeof(int));
      if (w < 0 || w >= nl || seen[(size_t)w]++) return fail(GICP_EINVAL, "tie tree points are not the local target's");
      const float4& l = by_orig[(size_t)w];
      if (l.x != p.x || l.y != p.y || l.z != p.z)
        return fail(GICP_EINVAL, "tie tree points are not the local target's (local_index does not map the local "
                                 "target's points onto the whole cloud's)");
    }
  }
  auto t = std::make_shared<NfTreeData>();
  t->n = nl;
  t->cap = h.nnodes;
  HIP_TRY(t->vpts.ensure(sizeof(float4) * (size_t)nl));
  HIP_TRY(t->nodes.ensure(sizeof(NfNode) * (size_t)h.nnodes));
  HIP_TRY(t->box.ensure(2 * sizeof(float4)));
  HIP_TRY(t->status.ensure(2 * sizeof(int)));
  HIP_TRY(hipEventCreateWithFlags(&t->ready, hipEventDisableTiming));
  const int status[2] = {0, h.nnodes};
  HIP_TRY(hipMemcpyAsync(t->vpts.p, pts.data(), sizeof(float4) * (size_t)nl, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(t->nodes.p, nodes.data(), sizeof(NfNode) * nodes.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(t->box.p, h.box, sizeof(h.box), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(t->status.p, status, sizeof(status), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(t->ready, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // the host vectors go out of scope
  c->tie_tree = t;
  invalidate_align(c);
  return GICP_OK;
}

gicp_status gicp_set_tie_target(gicp_ctx* c, const float* xyz, size_t n, size_t stride, const int32_t* local_index,
                                size_t n_local) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  if (n == 0) return gicp_set_tie_tree(c, nullptr, 0);
  if (!xyz || !local_index) return fail(GICP_EINVAL, "null argument");
  if (!c->tgt.cloud || (int)n_local != c->tgt.cloud->n) return fail(GICP_ESTATE, "set the local target first (n_local = its size)");
  gicp_status s = check_local_index(local_index, n_local, n);
  if (s) return s;
  s = gicp_tie_builder_set(c, xyz, n, stride);
  const void* blob = nullptr;
  size_t nb = 0;
  if (!s) s = gicp_tie_builder_export(c, local_index, n_local, &blob, &nb);
  if (!s) s = gicp_set_tie_tree(c, blob, nb);
  const gicp_status s2 = gicp_tie_builder_set(c, nullptr, 0, 0);   // the whole cloud does not stay
  return s ? s : s2;
}

gicp_status gicp_set_tie_trees_from_root(gicp_ctx* c, int root, const void* const* blobs, const size_t* sizes) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  if (!c->comm) return fail(GICP_ESTATE, "no communicator (gicp_set_comm)");
  if (root < 0 || root >= c->nranks) return fail(GICP_EINVAL, "root out of range");
  const int R = c->nranks, me = c->rank;
  // A root without blobs (its builder failed) still enters the collective and
  // broadcasts a failure word, so no rank waits forever on the broadcast.
  const bool root_failed = me == root && (!blobs || !sizes);
  if (R == 1) {
    if (root_failed) return fail(GICP_EINVAL, "the root passes every rank's blob");
    return gicp_set_tie_tree(c, blobs[0], sizes[0]);   // nothing to send
  }
  const Rccl& r = rccl();
  if (!r.ok || !r.broadcast || !r.send || !r.recv || !r.group_start || !r.group_end)
    return fail(GICP_ECOMM, "RCCL point-to-point entry points missing");
  gicp_status s = set_device(c);
  if (s) return s;
  s = drain_tail(c);
  if (s) return s;
  // every rank's blob size and the root's status word (one broadcast), then
  // root -> rank point-to-point
  DevBuf dsz;
  HIP_TRY(dsz.ensure(sizeof(unsigned long long) * ((size_t)R + 1)));
  std::vector<unsigned long long> sz((size_t)R + 1, 0);
  if (me == root) {
    if (root_failed) sz[(size_t)R] = 1;
    else
      for (int k = 0; k < R; ++k) sz[(size_t)k] = sizes[k];
  }
  HIP_TRY(hipMemcpyAsync(dsz.p, sz.data(), sizeof(unsigned long long) * (R + 1), hipMemcpyHostToDevice, c->stream));
  NCCL_TRY(r.broadcast(dsz.p, dsz.p, (size_t)R + 1, ncclUint64, root, c->comm, c->stream));
  HIP_TRY(hipMemcpyAsync(sz.data(), dsz.p, sizeof(unsigned long long) * (R + 1), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (root_failed) return fail(GICP_EINVAL, "the root passes every rank's blob");
  if (sz[(size_t)R]) return fail(GICP_ECOMM, "the root's tie-tree builder failed (no blobs sent)");
  DevBuf sendb, recvb;
  std::vector<size_t> off((size_t)R + 1, 0);
  for (int k = 0; k < R; ++k) off[(size_t)k + 1] = off[(size_t)k] + (k == root ? 0 : (size_t)sz[(size_t)k]);
  if (me == root && off[(size_t)R] > 0) {
    HIP_TRY(sendb.ensure(off[(size_t)R]));
    for (int k = 0; k < R; ++k)
      if (k != root && sz[(size_t)k])
        HIP_TRY(hipMemcpyAsync(sendb.as<char>() + off[(size_t)k], blobs[k], sz[(size_t)k], hipMemcpyHostToDevice, c->stream));
  }
  if (me != root && sz[(size_t)me]) HIP_TRY(recvb.ensure(sz[(size_t)me]));
  NCCL_TRY(r.group_start());
  if (me == root) {
    for (int k = 0; k < R; ++k)
      if (k != root && sz[(size_t)k]) NCCL_TRY(r.send(sendb.as<char>() + off[(size_t)k], sz[(size_t)k], ncclUint8, k, c->comm, c->stream));
  } else if (sz[(size_t)me]) {
    NCCL_TRY(r.recv(recvb.p, sz[(size_t)me], ncclUint8, root, c->comm, c->stream));
  }
  NCCL_TRY(r.group_end());
  std::vector<unsigned char> mine;
  if (me != root && sz[(size_t)me]) {
    mine.resize(sz[(size_t)me]);
    HIP_TRY(hipMemcpyAsync(mine.data(), recvb.p, mine.size(), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (me == root) return gicp_set_tie_tree(c, blobs[root], sizes[root]);
  return gicp_set_tie_tree(c, mine.data(), mine.size());
}

}  // extern "C"
