// seg_tracks.hip — the tracks' pixel lists on the device
// (include/ddlo_seg_tracks.h).
//
// A filter keeps the pixel indices of the scan it last matched
// (bounding_box_filter.cpp:69,133-136) and the scan loses the union of the
// non-static filters' indices (odom.cc:867-892, tracking.cpp:192-208).  The
// lists stay on the device, in a pool of two int buffers that swap:
//   k_trk_gather  one launch builds the next pool from a host-built table with
//                 one entry per live track: the source (the old pool at an
//                 offset, or a segment of the current scan's CSR, whose offset
//                 the kernel reads from the device CSR itself), the length and
//                 the destination offset.  The host knows every length (the
//                 old table, or the segments' lengths), so the destination
//                 offsets are a host prefix sum: no atomic, no scan.  Several
//                 workgroups copy one entry (grid (chunks, entries), as
//                 k_lbl_drop); consecutive threads read and write consecutive
//                 ints.
//   k_trk_drop    NaN over the pixels the removed tracks list in the packed
//                 float4 scan, per removed track over its pool range.
// The buffer written is always the one not in use, so growing it needs no
// copy: it is reallocated (geometrically) before the gather fills it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ddlo_segment.h"
#include "runtime.hpp"
#include "seg_state.hpp"

namespace ddlo {

namespace {

using rt::DevBuf;
using rt::fail;

constexpr int kTrkThreads = 256;
constexpr size_t kTrkInitialCap = 4096;   // indices; the pool doubles from here
constexpr int kTrkMaxEntries = 65535;     // gridDim.y

// one list of the next pool
struct TrkEntry {
  int src;   // >= 0: offset in the old pool; < 0: segment -src of the current CSR
  int len;
  int dst;   // offset in the next pool
  int pad;
};

__global__ __launch_bounds__(kTrkThreads) void k_trk_gather(const TrkEntry* __restrict__ table,
                                                            const int* __restrict__ old_pool,
                                                            const int* __restrict__ csr_off,
                                                            const int* __restrict__ csr_pix, int* __restrict__ next) {
  const TrkEntry e = table[blockIdx.y];   // (uniform)
  const int* src;
  int len = e.len;
  if (e.src >= 0) {
    src = old_pool + e.src;
  } else {
    const int b = csr_off[-e.src];
    src = csr_pix + b;
    len = min(len, csr_off[-e.src + 1] - b);   // (equal by construction: never read past the segment)
  }
  int* const dst = next + e.dst;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

// A pixel can be in several removed lists (a stale list and the current
// one of another track overlap where an object stood still): every writer
// stores the same bits, (NaN, NaN, NaN, kRemovedW: the removed flag of the
// row/column filter's keyframe pass), so the result does not depend on which
// store lands last.  Neither atomics nor a pass that removes duplicates.
// FLAGS (seg_removed_flags: w is the intensity): the flag is a byte of the pixel's, 1 from every writer.
template <bool FLAGS>
__global__ __launch_bounds__(kTrkThreads) void k_trk_drop(const int2* __restrict__ ranges,
                                                          const int* __restrict__ pool, float4* __restrict__ pts,
                                                          int npix, unsigned char* __restrict__ flags) {
  const int2 r = ranges[blockIdx.y];   // (offset, length)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < r.y; i += gridDim.x * blockDim.x) {
    const int p = pool[r.x + i];
    if ((unsigned)p < (unsigned)npix) {
      pts[p] = make_float4(NAN, NAN, NAN, FLAGS ? 0.f : kRemovedW);
      if (FLAGS) flags[p] = 1;
    }
  }
}

int chunks_for(int maxlen) { return std::max(1, std::min(16, (maxlen + 4 * kTrkThreads - 1) / (4 * kTrkThreads))); }

struct Live {
  int id, off, len;
};

}  // namespace

struct SegTracks {
  DevBuf pool[2];
  size_t cap[2] = {0, 0};   // indices
  int cur = 0;
  size_t used = 0;
  std::vector<Live> live;   // in pool order
  DevBuf dtable;
  rt::PinBuf stage;         // pinned staging of the table / the ranges

  const Live* find(int id) const {
    for (const Live& l : live)
      if (l.id == id) return &l;
    return nullptr;
  }
};

void SegPartFree::operator()(SegTracks* t) const { delete t; }

namespace {

const Live* find_list(const ddlo_seg* s, int id) { return s->tracks ? s->tracks->find(id) : nullptr; }

gicp_status tracks_sync(ddlo_seg* s, const int32_t* track_ids, const int32_t* seg_ids, size_t n_set,
                        const int32_t* dead_ids, size_t n_dead) {
  if (!s || (n_set && (!track_ids || !seg_ids)) || (n_dead && !dead_ids)) return fail(GICP_EINVAL, "invalid argument");
  if (n_set && !s->have) return fail(GICP_EINVAL, "no processed scan");
  const int segments = s->have ? s->last.segments : 0;
  for (size_t i = 0; i < n_set; ++i) {
    if (seg_ids[i] < 1 || seg_ids[i] > segments) return fail(GICP_EINVAL, "seg_ids names no segment of the last scan");
    for (size_t j = 0; j < i; ++j)
      if (track_ids[j] == track_ids[i]) return fail(GICP_EINVAL, "a track id is set twice");
  }
  for (size_t i = 0; i < n_dead; ++i) {
    if (!find_list(s, dead_ids[i])) return fail(GICP_EINVAL, "a dead track holds no list");
    for (size_t j = 0; j < i; ++j)
      if (dead_ids[j] == dead_ids[i]) return fail(GICP_EINVAL, "a dead track is named twice");
  }
  if (n_set == 0 && n_dead == 0) return GICP_OK;   // nothing moves: no launch
  SegCsr csr;   // (only now: an invalid call does no device work)
  if (n_set)
    if (gicp_status st = seg_csr(s, &csr)) return st;
  HIP_TRY(hipSetDevice(s->device));
  if (!s->tracks) s->tracks.reset(new SegTracks());
  SegTracks* const t = s->tracks.get();
  // the next pool: the survivors in their order, then the lists set now
  std::vector<Live> next;
  std::vector<TrkEntry> table;
  size_t total = 0;
  int maxlen = 0;
  auto add = [&](int id, int src, int len) {
    next.push_back(Live{id, (int)total, len});
    table.push_back(TrkEntry{src, len, (int)total, 0});
    total += (size_t)len;
    maxlen = std::max(maxlen, len);
  };
  for (const Live& l : t->live) {
    bool gone = false;
    for (size_t i = 0; i < n_dead && !gone; ++i) gone = dead_ids[i] == l.id;
    for (size_t i = 0; i < n_set && !gone; ++i) gone = track_ids[i] == l.id;
    if (!gone) add(l.id, l.off, l.len);
  }
  for (size_t i = 0; i < n_set; ++i) add(track_ids[i], -seg_ids[i], csr.len[seg_ids[i]]);
  if (total > (size_t)INT32_MAX / 2 || table.size() > (size_t)kTrkMaxEntries)
    return fail(GICP_EINVAL, "too many track indices");
  const int nxt = t->cur ^ 1;
  if (total > t->cap[nxt]) {   // (its contents are of no use: the gather rewrites it)
    size_t c = std::max(kTrkInitialCap, std::max(t->cap[0], t->cap[1]));
    while (c < total) c *= 2;
    HIP_TRY(t->pool[nxt].ensure(sizeof(int) * c));
    t->cap[nxt] = c;
  }
  if (!table.empty() && total > 0) {
    const size_t tb = sizeof(TrkEntry) * table.size();
    HIP_TRY(t->stage.ensure(tb));
    HIP_TRY(t->dtable.ensure(tb));
    std::memcpy(t->stage.p, table.data(), tb);
    HIP_TRY(hipMemcpyAsync(t->dtable.p, t->stage.p, tb, hipMemcpyHostToDevice, s->s));
    k_trk_gather<<<dim3(chunks_for(maxlen), (unsigned)table.size()), kTrkThreads, 0, s->s>>>(
        t->dtable.as<TrkEntry>(), t->pool[t->cur].as<int>(), csr.d_off, csr.d_pix, t->pool[nxt].as<int>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->s));   // the stagings and the old pool are free again
  }
  t->cur = nxt;
  t->used = total;
  t->live.swap(next);
  return GICP_OK;
}

}  // namespace

gicp_status seg_tracks_ranges(ddlo_seg* s, const int32_t* track_ids, size_t n, std::vector<int2>* ranges,
                              const int** pool) {
  if (!s || !ranges || !pool || (n && !track_ids)) return fail(GICP_EINVAL, "invalid argument");
  ranges->clear();
  for (size_t i = 0; i < n; ++i) {
    const Live* l = find_list(s, track_ids[i]);
    if (!l) return fail(GICP_EINVAL, "a track to classify holds no list");
    ranges->push_back(make_int2(l->off, l->len));
  }
  *pool = s->tracks ? s->tracks->pool[s->tracks->cur].as<int>() : nullptr;
  return GICP_OK;
}

// the removal by track list: NaN over every pixel the removed tracks list
gicp_status seg_static_cloud_tracks_dev(ddlo_seg* s, const int32_t* track_ids, size_t n, const float centre[3],
                                        double crop_size, double leaf, const float4** pts, int* count,
                                        int64_t* dropped) {
  if (!s || (n && !track_ids)) return fail(GICP_EINVAL, "invalid argument");
  std::vector<int2> ranges;
  int maxlen = 0;
  int64_t sum = 0;
  for (size_t i = 0; i < n; ++i) {
    const Live* l = find_list(s, track_ids[i]);
    if (!l) return fail(GICP_EINVAL, "a track to remove holds no list");
    if (l->len > 0) ranges.push_back(make_int2(l->off, l->len));
    maxlen = std::max(maxlen, l->len);
    sum += l->len;
  }
  if (ranges.size() > (size_t)kTrkMaxEntries) return fail(GICP_EINVAL, "too many tracks to remove");
  if (dropped) *dropped = sum;
  if (gicp_status st = seg_static_begin(s, centre, pts, count)) return st;
  if (!ranges.empty()) {
    SegTracks* const t = s->tracks.get();   // (a list was found: the part exists)
    const size_t rb = sizeof(int2) * ranges.size();
    HIP_TRY(t->stage.ensure(rb));
    HIP_TRY(t->dtable.ensure(rb));
    std::memcpy(t->stage.p, ranges.data(), rb);
    HIP_TRY(hipMemcpyAsync(t->dtable.p, t->stage.p, rb, hipMemcpyHostToDevice, s->s));
    const dim3 grid(chunks_for(maxlen), (unsigned)ranges.size());
    if (unsigned char* const flags = seg_removed_flags(s))
      k_trk_drop<true><<<grid, kTrkThreads, 0, s->s>>>(t->dtable.as<int2>(), t->pool[t->cur].as<int>(),
                                                        s->f4.as<float4>(), (int)s->hn, flags);
    else
      k_trk_drop<false><<<grid, kTrkThreads, 0, s->s>>>(t->dtable.as<int2>(), t->pool[t->cur].as<int>(),
                                                         s->f4.as<float4>(), (int)s->hn, nullptr);
    HIP_TRY(hipGetLastError());
  }
  return seg_static_finish(s, centre, crop_size, leaf, pts, count);   // (waits for the stream)
}

}  // namespace ddlo

using namespace ddlo;

extern "C" {

gicp_status ddlo_seg_tracks_sync(ddlo_seg* s, const int32_t* track_ids, const int32_t* seg_ids, size_t n_set,
                                 const int32_t* dead_ids, size_t n_dead) {
  return tracks_sync(s, track_ids, seg_ids, n_set, dead_ids, n_dead);
}

gicp_status ddlo_seg_static_cloud_tracks(ddlo_seg* s, const int32_t* track_ids, size_t n, const float centre[3],
                                         double crop_size, double leaf, float* out, size_t cap, size_t* nout) {
  if (!nout || (!out && cap)) return fail(GICP_EINVAL, "invalid argument");
  const float4* pts = nullptr;
  int m = 0;
  gicp_status st = seg_static_cloud_tracks_dev(s, track_ids, n, centre, crop_size, leaf, &pts, &m, nullptr);
  if (st) return st;
  *nout = (size_t)m;
  if (!out || m == 0) return GICP_OK;
  if ((size_t)m > cap) return fail(GICP_EINVAL, "output capacity too small");
  return rt::read_xyz(s->s, pts, (size_t)m, out);
}

gicp_status ddlo_seg_track_indices(ddlo_seg* s, int32_t track_id, int32_t* out, size_t cap, size_t* n) {
  if (!s || !n || (!out && cap)) return fail(GICP_EINVAL, "invalid argument");
  const Live* l = find_list(s, track_id);
  if (!l) return fail(GICP_EINVAL, "the track holds no list");
  *n = (size_t)l->len;
  if (!out || l->len == 0) return GICP_OK;
  HIP_TRY(hipSetDevice(s->device));
  std::vector<int32_t> h((size_t)l->len);
  HIP_TRY(hipMemcpyAsync(h.data(), s->tracks->pool[s->tracks->cur].as<int>() + l->off, sizeof(int) * h.size(),
                         hipMemcpyDeviceToHost, s->s));
  HIP_TRY(hipStreamSynchronize(s->s));
  // ddlo_seg_label_indices' order is ascending row-major index; the host
  // labelling's lists reach the device in its push order
  std::sort(h.begin(), h.end());
  for (size_t i = 0; i < h.size() && i < cap; ++i) out[i] = h[i];
  return GICP_OK;
}

gicp_status ddlo_seg_tracks_stats(const ddlo_seg* s, int32_t* lists, int64_t* indices, int64_t* capacity) {
  if (!s) return fail(GICP_EINVAL, "null handle");
  const SegTracks* t = s->tracks.get();
  if (lists) *lists = t ? (int32_t)t->live.size() : 0;
  if (indices) *indices = t ? (int64_t)t->used : 0;
  if (capacity) *capacity = t ? (int64_t)t->cap[t->cur] : 0;
  return GICP_OK;
}

}  // extern "C"
