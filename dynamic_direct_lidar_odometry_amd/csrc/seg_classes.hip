// seg_classes.hip — the class of every pixel of the last scan and what is
// read off it: counts, index sets, the frame's four clouds
// (include/ddlo_seg_classes.h).
//
// The class image is one byte per pixel, padded to a whole 32-bit word:
//   k_cls_base    writes every byte (the padding: 0): VALID from the scan in
//                 the handle's raw buffer, GROUND from the device ground image
//                 within the bottom ground_rows rows;
//   k_cls_paint   grid (chunks, tracks) as k_trk_drop: every pool entry of a
//                 track ORs the track's status bit into its pixel's byte, as
//                 an integer atomicOr (agent scope) on the word the byte lies
//                 in.  Two lists that share a pixel, or two pixels that share
//                 a word, only ever add bits: whichever lands first, the word
//                 ends the same.
//   k_cls_count / k_cls_count_sum   per-workgroup counts by ballot and
//                 popcount, then one workgroup adds the partials in index
//                 order.  (One same-address counter atomic per wavefront is
//                 what DESIGN.md §11 measured and dropped.)
// Sets and clouds: k_cls_part_count / _scan / _write, a stable partition of
// the pixels into up to four overlapping selections.  A selection is three
// masks over the class byte: (b & any) != 0, (b & none) == 0, (b & must) ==
// must.  A workgroup is 256 consecutive pixels, a wavefront 64 of them, so
// offset[workgroup] + sum of the earlier wavefronts + popcount of the lower
// lanes' ballot bits is the pixel's rank in ascending pixel order, whatever
// the grid.  No atomics.
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

constexpr int kClsThreads = 256;
constexpr int kClsWaves = kClsThreads / 64;
constexpr int kClsMaxTracks = 65535;   // gridDim.y
constexpr int kClsCounts = 8;          // ints of one workgroup's partial counts (7 used)
constexpr int kClsSels = 4;

struct ClsBaseArgs {
  const unsigned char* raw;
  size_t stride;
  const signed char* ground;
  int npix, npad;
  int first_ground;   // first pixel of the bottom ground_rows rows
  unsigned char* img;
};

__global__ __launch_bounds__(kClsThreads) void k_cls_base(ClsBaseArgs a) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.npad) return;
  unsigned b = 0;
  if (p < a.npix) {
    const float* q = reinterpret_cast<const float*>(a.raw + (size_t)p * a.stride);
    if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) b |= DDLO_CLS_VALID;
    if (p >= a.first_ground && a.ground[p] == 1) b |= DDLO_CLS_GROUND;
  }
  a.img[p] = (unsigned char)b;
}

// one track: its pool range and its status bit
struct ClsTrack {
  int off, len, bit, pad;
};

__global__ __launch_bounds__(kClsThreads) void k_cls_paint(const ClsTrack* __restrict__ table,
                                                           const int* __restrict__ pool, unsigned* __restrict__ words,
                                                           int npix) {
  const ClsTrack e = table[blockIdx.y];   // (uniform)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < e.len; i += gridDim.x * blockDim.x) {
    const int p = pool[e.off + i];
    if ((unsigned)p < (unsigned)npix) atomicOr(&words[p >> 2], (unsigned)e.bit << (8 * (p & 3)));
  }
}

__global__ __launch_bounds__(kClsThreads) void k_cls_count(const unsigned char* __restrict__ img, int npix,
                                                           int* __restrict__ partial) {
  __shared__ int sh[kClsWaves][kClsCounts];
  const int p = blockIdx.x * kClsThreads + threadIdx.x;
  const unsigned b = p < npix ? img[p] : 0u;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool ns = (b & DDLO_CLS_NON_STATIC) != 0;
  const bool f[7] = {(b & DDLO_CLS_VALID) != 0,  (b & DDLO_CLS_GROUND) != 0,  (b & DDLO_CLS_UNDEFINED) != 0,
                     (b & DDLO_CLS_STATIC) != 0, (b & DDLO_CLS_DYNAMIC) != 0, ns,
                     (b & DDLO_CLS_VALID) != 0 && !ns};
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const int c = __popcll(__ballot(f[k]));
    if (lane == 0) sh[w][k] = c;
  }
  __syncthreads();
  if (threadIdx.x < kClsCounts) {
    int s = 0;
    if (threadIdx.x < 7)
      for (int j = 0; j < kClsWaves; ++j) s += sh[j][threadIdx.x];
    partial[blockIdx.x * kClsCounts + threadIdx.x] = s;
  }
}

// one workgroup: thread t adds count t % 8 of the workgroups t / 8, t / 8 + 32, ...; thread k < 8 then adds the 32 sums
__global__ __launch_bounds__(kClsThreads) void k_cls_count_sum(const int* __restrict__ partial, int nwg,
                                                               int* __restrict__ out) {
  __shared__ int sh[kClsThreads];
  const int k = threadIdx.x % kClsCounts;
  int s = 0;
  for (int g = threadIdx.x / kClsCounts; g < nwg; g += kClsThreads / kClsCounts) s += partial[g * kClsCounts + k];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < kClsCounts) {
    int t = 0;
    for (int j = 0; j < kClsThreads / kClsCounts; ++j) t += sh[j * kClsCounts + threadIdx.x];
    out[threadIdx.x] = t;
  }
}

struct ClsSel {
  unsigned any, none, must;
};
struct ClsSelSet {
  ClsSel s[kClsSels];
  int n;
};

__device__ __forceinline__ bool cls_member(unsigned b, const ClsSel& s) {
  return (b & s.any) != 0 && (b & s.none) == 0 && (b & s.must) == s.must;
}

// 1. counts[workgroup][selection]
__global__ __launch_bounds__(kClsThreads) void k_cls_part_count(const unsigned char* __restrict__ img, int npix,
                                                                ClsSelSet sel, int* __restrict__ counts) {
  __shared__ int sh[kClsWaves][kClsSels];
  const int p = blockIdx.x * kClsThreads + threadIdx.x;
  const unsigned b = p < npix ? img[p] : 0u;   // (a byte past the image is in no selection: any != 0 needs a bit)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < kClsSels; ++c) {
    const int m = __popcll(__ballot(c < sel.n && p < npix && cls_member(b, sel.s[c])));
    if (lane == 0) sh[w][c] = m;
  }
  __syncthreads();
  if (threadIdx.x < kClsSels) {
    int s = 0;
    for (int j = 0; j < kClsWaves; ++j) s += sh[j][threadIdx.x];
    counts[blockIdx.x * kClsSels + threadIdx.x] = s;
  }
}

// 2. one workgroup, wavefront c scans selection c's column: offs = exclusive sums, totals[c] = the sum
__global__ __launch_bounds__(kClsThreads) void k_cls_part_scan(const int* __restrict__ counts, int nwg,
                                                               int* __restrict__ offs, int* __restrict__ totals) {
  const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;   // kClsWaves == kClsSels
  int carry = 0;
  for (int base = 0; base < nwg; base += 64) {   // (uniform in the wavefront)
    const int i = base + lane;
    const int v = i < nwg ? counts[i * kClsSels + c] : 0;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    if (i < nwg) offs[i * kClsSels + c] = carry + incl - v;
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0) totals[c] = carry;
}
static_assert(kClsWaves == kClsSels, "k_cls_part_scan gives one wavefront to every selection");

// 3. every member at offs + the earlier wavefronts' members + its ballot prefix:
// kIds: the pixel index into ids[c * cap ..]; else the point into pts[c * cap ..]
template <bool kIds>
__global__ __launch_bounds__(kClsThreads) void k_cls_part_write(const unsigned char* __restrict__ img, int npix,
                                                                ClsSelSet sel, const int* __restrict__ offs,
                                                                const unsigned char* __restrict__ raw, size_t stride,
                                                                float4* __restrict__ pts, int* __restrict__ ids,
                                                                int cap) {
  __shared__ int sh[kClsWaves][kClsSels];
  const int p = blockIdx.x * kClsThreads + threadIdx.x;
  const unsigned b = p < npix ? img[p] : 0u;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  bool in[kClsSels];
  int rank[kClsSels];
#pragma unroll
  for (int c = 0; c < kClsSels; ++c) {
    in[c] = c < sel.n && p < npix && cls_member(b, sel.s[c]);
    const unsigned long long m = __ballot(in[c]);
    rank[c] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) sh[w][c] = __popcll(m);
  }
  __syncthreads();
  float4 pt = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!kIds && p < npix) {
    const float* q = reinterpret_cast<const float*>(raw + (size_t)p * stride);
    pt = make_float4(q[0], q[1], q[2], 0.f);
  }
#pragma unroll
  for (int c = 0; c < kClsSels; ++c) {
    if (!in[c]) continue;
    int at = offs[blockIdx.x * kClsSels + c] + rank[c];
    for (int j = 0; j < w; ++j) at += sh[j][c];
    if ((unsigned)at >= (unsigned)cap) continue;   // (never: a selection has at most npix <= cap members)
    if (kIds) ids[(size_t)c * cap + at] = p;
    else pts[(size_t)c * cap + at] = pt;
  }
}

int chunks_for(int maxlen) {
  return std::max(1, std::min(16, (maxlen + 4 * kClsThreads - 1) / (4 * kClsThreads)));
}

// the clouds' selections, in ddlo_seg_frame_clouds_out's order
const ClsSelSet kCloudSels = {{{DDLO_CLS_GROUND, 0, DDLO_CLS_VALID},
                               {DDLO_CLS_NON_STATIC, 0, DDLO_CLS_VALID},
                               {DDLO_CLS_DYNAMIC, 0, DDLO_CLS_VALID},
                               {DDLO_CLS_VALID, DDLO_CLS_NON_STATIC, 0}},
                              4};

}  // namespace

struct SegClasses {
  DevBuf img, table, partial, counts, pcount, poffs, totals, clouds, ids;
  rt::PinBuf pin_table;            // pinned staging of the tracks' table
  rt::PinBuf pin_back;             // pinned: counts (8 ints), then totals (4 ints)
  bool have_img = false;
  unsigned long long serial = 0;   // the scan the image belongs to
  bool have_clouds = false;
  int cloud_n[kClsSels] = {0, 0, 0, 0};

  // room for the table of `tracks` tracks (doubled, 64 at least), and the read-back block
  gicp_status stage(size_t tracks) {
    if (!pin_back.p) HIP_TRY(pin_back.reset(sizeof(int) * 16));
    if (sizeof(ClsTrack) * tracks <= pin_table.bytes) return GICP_OK;
    HIP_TRY(pin_table.reset(sizeof(ClsTrack) * std::max<size_t>(2 * tracks, 64)));
    return GICP_OK;
  }
};

void SegPartFree::operator()(SegClasses* c) const { delete c; }

namespace {

int workgroups(int npix) { return (npix + kClsThreads - 1) / kClsThreads; }

// the class image of the last scan, or GICP_EINVAL
gicp_status current(ddlo_seg* s, SegClasses** c) {
  if (!s->have) return fail(GICP_EINVAL, "no processed scan");
  *c = s->classes.get();
  if (!*c || !(*c)->have_img || (*c)->serial != s->scan_serial)
    return fail(GICP_EINVAL, "the last scan is not classified (ddlo_seg_classify)");
  HIP_TRY(hipSetDevice(s->device));
  return GICP_OK;
}

// the three-step partition over c->img; the totals reach pin_back[8 ..] with the stream's next wait
template <bool kIds>
gicp_status partition(const ddlo_seg* s, SegClasses* c, const ClsSelSet& sel) {
  const int npix = s->p.rows * s->p.cols, nwg = workgroups(npix);
  const hipStream_t stream = s->s;
  HIP_TRY(c->pcount.ensure(sizeof(int) * kClsSels * (size_t)nwg));
  HIP_TRY(c->poffs.ensure(sizeof(int) * kClsSels * (size_t)nwg));
  HIP_TRY(c->totals.ensure(sizeof(int) * kClsSels));
  if (kIds) HIP_TRY(c->ids.ensure(sizeof(int) * (size_t)npix * (size_t)sel.n));
  else HIP_TRY(c->clouds.ensure(sizeof(float4) * (size_t)npix * (size_t)sel.n));
  k_cls_part_count<<<nwg, kClsThreads, 0, stream>>>(c->img.as<unsigned char>(), npix, sel, c->pcount.as<int>());
  k_cls_part_scan<<<1, kClsThreads, 0, stream>>>(c->pcount.as<int>(), nwg, c->poffs.as<int>(), c->totals.as<int>());
  k_cls_part_write<kIds><<<nwg, kClsThreads, 0, stream>>>(c->img.as<unsigned char>(), npix, sel, c->poffs.as<int>(),
                                                         s->raw.as<unsigned char>(), s->raw_stride,
                                                         c->clouds.as<float4>(), c->ids.as<int>(), npix);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->pin_back.as<int>() + 8, c->totals.p, sizeof(int) * kClsSels, hipMemcpyDeviceToHost, stream));
  return GICP_OK;
}

gicp_status ensure_clouds(const ddlo_seg* s, SegClasses* c) {
  if (c->have_clouds) return GICP_OK;
  if (gicp_status st = partition<false>(s, c, kCloudSels)) return st;
  HIP_TRY(hipStreamSynchronize(s->s));
  for (int k = 0; k < kClsSels; ++k) c->cloud_n[k] = c->pin_back.as<int>()[8 + k];
  c->have_clouds = true;
  return GICP_OK;
}

}  // namespace

gicp_status seg_frame_clouds_dev(ddlo_seg* s, const float4* pts[4], int count[4]) {
  if (!s || !pts || !count) return fail(GICP_EINVAL, "null argument");
  SegClasses* c = nullptr;
  if (gicp_status st = current(s, &c)) return st;
  if (gicp_status st = ensure_clouds(s, c)) return st;
  const size_t npix = (size_t)s->p.rows * s->p.cols;
  for (int k = 0; k < kClsSels; ++k) {
    pts[k] = c->clouds.as<float4>() + npix * k;
    count[k] = c->cloud_n[k];
  }
  return GICP_OK;
}

gicp_status seg_class_image_dev(ddlo_seg* s, const unsigned char** img) {
  if (!s || !img) return fail(GICP_EINVAL, "null argument");
  SegClasses* c = nullptr;
  if (gicp_status st = current(s, &c)) return st;
  *img = c->img.as<unsigned char>();
  return GICP_OK;
}

}  // namespace ddlo

using namespace ddlo;

extern "C" {

gicp_status ddlo_seg_classify(ddlo_seg* s, const int32_t* track_ids, const int32_t* statuses, size_t n,
                              ddlo_seg_class_counts* counts) {
  if (!s || (n && (!track_ids || !statuses))) return fail(GICP_EINVAL, "invalid argument");
  if (!s->have) return fail(GICP_EINVAL, "no processed scan");
  if (n > (size_t)kClsMaxTracks) return fail(GICP_EINVAL, "too many tracks");
  for (size_t i = 0; i < n; ++i) {
    if (statuses[i] < 0 || statuses[i] > 2) return fail(GICP_EINVAL, "a status is not 0, 1 or 2");
    for (size_t j = 0; j < i; ++j)
      if (track_ids[j] == track_ids[i]) return fail(GICP_EINVAL, "a track id is named twice");
  }
  std::vector<int2> ranges;
  const int* pool = nullptr;
  if (gicp_status st = seg_tracks_ranges(s, track_ids, n, &ranges, &pool)) return st;
  // valid: from here on the image is rewritten
  HIP_TRY(hipSetDevice(s->device));
  if (!s->classes) s->classes.reset(new SegClasses());
  SegClasses* const c = s->classes.get();
  const hipStream_t stream = s->s;
  const int npix = s->p.rows * s->p.cols, npad = (npix + 3) / 4 * 4, nwg = workgroups(npix);
  std::vector<ClsTrack> table;
  int maxlen = 0;
  for (size_t i = 0; i < n; ++i) {
    if (ranges[i].y <= 0) continue;
    table.push_back(ClsTrack{ranges[i].x, ranges[i].y, DDLO_CLS_UNDEFINED << statuses[i], 0});
    maxlen = std::max(maxlen, ranges[i].y);
  }
  if (gicp_status st = c->stage(table.size())) return st;
  HIP_TRY(c->img.ensure((size_t)npad));
  c->have_img = false;
  c->have_clouds = false;
  ClsBaseArgs a{s->raw.as<unsigned char>(), s->raw_stride, s->ground.as<signed char>(), npix, npad,
                (s->p.rows - s->p.ground_rows) * s->p.cols, c->img.as<unsigned char>()};
  k_cls_base<<<(npad + kClsThreads - 1) / kClsThreads, kClsThreads, 0, stream>>>(a);
  if (!table.empty() && pool) {
    const size_t tb = sizeof(ClsTrack) * table.size();
    HIP_TRY(c->table.ensure(tb));
    std::memcpy(c->pin_table.p, table.data(), tb);
    HIP_TRY(hipMemcpyAsync(c->table.p, c->pin_table.p, tb, hipMemcpyHostToDevice, stream));
    k_cls_paint<<<dim3(chunks_for(maxlen), (unsigned)table.size()), kClsThreads, 0, stream>>>(
        c->table.as<ClsTrack>(), pool, c->img.as<unsigned>(), npix);
  }
  if (counts) {
    HIP_TRY(c->partial.ensure(sizeof(int) * kClsCounts * (size_t)nwg));
    HIP_TRY(c->counts.ensure(sizeof(int) * kClsCounts));
    k_cls_count<<<nwg, kClsThreads, 0, stream>>>(c->img.as<unsigned char>(), npix, c->partial.as<int>());
    k_cls_count_sum<<<1, kClsThreads, 0, stream>>>(c->partial.as<int>(), nwg, c->counts.as<int>());
    HIP_TRY(hipMemcpyAsync(c->pin_back.p, c->counts.p, sizeof(int) * kClsCounts, hipMemcpyDeviceToHost, stream));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(stream));   // the staged table is free again; the image is complete
  c->have_img = true;
  c->serial = s->scan_serial;
  if (counts) {
    const int* b = c->pin_back.as<int>();
    *counts = ddlo_seg_class_counts{b[0], b[1], b[2], b[3], b[4], b[5], b[6], 0};
  }
  return GICP_OK;
}

gicp_status ddlo_seg_class_image(ddlo_seg* s, uint8_t* img) {
  if (!s || !img) return fail(GICP_EINVAL, "invalid argument");
  SegClasses* c = nullptr;
  if (gicp_status st = current(s, &c)) return st;
  HIP_TRY(hipMemcpyAsync(img, c->img.p, (size_t)s->p.rows * s->p.cols, hipMemcpyDeviceToHost, s->s));
  HIP_TRY(hipStreamSynchronize(s->s));
  return GICP_OK;
}

gicp_status ddlo_seg_class_indices(ddlo_seg* s, int any, int none, int32_t* out, size_t cap, size_t* n) {
  if (!s || !n || (!out && cap)) return fail(GICP_EINVAL, "invalid argument");
  if ((any & ~0xff) || (none & ~0xff)) return fail(GICP_EINVAL, "any and none are masks over the class byte");
  SegClasses* c = nullptr;
  if (gicp_status st = current(s, &c)) return st;
  const ClsSelSet sel = {{{(unsigned)any, (unsigned)none, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, 1};
  if (gicp_status st = partition<true>(s, c, sel)) return st;
  HIP_TRY(hipStreamSynchronize(s->s));
  const size_t m = (size_t)c->pin_back.as<int>()[8];
  *n = m;
  const size_t k = std::min(m, cap);
  if (!out || k == 0) return GICP_OK;
  HIP_TRY(hipMemcpyAsync(out, c->ids.p, sizeof(int32_t) * k, hipMemcpyDeviceToHost, s->s));
  HIP_TRY(hipStreamSynchronize(s->s));
  return GICP_OK;
}

gicp_status ddlo_seg_frame_clouds(ddlo_seg* s, ddlo_seg_frame_clouds_out* out) {
  if (!s || !out) return fail(GICP_EINVAL, "invalid argument");
  SegClasses* c = nullptr;
  if (gicp_status st = current(s, &c)) return st;
  if (gicp_status st = ensure_clouds(s, c)) return st;
  ddlo_seg_cloud_out* const o[kClsSels] = {&out->ground, &out->non_static, &out->dynamic, &out->static_points};
  for (int k = 0; k < kClsSels; ++k) {
    o[k]->n = (size_t)c->cloud_n[k];
    if (o[k]->xyz && o[k]->cap < o[k]->n) return fail(GICP_EINVAL, "output capacity too small");
  }
  const size_t npix = (size_t)s->p.rows * s->p.cols;
  for (int k = 0; k < kClsSels; ++k) {
    if (!o[k]->xyz || o[k]->n == 0) continue;
    if (gicp_status st = rt::read_xyz(s->s, c->clouds.as<float4>() + npix * k, o[k]->n, o[k]->xyz)) return st;
  }
  return GICP_OK;
}

}  // extern "C"
