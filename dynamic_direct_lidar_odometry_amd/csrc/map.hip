// map.hip — the global map on the device (include/ddlo_map.h): MapNode of
// the reference (dynamic_direct_lidar_odometry/src/odometry/map.cc) with its
// cloud in device memory.
//   keyframeCB        :101-117   add_points(): voxel filter of the keyframe
//                                (preprocess.hip) straight into the map's tail
//   dynamicObjectsCB  :133-156   ddlo_map_clear_boxes(): k_map_box_flags +
//                                the order-keeping compaction of preprocess.hip
//   savePcd           :158-189   export(): the voxelised copy, read back and
//                                written by the host
// The reference removes the boxes one at a time, one negative pcl::CropBox
// pass over the whole map (and one copy of it) per box.  A point survives
// that loop exactly when it is outside every box, so here the boxes become
// packed records, one kernel flags every point against all of them and one
// compaction keeps the survivors' order.
//
// Compiled with -ffp-contract=off: the box test's float operation order is
// the one stated in ddlo_map.h and restated in tests/map_ref.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ddlo_map.h"
#include "gicp_types.hpp"
#include "launch.hpp"
#include "runtime.hpp"
#include "devknobs.hpp"
#include "odom_internal.hpp"

namespace ddlo {

// boxes staged per pass over the block's LDS list
constexpr int kBoxChunk = 512;
constexpr int kMapInitialCapacity = 16384;   // points (ddlo_map.h states it)
constexpr int kNoCullBoxes = 4;              // at most this many boxes: no block-level cull

// One box on the device: aabb[2 b], aabb[2 b + 1] = its world-frame bounds
// (conservative, low / high corner); rec[3 b .. 3 b + 2] = what the point
// test reads:
//   rec[0] = centre x, y, z, c = cosf(yaw)
//   rec[1] = s = sinf(yaw), min x, y, z
//   rec[2] = max x, y, z, 1.f if yaw != 0 (else the rotation is skipped)

// keep[i] = 1 if point i is finite and outside every box.  One thread per
// point; the workgroup's 256 consecutive points (a thin strip of one
// keyframe's voxel order) share a bounding box, and only the boxes whose
// world bounds meet it are kept in LDS for the per-point test.  CULL = false
// (a handful of boxes; development, DDLO_MAP_NO_CULL): every box is kept.
// The flags are the same either way.
template <bool CULL>
__global__ __launch_bounds__(256) void k_map_box_flags(const float4* __restrict__ pts, int n,
                                                       const float4* __restrict__ aabb,
                                                       const float4* __restrict__ rec, int nb,
                                                       int* __restrict__ keep) {
  __shared__ float4 s_rec[kBoxChunk * 3];
  __shared__ float s_red[4][6];
  __shared__ int s_cnt[2][4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long long i = (long long)blockIdx.x * 256 + t;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  bool finite = false;
  if (i < n) {
    p = pts[i];
    finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
  }
  // the block's bounds: wavefront shuffles, then the four wavefronts' rows
  float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (CULL) {
    if (finite) {
      blo[0] = bhi[0] = p.x;
      blo[1] = bhi[1] = p.y;
      blo[2] = bhi[2] = p.z;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        blo[a] = fminf(blo[a], __shfl_xor(blo[a], d));
        bhi[a] = fmaxf(bhi[a], __shfl_xor(bhi[a], d));
      }
    if (lane == 0)
      for (int a = 0; a < 3; ++a) {
        s_red[w][a] = blo[a];
        s_red[w][3 + a] = bhi[a];
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        blo[a] = fminf(blo[a], s_red[k][a]);
        bhi[a] = fmaxf(bhi[a], s_red[k][3 + a]);
      }
  }
  bool hit = false;   // inside some box
  for (int base = 0; base < nb; base += kBoxChunk) {
    const int m = min(kBoxChunk, nb - base);
    // the chunk's boxes that meet the block, in box order: a ballot and a
    // prefix count per wavefront of 64, the wavefronts' counts through LDS
    int total = 0;
#pragma unroll
    for (int j = 0; j < kBoxChunk / 256; ++j) {
      const int b = j * 256 + t;
      bool take = b < m;
      if (CULL && take) {
        const float4 l = aabb[2 * (size_t)(base + b)], h = aabb[2 * (size_t)(base + b) + 1];
        take = l.x <= bhi[0] && h.x >= blo[0] && l.y <= bhi[1] && h.y >= blo[1] && l.z <= bhi[2] && h.z >= blo[2];
      }
      const unsigned long long mask = __ballot(take);
      if (lane == 0) s_cnt[j][w] = __popcll(mask);
      __syncthreads();
      int off = total;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = s_cnt[j][k];
        if (k < w) off += c;
        total += c;
      }
      if (take) {
        const int slot = off + __popcll(mask & ((1ull << lane) - 1ull));
        const float4* r = rec + 3 * (size_t)(base + b);
        s_rec[3 * slot] = r[0];
        s_rec[3 * slot + 1] = r[1];
        s_rec[3 * slot + 2] = r[2];
      }
    }
    __syncthreads();
    if (finite && !hit) {
      for (int k = 0; k < total; ++k) {
        const float4 A = s_rec[3 * k], B = s_rec[3 * k + 1], C = s_rec[3 * k + 2];
        const float dx = p.x - A.x, dy = p.y - A.y, dz = p.z - A.z;
        float lx = dx, ly = dy;
        if (C.w != 0.f) {   // R(yaw)^T d
          lx = (A.w * dx) + (B.x * dy);
          ly = (A.w * dy) - (B.x * dx);
        }
        // CropBox: outside when a coordinate is below min or above max
        if (!(lx < B.y || ly < B.z || dz < B.w || lx > C.x || ly > C.y || dz > C.z)) {
          hit = true;
          break;
        }
      }
    }
    __syncthreads();   // the next chunk overwrites the list
  }
  if (i < n) keep[i] = finite && !hit ? 1 : 0;
}

}  // namespace ddlo

struct ddlo_map {
  int device = 0;
  ddlo_map_params p{};
  hipStream_t s = nullptr;
  hipEvent_t ev = nullptr;   // the odometry driver's stream -> the map's (add_odom_keyframe)
  DevBuf pts, alt;           // float4: the map, and the compaction target of the same capacity
  int size = 0, cap = 0;     // points
  int inten = 0;             // ddlo_map_set_intensity: the points' w is the channel (else it is never read)
  // scratch (device): the upload, its float4 form, the flags and their scan, the voxel filter's, hipcub's, the boxes
  DevBuf up, a, keep, pos, vscratch, cubtmp, boxes;
  PinBuf pin;                // pinned: 16 ints, the count read-backs
};

namespace {

using namespace ddlo;
using namespace ddlo::rt;

void swap_buf(DevBuf& x, DevBuf& y) {
  std::swap(x.p, y.p);
  std::swap(x.bytes, y.bytes);
  std::swap(x.dev, y.dev);
}

// room for `total` points: DevBuf::ensure drops the contents, so the map
// moves to its new block with a device-to-device copy
gicp_status ensure_room(ddlo_map* m, size_t total) {
  if (total > (size_t)INT_MAX) return fail(GICP_EINVAL, "the map would exceed INT_MAX points");
  if (total <= (size_t)m->cap) return GICP_OK;
  const size_t cap = std::max(total, std::min<size_t>(2 * (size_t)m->cap, (size_t)INT_MAX));
  DevBuf grown;
  HIP_TRY(grown.ensure(sizeof(float4) * cap));
  if (m->size > 0) {
    HIP_TRY(hipMemcpyAsync(grown.p, m->pts.p, sizeof(float4) * (size_t)m->size, hipMemcpyDeviceToDevice, m->s));
    HIP_TRY(hipStreamSynchronize(m->s));
  }
  swap_buf(m->pts, grown);
  m->alt.reset();   // sized again by the next removal
  m->cap = (int)cap;
  return GICP_OK;
}

// keyframeCB (map.cc:101-117) for n float4 points on the device, ready on m->s
gicp_status add_points(ddlo_map* m, const float4* in, int n, size_t* added) {
  if (added) *added = 0;
  if (n <= 0) return GICP_OK;
  gicp_status st = ensure_room(m, (size_t)m->size + (size_t)n);
  if (st) return st;
  float4* const tail = m->pts.as<float4>() + m->size;
  HIP_TRY(m->cubtmp.ensure(std::max(crop_box_tmp_bytes(n), voxel_tmp_bytes(n))));
  int c = 0;
  bool vox = m->p.voxel_filter_use != 0;
  if (vox) {
    HIP_TRY(m->vscratch.ensure(sizeof(int) * voxel_scratch_ints(n)));
    if (voxel_grid(m->s, in, n, (float)m->p.leaf_size, tail, m->vscratch.as<int>(), m->cubtmp.p, m->cubtmp.bytes, &c, 0.f,
                   m->pin.as<int>(), CropCentre(), 0, nullptr, m->inten != 0))
      return fail(GICP_EHIP, "voxel filter scratch too small");
    if (c < 0) vox = false;   // voxel-index overflow: PCL leaves the cloud as it is
  }
  if (!vox) {   // the finite points in input order
    HIP_TRY(m->keep.ensure(sizeof(int) * (size_t)n));
    HIP_TRY(m->pos.ensure(sizeof(int) * (size_t)n));
    if (crop_box(m->s, in, n, 0.f, tail, m->keep.as<int>(), m->pos.as<int>(), m->cubtmp.p, m->cubtmp.bytes, &c, m->pin.as<int>(),
                 CropCentre(), false))
      return fail(GICP_EHIP, "compaction scratch too small");
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(m->s));   // the input (the caller's, or the upload) is free again
  m->size += c;
  if (added) *added = (size_t)c;
  return GICP_OK;
}

// dynamicObjectsCB's per-box values (map.cc:143-152) as the kernel's record
bool pack_box(const ddlo_map_box& b, double margin, float4* aabb, float4* rec) {
  const double f[7] = {b.position[0], b.position[1], b.position[2], b.orientation_z,
                       b.dimensions[0], b.dimensions[1], b.dimensions[2]};
  for (double v : f)
    if (!std::isfinite(v)) return false;
  if (std::fabs(b.orientation_z) > 1.0) return false;
  const float yaw = (float)(2 * std::asin(b.orientation_z));
  const float c = cosf(yaw), s = sinf(yaw);
  float ctr[3], mn[3], mx[3];
  for (int a = 0; a < 3; ++a) {
    ctr[a] = (float)b.position[a];
    mn[a] = (float)(-b.dimensions[a] / 2 - margin);
    mx[a] = (float)(b.dimensions[a] / 2 + margin);
    if (!std::isfinite(ctr[a]) || !std::isfinite(mn[a]) || !std::isfinite(mx[a])) return false;
  }
  rec[0] = make_float4(ctr[0], ctr[1], ctr[2], c);
  rec[1] = make_float4(s, mn[0], mn[1], mn[2]);
  rec[2] = make_float4(mx[0], mx[1], mx[2], yaw != 0.f ? 1.f : 0.f);
  // world bounds of the rotated box, in double, inflated by 1 mm (plus 1e-5
  // of the extent) over the float rounding of the kernel's test, rounded outwards
  double h[3];
  for (int a = 0; a < 3; ++a) h[a] = std::max(std::fabs((double)mn[a]), std::fabs((double)mx[a]));
  const double ac = std::fabs((double)c), as = std::fabs((double)s);
  const double e[3] = {ac * h[0] + as * h[1], as * h[0] + ac * h[1], h[2]};
  const double infl = 1e-3 + 1e-5 * (e[0] + e[1] + e[2]);
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = std::nextafterf((float)((double)ctr[a] - e[a] - infl), -INFINITY);
    hi[a] = std::nextafterf((float)((double)ctr[a] + e[a] + infl), INFINITY);
  }
  aabb[0] = make_float4(lo[0], lo[1], lo[2], 0.f);
  aabb[1] = make_float4(hi[0], hi[1], hi[2], 0.f);
  return true;
}

// the map's points on the host; leaf > 0: savePcd's voxelised copy
// (map.cc:169-177), its scratch allocated for the call: *count of them, as
// triples in xyz (room for cap points) unless it is nullptr; xyzi: as x, y, z,
// intensity, 16 B per point
gicp_status export_points(ddlo_map* m, double leaf, float* xyz, size_t cap, size_t* count, bool xyzi = false) {
  *count = 0;
  if (m->size == 0) return GICP_OK;
  HIP_TRY(hipSetDevice(m->device));
  const int n = m->size;
  const float4* src = m->pts.as<float4>();
  int c = n;
  DevBuf out, scratch, tmp;
  if (leaf > 0) {
    HIP_TRY(out.ensure(sizeof(float4) * (size_t)n));
    HIP_TRY(scratch.ensure(sizeof(int) * voxel_scratch_ints(n)));
    HIP_TRY(tmp.ensure(voxel_tmp_bytes(n)));
    if (voxel_grid(m->s, src, n, (float)leaf, out.as<float4>(), scratch.as<int>(), tmp.p, tmp.bytes, &c, 0.f,
                   m->pin.as<int>(), CropCentre(), 0, nullptr, xyzi))
      return fail(GICP_EHIP, "voxel filter scratch too small");
    HIP_TRY(hipGetLastError());
    if (c < 0) c = n;   // voxel-index overflow: the map as it is
    else src = out.as<float4>();
  }
  *count = (size_t)c;
  // either way the stream is waited for: the scratch goes back to the pool idle
  if (xyz && (size_t)c <= cap && xyzi) {
    if (c > 0) HIP_TRY(hipMemcpyAsync(xyz, src, sizeof(float4) * (size_t)c, hipMemcpyDeviceToHost, m->s));
    HIP_TRY(hipStreamSynchronize(m->s));
    return GICP_OK;
  }
  if (xyz && (size_t)c <= cap) return read_xyz(m->s, src, (size_t)c, xyz);
  HIP_TRY(hipStreamSynchronize(m->s));
  return xyz ? fail(GICP_EINVAL, "output capacity too small") : GICP_OK;
}

}  // namespace

extern "C" {

gicp_status ddlo_map_default_params(ddlo_map_params* out) {
  if (!out) return fail(GICP_EINVAL, "null params");
  out->voxel_filter_use = 1;
  out->leaf_size = 0.25;
  out->filter_bboxes = 1;
  out->filter_margin = 0.0;
  return GICP_OK;
}

gicp_status ddlo_map_create(int device, const ddlo_map_params* p, ddlo_map** out) {
  if (!out) return fail(GICP_EINVAL, "null out");
  *out = nullptr;
  auto m = std::make_unique<ddlo_map>();
  if (p) m->p = *p;
  else ddlo_map_default_params(&m->p);
  if (m->p.voxel_filter_use && !(m->p.leaf_size > 0 && std::isfinite(m->p.leaf_size)))
    return fail(GICP_EINVAL, "leaf_size must be positive");
  if (!std::isfinite(m->p.filter_margin)) return fail(GICP_EINVAL, "filter_margin must be finite");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(GICP_EHIP, "no HIP device " + std::to_string(device) + " (HIP library present, device not visible)");
  m->device = device;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(stream_pool().acquire(&m->s));
  if (hipEventCreateWithFlags(&m->ev, hipEventDisableTiming) != hipSuccess ||
      m->pin.reset(sizeof(int) * 16) != hipSuccess ||
      m->pts.ensure(sizeof(float4) * (size_t)kMapInitialCapacity) != hipSuccess) {
    if (m->ev) (void)hipEventDestroy(m->ev);
    stream_pool().release(device, m->s);
    return fail(GICP_EHIP, "allocation failed");
  }
  m->cap = kMapInitialCapacity;
  *out = m.release();
  return GICP_OK;
}

gicp_status ddlo_map_destroy(ddlo_map* m) {
  if (!m) return GICP_OK;
  (void)hipSetDevice(m->device);
  (void)hipStreamSynchronize(m->s);
  if (m->ev) (void)hipEventDestroy(m->ev);
  stream_pool().release(m->device, m->s);
  delete m;
  return GICP_OK;
}

// ddlo_map_add_keyframe (ioff = 0) and ddlo_map_add_keyframe_xyzi
static gicp_status add_keyframe(ddlo_map* m, const float* xyz, size_t n, size_t stride, size_t ioff, size_t* added) {
  if (added) *added = 0;
  if (n == 0) return GICP_OK;
  if (n > (size_t)INT_MAX || (size_t)m->size + n > (size_t)INT_MAX)
    return fail(GICP_EINVAL, "the map would exceed INT_MAX points");
  HIP_TRY(hipSetDevice(m->device));
  const size_t raw = (n - 1) * stride + std::max<size_t>(12, ioff ? ioff + 4 : 0);
  HIP_TRY(m->up.ensure(raw));
  HIP_TRY(hipMemcpyAsync(m->up.p, xyz, raw, hipMemcpyHostToDevice, m->s));
  HIP_TRY(m->a.ensure(sizeof(float4) * n));
  launch_pack4(m->s, m->up.as<unsigned char>(), stride, (int)n, m->a.as<float4>(), ioff);
  return add_points(m, m->a.as<float4>(), (int)n, added);
}

gicp_status ddlo_map_add_keyframe(ddlo_map* m, const float* xyz, size_t n, size_t stride, size_t* added) {
  if (!m || (!xyz && n) || stride < 12 || stride % 4) return fail(GICP_EINVAL, "invalid argument");
  return add_keyframe(m, xyz, n, stride, 0, added);
}

gicp_status ddlo_map_add_keyframe_xyzi(ddlo_map* m, const float* pts, size_t n, size_t stride, size_t offset_bytes,
                                       size_t* added) {
  if (!m || (!pts && n) || stride < 12 || stride % 4) return fail(GICP_EINVAL, "invalid argument");
  if (!m->inten) return fail(GICP_EINVAL, "the map carries no intensity (ddlo_map_set_intensity)");
  if (offset_bytes % 4 || offset_bytes < 12 || offset_bytes + 4 > stride)
    return fail(GICP_EINVAL, "intensity offset: a multiple of 4, >= 12 and offset + 4 <= stride");
  return add_keyframe(m, pts, n, stride, offset_bytes, added);
}

gicp_status ddlo_map_set_intensity(ddlo_map* m, int use) {
  if (!m) return fail(GICP_EINVAL, "null handle");
  if ((use != 0) != (m->inten != 0) && m->size != 0)
    return fail(GICP_EINVAL, "intensity: accepted only while the map is empty");
  m->inten = use != 0;
  return GICP_OK;
}

gicp_status ddlo_map_get_intensity(const ddlo_map* m, int* use) {
  if (!m || !use) return fail(GICP_EINVAL, "null argument");
  *use = m->inten;
  return GICP_OK;
}

gicp_status ddlo_map_points_xyzi(ddlo_map* m, double leaf, float* xyzi, size_t cap, size_t* n) {
  if (!m || !n || (!xyzi && cap)) return fail(GICP_EINVAL, "invalid argument");
  if (!m->inten) return fail(GICP_EINVAL, "the map carries no intensity (ddlo_map_set_intensity)");
  return export_points(m, leaf, xyzi, cap, n, true);
}

gicp_status ddlo_map_add_odom_keyframe(ddlo_map* m, const ddlo_odom* odom, int k, size_t* added) {
  if (!m || !odom) return fail(GICP_EINVAL, "null argument");
  if (added) *added = 0;
  const float4* pts = nullptr;
  int n = 0, dev = 0;
  hipStream_t os = nullptr;
  gicp_status st = odom_keyframe_dev(odom, k, &pts, &n, &dev, &os);
  if (st) return st;
  if (dev != m->device) return fail(GICP_EINVAL, "the map and the odometry driver are on different devices");
  if (m->inten && !odom_has_intensity(odom))
    return fail(GICP_EINVAL, "the map carries intensity and the odometry driver does not");
  HIP_TRY(hipSetDevice(m->device));
  // after the driver's queued work, without a host wait
  HIP_TRY(hipEventRecord(m->ev, os));
  HIP_TRY(hipStreamWaitEvent(m->s, m->ev, 0));
  return add_points(m, pts, n, added);
}

gicp_status ddlo_map_clear_boxes(ddlo_map* m, const ddlo_map_box* boxes, size_t nboxes, size_t* removed) {
  if (!m || (!boxes && nboxes)) return fail(GICP_EINVAL, "invalid argument");
  if (removed) *removed = 0;
  if (!m->p.filter_bboxes) return GICP_OK;   // the node does not subscribe (map.cc:38-39)
  if (nboxes > (size_t)(1 << 24)) return fail(GICP_EINVAL, "too many boxes");
  const int nb = (int)nboxes;
  std::vector<float4> h(5 * (size_t)nb);   // [aabb 2 nb][rec 3 nb]
  for (int b = 0; b < nb; ++b)
    if (!pack_box(boxes[b], m->p.filter_margin, &h[2 * (size_t)b], &h[2 * (size_t)nb + 3 * (size_t)b]))
      return fail(GICP_EINVAL, "box " + std::to_string(b) + ": |orientation_z| > 1 or a non-finite field");
  if (nb == 0 || m->size == 0) return GICP_OK;
  HIP_TRY(hipSetDevice(m->device));
  const int n = m->size;
  HIP_TRY(m->boxes.ensure(sizeof(float4) * h.size()));
  HIP_TRY(hipMemcpyAsync(m->boxes.p, h.data(), sizeof(float4) * h.size(), hipMemcpyHostToDevice, m->s));
  HIP_TRY(m->alt.ensure(sizeof(float4) * (size_t)m->cap));
  HIP_TRY(m->keep.ensure(sizeof(int) * (size_t)n));
  HIP_TRY(m->pos.ensure(sizeof(int) * (size_t)n));
  HIP_TRY(m->cubtmp.ensure(crop_box_tmp_bytes(n)));
  const float4* aabb = m->boxes.as<float4>();
  const float4* rec = aabb + 2 * (size_t)nb;
  const int grid = (int)(((long long)n + 255) / 256);
  // up to kNoCullBoxes boxes every workgroup tests them all: the block bounds
  // cost more than the tests they would save
  static const bool no_cull = dev_getenv("DDLO_MAP_NO_CULL") != nullptr;   // A/B, development
  if (no_cull || nb <= kNoCullBoxes)
    k_map_box_flags<false><<<grid, 256, 0, m->s>>>(m->pts.as<float4>(), n, aabb, rec, nb, m->keep.as<int>());
  else
    k_map_box_flags<true><<<grid, 256, 0, m->s>>>(m->pts.as<float4>(), n, aabb, rec, nb, m->keep.as<int>());
  int c = 0;
  if (compact_flagged(m->s, m->pts.as<float4>(), n, m->alt.as<float4>(), m->keep.as<int>(), m->pos.as<int>(),
                      m->cubtmp.p, m->cubtmp.bytes, &c, m->pin.as<int>()))
    return fail(GICP_EHIP, "compaction scratch too small");
  HIP_TRY(hipGetLastError());
  swap_buf(m->pts, m->alt);
  m->size = c;
  if (removed) *removed = (size_t)(n - c);
  return GICP_OK;
}

gicp_status ddlo_map_size(const ddlo_map* m, size_t* n) {
  if (!m || !n) return fail(GICP_EINVAL, "null argument");
  *n = (size_t)m->size;
  return GICP_OK;
}

gicp_status ddlo_map_points(ddlo_map* m, double leaf, float* xyz, size_t cap, size_t* n) {
  if (!m || !n || (!xyz && cap)) return fail(GICP_EINVAL, "invalid argument");
  return export_points(m, leaf, xyz, cap, n);
}

gicp_status ddlo_map_save_pcd(ddlo_map* m, const char* path, double leaf) {
  if (!m || !path) return fail(GICP_EINVAL, "null argument");
  size_t n = 0;
  const bool xyzi = m->inten != 0;
  const size_t nf = xyzi ? 4 : 3;
  std::vector<float> xyz(nf * (size_t)m->size + 1);   // (the voxelised copy is no larger; + 1: never a null pointer)
  gicp_status st = export_points(m, leaf, xyz.data(), (size_t)m->size, &n, xyzi);
  if (st) return st;
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(GICP_EINVAL, std::string("cannot open ") + path);
  // the header pcl::PCDWriter::writeBinary gives an unorganized cloud of x, y, z
  // (with intensity: the four fields of the reference's PointXYZI map, packed)
  std::fprintf(f,
               xyzi ? "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\n"
                      "TYPE F F F F\nCOUNT 1 1 1 1\nWIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %zu\nDATA binary\n"
                    : "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\n"
                      "COUNT 1 1 1\nWIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %zu\nDATA binary\n",
               n, n);
  const size_t wrote = n ? std::fwrite(xyz.data(), sizeof(float) * nf, n, f) : 0;
  const bool closed = std::fclose(f) == 0;
  if (wrote != n || !closed) return fail(GICP_EINVAL, std::string("write failed: ") + path);
  return GICP_OK;
}

}  // extern "C"
