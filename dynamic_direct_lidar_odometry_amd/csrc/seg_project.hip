// seg_project.hip — an unorganized cloud into the segmentation's range image
// and the way back from pixels to the caller's points
// (include/ddlo_seg_project.h: the model, the two deviations from the
// reference's commented loop, the conventions).
//
//   k_proj_claim          one thread per input point of the strided raw upload
//                         (the layout k_pack4 / k_transform_raw read):
//                         pix_of_point[i], and an integer atomicMax (agent
//                         scope) of i on winner[pixel].  The winner image is
//                         reset to -1 on the stream before the launch and read
//                         by plain loads in the next launch: the k_resimg_claim
//                         / k_resimg_fill pattern (outputs.hip).
//   k_proj_fill           one thread per pixel: T * p[winner] as a float4 into
//                         the segmentation's staged input, k_transform_raw's
//                         operation order (this file is compiled with
//                         -ffp-contract=off as every other); no winner: NaN.
//   k_proj_sum            one workgroup adds the per-workgroup partial counts
//                         of the two kernels above (invalid and out-of-view
//                         points; occupied pixels).  The partials come from
//                         wavefront ballots added through LDS; there is no
//                         same-address counter atomic (DESIGN.md §11 measured
//                         what one per wavefront costs) and no floating-point
//                         atomic anywhere.
//   k_proj_point_classes  one thread per input point: the class byte of the
//                         pixel it fell into.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/ddlo_segment.h"
#include "runtime.hpp"
#include "seg_state.hpp"

namespace ddlo {

namespace {

using rt::DevBuf;
using rt::fail;

constexpr int kProjThreads = 256;
constexpr int kProjWaves = kProjThreads / 64;
constexpr double kDegPerRad = 180.0 / M_PI;

// the projection as the kernel reads it: every parameter promoted to double on the host
struct ProjModel {
  double elev_top, elev_res, azim0, azim_sign, col_width;   // col_width = 360.0 / cols
  int rows, cols;
};

enum : int { kProjInvalid = -1, kProjOutOfView = -2 };

// the pixel of a point (ddlo_seg_project.h: these operations in this order), or kProjInvalid / kProjOutOfView
__device__ __forceinline__ int proj_pixel(float xf, float yf, float zf, const ProjModel& m) {
  if (!(isfinite(xf) && isfinite(yf) && isfinite(zf))) return kProjInvalid;
  if (xf == 0.f && yf == 0.f && zf == 0.f) return kProjInvalid;
  const double x = (double)xf, y = (double)yf, z = (double)zf;
  const double e = atan2(z, sqrt(x * x + y * y)) * kDegPerRad;
  const double qr = (m.elev_top - e) / m.elev_res;
  const double row = floor(qr + 0.5);
  if (!(row >= 0.0 && row < (double)m.rows)) return kProjOutOfView;
  const double a = atan2(y, x) * kDegPerRad;
  const double qc = m.azim_sign * (a - m.azim0) / m.col_width;
  const double c = floor(qc + 0.5);
  // ((c mod cols) + cols) mod cols; fmod is exact, so this is the integer remainder whatever the size of c
  double col = fmod(c, (double)m.cols);
  if (col < 0.0) col += (double)m.cols;
  return (int)row * m.cols + (int)col;
}

// partial[2 * workgroup] = invalid points, [+ 1] = out-of-view points of the workgroup's 256
__global__ __launch_bounds__(kProjThreads) void k_proj_claim(const unsigned char* __restrict__ raw, size_t stride, int n,
                                                             ProjModel m, int npix, int* __restrict__ winner,
                                                             int* __restrict__ pix_of_point, int* __restrict__ partial) {
  __shared__ int sh[kProjWaves][2];
  const int i = blockIdx.x * kProjThreads + threadIdx.x;
  int pix = 0;   // (a thread past the end counts as neither)
  if (i < n) {
    const float* p = reinterpret_cast<const float*>(raw + (size_t)i * stride);
    pix = proj_pixel(p[0], p[1], p[2], m);
    if ((unsigned)pix >= (unsigned)npix && pix >= 0) pix = kProjOutOfView;   // (never: row < rows and col < cols)
    pix_of_point[i] = pix >= 0 ? pix : -1;
    if (pix >= 0) atomicMax(&winner[pix], i);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ninv = __popcll(__ballot(pix == kProjInvalid));
  const int noov = __popcll(__ballot(pix == kProjOutOfView));
  if (lane == 0) {
    sh[w][0] = ninv;
    sh[w][1] = noov;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int s = 0;
    for (int j = 0; j < kProjWaves; ++j) s += sh[j][threadIdx.x];
    partial[2 * blockIdx.x + threadIdx.x] = s;
  }
}

struct ProjPose {
  float m[12];
};

// partial[workgroup] = occupied pixels of the workgroup's 256
// INTEN: the winner brings its own intensity (the float ioff bytes into its record) into w; else w = 0
template <bool INTEN>
__global__ __launch_bounds__(kProjThreads) void k_proj_fill(const int* __restrict__ winner, int npix,
                                                            const unsigned char* __restrict__ raw, size_t stride, int n,
                                                            ProjPose T, size_t ioff, float4* __restrict__ out,
                                                            int* __restrict__ partial) {
  __shared__ int sh[kProjWaves];
  const int p = blockIdx.x * kProjThreads + threadIdx.x;
  bool occupied = false;
  if (p < npix) {
    const int o = winner[p];
    float4 r = make_float4(NAN, NAN, NAN, 0.f);
    if ((unsigned)o < (unsigned)n) {   // (-1: no winner)
      occupied = true;
      const unsigned char* rec = raw + (size_t)o * stride;
      const float* q = reinterpret_cast<const float*>(rec);
      const float x = q[0], y = q[1], z = q[2];
      const float* m = T.m;
      r = make_float4((m[0] * x + m[1] * y) + (m[2] * z + m[3]), (m[4] * x + m[5] * y) + (m[6] * z + m[7]),
                      (m[8] * x + m[9] * y) + (m[10] * z + m[11]),
                      INTEN ? *reinterpret_cast<const float*>(rec + ioff) : 0.f);
    }
    out[p] = r;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = __popcll(__ballot(occupied));
  if (lane == 0) sh[w] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int j = 0; j < kProjWaves; ++j) s += sh[j];
    partial[blockIdx.x] = s;
  }
}

// one workgroup: out[0] = invalid, out[1] = out of view, out[2] = occupied.  Thread t adds count t % 4 of the
// workgroups t / 4, t / 4 + 64, ...; thread k < 3 then adds the 64 sums in index order.
__global__ __launch_bounds__(kProjThreads) void k_proj_sum(const int* __restrict__ claim, int nwg_claim,
                                                           const int* __restrict__ fill, int nwg_fill,
                                                           int* __restrict__ out) {
  __shared__ int sh[kProjThreads];
  const int k = threadIdx.x & 3;
  int s = 0;
  if (k < 2)
    for (int g = threadIdx.x >> 2; g < nwg_claim; g += kProjThreads / 4) s += claim[2 * g + k];
  else if (k == 2)
    for (int g = threadIdx.x >> 2; g < nwg_fill; g += kProjThreads / 4) s += fill[g];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < 3) {
    int t = 0;
    for (int j = 0; j < kProjThreads / 4; ++j) t += sh[4 * j + threadIdx.x];
    out[threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(kProjThreads) void k_proj_point_classes(const int* __restrict__ pix_of_point, int n,
                                                                     const unsigned char* __restrict__ img, int npix,
                                                                     unsigned char* __restrict__ out) {
  const int i = blockIdx.x * kProjThreads + threadIdx.x;
  if (i >= n) return;
  const int p = pix_of_point[i];
  out[i] = (unsigned)p < (unsigned)npix ? img[p] : (unsigned char)0;
}

int workgroups(int n) { return (n + kProjThreads - 1) / kProjThreads; }

// scratch that follows the cloud's size: grown by half again at least, so a
// stream of clouds of slowly varying size does not reallocate every scan
hipError_t reserve(DevBuf& b, size_t bytes) {
  if (bytes <= b.bytes && b.p) return hipSuccess;
  return b.ensure(std::max(bytes, b.bytes + b.bytes / 2));
}

}  // namespace

struct SegProject {
  DevBuf up;        // ddlo_seg_process_cloud's upload
  DevBuf winner;    // [npix]
  DevBuf pix;       // [n] pixel_of_point
  DevBuf partial;   // [2 * claim workgroups][fill workgroups]
  DevBuf counts;    // [4]
  DevBuf pcls;      // [n] ddlo_seg_point_classes' result
  rt::PinBuf pin;       // pinned: the counts' read-back (4 ints)
  int n = 0;            // points of the last projection
  bool staged = false;  // seg_project_dev ran; seg_project_commit has not
  bool have = false;    // the maps are those of scan `serial`
  unsigned long long serial = 0;
};

void SegPartFree::operator()(SegProject* p) const { delete p; }

namespace {

// the part, made on first use (the device is set)
gicp_status project_of(ddlo_seg* s, SegProject** out) {
  if (!s->project) s->project.reset(new SegProject());
  SegProject* const p = s->project.get();
  if (!p->pin.p) HIP_TRY(p->pin.reset(sizeof(int) * 4));
  *out = p;
  return GICP_OK;
}

// the maps of the handle's scan, or GICP_EINVAL
gicp_status current(ddlo_seg* s, SegProject** p) {
  *p = s->project.get();
  if (!*p || !(*p)->have) return fail(GICP_EINVAL, "no projected scan (ddlo_seg_process_cloud)");
  if (!s->have || (*p)->serial != s->scan_serial)
    return fail(GICP_EINVAL, "the last scan was organized: the projection maps belong to an earlier scan");
  HIP_TRY(hipSetDevice(s->device));
  return GICP_OK;
}

gicp_status default_projection(const ddlo_seg_params& p, ddlo_seg_projection* out) {
  if (p.rows < 2) return fail(GICP_EINVAL, "rows must be at least 2");
  out->elev_top_deg = p.ang_bottom;
  out->elev_res_deg = 2 * p.ang_bottom / float(p.rows - 1);
  out->azim0_deg = 0.f;
  out->azim_sign = 1;
  return GICP_OK;
}

gicp_status check_projection(const ddlo_seg_projection& q) {
  if (!std::isfinite(q.elev_top_deg) || !std::isfinite(q.elev_res_deg) || !std::isfinite(q.azim0_deg))
    return fail(GICP_EINVAL, "projection: a parameter is not finite");
  if (!(q.elev_res_deg > 0.f)) return fail(GICP_EINVAL, "projection: elev_res_deg must be positive");
  if (q.azim_sign != 1 && q.azim_sign != -1) return fail(GICP_EINVAL, "projection: azim_sign must be +1 or -1");
  return GICP_OK;
}

}  // namespace

gicp_status seg_projection_resolve(ddlo_seg* s, const ddlo_seg_projection* proj, ddlo_seg_projection* out) {
  if (!s || !out) return fail(GICP_EINVAL, "null argument");
  if (proj) {
    *out = *proj;
  } else {
    if (gicp_status st = default_projection(s->p, out)) return st;
  }
  return check_projection(*out);
}

gicp_status seg_project_dev(ddlo_seg* s, hipStream_t st, const unsigned char* raw, size_t stride, int n, const float T[16],
                            const ddlo_seg_projection& proj, ddlo_seg_projection_result* out, size_t ioff) {
  if (!s || !T || (!raw && n) || n < 0) return fail(GICP_EINVAL, "invalid argument");
  if (gicp_status e = check_projection(proj)) return e;
  HIP_TRY(hipSetDevice(s->device));
  SegProject* p = nullptr;
  if (gicp_status e = project_of(s, &p)) return e;
  // valid: from here on the maps and the staged input are rewritten
  p->have = false;
  p->staged = false;
  float4* buf = nullptr;
  int npix = 0;
  if (gicp_status e = seg_stage_input(s, &buf, &npix)) return e;
  const int nwg_c = workgroups(n), nwg_f = workgroups(npix);
  HIP_TRY(p->winner.ensure(sizeof(int) * (size_t)npix));
  HIP_TRY(reserve(p->pix, sizeof(int) * (size_t)std::max(n, 1)));
  HIP_TRY(reserve(p->partial, sizeof(int) * (2 * (size_t)nwg_c + (size_t)nwg_f)));
  HIP_TRY(p->counts.ensure(sizeof(int) * 4));
  ProjModel m;
  m.elev_top = (double)proj.elev_top_deg;
  m.elev_res = (double)proj.elev_res_deg;
  m.azim0 = (double)proj.azim0_deg;
  m.azim_sign = (double)proj.azim_sign;
  m.col_width = 360.0 / s->p.cols;
  m.rows = s->p.rows;
  m.cols = s->p.cols;
  ProjPose P;
  for (int e = 0; e < 12; ++e) P.m[e] = T[e];
  int* claim_part = p->partial.as<int>();
  int* fill_part = claim_part + 2 * (size_t)nwg_c;
  HIP_TRY(hipMemsetAsync(p->winner.p, 0xff, sizeof(int) * (size_t)npix, st));   // -1: no winner
  if (n > 0)
    k_proj_claim<<<nwg_c, kProjThreads, 0, st>>>(raw, stride, n, m, npix, p->winner.as<int>(), p->pix.as<int>(),
                                                 claim_part);
  if (ioff)
    k_proj_fill<true><<<nwg_f, kProjThreads, 0, st>>>(p->winner.as<int>(), npix, raw, stride, n, P, ioff, buf, fill_part);
  else
    k_proj_fill<false><<<nwg_f, kProjThreads, 0, st>>>(p->winner.as<int>(), npix, raw, stride, n, P, 0, buf, fill_part);
  k_proj_sum<<<1, kProjThreads, 0, st>>>(claim_part, nwg_c, fill_part, nwg_f, p->counts.as<int>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(p->pin.p, p->counts.p, sizeof(int) * 3, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  p->n = n;
  p->staged = true;
  if (out) {
    const int* c = p->pin.as<int>();
    out->points = n;
    out->invalid = c[0];
    out->out_of_view = c[1];
    out->occupied_pixels = c[2];
    out->collisions = n - c[0] - c[1] - c[2];
  }
  return GICP_OK;
}

gicp_status seg_project_commit(ddlo_seg* s) {
  if (!s) return fail(GICP_EINVAL, "null argument");
  SegProject* const p = s->project.get();
  if (!p || !p->staged || !s->have) return fail(GICP_ESTATE, "no projected scan was staged");
  p->staged = false;
  p->serial = s->scan_serial;
  p->have = true;
  return GICP_OK;
}

}  // namespace ddlo

using namespace ddlo;

extern "C" {

gicp_status ddlo_seg_default_projection(const ddlo_seg_params* p, ddlo_seg_projection* out) {
  if (!p || !out) return fail(GICP_EINVAL, "null argument");
  return default_projection(*p, out);
}

gicp_status ddlo_seg_process_cloud(ddlo_seg* s, const float* xyz, size_t n, size_t stride, const float T[16],
                                   const ddlo_seg_projection* proj, const float* residual, ddlo_seg_result* res,
                                   ddlo_seg_projection_result* proj_res) {
  if (!s || !T || (!xyz && n) || stride < 12 || stride % 4) return fail(GICP_EINVAL, "invalid argument");
  if (n > (size_t)INT32_MAX / 2) return fail(GICP_EINVAL, "cloud too large");
  const size_t ioff = s->inten_use ? s->inten_off : 0;
  if (ioff && (ioff % 4 || ioff < 12 || ioff + 4 > stride))
    return fail(GICP_EINVAL, "intensity offset: a multiple of 4, >= 12 and offset + 4 <= stride");
  ddlo_seg_projection q;
  if (gicp_status st = seg_projection_resolve(s, proj, &q)) return st;
  HIP_TRY(hipSetDevice(s->device));
  SegProject* p = nullptr;
  if (gicp_status st = project_of(s, &p)) return st;
  if (n) {
    const size_t raw_sz = (n - 1) * stride + std::max<size_t>(12, ioff ? ioff + 4 : 0);
    HIP_TRY(reserve(p->up, raw_sz));
    HIP_TRY(hipMemcpyAsync(p->up.p, xyz, raw_sz, hipMemcpyHostToDevice, s->s));
  }
  ddlo_seg_projection_result pr{};
  if (gicp_status st = seg_project_dev(s, s->s, n ? p->up.as<unsigned char>() : nullptr, stride, (int)n, T, q, &pr, ioff))
    return st;
  if (gicp_status st = seg_process_staged(s, T, residual, res)) return st;
  if (gicp_status st = seg_project_commit(s)) return st;
  if (proj_res) *proj_res = pr;
  return GICP_OK;
}

gicp_status ddlo_seg_projection_maps(ddlo_seg* s, int32_t* winner, int32_t* pixel_of_point, size_t cap, size_t* n) {
  if (!s || !n || (!pixel_of_point && cap)) return fail(GICP_EINVAL, "invalid argument");
  SegProject* p = nullptr;
  if (gicp_status st = current(s, &p)) return st;
  *n = (size_t)p->n;
  const size_t npix = (size_t)s->p.rows * s->p.cols, k = std::min(cap, (size_t)p->n);
  if (winner) HIP_TRY(hipMemcpyAsync(winner, p->winner.p, sizeof(int32_t) * npix, hipMemcpyDeviceToHost, s->s));
  if (pixel_of_point && k)
    HIP_TRY(hipMemcpyAsync(pixel_of_point, p->pix.p, sizeof(int32_t) * k, hipMemcpyDeviceToHost, s->s));
  HIP_TRY(hipStreamSynchronize(s->s));
  return GICP_OK;
}

gicp_status ddlo_seg_point_classes(ddlo_seg* s, uint8_t* out, size_t cap, size_t* n) {
  if (!s || !n || (!out && cap)) return fail(GICP_EINVAL, "invalid argument");
  SegProject* p = nullptr;
  if (gicp_status st = current(s, &p)) return st;
  const unsigned char* img = nullptr;
  if (gicp_status st = seg_class_image_dev(s, &img)) return st;
  *n = (size_t)p->n;
  const size_t k = std::min(cap, (size_t)p->n);
  if (!out || k == 0) return GICP_OK;
  HIP_TRY(reserve(p->pcls, (size_t)p->n));
  k_proj_point_classes<<<workgroups(p->n), kProjThreads, 0, s->s>>>(p->pix.as<int>(), p->n, img, s->p.rows * s->p.cols,
                                                                     p->pcls.as<unsigned char>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, p->pcls.p, k, hipMemcpyDeviceToHost, s->s));
  HIP_TRY(hipStreamSynchronize(s->s));
  return GICP_OK;
}

}  // extern "C"
