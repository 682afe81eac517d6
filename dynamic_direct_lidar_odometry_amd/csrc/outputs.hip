// outputs.hip — K6 of the GICP hot path: what an align hands back.
//
//   K6 outputs          k_residuals, k_resimg_claim /   getResiduals :225-232,
//                       k_resimg_fill, k_transform,     transformPointCloud lsq:125
//                       k_export_corr
// Compiled with -ffp-contract=off (see index_build.hip).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gicp_types.hpp"
#include "search.hpp"
#include "launch.hpp"
#include "launch_util.hpp"

namespace ddlo {

// ---------------------------------------------------------------------------
// K6: residuals (getResiduals) — unbounded 1-NN for points without a
// correspondence, at the pose of the last linearization.
__global__ __launch_bounds__(256) void k_residuals(const AlignJob* __restrict__ job, double* __restrict__ out) {
  const CloudDev src = job->src;
  const CloudDev tgt = job->tgt;
  const AlignState* st = job->state;
  float Rf[9], tf[3];
  for (int e = 0; e < 9; ++e) Rf[e] = (float)st->last_lin_R[e];
  for (int e = 0; e < 3; ++e) tf[e] = (float)st->last_lin_t[e];
  __shared__ WaveLds lds[4];
  WaveLds* L = &lds[threadIdx.x >> 6];
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves_total = (gridDim.x * blockDim.x) >> 6;
  const int ngroups = (src.n + 63) >> 6;
  for (int g = wave; g < ngroups; g += nwaves_total) {
    const int i = g * 64 + lane_id();
    const bool active = i < src.n;
    float d2 = active ? job->sqd[i] : 0.f;
    const bool need = active && !(d2 < INFINITY);
    if (__any(need)) {
      const float4 a = ldg4(src.pts, active ? i : src.n - 1);
      NN1Visitor vis;
      vis.qx = (Rf[0] * a.x + Rf[1] * a.y) + (Rf[2] * a.z + tf[0]);
      vis.qy = (Rf[3] * a.x + Rf[4] * a.y) + (Rf[5] * a.z + tf[1]);
      vis.qz = (Rf[6] * a.x + Rf[7] * a.y) + (Rf[8] * a.z + tf[2]);
      vis.active = need;
      vis.best = need ? INFINITY : -1.f;
      vis.bestj = -1;
      // seed: the nearest of a Morton window per lane (finite bound)
      if (need) {
        const int pos = min(wave_lower_bound_lane(tgt.keys, tgt.n,
                                                  morton_key(vis.qx, vis.qy, vis.qz, tgt.quant)), tgt.n - 1);
        for (int o = -4; o <= 4; ++o) {
          const int j = pos + o;
          if (j < 0 || j >= tgt.n) continue;
          const float4 p = ldg4(tgt.pts, j);
          const float d = dist2(vis.qx, vis.qy, vis.qz, p.x, p.y, p.z);
          if (d < vis.best || (d == vis.best && (unsigned)j < (unsigned)vis.bestj)) {
            vis.best = d;
            vis.bestj = j;
          }
        }
      }
      vis.skip_lo = 1;
      vis.skip_hi = 0;
      vis.box = make_wave_box(need, vis.qx, vis.qy, vis.qz, vis.best);
      traverse(tgt, vis, L);
      if (need) {
        d2 = vis.best;
        job->sqd[i] = d2;
      }
    }
    if (active && out) out[src.perm[i]] = sqrt((double)d2);
  }
}

// Residual image (odom.cc:804-827 -> detection.cpp
// projectResiduals :203-252).  Pixel of source point i (sensor frame, the
// scan the residuals belong to): theta = atan2(x, z), phi = atan2(y,
// sqrt(x^2 + z^2)) in double, u = int((theta - tmin) / (tmax - tmin) * W),
// v likewise with phi; points outside [0, W) x [0, H) are skipped.
// (Which atan2/sqrt overload the reference's unqualified calls on float
// members resolve to depends on the headers reaching odom.cc; this takes
// the C double functions.  Only pixel-boundary cases can differ.)  The
// reference fills the image in point order, so the HIGHEST original index
// that lands on a pixel wins: atomicMax of the index, then a gather pass.
__global__ __launch_bounds__(256) void k_resimg_claim(const float4* __restrict__ pts, const int* __restrict__ perm,
                                                      int n, double tmin, double tmax, int W, int H,
                                                      int* __restrict__ winner) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  // x*x + z*z is float arithmetic in the reference (PointXYZI members);
  // atan2 / sqrt then run on the promoted values
  const float xz2 = p.x * p.x + p.z * p.z;
  const double theta = atan2((double)p.x, (double)p.z);
  const double phi = atan2((double)p.y, sqrt((double)xz2));
  const int u = (int)((theta - tmin) / (tmax - tmin) * W);
  const int v = (int)((phi - tmin) / (tmax - tmin) * H);
  if (u < 0 || u >= W || v < 0 || v >= H) return;
  atomicMax(&winner[(size_t)v * W + u], perm[i]);
}

__global__ __launch_bounds__(256) void k_resimg_fill(const int* __restrict__ winner, int npix,
                                                     const double* __restrict__ residual,
                                                     const float4* __restrict__ pts, const int* __restrict__ inv_perm,
                                                     float* __restrict__ img, float* __restrict__ xyz) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const int o = winner[p];
  float r = 0.f, x = 0.f, y = 0.f, z = 0.f;   // empty pixel: PCL's default point, intensity 0
  if (o >= 0) {
    r = (float)residual[o];
    const float4 q = pts[inv_perm[o]];
    x = q.x; y = q.y; z = q.z;
  }
  img[p] = r;
  if (xyz) {
    xyz[3 * (size_t)p + 0] = x;
    xyz[3 * (size_t)p + 1] = y;
    xyz[3 * (size_t)p + 2] = z;
  }
}

// pcl::transformPointCloud with final_transformation_ (float 4x4)
__global__ __launch_bounds__(256) void k_transform(const float4* __restrict__ pts, int n, const int* __restrict__ perm,
                                                   const float* __restrict__ T16, float* __restrict__ out,
                                                   size_t stride_floats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 a = pts[i];
  float* o = out + (size_t)perm[i] * stride_floats;
  o[0] = (T16[0] * a.x + T16[1] * a.y) + (T16[2] * a.z + T16[3]);
  o[1] = (T16[4] * a.x + T16[5] * a.y) + (T16[6] * a.z + T16[7]);
  o[2] = (T16[8] * a.x + T16[9] * a.y) + (T16[10] * a.z + T16[11]);
}

// correspondences in original source order (original target indices)
__global__ __launch_bounds__(256) void k_export_corr(const AlignJob* __restrict__ job, int* __restrict__ corr_out,
                                                     float* __restrict__ sqd_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // sorted source index
  if (i >= job->src.n) return;
  const int o = job->src.perm[i];
  const int j = job->corr[i];
  if (corr_out) corr_out[o] = j >= 0 ? job->tgt.perm[j] : -1;
  if (sqd_out) sqd_out[o] = job->sqd[i];
}

void launch_residual_image(hipStream_t s, const float4* pts, const int* perm, const int* inv_perm, int n,
                           const double* residual, double tmin, double tmax, int W, int H, int* winner, float* img,
                           float* xyz) {
  k_resimg_claim<<<cdiv(n, 256), 256, 0, s>>>(pts, perm, n, tmin, tmax, W, H, winner);
  k_resimg_fill<<<cdiv((long)W * H, 256), 256, 0, s>>>(winner, W * H, residual, pts, inv_perm, img, xyz);
}
void launch_residuals(hipStream_t s, const AlignJob* job, int nsrc, double* out) {
  k_residuals<<<group_blocks(nsrc), 256, 0, s>>>(job, out);
}
void launch_transform(hipStream_t s, const float4* pts, int n, const int* perm, const float* T16, float* out,
                      size_t stride_floats) {
  k_transform<<<cdiv(n, 256), 256, 0, s>>>(pts, n, perm, T16, out, stride_floats);
}
void launch_export_corr(hipStream_t s, const AlignJob* job, int nsrc, int* corr, float* sqd) {
  k_export_corr<<<cdiv(nsrc, 256), 256, 0, s>>>(job, corr, sqd);
}

}  // namespace ddlo
