// segment.hip — range-image segmentation of one organized scan
// (include/ddlo_segment.h).
//
// Device: k_seg_pixels, one thread per pixel, fuses
//   projectScan    (detection.cpp:292-329): range from the sensor position,
//                  minimum range, the "full cloud" (NaN where no range);
//   groundRemoval  (:458-491): the reference walks each column from the
//                  bottom, and a pixel's mark is written by the test of its
//                  own row pair (lower = r: no info -> -1, ground -> 1) after
//                  the test of the pair below it (lower = r + 1: ground -> 1
//                  on the upper pixel).  The last write decides, so
//                    ground(r) = -1 if test(r) has no info, 1 if test(r) is
//                    ground, else 1 if test(r + 1) is ground, else 0
//                  for r in the tested rows; the row just above them only
//                  receives the test(r + 1) write.  Each thread evaluates the
//                  (at most two) tests that write its pixel: no column walk;
//   label init     (:493-504): -1 for ground or no-range pixels, else 0.
// Labelling (cloudSegmentation / labelComponents, :510-724), two modes
// (ddlo_seg_set_labelling):
//   host (the default): the reference's breadth-first search, literally, over
//     the images read back -- segment numbers follow the row-major scan,
//     min_z / max_z is an if / else-if over the push order, the residual sum
//     is a float sum in push order;
//   device (seg_label.hip): the same labels and segment count without the
//     search order (connected components, a replayed prefix for max_z); the
//     average residuals are a double sum in row-major order, within
//     (m + 1) 2^-24 of the host's float sum.  No image leaves the device
//     unless a getter asks for it.
//
// Float behaviour follows the reference, where ddlo.h:35 includes <stdlib.h>
// (libstdc++'s wrapper brings std::abs into the global namespace, <cmath>
// the float atan2 / sqrt) so the unqualified abs / atan2 / sqrt calls on
// floats are the float overloads; -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/ddlo_segment.h"
#include "gicp_types.hpp"
#include "launch.hpp"
#include "runtime.hpp"
#include "seg_internal.hpp"
#include "seg_label.hpp"
#include "seg_state.hpp"

namespace ddlo {
namespace {

using rt::DevBuf;
using rt::fail;

constexpr int kRejected = DDLO_SEG_REJECTED;

struct SegPixelArgs {
  const unsigned char* raw;
  size_t stride;
  int H, W;
  float x0, y0, z0;      // -T(0:3, 3)
  float min_range;
  int ground_rows;
  float mount, thr;
  float* range;
  signed char* ground;
  int* label;
  float* zout;           // cloud_in_t z of every pixel (a scan staged on the device), or nullptr
};

// full_cloud_ point of pixel i (:309-327): the cloud point when finite with
// range >= minimum_range_, else nan_point_.
__device__ __forceinline__ float3 full_point(const SegPixelArgs& a, int i, float* range_out) {
  const float* p = reinterpret_cast<const float*>(a.raw + (size_t)i * a.stride);
  const float px = p[0], py = p[1], pz = p[2];
  float r = 0.f;
  float3 f = make_float3(NAN, NAN, NAN);
  if (isfinite(px) && isfinite(py) && isfinite(pz)) {   // pcl::isFinite
    const float x = px + a.x0, y = py + a.y0, z = pz + a.z0;
    const float d = (float)sqrt((double)((x * x + y * y) + z * z));   // correctly rounded sqrtf
    if (!(d < a.min_range)) {
      r = d;
      f = make_float3(px, py, pz);
    }
  }
  if (range_out) *range_out = r;
  return f;
}

// One ground test, lower = (row, col), upper = (row - 1, col): -1 no info,
// 1 ground, 0 neither (:470-489).
__device__ __forceinline__ int ground_test(const float3& lo, const float3& up, float mount, float thr) {
  if (lo.x == 0.f || up.x == 0.f) return -1;   // a NaN point is not == 0: it falls through to a NaN angle
  const float dx = up.x - lo.x, dy = up.y - lo.y, dz = up.z - lo.z;
  // atan2(float, float) * 180 -> float, / M_PI -> double, stored as float.
  // atan2f is defined as the double atan2 rounded to float (the device's own
  // atan2f is less accurate).  glibc 2.35's atan2f is not that function: over
  // 200,000 pairs within a few float ulps of a 10 or 80 degree threshold it
  // is one ulp off the rounded double in 6.0 % and decides the other way in
  // 0.6 %; away from a threshold the ulp cannot matter.  The tests hold this
  // kernel bit for bit to the reference's loop with the rounded double
  // (tests/test_gpu_seg_pixels.py).
  const float s = (float)sqrt((double)(dx * dx + dy * dy));
  const float at = (float)atan2((double)dz, (double)s);
  const float angle = (float)((double)(at * 180.f) / M_PI);
  return fabsf(angle - mount) <= thr ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_seg_pixels(SegPixelArgs a) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  const int row = blockIdx.y;
  if (col >= a.W) return;
  const int i = row * a.W + col;
  float r;
  const float3 me = full_point(a, i, &r);
  const int first = a.H - a.ground_rows;   // tested lower rows: first .. H - 1
  signed char g = 0;
  if (row >= first) {   // own test (lower = row, upper = row - 1; row >= 1 since ground_rows < H)
    const float3 up = full_point(a, i - a.W, nullptr);
    const int t = ground_test(me, up, a.mount, a.thr);
    if (t != 0) g = (signed char)t;
  }
  if (g == 0 && row + 1 < a.H && row + 1 >= first) {   // the test below, which marks this pixel as its upper
    const float3 lo = full_point(a, i + a.W, nullptr);
    if (ground_test(lo, me, a.mount, a.thr) == 1) g = 1;
  }
  a.range[i] = r;
  if (a.zout) a.zout[i] = reinterpret_cast<const float*>(a.raw + (size_t)i * a.stride)[2];
  a.ground[i] = g;
  a.label[i] = (g == 1 || r == 0.f) ? DDLO_SEG_EXCLUDED : DDLO_SEG_UNLABELLED;
}

inline int cdiv_s(long a, long b) { return (int)((a + b - 1) / b); }

// cloudSegmentation + labelComponents (detection.cpp:510-724) over host images.
struct Labeller {
  const ddlo_seg_params& p;
  const float* range;     // H x W
  const float* z;         // H x W: cloud_in_t z
  const float* resid;     // H x W or nullptr (icp_residuals_set_ false)
  int* label;             // H x W, in: -1 / 0
  float sin_x, cos_x, sin_y, cos_y, sensor_z;
  // the angle test without atan2 away from the threshold (EdgeTrig, seg_label.hpp)
  double tan_lo = 0.0, tan_hi = 0.0;
  bool tan_ok = false;
  int label_count = 1;
  std::vector<double>& avg_residual;   // by label
  std::vector<int>& qy;
  std::vector<int>& qx;
  std::vector<int>& py;
  std::vector<int>& px;
  std::vector<int>& rows_hit;
  std::vector<char>& line_flag;
  std::vector<int>& seg_off;
  std::vector<int>& seg_pix;

  Labeller(const ddlo_seg_params& p_, const float* range_, const float* z_, const float* resid_, int* label_,
           float sensor_z_, std::vector<double>& avg, LabelWork& w)
      : p(p_), range(range_), z(z_), resid(resid_), label(label_), sensor_z(sensor_z_), avg_residual(avg), qy(w.qy),
        qx(w.qx), py(w.py), px(w.px), rows_hit(w.rows_hit), line_flag(w.line_flag), seg_off(w.seg_off), seg_pix(w.seg_pix) {
    const int H = p.rows, W = p.cols;
    const EdgeTrig t = edge_trig(p);   // (seg_label.hpp: shared with the device labelling)
    sin_x = t.sin_x;
    cos_x = t.cos_x;
    sin_y = t.sin_y;
    cos_y = t.cos_y;
    tan_ok = t.tan_ok != 0;
    tan_lo = t.tan_lo;
    tan_hi = t.tan_hi;
    const size_t n = (size_t)H * W;
    if (qy.size() < n) {   // (grown once; every slot is written before it is read)
      qy.resize(n);
      qx.resize(n);
      py.resize(n);
      px.resize(n);
    }
    if (line_flag.size() != (size_t)H) line_flag.assign(H, 0);
    rows_hit.clear();
    rows_hit.reserve(H);
    avg_residual.assign(1, 0.0);
    seg_off.assign(2, 0);
    seg_pix.clear();
  }

  bool in_window(int r, int c) const { return r >= p.win_row0 && r <= p.win_row1 && c >= p.win_col0 && c <= p.win_col1; }

  void run() {
    // seeds in row-major order inside the window (:519-522)
    const int r0 = std::max(0, p.win_row0), r1 = std::min(p.rows - 1, p.win_row1);
    const int c0 = std::max(0, p.win_col0), c1 = std::min(p.cols - 1, p.win_col1);
    for (int i = r0; i <= r1; ++i)
      for (int j = c0; j <= c1; ++j)
        if (label[(size_t)i * p.cols + j] == 0) component(i, j);
  }

  void component(int row, int col) {
    const int H = p.rows, W = p.cols;
    int head = 0, tail = 1;
    qy[0] = row;
    qx[0] = col;
    float min_z = 1e6f, max_z = -1e6f, min_dist = 1e6f, max_dist = -1e6f, total_res = 0.f;
    int res_count = 0;
    py[0] = row;
    px[0] = col;
    int pushed = 1;
    static const int dr[4] = {-1, 0, 0, 1}, dc[4] = {0, 1, -1, 0};   // neighbor_iterator_ (:133-145)
    while (head < tail) {
      const int fy = qy[head], fx = qx[head];
      ++head;
      label[(size_t)fy * W + fx] = label_count;
      for (int k = 0; k < 4; ++k) {
        const int ty = fy + dr[k];
        int tx = fx + dc[k];
        if (ty < 0 || ty >= H) continue;
        if (!in_window(ty, tx)) continue;   // (size_t) compare in the reference: negative never passes
        if (tx < 0) tx = W - 1;             // wrap after the window test, as :598-601
        if (tx >= W) tx = 0;
        const size_t t = (size_t)ty * W + tx, f = (size_t)fy * W + fx;
        if (label[t] != 0) continue;
        const float d1 = std::max(range[f], range[t]);
        const float d2 = std::min(range[f], range[t]);
        const float sa = dr[k] == 0 ? sin_x : sin_y, ca = dr[k] == 0 ? cos_x : cos_y;
        const float y = d2 * sa, x = d1 - d2 * ca;
        bool pass;
        const double ratio = x > 0.f ? (double)y / (double)x : 0.0;
        if (tan_ok && x > 0.f && ratio > tan_hi) pass = true;
        else if (tan_ok && x > 0.f && ratio < tan_lo) pass = false;
        else pass = std::atan2(y, x) > p.theta;
        if (pass) {
          const double zz = z[t];
          if (zz < min_z && zz != 0) min_z = (float)zz;
          else if (zz > max_z) max_z = (float)zz;
          min_dist = std::min(min_dist, std::min(d1, d2));
          max_dist = std::max(max_dist, std::max(d1, d2));
          qy[tail] = ty;
          qx[tail] = tx;
          ++tail;
          label[t] = label_count;
          if (!line_flag[ty]) {
            line_flag[ty] = 1;
            rows_hit.push_back(ty);
          }
          py[pushed] = ty;
          px[pushed] = tx;
          ++pushed;
          if (resid && resid[t] > 0) {
            total_res += resid[t];
            ++res_count;
          }
        }
      }
    }
    const int lines = (int)rows_hit.size();
    for (int r : rows_hit) line_flag[r] = 0;
    rows_hit.clear();
    (void)min_dist;
    bool feasible = false;
    if (pushed >= 50 && lines >= p.min_line_num) feasible = true;
    else if (pushed >= p.valid_point_num && lines >= p.valid_line_num) feasible = true;
    if (feasible) feasible = max_dist <= p.max_distance;
    if (feasible) {
      const float dz = max_z - min_z;
      feasible = p.min_delta_z <= dz && dz <= p.max_delta_z;
    }
    // avg_residuum = res_count > 0 ? total_residuum / res_count : 0 — a float
    // quotient (float / int, float / int conditional), stored as double
    double avg = 0.0;
    if (feasible && resid) avg = (double)(res_count > 0 ? total_res / (float)res_count : 0.f);
    if (feasible) feasible = min_z - sensor_z <= p.max_elevation;
    if (feasible) {
      avg_residual.push_back(avg);   // avg_residuals_[label_count_]
      for (int i = 0; i < pushed; ++i) seg_pix.push_back(py[i] * W + px[i]);
      seg_off.push_back((int)seg_pix.size());
      ++label_count;
    } else {
      for (int i = 0; i < pushed; ++i) label[(size_t)py[i] * W + px[i]] = kRejected;
    }
  }
};

gicp_status check_params(const ddlo_seg_params* p) {
  if (!p) return fail(GICP_EINVAL, "null params");
  if (p->rows < 2 || p->cols < 1 || (long)p->rows * p->cols > INT32_MAX / 4) return fail(GICP_EINVAL, "invalid image size");
  if (p->ground_rows < 0 || p->ground_rows >= p->rows) return fail(GICP_EINVAL, "ground_rows must be in [0, rows)");
  return GICP_OK;
}

// ---- objects: one oriented bounding box per segment (getObject, detection.cpp:726-782) ----
// One workgroup per segment, over the segment's pixel list (the labelling
// records it; ddlo_seg_objects_from derives it from the label image), three
// times:
//   1. sum x, sum y, min / max z                   -> the centroid
//   2. the centred 2 x 2 covariance of (x, y)      -> the principal axes, in
//      closed form (every lane computes the same values from the same sums)
//   3. min / max of the points projected on them   -> centre and dimensions
// Sums are doubles reduced in a fixed order: each thread adds its pixels in
// list order (thread t takes entries t, t + 1024, ...), the wavefront folds by
// shuffles, the sixteen wavefront sums are added 0..15 from LDS.  No atomics:
// the result does not depend on the grid or on timing, only on the list's
// order.  The kernel is bound by the latency of its dependent loads (list
// entry, then point), so the workgroup is as wide as it can be: a 6000-point
// segment is six rounds per pass.  (Measured on a 512 x 512 frame's ten
// segments: 37 us with 256 threads; 194 us for a first version that walked
// the segment's rows of the label image instead of a list.)
constexpr int kObjThreads = 1024;

struct SegObjArgs {
  const unsigned char* raw;
  size_t stride;
  const int* off;         // CSR: segment l's pixels are pix[off[l] .. off[l + 1])
  const int* pix;         // row-major pixel indices
  ddlo_seg_object* out;   // [l - 1]
};

struct OpSum {
  __device__ static double f(double a, double b) { return a + b; }
};
struct OpMax {
  __device__ static double f(double a, double b) { return fmax(a, b); }
};

// v[k] <- the block's reduction of v[k], in every thread
template <class Op, int K>
__device__ __forceinline__ void block_reduce(double (&v)[K], double (*sh)[kObjThreads / 64]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v[k] = Op::f(v[k], __shfl_down(v[k], d, 64));
  __syncthreads();   // the previous reduction's readers are done with sh
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k][w] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double r = sh[k][0];
#pragma unroll
    for (int j = 1; j < kObjThreads / 64; ++j) r = Op::f(r, sh[k][j]);
    v[k] = r;
  }
}

__global__ __launch_bounds__(kObjThreads) void k_seg_objects(SegObjArgs a) {
  __shared__ double sh[4][kObjThreads / 64];
  const int l = blockIdx.x + 1;
  ddlo_seg_object* const out = a.out + blockIdx.x;
  const int first = a.off[l], last = a.off[l + 1];   // (first == last: no pixel, the loops do not run)
  auto point = [&](int i) { return reinterpret_cast<const float*>(a.raw + (size_t)a.pix[i] * a.stride); };
  // 1. centroid, z range (float min / max are exact in any order)
  const int cnt = last - first;
  if (cnt == 0) {   // (uniform)
    if (threadIdx.x == 0) {
      out->id = l;
      out->num_points = 0;
    }
    return;
  }
  double s1[2] = {0.0, 0.0};             // sum x, sum y
  double zr[2] = {-INFINITY, -INFINITY}; // max z, max -z
  for (int i = first + (int)threadIdx.x; i < last; i += kObjThreads) {
    const float* p = point(i);
    s1[0] += (double)p[0];
    s1[1] += (double)p[1];
    zr[0] = fmax(zr[0], (double)p[2]);
    zr[1] = fmax(zr[1], -(double)p[2]);
  }
  block_reduce<OpSum>(s1, sh);
  block_reduce<OpMax>(zr, sh);
  const double cx = s1[0] / (double)cnt, cy = s1[1] / (double)cnt;
  // 2. centred covariance (its scale does not matter to the axes)
  double s2[3] = {0.0, 0.0, 0.0};
  for (int i = first + (int)threadIdx.x; i < last; i += kObjThreads) {
    const float* p = point(i);
    const double dx = (double)p[0] - cx, dy = (double)p[1] - cy;
    s2[0] += dx * dx;
    s2[1] += dx * dy;
    s2[2] += dy * dy;
  }
  block_reduce<OpSum>(s2, sh);
  // symmetric 2 x 2 [[cxx, cxy], [cxy, cyy]]: the major axis is (d + h, 2 cxy)
  // for d = cxx - cyy >= 0, (2 cxy, h - d) otherwise, h = hypot(d, 2 cxy); the
  // minor axis is its normal.  h == 0: equal eigenvalues, axis (1, 0).
  double ax = 1.0, ay = 0.0;
  {
    const double d = s2[0] - s2[2], b2 = 2.0 * s2[1];
    const double h = sqrt(d * d + b2 * b2);
    if (h > 0.0) {
      const double mx = d >= 0.0 ? d + h : b2, my = d >= 0.0 ? b2 : h - d;
      const double nrm = sqrt(mx * mx + my * my);
      ax = -my / nrm;
      ay = mx / nrm;
      if (ax < 0.0 || (ax == 0.0 && ay < 0.0)) {
        ax = -ax;
        ay = -ay;
      }
    }
  }
  // 3. extent along the axes (axis, then (-axis.y, axis.x)), about the centroid
  double e[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};   // max u, max -u, max v, max -v
  for (int i = first + (int)threadIdx.x; i < last; i += kObjThreads) {
    const float* p = point(i);
    const double dx = (double)p[0] - cx, dy = (double)p[1] - cy;
    const double u = ax * dx + ay * dy, v = ax * dy - ay * dx;
    e[0] = fmax(e[0], u);
    e[1] = fmax(e[1], -u);
    e[2] = fmax(e[2], v);
    e[3] = fmax(e[3], -v);
  }
  block_reduce<OpMax>(e, sh);
  if (threadIdx.x != 0) return;
  const double umax = e[0], umin = -e[1], vmax = e[2], vmin = -e[3];
  const double mu = 0.5 * (umax + umin), mv = 0.5 * (vmax + vmin);
  const double du = umax - umin, dv = vmax - vmin;
  const float zmax = (float)zr[0], zmin = (float)-zr[1];
  const float dz = zmax - zmin;
  out->id = l;
  out->num_points = cnt;
  out->state[0] = (float)((ax * mu - ay * mv) + cx);   // eigen_vectors_PCA * mean_XY + centroid
  out->state[1] = (float)((ay * mu + ax * mv) + cy);
  out->state[2] = 0.5f * (zmax + zmin);
  // sin(atan2(ay, ax) / 2) with ax >= 0: sin(t / 2) = sin t / sqrt(2 (1 + cos t))
  out->state[3] = (float)(ay / sqrt(2.0 * (1.0 + ax)));
  out->state[4] = (float)du;
  out->state[5] = (float)dv;
  out->state[6] = dz;
  out->axis[0] = (float)ax;
  out->axis[1] = (float)ay;
  out->density = (float)((double)cnt / ((du * dv) * (double)dz));
  out->avg_residuum = 0.0;   // the host fills it in
}

// the pixels of the removed segments made NaN in the packed scan: the crop
// box / voxel pass drops non-finite points, so the removal, the finite test
// and the crop are one keep predicate there
// w = kRemovedW marks the pixel as removed (a no-return pixel is NaN with the
// w = 0 the pack gave it): the row/column filter's keyframe pass tells them
// apart.  A pixel named twice gets the same bits twice.
// FLAGS (ddlo_seg_set_intensity with the row/column filter on: w is the channel, of a kept pixel any
// value and of a no-return pixel too): the mark is a byte of the pixel's instead, and w is left 0.
template <bool FLAGS>
__global__ __launch_bounds__(256) void k_static_drop(const int* __restrict__ pix, int m, float4* __restrict__ pts,
                                                     unsigned char* __restrict__ flags) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  pts[pix[j]] = make_float4(NAN, NAN, NAN, FLAGS ? 0.f : kRemovedW);
  if (FLAGS) flags[pix[j]] = 1;
}

// ---- the row/column filter's keyframe pass (odom.cc:902-906) ----------------
// The reference extracts the non-static pixels without keep-organized and
// then runs the filter of the registration pass, with its absolute index set
// S, over the compacted cloud of n' points: the point at position j stays if j
// is in S.  Pixel p, if not removed, has position j = p - (removed pixels
// before p); a no-return pixel keeps its position.  Two launches, a workgroup
// of kDsThreads per kDsThreads consecutive pixels, one pixel per thread:
//   k_ds_count  the removed pixels of every workgroup's pixels -> part[workgroup]
//   k_ds_keep   every workgroup sums part (the workgroups before it: its
//               offset; all of them: n' = n - total, and with it the |S| <= n'
//               decision, taken here by every workgroup alike), ranks its own
//               pixels and writes the verdicts: keep_out[p] (the debug entry),
//               or NaN over the points that leave (pts; the crop box / voxel
//               pass drops them).
// Within a workgroup: one 64-bit ballot gives a lane the removed pixels before
// it in its wavefront, the four wavefront totals go through LDS.  Every lane
// reaches the ballot and the shuffles (a pixel past n counts as not removed).
// Integer arithmetic throughout: exact for any number of workgroups.  Each
// workgroup reads all of part: quadratic in the workgroups, a few hundred for
// the images this runs on, where exactness matters and speed does not.
constexpr int kDsThreads = 256, kDsWaves = kDsThreads / 64;

// whether this thread's pixel was removed; *before = the removed pixels of the workgroup's before
// it, *total = all of them.  sh: kDsWaves ints.
__device__ bool ds_block_rank(const unsigned char* __restrict__ flags, const float4* __restrict__ pts, int n, int* sh,
                              int* before, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * kDsThreads + threadIdx.x;
  const bool removed = p < n && (flags ? flags[p] != 0 : pts[p].w != 0.f);
  const unsigned long long b = __ballot(removed);
  if (lane == 0) sh[wave] = __popcll(b);
  __syncthreads();
  int run = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
  for (int w = 0; w < kDsWaves; ++w) {
    if (w < wave) run += sh[w];
    all += sh[w];
  }
  *before = run;
  *total = all;
  return removed;
}

__global__ __launch_bounds__(kDsThreads) void k_ds_count(const unsigned char* __restrict__ flags,
                                                         const float4* __restrict__ pts, int n, int* __restrict__ part) {
  __shared__ int sh[kDsWaves];
  int before, total;
  (void)ds_block_rank(flags, pts, n, sh, &before, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// ctrl[0] = 1 if |S| > n' (nothing filtered), ctrl[1] = the removed pixels
__global__ __launch_bounds__(kDsThreads) void k_ds_keep(const unsigned char* __restrict__ flags, float4* __restrict__ pts,
                                                        int n, const int* __restrict__ part, int W, int row_step,
                                                        int col_step, long long s_size,
                                                        unsigned char* __restrict__ keep_out, int* __restrict__ ctrl) {
  __shared__ int sh[kDsWaves];
  __shared__ int sums[2][kDsWaves];
  // the removed pixels of the workgroups before this one, and of all
  int lo = 0, all = 0;
  for (int b = threadIdx.x; b < (int)gridDim.x; b += kDsThreads) {
    const int v = part[b];
    all += v;
    if (b < (int)blockIdx.x) lo += v;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    lo += __shfl_down(lo, d);
    all += __shfl_down(all, d);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sums[0][wave] = lo;
    sums[1][wave] = all;
  }
  __syncthreads();
  lo = all = 0;
#pragma unroll
  for (int w = 0; w < kDsWaves; ++w) {
    lo += sums[0][w];
    all += sums[1][w];
  }
  const bool skip = s_size > (long long)(n - all);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctrl[0] = skip ? 1 : 0;
    ctrl[1] = all;
  }
  int before, total;
  const bool removed = ds_block_rank(flags, pts, n, sh, &before, &total);
  const int p = blockIdx.x * kDsThreads + threadIdx.x;
  if (p >= n) return;
  const int j = p - (lo + before);
  const bool stays = !removed && (skip || ((j / W) % row_step == 0 && (j % W) % col_step == 0));
  if (keep_out) keep_out[p] = stays ? 1 : 0;
  else if (!removed && !stays) pts[p] = make_float4(NAN, NAN, NAN, 0.f);
}

inline int ds_blocks(int n) { return (int)(((long)n + kDsThreads - 1) / kDsThreads); }
size_t downsample_scratch_ints(int n) { return (size_t)ds_blocks(n) + 2; }

// flags (n bytes) or, if null, the w of pts mark the removed pixels; scratch: downsample_scratch_ints(n)
// ints, the control words last (returned).  keep_out null: the pixels that leave become NaN in pts.
int* launch_downsample_keep(hipStream_t s, const unsigned char* flags, float4* pts, int n, int rows, int cols,
                            int row_step, int col_step, unsigned char* keep_out, int* scratch) {
  const int blocks = ds_blocks(n);
  int* const ctrl = scratch + blocks;
  k_ds_count<<<blocks, kDsThreads, 0, s>>>(flags, pts, n, scratch);
  k_ds_keep<<<blocks, kDsThreads, 0, s>>>(flags, pts, n, scratch, cols, row_step, col_step,
                                          rowcol_size(rows, cols, row_step, col_step), keep_out, ctrl);
  return ctrl;
}

// computeAllObjects' ratio test (:800-804) and avg_residuals_ on the kernel's records
void filter_objects(const std::vector<ddlo_seg_object>& recs, const double* avg, size_t avg_n, float max_dim_ratio,
                    std::vector<ddlo_seg_object>& out) {
  out.clear();
  for (const ddlo_seg_object& r : recs) {
    if (r.num_points <= 0) continue;
    double d[3] = {r.state[4], r.state[5], r.state[6]};
    std::sort(d, d + 3);
    if (d[2] / d[1] >= max_dim_ratio) continue;
    ddlo_seg_object o = r;
    o.avg_residuum = (avg && (size_t)r.id < avg_n) ? avg[r.id] : 0.0;
    out.push_back(o);
  }
}

// the segments' rows for k_seg_objects and k_trk_gather: the L + 2 offsets,
// then the pixel lists (CSR, as ddlo_seg_label_indices), joined in rows
// (staging of the caller's, off[L + 1] + L + 2 ints) and sent up in one copy
gicp_status upload_csr(hipStream_t s, const std::vector<int>& off, const std::vector<int>& pix, int L, DevBuf& dcsr,
                       int* rows) {
  const size_t noff = (size_t)L + 2, npix = (size_t)off[L + 1];
  HIP_TRY(dcsr.ensure(sizeof(int) * (noff + npix)));
  std::memcpy(rows, off.data(), sizeof(int) * noff);
  if (npix) std::memcpy(rows + noff, pix.data(), sizeof(int) * npix);
  HIP_TRY(hipMemcpyAsync(dcsr.p, rows, sizeof(int) * (noff + npix), hipMemcpyHostToDevice, s));
  return GICP_OK;
}

// where the records of L segments come back to in the pinned block that staged their rows
size_t rec_offset(const std::vector<int>& off, int L) {
  return (sizeof(int) * ((size_t)L + 2 + (size_t)off[L + 1]) + 63) / 64 * 64;
}

// launch the object kernel for labels 1 .. L over a CSR on the device and read
// the records back: through rec_pin (pinned, L records), or with a pageable
// copy when it is nullptr
gicp_status run_objects(hipStream_t s, const unsigned char* raw, size_t stride, const int* off, const int* pix, int L,
                        DevBuf& dobj, std::vector<ddlo_seg_object>& recs, void* rec_pin) {
  const size_t rec_b = sizeof(ddlo_seg_object) * (size_t)L;
  HIP_TRY(dobj.ensure(rec_b));
  SegObjArgs a{raw, stride, off, pix, dobj.as<ddlo_seg_object>()};
  k_seg_objects<<<L, kObjThreads, 0, s>>>(a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(rec_pin ? rec_pin : recs.data(), dobj.p, rec_b, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (rec_pin) std::memcpy(recs.data(), rec_pin, rec_b);
  return GICP_OK;
}

// every label's pixels, row-major within a label (:527-537), as CSR: a
// counting sort of the label image (labels 1 .. L), in its two passes: the
// L + 2 offsets, then the off[L + 1] pixels
void label_csr_offsets(const int32_t* label, size_t n, int L, std::vector<int32_t>& off) {
  off.assign((size_t)L + 2, 0);
  for (size_t i = 0; i < n; ++i) {
    const int l = label[i];
    if (l > 0 && l != kRejected) ++off[l + 1];
  }
  for (int l = 1; l <= L + 1; ++l) off[l] += off[l - 1];
}
void label_csr_pixels(const int32_t* label, size_t n, const std::vector<int32_t>& off, int32_t* pix) {
  std::vector<int32_t> at(off.begin(), off.end() - 1);
  for (size_t i = 0; i < n; ++i) {
    const int l = label[i];
    if (l > 0 && l != kRejected) pix[at[l]++] = (int32_t)i;
  }
}

}  // namespace

gicp_status seg_check_params(const ddlo_seg_params* p) { return check_params(p); }

}  // namespace ddlo

using namespace ddlo;

// the pinned record: the ints and the first averages in one copy
constexpr size_t kRecPinBytes = kLabelRecMinBytes;
constexpr size_t kRecPinAvg = (kRecPinBytes - sizeof(int) * kLabelRecInts) / sizeof(double);

namespace ddlo {

gicp_status fetch_images(ddlo_seg* o, unsigned want) {
  if (o->labelling != DDLO_SEG_LABEL_DEVICE) return GICP_OK;
  const unsigned need = want & ~o->fetched;
  if (!need) return GICP_OK;
  const size_t n = o->hn;
  HIP_TRY(hipSetDevice(o->device));
  if (need & kImgRange)
    HIP_TRY(hipMemcpyAsync(const_cast<float*>(o->h_range), o->range.p, sizeof(float) * n, hipMemcpyDeviceToHost, o->s));
  if (need & kImgGround)
    HIP_TRY(hipMemcpyAsync(const_cast<signed char*>(o->h_ground), o->ground.p, n, hipMemcpyDeviceToHost, o->s));
  if (need & kImgLabel) HIP_TRY(hipMemcpyAsync(o->h_label, o->label.p, sizeof(int) * n, hipMemcpyDeviceToHost, o->s));
  HIP_TRY(hipStreamSynchronize(o->s));
  o->fetched |= need;
  return GICP_OK;
}

}  // namespace ddlo

extern "C" {

gicp_status ddlo_seg_default_params(ddlo_seg_params* p) {
  if (!p) return fail(GICP_EINVAL, "null params");
  std::memset(p, 0, sizeof(*p));
  p->rows = 128;
  p->cols = 1024;
  p->ang_bottom = 45.f;
  p->ground_rows = 30;
  p->ground_angle_threshold = 10.f;
  p->minimum_range = 10.f;
  p->sensor_mount_angle = 10.f;
  p->theta = (float)(60.0 / 180.0 * M_PI);
  p->valid_point_num = 15;
  p->min_line_num = 5;
  p->valid_line_num = 5;
  p->min_delta_z = 0.1f;
  p->max_delta_z = 3.0f;
  p->max_distance = 20.f;
  p->max_elevation = 2.0f;
  p->win_row0 = p->win_col0 = 156;
  p->win_row1 = p->win_col1 = 356;
  return GICP_OK;
}

gicp_status ddlo_seg_create(int device, const ddlo_seg_params* p, ddlo_seg** out) {
  if (!out) return fail(GICP_EINVAL, "null out");
  *out = nullptr;
  auto o = std::make_unique<ddlo_seg>();
  if (p) o->p = *p;
  else ddlo_seg_default_params(&o->p);
  if (gicp_status st = check_params(&o->p)) return st;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(GICP_EHIP, "no HIP device " + std::to_string(device) + " (HIP library present, device not visible)");
  o->device = device;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreateWithFlags(&o->s, hipStreamNonBlocking));
  const size_t n = (size_t)o->p.rows * o->p.cols;
  if (o->pin.reset(n * (sizeof(float) + sizeof(int) + sizeof(float)) + n) != hipSuccess ||
      o->cnt_pin.reset(sizeof(int) * 20) != hipSuccess) {
    (void)hipStreamDestroy(o->s);
    return fail(GICP_EHIP, "pinned allocation failed");
  }
  *out = o.release();
  return GICP_OK;
}

gicp_status ddlo_seg_destroy(ddlo_seg* s) {
  if (!s) return GICP_OK;
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(s->s);
  (void)hipStreamDestroy(s->s);
  delete s;   // (the buffers and the parts: their owners' destructors)
  return GICP_OK;
}

}  // extern "C"

// the pinned read-back images of a handle: range | label | z (staged scans) | ground
struct HostImages {
  float* range;
  int* label;
  float* z;
  signed char* ground;
};
static HostImages host_images(const ddlo_seg* o, size_t n) {
  HostImages h;
  h.range = o->pin.as<float>();
  h.label = reinterpret_cast<int*>(h.range + n);
  h.z = reinterpret_cast<float*>(h.label + n);
  h.ground = reinterpret_cast<signed char*>(h.z + n);
  return h;
}

// seg_run's tail in device mode: the labelling reads z from the scan itself;
// only the record comes back: the counts and the first averages, then the
// other averages if there are more
static gicp_status label_tail_device(ddlo_seg* o, size_t n, const float T[16], const float* residual, ddlo_seg_result* r) {
  const float* dres = nullptr;
  if (residual) {
    HIP_TRY(rt::grow(o->dresid, sizeof(float) * n, o->s));
    HIP_TRY(hipMemcpyAsync(o->dresid.p, residual, sizeof(float) * n, hipMemcpyHostToDevice, o->s));
    dres = o->dresid.as<float>();
  }
  const LabelDevIn in{o->range.as<float>(), o->raw.as<unsigned char>() + 8, o->raw_stride, dres,
                      o->ground.as<signed char>(), o->label.as<int>(), T[11]};
  if (gicp_status st = label_device_run(o->s, o->p, o->ldev, in)) return st;
  HIP_TRY(hipMemcpyAsync(o->rec_pin.p, o->ldev.rec.p, kRecPinBytes, hipMemcpyDeviceToHost, o->s));
  HIP_TRY(hipStreamSynchronize(o->s));
  const int* ri = o->rec_pin.as<int>();
  if (ri[kRecError]) return fail(GICP_EHIP, "device labelling: a replay queue left its component's range");
  const size_t navg = (size_t)ri[kRecSegments] + 1;
  o->avg.assign(navg, 0.0);
  const double* pavg = reinterpret_cast<const double*>(ri + kLabelRecInts);
  for (size_t l = 0; l < navg && l < kRecPinAvg; ++l) o->avg[l] = pavg[l];
  if (navg > kRecPinAvg) {
    HIP_TRY(hipMemcpyAsync(o->avg.data() + kRecPinAvg, o->ldev.avg() + kRecPinAvg, sizeof(double) * (navg - kRecPinAvg),
                           hipMemcpyDeviceToHost, o->s));
    HIP_TRY(hipStreamSynchronize(o->s));
  }
  o->fetched = 0;
  o->replayed = ri[kRecReplayed];
  o->longest_prefix = ri[kRecLongestPrefix];
  *r = ddlo_seg_result{ri[kRecSegments], ri[kRecGround], ri[kRecRange], ri[kRecRejected]};
  return GICP_OK;
}

// seg_run's tail in host mode: the images come back and the reference's search
// runs over them.  It reads cloud_in_t z (:629): gathered from xyz_t while the
// device works, or (a staged scan) read back with the images from o->zimg.
static gicp_status label_tail_host(ddlo_seg* o, size_t n, const HostImages& h, const float* xyz_t, const float T[16],
                                   const float* residual, ddlo_seg_result* r) {
  HIP_TRY(hipMemcpyAsync(h.range, o->range.p, sizeof(float) * n, hipMemcpyDeviceToHost, o->s));
  HIP_TRY(hipMemcpyAsync(h.label, o->label.p, sizeof(int) * n, hipMemcpyDeviceToHost, o->s));
  HIP_TRY(hipMemcpyAsync(h.ground, o->ground.p, n, hipMemcpyDeviceToHost, o->s));
  const float* zsrc = h.z;
  if (xyz_t) {
    o->z.resize(n);
    const unsigned char* b = reinterpret_cast<const unsigned char*>(xyz_t);
    const size_t stride = o->raw_stride;
    for (size_t i = 0; i < n; ++i) std::memcpy(&o->z[i], b + i * stride + 8, sizeof(float));
    zsrc = o->z.data();
  } else {
    HIP_TRY(hipMemcpyAsync(h.z, o->zimg.p, sizeof(float) * n, hipMemcpyDeviceToHost, o->s));
  }
  HIP_TRY(hipStreamSynchronize(o->s));
  Labeller lb(o->p, h.range, zsrc, residual, h.label, T[11], o->avg, o->work);
  lb.run();
  ddlo_seg_result c{};   // (a local: the counting loop keeps its sums in registers)
  c.segments = lb.label_count - 1;
  for (size_t i = 0; i < n; ++i) {
    c.ground_pixels += h.ground[i] == 1;
    c.range_pixels += h.range[i] > 0.f;
    c.rejected_pixels += h.label[i] == kRejected;
  }
  *r = c;
  return GICP_OK;
}

// ddlo_seg_process; xyz_t == nullptr: the scan is already in o->raw (seg_stage_input)
static gicp_status seg_run(ddlo_seg* o, const float* xyz_t, size_t stride, const float T[16], const float* residual,
                           ddlo_seg_result* res) {
  const ddlo_seg_params& p = o->p;
  const int H = p.rows, W = p.cols;
  const size_t n = (size_t)H * W;
  HIP_TRY(hipSetDevice(o->device));
  o->have = false;   // until the end: every error return leaves the handle without a scan
  o->have_objects = false;
  o->csr_ready = o->csr_len_ready = false;
  ++o->scan_serial;
  const size_t ioff = xyz_t && o->inten_use ? o->inten_off : 0;
  const size_t raw_sz = (n - 1) * stride + std::max<size_t>(12, ioff ? ioff + 4 : 0);
  HIP_TRY(o->raw.ensure(raw_sz));
  o->raw_stride = stride;
  o->raw_staged = !xyz_t;
  o->raw_inten_off = ioff;
  HIP_TRY(o->range.ensure(sizeof(float) * n));
  HIP_TRY(o->ground.ensure(n));
  HIP_TRY(o->label.ensure(sizeof(int) * n));
  const bool dev_label = o->labelling == DDLO_SEG_LABEL_DEVICE;
  // a staged scan's z reaches the host labelling as an image of its own
  // (xyz_t: gathered on the host; device labelling: read from the scan)
  const bool z_image = !xyz_t && !dev_label;
  if (xyz_t) HIP_TRY(hipMemcpyAsync(o->raw.p, xyz_t, raw_sz, hipMemcpyHostToDevice, o->s));
  if (z_image) HIP_TRY(o->zimg.ensure(sizeof(float) * n));
  SegPixelArgs a{};
  a.raw = o->raw.as<unsigned char>();
  a.stride = stride;
  a.H = H;
  a.W = W;
  a.x0 = -T[3];   // projectScan: sensor position = T(0:3, 3) (:296-298)
  a.y0 = -T[7];
  a.z0 = -T[11];
  a.min_range = p.minimum_range;
  a.ground_rows = p.ground_rows;
  a.mount = p.sensor_mount_angle;
  a.thr = p.ground_angle_threshold;
  a.range = o->range.as<float>();
  a.ground = o->ground.as<signed char>();
  a.label = o->label.as<int>();
  a.zout = z_image ? o->zimg.as<float>() : nullptr;
  k_seg_pixels<<<dim3(cdiv_s(W, 256), H), 256, 0, o->s>>>(a);
  HIP_TRY(hipGetLastError());
  const HostImages h = host_images(o, n);
  ddlo_seg_result r{};
  if (gicp_status st = dev_label ? label_tail_device(o, n, T, residual, &r)
                                 : label_tail_host(o, n, h, xyz_t, T, residual, &r))
    return st;
  o->h_range = h.range;
  o->h_ground = h.ground;
  o->h_label = h.label;
  o->hn = n;
  o->last = r;
  o->have = true;
  if (res) *res = r;
  return GICP_OK;
}

extern "C" {

gicp_status ddlo_seg_process(ddlo_seg* o, const float* xyz_t, size_t stride, const float T[16], const float* residual,
                             ddlo_seg_result* res) {
  if (!o || !xyz_t || !T || stride < 12 || stride % 4) return fail(GICP_EINVAL, "invalid argument");
  if (o->inten_use && (o->inten_off % 4 || o->inten_off < 12 || o->inten_off + 4 > stride))
    return fail(GICP_EINVAL, "intensity offset: a multiple of 4, >= 12 and offset + 4 <= stride");
  return seg_run(o, xyz_t, stride, T, residual, res);
}

gicp_status ddlo_seg_images(ddlo_seg* o, float* range, int8_t* ground, int32_t* label) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (!o->have) return fail(GICP_EINVAL, "no processed scan");
  if (gicp_status st = fetch_images(o, (range ? kImgRange : 0u) | (ground ? kImgGround : 0u) | (label ? kImgLabel : 0u)))
    return st;
  const size_t n = o->hn;
  if (range) std::memcpy(range, o->h_range, sizeof(float) * n);
  if (ground) std::memcpy(ground, o->h_ground, n);
  if (label) std::memcpy(label, o->h_label, sizeof(int) * n);
  return GICP_OK;
}

gicp_status ddlo_seg_avg_residuals(ddlo_seg* o, double* out, size_t cap, size_t* n) {
  if (!o || (!out && cap)) return fail(GICP_EINVAL, "invalid argument");
  if (!o->have) return fail(GICP_EINVAL, "no processed scan");
  for (size_t l = 0; l < cap && l < o->avg.size(); ++l) out[l] = o->avg[l];
  if (n) *n = o->avg.size();
  return GICP_OK;
}

gicp_status ddlo_seg_ground_indices(ddlo_seg* o, int32_t* out, size_t cap, size_t* n) {
  if (!o || !n || (!out && cap)) return fail(GICP_EINVAL, "invalid argument");
  if (!o->have) return fail(GICP_EINVAL, "no processed scan");
  if (gicp_status st = fetch_images(o, kImgGround)) return st;
  const int H = o->p.rows, W = o->p.cols;
  size_t k = 0;
  for (int col = 0; col < W; ++col)
    for (int ri = 0; ri < o->p.ground_rows; ++ri) {
      const int row = H - 1 - ri;
      if (o->h_ground[(size_t)row * W + col] == 1) {
        if (k < cap) out[k] = row * W + col;
        ++k;
      }
    }
  *n = k;
  return GICP_OK;
}

gicp_status ddlo_seg_label_indices(ddlo_seg* o, int32_t* offsets, size_t offsets_cap, int32_t* indices,
                                   size_t indices_cap, size_t* n_indices) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (!o->have) return fail(GICP_EINVAL, "no processed scan");
  if (gicp_status st = fetch_images(o, kImgLabel)) return st;
  const int L = o->last.segments;
  if (offsets && offsets_cap < (size_t)L + 2) return fail(GICP_EINVAL, "offsets needs segments + 2 entries");
  std::vector<int32_t> cnt;
  label_csr_offsets(o->h_label, o->hn, L, cnt);
  const size_t total = (size_t)cnt[L + 1];
  if (n_indices) *n_indices = total;
  if (offsets) std::memcpy(offsets, cnt.data(), sizeof(int32_t) * (L + 2));
  if (indices) {
    if (indices_cap < total) return fail(GICP_EINVAL, "indices buffer too small");
    label_csr_pixels(o->h_label, o->hn, cnt, indices);
  }
  return GICP_OK;
}

gicp_status ddlo_seg_label(const ddlo_seg_params* p, const float* range, const float* z, const float* residual,
                           float sensor_z, int32_t* label, double* avg_residual, size_t avg_cap, int32_t* segments) {
  if (gicp_status st = check_params(p)) return st;
  if (!range || !z || !label || (!avg_residual && avg_cap)) return fail(GICP_EINVAL, "invalid argument");
  std::vector<double> avg;
  LabelWork work;
  Labeller lb(*p, range, z, residual, label, sensor_z, avg, work);
  lb.run();
  for (size_t l = 0; l < avg_cap; ++l) avg_residual[l] = l < avg.size() ? avg[l] : 0.0;
  if (segments) *segments = lb.label_count - 1;
  return GICP_OK;
}

}  // extern "C"

namespace ddlo {

int seg_device(const ddlo_seg* s) { return s->device; }

gicp_status seg_get_params(const ddlo_seg* s, ddlo_seg_params* out) {
  if (!s || !out) return fail(GICP_EINVAL, "null argument");
  *out = s->p;
  return GICP_OK;
}

gicp_status seg_stage_input(ddlo_seg* o, float4** buf, int* npix) {
  if (!o || !buf || !npix) return fail(GICP_EINVAL, "null argument");
  const size_t n = (size_t)o->p.rows * o->p.cols;
  HIP_TRY(hipSetDevice(o->device));
  o->have = false;   // the scan in raw is no longer the one the images belong to
  ++o->scan_serial;
  HIP_TRY(o->raw.ensure(sizeof(float4) * n));
  *buf = o->raw.as<float4>();
  *npix = (int)n;
  return GICP_OK;
}

gicp_status seg_process_staged(ddlo_seg* o, const float T[16], const float* residual, ddlo_seg_result* res) {
  if (!o || !T) return fail(GICP_EINVAL, "null argument");
  return seg_run(o, nullptr, sizeof(float4), T, residual, res);
}

// The last scan's L >= 1 segments as CSR on the device.  Device labelling: the
// labelling's own.  Host labelling: the labelling's lists joined and sent up
// into dcsr (enqueued, not waited for), once per scan, by whoever asks first;
// the rows are staged in obj_stage, which is sized here for the records that
// ddlo_seg_objects reads back behind them, so it does not move while the copy runs.
static gicp_status csr_pointers(ddlo_seg* o, const int** off, const int** pix) {
  if (o->labelling == DDLO_SEG_LABEL_DEVICE) {
    *off = o->ldev.off();
    *pix = o->ldev.pixels();
    return GICP_OK;
  }
  const int L = o->last.segments;
  if (!o->csr_ready) {
    HIP_TRY(o->obj_stage.ensure(rec_offset(o->work.seg_off, L) + sizeof(ddlo_seg_object) * (size_t)L));
    if (gicp_status st = upload_csr(o->s, o->work.seg_off, o->work.seg_pix, L, o->dcsr, o->obj_stage.as<int>())) return st;
    o->csr_ready = true;
  }
  *off = o->dcsr.as<int>();
  *pix = o->dcsr.as<int>() + L + 2;
  return GICP_OK;
}

gicp_status seg_csr(ddlo_seg* o, SegCsr* out) {
  if (!o || !out) return fail(GICP_EINVAL, "null argument");
  if (!o->have) return fail(GICP_EINVAL, "no processed scan");
  const int L = o->last.segments;
  *out = SegCsr{};
  out->L = L;
  if (L > 0) {
    HIP_TRY(hipSetDevice(o->device));
    if (gicp_status st = csr_pointers(o, &out->d_off, &out->d_pix)) return st;
  }
  if (!o->csr_len_ready) {
    std::vector<int>& len = o->csr_len;
    len.assign((size_t)L + 1, 0);
    if (o->labelling != DDLO_SEG_LABEL_DEVICE) {
      for (int l = 1; l <= L; ++l) len[l] = o->work.seg_off[l + 1] - o->work.seg_off[l];
    } else if (o->have_objects) {   // the object records carry every segment's length
      for (int l = 1; l <= L; ++l) len[l] = o->objects[(size_t)l - 1].num_points;
    } else if (L > 0) {
      std::vector<int> off((size_t)L + 2);
      HIP_TRY(hipMemcpyAsync(off.data(), o->ldev.off(), sizeof(int) * off.size(), hipMemcpyDeviceToHost, o->s));
      HIP_TRY(hipStreamSynchronize(o->s));
      for (int l = 1; l <= L; ++l) len[l] = off[l + 1] - off[l];
    }
    o->csr_len_ready = true;
  }
  out->len = o->csr_len.data();
  return GICP_OK;
}

gicp_status seg_objects_vec(ddlo_seg* o, float max_dim_ratio, std::vector<ddlo_seg_object>& out) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (!o->have) return fail(GICP_EINVAL, "no processed scan");
  HIP_TRY(hipSetDevice(o->device));
  if (!o->have_objects) {
    const int L = o->last.segments;
    o->objects.assign((size_t)L, ddlo_seg_object{});
    if (L > 0) {
      // the records come back through obj_stage: behind the rows it staged (host labelling), or at its start
      const bool dev_label = o->labelling == DDLO_SEG_LABEL_DEVICE;
      if (dev_label) HIP_TRY(o->obj_stage.ensure(sizeof(ddlo_seg_object) * (size_t)L));
      const int *off = nullptr, *pix = nullptr;
      if (gicp_status st = csr_pointers(o, &off, &pix)) return st;
      void* const rec_pin = o->obj_stage.as<char>() + (dev_label ? 0 : rec_offset(o->work.seg_off, L));
      if (gicp_status st = run_objects(o->s, o->raw.as<unsigned char>(), o->raw_stride, off, pix, L, o->dobj, o->objects, rec_pin))
        return st;
    }
    o->have_objects = true;
  }
  filter_objects(o->objects, o->avg.data(), o->avg.size(), max_dim_ratio, out);
  return GICP_OK;
}

gicp_status seg_static_begin(ddlo_seg* o, const float centre[3], const float4** pts, int* count) {
  if (!o || !pts || !count || !centre) return fail(GICP_EINVAL, "invalid argument");
  if (!o->have) return fail(GICP_EINVAL, "no processed scan");
  HIP_TRY(hipSetDevice(o->device));
  const int n = (int)o->hn;
  HIP_TRY(o->f4.ensure(sizeof(float4) * (size_t)n));
  HIP_TRY(o->f4b.ensure(sizeof(float4) * (size_t)n));
  HIP_TRY(o->keep.ensure(sizeof(int) * (size_t)n));
  HIP_TRY(o->pos.ensure(sizeof(int) * (size_t)n));
  HIP_TRY(o->vscratch.ensure(sizeof(int) * voxel_scratch_ints(n)));
  HIP_TRY(o->cubtmp.ensure(std::max(crop_box_tmp_bytes(n), voxel_tmp_bytes(n))));
  if (o->voxel_order != 0) HIP_TRY(o->voscratch.ensure(sizeof(int) * voxel_order_scratch_ints(n)));
  if (o->ds_use) HIP_TRY(o->ds_part.ensure(sizeof(int) * downsample_scratch_ints(n)));
  launch_pack4(o->s, o->raw.as<unsigned char>(), o->raw_stride, n, o->f4.as<float4>(), seg_raw_intensity_offset(o));
  if (o->inten_use && o->ds_use) {
    HIP_TRY(o->rm_flags.ensure((size_t)n));
    HIP_TRY(hipMemsetAsync(o->rm_flags.p, 0, (size_t)n, o->s));
  }
  return GICP_OK;
}

gicp_status seg_static_finish(ddlo_seg* o, const float centre[3], double crop_size, double leaf, const float4** pts,
                              int* count) {
  const int n = (int)o->hn;
  const CropCentre cc{centre[0], centre[1], centre[2]};
  const bool crop = crop_size > 0;
  int m = -1;
  int* const skipped = o->cnt_pin.as<int>() + 16;
  *skipped = 0;
  if (o->ds_use) {
    // the row/column filter's keyframe pass, between the removal and the crop: NaN over the points
    // that leave.  Its |S| <= n' decision is taken on the device; the bit comes back in stream order
    // with the filters' count below, which is waited for anyway.
    const int* ctrl = launch_downsample_keep(o->s, seg_removed_flags(o), o->f4.as<float4>(), n, o->p.rows, o->p.cols, o->ds_row,
                                             o->ds_col, nullptr, o->ds_part.as<int>());
    HIP_TRY(hipMemcpyAsync(skipped, ctrl, sizeof(int), hipMemcpyDeviceToHost, o->s));
  }
  if (leaf > 0) {   // the crop box folded into the voxel pass (as the driver's preprocessing does)
    if (voxel_grid(o->s, o->f4.as<float4>(), n, (float)leaf, o->f4b.as<float4>(), o->vscratch.as<int>(), o->cubtmp.p,
                   o->cubtmp.bytes, &m, crop ? (float)crop_size : 0.f, o->cnt_pin.as<int>(), cc, o->voxel_order,
                   o->voscratch.as<int>(), o->inten_use != 0))
      return fail(GICP_EHIP, "voxel filter scratch too small");
  }
  if (m < 0) {   // no voxel filter, or its grid overflows (the reference then keeps the cloud as it is)
    if (crop_box(o->s, o->f4.as<float4>(), n, (float)crop_size, o->f4b.as<float4>(), o->keep.as<int>(), o->pos.as<int>(),
                 o->cubtmp.p, o->cubtmp.bytes, &m, o->cnt_pin.as<int>(), cc, crop))
      return fail(GICP_EHIP, "crop box scratch too small");
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(o->s));
  o->ds_skipped = *skipped != 0;
  *pts = o->f4b.as<float4>();
  *count = m;
  return GICP_OK;
}

// the removal by segment id.  Host labelling: the removed segments' pixels go
// up (an id named twice is listed twice: harmless); device labelling: only
// their ids, the pixel lists are on the device.  Both through drop_stage.
gicp_status seg_static_cloud_dev(ddlo_seg* o, const int32_t* remove_ids, size_t n_remove, const float centre[3],
                                 double crop_size, double leaf, const float4** pts, int* count) {
  if (!o || !pts || !count || !centre || (!remove_ids && n_remove)) return fail(GICP_EINVAL, "invalid argument");
  if (!o->have) return fail(GICP_EINVAL, "no processed scan");
  const bool dev_label = o->labelling == DDLO_SEG_LABEL_DEVICE;
  const std::vector<int>& off = o->work.seg_off;
  size_t ndrop = 0;
  for (size_t k = 0; k < n_remove; ++k) {
    if (remove_ids[k] < 1 || remove_ids[k] > o->last.segments)
      return fail(GICP_EINVAL, "remove_ids names no segment of the last scan");
    if (!dev_label) ndrop += (size_t)(off[remove_ids[k] + 1] - off[remove_ids[k]]);
  }
  if (gicp_status st = seg_static_begin(o, centre, pts, count)) return st;
  HIP_TRY(o->drop_stage.ensure(sizeof(int) * std::max<size_t>(dev_label ? n_remove : ndrop, 1)));
  int* const drop = o->drop_stage.as<int>();
  if (dev_label && n_remove) {
    std::memcpy(drop, remove_ids, sizeof(int) * n_remove);
    HIP_TRY(rt::grow(o->dids, sizeof(int) * n_remove, o->s));
    HIP_TRY(hipMemcpyAsync(o->dids.p, drop, sizeof(int) * n_remove, hipMemcpyHostToDevice, o->s));
    if (gicp_status st = label_device_drop(o->s, o->ldev, o->dids.as<int>(), (int)n_remove, o->f4.as<float4>(),
                                           seg_removed_flags(o)))
      return st;
  }
  if (ndrop) {
    size_t w = 0;
    for (size_t k = 0; k < n_remove; ++k) {
      const int b = off[remove_ids[k]], e = off[remove_ids[k] + 1];
      std::memcpy(drop + w, o->work.seg_pix.data() + b, sizeof(int) * (size_t)(e - b));
      w += (size_t)(e - b);
    }
    HIP_TRY(o->ddrop.ensure(sizeof(int) * ndrop));
    HIP_TRY(hipMemcpyAsync(o->ddrop.p, drop, sizeof(int) * ndrop, hipMemcpyHostToDevice, o->s));
    if (unsigned char* const flags = seg_removed_flags(o))
      k_static_drop<true><<<cdiv_s((long)ndrop, 256), 256, 0, o->s>>>(o->ddrop.as<int>(), (int)ndrop, o->f4.as<float4>(), flags);
    else
      k_static_drop<false><<<cdiv_s((long)ndrop, 256), 256, 0, o->s>>>(o->ddrop.as<int>(), (int)ndrop, o->f4.as<float4>(),
                                                                       nullptr);
  }
  HIP_TRY(hipGetLastError());
  return seg_static_finish(o, centre, crop_size, leaf, pts, count);
}

}  // namespace ddlo

extern "C" {

gicp_status ddlo_seg_objects(ddlo_seg* o, float max_dim_ratio, ddlo_seg_object* out, size_t cap, size_t* n) {
  if (!o || !n || (!out && cap)) return fail(GICP_EINVAL, "invalid argument");
  std::vector<ddlo_seg_object> v;
  gicp_status st = seg_objects_vec(o, max_dim_ratio, v);
  if (st) return st;
  for (size_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
  *n = v.size();
  return GICP_OK;
}

gicp_status ddlo_seg_objects_from(int device, const float* xyz_t, size_t stride, int rows, int cols, const int32_t* label,
                                  const double* avg_residual, size_t avg_n, float max_dim_ratio, ddlo_seg_object* out,
                                  size_t cap, size_t* n) {
  if (!xyz_t || !label || !n || (!out && cap) || stride < 12 || stride % 4 || rows < 1 || cols < 1 ||
      (long)rows * cols > INT32_MAX / 4)
    return fail(GICP_EINVAL, "invalid argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(GICP_EHIP, "no HIP device " + std::to_string(device) + " (HIP library present, device not visible)");
  HIP_TRY(hipSetDevice(device));
  const size_t np = (size_t)rows * cols;
  // every label's pixels, row-major, as CSR (a counting sort, as ddlo_seg_label_indices)
  int L = 0;
  for (size_t i = 0; i < np; ++i)
    if (label[i] > L && label[i] != kRejected) L = label[i];
  std::vector<int> off;
  label_csr_offsets(label, np, L, off);
  std::vector<int> pix((size_t)off[L + 1]);
  label_csr_pixels(label, np, off, pix.data());
  DevBuf raw, dcsr, dobj;
  const size_t raw_sz = (np - 1) * stride + 12;
  HIP_TRY(raw.ensure(raw_sz));
  hipStream_t s = nullptr;   // the null stream: the copy below is synchronous with it
  HIP_TRY(hipMemcpy(raw.p, xyz_t, raw_sz, hipMemcpyHostToDevice));
  std::vector<ddlo_seg_object> recs((size_t)L), v;
  if (L > 0) {   // pageable staging both ways
    std::vector<int> rows(off.size() + pix.size());
    if (gicp_status st = upload_csr(s, off, pix, L, dcsr, rows.data())) return st;
    if (gicp_status st = run_objects(s, raw.as<unsigned char>(), stride, dcsr.as<int>(), dcsr.as<int>() + off.size(), L, dobj,
                                     recs, nullptr))
      return st;
  }
  filter_objects(recs, avg_residual, avg_residual ? avg_n : 0, max_dim_ratio, v);
  for (size_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
  *n = v.size();
  return GICP_OK;
}

gicp_status ddlo_seg_static_cloud(ddlo_seg* o, const int32_t* remove_ids, size_t n_remove, const float centre[3],
                                  double crop_size, double leaf, float* out, size_t cap, size_t* nout) {
  if (!nout || (!out && cap)) return fail(GICP_EINVAL, "invalid argument");
  const float4* pts = nullptr;
  int m = 0;
  gicp_status st = seg_static_cloud_dev(o, remove_ids, n_remove, centre, crop_size, leaf, &pts, &m);
  if (st) return st;
  *nout = (size_t)m;
  if (!out || m == 0) return GICP_OK;
  if ((size_t)m > cap) return fail(GICP_EINVAL, "output capacity too small");
  return rt::read_xyz(o->s, pts, (size_t)m, out);
}

gicp_status ddlo_seg_static_cloud_xyzi(ddlo_seg* o, const int32_t* remove_ids, size_t n_remove, const float centre[3],
                                       double crop_size, double leaf, float* out_xyzi, size_t cap, size_t* nout) {
  if (!o || !nout || (!out_xyzi && cap)) return fail(GICP_EINVAL, "invalid argument");
  if (!o->inten_use) return fail(GICP_EINVAL, "the segmentation carries no intensity (ddlo_seg_set_intensity)");
  const float4* pts = nullptr;
  int m = 0;
  gicp_status st = seg_static_cloud_dev(o, remove_ids, n_remove, centre, crop_size, leaf, &pts, &m);
  if (st) return st;
  *nout = (size_t)m;
  if (!out_xyzi || m == 0) return GICP_OK;
  if ((size_t)m > cap) return fail(GICP_EINVAL, "output capacity too small");
  HIP_TRY(hipMemcpyAsync(out_xyzi, pts, sizeof(float4) * (size_t)m, hipMemcpyDeviceToHost, o->s));
  HIP_TRY(hipStreamSynchronize(o->s));
  return GICP_OK;
}

gicp_status ddlo_seg_set_intensity(ddlo_seg* o, int use, size_t offset_bytes) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  o->inten_use = use != 0;
  o->inten_off = use ? offset_bytes : 0;
  return GICP_OK;
}

gicp_status ddlo_seg_get_intensity(const ddlo_seg* o, int* use, size_t* offset_bytes) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (use) *use = o->inten_use;
  if (offset_bytes) *offset_bytes = o->inten_off;
  return GICP_OK;
}

}  // extern "C"

extern "C" {

gicp_status ddlo_seg_set_labelling(ddlo_seg* o, int mode) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (mode != DDLO_SEG_LABEL_HOST && mode != DDLO_SEG_LABEL_DEVICE) return fail(GICP_EINVAL, "unknown labelling mode");
  if (mode == DDLO_SEG_LABEL_DEVICE) {
    if (!label_device_window_ok(o->p))
      return fail(GICP_EINVAL, "device labelling needs 0 <= win_col0 and win_col1 <= cols - 1");
    if (!o->rec_pin.p) {
      HIP_TRY(hipSetDevice(o->device));
      HIP_TRY(o->rec_pin.reset(kRecPinBytes));
    }
  }
  if (mode != o->labelling) {   // the last scan's results belong to the other mode's data
    o->have = false;
    o->have_objects = false;
    o->csr_ready = o->csr_len_ready = false;
  }
  o->labelling = mode;
  return GICP_OK;
}

gicp_status ddlo_seg_set_voxel_order(ddlo_seg* o, int order) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (order != DDLO_VOXEL_ORDER_INPUT && order != DDLO_VOXEL_ORDER_PCL) return fail(GICP_EINVAL, "unknown voxel order");
  o->voxel_order = order;
  return GICP_OK;
}

gicp_status ddlo_seg_get_voxel_order(const ddlo_seg* o, int* order) {
  if (!o || !order) return fail(GICP_EINVAL, "null argument");
  *order = o->voxel_order;
  return GICP_OK;
}

gicp_status ddlo_seg_set_downsampling(ddlo_seg* o, int use, int row_step, int col_step) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (row_step < 1 || col_step < 1) return fail(GICP_EINVAL, "downsampling: steps must be >= 1");
  o->ds_use = use != 0;
  o->ds_row = row_step;
  o->ds_col = col_step;
  return GICP_OK;
}

gicp_status ddlo_seg_get_downsampling(const ddlo_seg* o, int* use, int* row_step, int* col_step) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (use) *use = o->ds_use;
  if (row_step) *row_step = o->ds_row;
  if (col_step) *col_step = o->ds_col;
  return GICP_OK;
}

gicp_status ddlo_seg_downsampling_skipped(const ddlo_seg* o, int* skipped) {
  if (!o || !skipped) return fail(GICP_EINVAL, "null argument");
  *skipped = o->ds_skipped ? 1 : 0;
  return GICP_OK;
}

gicp_status ddlo_debug_downsample_keep(int device, const uint8_t* removed, size_t n, int rows, int cols, int row_step,
                                       int col_step, uint8_t* keep_out, int* skipped_out) {
  if (!removed || !keep_out || rows < 1 || cols < 1 || row_step < 1 || col_step < 1 ||
      (long long)rows * cols > INT32_MAX / 4 || n != (size_t)rows * (size_t)cols)
    return fail(GICP_EINVAL, "invalid argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(GICP_EHIP, "no HIP device " + std::to_string(device) + " (HIP library present, device not visible)");
  HIP_TRY(hipSetDevice(device));
  DevBuf flags, keep, scratch;
  HIP_TRY(flags.ensure(n));
  HIP_TRY(keep.ensure(n));
  HIP_TRY(scratch.ensure(sizeof(int) * downsample_scratch_ints((int)n)));
  hipStream_t s = nullptr;   // the null stream: the copies below are synchronous with it
  HIP_TRY(hipMemcpy(flags.p, removed, n, hipMemcpyHostToDevice));
  const int* ctrl = launch_downsample_keep(s, flags.as<unsigned char>(), nullptr, (int)n, rows, cols, row_step, col_step,
                                           keep.as<unsigned char>(), scratch.as<int>());
  HIP_TRY(hipGetLastError());
  int h[2] = {0, 0};
  HIP_TRY(hipMemcpy(h, ctrl, sizeof(h), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(keep_out, keep.p, n, hipMemcpyDeviceToHost));
  if (skipped_out) *skipped_out = h[0];
  return GICP_OK;
}

gicp_status ddlo_seg_get_labelling(const ddlo_seg* o, int* mode) {
  if (!o || !mode) return fail(GICP_EINVAL, "null argument");
  *mode = o->labelling;
  return GICP_OK;
}

gicp_status ddlo_seg_labelling_stats(const ddlo_seg* o, int32_t* replayed, int32_t* longest_prefix) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (!o->have || o->labelling != DDLO_SEG_LABEL_DEVICE) return fail(GICP_EINVAL, "no scan processed in device mode");
  if (replayed) *replayed = o->replayed;
  if (longest_prefix) *longest_prefix = o->longest_prefix;
  return GICP_OK;
}

}  // extern "C"
