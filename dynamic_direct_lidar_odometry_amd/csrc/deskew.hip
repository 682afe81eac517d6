// deskew.hip — the opt-in motion deskew of include/ddlo_deskew.h:
//
//   k_deskew             the in-place pass over an uploaded scan: every point
//                        from the sensor frame at its capture time into the
//                        sensor frame of the reference instant
//   ddlo_se3_split_log   (Exp(omega), t) -> (omega, t) on the host
//   ddlo_deskew          the pass on its own (upload, pass, read-back)
//
// The driver's side (ddlo_odom_set_deskew, the pending and the predicted
// twist, the launch after the upload) lives with the handle in odom.hip.
//
// Compiled with -ffp-contract=off: the header states the fp64 operation order
// and tests/deskew_ref.py restates it; the pure-translation case is bit exact.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ddlo_odom.h"
#include "gicp_types.hpp"
#include "launch.hpp"
#include "runtime.hpp"

namespace ddlo {

namespace {

inline int cdiv_l(long a, long b) { return (int)((a + b - 1) / b); }

// One lane per point; the record's fields are read and written as dwords at
// the caller's stride.  TT: the time field's type (ddlo_time_type); ROT: theta
// != 0 (else pure translation: no sin, no cos).  The per-scan constants arrive
// by value.
template <int TT, bool ROT>
__global__ __launch_bounds__(256) void k_deskew(unsigned char* __restrict__ raw, size_t stride, int n, size_t toff,
                                                DeskewTwist w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned char* rec = raw + (size_t)i * stride;
  float* p = reinterpret_cast<float*>(rec);
  const float fx = p[0], fy = p[1], fz = p[2];
  double tau;
  if (TT == DDLO_TIME_F32_S) {
    tau = (double)*reinterpret_cast<const float*>(rec + toff);
  } else if (TT == DDLO_TIME_U32_NS) {
    tau = (double)*reinterpret_cast<const unsigned*>(rec + toff) * 1e-9;
  } else {   // two dwords: the record is 8-aligned only by the caller's word (checked on the host all the same)
    const unsigned lo = *reinterpret_cast<const unsigned*>(rec + toff), hi = *reinterpret_cast<const unsigned*>(rec + toff + 4);
    tau = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
  }
  if (!(isfinite(fx) && isfinite(fy) && isfinite(fz)) || !isfinite(tau)) return;   // keeps its twelve bytes
  const double s = (tau - w.ref_time) / w.period;
  const double px = fx, py = fy, pz = fz;
  const double stx = s * w.t[0], sty = s * w.t[1], stz = s * w.t[2];
  if (!ROT) {
    p[0] = (float)(px + stx);
    p[1] = (float)(py + sty);
    p[2] = (float)(pz + stz);
    return;
  }
  const double kx = w.k[0], ky = w.k[1], kz = w.k[2];
  const double a = s * w.theta;
  const double sn = sin(a), cs = cos(a);
  const double cx = ky * pz - kz * py, cy = kz * px - kx * pz, cz = kx * py - ky * px;
  const double d = (kx * px + ky * py) + kz * pz;
  const double e = d * (1.0 - cs);
  p[0] = (float)(((px * cs + cx * sn) + kx * e) + stx);
  p[1] = (float)(((py * cs + cy * sn) + ky * e) + sty);
  p[2] = (float)(((pz * cs + cz * sn) + kz * e) + stz);
}

template <int TT>
void launch_tt(hipStream_t s, unsigned char* raw, size_t stride, int n, size_t toff, const DeskewTwist& w) {
  if (w.theta != 0.0) k_deskew<TT, true><<<cdiv_l(n, 256), 256, 0, s>>>(raw, stride, n, toff, w);
  else k_deskew<TT, false><<<cdiv_l(n, 256), 256, 0, s>>>(raw, stride, n, toff, w);
}

// a = 0.5 (R32 - R23, R13 - R31, R21 - R12), theta = atan2(|a|, (trace - 1) / 2), omega = a theta / |a|
void split_log(const double* T, double* omega, double* t) {
  t[0] = T[3];
  t[1] = T[7];
  t[2] = T[11];
  const double ax = 0.5 * (T[9] - T[6]), ay = 0.5 * (T[2] - T[8]), az = 0.5 * (T[4] - T[1]);
  const double na = std::sqrt(ax * ax + ay * ay + az * az);
  if (na == 0.0) {
    omega[0] = omega[1] = omega[2] = 0.0;
    return;
  }
  const double theta = std::atan2(na, ((T[0] + T[5] + T[10]) - 1.0) / 2.0);
  const double f = theta / na;
  omega[0] = ax * f;
  omega[1] = ay * f;
  omega[2] = az * f;
}

}  // namespace

bool deskew_twist(const double* omega, const double* t, double ref_time, double period, DeskewTwist* w) {
  const bool zero = omega[0] == 0.0 && omega[1] == 0.0 && omega[2] == 0.0 && t[0] == 0.0 && t[1] == 0.0 && t[2] == 0.0;
  w->theta = std::sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
  for (int a = 0; a < 3; ++a) {
    w->k[a] = w->theta != 0.0 ? omega[a] / w->theta : 0.0;
    w->t[a] = t[a];
  }
  w->ref_time = ref_time;
  w->period = period;
  return !zero;
}

const char* deskew_field_error(int time_type, size_t toff, size_t stride, bool inten, size_t ioff) {
  const bool f64 = time_type == DDLO_TIME_F64_S;
  const size_t size = f64 ? 8 : 4, al = f64 ? 8 : 4;
  if (toff % al) return f64 ? "deskew: a double time's offset must be a multiple of 8" : "deskew: the time's offset must be a multiple of 4";
  if (f64 && stride % 8) return "deskew: a double time needs a stride that is a multiple of 8";
  if (toff < 12) return "deskew: the time's offset must be >= 12";
  if (toff + size > stride) return "deskew: the time field must end inside the record";
  if (inten && ioff < toff + size && toff < ioff + 4) return "deskew: the time field overlaps the intensity";
  return nullptr;
}

void deskew_between(const float* Ta, const float* Tb, double* omega, double* t) {
  double D[16] = {0};
  // inv(T_a) = (R^T, -R^T t_a)
  double ti[3];
  for (int r = 0; r < 3; ++r)
    ti[r] = -(((double)Ta[r] * (double)Ta[3] + (double)Ta[4 + r] * (double)Ta[7]) + (double)Ta[8 + r] * (double)Ta[11]);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 4; ++c)
      D[4 * r + c] = ((double)Ta[r] * (double)Tb[c] + (double)Ta[4 + r] * (double)Tb[4 + c]) + (double)Ta[8 + r] * (double)Tb[8 + c];
    D[4 * r + 3] += ti[r];
  }
  D[15] = 1.0;
  split_log(D, omega, t);
}

void launch_deskew(hipStream_t s, unsigned char* raw, size_t stride, int n, int time_type, size_t toff,
                   const DeskewTwist& w) {
  if (n <= 0) return;
  if (time_type == DDLO_TIME_F32_S) launch_tt<DDLO_TIME_F32_S>(s, raw, stride, n, toff, w);
  else if (time_type == DDLO_TIME_U32_NS) launch_tt<DDLO_TIME_U32_NS>(s, raw, stride, n, toff, w);
  else launch_tt<DDLO_TIME_F64_S>(s, raw, stride, n, toff, w);
}

}  // namespace ddlo

extern "C" {

using namespace ddlo;
using ddlo::rt::fail;

gicp_status ddlo_se3_split_log(const float T[16], double omega[3], double t[3]) {
  if (!T || !omega || !t) return fail(GICP_EINVAL, "null argument");
  double Td[16];
  for (int i = 0; i < 16; ++i) Td[i] = (double)T[i];
  split_log(Td, omega, t);
  return GICP_OK;
}

gicp_status ddlo_deskew(int device, const void* records, size_t n, size_t stride, const ddlo_deskew_params* p,
                        const double omega[3], const double t[3], float* out_xyz) {
  if (!p || !omega || !t || (n && (!records || !out_xyz)) || stride < 12 || stride % 4 || n > (size_t)INT32_MAX / 2)
    return fail(GICP_EINVAL, "invalid argument");
  if (p->time_type < DDLO_TIME_F32_S || p->time_type > DDLO_TIME_F64_S) return fail(GICP_EINVAL, "deskew: unknown time type");
  if (!std::isfinite(p->period) || !(p->period > 0) || !std::isfinite(p->ref_time))
    return fail(GICP_EINVAL, "deskew: the period must be finite and > 0, the reference time finite");
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(omega[a]) || !std::isfinite(t[a])) return fail(GICP_EINVAL, "deskew: non-finite twist");
  if (const char* e = deskew_field_error(p->time_type, p->time_offset_bytes, stride, false, 0)) return fail(GICP_EINVAL, e);
  if (n == 0) return GICP_OK;
  HIP_TRY(hipSetDevice(device));
  const size_t tsize = p->time_type == DDLO_TIME_F64_S ? 8 : 4;
  const size_t raw = (n - 1) * stride + std::max<size_t>(12, p->time_offset_bytes + tsize);
  rt::DevBuf up;
  HIP_TRY(up.ensure(raw));
  hipStream_t s = nullptr;   // the null stream: a one-off entry
  HIP_TRY(hipMemcpyAsync(up.p, records, raw, hipMemcpyHostToDevice, s));
  DeskewTwist w;
  if (deskew_twist(omega, t, p->ref_time, p->period, &w))
    launch_deskew(s, up.as<unsigned char>(), stride, (int)n, p->time_type, p->time_offset_bytes, w);
  HIP_TRY(hipGetLastError());
  std::vector<unsigned char> h(raw);
  HIP_TRY(hipMemcpyAsync(h.data(), up.p, raw, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (size_t i = 0; i < n; ++i) std::memcpy(out_xyz + 3 * i, h.data() + i * stride, 12);
  return GICP_OK;
}

gicp_status ddlo_debug_deskew_time(int device, const void* records, size_t n, size_t stride, const ddlo_deskew_params* p,
                                   const double omega[3], const double t[3], int reps, float* ms_out) {
  if (!p || !omega || !t || !records || !ms_out || n == 0 || reps < 1 || stride < 12 || stride % 4 ||
      n > (size_t)INT32_MAX / 2 || p->time_type < DDLO_TIME_F32_S || p->time_type > DDLO_TIME_F64_S || !(p->period > 0))
    return fail(GICP_EINVAL, "invalid argument");
  if (const char* e = deskew_field_error(p->time_type, p->time_offset_bytes, stride, false, 0)) return fail(GICP_EINVAL, e);
  DeskewTwist w;
  if (!deskew_twist(omega, t, p->ref_time, p->period, &w)) return fail(GICP_EINVAL, "the identity twist launches nothing");
  HIP_TRY(hipSetDevice(device));
  const size_t raw = (n - 1) * stride + std::max<size_t>(12, p->time_offset_bytes + (p->time_type == DDLO_TIME_F64_S ? 8 : 4));
  rt::DevBuf up;
  rt::PinBuf pin;
  HIP_TRY(up.ensure(raw));
  HIP_TRY(pin.reset(raw));
  std::memcpy(pin.p, records, raw);
  hipStream_t s = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  gicp_status st = GICP_OK;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) st = fail(GICP_EHIP, "event creation failed");
  // each repetition as the driver runs it: the upload, then the pass on the same stream; the events bracket the pass
  for (int r = 0; r < reps && st == GICP_OK; ++r) {
    hipError_t e = hipMemcpyAsync(up.p, pin.p, raw, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(e0, s);
    if (e == hipSuccess) {
      launch_deskew(s, up.as<unsigned char>(), stride, (int)n, p->time_type, p->time_offset_bytes, w);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms_out[r], e0, e1);
    if (e != hipSuccess) st = fail(GICP_EHIP, hipGetErrorString(e));
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  return st;
}

}  // extern "C"
