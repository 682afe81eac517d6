// seg_label.hpp — the device labelling (seg_label.hip) as segment.hip drives
// it: the scratch a ddlo_seg keeps, the inputs of one run, and the edge
// test's constants, computed on the host once for both labellings.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ddlo_segment.h"
#include "runtime.hpp"

namespace ddlo {

// loadParams :82-83,108-111: ang_res_x_ = 360.0 / float(W_) (double, stored
// as float), ang_res_y_ = 2 * ang_bottom_ / float(H_ - 1) (float); double
// sin / cos.  The angle test without atan2 away from the threshold: atan is
// monotonic, so for x > 0 the float atan2f(y, x) (within 1 ulp of
// atan(y / x)) is above theta when y / x > tan(theta (1 + 1e-6)) and not above
// it when y / x < tan(theta (1 - 1e-6)); in between (and for x <= 0) the
// reference's atan2 decides.  Same decisions, one division per edge.
struct EdgeTrig {
  float sin_x, cos_x, sin_y, cos_y;
  double tan_lo, tan_hi;
  int tan_ok;
};

inline EdgeTrig edge_trig(const ddlo_seg_params& p) {
  EdgeTrig t{};
  const float ang_res_x = (float)(360.0 / (double)(float)p.cols);
  const float ang_res_y = 2.f * p.ang_bottom / (float)(p.rows - 1);
  t.sin_x = (float)std::sin(ang_res_x / 180.0 * M_PI);
  t.cos_x = (float)std::cos(ang_res_x / 180.0 * M_PI);
  t.sin_y = (float)std::sin(ang_res_y / 180.0 * M_PI);
  t.cos_y = (float)std::cos(ang_res_y / 180.0 * M_PI);
  const double th = (double)p.theta;
  t.tan_ok = th > 1e-3 && th < 1.5;   // a threshold well inside (0, pi / 2): both bounds finite and ordered
  if (t.tan_ok) {
    t.tan_lo = std::tan(th * (1.0 - 1e-6));
    t.tan_hi = std::tan(th * (1.0 + 1e-6));
  }
  return t;
}

// The record a run leaves on the device (LabelDev::rec): kLabelRecInts ints,
// then the average residuals by label (doubles, [0] = 0).
enum { kRecSegments = 0, kRecGround, kRecRange, kRecRejected, kRecReplayed, kRecLongestPrefix, kRecError, kRecEligible, kLabelRecInts = 8 };
constexpr size_t kLabelRecMinBytes = 512;   // LabelDev::rec is never smaller

struct LabelDevIn {
  const float* range;           // rows x cols
  const unsigned char* z;       // pixel i's cloud_in_t z is the float at z + i * z_stride
  size_t z_stride;
  const float* resid;           // rows x cols, or nullptr
  const signed char* ground;    // rows x cols, or nullptr: no ground / range pixel counts
  int* label;                   // in: -1 / 0, out: the labels
  float sensor_z;
};

// Scratch of the device labelling, grown once per image and window size, and
// what a run leaves behind: rec, and the feasible segments' pixels as CSR
// (row-major within a segment, as ddlo_seg_label_indices): segment l's are
// seg_pix[seg_off[l] .. seg_off[l + 1]), seg_off[0] = seg_off[1] = 0.
struct LabelDev {
  rt::DevBuf parent, comp, mark, keys_in, vals_in, keys, pix, queue, scan_in, scan_out, cubtmp, seg_off, seg_pix, rec, partial;
  int* off() const { return seg_off.as<int>(); }
  int* pixels() const { return seg_pix.as<int>(); }
  int* ints() const { return rec.as<int>(); }
  double* avg() const { return reinterpret_cast<double*>(rec.as<int>() + kLabelRecInts); }
};

// device mode needs 0 <= win_col0 and win_col1 <= cols - 1: a window that
// reaches outside the columns makes directed wrap edges (the reference tests
// the window before it wraps the column) and an order-dependent result
bool label_device_window_ok(const ddlo_seg_params& p);

// Enqueue one labelling on s (no wait).  Afterwards, on the stream: in.label
// holds the labels, w.rec the record, w.seg_off / w.seg_pix the segments.
gicp_status label_device_run(hipStream_t s, const ddlo_seg_params& p, LabelDev& w, const LabelDevIn& in);

// The removed flag of the static cloud's packed scan: the drop kernels (here, segment.hip,
// seg_tracks.hip) write (NaN, NaN, NaN, kRemovedW) over a removed pixel, the pack writes w = 0, so a
// removed pixel and a no-return pixel stay apart for the row/column filter's keyframe pass.  Nothing
// else reads w.
constexpr float kRemovedW = 1.f;

// pts[pixel] = NaN (w = kRemovedW) for the pixels of the segments ids[0 .. nids) (device ints, each in 1 .. segments)
// flags (optional, seg_state.hpp's seg_removed_flags): the mark goes there, 1 per removed pixel, and w is left 0
gicp_status label_device_drop(hipStream_t s, const LabelDev& w, const int* ids, int nids, float4* pts,
                              unsigned char* flags = nullptr);

gicp_status seg_check_params(const ddlo_seg_params* p);

}  // namespace ddlo
