/*
 * ddlo_deskew.h — opt-in motion deskew: every point of a scan carries the time
 * it was captured at, and one in-place pass on the device moves the points
 * into the sensor frame of one reference instant before anything else reads
 * them.  Part of ddlo_odom.h, which includes it; include that.
 *
 * Off by default, and with it off every entry point does what it always did:
 * no added launch, no changed bit.  The reference has no such step (it treats
 * a sweep as an instant); this is an addition, not a restatement.
 *
 * Model.  The sensor's motion over one frame period, expressed in the frame
 * of the reference instant, is a split twist (omega[3], t[3]): a rotation
 * Exp(omega) (omega = axis * angle, rad) and a translation t (m).  At fraction
 * s of a period the sensor's pose relative to the reference instant is
 *     (Exp(s * omega), s * t).
 * Rotation and translation are interpolated INDEPENDENTLY: this is not a
 * screw motion (the se(3) exponential of s * (omega, v)), whose translation
 * would bend with the rotation.  Over one sweep the two differ by second-order
 * terms in |omega| * |t|; the split form is what ddlo_se3_split_log inverts
 * exactly and what an IMU / wheel-odometry pair delivers.
 *
 * A point p captured at time tau becomes, in the reference-instant frame,
 *     s  = (tau_seconds - ref_time) / period                  (double)
 *     p' = Exp(s * omega) * p + s * t.
 * Arithmetic: fp64 throughout, left to right, no fused multiply-add
 * (-ffp-contract=off):
 *     theta = sqrt(wx*wx + wy*wy + wz*wz)        (host)
 *     k     = omega / theta                      (host)
 *     a     = s * theta,  sn = sin(a),  cs = cos(a)
 *     c     = k x p   (cx = ky*pz - kz*py, cy = kz*px - kx*pz, cz = kx*py - ky*px)
 *     d     = k . p   ((kx*px + ky*py) + kz*pz)
 *     p'_i  = float(((p_i*cs + c_i*sn) + k_i*(d*(1.0 - cs))) + s*t_i)
 * with one rounding to float per coordinate.  Special cases:
 *   - theta == 0 is pure translation, p'_i = float(double(p_i) + s*t_i): no sin
 *     or cos is evaluated and the result is exactly reproducible.
 *   - A point with a non-finite coordinate, or with a non-finite time, keeps
 *     its twelve bytes (an organized scan's no-return pixels stay NaN bit for bit).
 *   - An identity twist (omega == 0 and t == 0) launches nothing.
 * Only x, y, z of the DEVICE copy of the scan are rewritten.  The caller's
 * buffer, the intensity and the time field are not.
 *
 * Where it runs.  ddlo_odom_process and its _dynamic, _tracked, _dynamic_cloud
 * and _tracked_cloud twins upload the caller's records once; the pass runs on
 * that upload, over the whole scan, before the registration pack.  So:
 *   - the registration scan (with or without the row/column filter, which
 *     picks its pixels after the pass), the crop box and the voxel filter,
 *   - the organized world-frame scan of the dynamic entries: a pixel stays
 *     where it is, only its point moves,
 *   - the projection of the _cloud entries: in ddlo_seg_project.h's terms, a
 *     point's pixel comes from the elevation and azimuth of the DESKEWED
 *     sensor-frame point, and the winner's T_ * p' goes into the image,
 *   - keyframes, the submap and a map fed from them
 * all see the deskewed scan.  INIT and SKIPPED frames upload nothing and
 * deskew nothing.  The stand-alone ddlo_seg_* entries are unchanged: a caller
 * deskews first with ddlo_deskew.  The map handle's own entries, the RCCL and
 * shard paths and gicp_s2s_batch are out of scope.
 */
#ifndef DDLO_DESKEW_H
#define DDLO_DESKEW_H

#include "ddlo_odom.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The per-point time field's type: float seconds (Velodyne `time`), uint32
 * nanoseconds (Ouster `t`; multiplied by 1e-9 in double) or double seconds
 * (absolute stamps; the subtraction of ref_time is done in double). */
typedef enum { DDLO_TIME_F32_S = 0, DDLO_TIME_U32_NS = 1, DDLO_TIME_F64_S = 2 } ddlo_time_type;

typedef struct ddlo_deskew_params {
  int32_t use;               /* 0 (default): off, the other fields are stored and ignored */
  int32_t time_type;         /* ddlo_time_type */
  size_t time_offset_bytes;  /* the time's place in a point record */
  double ref_time;           /* the instant the scan's pose refers to, same clock as the point times, seconds */
  double period;             /* the frame period the twist spans, seconds, finite and > 0 */
} ddlo_deskew_params;

/* From the next scan on.  period not finite or <= 0, or an unknown time_type,
 * is GICP_EINVAL and changes nothing (whatever `use` says).  The field's place
 * is checked at each process call, where the stride is known:
 *   time_offset_bytes % 4 == 0  (F64: % 8 == 0, and stride_bytes % 8 == 0),
 *   time_offset_bytes >= 12,
 *   time_offset_bytes + size <= stride_bytes  (size 4, F64: 8),
 *   no byte shared with the intensity field when both channels are on;
 * a violation is GICP_EINVAL before the scan or any state is touched (a pending
 * motion included), and the driver stays usable.  ref_time usually changes with
 * every scan: call this before each process call. */
gicp_status ddlo_odom_set_deskew(struct ddlo_odom* o, const ddlo_deskew_params* p);
gicp_status ddlo_odom_get_deskew(const struct ddlo_odom* o, ddlo_deskew_params* p);

/* The caller's twist (IMU, wheel odometry) in the model's units: used for the
 * next scan that reaches the upload (not an INIT or SKIPPED frame, not a
 * refused call), and for that scan only.  With deskew off that scan drops it
 * unused.  omega == NULL or t == NULL clears a pending one.  Non-finite values
 * are GICP_EINVAL and leave a pending one as it is. */
gicp_status ddlo_odom_set_deskew_motion(struct ddlo_odom* o, const double omega[3], const double t[3]);

/* What was applied to the last scan given to a process call (any output may
 * be NULL).  *source: 0 none (identity: deskew off, an INIT or SKIPPED frame,
 * no prediction yet, or a zero twist; no launch), 1 predicted, 2 the caller's.
 *
 * Prediction (constant velocity), used when deskew is on and no caller's
 * twist is pending: D = inv(T_a) * T_b of the last two poses T_ the driver
 * produced, formed in double from the float matrices with the rigid inverse
 * (R^T, -R^T t), then ddlo_se3_split_log's arithmetic.  A pose counts after a
 * FIRST frame (T_ is the identity there) and after every TRACKED frame; INIT
 * and SKIPPED frames neither deskew nor advance this history; until two poses
 * exist the twist is none.  The prediction assumes EVENLY SPACED scans, one
 * period apart: after a dropped scan D spans two periods and the next scan
 * would be over-corrected, so there the caller should pass the motion
 * themselves.  The prediction is undamped and feeds the driver's own pose
 * error into the next scan: measured on a synthetic sequence
 * it did worse than no deskew, while the true twist handed in matched the
 * unskewed chain.  Treat it as a fallback for short gaps in the caller's
 * motion, and measure on your own data before relying on it. */
gicp_status ddlo_odom_deskew_motion(const struct ddlo_odom* o, double omega[3], double t[3], int* source);

/* The split log of a row-major 4x4 transform (host only): t = the translation
 * column; a = 0.5 * (R32 - R23, R13 - R31, R21 - R12), theta = atan2(|a|,
 * (trace - 1) / 2), omega = a * (theta / |a|), or 0 when |a| == 0.  Defined
 * for any 3x3 block, orthonormal or not, for theta < pi. */
gicp_status ddlo_se3_split_log(const float T[16], double omega[3], double t[3]);

/* The pass on its own: uploads the n records (stride_bytes apart: x, y, z
 * float first, the time where p says; p->use is ignored), runs the same
 * in-place kernel with the twist (omega, t), and reads back 12 B per point
 * into out_xyz.  The field rules above apply (no intensity here).  n == 0 is
 * GICP_OK. */
gicp_status ddlo_deskew(int device, const void* records, size_t n, size_t stride_bytes, const ddlo_deskew_params* p,
                        const double omega[3], const double t[3], float* out_xyz);

/* The pass's device time (tools/deskew_bench.py): reps times the upload of the
 * n records from pinned memory followed by the pass on the same stream, as the
 * driver runs them, with device events around the pass alone; ms_out[r] = the
 * r-th pass in milliseconds.  The identity twist is GICP_EINVAL here. */
gicp_status ddlo_debug_deskew_time(int device, const void* records, size_t n, size_t stride_bytes,
                                   const ddlo_deskew_params* p, const double omega[3], const double t[3], int reps,
                                   float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_DESKEW_H */
