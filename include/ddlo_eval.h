/*
 * ddlo_eval.h — the evaluation files DetectionModule::evaluate writes per
 * frame (reference dynamic_direct_lidar_odometry/src/detection/detection.cpp:
 * 936-954): the dynamic pixel indices and the pose, which is what the DOALS
 * benchmark scores a dynamic-object method by.  Host code only: like
 * ddlo_track.h it needs no GPU.
 *
 * Per ddlo_eval_write, as evaluate() does:
 *   <dir>/<seq as %04u>.txt   the indices appended, one per line;
 *   <dir>/poses.txt           appended: stamp_ns, a newline, the 4 x 4 pose,
 *                             then ";" and a newline.
 * The pose is printed as Eigen's default operator<< prints a Matrix4f: 6
 * significant digits (an ostream's default float format, printf's %.6g),
 * coefficients of a row separated by one space, every coefficient
 * right-aligned to the width of the widest of the sixteen, rows on separate
 * lines.  The whitespace layout is unpinned: it is restated from Eigen's
 * documentation of IOFormat, with no Eigen build to compare against.  What a
 * parser sees (the stamp, sixteen numbers to 6 significant digits in
 * row-major order, the ";" terminator) is what the tests hold.
 *
 * The indices are the caller's: ddlo_seg_class_indices(DDLO_CLS_DYNAMIC, 0)
 * gives getIndices(DYNAMIC) as an ascending set (ddlo_seg_classes.h; the
 * reference writes the filters' lists one after another, duplicates
 * included).  Not restated: setupEvaluation's time-stamped sub-directory and
 * its copy of the yaml file.
 */
#ifndef DDLO_EVAL_H
#define DDLO_EVAL_H

#include "ddlo_gicp.h"

#ifdef __cplusplus
extern "C" {
#endif

struct ddlo_eval;

/* Creates dir (and its parents) if it is missing.  A directory that cannot
   be created or written to is GICP_EINVAL. */
gicp_status ddlo_eval_open(const char* dir, struct ddlo_eval** out);
/* One frame.  T: the pose, row-major 4 x 4.  n == 0 still creates (or leaves)
   the index file and appends the pose.  A second write with the same seq
   appends to the same index file, as the reference's std::ios::app does. */
gicp_status ddlo_eval_write(struct ddlo_eval* e, uint32_t seq, uint64_t stamp_ns, const float T[16],
                            const int32_t* dynamic_idx, size_t n);
gicp_status ddlo_eval_close(struct ddlo_eval* e);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_EVAL_H */
