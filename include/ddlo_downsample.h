/*
 * ddlo_downsample.h — the organized-scan row/column filter of
 * OdomNode::preprocessPoints and applySegmentation (odom.cc:125-130, 219-223,
 * 445-455, 902-906) and its setting on a ddlo_seg.  Part of ddlo_segment.h,
 * which includes it; include that header (the driver's side,
 * ddlo_odom_set_downsampling and ddlo_preprocess_downsampled, is in
 * ddlo_odom.h).
 *
 * The reference builds one index set for an image of rows x cols pixels,
 *   S = { r * cols + c : r = 0, row_step, 2 row_step, ... < rows;
 *                        c = 0, col_step, 2 col_step, ... < cols },
 * and runs one pcl::ExtractIndices (keep-organized) with it twice:
 *
 *   registration pass  over the organized scan before the crop box and the
 *                      voxel filter: pixel p stays if p is in S.
 *   keyframe pass      over the compacted cloud left once the non-static
 *                      pixels were extracted: the point at POSITION j of that
 *                      cloud stays if j is in S.  No-return (NaN) pixels keep
 *                      their positions, removed pixels do not, so from the
 *                      first removed pixel on the positions are not the pixels.
 *
 * ExtractIndices (PCL 1.10) on an input of n points: if |S| > n it reports
 * "indices size exceeds the size of the input" and passes the input on
 * unchanged; otherwise every position outside S becomes NaN (indices of S
 * that are >= n have no effect) and the crop box and the voxel filter, which
 * skip non-finite points, drop them.
 */
#ifndef DDLO_DOWNSAMPLE_H
#define DDLO_DOWNSAMPLE_H

#include "ddlo_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The keyframe pass inside ddlo_seg_static_cloud and
   ddlo_seg_static_cloud_tracks, between the removal and the crop box, from
   the next call on (odomNode/preprocessing/downsampling/{use,row,col}; rows
   and columns are the handle's own).  use == 0: off, the default; the steps
   are stored all the same.  A step < 1 is GICP_EINVAL and changes nothing.
   ddlo_odom_process_dynamic / _tracked require the same setting on the
   driver (ddlo_odom_set_downsampling). */
gicp_status ddlo_seg_set_downsampling(ddlo_seg* s, int use, int row_step, int col_step);
gicp_status ddlo_seg_get_downsampling(const ddlo_seg* s, int* use, int* row_step, int* col_step);
/* *skipped = 1 if the keyframe pass of the last static cloud met |S| > n'
   (n' = pixels not removed) and filtered nothing, as the reference then
   does; 0 otherwise, and when the pass is off. */
gicp_status ddlo_seg_downsampling_skipped(const ddlo_seg* s, int* skipped);

/* The keyframe pass's rank-and-mask kernels on their own (tests).  removed:
   n = rows * cols flags, non-zero = the pixel was extracted before the pass.
   Pixel p not removed has position j = p - (removed pixels before p) in the
   compacted cloud of n' points; keep_out[p] = 1 if it is not removed and
   (j / cols) % row_step == 0 && (j % cols) % col_step == 0, or if |S| > n',
   when the pass filters nothing and *skipped_out (optional) = 1. */
gicp_status ddlo_debug_downsample_keep(int device, const uint8_t* removed, size_t n, int rows, int cols, int row_step,
                                       int col_step, uint8_t* keep_out, int* skipped_out);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_DOWNSAMPLE_H */
