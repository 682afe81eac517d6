/*
 * ddlo_seg_classes.h — the class of every pixel of the last scan, on the
 * device: ground, and the status of the tracks whose pixel lists name it.
 * Part of ddlo_segment.h, which includes it.
 *
 * Restates what OdomNode::applySegmentation builds per frame from the
 * tracker's index lists and the ground image (reference src/odometry/odom.cc:
 * 859-899: the ground, non-static, dynamic and static clouds) and the dynamic
 * pixel indices DetectionModule::evaluate writes (src/detection/detection.cpp:
 * 936-954; the files themselves: ddlo_eval.h).  The lists (ddlo_seg_tracks.h),
 * the ground image and the world-frame scan are in the segmentation handle
 * already, so one pass over them gives every pixel's class:
 *   k_cls_base    one thread per pixel: VALID from the scan as
 *                 ddlo_seg_process saw it (not the packed copy that
 *                 ddlo_seg_static_cloud* writes NaN over: a classification
 *                 after such a call equals one before it), GROUND from the
 *                 device ground image;
 *   k_cls_paint   grid (chunks, tracks) over each track's pool range: the
 *                 track's status bit ORed into the pixel's byte by an integer
 *                 atomic OR on the 32-bit word four pixels share.  OR
 *                 commutes: the image does not depend on the launch order and
 *                 is the same bits from run to run;
 *   counts        per-workgroup partial counts, added in a fixed order.
 * The clouds and the index sets are one three-step partition (count per
 * workgroup by wavefront ballots, an exclusive scan of the counts by one
 * workgroup, a write at offset + ballot prefix): no atomics, ascending pixel
 * order, independent of the grid.
 *
 * Conventions.
 *   - An index set (ddlo_seg_class_indices) is the ascending union without
 *     duplicates.  The reference concatenates the filters' lists in filter
 *     order, duplicates included (tracking.cpp:192-208); as a set it is the
 *     same, and the DOALS evaluation reads a set.
 *   - An index set may contain pixels whose current point is not VALID: a
 *     coasting track keeps the pixels of the scan it last matched, and the
 *     reference writes those indices too.  For the same reason a pixel may
 *     carry several track bits (a stale UNDEFINED list over a current
 *     DYNAMIC one).
 *   - The clouds contain only VALID points.
 *   - The static cloud is the scan without the non-static pixels and without
 *     no-return pixels, taken before any crop or voxel filter
 *     (odom.cc:887-899); ddlo_seg_static_cloud_tracks is the filtered one.
 */
#ifndef DDLO_SEG_CLASSES_H
#define DDLO_SEG_CLASSES_H

#include "ddlo_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DDLO_CLS_VALID 1       /* the world-frame point of the last ddlo_seg_process is finite */
#define DDLO_CLS_GROUND 2      /* in ddlo_seg_ground_indices' set: ground_mat_ == 1 within the bottom ground_rows rows */
#define DDLO_CLS_UNDEFINED 4   /* in the list of at least one track given as DDLO_TRACK_UNDEFINED (0) */
#define DDLO_CLS_STATIC 8      /* ... as DDLO_TRACK_STATIC (1) */
#define DDLO_CLS_DYNAMIC 16    /* ... as DDLO_TRACK_DYNAMIC (2) */
#define DDLO_CLS_NON_STATIC (DDLO_CLS_UNDEFINED | DDLO_CLS_DYNAMIC)

/* pixels per bit; non_static: UNDEFINED or DYNAMIC; static_points: VALID and not non-static */
typedef struct ddlo_seg_class_counts {
  int32_t valid, ground, undefined, static_tracks, dynamic;
  int32_t non_static, static_points;
  int32_t reserved;
} ddlo_seg_class_counts;

/* Classifies the last processed scan: VALID and GROUND from the scan, and
   for i < n the bit of statuses[i] (0..2, ddlo_track_status) on every pixel
   of track_ids[i]'s list.  n == 0 gives only VALID and GROUND.  A track id
   that holds no list, a status outside 0..2, a track id named twice, or a
   handle without a processed scan is GICP_EINVAL and changes nothing (an
   earlier class image stays in place).  counts is optional. */
gicp_status ddlo_seg_classify(ddlo_seg* s, const int32_t* track_ids, const int32_t* statuses, size_t n,
                              ddlo_seg_class_counts* counts);

/* The getters below need a ddlo_seg_classify of the last processed scan
   (GICP_EINVAL otherwise). */

/* The class image, rows x cols bytes, row-major. */
gicp_status ddlo_seg_class_image(ddlo_seg* s, uint8_t* img);

/* The pixels p with (img[p] & any) != 0 and (img[p] & none) == 0, ascending:
   out[i] for i < cap; *n = their number; out may be NULL. */
gicp_status ddlo_seg_class_indices(ddlo_seg* s, int any, int none, int32_t* out, size_t cap, size_t* n);

/* One cloud of ddlo_seg_frame_clouds: xyz receives n points (x, y, z floats)
   when it is not NULL, and cap < n is then GICP_EINVAL; n is always set. */
typedef struct ddlo_seg_cloud_out {
  float* xyz;
  size_t cap;
  size_t n;
} ddlo_seg_cloud_out;

/* applySegmentation's four clouds of this frame, each the VALID points of its
   pixels in ascending pixel order: ground (GROUND), non_static (UNDEFINED or
   DYNAMIC), dynamic (DYNAMIC), static_points (not non-static).  The sets
   overlap.  The partition runs once per classification; later calls only
   copy. */
typedef struct ddlo_seg_frame_clouds_out {
  ddlo_seg_cloud_out ground, non_static, dynamic, static_points;
} ddlo_seg_frame_clouds_out;

gicp_status ddlo_seg_frame_clouds(ddlo_seg* s, ddlo_seg_frame_clouds_out* out);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_SEG_CLASSES_H */
