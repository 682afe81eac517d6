/*
 * ddlo_seg_project.h — an unorganized cloud into the range image, on the
 * device: every point gets a row from its elevation and a column from its
 * azimuth, the segmentation then runs on the image as on an organized scan,
 * and two maps lead back from pixels to the caller's point indices.
 * Part of ddlo_segment.h, which includes it.
 *
 * The upstream project projected each point this way; the reference fork
 * still carries that loop, commented out (src/detection/detection.cpp:341-357),
 * and takes the pixel from the organized cloud's index instead.  This header
 * restates the commented loop with two deviations:
 *   - The projection uses the SENSOR-frame point.  The commented loop used
 *     the world-axis-aligned, sensor-centred one (cloud_in_t minus the sensor
 *     position), which shears the rows as soon as the sensor pitches or rolls.
 *   - A point whose row falls outside the image is dropped and counted
 *     (out_of_view).  The commented loop clamped it into the last row.
 *
 * The model.  ddlo_seg_default_projection gives the ring model of a sensor
 * whose beams are evenly spaced between +ang_bottom (row 0) and -ang_bottom
 * (the last row) and whose column 0 looks along +x, columns growing with
 * atan2(y, x): elev_top = ang_bottom, elev_res = 2 ang_bottom / float(rows - 1)
 * (the reference's ang_res_y_, detection.cpp:83, computed in float), azim0 = 0,
 * azim_sign = +1.  The commented loop's horizontal angle atan2(x, y) is
 * azim0 = 90, azim_sign = -1.
 *
 * The pixel of a point, entirely in double, from the float coordinates
 * promoted first, these operations in this order (no contraction):
 *   invalid      any coordinate non-finite, or x == y == z == 0 (the drivers'
 *                "no return")
 *   e  = atan2(z, sqrt(x*x + y*y)) * (180 / pi)
 *   qr = (elev_top - e) / elev_res;   row = floor(qr + 0.5)
 *   out of view  unless 0 <= row < rows
 *   a  = atan2(y, x) * (180 / pi)
 *   qc = azim_sign * (a - azim0) / (360.0 / cols);   c = floor(qc + 0.5)
 *   col = ((c mod cols) + cols) mod cols      (columns wrap; none is dropped;
 *                the remainder is taken exactly, whatever the size of c)
 * Among the valid, in-view points of one pixel the HIGHEST input index wins:
 * the sequential overwrite of the reference's loop, and the rule of the
 * residual image (gicp_residual_image).
 *
 * On the device (csrc/seg_project.hip):
 *   k_proj_claim   one thread per point: pixel_of_point[i] (-1: invalid or
 *                  out of view) and an integer atomic max of i on the pixel's
 *                  winner (reset to -1 on the stream before each scan);
 *   k_proj_fill    one thread per pixel: T * p[winner] with the operation
 *                  order of the organized entries' transform, so an organized
 *                  scan handed over as a cloud gives the same bits; a pixel
 *                  without a winner is (NaN, NaN, NaN);
 *   counts         one partial per workgroup (wavefront ballots), added in
 *                  index order by one workgroup: no counter atomics, no
 *                  floating-point atomics.
 */
#ifndef DDLO_SEG_PROJECT_H
#define DDLO_SEG_PROJECT_H

#include "ddlo_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ddlo_seg_projection {
  float elev_top_deg;   /* elevation of row 0 (the top beam) */
  float elev_res_deg;   /* > 0: elevation step from one row down to the next */
  float azim0_deg;      /* azimuth of column 0 */
  int32_t azim_sign;    /* +1: columns grow with atan2(y, x); -1: against it */
} ddlo_seg_projection;

/* points = invalid + out_of_view + occupied_pixels + collisions: a collision
   is a valid, in-view point that lost its pixel to a higher index. */
typedef struct ddlo_seg_projection_result {
  int32_t points;
  int32_t invalid;
  int32_t out_of_view;
  int32_t occupied_pixels;
  int32_t collisions;
} ddlo_seg_projection_result;

/* The ring model of p (above). */
gicp_status ddlo_seg_default_projection(const ddlo_seg_params* p, ddlo_seg_projection* out);

/* ddlo_seg_process for one unorganized cloud: n sensor-frame points (x, y, z
   float first, consecutive points stride_bytes apart; n <= INT32_MAX / 2,
   n == 0 is legal and gives an image of NaN), uploaded, projected, moved to
   the world frame by T (row-major 4x4, the scan's pose) and segmented.
   proj NULL: the defaults of the handle's parameters.  residual and res as in
   ddlo_seg_process; proj_res optional.  Afterwards everything works on the
   handle as after ddlo_seg_process: images, objects, static clouds, tracks,
   classes.  GICP_EINVAL, before anything is launched and with the handle's
   last scan, images and maps left as they were: a non-finite parameter,
   elev_res_deg <= 0, azim_sign not +1 or -1, a stride below 12 or not a
   multiple of 4, n too large. */
gicp_status ddlo_seg_process_cloud(ddlo_seg* s, const float* xyz_sensor, size_t n, size_t stride_bytes,
                                   const float T[16], const ddlo_seg_projection* proj, const float* residual,
                                   ddlo_seg_result* res, ddlo_seg_projection_result* proj_res);

/* The two maps of the last projected scan: winner (rows x cols: the input
   index whose point the pixel holds, -1 for an empty pixel) and
   pixel_of_point (pixel_of_point[i] for i < cap: the row-major pixel point i
   fell into, whether it won the pixel or not; -1 if it was invalid or out of
   view).  Either may be NULL; *n = the scan's point count.  The maps belong
   to a scan: GICP_EINVAL before any projected scan, and once a later
   organized scan (ddlo_seg_process, ddlo_odom_process_dynamic / _tracked) has
   replaced it. */
gicp_status ddlo_seg_projection_maps(ddlo_seg* s, int32_t* winner, int32_t* pixel_of_point, size_t cap, size_t* n);

/* The class byte (ddlo_seg_classes.h) of every input point of the last
   projected scan: out[i] = class_image[pixel_of_point[i]] for i < cap, 0 for
   a point that was invalid or out of view; *n = the point count; out may be
   NULL.  A point that lost its pixel to a higher index gets the byte of the
   pixel it fell into: it lies on the same ray cell as the winner, and "which
   of my points are dynamic" should not depend on the order they arrived in.
   GICP_EINVAL as for ddlo_seg_projection_maps, and until the projected scan
   has been classified (ddlo_seg_classify, ddlo_odom_classify). */
gicp_status ddlo_seg_point_classes(ddlo_seg* s, uint8_t* out, size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_SEG_PROJECT_H */
