/*
 * ddlo_odom.h — C-ABI of the odometry driver around the GICP core
 * (with the device voxel filter of rank 3).
 *
 * One ddlo_odom == the registration half of OdomNode (reference
 * dynamic_direct_lidar_odometry/src/odometry/odom.cc): per scan the
 * preprocessing (crop box + voxel filter, odom.cc:442-478), the spaciousness
 * metric and adaptive keyframe threshold (:981-1001, :1156-1178), S2S then
 * S2M registration with pose propagation (:745-851, :921-939), keyframe
 * selection (:1067-1154) and submap assembly from the k nearest / convex-hull
 * / concave-hull keyframes (:1180-1315).  Everything that touches points —
 * scans, keyframe clouds, their covariances and the submap — stays in device
 * memory; the host keeps only poses and index lists.
 *
 * ddlo_odom_process_dynamic adds the step that makes the reference *Dynamic*
 * DLO (odom.cc:685-693, :853-918): every tracked scan is segmented
 * (ddlo_segment.h), its segments become objects, and the objects the caller's
 * tracker does not know to be static are cut out of the scan before it may
 * become a keyframe, so that moving things never enter the submap.
 *
 * The organized-scan row/column filter of both shipped configurations
 * (preprocessing/downsampling, odom.cc:445-455 and :902-906) is opt-in:
 * ddlo_odom_set_downsampling here, ddlo_seg_set_downsampling on the
 * segmentation handle (ddlo_downsample.h states its two passes).
 *
 * Not restated (outside the GICP path): ROS I/O, IMU gravity
 * alignment, publishing and trajectory files.  The object tracker (trackDetections and
 * the bounding-box Kalman filter) is ddlo_track.h: ddlo_odom_process_tracked
 * runs it; ddlo_odom_process_dynamic takes a verdict through ddlo_nonstatic_fn.
 */
#ifndef DDLO_ODOM_H
#define DDLO_ODOM_H

#include "ddlo_gicp.h"
#include "ddlo_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

/* OdomNode parameters (odom.cc:196-252; defaults = cfg/ddlo.yaml:158-204). */
typedef struct ddlo_odom_params {
  gicp_params s2s;                 /* odomNode/gicp/s2s/... (k 10, maxCorr 1.0, maxIter 32, transEps 0.01) */
  gicp_params s2m;                 /* odomNode/gicp/s2m/... (k 20, maxCorr 2.0, maxIter 32, transEps 0.01) */
  int32_t min_num_points;          /* odomNode/gicp/minNumPoints (10): smaller scans are skipped (:635-639) */
  double keyframe_thresh_dist;     /* odomNode/keyframe/threshD (1.0 m); replaced every scan when adaptive */
  double keyframe_thresh_rot;      /* odomNode/keyframe/threshR (0.1 deg) */
  int32_t submap_knn;              /* odomNode/submap/keyframe/knn (10) */
  int32_t submap_kcv;              /* .../kcv (10) */
  int32_t submap_kcc;              /* .../kcc (10) */
  int32_t adaptive;                /* 1 = setAdaptiveParams every scan (the reference always does) */
  int32_t crop_use;                /* preprocessing/cropBoxFilter/use (1) */
  double crop_size;                /* .../size (1.0 m): points inside [-s, s]^3 are removed */
  int32_t vf_scan_use;             /* preprocessing/voxelFilter/scan/use (1) */
  double vf_scan_res;              /* .../res (0.1 m) */
  int32_t vf_submap_use;           /* preprocessing/voxelFilter/submap/use (1): applied to keyframes */
  double vf_submap_res;            /* .../res (0.1 m) */
  int32_t skip_first_scan;         /* 1 (reference): the first scan with >= min_num_points points only
                                      initialises (initializeDDLO, odom.cc:641-646), so keyframe 0 is
                                      the second one; 0: the first scan becomes the target at once */
  int32_t s2m_target_grid;         /* candidate cells of the S2M submap (gicp_set_target_grid): 0 off
                                      (default: a submap lives ~20 scans, fewer than the build pays for),
                                      1 auto, 2 on */
} ddlo_odom_params;

typedef enum ddlo_odom_status {
  DDLO_ODOM_TRACKED = 0,   /* S2S + S2M ran, the pose was updated               */
  DDLO_ODOM_FIRST = 1,     /* first scan: became the S2S target and keyframe 0 */
  DDLO_ODOM_SKIPPED = 2,   /* fewer than min_num_points points (reference: return) */
  DDLO_ODOM_INIT = 3       /* consumed by the initialisation (initializeDDLO, odom.cc:641-646) */
} ddlo_odom_status;

typedef struct ddlo_odom_result {
  int32_t status;                  /* ddlo_odom_status */
  int32_t scan_points;             /* points after preprocessing */
  float T[16];                     /* T_: global pose after S2M (row-major) */
  float T_s2s[16];                 /* T_s2s_: global S2S estimate (the S2M guess) */
  float T_s2s_local[16];           /* T_S2S: scan-to-scan transform */
  gicp_result s2s;
  gicp_result s2m;
  int32_t keyframe_added;          /* updateKeyframes appended a keyframe */
  int32_t submap_changed;          /* submap_hasChanged_ */
  int32_t num_keyframes;
  int32_t submap_keyframes;        /* keyframes in the current submap */
  int64_t submap_points;
  double spaciousness;             /* metrics_.spaciousness.back() */
  double keyframe_thresh_dist;     /* the threshold in effect for this scan */
} ddlo_odom_result;

gicp_status ddlo_odom_default_params(ddlo_odom_params* out);
gicp_status ddlo_odom_create(int device, const ddlo_odom_params* p, struct ddlo_odom** out);
gicp_status ddlo_odom_destroy(struct ddlo_odom* o);
/* OdomNode::icpCB for one scan (odom.cc:614-729, registration part).  xyz:
 * float x, y, z of point 0, consecutive points stride_bytes apart; copied.
 * A keyframe whose submap-voxel-filtered cloud has fewer points than the S2S
 * k gets covariances from all of its points (the reference reads
 * uninitialised neighbour slots there, nanoflann.hpp:149-155).  An error
 * return leaves the driver unusable: destroy it. */
gicp_status ddlo_odom_process(struct ddlo_odom* o, const float* xyz, size_t n, size_t stride_bytes,
                              ddlo_odom_result* res);
/* Keyframe k: world pose (x, y, z, qx, qy, qz, qw as the reference's pose_ /
 * rotq_) and its point count (after the submap voxel filter). */
gicp_status ddlo_odom_keyframe(const struct ddlo_odom* o, int k, float pose7[7], size_t* npoints);
/* Points of keyframe k (world frame, after the submap voxel filter): x, y, z
 * float, 12 B each; xyz[i] for i < cap, *n = the keyframe's point count. */
gicp_status ddlo_odom_keyframe_points(const struct ddlo_odom* o, int k, float* xyz, size_t cap, size_t* n);

/* The dynamic-object step of OdomNode::icpCB (odom.cc:685-693). */
typedef struct ddlo_dynamic_params {
  double theta_min, theta_max;     /* the residual image's angular window (odom.cc:804-805: -60 deg, +60 deg), rad */
  float max_dim_ratio;             /* odomNode/detection/maxDimRatio (10.0) */
} ddlo_dynamic_params;
gicp_status ddlo_dynamic_default_params(ddlo_dynamic_params* out);
/* The tracker's verdict: set non_static[i] = 1 for the objects to cut out
 * (ObjectStatus UNDEFINED or DYNAMIC); non_static arrives zeroed.  Return
 * non-zero to abort (ddlo_odom_process_dynamic then returns GICP_ESTATE and
 * the driver is unusable).  A NULL callback treats every detected object as
 * non-static, which is what the reference does with an object during its
 * first frames (bounding_box_filter.cpp:178-186). */
typedef int (*ddlo_nonstatic_fn)(void* user, const ddlo_seg_object* objs, size_t n, uint8_t* non_static);
/* ddlo_odom_process for one organized sensor-frame scan of seg's rows x cols
 * pixels (NaN = no return): the registration half is ddlo_odom_process on
 * that buffer, bit for bit.  On a TRACKED frame, between pose propagation and
 * updateKeyframes: the world-frame scan T_ * xyz (device) -> the S2M
 * context's residual image at seg's size -> ddlo_seg_process -> ddlo_seg_objects
 * -> decide.  If updateKeyframes then adds a keyframe, its cloud is
 * ddlo_seg_static_cloud without the non-static objects (crop centre pose_,
 * crop_size when crop_use, vf_scan_res when vf_scan_use), followed by the
 * submap voxel filter and the S2S-k covariances as for every keyframe.  The
 * first keyframe (initializeInputTarget) is the registration scan, as in
 * ddlo_odom_process.  INIT, FIRST and SKIPPED frames run no segmentation and
 * zero *seg_res.  dp NULL: the defaults; seg_res may be NULL. */
gicp_status ddlo_odom_process_dynamic(struct ddlo_odom* o, struct ddlo_seg* seg, const float* xyz, size_t stride_bytes,
                                      const ddlo_dynamic_params* dp, ddlo_nonstatic_fn decide, void* user,
                                      ddlo_odom_result* res, ddlo_seg_result* seg_res);
/* ddlo_odom_process_dynamic with the tracker on board (ddlo_track.h) instead
 * of a callback: scans in; poses, static keyframes and, with a map, a map
 * without moving things out.  On a TRACKED frame, in this order: the objects;
 * dt = stamp - time_prev_ (trackDetections, detection.cpp:820-832; time_prev_
 * starts at 0 and advances only on TRACKED frames); ddlo_track_update;
 * ddlo_seg_tracks_sync with the tracks this frame's detections updated or
 * created and the erased ones; then updateKeyframes on ddlo_seg_static_cloud_tracks
 * of every track whose status is UNDEFINED or DYNAMIC, which is the union the
 * reference removes (odom.cc:867-892, tracking.cpp:192-208): a track that was
 * not matched this frame still removes the pixels of the scan it last matched.
 * map (may be NULL): the box histories of the tracks that turned dynamic go
 * to ddlo_map_clear_boxes first; if a keyframe was added,
 * ddlo_map_add_odom_keyframe follows; that includes keyframe 0, made on the
 * FIRST frame (MapNode receives the first keyframe as every other).  INIT,
 * FIRST and SKIPPED frames touch neither the tracker nor the lists and zero
 * *seg_res and *track_res (both optional).  stamp: the scan's time in seconds.
 * The tracker advances before the lists and the map do: after an error return
 * the driver is unusable, as after ddlo_odom_process, and the tracker and the
 * segmentation's lists no longer agree: destroy them with it. */
struct ddlo_track;
struct ddlo_map;
struct ddlo_track_result;
gicp_status ddlo_odom_process_tracked(struct ddlo_odom* o, struct ddlo_seg* seg, struct ddlo_track* track,
                                      struct ddlo_map* map, const float* xyz, size_t stride_bytes, double stamp,
                                      const ddlo_dynamic_params* dp, ddlo_odom_result* res, ddlo_seg_result* seg_res,
                                      struct ddlo_track_result* track_res);
/* ddlo_odom_process_dynamic and ddlo_odom_process_tracked for an UNORGANIZED
 * sensor-frame cloud of n points (a Velodyne-style packet stream, a filtered
 * or merged cloud; ddlo_seg_project.h).  The registration half is
 * ddlo_odom_process on the same (xyz, n), bit for bit: every point registers,
 * those the image drops included.  On a TRACKED frame the world-frame
 * organized scan is not T_ * xyz pixel by pixel but the projection of the
 * frame's upload: every point's pixel from its sensor-frame elevation and
 * azimuth, the highest index wins a pixel, T_ * the winner goes into the
 * image (the same bits the organized entries compute for that point), an
 * empty pixel is NaN.  Everything after it is what the organized twins do.
 * proj NULL: ddlo_seg_default_projection of seg's parameters; an invalid
 * projection is GICP_EINVAL before the scan is touched.  proj_res (optional)
 * is zeroed on INIT, FIRST and SKIPPED frames, as *seg_res is.  Afterwards
 * ddlo_seg_projection_maps and, once classified, ddlo_seg_point_classes
 * answer in the caller's point indices. */
gicp_status ddlo_odom_process_dynamic_cloud(struct ddlo_odom* o, struct ddlo_seg* seg, const float* xyz,
                                            size_t stride_bytes, size_t n, const ddlo_dynamic_params* dp,
                                            ddlo_nonstatic_fn decide, void* user, const ddlo_seg_projection* proj,
                                            ddlo_odom_result* res, ddlo_seg_result* seg_res,
                                            ddlo_seg_projection_result* proj_res);
gicp_status ddlo_odom_process_tracked_cloud(struct ddlo_odom* o, struct ddlo_seg* seg, struct ddlo_track* track,
                                            struct ddlo_map* map, const float* xyz, size_t stride_bytes, size_t n,
                                            double stamp, const ddlo_dynamic_params* dp,
                                            const ddlo_seg_projection* proj, ddlo_odom_result* res,
                                            ddlo_seg_result* seg_res, struct ddlo_track_result* track_res,
                                            ddlo_seg_projection_result* proj_res);
/* The classes of the last scan's pixels (ddlo_seg_classes.h) from the
 * tracker's live filters: ddlo_seg_classify with the ids and statuses that
 * ddlo_track_tracks shows.  Meant to follow a ddlo_odom_process_tracked that
 * returned DDLO_ODOM_TRACKED (the lists then belong to these filters);
 * process_tracked itself does not classify: a caller who never asks pays
 * nothing.  counts optional.  The clouds, index sets and the image are read
 * with ddlo_seg_frame_clouds, ddlo_seg_class_indices, ddlo_seg_class_image. */
gicp_status ddlo_odom_classify(struct ddlo_seg* seg, const struct ddlo_track* track, ddlo_seg_class_counts* counts);
/* Keyframe indices of the current submap (sorted, submap_kf_idx_prev_). */
gicp_status ddlo_odom_submap(const struct ddlo_odom* o, int32_t* idx, size_t cap, size_t* n);
/* The S2S (which = 0) or S2M (which = 1) GICP context, for the gicp_* getters
 * (residuals, residual image, correspondences) of the last scan. */
gicp_status ddlo_odom_ctx(struct ddlo_odom* o, int which, struct gicp_ctx** ctx);
/* Device preprocessing on its own (tests, benchmarks): crop box (crop_size
 * > 0) then voxel filter (leaf > 0) of n points; writes the surviving points
 * (x, y, z float, 12 B each) to out and their count to *nout (cap = capacity
 * of out in points). */
gicp_status ddlo_preprocess(int device, const float* xyz, size_t n, size_t stride_bytes, double crop_size, double leaf,
                            float* out, size_t cap, size_t* nout);
/* ddlo_preprocess with the voxel filter's summation order chosen
 * (ddlo_voxel_order, ddlo_segment.h).  DDLO_VOXEL_ORDER_INPUT gives
 * ddlo_preprocess's bits; DDLO_VOXEL_ORDER_PCL gives pcl::VoxelGrid's.  A
 * grid overflow and a cloud without a finite point behave the same in both. */
gicp_status ddlo_preprocess_ordered(int device, const float* xyz, size_t n, size_t stride_bytes, double crop_size,
                                    double leaf, int order, float* out, size_t cap, size_t* nout);
/* The summation order of the driver's own voxel filters: the scan filter and
 * the keyframe (submap) filter of every ddlo_odom_process* entry, from the
 * next scan on.  An unknown value is GICP_EINVAL and changes nothing.  The
 * keyframes of the dynamic and tracked entries also pass through the caller's
 * segmentation handle: see ddlo_seg_set_voxel_order.  The global map's own
 * filter keeps input order. */
gicp_status ddlo_odom_set_voxel_order(struct ddlo_odom* o, int order);
gicp_status ddlo_odom_get_voxel_order(const struct ddlo_odom* o, int* order);
/* The organized-scan row/column filter (ddlo_downsample.h; cfg/ddlo.yaml
 * preprocessing/downsampling {use, row, col} and detection {rows, columns}),
 * from the next scan on.  row_step, col_step, rows and cols must each be >= 1,
 * otherwise GICP_EINVAL and nothing changes; use == 0 (the default) stores them
 * and leaves every entry as it is.  With use != 0:
 *  - ddlo_odom_process: the scan is organized, n == rows * cols; any other n is
 *    GICP_EINVAL before the scan is touched and the driver stays usable.  The
 *    min_num_points test stays on the raw n (odom.cc:635).  The registration
 *    pass runs before the crop box and the voxel filter: only the pixels of S
 *    are packed, in ascending index order, and everything after runs on
 *    ceil(rows / row_step) * ceil(cols / col_step) points.  That gives the
 *    bits of ExtractIndices' NaN fill: the filters only ever see the finite
 *    points in their original order.
 *  - ddlo_odom_process_dynamic / _tracked: seg's rows x cols and seg's own
 *    setting (ddlo_seg_set_downsampling: use, row_step, col_step) must equal
 *    these, otherwise GICP_EINVAL before the scan is touched.  The registration
 *    half is ddlo_odom_process with the same setting, bit for bit; the
 *    segmentation, the objects, the tracker and the classes see the
 *    full-resolution scan; the residual image comes from the decimated
 *    registration scan, as in the reference.  A keyframe added on a TRACKED
 *    frame is the static cloud with the keyframe pass applied; keyframe 0 is
 *    the preprocessed registration scan.
 *  - ddlo_odom_process_dynamic_cloud / _tracked_cloud: GICP_EINVAL.  For an
 *    unorganized cloud the reference warns and leaves preprocessPoints before
 *    the crop box and the voxel filter too (odom.cc:447-451): a configuration
 *    nobody wants, so it is refused here, not restated. */
gicp_status ddlo_odom_set_downsampling(struct ddlo_odom* o, int use, int row_step, int col_step, int rows, int cols);
gicp_status ddlo_odom_get_downsampling(const struct ddlo_odom* o, int* use, int* row_step, int* col_step, int* rows,
                                       int* cols);
/* The registration pass on its own (tests, benchmarks), as
 * ddlo_preprocess_ordered: the n points are the first n pixels of a rows x
 * cols image; the pixels of S below n are packed in ascending order, then the
 * crop box and the voxel filter in `order`.  If |S| > n (S built for other
 * dimensions) the scan passes unfiltered, as ExtractIndices leaves it. */
gicp_status ddlo_preprocess_downsampled(int device, const float* xyz, size_t n, size_t stride_bytes, int rows, int cols,
                                        int row_step, int col_step, double crop_size, double leaf, int order, float* out,
                                        size_t cap, size_t* nout);
/* The sort behind DDLO_VOXEL_ORDER_PCL on its own (tests): perm_out[r] = the
 * original index at rank r after std::sort of the pairs (keys[i], i) compared
 * by key alone, computed on the device.  stats (optional): which paths the
 * input took. */
typedef struct ddlo_sort_order_stats {
  int32_t levels;          /* partition levels run (the depth limit is 2 floor(log2 n)) */
  int32_t global_levels;   /* of those, levels run on segments too long for one workgroup's LDS */
  int32_t lds_segments;    /* segments handed to the LDS finish */
  int32_t heap_segments;   /* segments heap-sorted at the depth limit */
  int32_t heap_longest;    /* the longest of them */
  int32_t threshold;       /* a segment of at most this many pairs is handed over */
} ddlo_sort_order_stats;
gicp_status ddlo_debug_sort_order(int device, const uint32_t* keys, size_t n, int32_t* perm_out,
                                  ddlo_sort_order_stats* stats_out);
/* The median range behind the spaciousness metric on its own (computeSpaciousness,
 * odom.cc:981-1001): element n / 2 of the sorted ranges float(sqrt(x^2 + y^2 +
 * z^2)) of the n points as they are, with no preprocessing; n == 0 gives 0.
 * Exposed for the tests. */
gicp_status ddlo_median_range(int device, const float* xyz, size_t n, size_t stride_bytes, float* median);

/* Hull keyframe selection (OdomNode::computeConvexHull / computeConcaveHull,
 * odom.cc:1003-1065, pcl::ConvexHull / pcl::ConcaveHull with setDimension(3),
 * odom.cc:87-88, over the keyframe positions): indices of the input points on
 * the hull, ascending.  Convex: qhull's 3-D vertex set, empty for fewer than
 * 4 or coplanar points (qhull's flat-simplex error).  Concave: the vertices
 * of the 3-D alpha shape's boundary triangles (Delaunay triangles of
 * circumradius <= alpha not enclosed by two tetrahedra of circumradius <=
 * alpha).  idx receives at most cap indices; *nidx = the hull's size (it may
 * exceed cap).  Exposed for the tests. */
gicp_status ddlo_convex_hull(const float* xyz, int n, int32_t* idx, int cap, int* nidx);
gicp_status ddlo_concave_hull(const float* xyz, int n, double alpha, int32_t* idx, int cap, int* nidx);

#ifdef __cplusplus
}
#endif

/* the opt-in intensity channel: ddlo_odom_set_intensity, ddlo_odom_keyframe_points_xyzi, ddlo_preprocess_xyzi */
#include "ddlo_intensity.h"
/* the opt-in motion deskew: ddlo_odom_set_deskew, ddlo_odom_set_deskew_motion, ddlo_deskew, ddlo_se3_split_log */
#include "ddlo_deskew.h"

#endif /* DDLO_ODOM_H */
