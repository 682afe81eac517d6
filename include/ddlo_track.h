/*
 * ddlo_track.h — C-ABI of the object tracker: the host half of DDLO's dynamic
 * pipeline between the detected objects (ddlo_seg_objects) and the removal of
 * the non-static ones (ddlo_seg_static_cloud_tracks, ddlo_map_clear_boxes).
 *
 * One ddlo_track == TrackingModule (reference
 * dynamic_direct_lidar_odometry/src/tracking/tracking.cpp) with its
 * BoundingBoxFilter (bounding_box_filter.cpp), KalmanFilter (kalman.cpp),
 * HungarianAlgorithm (hungarian.cpp) and the rotated-box IoU
 * (include/util/bbox_iou.h), as OdomNode::trackDetections drives them
 * (detection.cpp:820-832).  The tracker is tens of filters of ten states: it
 * has no device work at all, so this handle needs no GPU and the calls below
 * run on a machine without one (the one exception to "no CPU fallback": there
 * is nothing to fall back from).
 *
 * Conventions where the reference reads undefined memory or mismatched sizes:
 *   - Object::state is a 10-vector of which getObject fills 7
 *     (detection.cpp:774): entries 7..9 of a detection are 0 here;
 *   - kfilter_.update(tracked_object_.state) hands a 10-vector to a 7-row C
 *     (bounding_box_filter.cpp:84): the measurement is the first 7 entries;
 *   - a pair of boxes whose volumes give 0 / 0 has IoU 0 here (the reference's
 *     NaN cost sends its Hungarian solver into an endless recursion:
 *     DESIGN.md §12).
 * Not restated: ROS messages, the marker text.  (The evaluation files:
 * ddlo_eval.h.)
 */
#ifndef DDLO_TRACK_H
#define DDLO_TRACK_H

#include "ddlo_map.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TrackingModule::load_params (tracking.cpp:16-25).  ddlo_track_default_params
 * gives cfg/ddlo.yaml:224-233: 30, 5, 1, 15, 0.75, 0.3 (the project's rule:
 * defaults are the yaml's).  The code defaults of tracking.cpp:19-24, used
 * when a key is missing: maxNoHits 5, minDynamicHits 3, maxUndefinedHits 10,
 * maxObjVelocity 10, minDistFromOrigin 0.5, residuumHeightRatio 0.0. */
typedef struct ddlo_track_params {
  int32_t max_no_hits;             /* odomNode/tracking/maxNoHits: a filter with sslu >= this is erased */
  int32_t min_dynamic_hits;        /* .../minDynamicHits */
  int32_t max_undefined_hits;      /* .../maxUndefinedHits */
  float max_obj_velocity;          /* .../maxObjVelocity (m/s; a float member, tracking.h:36) */
  double min_dist_from_origin;     /* .../minDistFromOrigin (m, x-y travel from the first pose) */
  double residuum_height_ratio;    /* odomNode/detection/residuumHeightRatio */
} ddlo_track_params;

typedef enum ddlo_track_status {   /* ObjectStatus (object.h:9-14) */
  DDLO_TRACK_UNDEFINED = 0,
  DDLO_TRACK_STATIC = 1,
  DDLO_TRACK_DYNAMIC = 2
} ddlo_track_status;

/* One BoundingBoxFilter as its getters show it. */
typedef struct ddlo_track_record {
  int32_t id;                      /* getFilterID */
  int32_t status;                  /* ddlo_track_status */
  int32_t hits;                    /* getHits (starts at 1) */
  int32_t sslu;                    /* getSSLU: predictions since the last update */
  double state[10];                /* getFullState: x, y, z, sin(yaw/2), dx, dy, dz, vx, vy, vz */
  int32_t num_points;              /* getNumPoints: of the detection last matched */
  int32_t object_id;               /* getObjectID: that detection's segment id, in ITS scan */
  double avg_residuum;             /* getAvgResiduum (a float in the reference) */
  double dist_to_origin;           /* getDistToOrigin */
  int32_t history;                 /* static_bboxes_.boxes.size() (0 .. 5) */
  int32_t reserved;
} ddlo_track_record;

typedef struct ddlo_track_result {
  int32_t undefined_tracks, static_tracks, dynamic_tracks;   /* getObjectsCount by status, after the update */
  int32_t matches;                 /* matches_ after the velocity gate */
  int32_t created;                 /* filters created (unmatched_detections_) */
  int32_t erased;                  /* filters erased (sslu >= max_no_hits) */
  int32_t turned_dynamic;          /* filters whose has_turned_dynamic_ was set */
  int32_t boxes_cleared;           /* boxes collected from them (publishBBoxes' clear_map) */
  int64_t indices_dropped;         /* ddlo_odom_process_tracked: sum of the removed lists' lengths; else 0 */
} ddlo_track_result;

#define DDLO_TRACK_MASK_UNDEFINED 1
#define DDLO_TRACK_MASK_STATIC 2
#define DDLO_TRACK_MASK_DYNAMIC 4

struct ddlo_track;

gicp_status ddlo_track_default_params(ddlo_track_params* out);
/* p NULL: the defaults. */
gicp_status ddlo_track_create(const ddlo_track_params* p, struct ddlo_track** out);
gicp_status ddlo_track_destroy(struct ddlo_track* t);
/* TrackingModule::update (tracking.cpp:27-78) for the n detections of one
 * scan, dt seconds after the previous one: predict, associate, update the
 * matched filters, create one per unmatched detection (ids count from 0),
 * erase, collect the cleared boxes.  out_track_id[i] (optional) = the id of
 * the filter detection i updated or created.  res optional. */
gicp_status ddlo_track_update(struct ddlo_track* t, double dt, const ddlo_seg_object* objs, size_t n,
                              int32_t* out_track_id, ddlo_track_result* res);
/* The filters in filters_ order: out[i] for i < cap; *n = their number. */
gicp_status ddlo_track_tracks(const struct ddlo_track* t, ddlo_track_record* out, size_t cap, size_t* n);
/* getObjectsCount over a DDLO_TRACK_MASK_* mask. */
gicp_status ddlo_track_count(const struct ddlo_track* t, int status_mask, size_t* n);
/* Ids of the filters the last update erased. */
gicp_status ddlo_track_erased(const struct ddlo_track* t, int32_t* ids, size_t cap, size_t* n);
/* The box histories collected since the last call (publishBBoxes,
 * tracking.cpp:257-282), as ddlo_map_clear_boxes takes them; emptied when out
 * is given and cap suffices.  out NULL queries *n. */
gicp_status ddlo_track_take_cleared_boxes(struct ddlo_track* t, ddlo_map_box* out, size_t cap, size_t* n);
/* The last associate(): cost (double) and displacement (float) matrices,
 * rows = detections, cols = filters, row-major; assignment[rows] as the
 * Hungarian solver left it (before the gate).  Any pointer may be NULL; a
 * frame without detections or without filters has rows = cols = 0. */
gicp_status ddlo_track_last_costs(const struct ddlo_track* t, double* cost, float* disp, int32_t* assignment, size_t cap,
                                  int32_t* rows, int32_t* cols);
/* HungarianAlgorithm::Solve on its own: cost rows x cols row-major,
 * assignment[rows] (-1: unassigned).  A NaN entry is GICP_EINVAL. */
gicp_status ddlo_track_assign(const double* cost, int rows, int cols, int32_t* assignment);
/* A ready-made ddlo_nonstatic_fn for ddlo_odom_process_dynamic, user = the
 * tracker: updates it with the step set by ddlo_track_set_dt (default 0.1 s)
 * and flags the objects whose filter is UNDEFINED or DYNAMIC.  It can only
 * cut objects of the current scan: the stale lists of coasting filters need
 * ddlo_odom_process_tracked. */
int ddlo_track_decide(void* user, const ddlo_seg_object* objs, size_t n, uint8_t* non_static);
gicp_status ddlo_track_set_dt(struct ddlo_track* t, double dt);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_TRACK_H */
