/*
 * ddlo_map.h — C-ABI of the global map: the device counterpart of MapNode
 * (reference dynamic_direct_lidar_odometry/src/odometry/map.cc).
 *
 * One ddlo_map == MapNode's ddlo_map_ cloud and its three callbacks: every
 * keyframe is voxel-filtered and appended (keyframeCB, map.cc:101-117), the
 * points inside the past bounding boxes of an object the tracker has found to
 * be dynamic are removed (dynamicObjectsCB, map.cc:133-156, fed by
 * TrackingModule::publishBBoxes, tracking.cpp:257-282), and the map is
 * written out, voxelised on request (savePcd, map.cc:158-189).  The map is
 * one float4 buffer in device memory on the map's own stream; points visit
 * the host only in ddlo_map_points and ddlo_map_save_pcd.
 *
 * Where this departs from the reference, on purpose:
 *   - non-finite input points are dropped when a keyframe is added, with the
 *     voxel filter on or off (the reference would keep them, with the filter
 *     off or on a voxel-index overflow, until the next CropBox drops them);
 *   - a box with |orientation_z| > 1 or a non-finite field is GICP_EINVAL and
 *     the map stays as it is (in the reference every comparison of such a box
 *     is false and the negative CropBox erases the whole map);
 *   - the yaw rotation is undone with the transpose of the rotation (the
 *     reference inverts the affine matrix with Eigen's general inverse), so a
 *     point within float rounding of a rotated box's face is not pinned;
 *   - intensity is carried only on request (ddlo_map_set_intensity,
 *     ddlo_intensity.h); by default the map holds x, y, z alone.
 *
 * Not restated: ROS publishing (publishTimerCB), the tracker that produces
 * the boxes.
 */
#ifndef DDLO_MAP_H
#define DDLO_MAP_H

#include "ddlo_odom.h"
#include "ddlo_intensity.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MapNode parameters (map.cc:52-62; defaults = cfg/ddlo.yaml:150-156). */
typedef struct ddlo_map_params {
  int32_t voxel_filter_use;        /* mapNode/useVoxelFilter (1) */
  double leaf_size;                /* mapNode/leafSize (0.25 m) */
  int32_t filter_bboxes;           /* mapNode/filterBboxHistory (1): 0 = ddlo_map_clear_boxes does nothing
                                      (the node does not subscribe, map.cc:38-39) */
  double filter_margin;            /* mapNode/filterMargin (0.0 m): added to every face of a box */
} ddlo_map_params;

/* The jsk_recognition_msgs::BoundingBox fields dynamicObjectsCB reads. */
typedef struct ddlo_map_box {
  double position[3];              /* pose.position: the box centre, world frame */
  double orientation_z;            /* pose.orientation.z = sin(yaw / 2); ddlo_seg_object.state[3] */
  double dimensions[3];            /* full extents along the box's own x, y, z */
} ddlo_map_box;

struct ddlo_map;

gicp_status ddlo_map_default_params(ddlo_map_params* out);
/* MapNode's constructor (map.cc:27-50): an empty map on `device` with its own
 * stream.  p NULL: the defaults.  The map starts with room for 16384 points and grows
 * geometrically (its points are copied device to device). */
gicp_status ddlo_map_create(int device, const ddlo_map_params* p, struct ddlo_map** out);
gicp_status ddlo_map_destroy(struct ddlo_map* m);
/* MapNode::keyframeCB (map.cc:101-117) for one world-frame keyframe.  xyz:
 * float x, y, z of point 0, consecutive points stride_bytes apart; copied.
 * voxel_filter_use: pcl::VoxelGrid at leaf_size over the keyframe's finite
 * points, the centroids appended in voxel-index order; if the voxel index
 * would overflow an int the keyframe is appended unfiltered, as PCL does.
 * The map's filter (here and in ddlo_map_points / ddlo_map_save_pcd) sums a
 * voxel's points in input order: the PCL order that ddlo_odom_set_voxel_order
 * selects for the driver's filters has no counterpart here.
 * Filter off: the finite points are appended in input order.  Non-finite
 * points are dropped in both modes (see above).  *added (optional) = points
 * appended.  A map that would exceed INT_MAX points: GICP_EINVAL. */
gicp_status ddlo_map_add_keyframe(struct ddlo_map* m, const float* xyz, size_t n, size_t stride_bytes, size_t* added);
/* The same for keyframe k of an odometry driver on the same device, read
 * from its device cloud (no host copy): the result equals
 * ddlo_map_add_keyframe of ddlo_odom_keyframe_points(k) bit for bit. */
gicp_status ddlo_map_add_odom_keyframe(struct ddlo_map* m, const struct ddlo_odom* odom, int k, size_t* added);
/* MapNode::dynamicObjectsCB (map.cc:133-156): removes every map point inside
 * at least one of the boxes; the survivors keep their order.  The reference
 * runs one negative pcl::CropBox over the whole map per box; a point
 * survives that loop exactly when it is outside every box, so this is one
 * pass.  Per box: min / max = (float)(-+dimensions / 2 -+ filter_margin)
 * (map.cc:143-148), translation = (float)position, yaw = (float)(2 *
 * asin(orientation_z)) about z (:151-152).  A point p is inside when no
 * coordinate of R(yaw)^T (p - translation) is below min or above max, all in
 * float; a point on a face is inside.  yaw == 0 applies no rotation (CropBox
 * skips a zero rotation).  *removed (optional) = points removed.  A box with
 * |orientation_z| > 1 or a non-finite field: GICP_EINVAL, the map unchanged.
 * filter_bboxes == 0: nothing is done, *removed = 0. */
gicp_status ddlo_map_clear_boxes(struct ddlo_map* m, const ddlo_map_box* boxes, size_t nboxes, size_t* removed);
/* The point count publishTimerCB reports as map_info (map.cc:93-98). */
gicp_status ddlo_map_size(const struct ddlo_map* m, size_t* n);
/* The map's points: x, y, z float, 12 B each; xyz[i] for i < cap, *n = the
 * point count.  leaf > 0: savePcd's voxelised copy (map.cc:169-177), the map
 * itself unchanged; on a voxel-index overflow the map as it is, as PCL does.
 * leaf <= 0: the map.  xyz NULL (cap 0) only queries *n.  A cap below *n
 * with xyz set: GICP_EINVAL (*n is still set); cap = ddlo_map_size always
 * suffices. */
gicp_status ddlo_map_points(struct ddlo_map* m, double leaf, float* xyz, size_t cap, size_t* n);
/* savePcd (map.cc:158-189): ddlo_map_points(leaf) written by the host as a
 * binary PCD v0.7 file with FIELDS x y z (float). */
gicp_status ddlo_map_save_pcd(struct ddlo_map* m, const char* path, double leaf);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_MAP_H */
