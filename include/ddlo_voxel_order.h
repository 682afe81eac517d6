/*
 * ddlo_voxel_order.h — the summation order of the device voxel filters and
 * its setting on a ddlo_seg.  Part of ddlo_segment.h, which includes it;
 * include that header (the driver's side is in ddlo_odom.h).
 */
#ifndef DDLO_VOXEL_ORDER_H
#define DDLO_VOXEL_ORDER_H

#include "ddlo_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The order in which a device voxel filter sums the points of one voxel
   (float32 sums: the order decides the centroid's last bit).
   INPUT: input order, the default.  PCL: the order pcl::VoxelGrid sums in,
   which is what libstdc++'s std::sort (introsort, unstable, comparing the
   voxel index alone) leaves on the (voxel index, point index) pairs; the
   centroids then equal PCL's bit for bit. */
typedef enum ddlo_voxel_order {
  DDLO_VOXEL_ORDER_INPUT = 0,
  DDLO_VOXEL_ORDER_PCL = 1
} ddlo_voxel_order;

/* The order of the voxel pass of ddlo_seg_static_cloud and
   ddlo_seg_static_cloud_tracks, from the next call on.  An unknown value is
   GICP_EINVAL and changes nothing.  ddlo_odom_process_dynamic / _tracked (and
   their _cloud twins) build their keyframes through the caller's
   segmentation handle: a caller who wants the PCL order there sets it on both
   handles (ddlo_odom_set_voxel_order, ddlo_odom.h). */
gicp_status ddlo_seg_set_voxel_order(ddlo_seg* s, int order);
gicp_status ddlo_seg_get_voxel_order(const ddlo_seg* s, int* order);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_VOXEL_ORDER_H */
