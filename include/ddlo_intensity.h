/*
 * ddlo_intensity.h — the opt-in intensity channel: the fourth field of the
 * reference's pcl::PointXYZI, carried from the caller's point record through
 * the odometry driver's filters into the keyframe clouds, and through the
 * global map into its exports and the PCD file.  Part of ddlo_odom.h and
 * ddlo_map.h, which include it; include one of those.
 *
 * Off by default, and with it off every entry point does what it always did.
 * With it on, x, y, z, counts, orders, poses, keyframe decisions and submaps
 * keep their bits: the channel rides in the fourth lane of the float4 point
 * buffers, which the registration never reads.
 *
 * Semantics (PCL 1.10, the version the reference builds against):
 *   - No decision reads intensity.  The finite test, the crop box, voxel
 *     indices, box removal and the row/column selection use x, y, z only; an
 *     intensity of NaN or Inf never drops a point, it propagates.
 *   - Voxel filter (VoxelGrid with downsample_all_data_, CentroidPoint /
 *     AccumulatorIntensity): a voxel's intensity is the float sum of its
 *     points' intensities, from 0.f, in exactly the order the x, y, z sums run
 *     in (input order, or std::sort's under DDLO_VOXEL_ORDER_PCL), divided by
 *     (float)count.  On a voxel-index overflow the input passes through
 *     unchanged, intensity included.
 *   - Crop box, compaction, the world-frame transform of a keyframe, the
 *     map's append and its box removal: a surviving point keeps its intensity
 *     bit for bit.
 *   - Unorganized clouds (the _cloud entries): the point that wins a pixel
 *     brings its own intensity.
 *   - ddlo_odom_process_dynamic / _tracked and their _cloud twins build their
 *     keyframes through the caller's ddlo_seg: the channel is set on both
 *     handles (as the voxel order and the downsampling are), else GICP_EINVAL.
 *
 * Out of scope:
 *   - The clouds of ddlo_seg_classes / ddlo_odom_classify: they return the
 *     caller's point indices, from which a caller gathers any field.
 *   - A PCL-order voxel filter for the map (it has none), and the RCCL and
 *     shard paths.
 */
#ifndef DDLO_INTENSITY_H
#define DDLO_INTENSITY_H

#include "ddlo_odom.h"

#ifdef __cplusplus
extern "C" {
#endif

struct ddlo_map;

/* Whether ddlo_odom_process reads an intensity from every point record, and
 * where: offset_bytes is the float's place in the record (16 for
 * pcl::PointXYZI, 12 for packed x y z i).  use = 0 ignores offset_bytes.  The
 * offset is checked against the stride at each process call, where the stride
 * is known: offset_bytes % 4 == 0, offset_bytes >= 12 and offset_bytes + 4 <=
 * stride_bytes, else GICP_EINVAL and the driver's state is untouched.
 * A driver's keyframes either all have the channel or none do: turning it on
 * or off once a keyframe exists is GICP_EINVAL (the offset may still change). */
gicp_status ddlo_odom_set_intensity(struct ddlo_odom* o, int use, size_t offset_bytes);
gicp_status ddlo_odom_get_intensity(const struct ddlo_odom* o, int* use, size_t* offset_bytes);

/* ddlo_odom_keyframe_points with the channel: 16 B per point (x, y, z,
 * intensity), same order and same x, y, z bits.  GICP_EINVAL if the driver
 * carries no intensity. */
gicp_status ddlo_odom_keyframe_points_xyzi(const struct ddlo_odom* o, int k, float* xyzi, size_t cap, size_t* n);

/* ddlo_preprocess_ordered with the channel: the float offset_bytes into every
 * record (the rules above) goes through the crop box and the voxel filter
 * with its point; out_xyzi takes 16 B per point. */
gicp_status ddlo_preprocess_xyzi(int device, const float* pts, size_t n, size_t stride_bytes, size_t offset_bytes,
                                 double crop_size, double leaf, int order, float* out_xyzi, size_t cap, size_t* n_out);

/* The segmentation handle's side: ddlo_seg_static_cloud's points with their
 * intensity.  The channel is read from the scan the handle holds on the
 * device: at offset_bytes of the records of ddlo_seg_process /
 * ddlo_seg_process_cloud (checked there against the stride, the rules above),
 * or from the fourth lane of the scan the odometry driver staged (which the
 * driver filled from its own offset).  Takes effect with the next scan.
 * No removal decision changes: with the row/column filter on, a removed pixel
 * is marked in a byte of its own instead of the fourth lane, so a removed
 * pixel of any intensity and a kept pixel of intensity 0 are told apart. */
gicp_status ddlo_seg_set_intensity(ddlo_seg* s, int use, size_t offset_bytes);
gicp_status ddlo_seg_get_intensity(const ddlo_seg* s, int* use, size_t* offset_bytes);
/* ddlo_seg_static_cloud with the channel, 16 B per point; GICP_EINVAL if the
 * handle carries no intensity. */
gicp_status ddlo_seg_static_cloud_xyzi(ddlo_seg* s, const int32_t* remove_ids, size_t n_remove, const float centre[3],
                                       double crop_size, double leaf, float* out_xyzi, size_t cap, size_t* nout);

/* Whether the map carries the channel.  Accepted only while the map is empty
 * (GICP_EINVAL otherwise, unless nothing would change). */
gicp_status ddlo_map_set_intensity(struct ddlo_map* m, int use);
gicp_status ddlo_map_get_intensity(const struct ddlo_map* m, int* use);

/* ddlo_map_add_keyframe with the channel read from offset_bytes of every
 * record (the rules above).  GICP_EINVAL on a map without intensity.
 * (ddlo_map_add_keyframe on a map with intensity adds points of intensity 0.)
 * ddlo_map_add_odom_keyframe copies the channel when both handles carry it,
 * and equals ddlo_odom_keyframe_points_xyzi followed by this call bit for
 * bit; a map with intensity fed from a driver without it is GICP_EINVAL. */
gicp_status ddlo_map_add_keyframe_xyzi(struct ddlo_map* m, const float* pts, size_t n, size_t stride_bytes,
                                       size_t offset_bytes, size_t* added);

/* ddlo_map_points with the channel, 16 B per point; GICP_EINVAL on a map
 * without intensity.  ddlo_map_save_pcd of a map with intensity writes
 * FIELDS x y z intensity / SIZE 4 4 4 4 / TYPE F F F F / COUNT 1 1 1 1 and
 * these 16 B per point; of a map without, the file it always wrote. */
gicp_status ddlo_map_points_xyzi(struct ddlo_map* m, double leaf, float* xyzi, size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_INTENSITY_H */
