// seg_internal.hpp — the segmentation's entries for the odometry driver
// (odom.hip, ddlo_odom_process_dynamic): the scan and the keyframe cloud stay
// on the device between the two.  The handle itself is seg_state.hpp's.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/ddlo_segment.h"

namespace ddlo {

// The segmentation's input buffer for rows x cols float4 points (world
// frame, NaN = no return), for the caller to fill on its own stream.
gicp_status seg_stage_input(ddlo_seg* s, float4** buf, int* npix);
// ddlo_seg_process over the staged input (the caller's writes are complete).
gicp_status seg_process_staged(ddlo_seg* s, const float T[16], const float* residual, ddlo_seg_result* res);
// ddlo_seg_objects into a vector.
gicp_status seg_objects_vec(ddlo_seg* s, float max_dim_ratio, std::vector<ddlo_seg_object>& out);
// ddlo_seg_static_cloud, the result left on the device: *pts (float4, valid
// until the next call on s) and *count; complete when the call returns.
gicp_status seg_static_cloud_dev(ddlo_seg* s, const int32_t* remove_ids, size_t n_remove, const float centre[3],
                                 double crop_size, double leaf, const float4** pts, int* count);
// ddlo_seg_static_cloud_tracks (seg_tracks.hip), the result left on the device
// as seg_static_cloud_dev leaves it; *dropped (optional) = the sum of the
// removed lists' lengths
gicp_status seg_static_cloud_tracks_dev(ddlo_seg* s, const int32_t* track_ids, size_t n, const float centre[3],
                                        double crop_size, double leaf, const float4** pts, int* count, int64_t* dropped);
// the pool ranges (offset, length) of the lists of the tracks in track_ids,
// one per id in their order, and the pool buffer in use; a track id that holds
// no list is GICP_EINVAL.  No device work.
gicp_status seg_tracks_ranges(ddlo_seg* s, const int32_t* track_ids, size_t n, std::vector<int2>* ranges,
                              const int** pool);

// ddlo_seg_frame_clouds' results as they lie on the device after it (ground,
// non-static, dynamic, static: float4, w = 0), valid until the next
// ddlo_seg_classify on s; complete when the call returns.
gicp_status seg_frame_clouds_dev(ddlo_seg* s, const float4* pts[4], int count[4]);
// the class image of the last scan on the device (rows x cols bytes), or
// GICP_EINVAL as ddlo_seg_class_image; no device work
gicp_status seg_class_image_dev(ddlo_seg* s, const unsigned char** img);

// The projection of an unorganized cloud (seg_project.hip).
// proj (NULL: the defaults of s) checked and resolved into *out; no device work
gicp_status seg_projection_resolve(ddlo_seg* s, const ddlo_seg_projection* proj, ddlo_seg_projection* out);
// Claim and fill: the n points in raw (device memory, stride bytes apart,
// complete on st) into the segmentation's staged input (seg_stage_input),
// moved by T; runs on st and waits for it.  *out: the counts.  proj: resolved.
// ioff: where the float intensity sits in raw's records (the pixel's winner brings its own into the
// staged input's w); 0: w = 0
gicp_status seg_project_dev(ddlo_seg* s, hipStream_t st, const unsigned char* raw, size_t stride, int n, const float T[16],
                            const ddlo_seg_projection& proj, ddlo_seg_projection_result* out, size_t ioff = 0);
// after the seg_process_staged that followed seg_project_dev: the maps are
// those of the handle's scan
gicp_status seg_project_commit(ddlo_seg* s);

int seg_device(const ddlo_seg* s);
gicp_status seg_get_params(const ddlo_seg* s, ddlo_seg_params* out);

}  // namespace ddlo
