// seg_internal.hpp — the segmentation's entries for the odometry driver
// (odom.hip, ddlo_odom_process_dynamic): the scan and the keyframe cloud stay
// on the device between the two.
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
int seg_device(const ddlo_seg* s);
gicp_status seg_get_params(const ddlo_seg* s, ddlo_seg_params* out);

}  // namespace ddlo
