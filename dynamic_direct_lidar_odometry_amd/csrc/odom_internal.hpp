// odom_internal.hpp — the odometry driver's entry for the global map
// (map.hip, ddlo_map_add_odom_keyframe): a keyframe's cloud is read where it
// lives, on the device.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ddlo_odom.h"

namespace ddlo {

// Keyframe k's device cloud (float4, world frame, after the submap voxel
// filter; valid while the driver lives), its point count, the driver's
// device and the stream its work is queued on.
gicp_status odom_keyframe_dev(const ddlo_odom* o, int k, const float4** pts, int* n, int* device, hipStream_t* stream);
// whether the keyframes' fourth lane holds the intensity (ddlo_odom_set_intensity), not 0
bool odom_has_intensity(const ddlo_odom* o);

}  // namespace ddlo
