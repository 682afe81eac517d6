// track_internal.hpp — the tracker's entries for the odometry driver
// (odom.hip, ddlo_odom_process_tracked).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/ddlo_track.h"

namespace ddlo {

// the live filters' ids and statuses (ddlo_track_status), in filters_ order
void track_live(const ddlo_track* t, std::vector<int32_t>& ids, std::vector<int32_t>& status);
// ids of the filters the last update erased
const std::vector<int>& track_erased(const ddlo_track* t);

}  // namespace ddlo
