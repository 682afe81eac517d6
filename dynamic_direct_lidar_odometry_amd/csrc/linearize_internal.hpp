// linearize_internal.hpp — the correspondence-search launches of
// corr_search.hip that launch_linearize (moments.hip) issues ahead of the
// moment kernel.  Not part of launch.hpp: the host runtime never calls them.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.hpp"

namespace ddlo {

// candidate-cell lookup (k_cell_lookup), one 16-query sub-group per wave
void launch_cell_lookup(hipStream_t s, const AlignJob* job, const LinGeom& g);
// the walk: k_nn_seed, then k_nn_scan over its task list; with candidate cells
// (g.grid) small grids over the few sub-groups the lookup left, scanned inline
void launch_nn_walk(hipStream_t s, const AlignJob* job, const LinGeom& g);

}  // namespace ddlo
