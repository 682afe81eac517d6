// launch_util.hpp — host helpers shared by the stage files' launchers
// (index_build, covariance, corr_search, moments, outputs).
#pragma once
#include <algorithm>
#include <cstdlib>

#include "devknobs.hpp"

namespace ddlo {

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline int group_blocks(int n) {  // 4 waves (256 threads) per block, one 64-query group per wave
  const int groups = cdiv(n, 64);
  return std::max(1, std::min(cdiv(groups, 4), 4096));
}
static inline int env_knob(const char* name, int dflt) {   // development knobs (A/B of launch shapes)
  const char* v = dev_getenv(name);
  return v && *v ? std::atoi(v) : dflt;
}

}  // namespace ddlo
