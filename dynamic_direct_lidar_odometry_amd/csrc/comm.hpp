// comm.hpp — the RCCL entry points of a sharded ctx (comm.hip).  Used by the
// align engine's all-reduce between linearize and LM step (align.hip) and by
// the residual read-backs and ctx destruction (capi.hip).
#pragma once
#include <rccl/rccl.h>  // types only: RCCL is dlopen'ed on first use

#include <string>

#include "runtime.hpp"

namespace ddlo {
namespace rt {

// RCCL entry points, resolved at run time so the single-GPU library carries
// no link dependency on RCCL.  dlopen by soname: in a process that already
// loaded torch, this returns torch's RCCL, which shares torch's HIP runtime
// with this library (same libamdhip64.so.7 soname), so streams are compatible.
struct Rccl {
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclAllReduce) all_reduce = nullptr;
  decltype(&ncclBroadcast) broadcast = nullptr;   // gicp_set_tie_trees_from_root
  decltype(&ncclSend) send = nullptr;
  decltype(&ncclRecv) recv = nullptr;
  decltype(&ncclGroupStart) group_start = nullptr;
  decltype(&ncclGroupEnd) group_end = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
  bool ok = false;
  std::string why;
};
const Rccl& rccl();

}  // namespace rt
}  // namespace ddlo

#define NCCL_TRY(expr)                                                                      \
  do {                                                                                      \
    ncclResult_t _r = (expr);                                                               \
    if (_r != ncclSuccess)                                                                  \
      return fail(GICP_ECOMM, std::string(#expr) + ": " + rccl().error_string(_r));         \
  } while (0)
