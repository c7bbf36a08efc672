// An RCCL all-gather between the devices of one process, resolved at run time and brought up under a watchdog (rccl_gather.hip).
// Host only.  The three calls lock the process-wide communicators themselves.
#pragma once
#include <string>
#include <vector>

#include "ctx.hpp"

namespace zkp {

using RcclComms = std::vector<void*>;      // one communicator per device, rank order

// The communicators of this device set, brought up (library, ncclCommInitAll, probe all-gather) on first use and kept for the life
// of the process; nullptr when RCCL cannot carry the exchange, and *why says so.  timeout_ms: the deadline of each bring-up stage.
const RcclComms* rccl_comms_for(const std::vector<zkp_ctx*>& devs, int timeout_ms, std::string* why);
// One group of all-gathers: device k sends `bytes` bytes from send[k] and receives every device's into recv[k], on its current stream
void rccl_all_gather(const RcclComms& comms, const std::vector<zkp_ctx*>& devs, void* const* send, void* const* recv, size_t bytes);
// whether a bring-up hung or failed its probe: RCCL then stays off for the life of the process
bool rccl_watchdog_fired();

}  // namespace zkp
