// The device-wide flow fence (mfgp_fence.hip): what a flow launch sequence needs of it.  Host-only.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/mfgp.h"

namespace mfgp {

struct FlowFence;

// An eager flow launch's turn at the fence.  Taken before the first launch of the
// sequence: the bounded host wait happens here, so a fence held past its bound by another thread
// fails the call with NOTHING enqueued.  The fence's mutex is then kept until commit(), which
// follows the flow launch and records the event unconditionally: no other thread's flow, WAIT or
// hold can be ordered between this launch's wait and its record, and a launch that was enqueued
// always becomes the fence's last flow.
struct FenceTurn {
    FlowFence* f = nullptr;
    std::unique_lock<std::mutex> lk;
    int dev = -1;
    int rc = MFGP_OK;
    FenceTurn(int device, hipStream_t s);
    void commit(hipStream_t s);
};

}  // namespace mfgp
