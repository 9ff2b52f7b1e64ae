// The device-wide flow fence and its C-ABI entry mfgp_flow_fence (include/mfgp.h).  Host code only.
#include <stdlib.h>

#include <chrono>
#include <condition_variable>
#include <thread>

#include "mfgp_fence.h"
#include "mfgp_host.h"

namespace mfgp {

// ---------------------------------------------------------------- device-wide flow fence
// k_chol_flow needs every CU: two flows whose workgroups interleave (launched on two streams
// at once) each wait for workgroups the other keeps off the CUs, and stall to the hand-off bound.
// One fence per device for the whole process (every handle, every stream, every host thread):
// each flow launch waits for the previous one and becomes the new last one.  Stream-ordered
// (hipStreamWaitEvent), never a host synchronisation.  Inside a stream capture the wait / record
// are skipped (an event recorded outside a capture cannot be waited on inside it): the caller
// orders the replay of such a graph with mfgp_flow_fence (the Python sessions do).
// mfgp_flow_fence(WAIT) .. (RECORD) brackets such a replay and HOLDS the fence in between: a flow
// launch from another host thread blocks on the host (a condition variable, no device
// synchronisation) until the holder records, so it cannot be enqueued beside the replay's
// unfenced flows.  The holding thread itself passes (its eager calls inside the bracket are
// ordered by their streams as usual).
// Holds nest per thread (Engine.ordered blocks inside one another): only the outermost RECORD
// releases.  A thread that finds the fence held by another waits at most fence_bound() on the
// host (10 s; env MFGP_FENCE_BOUND_MS) and then fails with MFGP_ERR_FENCE (a client that issued
// WAIT and never RECORD cannot block every other thread's flow launches for ever).
static std::chrono::milliseconds fence_bound() {
    const char* e = getenv("MFGP_FENCE_BOUND_MS");
    const long ms = e ? atol(e) : 10000;
    return std::chrono::milliseconds(ms > 0 ? ms : 10000);
}
struct FlowFence {
    std::mutex mu;
    std::condition_variable cv;
    hipEvent_t ev = nullptr;
    bool armed = false;
    bool held = false;
    int depth = 0;   // WAITs of the holder not yet matched by a RECORD
    std::thread::id holder;
};
constexpr int FENCE_MAX_DEVICES = 64;
static FlowFence g_fence[FENCE_MAX_DEVICES];

static bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

// with f.mu locked: wait (bounded) until no other thread holds the fence
static bool fence_enter(FlowFence& f, std::unique_lock<std::mutex>& lk) {
    const std::thread::id me = std::this_thread::get_id();
    return f.cv.wait_for(lk, fence_bound(), [&] { return !f.held || f.holder == me; });
}

static int fence_wait(int dev, hipStream_t s, bool hold = false) {
    if (dev < 0 || dev >= FENCE_MAX_DEVICES || stream_capturing(s)) return MFGP_OK;
    FlowFence& f = g_fence[dev];
    std::unique_lock<std::mutex> lk(f.mu);
    if (!fence_enter(f, lk)) return MFGP_ERR_FENCE;
    if (f.armed) (void)hipStreamWaitEvent(s, f.ev, 0);
    if (hold) {
        if (f.held) {
            ++f.depth;   // nested hold of the same thread
        } else {
            f.held = true;
            f.depth = 1;
            f.holder = std::this_thread::get_id();
        }
    }
    return MFGP_OK;
}

// with f.mu locked: record the fence event on s (created on first use)
static void fence_arm(FlowFence& f, int dev, hipStream_t s) {
    if (!f.ev) {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (cur != dev) (void)hipSetDevice(dev);
        if (hipEventCreateWithFlags(&f.ev, hipEventDisableTiming) != hipSuccess) f.ev = nullptr;
        if (cur >= 0 && cur != dev) (void)hipSetDevice(cur);
    }
    if (f.ev && hipEventRecord(f.ev, s) == hipSuccess) f.armed = true;
}

static int fence_record(int dev, hipStream_t s, bool release = false) {
    if (dev < 0 || dev >= FENCE_MAX_DEVICES || stream_capturing(s)) return MFGP_OK;
    FlowFence& f = g_fence[dev];
    std::unique_lock<std::mutex> lk(f.mu);
    if (!fence_enter(f, lk)) return MFGP_ERR_FENCE;
    fence_arm(f, dev, s);
    if (release && f.held && --f.depth <= 0) {   // the outermost RECORD of the holder
        f.held = false;
        f.depth = 0;
        lk.unlock();
        f.cv.notify_all();
    }
    return MFGP_OK;
}

// FenceTurn (mfgp_fence.h)
FenceTurn::FenceTurn(int device, hipStream_t s) {
    if (device < 0 || device >= FENCE_MAX_DEVICES || stream_capturing(s)) return;
    FlowFence& ff = g_fence[device];
    lk = std::unique_lock<std::mutex>(ff.mu);
    if (!fence_enter(ff, lk)) {
        rc = MFGP_ERR_FENCE;
        lk.unlock();
        return;
    }
    if (ff.armed) (void)hipStreamWaitEvent(s, ff.ev, 0);
    f = &ff;
    dev = device;
}
void FenceTurn::commit(hipStream_t s) {
    if (!f) return;
    fence_arm(*f, dev, s);
    f = nullptr;
    lk.unlock();
}

}  // namespace mfgp

using namespace mfgp;

extern "C" {

int mfgp_flow_fence(mfgp_handle_t h, int op) {
    CHECK_H(h);
    // only the fence's own outcome: it enqueues an event wait / record, no kernel (hipGetLastError
    // would report whatever an earlier call left behind)
    if (op == MFGP_FENCE_WAIT) return fence_wait(h->device, h->stream, true);
    if (op == MFGP_FENCE_RECORD) return fence_record(h->device, h->stream, true);
    return MFGP_ERR_ARG;
}

}  // extern "C"
