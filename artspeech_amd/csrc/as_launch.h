// Host-side launch helpers shared by the translation units of libartspeech_hip.so (header-inline, host only).
#pragma once
#include <atomic>
#include <mutex>
#include <vector>

#include "gemm_internal.h"

// one copy (and one cache) per library, not exported from it
#define AS_LAUNCH_INLINE __attribute__((visibility("hidden"))) inline

// Dynamic LDS beyond 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize.  The attribute belongs to one kernel (its
// address, not its type: the instantiations of a kernel template share a function-pointer type) on the device that is
// current when it is set, so a grant is remembered per (kernel, device); a failure is not remembered (the next call asks
// again).  hipSuccess = the current device has granted `kernel` at least `bytes`.
AS_LAUNCH_INLINE hipError_t as_allow_dynamic_lds(const void* kernel, int bytes) {
    struct Grant { const void* kernel; int dev, bytes; };
    static std::mutex mu;
    static std::vector<Grant> grants;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    Grant* have = nullptr;
    for (Grant& g : grants)
        if (g.kernel == kernel && g.dev == dev) have = &g;
    if (have && have->bytes >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // reported here: a caller that falls back to 64 KB must not find it behind its own launch
        return e;
    }
    if (have) have->bytes = bytes;
    else grants.push_back({kernel, dev, bytes});
    return hipSuccess;
}
template <typename K>
AS_LAUNCH_INLINE hipError_t as_allow_dynamic_lds(K* kernel, int bytes) {
    return as_allow_dynamic_lds(reinterpret_cast<const void*>(kernel), bytes);
}

// compute units of the current device (cached per device); 0 = unknown
AS_LAUNCH_INLINE int as_cu_count() {
    constexpr int MAX_DEV = 64;
    static std::atomic<int> cus[MAX_DEV];
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    const bool slot = dev >= 0 && dev < MAX_DEV;
    if (slot && (n = cus[dev].load(std::memory_order_relaxed)) > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) return 0;
    if (slot) cus[dev].store(n, std::memory_order_relaxed);
    return n;
}

// The stop-event hand-over (gemm_internal.h) for one launch sequence: arms the slot with `ev` (null: nothing armed), take()
// = the event if no launch of the sequence has consumed it, and the slot is empty again on every way out of the scope -- an
// error return included, so that no later launch of this thread binds the event to its own completion.
struct AsStopEventScope {
    explicit AsStopEventScope(hipEvent_t ev) { as_stop_event_set(ev); }
    ~AsStopEventScope() { (void)as_stop_event_take(); }
    AsStopEventScope(const AsStopEventScope&) = delete;
    AsStopEventScope& operator=(const AsStopEventScope&) = delete;
    hipEvent_t take() { return as_stop_event_take(); }
};
