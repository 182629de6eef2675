// RGK_POISON=1: every fresh device allocation of the library -- the scene's DevBuf members (rgk_scene_impl.h) and the device
// builder's scratch, hipcub's temporary storage included (rgk_build.hip) -- is filled with 0xFF bytes (NaN as float, huge as
// index), so that any read of memory the pipeline did not write first shows in the results instead of hiding behind zero-filled
// fresh pages.  The environment is read once per process; without the switch nothing happens and the total stays 0.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#pragma GCC visibility push(hidden)
// bytes filled so far in this process (rgk_debug_poisoned_bytes): the proof that a poisoned run poisoned something
inline std::atomic<uint64_t>& rgk_poison_total() {
    static std::atomic<uint64_t> total{0};
    return total;
}
inline bool rgk_poison_on() {
    static const bool on = std::getenv("RGK_POISON") != nullptr;
    return on;
}
// `p`: what hipMalloc has just returned.  The fill runs on the null stream and the library's streams are non-blocking: wait for
// it, or it lands on top of real data.
inline void rgk_poison_fill(void* p, size_t bytes) {
    if (!rgk_poison_on() || !p || !bytes) return;
    (void)hipMemset(p, 0xFF, bytes);
    (void)hipDeviceSynchronize();
    rgk_poison_total().fetch_add(bytes, std::memory_order_relaxed);
}
#pragma GCC visibility pop
