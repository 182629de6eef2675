// The record ring of k_last_vertex (rgk_shade.h), the part that needs no device: a workgroup of `block` threads appends at most
// `block` records per iteration of its queue loop (phase A: one thread per queue entry, the live vertices leave a record) and
// takes `block` records at a time as soon as that many are pending (phase B: one thread per record, full waves), the remainder
// once, after the loop.  Pure functions over plain integers, like rgk_plan.h: tests/cpp/ring_main.cpp includes this header alone.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RGK_RING_HD __host__ __device__
#else
#define RGK_RING_HD
#endif

// Records the ring holds.  Before an append at most block - 1 records are pending (block or more would have been taken), the
// append adds at most block: 2 * block - 1 at the most.  `block` is a power of two, so a position wraps with a mask.
RGK_RING_HD constexpr uint32_t rgk_ring_capacity(uint32_t block) { return 2u * block; }
RGK_RING_HD constexpr uint32_t rgk_ring_wrap(uint32_t pos, uint32_t block) { return pos & (rgk_ring_capacity(block) - 1u); }
// where the record of rank `rank` among an iteration's live threads goes: behind the `pending` records that start at `head`
RGK_RING_HD constexpr uint32_t rgk_ring_append_at(uint32_t head, uint32_t pending, uint32_t rank, uint32_t block) { return rgk_ring_wrap(head + pending + rank, block); }
// records phase B takes now, from `head` on: a full workgroup's worth inside the loop, whatever is left behind it (`final`)
RGK_RING_HD constexpr uint32_t rgk_ring_take(uint32_t pending, uint32_t block, bool final) { return final ? pending : (pending >= block ? block : 0u); }
// the record thread t of phase B reads
RGK_RING_HD constexpr uint32_t rgk_ring_read_at(uint32_t head, uint32_t t, uint32_t block) { return rgk_ring_wrap(head + t, block); }
