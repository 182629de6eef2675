// The record ring of k_last_vertex (rgk_amd/csrc/rgk_ring.h) and the launch's plan (rgk_plan.h: rgk_last_bounce,
// rgk_last_vertex_grid) on the CPU: this file includes those two headers and nothing else of the library.  `values`: capacity,
// wrap and take, written out.  `workgroup`: the kernel's loop restated with a ring of record NUMBERS -- append the live threads'
// records, take a workgroup's worth when pending, the rest behind the loop -- under a model that poisons a cell when it is read:
// every record is read exactly once, in order, never before it is written and never overwritten while unread; a full take
// happens only inside the loop, the final take is short of a workgroup.  `plan`: which bounce is the last, and the grids.
// Usage: ring_main <case>; exit status 0 = every condition held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rgk_amd/csrc/rgk_plan.h"
#include "../../rgk_amd/csrc/rgk_ring.h"

static int failures = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
    } while (0)

static void values() {
    static_assert(rgk_ring_capacity(256) == 512 && rgk_ring_capacity(64) == 128, "two workgroups' worth");
    CHECK(rgk_ring_wrap(0, 256) == 0 && rgk_ring_wrap(511, 256) == 511 && rgk_ring_wrap(512, 256) == 0 && rgk_ring_wrap(1023 + 5, 256) == 4);
    CHECK(rgk_ring_append_at(500, 10, 1, 256) == 511 && rgk_ring_append_at(500, 10, 2, 256) == 0 && rgk_ring_append_at(256, 255, 255, 256) == 254);
    CHECK(rgk_ring_read_at(300, 0, 256) == 300 && rgk_ring_read_at(300, 255, 256) == 43);
    // inside the loop: nothing below a workgroup's worth, exactly one above; behind it: all that is left
    CHECK(rgk_ring_take(0, 256, false) == 0 && rgk_ring_take(255, 256, false) == 0 && rgk_ring_take(256, 256, false) == 256 && rgk_ring_take(511, 256, false) == 256);
    CHECK(rgk_ring_take(0, 256, true) == 0 && rgk_ring_take(1, 256, true) == 1 && rgk_ring_take(255, 256, true) == 255);
}

// One workgroup of `block` threads over `iters` iterations; live(it, t): thread t's vertex of iteration it is live.
template <class Live>
static void run_workgroup(uint32_t block, uint32_t iters, Live live) {
    const uint32_t cap = rgk_ring_capacity(block);
    const long EMPTY = -1;
    std::vector<long> cell(cap, EMPTY);
    long written = 0, read = 0;
    uint32_t head = 0, pending = 0;
    auto take = [&](bool final) {
        const uint32_t n = rgk_ring_take(pending, block, final);
        CHECK(final ? n < block : (n == 0 || n == block)); // threads 0..n-1 exist
        for (uint32_t t = 0; t < n; t++) {
            const uint32_t p = rgk_ring_read_at(head, t, block);
            CHECK(p < cap && cell[p] == read); // written, unread, and in the order of the appends
            cell[p] = EMPTY; read++;
        }
        head = rgk_ring_wrap(head + n, block); pending -= n;
    };
    for (uint32_t it = 0; it < iters; it++) {
        uint32_t rank = 0;
        for (uint32_t t = 0; t < block; t++) {
            if (!live(it, t)) continue;
            const uint32_t p = rgk_ring_append_at(head, pending, rank++, block);
            CHECK(p < cap && cell[p] == EMPTY); // never over an unread record
            cell[p] = written++;
        }
        pending += rank;
        CHECK(pending < cap);
        take(false);
        CHECK(pending < block);
    }
    take(true);
    CHECK(pending == 0 && read == written);
    for (long c : cell) CHECK(c == EMPTY);
}

static void workgroup() {
    for (uint32_t block : {64u, 256u}) {
        run_workgroup(block, 0, [](uint32_t, uint32_t) { return true; });                 // an empty queue: nothing to flush
        run_workgroup(block, 40, [](uint32_t, uint32_t) { return false; });               // all sky: the ring stays empty
        run_workgroup(block, 40, [](uint32_t, uint32_t) { return true; });                // all live: a take per iteration
        run_workgroup(block, 1, [](uint32_t, uint32_t t) { return t < 8; });              // a queue below a workgroup: the final flush alone
        run_workgroup(block, 41, [&](uint32_t, uint32_t t) { return t + 1 < block; });    // block - 1 per iteration: pending climbs to 2 * block - 2
        run_workgroup(block, 37, [](uint32_t it, uint32_t t) { return ((t * 2654435761u + it * 40503u) >> 7) % 100u < 45u; }); // the headline's 45 %
        run_workgroup(block, 53, [](uint32_t it, uint32_t t) { return (it % 3 == 0) ? true : ((t + it) % 7 == 0); });
    }
}

static void plan() {
    // bounce b holds the vertices with n == b + 1: the last bounce is depth - 1, never bounce 0, never in a bidirectional round
    CHECK(!rgk_last_bounce(0, 1, false) && !rgk_last_bounce(0, 2, false) && rgk_last_bounce(1, 2, false) && !rgk_last_bounce(1, 3, false));
    CHECK(rgk_last_bounce(2, 3, false) && rgk_last_bounce(9, 10, false) && !rgk_last_bounce(8, 10, false) && !rgk_last_bounce(1, 2, true));
    CHECK(!rgk_last_bounce(3, 0, false)); // (depth 0: no bounce runs)
    CHECK(rgk_last_vertex_grid(0xffffffffu) == 1536 && rgk_last_vertex_grid(0u) == 1 && rgk_last_vertex_grid(256u) == 1 && rgk_last_vertex_grid(257u) == 2);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s values|workgroup|plan\n", argv[0]); return 2; }
    if (!std::strcmp(argv[1], "values")) values();
    else if (!std::strcmp(argv[1], "workgroup")) workgroup();
    else if (!std::strcmp(argv[1], "plan")) plan();
    else { std::fprintf(stderr, "unknown case %s\n", argv[1]); return 2; }
    return failures ? 1 : 0;
}
