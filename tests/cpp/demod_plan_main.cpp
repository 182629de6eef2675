// The plans of the demodulated round's two launches (rgk_amd/csrc/rgk_plan.h rgk_resolve_demod_plan, rgk_demod_divisor_grid) on the
// CPU: this file includes that header and nothing else of the library.  The expected values are written out from what the kernels
// need -- a wave of 64 lanes owns a tile, one lane per pixel; two planes of [PT][2^g + 1] float4 in LDS -- not computed by the unit.
// Exit status 0 = every condition held.
#include <cstdio>

#include "../../rgk_amd/csrc/rgk_plan.h"

static int failures = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
    } while (0)

int main() {
    static_assert(RGK_CUS == 256, "the grids below are those of 256 compute units");
    // known answers: pixels per tile and LDS bytes per gshift (16 B per float4, two planes)
    const uint32_t want_pt[7] = {64, 64, 64, 64, 32, 16, 8};
    const size_t want_lds[7] = {0, 2 * 64 * 3 * 16, 2 * 64 * 5 * 16, 2 * 64 * 9 * 16, 2 * 32 * 17 * 16, 2 * 16 * 33 * 16, 2 * 8 * 65 * 16};
    const uint32_t pixels[] = {1, 7, 8, 63, 64, 65, 576, 703, 1024, 1189, 2073600, 0x7fffffffu};
    for (uint32_t g = 0; g <= 6; g++)
        for (uint32_t npix : pixels) {
            const RgkResolvePlan r = rgk_resolve_demod_plan(npix, g);
            CHECK(r.PT == want_pt[g]);
            CHECK(r.PT >= 1 && r.PT <= 64); // a wave: lane p owns pixel p of the tile
            CHECK(r.lds == want_lds[g]);
            CHECK(r.lds <= 64 * 1024);
            if (g > 0) {
                CHECK(r.lds == 2 * (size_t)r.PT * ((1u << g) + 1u) * 16);
                CHECK(r.lds == 2 * rgk_resolve_plan(npix, g).lds && r.PT == rgk_resolve_plan(npix, g).PT);
            }
            const uint64_t tiles = ((uint64_t)npix + r.PT - 1) / r.PT;
            CHECK(r.grid >= 1 && (uint64_t)r.grid <= tiles);                       // no workgroup without a tile
            CHECK((uint64_t)r.grid == tiles || r.grid == RGK_CUS * 64);          // all of them, or the bounded grid (the kernel strides)
        }
    CHECK(rgk_resolve_demod_plan(576, 0).grid == 9 && rgk_resolve_demod_plan(703, 3).grid == 11 && rgk_resolve_demod_plan(2073600, 3).grid == 16384);
    // the divisor kernel: workgroups of 256 striding over the slots, at most 8 per compute unit
    CHECK(rgk_demod_divisor_grid(0u) == 1);
    CHECK(rgk_demod_divisor_grid(1u) == 1);
    CHECK(rgk_demod_divisor_grid(256u) == 1);
    CHECK(rgk_demod_divisor_grid(257u) == 2);
    CHECK(rgk_demod_divisor_grid(703u * 16u) == 44);
    CHECK(rgk_demod_divisor_grid(2048u * 256u) == 2048);
    CHECK(rgk_demod_divisor_grid(2048u * 256u + 1u) == 2048);
    CHECK(rgk_demod_divisor_grid(0xffffffffu) == 2048); // no 32-bit overflow
    if (failures) std::fprintf(stderr, "%d condition(s) failed\n", failures);
    return failures ? 1 : 0;
}
