// The launch-plan unit (rgk_amd/csrc/rgk_plan.h) on the CPU: this file includes that header and nothing else of the library, and
// links without the HIP runtime.  Every expected value below is written out from the formulas the launch wrappers and the host
// carried before the unit existed and from the pass plans tests/test_gpu_invariance.py names in its comments -- never computed
// by the unit itself.  Usage: plan_main <case>; exit status 0 = every condition held.
#include <cstdio>
#include <cstring>

#include "../../rgk_amd/csrc/rgk_plan.h"

static int failures = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
    } while (0)

static void grids() {
    static_assert(RGK_CUS == 256, "the grids below are those of 256 compute units");
    // persistent walkers: LDS-limited residency x 256 CUs
    CHECK(rgk_trace_grid(8) == 2048);
    CHECK(rgk_trace_grid(16) == 2048);
    CHECK(rgk_trace_grid(32) == 1280);
    CHECK(rgk_bounded_grid(2048, 0u, 256u) == 1);
    CHECK(rgk_bounded_grid(2048, 256u, 256u) == 1);
    CHECK(rgk_bounded_grid(2048, 257u, 256u) == 2);
    CHECK(rgk_bounded_grid(2048, 0xffffffffu, 256u) == 2048); // no 32-bit overflow
    CHECK(rgk_bounded_grid(1280, 1280u * 256u + 1u, 256u) == 1280);
    // the shade pair: bounce 0 in blocks of 512, later bounces in blocks of 256
    const uint32_t full = 0xffffffffu;
    RgkGridPair g = rgk_shade_grids(0, full);
    CHECK(g.block == 512 && g.fast == 1024 && g.generic == 512);
    g = rgk_shade_grids(0, 0u);
    CHECK(g.block == 512 && g.fast == 1 && g.generic == 1);
    g = rgk_shade_grids(0, 1000u); // ceil(1000 / 512) = 2
    CHECK(g.fast == 2 && g.generic == 2);
    g = rgk_shade_grids(0, 512u * 600u + 1u); // 601 blocks asked for: the generic launch is full at 512
    CHECK(g.fast == 601 && g.generic == 512);
    for (uint32_t b = 1; b < 4; b++) {
        g = rgk_shade_grids(b, full);
        CHECK(g.block == 256 && g.fast == 2048 && g.generic == 1024);
        g = rgk_shade_grids(b, 0u);
        CHECK(g.fast == 1 && g.generic == 1);
        g = rgk_shade_grids(b, 37u);
        CHECK(g.fast == 1 && g.generic == 1);
        g = rgk_shade_grids(b, 256u * 1500u + 1u); // 1501 blocks
        CHECK(g.fast == 1501 && g.generic == 1024);
    }
    // the light sub-path's launches and the connections
    g = rgk_light_grids(full);
    CHECK(g.block == 512 && g.fast == 1024 && g.generic == 512);
    g = rgk_light_grids(0u);
    CHECK(g.fast == 1 && g.generic == 1);
    g = rgk_light_grids(64u * 64u * 8u); // Cornell 64 x 64 x 8: 32768 / 512
    CHECK(g.fast == 64 && g.generic == 64);
    CHECK(RGK_CONNECT_BLOCK == 256);
    CHECK(rgk_connect_grid(full) == 2048);
    CHECK(rgk_connect_grid(0u) == 1);
    CHECK(rgk_connect_grid(257u) == 2);
    // the bundle walker's queue: one entry per 8 rays
    CHECK(rgk_beam_bound(0u) == 1u);
    CHECK(rgk_beam_bound(8u) == 2u);
    CHECK(rgk_beam_bound(2097152u) == 262145u);
    CHECK(rgk_beam_bound(full) == 0x20000000u);
}

static void resolve() {
    // gshift 0: a thread per pixel, min(ceil(npix / 256), 4096) blocks
    RgkResolvePlan r = rgk_resolve_plan(1u, 0);
    CHECK(r.grid == 1);
    r = rgk_resolve_plan(62138u, 0); // ceil(62138 / 256) = 243
    CHECK(r.grid == 243);
    r = rgk_resolve_plan(4096u * 256u, 0);
    CHECK(r.grid == 4096);
    r = rgk_resolve_plan(4096u * 256u + 1u, 0);
    CHECK(r.grid == 4096);
    // tiled: PT pixels per wave, [PT][G + 1] float4 of LDS, at most 16384 tiles
    r = rgk_resolve_plan(262144u, 3); // G = 8
    CHECK(r.PT == 64u && r.lds == 64u * 9u * 16u && r.grid == 4096);
    r = rgk_resolve_plan(200006u, 3); // ceil(200006 / 64) = 3126
    CHECK(r.grid == 3126);
    r = rgk_resolve_plan(16384u * 64u + 1u, 3);
    CHECK(r.grid == 16384);
    r = rgk_resolve_plan(65536u, 6); // G = 64
    CHECK(r.PT == 8u && r.lds == 8u * 65u * 16u && r.grid == 8192);
    r = rgk_resolve_plan(16384u * 8u + 1u, 6);
    CHECK(r.grid == 16384);
    r = rgk_resolve_plan(100u, 1); // G = 2
    CHECK(r.PT == 64u && r.lds == 64u * 3u * 16u && r.grid == 2);
    r = rgk_resolve_plan(100u, 4); // G = 16: 512 / 16 pixels
    CHECK(r.PT == 32u && r.lds == 32u * 17u * 16u && r.grid == 4);
}

static void walker() {
    RgkWalker v = rgk_walker_variant(RgkTraceCfg{32, 32, nullptr});
    CHECK(v.stack == 32 && v.lds == 32);
    v = rgk_walker_variant(RgkTraceCfg{256, 32, nullptr});
    CHECK(v.stack == 256 && v.lds == 32);
    v = rgk_walker_variant(RgkTraceCfg{256, 16, nullptr});
    CHECK(v.stack == 256 && v.lds == 16);
    // the bundle walk, the whole table: wanted by switch 2, or by switch 1 while the lists are uncapped; taken by a pinhole camera
    // at gshift 3 over a stack with an overflow area
    for (int beam = 0; beam < 3; beam++)
        for (int capped = 0; capped < 2; capped++) {
            const bool wanted = rgk_beam_wanted(beam, capped != 0);
            CHECK(wanted == (beam == 2 || (beam == 1 && capped == 0)));
            for (int gi = 0; gi < 2; gi++)
                for (int lens = 0; lens < 2; lens++)
                    for (int ovf = 0; ovf < 2; ovf++) {
                        const uint32_t gshift = gi ? 3u : 0u;
                        const RgkTraceCfg tc = ovf ? RgkTraceCfg{256, 16, nullptr} : RgkTraceCfg{32, 32, nullptr};
                        const bool expect = wanted && gi == 1 && lens == 0 && ovf == 1;
                        CHECK(rgk_beam_taken(wanted, gshift, lens != 0, tc) == expect);
                    }
        }
    CHECK(rgk_beam_taken(true, 3u, false, RgkTraceCfg{256, 32, nullptr}));
    CHECK(!rgk_beam_taken(true, 2u, false, RgkTraceCfg{256, 16, nullptr}));
}

// the passes the host's two loops make of a plan: pixel ranges x sample passes
struct Passes {
    size_t ranges = 0, first_range = 0, last_range = 0;
    uint32_t sample_passes = 0, ns[64] = {};
};
static Passes expand(size_t P, uint32_t multisample, const RgkPassPlan& p) {
    Passes o;
    for (size_t j0 = 0; j0 < P; j0 += p.npix_pass) {
        const size_t n = P - j0 < p.npix_pass ? P - j0 : p.npix_pass;
        if (o.ranges++ == 0) o.first_range = n;
        o.last_range = n;
    }
    for (uint32_t s0 = 0; s0 < multisample; s0 += p.ns_pass) o.ns[o.sample_passes++] = multisample - s0 < p.ns_pass ? multisample - s0 : p.ns_pass;
    return o;
}
static void passes() {
    // Cornell 512 x 512 x 16 spp
    Passes o = expand(262144, 16, rgk_plan_passes(262144, 16, 2097152));
    CHECK(o.ranges == 1 && o.first_range == 262144 && o.sample_passes == 2 && o.ns[0] == 8 && o.ns[1] == 8);
    o = expand(262144, 16, rgk_plan_passes(262144, 16, 1572864));
    CHECK(o.ranges == 1 && o.first_range == 262144 && o.sample_passes == 3 && o.ns[0] == 6 && o.ns[1] == 6 && o.ns[2] == 4);
    o = expand(262144, 16, rgk_plan_passes(262144, 16, 524288));
    CHECK(o.ranges == 1 && o.sample_passes == 8);
    for (int k = 0; k < 8; k++) CHECK(o.ns[k] == 2);
    o = expand(262144, 16, rgk_plan_passes(262144, 16, 200006));
    CHECK(o.ranges == 2 && o.first_range == 200006 && o.last_range == 62138 && o.sample_passes == 16);
    for (int k = 0; k < 16; k++) CHECK(o.ns[k] == 1);
    // Cornell 256 x 256 x 32 spp
    o = expand(65536, 32, rgk_plan_passes(65536, 32, 50000));
    CHECK(o.ranges == 2 && o.first_range == 50000 && o.last_range == 15536 && o.sample_passes == 32);
    for (int k = 0; k < 32; k++) CHECK(o.ns[k] == 1);
    o = expand(65536, 32, rgk_plan_passes(65536, 32, 300000));
    CHECK(o.ranges == 1 && o.first_range == 65536 && o.sample_passes == 8);
    for (int k = 0; k < 8; k++) CHECK(o.ns[k] == 4);
    // room for everything: one pass
    o = expand(4096, 8, rgk_plan_passes(4096, 8, (size_t)1 << 28));
    CHECK(o.ranges == 1 && o.sample_passes == 1 && o.ns[0] == 8);

    // 2^gshift samples side by side: the asked-for group, lowered until it divides the pass's samples
    CHECK(rgk_plan_gshift(-1, 3u, 8u) == 3u);
    CHECK(rgk_plan_gshift(-1, 3u, 6u) == 1u);
    CHECK(rgk_plan_gshift(-1, 3u, 4u) == 2u);
    CHECK(rgk_plan_gshift(-1, 3u, 1u) == 0u);
    CHECK(rgk_plan_gshift(6, 3u, 16u) == 4u);
    CHECK(rgk_plan_gshift(6, 3u, 64u) == 6u);
    CHECK(rgk_plan_gshift(0, 3u, 8u) == 0u);

    // pixel groups of 8 consecutive pixels of the round's list
    static_assert(RGK_ENTRY_SHIFT == 3 && RGK_ENTRY_PIX == 8u, "groups of 8 pixels");
    RgkGroupRange g = rgk_group_range(200006u, 62138u); // pixel 200006 sits in group 25000, pixel 262143 in group 32767
    CHECK(g.first == 25000u && g.last == 32768u && g.count() == 7768u);
    g = rgk_group_range(0u, 200006u); // ... and pixel 200005 in group 25000 as well: both ranges touch it
    CHECK(g.first == 0u && g.last == 25001u);
    g = rgk_group_range(0u, 8u);
    CHECK(g.first == 0u && g.last == 1u);
    g = rgk_group_range(0u, 9u);
    CHECK(g.last == 2u);
    g = rgk_group_range(0x7ffffff0u, 0xfu); // the last pixels a round can hold: no 32-bit overflow
    CHECK(g.first == 0x0ffffffeu && g.last == 0x10000000u);
}

int main(int argc, char** argv) {
    const char* c = argc > 1 ? argv[1] : "";
    if (!std::strcmp(c, "grids")) grids();
    else if (!std::strcmp(c, "resolve")) resolve();
    else if (!std::strcmp(c, "walker")) walker();
    else if (!std::strcmp(c, "passes")) passes();
    else { std::fprintf(stderr, "unknown case '%s'\n", c); return 2; }
    if (failures) std::fprintf(stderr, "%d condition(s) failed in case %s\n", failures, c);
    return failures ? 1 : 0;
}
