// Launch plans, the part that needs no device: how a round is cut into passes, which walker a launch takes and how large
// every grid is.  Pure functions over plain integers -- no call into the HIP runtime, no stream, no device buffer -- so the
// unit builds with any host compiler and runs under sanitizers (tests/cpp/plan_main.cpp includes it alone).  The host
// (rgk_scene.cpp, rgk_round.cpp) and the launch wrappers (rgk_kernels.hip) call these instead of restating the formulas.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#ifndef RGK_TRACE_BLOCK
#define RGK_TRACE_BLOCK 256
#endif
#ifndef RGK_SHADE_BLOCK
#define RGK_SHADE_BLOCK 512
#endif
#ifndef RGK_LIGHT_BLOCK
#define RGK_LIGHT_BLOCK RGK_SHADE_BLOCK // the light sub-path's kernels (rgk_bdpt.h)
#endif
#ifndef RGK_SHADE_BLOCK_LATER
#define RGK_SHADE_BLOCK_LATER 256 // k_shade at bounce >= 1 (see there)
#endif
#ifndef RGK_ENTRY_SHIFT
#define RGK_ENTRY_SHIFT 3 // log2 of the pixels per group: consecutive pixels of the round's list (8x8 blocks, row-major inside: a row of 8)
// (Sponza proxy, ms per round: off 146.6; K, pixels = 4, 64: 138.8; 8, 64: 137.5; 4, 16: 139.4; 4, 8: 139.1; 6, 8: 136.3; 8, 8: 136.2)
#endif
#define RGK_ENTRY_PIX (1u << RGK_ENTRY_SHIFT)
#if defined(__HIPCC__)
#define RGK_PLAN_HD __host__ __device__ // what a kernel calls too
#else
#define RGK_PLAN_HD
#endif

// Compute units every full grid is sized for (MI355X).  A constant, not a device query: the grids are part of what was measured.
constexpr int RGK_CUS = 256;

// traversal-stack configuration of a scene: entries its tree can need, how many of them live in LDS, overflow area
struct RgkTraceCfg {
    int stack, lds;
    int* ovf;
};

// ------------------------------------------------------------------ passes of a round
// P pixels x `multisample` samples with room for B paths per pass: pixel ranges of npix_pass pixels x equal-sized sample passes
// of ns_pass samples (the last of either may be shorter).
struct RgkPassPlan { size_t npix_pass; uint32_t ns_pass; };
inline RgkPassPlan rgk_plan_passes(size_t P, uint32_t multisample, size_t B) {
    const size_t npix_pass = std::min(P, B);
    const uint32_t ns_max = (uint32_t)std::max<size_t>(1, std::min<size_t>(multisample, B / npix_pass));
    const uint32_t n_sample_passes = (multisample + ns_max - 1) / ns_max;
    return {npix_pass, (multisample + n_sample_passes - 1) / n_sample_passes}; // equal-sized passes
}
// 2^gshift samples of a pixel side by side in the slot order (rgk_kernels.h PassParams): the scene's sample_group (-1: `dflt`),
// lowered until it divides the pass's ns samples
inline uint32_t rgk_plan_gshift(int sample_group, uint32_t dflt, uint32_t ns) {
    uint32_t g = sample_group >= 0 ? (uint32_t)sample_group : dflt;
    while (g && (ns & ((1u << g) - 1u))) g--;
    return g;
}
// the pixel groups [first, last) a pass over pixels [j0, j0 + npix) of the round's list touches
struct RgkGroupRange { uint32_t first, last; uint32_t count() const { return last - first; } };
inline RgkGroupRange rgk_group_range(uint32_t j0, uint32_t npix) { return {j0 >> RGK_ENTRY_SHIFT, (uint32_t)(((size_t)j0 + npix + RGK_ENTRY_PIX - 1u) >> RGK_ENTRY_SHIFT)}; }

// ------------------------------------------------------------------ the bundle walk of bounce 0 (k_trace_camera_beam)
// Asked for (PassParams::beam) by the scene's switch -- 1: while the pass's entry lists are uncapped, 2: always, 0: never:
// measured on the headline workload, camera launch 20.6 (per ray, uncapped) -> 17.2 ms (bundles), a one-round frame
// 135.2 -> 130.8 ms; against CAPPED lists the per-ray walk is the faster one (16.1 vs 17.2: a bundle tests every triangle it
// meets against all 8 rays, 2.86 tests per ray instead of 2.57, at half the occupancy)
inline bool rgk_beam_wanted(int tune_beam, bool lists_capped) { return tune_beam == 2 || (tune_beam == 1 && !lists_capped); }
// ... and taken by the launch when a lane can hold a pixel's 8 samples: pinhole camera, gshift 3, a stack with an overflow area
inline bool rgk_beam_taken(bool wanted, uint32_t gshift, bool lens, const RgkTraceCfg& tc) { return wanted && gshift == 3 && !lens && tc.lds < tc.stack; }
// its queue holds one entry per 8 rays
inline uint32_t rgk_beam_bound(uint32_t bound) { return (bound >> 3) + 1u; }

// ------------------------------------------------------------------ grids
// `bound`: an upper bound on the length of the queue a launch consumes (the host reads a queue counter back every few bounces of
// a deep path loop): a 40-bounce round ends in dozens of launches over a few hundred rays, and a full persistent grid of 3000
// waves then costs more in work-fetch atomics and LDS fills than the rays themselves.  Every consumer is persistent or
// grid-stride, so a bound changes the time a launch takes and never its result.
inline int rgk_bounded_grid(int full, uint32_t items, uint32_t per_block) {
    const uint64_t need = ((uint64_t)items + per_block - 1) / per_block;
    return (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)full, need));
}
// workgroups of a full persistent trace launch: LDS-limited residency (entries * RGK_TRACE_BLOCK * 4 B per block out of 160 KiB) x CUs
inline int rgk_trace_grid(int lds_entries) { return RGK_CUS * std::max(1, std::min(8, (160 * 1024) / (lds_entries * RGK_TRACE_BLOCK * 4))); }
// (stack need, LDS entries) variants of the walkers.  Default 256/16: 16 entries per lane in LDS, the rest -- reached only by the
// deep part of a walk -- per lane in global memory.  That keeps 8 workgroups per CU resident whatever the tree depth
// (occupancy was LDS-bound: 5 per CU with 32 entries, 3 with 48), and more waves are what the L1-latency-bound half
// of the kernel wanted: Sponza trace launch 40.3 -> 33.8 ms, shadow 25 -> 20 ms per round (32 / 24 / 16 / 12 / 8
// entries: 40.3 / 37.0 / 35.1 / 35.5 / 35.2 ms at 7 waves per SIMD; 16 entries at 8 waves: 34.2).
// RGK_STACK_LDS=32 selects 256/32, RGK_STACK_OVF=0 the all-LDS 32/32 (shallow trees only).
struct RgkWalker { int stack, lds; }; // the kernels' <STACK, LDSN>
inline RgkWalker rgk_walker_variant(const RgkTraceCfg& tc) { return (tc.stack <= 32 && tc.lds == 32) ? RgkWalker{32, 32} : RgkWalker{256, tc.lds == 32 ? 32 : 16}; }
// a fast / GENERIC pair of shading launches over the same queue (k_shade, k_shade_light): the second shades what the first listed
struct RgkGridPair { int fast, generic, block; };
inline RgkGridPair rgk_pair_grids(int block, uint32_t bound) {
    return {rgk_bounded_grid(RGK_CUS * 4 * 512 / block, bound, (uint32_t)block), rgk_bounded_grid(RGK_CUS * 2 * 512 / block, bound, (uint32_t)block), block};
}
inline RgkGridPair rgk_shade_grids(uint32_t bounce, uint32_t bound) { return rgk_pair_grids(bounce == 0 ? RGK_SHADE_BLOCK : RGK_SHADE_BLOCK_LATER, bound); }
// The bounce whose vertices are all their paths' last (k_last_vertex, rgk_shade.h): bounce b's queue holds the vertices with
// n == b + 1.  Bounce 0 keeps k_shade<FIRST> (it samples the path's light and starts the slot sums), bidirectional rounds k_shade<BDPT>.
inline bool rgk_last_bounce(uint32_t bounce, uint32_t depth, bool bdpt) { return bounce >= 1 && bounce + 1 == depth && !bdpt; }
// ... and its grid: the record ring (rgk_ring.h) leaves room for three workgroups of 256 per CU, the grid is two rounds of them.
// (Measured on the headline, ms of the launch per step at 3 / 6 / 12 / 24 workgroups per CU: 17.18 / 17.14 / 17.03 / 17.00 -- within
// the launch's own spread, profiles/last_vertex_kernel.txt.)
#ifndef RGK_LAST_VERTEX_WGS
#define RGK_LAST_VERTEX_WGS 6
#endif
inline int rgk_last_vertex_grid(uint32_t bound) { return rgk_bounded_grid(RGK_CUS * RGK_LAST_VERTEX_WGS, bound, RGK_SHADE_BLOCK_LATER); }
// the light sub-path: k_shade_light's pair; k_raygen_light and k_list_hits take the pair's first grid
inline RgkGridPair rgk_light_grids(uint32_t bound) { return rgk_pair_grids(RGK_LIGHT_BLOCK, bound); }
constexpr int RGK_CONNECT_BLOCK = 256;
inline int rgk_connect_grid(uint32_t bound) { return rgk_bounded_grid(RGK_CUS * 8, bound, RGK_CONNECT_BLOCK); }
// k_aov_hop (rgk_post.hip): workgroups of 256 over a queue of at most `bound` entries (the call's pixels)
inline int rgk_aov_hop_grid(uint32_t bound) { return rgk_bounded_grid(RGK_CUS * 8, bound, 256u); }
// k_resolve (gshift 0: a thread per pixel) or k_resolve_tiled (a wave per `PT` pixels, staged through `lds` bytes)
struct RgkResolvePlan { int grid; uint32_t PT; size_t lds; };
inline RgkResolvePlan rgk_resolve_plan(uint32_t npix, uint32_t gshift) {
    if (gshift == 0) return {(int)std::min<uint32_t>((npix + 255u) / 256u, RGK_CUS * 16), 0u, 0};
    const uint32_t G = 1u << gshift;
    const uint32_t PT = G <= 8 ? 64u : 512u / G; // pixels per tile: ~9 KB of LDS per wave (more waves per CU matter more here than full lanes in the short summing phase)
    return {(int)std::min<uint32_t>((npix + PT - 1) / PT, RGK_CUS * 64), PT, (size_t)PT * (G + 1) * 16}; // (16: sizeof(float4))
}
// k_demod_divisor (rgk_post.hip): workgroups of 256 striding over the pass's slots; each fills the LDS tables once
inline int rgk_demod_divisor_grid(uint32_t slots) { return rgk_bounded_grid(RGK_CUS * 8, slots, 256u); }
// k_resolve_demod (rgk_post.hip): waves of 64 lanes for both slot orders, a lane per pixel; gshift > 0 stages two planes, tot and the
// divisors, so twice k_resolve_tiled's LDS at its tile size
inline RgkResolvePlan rgk_resolve_demod_plan(uint32_t npix, uint32_t gshift) {
    if (gshift == 0) return {(int)std::min<uint32_t>((npix + 63u) / 64u, RGK_CUS * 64), 64u, 0};
    const RgkResolvePlan r = rgk_resolve_plan(npix, gshift);
    return {r.grid, r.PT, 2 * r.lds};
}

// ------------------------------------------------------------------ denoisers and noise estimate (rgk_post.hip, k_dn_* / k_nz_*)
// a thread per pixel in blocks of 256; the filters' 2-D workgroups of 32 x 8 pixels; the statistics' workgroup per tile of
// tile_size x tile_size pixels (ragged at the right and bottom edges), tiles row-major
constexpr int RGK_POST_BLOCK = 256, RGK_POST_BX = 32, RGK_POST_BY = 8;
struct RgkGrid2 { uint32_t x, y; size_t count() const { return (size_t)x * y; } };
inline uint32_t rgk_post_pixel_grid(size_t P) { return (uint32_t)((P + RGK_POST_BLOCK - 1) / RGK_POST_BLOCK); }
inline RgkGrid2 rgk_post_filter_grid(uint32_t xres, uint32_t yres) { return {(xres + RGK_POST_BX - 1) / RGK_POST_BX, (yres + RGK_POST_BY - 1) / RGK_POST_BY}; }
inline RgkGrid2 rgk_nz_tile_grid(uint32_t xres, uint32_t yres, uint32_t tile_size) {
    return {(uint32_t)(((uint64_t)xres + tile_size - 1) / tile_size), (uint32_t)(((uint64_t)yres + tile_size - 1) / tile_size)};
}

// ------------------------------------------------------------------ display output (rgk_post.hip, k_display_hist / k_display_encode)
// Four pixels per lane when the planes a launch is given (a NULL one does not count) all start on 16-byte boundaries, else one; an
// item is such a group or one of the P % 4 pixels behind the last group (every pixel when not vectorised).  The grids: workgroups of
// RGK_POST_BLOCK lanes striding over the items, bounded -- each fills an LDS table (the histogram, the transfer table) once, and
// every workgroup of the histogram kernel ends with one global integer add per non-empty bin, all workgroups onto the same 257
// words: its time grows with the workgroups.  Measured at 1920 x 1080 on the Sponza proxy, ms by HIP events, at 256 / 512 / 1024 /
// 2048 / 4096 workgroups: k_display_hist 0.0155 / 0.0174 / 0.0252 / 0.0429 / 0.0435; k_display_encode (filmic) 0.0292 / 0.0210 /
// 0.0179 / 0.0169 / 0.0168 (an empty launch between two events reads 0.008).  So one workgroup per CU for the histogram, four for
// the encode (the last 0.001 ms is not worth a bound that only frames above two million pixels would reach).
#ifndef RGK_DISPLAY_HIST_WGS
#define RGK_DISPLAY_HIST_WGS RGK_CUS
#endif
#ifndef RGK_DISPLAY_ENCODE_WGS
#define RGK_DISPLAY_ENCODE_WGS (RGK_CUS * 4)
#endif
inline bool rgk_display_vec(const void* a, const void* b, const void* c) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0; }
inline size_t rgk_display_items(size_t P, bool vec) { return vec ? P / 4 + P % 4 : P; }
inline int rgk_display_grid(size_t P, bool vec, int full) {
    const size_t need = (rgk_display_items(P, vec) + RGK_POST_BLOCK - 1) / RGK_POST_BLOCK;
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)full, need));
}

// ------------------------------------------------------------------ the round fold (rgk_post.hip, k_round_fold)
// Workgroup (i, b) of RGK_POST_BLOCK threads takes band b of listed tile i: its rows [b * RGK_FOLD_ROWS, + RGK_FOLD_ROWS), cut at
// the tile's height (a band past it is empty: the grid is as high as the list's highest tile needs).  A band of `rows` rows of a
// tile `tw` pixels wide is rows * tw * C consecutive elements k of a plane with C values per pixel, row after row; thread t takes
// k = t, t + RGK_POST_BLOCK, ...: a wave's 64 lanes are 256 contiguous bytes of a row, or the end of one row and the start of
// the next.  A 32-pixel tile row is 96 floats (384 B) of an rgb plane; 8 rows are 3 rgb elements and one count per thread.
constexpr uint32_t RGK_FOLD_ROWS = 8;
inline RgkGrid2 rgk_fold_grid(uint32_t n_tiles, uint32_t max_tile_height) { return {n_tiles, (max_tile_height + RGK_FOLD_ROWS - 1) / RGK_FOLD_ROWS}; }
struct RgkRowRange { uint32_t r0, r1; };
RGK_PLAN_HD inline RgkRowRange rgk_fold_band(uint32_t band, uint32_t tile_height) {
    const uint64_t a = (uint64_t)band * RGK_FOLD_ROWS, b = a + RGK_FOLD_ROWS;
    return {(uint32_t)(a < tile_height ? a : tile_height), (uint32_t)(b < tile_height ? b : tile_height)};
}
// element k of the band that starts at frame row y (tile column x0, width tw) -> its index in a plane of xres * C values per row
RGK_PLAN_HD inline size_t rgk_fold_element(uint32_t xres, uint32_t x0, uint32_t y, uint32_t tw, uint32_t C, uint32_t k) {
    const uint32_t row = k / (tw * C), col = k - row * (tw * C);
    return ((size_t)(y + row) * xres + x0) * C + col;
}
