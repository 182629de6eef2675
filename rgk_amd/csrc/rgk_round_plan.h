// The host runtime's arithmetic, the part that needs no device: the workspace a pass of B paths takes, what a finished pass adds to
// the round's counters, how the per-launch records fold into the kernel classes, the tile list -> pixel-list offsets, the
// centre-out task list, the key of a frame's cached lists, and the traversal-stack configuration of a tree.  Plain C++17 over
// rgk.h's structs -- no call into the HIP runtime -- so the unit builds with any host compiler and runs under sanitizers
// (tests/cpp/round_plan_main.cpp includes it alone).  The host files call these instead of restating the formulas.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rgk.h"
#include "rgk_plan.h" // rgk_trace_grid, RGK_ENTRY_PIX

#pragma GCC visibility push(hidden) // host-internal: nothing here is an export of the library (popped at the end)

// What this unit needs of rgk_kernels.h, which needs the HIP runtime: the words of a device counter block the host reads, the
// float4 per stored light vertex, the entry nodes per pixel group.  rgk_round.cpp static_asserts each against that header.
constexpr uint32_t RGK_RP_CNT_QUEUE = 0, RGK_RP_CNT_SHADOW = 64, RGK_RP_CNT_HITS = 320, RGK_RP_CNT_SRAYS = 384, RGK_RP_CNT_CONN = 448, RGK_RP_CNT_TOTAL = 576;
constexpr uint32_t RGK_RP_LV_FLOAT4 = 6;
#ifndef RGK_ENTRY_K
#define RGK_ENTRY_K 6 // (the same guarded default as rgk_kernels.h)
#endif

// ------------------------------------------------------------------ workspace
// The per-path planes of the workspace, in allocation order: a plane holds (per_path + per_reverse * reverse) elements of `bytes`
// bytes per path; the `bidir` ones exist only for reverse > 0.  ensure_workspace allocates by this table, batch_paths sums it.
enum RgkPlaneId {
    RGK_WS_RAYA0, RGK_WS_RAYB0, RGK_WS_RAYA1, RGK_WS_RAYB1, RGK_WS_HIT, RGK_WS_THR, RGK_WS_TOT,
    RGK_WS_SHA, RGK_WS_SHB, RGK_WS_SHC, // plain shadow queue: one ray {shA, shB, shC} per path and bounce
    RGK_WS_LSTART, RGK_WS_LV, RGK_WS_HITLIST, RGK_WS_LVMASK, RGK_WS_CONNLIST,
    RGK_WS_CONN, // the record a camera vertex with connections leaves
    RGK_WS_JOBS, // vertex queue: {vertex}{contribution, mask}{emission}{NEE ray start}
    RGK_WS_RADS, // ... and one radiance per ray
    RGK_WS_LIGHT, RGK_WS_GENERIC, RGK_WS_PLANES
};
struct RgkWorkspacePlane { RgkPlaneId id; const char* name; uint32_t bytes, per_path, per_reverse; bool bidir; };
constexpr RgkWorkspacePlane RGK_WORKSPACE[RGK_WS_PLANES] = {
    {RGK_WS_RAYA0, "rayA0", 16, 1, 0, false}, {RGK_WS_RAYB0, "rayB0", 16, 1, 0, false}, {RGK_WS_RAYA1, "rayA1", 16, 1, 0, false}, {RGK_WS_RAYB1, "rayB1", 16, 1, 0, false},
    {RGK_WS_HIT, "hit", 16, 1, 0, false}, {RGK_WS_THR, "thr", 16, 1, 0, false}, {RGK_WS_TOT, "tot", 16, 1, 0, false},
    {RGK_WS_SHA, "shA", 16, 1, 0, false}, {RGK_WS_SHB, "shB", 16, 1, 0, false}, {RGK_WS_SHC, "shC", 16, 1, 0, false},
    {RGK_WS_LSTART, "lstart", 16, 1, 0, true}, {RGK_WS_LV, "lv", 16, 0, RGK_RP_LV_FLOAT4, true},
    {RGK_WS_HITLIST, "hitlist", 4, 1, 0, true}, {RGK_WS_LVMASK, "lvmask", 4, 1, 0, true}, {RGK_WS_CONNLIST, "connlist", 4, 1, 0, true},
    {RGK_WS_CONN, "conn", 16, 6, 0, true}, {RGK_WS_JOBS, "jobs", 16, 4, 0, true}, {RGK_WS_RADS, "rads", 16, 1, 1, true},
    {RGK_WS_LIGHT, "light", 16, 1, 0, false}, {RGK_WS_GENERIC, "generic", 4, 1, 0, false},
};
// elements of a plane for `paths` paths (0: the plane does not exist at this `reverse`)
inline size_t rgk_plane_elems(const RgkWorkspacePlane& pl, size_t paths, uint32_t reverse) {
    return (pl.bidir && !reverse) ? 0 : paths * ((size_t)pl.per_path + (size_t)pl.per_reverse * reverse);
}
inline size_t rgk_workspace_bytes_per_path(uint32_t reverse) {
    size_t b = 0;
    for (const RgkWorkspacePlane& pl : RGK_WORKSPACE) b += rgk_plane_elems(pl, 1, reverse) * pl.bytes;
    return b;
}

// ------------------------------------------------------------------ round counters
// A finished pass's share of the round's totals, from its host counter blocks (`cam`: camera phase, `light`: light sub-path phase):
// path and shadow rays as the reference counts them, and what each kernel processed (rays / vertices / paths).  n0: npix * ns.
inline void rgk_add_pass_counters(const uint32_t* cam, const uint32_t* light, uint32_t depth, uint32_t reverse, uint32_t n0, bool light_entry, rgk_counters& c) {
    auto units = [&c](int k) -> uint64_t& { return c.kernel[k].units; };
    for (uint32_t b = 0; b < depth; b++) { c.path_rays += cam[RGK_RP_CNT_QUEUE + b]; c.shadow_rays += cam[RGK_RP_CNT_SHADOW + b] + cam[RGK_RP_CNT_SRAYS + b]; }
    units(RGK_K_TRACE_CAMERA) += cam[RGK_RP_CNT_QUEUE]; units(RGK_K_SHADE_FIRST) += cam[RGK_RP_CNT_QUEUE];
    for (uint32_t b = 1; b < depth; b++) { units(RGK_K_TRACE_CLOSEST) += cam[RGK_RP_CNT_QUEUE + b]; units(RGK_K_SHADE) += cam[RGK_RP_CNT_QUEUE + b]; }
    for (uint32_t b = 0; b < depth; b++) {
        units((b == 0 && light_entry) ? RGK_K_SHADOW_FIRST : RGK_K_SHADOW) += cam[RGK_RP_CNT_SHADOW + b];
        units(RGK_K_SHADOW_JOBS) += cam[RGK_RP_CNT_CONN + b]; units(RGK_K_CONNECT) += cam[RGK_RP_CNT_CONN + b];
    }
    for (uint32_t k = 0; k < reverse; k++) {
        units(RGK_K_LIGHT_TRACE) += light[RGK_RP_CNT_QUEUE + k]; units(RGK_K_LIGHT_SHADE) += light[RGK_RP_CNT_HITS + k];
        units(RGK_K_LIGHT_SPLAT) += light[RGK_RP_CNT_SHADOW + k];
    }
    units(RGK_K_RESOLVE) += n0;
    // (light rays: the reference traces and counts one per path, path_tracer.cpp:126,349 -- the ones culled before the queue included)
    for (uint32_t k = 0; k < reverse; k++) { c.path_rays += k == 0 ? n0 : light[RGK_RP_CNT_QUEUE + k]; c.shadow_rays += light[RGK_RP_CNT_SHADOW + k]; }
}

// ------------------------------------------------------------------ kernel classes
// The class of a launch's kernel (rgk_kernel_id): closest-hit traversal, shadow traversal, shading, the rest.
enum RgkKernelClass { RGK_CLASS_CLOSEST, RGK_CLASS_SHADOW, RGK_CLASS_SHADE, RGK_CLASS_OTHER };
inline RgkKernelClass rgk_kernel_class(int k) {
    if (k == RGK_K_TRACE_CAMERA || k == RGK_K_TRACE_CLOSEST || k == RGK_K_LIGHT_TRACE) return RGK_CLASS_CLOSEST;
    if (k == RGK_K_SHADOW_FIRST || k == RGK_K_SHADOW || k == RGK_K_SHADOW_JOBS || k == RGK_K_LIGHT_SPLAT) return RGK_CLASS_SHADOW;
    if (k == RGK_K_SHADE_FIRST || k == RGK_K_SHADE || k == RGK_K_CONNECT || k == RGK_K_LIGHT_SHADE) return RGK_CLASS_SHADE;
    return RGK_CLASS_OTHER;
}
inline bool rgk_kernel_traverses(int k) { return rgk_kernel_class(k) <= RGK_CLASS_SHADOW; }
struct RgkLaunchTime { int kernel; float ms; };                // a timed launch
struct RgkStatSnap { int kernel; unsigned long long v[4]; };   // the traversal counters read back behind a traversal launch:
                                                               // closest nodes / triangles, shadow nodes / triangles (running totals)
// The launch records of a round -> rgk_counters::kernel and the four class sums.  A kernel's traversal counters are the
// differences between consecutive read-backs, in its class's pair of words.
inline void rgk_fold_kernel_log(const RgkLaunchTime* times, size_t n_times, const RgkStatSnap* snaps, size_t n_snaps, rgk_counters& c) {
    for (size_t i = 0; i < n_times; i++) {
        const float ms = times[i].ms;
        rgk_kernel_stat& ks = c.kernel[times[i].kernel];
        ks.ms += ms; ks.launches++;
        switch (rgk_kernel_class(times[i].kernel)) {
        case RGK_CLASS_CLOSEST: c.ms_trace += ms; c.n_trace_launches++; break;
        case RGK_CLASS_SHADOW: c.ms_shadow += ms; c.n_shadow_launches++; break;
        case RGK_CLASS_SHADE: c.ms_shade += ms; c.n_shade_launches++; break;
        case RGK_CLASS_OTHER: c.ms_other += ms; break;
        }
    }
    unsigned long long prev[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < n_snaps; i++) {
        rgk_kernel_stat& ks = c.kernel[snaps[i].kernel];
        const int o = rgk_kernel_class(snaps[i].kernel) == RGK_CLASS_CLOSEST ? 0 : 2;
        ks.node_visits += snaps[i].v[o] - prev[o];
        ks.tri_tests += snaps[i].v[o + 1] - prev[o + 1];
        for (int w = 0; w < 4; w++) prev[w] = snaps[i].v[w];
    }
}

// ------------------------------------------------------------------ tiles and tasks
static_assert(sizeof(rgk_tile) == 5 * sizeof(uint32_t), "rgk_tile layout"); // (device tile lists are 5 words per tile)
// The tiles checked against the frame, and their offsets into the pixel list they make (toff[n_tiles]: its length, < 2^31).
// `bad`: the tile at which the list was refused.
enum RgkTilesStatus { RGK_TILES_OK = 0, RGK_TILES_OUTSIDE, RGK_TILES_TOO_MANY_PIXELS };
inline RgkTilesStatus rgk_tile_offsets(uint32_t xres, uint32_t yres, const rgk_tile* tiles, uint32_t n_tiles, std::vector<uint32_t>& toff, uint32_t& bad) {
    toff.assign((size_t)n_tiles + 1, 0u);
    for (uint32_t i = 0; i < n_tiles; i++) {
        const rgk_tile& t = tiles[i];
        bad = i;
        if (t.x1 > xres || t.y1 > yres || t.x0 > t.x1 || t.y0 > t.y1) return RGK_TILES_OUTSIDE;
        const uint64_t n = (uint64_t)toff[i] + (uint64_t)(t.x1 - t.x0) * (t.y1 - t.y0);
        if (n >= (1ull << 31)) return RGK_TILES_TOO_MANY_PIXELS;
        toff[i + 1] = (uint32_t)n;
    }
    return RGK_TILES_OK;
}
// GenerateTaskList: the frame cut into tiles of tile_size, row-major, then stably sorted by the distance of a tile's midpoint from
// (mid_x, mid_y); task i gets seed0 + i (`seedstart + c`, render_driver.cpp:160,173).
inline std::vector<rgk_tile> rgk_task_list(uint32_t tile_size, uint32_t xres, uint32_t yres, float mid_x, float mid_y, uint32_t seed0) {
    struct T { rgk_tile t; float d; };
    std::vector<T> v;
    for (uint32_t yp = 0; yp < yres; yp += tile_size)
        for (uint32_t xp = 0; xp < xres; xp += tile_size) {
            T t;
            t.t.x0 = xp; t.t.x1 = std::min(xres, xp + tile_size);
            t.t.y0 = yp; t.t.y1 = std::min(yres, yp + tile_size);
            t.t.seed = 0;
            float mx = (t.t.x0 + t.t.x1) / 2.0f, my = (t.t.y0 + t.t.y1) / 2.0f; // RenderTask::midpoint tracer.hpp:18
            float dx = mid_x - mx, dy = mid_y - my;
            t.d = std::sqrt(dx * dx + dy * dy);
            v.push_back(t);
        }
    std::stable_sort(v.begin(), v.end(), [](const T& a, const T& b) { return a.d < b.d; });
    std::vector<rgk_tile> out(v.size());
    for (size_t i = 0; i < v.size(); i++) { out[i] = v[i].t; out[i].seed = seed0 + (uint32_t)i; }
    return out;
}
// The key of a frame's cached lists (entry nodes per pixel group): they depend on the camera and on which pixels the round's list
// holds in which order -- not on the seeds, so a frame's rounds share them.  FNV-1a over the camera, the resolution and
// x0, x1, y0, y1 of every tile (the seed is the fifth word).
inline uint64_t rgk_frame_list_key(const rgk_camera& camera, uint32_t xres, uint32_t yres, const rgk_tile* tiles, uint32_t n_tiles) {
    uint64_t key = 1469598103934665603ull;
    auto mix = [&key](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; i++) { key ^= b[i]; key *= 1099511628211ull; } };
    mix(&camera, sizeof(camera)); mix(&xres, sizeof(xres)); mix(&yres, sizeof(yres));
    for (uint32_t t = 0; t < n_tiles; t++) mix(&tiles[t], 4 * sizeof(uint32_t));
    return key;
}

// ------------------------------------------------------------------ traversal stack
// Entries per lane in LDS + per-lane overflow in global memory (rgk_kernels.hip RGK_TRACE_DISPATCH) for a tree that needs
// max_stack entries: the all-LDS 32/32 where the overflow is switched off and 32 are enough, else 256 / stack_lds.
// ovf_per_lane: overflow entries per lane (0: no overflow area); the area is rgk_trace_grid(lds) * RGK_TRACE_BLOCK lanes.
struct RgkStackPlan { int stack, lds; size_t ovf_per_lane; };
inline bool rgk_stack_plan(uint32_t max_stack, bool stack_ovf, int stack_lds, RgkStackPlan& out) { // false: the tree is too deep
    if (max_stack + 1 + RGK_ENTRY_K > 256) return false;
    const int need = (int)max_stack + 1 + RGK_ENTRY_K; // (+ the entry nodes a camera ray starts with)
    if (!stack_ovf && need <= 32) out = {32, 32, 0};
    else out = {256, stack_lds, 0};
    if (out.lds < out.stack) out.ovf_per_lane = (size_t)std::max(need - std::min(out.lds, 8), 1); // (k_trace_camera_beam keeps 8 entries in LDS)
    return true;
}
#pragma GCC visibility pop
