// Hand-written HIP kernels for gfx950 (MI355X): the wavefront path-tracing pipeline.  The kernels live in the headers below, one per
// concern, and the launch layer (host) follows them in the same order.  This translation unit instantiates all of them but k_shade
// and k_last_vertex: those two are rgk_shade_kernels.hip's, which is built with flags of its own (rgk_amd/build.py SOURCE_FLAGS).
//
//   rgk_trace.h          k_trace_camera  K1+K2  RenderPixel ray generation + FindIntersectKdOtherThan  reference src/path_tracer.cpp:53-61, src/camera.cpp:32-46
//                        k_trace_closest K2  FindIntersectKdOtherThan  reference src/scene_intersect.cpp:211-327 + src/primitives.cpp:75-166
//                        k_trace_shadow[_first][_cl], k_trace_shadow_jobs  K5  Scene::Visibility + accumulate  reference src/scene.cpp:670-673, src/path_tracer.cpp:431,455-457
//   rgk_shade.h          k_shade  K3/K4/K6/K7  GeneratePath body + NEE + compaction  reference src/path_tracer.cpp:134-300,427-460,485-496
//                        (launched from rgk_shade_kernels.hip);
//                        the queue records, the compaction and the path step that k_shade_light shares with it;
//                        k_last_vertex  the last bounce of a unidirectional pass: k_shade's last vertex in two phases (ring: rgk_ring.h)
//   rgk_bdpt.h           k_raygen_light, k_list_hits, k_shade_light, k_connect  K8  the bidirectional half (reverse > 0)
//   rgk_resolve.h        k_resolve[_tiled]  K9  clamp / NaN scrub / AddPixel  reference src/path_tracer.cpp:502-507, src/tracer.cpp:18, src/texture.cpp:342-347
//                        k_build_pixel_list, k_build_halton_table, k_init_counters  Tracer::Render pixel order + seeds; halton_raw per round
//   rgk_probe_kernels.h  k_pack_rays, k_pack_visibility, k_unpack_hits, k_sampler_eval, k_bxdf_value, k_bxdf_sample, k_texture_sample,
//                        k_libm_eval: the unit-level entries of rgk_probe.cpp; no round launches them
//   rgk_entry.h          k_entry_points, k_group_trange_wave, k_entry_points_light  where a pixel group's camera rays / first shadow rays
//                        start in the tree (no reference counterpart: work shared by the rays of a group)
//   here                 k_stage_mark, beside its launcher
// The order of the includes, and of the launchers that instantiate kernel templates, is the order of the kernels in the assembly:
// a kernel's labels carry its number in the file, so a reordering changes the text of every kernel behind it
// (tools/device_code_diff.sh, profiles/shade_pieces_device_code.txt).
//
// Design: one path per slot, SoA-of-float4 queues so every lane moves 16 B
// per load; persistent waves pull 64 rays at a time from a device-side counter; a
// per-lane traversal stack lives in LDS ([depth][lane] -> conflict-free) and idle lanes are
// refilled with fresh rays (rgk_trace.h); surviving paths are compacted into the next
// bounce's queue with a wave ballot + prefix popcount and one atomic per workgroup.
// No MFMA: there is no dense contraction on this path.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <type_traits>
#include "rgk_device.h"
#include "rgk_kernels.h"

#include "rgk_trace.h" // K2 / K5: persistent traversal with lane refill
#include "rgk_shade.h" // K3 / K4 / K6 / K7
#include "rgk_bdpt.h" // K8: light sub-path, splats, connections (reverse > 0)
#include "rgk_resolve.h" // K9, the round's lists
#include "rgk_probe_kernels.h" // the kernels behind rgk_probe.cpp
#include "rgk_entry.h" // entry points of camera rays and first shadow rays

// ------------------------------------------------------------------ launch wrappers (host): rgk_trace.h
// Grids, walker variants and the bounds that shrink them: rgk_plan.h.  A walker launch takes its grid from the bound the caller
// passes and its kernel's <COUNT, STACK, LDSN> from `count_stats` and the scene's stack configuration `tc`: launch(grid, variant)
// gets the three as the constants of the variant's type.
template <bool C, int S, int L>
struct WalkerKernel { static constexpr bool COUNT = C; static constexpr int STACK = S, LDSN = L; };
template <class Launch>
static void trace_dispatch(const RgkTraceCfg& tc, bool count_stats, uint32_t bound, Launch launch) {
    const int grid = rgk_bounded_grid(rgk_trace_grid(tc.lds), bound, RGK_TRACE_BLOCK);
    const RgkWalker v = rgk_walker_variant(tc);
    if (v.stack == 32) { if (count_stats) launch(grid, WalkerKernel<true, 32, 32>{}); else launch(grid, WalkerKernel<false, 32, 32>{}); }
    else if (v.lds == 32) { if (count_stats) launch(grid, WalkerKernel<true, 256, 32>{}); else launch(grid, WalkerKernel<false, 256, 32>{}); }
    else { if (count_stats) launch(grid, WalkerKernel<true, 256, 16>{}); else launch(grid, WalkerKernel<false, 256, 16>{}); }
}

// bounce 0 of a unidirectional pass: camera rays generated in the traversal kernel (no queue)
void rgk_launch_trace_camera(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, const RgkTraceCfg& tc, bool count_stats, float4* hit,
                             const RgkWalk& w, unsigned long long* stats) {
    if (rgk_beam_taken(pp.beam != 0, pp.gshift, cam.lens_size != 0.0f, tc)) {
        // 8 stack entries per lane in LDS (the rest in the overflow area): with the bundle's 32 floats per lane that makes 40 KB per
        // workgroup, four workgroups per CU
        const int grid = rgk_bounded_grid(rgk_trace_grid(tc.lds), rgk_beam_bound(w.bound), RGK_TRACE_BLOCK);
        if (count_stats) k_trace_camera_beam<true, 256, 8><<<grid, RGK_TRACE_BLOCK, 0, st>>>(sc, cam, pp, hit, w.count_ptr, w.fetch, stats, tc.ovf);
        else k_trace_camera_beam<false, 256, 8><<<grid, RGK_TRACE_BLOCK, 0, st>>>(sc, cam, pp, hit, w.count_ptr, w.fetch, stats, tc.ovf);
        return;
    }
    trace_dispatch(tc, count_stats, w.bound, [&](int grid, auto k) { k_trace_camera<k.COUNT, k.STACK, k.LDSN><<<grid, RGK_TRACE_BLOCK, 0, st>>>(sc, cam, pp, hit, w.count_ptr, w.fetch, stats, tc.ovf);
    });
}

void rgk_launch_trace_closest(hipStream_t st, const DevScene& sc, const RgkTraceCfg& tc, bool count_stats, const float4* rayA, const float4* rayB,
                              const float2* nearfar, float4* hit, const RgkWalk& w, unsigned long long* stats) {
    trace_dispatch(tc, count_stats, w.bound, [&](int grid, auto k) {
        k_trace_closest<k.COUNT, k.STACK, k.LDSN><<<grid, RGK_TRACE_BLOCK, 0, st>>>(sc, rayA, rayB, nearfar, hit, w.count_ptr, w.fetch, stats, tc.ovf);
    });
}

// Shadow rays, four kernels behind one entry.  first_pp: the pass whose FIRST vertices these rays leave, in a single-light scene:
// they start at the light-side entry nodes of their pixel group (pp.lentry).  rec32: the 32-byte records of the constant-light
// route, shA = {d.xyz, far}, shB = {radiance.rgb, slot}, every ray from sc.cl_pos with near = 20 eps (shC is not read).  Either of
// the two means a round's shadow launch: tot[slot] += radiance, so vis_out, mode and splat_rgb are for the plain kernel alone.
bool rgk_const_light_records() { return RGK_CL_REC32 != 0; }
void rgk_launch_trace_shadow(hipStream_t st, const DevScene& sc, const RgkTraceCfg& tc, bool count_stats, const float4* shA, const float4* shB,
                             const float4* shC, float4* tot, uint8_t* vis_out, int mode, float* splat_rgb, const RgkWalk& w, unsigned long long* stats,
                             const PassParams* first_pp, bool rec32) {
    if (!first_pp && !rec32) trace_dispatch(tc, count_stats, w.bound, [&](int grid, auto k) {
        k_trace_shadow<k.COUNT, k.STACK, k.LDSN><<<grid, RGK_TRACE_BLOCK, 0, st>>>(sc, shA, shB, shC, tot, vis_out, mode, splat_rgb, w.count_ptr, w.fetch, stats, tc.ovf);
    });
    else if (!rec32) trace_dispatch(tc, count_stats, w.bound, [&](int grid, auto k) {
        k_trace_shadow_first<k.COUNT, k.STACK, k.LDSN><<<grid, RGK_TRACE_BLOCK, 0, st>>>(sc, *first_pp, shA, shB, shC, tot, w.count_ptr, w.fetch, stats, tc.ovf);
    });
    else if (!first_pp) trace_dispatch(tc, count_stats, w.bound, [&](int grid, auto k) {
        k_trace_shadow_cl<k.COUNT, k.STACK, k.LDSN><<<grid, RGK_TRACE_BLOCK, 0, st>>>(sc, shA, shB, tot, w.count_ptr, w.fetch, stats, tc.ovf);
    });
    else trace_dispatch(tc, count_stats, w.bound, [&](int grid, auto k) {
        k_trace_shadow_first_cl<k.COUNT, k.STACK, k.LDSN><<<grid, RGK_TRACE_BLOCK, 0, st>>>(sc, *first_pp, shA, shB, tot, w.count_ptr, w.fetch, stats, tc.ovf);
    });
}

// ------------------------------------------------------------------ rgk_shade.h
// (k_shade and k_last_vertex are instantiated in rgk_shade_kernels.hip, a translation unit with compiler flags of its own; what this
// file takes from rgk_shade.h is the pieces that rgk_bdpt.h and rgk_probe_kernels.h share with them)

// ------------------------------------------------------------------ rgk_bdpt.h
void rgk_launch_raygen_light(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, float4* rayA, float4* rayB,
                             float4* thr, uint32_t* counters) {
    k_raygen_light<<<rgk_light_grids(pp.npix * pp.ns).fast, RGK_LIGHT_BLOCK, 0, st>>>(sc, cam, pp, rayA, rayB, thr, counters);
}
void rgk_launch_shade_light(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, uint32_t k, const float4* rayA,
                            const float4* rayB, const float4* hit, float4* thr, float4* nextA, float4* nextB, float4* shA, float4* shB,
                            float4* shC, uint32_t* counters, uint32_t bound) {
    const RgkGridPair g = rgk_light_grids(bound);
    k_shade_light<false><<<g.fast, g.block, RGK_LDS_SHADE_BYTES, st>>>(sc, cam, pp, k, rayA, rayB, hit, thr, nextA, nextB, shA, shB, shC, counters);
    k_shade_light<true><<<g.generic, g.block, RGK_LDS_SHADE_BYTES, st>>>(sc, cam, pp, k, rayA, rayB, hit, thr, nextA, nextB, shA, shB, shC, counters);
}
void rgk_launch_connect(hipStream_t st, const DevScene& sc, const PassParams& pp, uint32_t bounce, float4* jobs, float4* rads, uint32_t* counters, uint32_t bound) {
    k_connect<<<rgk_connect_grid(bound), RGK_CONNECT_BLOCK, RGK_LDS_SHADE_BYTES, st>>>(sc, pp, bounce, jobs, rads, counters);
}
void rgk_launch_list_hits(hipStream_t st, const float4* hit, const uint32_t* count_ptr, uint32_t* list, uint32_t* list_count, uint32_t bound) {
    k_list_hits<<<rgk_light_grids(bound).fast, RGK_LIGHT_BLOCK, 0, st>>>(hit, count_ptr, list, list_count);
}
// the walker of a bidirectional round's vertex queue (rgk_trace.h JOB).  Here, not with the other walker launchers: its kernels are
// the last walkers instantiated, and that is their place in the assembly
void rgk_launch_trace_shadow_jobs(hipStream_t st, const DevScene& sc, const PassParams& pp, const RgkTraceCfg& tc, bool count_stats, const float4* jobs, const float4* rads,
                                  float4* tot, const RgkWalk& w, unsigned long long* stats) {
    trace_dispatch(tc, count_stats, w.bound, [&](int grid, auto k) {
        k_trace_shadow_jobs<k.COUNT, k.STACK, k.LDSN><<<grid, RGK_TRACE_BLOCK, 0, st>>>(sc, pp, jobs, rads, tot, w.count_ptr, w.fetch, stats, tc.ovf);
    });
}

// ------------------------------------------------------------------ rgk_resolve.h
void rgk_launch_resolve(hipStream_t st, const PassParams& pp, const float4* tot, float4* pixsum, float* accum_rgb, uint32_t* accum_count) {
    const RgkResolvePlan r = rgk_resolve_plan(pp.npix, pp.gshift);
    if (pp.gshift == 0) k_resolve<<<r.grid, 256, 0, st>>>(pp, tot, pixsum, accum_rgb, accum_count);
    else k_resolve_tiled<<<r.grid, 64, r.lds, st>>>(pp, tot, pixsum, accum_rgb, accum_count, r.PT);
}

void rgk_launch_init_counters(hipStream_t st, uint32_t* counters, uint32_t n0) { k_init_counters<<<1, 256, 0, st>>>(counters, n0); }
void rgk_launch_build_pixel_list(hipStream_t st, const rgk_tile* tiles, const uint32_t* tile_off, uint32_t n_tiles, uint32_t* pix_xy, uint32_t* pix_seed) {
    k_build_pixel_list<<<n_tiles < 4096u ? n_tiles : 4096u, 256, 0, st>>>(tiles, tile_off, n_tiles, pix_xy, pix_seed);
}
void rgk_launch_build_halton_table(hipStream_t st, const DevScene& sc, uint32_t S, float* htab) {
    uint32_t n = 192u * S;
    k_build_halton_table<<<(n + 255) / 256, 256, 0, st>>>(sc, S, htab);
}
// the host's progress mark (defined here, behind the entry-point kernels of the includes: its place in the assembly)
__global__ void k_stage_mark(uint32_t* host_word, uint32_t v) { *(volatile uint32_t*)host_word = v; __threadfence_system(); }
void rgk_launch_stage_mark(hipStream_t st, uint32_t* host_word, uint32_t v) { k_stage_mark<<<1, 1, 0, st>>>(host_word, v); }

// ------------------------------------------------------------------ rgk_probe_kernels.h
void rgk_launch_pack_rays(hipStream_t st, uint32_t n, const float* rays, const int32_t* ignore, float4* rayA, float4* rayB, float2* nearfar) {
    k_pack_rays<<<(n + 255) / 256, 256, 0, st>>>(n, rays, ignore, rayA, rayB, nearfar);
}
void rgk_launch_pack_visibility(hipStream_t st, const DevScene& sc, uint32_t n, const float* a, const float* b, float4* shA, float4* shB, float4* shC) {
    k_pack_visibility<<<(n + 255) / 256, 256, 0, st>>>(sc, n, a, b, shA, shB, shC);
}
void rgk_launch_unpack_hits(hipStream_t st, uint32_t n, const float4* hit, rgk_hit* out) { k_unpack_hits<<<(n + 255) / 256, 256, 0, st>>>(n, hit, out); }
void rgk_launch_sampler_eval(hipStream_t st, const DevScene& sc, uint32_t n, const uint32_t* seed, const uint32_t* index, const uint32_t* dim,
                             int is2d, float* out) {
    k_sampler_eval<<<(n + 255) / 256, 256, 0, st>>>(sc, n, seed, index, dim, is2d, out);
}
void rgk_launch_libm_eval(hipStream_t st, int fn, uint32_t n, const float* a, const float* b, float* out) { k_libm_eval<<<(n + 255) / 256, 256, 0, st>>>(fn, n, a, b, out); }
void rgk_launch_bxdf_value(hipStream_t st, const DevScene& sc, uint32_t n, uint32_t route, const uint32_t* mat, const float* Vi, const float* Vr, const float* uv, float* out) {
    k_bxdf_value<<<(n + 255) / 256, 256, RGK_LDS_SHADE_BYTES, st>>>(sc, n, route, mat, Vi, Vr, uv, out);
}
void rgk_launch_bxdf_sample(hipStream_t st, const DevScene& sc, uint32_t n, uint32_t route, const uint32_t* mat, const float* Vi, const float* uv, const float* u,
                            float* out_dir, float* out_w, uint8_t* leak) {
    k_bxdf_sample<<<(n + 255) / 256, 256, RGK_LDS_SHADE_BYTES, st>>>(sc, n, route, mat, Vi, uv, u, out_dir, out_w, leak);
}
void rgk_launch_texture_sample(hipStream_t st, const DevScene& sc, uint32_t n, const TexRef* refs, const int32_t* tex, const float* uv, float* rgb, float* sr, float* sb) {
    k_texture_sample<<<(n + 255) / 256, 256, RGK_LDS_SHADE_BYTES, st>>>(sc, n, refs, tex, uv, rgb, sr, sb);
}

// ------------------------------------------------------------------ rgk_entry.h
void rgk_launch_entry_points(hipStream_t st, const DevScene& sc, const DevCamera& cam, uint32_t xres, uint32_t yres, const uint32_t* pix_xy, uint32_t n_pixels,
                             uint32_t g_first, uint32_t g_count, const uint32_t* trange, int* entries, float* cap) {
    k_entry_points<<<(g_count + 63u) / 64u, 64, 0, st>>>(sc, cam, xres, yres, pix_xy, n_pixels, g_first, g_count, trange, entries, cap);
}
// nearest / farthest first hit per pixel group of a finished bounce-0 trace of this pass
void rgk_launch_group_trange(hipStream_t st, const PassParams& pp, const float4* hit, uint32_t* trange) {
    const RgkGroupRange g = rgk_group_range(pp.j0, pp.npix);
    k_group_trange_wave<<<g.count(), 64, 0, st>>>(pp, hit, g.first, g.count(), trange);
}
void rgk_launch_light_entry_points(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, uint32_t n_pixels_round, const uint32_t* trange, int* entries, float4* lbox) {
    const RgkGroupRange g = rgk_group_range(pp.j0, pp.npix);
    k_entry_points_light<<<(g.count() + 63u) / 64u, 64, 0, st>>>(sc, cam, pp.xres, pp.yres, pp.pix_xy, n_pixels_round, g.first, g.count(), trange, entries, lbox);
}
