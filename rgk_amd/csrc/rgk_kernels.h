// Launch interface between the host runtime (rgk_host.cpp) and the kernels (rgk_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.h"
#include "rgk_plan.h" // block sizes, pixel groups, RgkTraceCfg; every grid a launch below takes

#ifndef RGK_SHADE_WAVES
#define RGK_SHADE_WAVES 4 // waves per SIMD the shade kernel is compiled for (128 VGPRs)
#endif
#define RGK_MAX_DEPTH 62
#define RGK_LV_FLOAT4 6 // float4 per stored light vertex: {pos,mat}{lightN,u}{Vr,v}{light_from_source,valid}{diffuse colour}{specular colour}

// device counter block (uint32), zeroed per pass by k_init_counters
#define RGK_CNT_QUEUE 0     // [b]  rays in bounce b's queue        (b = 0..depth)
#define RGK_CNT_SHADOW 64   // [b]  shadow rays issued at bounce b
#define RGK_CNT_FETCH_T 128 // [b]  work-fetch cursor of k_trace_closest at bounce b
#define RGK_CNT_FETCH_S 192 // [b]  work-fetch cursor of k_trace_shadow at bounce b
#define RGK_CNT_GENERIC 256 // [b]  vertices of bounce b left to the generic-BxDF shade launch
#define RGK_CNT_HITS 320    // [k]  light sub-path: rays of bounce k that hit something (k_list_hits)
#define RGK_CNT_SRAYS 384   // [b]  bidirectional rounds: shadow rays traced at bounce b (RGK_CNT_SHADOW counts the vertices queued)
#define RGK_CNT_CONN 448    // [b]  bidirectional rounds: camera vertices of bounce b with connections (k_connect; = entries of the vertex queue)
#define RGK_CNT_FETCH_J 512 // [b]  work-fetch cursor of k_trace_shadow_jobs at bounce b
#define RGK_CNT_TOTAL 576

// what k_trace_shadow does with a visible ray's payload
#define RGK_SHADOW_ADD 0   // tot[slot] += radiance                     (uni-directional path)
#define RGK_SHADOW_SPLAT 2 // atomicAdd(accum_rgb[pixel], radiance)     (BDPT: light-tracing side effect)

#ifndef RGK_ENTRY_K
#define RGK_ENTRY_K 6 // entry nodes per pixel group (unused ones hold the traversal's stack sentinel)
#endif
// One pass = pixels [j0, j0+npix) of the round's pixel list x samples [s0, s0+ns).
// Path slot = ((srel >> g) * npix + j) << g | (srel & (2^g - 1)) with srel = s - s0, j = pixel - j0, g = gshift: 2^g consecutive
// samples of a pixel sit side by side, so a wave of 64 slots is 64 >> g neighbouring pixels x 2^g samples -- rays that differ by
// sub-pixel jitter walk the same nodes and shade the same triangle and texels (g = 0: one sample of 64 pixels, round 1's
// order).  ns is a multiple of 2^g (the host falls back to g = 0 otherwise).
struct PassParams {
    uint32_t j0, npix, s0, ns;
    uint32_t gshift;
    uint32_t beam;            // bounce 0 of a pinhole camera with gshift == 3: one lane walks the tree for the 8 samples of a pixel (k_trace_camera_beam)
    uint32_t multisample, depth, xres, yres;
    float clamp, russian, bumpmap_scale;
    uint32_t reverse;
    const uint32_t* pix_xy;   // x | y << 16, per pixel of the round
    const uint32_t* pix_seed; // PathTracer::samplerSeed for that pixel (a2)
    const float* htab;        // halton_raw(hdim, s) for hdim < 192, s < multisample: htab[hdim * multisample + s]
    float4* light;            // per slot: the path's light {pos.xyz, code}, written by the first vertex of a path that goes on (not on the constant-light route)
    const float4* lbox;       // ... and the box {lo, hi} per group inside which a shadow ray must END to use them
    const int* lentry;        // first-vertex shadow rays of a single-light scene: entry nodes per pixel group (k_entry_points_light), or null
    const float* entry_cap;   // ... and per group the distance up to which that list is complete (+inf: all the way)
    const int* entry;         // camera rays: RGK_ENTRY_K node refs per group of RGK_ENTRY_PIX consecutive pixels of the round's list (k_entry_points), or null
    // bidirectional state (reverse > 0), null otherwise; per slot with stride `batch`
    float4* lstart;           // light_at_path_start.rgb
    float4* lv;               // light vertices: lv[(k*RGK_LV_FLOAT4 + c) * batch + slot], c: see RGK_LV_FLOAT4
    uint32_t* hitlist;        // light sub-path: queue indices of the rays that hit something (k_list_hits)
    uint32_t* lvmask;         // per slot: bit k = light vertex k exists, bit 7 = one of them has a generic-route material
    float4* conn;             // camera vertices with connections: conn[c * batch + i] for queue index i, c < 6 (k_shade<BDPT> -> k_connect)
    uint32_t* connlist;       // ... and the queue indices that have one
    uint32_t batch;
    uint32_t* generic;        // queue indices of the vertices whose material takes the generic BxDF route (k_shade)
};

// slot <-> (pixel of the pass, sample of the pass)
__device__ __forceinline__ void slot_decode(const PassParams& pp, uint32_t slot, uint32_t& j, uint32_t& srel) {
    const uint32_t r = slot >> pp.gshift, sb = r / pp.npix;
    j = r - sb * pp.npix;
    srel = (sb << pp.gshift) | (slot & ((1u << pp.gshift) - 1u));
}
__device__ __forceinline__ uint32_t slot_of(const PassParams& pp, uint32_t j, uint32_t srel) {
    return ((((srel >> pp.gshift) * pp.npix) + j) << pp.gshift) | (srel & ((1u << pp.gshift) - 1u));
}

void rgk_launch_entry_points(hipStream_t st, const DevScene& sc, const DevCamera& cam, uint32_t xres, uint32_t yres, const uint32_t* pix_xy, uint32_t n_pixels,
                             uint32_t g_first, uint32_t g_count, const uint32_t* trange, int* entries, float* cap);
void rgk_launch_group_trange(hipStream_t st, const PassParams& pp, const float4* hit, uint32_t* trange);
void rgk_launch_light_entry_points(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, uint32_t n_pixels_round, const uint32_t* trange, int* entries, float4* lbox);
void rgk_launch_stage_mark(hipStream_t st, uint32_t* host_word, uint32_t v); // progress: the device writes v to pinned host memory
void rgk_launch_init_counters(hipStream_t st, uint32_t* counters, uint32_t n0);
void rgk_launch_build_pixel_list(hipStream_t st, const rgk_tile* tiles, const uint32_t* tile_off, uint32_t n_tiles, uint32_t* pix_xy, uint32_t* pix_seed);
void rgk_launch_build_halton_table(hipStream_t st, const DevScene& sc, uint32_t S, float* htab);
// What a persistent walker consumes: the queue counter it reads its length from, its work-fetch cursor, and the caller's upper
// bound on that length, which sizes the grid (rgk_plan.h rgk_bounded_grid).  The launches that take a plain `bound` size theirs
// the same way.
struct RgkWalk { uint32_t bound; const uint32_t* count_ptr; uint32_t* fetch; };
void rgk_launch_trace_camera(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, const RgkTraceCfg& tc, bool count_stats, float4* hit,
                             const RgkWalk& w, unsigned long long* stats);
void rgk_launch_trace_closest(hipStream_t st, const DevScene& sc, const RgkTraceCfg& tc, bool count_stats, const float4* rayA, const float4* rayB,
                              const float2* nearfar, float4* hit, const RgkWalk& w, unsigned long long* stats);
// first_pp: these are the shadow rays of the pass's first vertices in a single-light scene (entry lists in pp.lentry), else null;
// rec32: the 32-byte records of the constant-light route (below).  The launch picks its kernel from the two.
void rgk_launch_trace_shadow(hipStream_t st, const DevScene& sc, const RgkTraceCfg& tc, bool count_stats, const float4* shA, const float4* shB,
                             const float4* shC, float4* tot, uint8_t* vis_out, int mode, float* splat_rgb, const RgkWalk& w, unsigned long long* stats,
                             const PassParams* first_pp = nullptr, bool rec32 = false);
void rgk_launch_raygen_light(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, float4* rayA, float4* rayB,
                             float4* thr, uint32_t* counters);
void rgk_launch_shade_light(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, uint32_t k, const float4* rayA,
                            const float4* rayB, const float4* hit, float4* thr, float4* nextA, float4* nextB, float4* shA, float4* shB,
                            float4* shC, uint32_t* counters, uint32_t bound);
void rgk_launch_list_hits(hipStream_t st, const float4* hit, const uint32_t* count_ptr, uint32_t* list, uint32_t* list_count, uint32_t bound);
void rgk_launch_connect(hipStream_t st, const DevScene& sc, const PassParams& pp, uint32_t bounce, float4* jobs, float4* rads, uint32_t* counters, uint32_t bound);
void rgk_launch_trace_shadow_jobs(hipStream_t st, const DevScene& sc, const PassParams& pp, const RgkTraceCfg& tc, bool count_stats, const float4* jobs, const float4* rads,
                                  float4* tot, const RgkWalk& w, unsigned long long* stats);
void rgk_launch_shade(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, uint32_t bounce, const float4* rayA,
                      const float4* rayB, const float4* hit, float4* thr, float4* tot, float4* nextA, float4* nextB, float4* shA,
                      float4* shB, float4* shC, uint32_t* counters, uint32_t bound, bool bdpt = false, bool const_light = false,
                      bool last_vertex = false); // last_vertex: at the last bounce of a unidirectional pass (rgk_plan.h rgk_last_bounce) the fast launch is k_last_vertex
// the constant-light route (rgk.h rgk_scene_info::const_light; never with bdpt): rgk_launch_shade(const_light = true) queues shadow
// rays as shA = {d.xyz, far}, shB = {radiance.rgb, slot} when rgk_const_light_records() says so, and rgk_launch_trace_shadow(rec32 =
// true) traces them
bool rgk_const_light_records();
void rgk_launch_resolve(hipStream_t st, const PassParams& pp, const float4* tot, float4* pixsum, float* accum_rgb, uint32_t* accum_count);
void rgk_launch_pack_rays(hipStream_t st, uint32_t n, const float* rays, const int32_t* ignore, float4* rayA, float4* rayB, float2* nearfar);
void rgk_launch_pack_visibility(hipStream_t st, const DevScene& sc, uint32_t n, const float* a, const float* b, float4* shA, float4* shB,
                                float4* shC);
void rgk_launch_unpack_hits(hipStream_t st, uint32_t n, const float4* hit, rgk_hit* out);
void rgk_launch_sampler_eval(hipStream_t st, const DevScene& sc, uint32_t n, const uint32_t* seed, const uint32_t* index,
                             const uint32_t* dim, int is2d, float* out);

void rgk_launch_bxdf_value(hipStream_t st, const DevScene& sc, uint32_t n, uint32_t route, const uint32_t* mat, const float* Vi, const float* Vr, const float* uv, float* out);
void rgk_launch_bxdf_sample(hipStream_t st, const DevScene& sc, uint32_t n, uint32_t route, const uint32_t* mat, const float* Vi, const float* uv, const float* u,
                            float* out_dir, float* out_w, uint8_t* leak);
void rgk_launch_texture_sample(hipStream_t st, const DevScene& sc, uint32_t n, const TexRef* refs, const int32_t* tex, const float* uv, float* rgb, float* sr, float* sb);
void rgk_launch_libm_eval(hipStream_t st, int fn, uint32_t n, const float* a, const float* b, float* out);

// post-processing (rgk_post.hip): the feature pass around rgk_launch_trace_closest, and the a-trous denoiser
void rgk_launch_aov_raygen(hipStream_t st, const DevCamera& cam, uint32_t xres, uint32_t yres, const uint32_t* pix_xy, uint32_t n, float4* rayA, float4* rayB);
void rgk_launch_aov_gather(hipStream_t st, const DevScene& sc, float bumpmap_scale, uint32_t xres, const uint32_t* pix_xy, uint32_t n, const float4* rayA,
                           const float4* rayB, const float4* hit, float* albedo, float* normal, float* depth, int32_t* tri);
// one hop of rgk_render_aov_chain_device: hop `hop`'s queue (rayA / rayB / hit, counters[RGK_CNT_QUEUE + hop] entries, at most n) ->
// the planes, or hop + 1's queue (nextA / nextB, counters[RGK_CNT_QUEUE + hop + 1]); state: per slot {T.rgb, L}; n: the call's pixels
void rgk_launch_aov_hop(hipStream_t st, const DevScene& sc, float bumpmap_scale, uint32_t xres, const uint32_t* pix_xy, uint32_t n, uint32_t hop, uint32_t max_hops,
                        const float4* rayA, const float4* rayB, const float4* hit, float4* state, float4* nextA, float4* nextB, uint32_t* counters, float* albedo,
                        float* normal, float* depth, int32_t* tri, uint8_t* hops);
// ... both denoisers (grids: rgk_plan.h rgk_post_*).  half_rgb == NULL: no half-buffer, the plane's variance is 0.
void rgk_launch_dn_prepare(hipStream_t st, size_t P, const float* accum_rgb, const uint32_t* accum_count, const float* half_rgb, const uint32_t* half_count,
                           const float* albedo, const float* normal, const float* depth, uint32_t demodulate, float albedo_floor, float4* col, float4* guide);
// one a-trous iteration; c: sigma_i^2 / sigma_k^2 / not read.  The variance mean is the variance-guided filter's prefilter, at step 1.
enum RgkDnMode { RGK_DN_FIXED_SIGMA, RGK_DN_VARIANCE_GUIDED, RGK_DN_VARIANCE_MEAN };
void rgk_launch_dn_atrous(hipStream_t st, RgkDnMode mode, uint32_t xres, uint32_t yres, uint32_t step, float c, float sigma_depth, uint32_t npow,
                          const float4* guide, const float4* src, float4* dst);
void rgk_launch_dn_finish(hipStream_t st, size_t P, const float4* col, const float* albedo, uint32_t demodulate, float albedo_floor, float* out_rgb);
// ... and the noise estimate from two half-buffers
void rgk_launch_nz_tile_sums(hipStream_t st, uint32_t xres, uint32_t yres, uint32_t tile_size, const float* accum_rgb, const uint32_t* accum_count,
                             const float* half_rgb, const uint32_t* half_count, rgk_noise_tile* tiles, float* variance);
void rgk_launch_nz_finish(hipStream_t st, size_t P, const float4* col, float* out_variance);
// the round fold: tiles / to_half on the device, n_tiles > 0 checked tiles (rgk_adapt.h rgk_fold_check_tiles gives max_tile_height)
void rgk_launch_round_fold(hipStream_t st, uint32_t xres, const rgk_tile* tiles, const uint8_t* to_half, uint32_t n_tiles, uint32_t max_tile_height,
                           float* round_rgb, uint32_t* round_count, float* total_rgb, uint32_t* total_count, float* half_rgb, uint32_t* half_count);
// temporal reuse: both cameras pinhole copies; n_triangles: a triangle id from there on gets no history (never an index)
void rgk_launch_tp_reproject(hipStream_t st, const DevScene& sc, uint32_t n_triangles, const DevCamera& cam, const DevCamera& prev, uint32_t xres, uint32_t yres,
                             const float* depth, const float* normal, const int32_t* tri, const float* depth_prev, const float* normal_prev, const int32_t* tri_prev,
                             const float* hist_rgb_prev, const float* hist_len_prev, float plane_tol, float normal_cos, float* hist_rgb, float* hist_len);
void rgk_launch_tp_blend(hipStream_t st, size_t P, const float* accum_rgb, const uint32_t* accum_count, const float* albedo, const float* hist_rgb, const float* hist_len,
                         float alpha_min, float max_len, uint32_t demodulate, float albedo_floor, float* out_hist_rgb, float* out_hist_len, float* out_rgb);
// guided upsampling: both cameras pinhole copies; rec: 3 * xl * yl records (prepare writes them, gather reads them); albedo planes may
// be NULL without demodulation, out_support may be NULL
void rgk_launch_us_prepare(hipStream_t st, const DevCamera& low, uint32_t xl, uint32_t yl, const float* accum_rgb, const uint32_t* accum_count, const float* albedo,
                           const float* normal, const float* depth, uint32_t demodulate, float albedo_floor, float4* rec);
void rgk_launch_us_gather(hipStream_t st, const DevCamera& cam, const DevCamera& low, uint32_t xres, uint32_t yres, uint32_t xl, uint32_t yl, const float* albedo,
                          const float* normal, const float* depth, const float* low_rgb, const uint32_t* low_count, const float4* rec, float plane_tol, float normal_cos,
                          uint32_t demodulate, float albedo_floor, float* out_rgb, uint8_t* out_support);
// per-sample demodulated accumulation (rgk_post.hip): the divisor per path slot behind bounce 0's walk (div: 16 B per slot of the pass),
// the second resolve (pixsum2: two float4 per pixel of the round), and out = in * dbar per pixel (div_count NULL: div_rgb is an albedo plane)
void rgk_launch_demod_divisor(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, const float4* hit, float albedo_floor, float4* div);
void rgk_launch_resolve_demod(hipStream_t st, const PassParams& pp, const float4* tot, const float4* div, float4* pixsum2, float* demod_rgb, float* div_rgb);
void rgk_launch_remodulate(hipStream_t st, size_t P, const float* in_rgb, const float* div_rgb, const uint32_t* div_count, float albedo_floor, float* out_rgb);
// display output (rgk_post.hip): the histogram of luminances into hist (RGK_DISPLAY_HIST_WORDS words, cleared by the caller on the stream),
// and the sRGB words; count may be NULL (rgb is a mean); table: the 256 thresholds on the device.  Both pick the four-pixel kernel
// when the planes are 16-byte aligned (rgk_plan.h rgk_display_vec).
void rgk_launch_display_hist(hipStream_t st, size_t P, const float* rgb, const uint32_t* count, uint32_t* hist);
void rgk_launch_display_encode(hipStream_t st, size_t P, const float* rgb, const uint32_t* count, const float* table, uint32_t op, float exposure, float white,
                               uint32_t* out);
// device output path (rgk_pack.hip, arithmetic: rgk_pack.h).  All pointers into the scene's one output byte buffer are 16-byte
// aligned by the caller.
//   out_max: the auto scale 1 / max of rgb / count over the counted pixels into *val, by way of `partial` (RGK_OUT_MAX_WGS floats, every
//            one written by the first launch before the one-workgroup second launch reads it)
//   out_pack_exr: the pixel-data region of the EXR file image (rgk_pack_exr_data_bytes) into out; count NULL: image mode; d_val NULL:
//            scale by `val`, else by *d_val
//   out_pack_png: the IDAT payload (rgk_pack_png_payload_bytes) into out, from one R, G, B, x word per pixel
//   out_png_sums: per piece of RGK_PACK_SEGMENT bytes the Adler pair of the raw stream (2 words each), then the CRCs of the pieces of
//            "IDAT" + payload (1 word each), into sums
constexpr uint32_t RGK_OUT_MAX_WGS = 1024;
void rgk_launch_out_max(hipStream_t st, size_t P, const float* rgb, const uint32_t* count, float* partial, float* val);
void rgk_launch_out_pack_exr(hipStream_t st, uint32_t xres, uint32_t yres, const float* rgb, const uint32_t* count, float val, const float* d_val, uint8_t* out);
void rgk_launch_out_pack_png(hipStream_t st, uint32_t xres, uint32_t yres, const uint32_t* rgba, uint8_t* out);
void rgk_launch_out_png_sums(hipStream_t st, uint32_t xres, uint32_t yres, const uint8_t* payload, uint32_t* sums);
