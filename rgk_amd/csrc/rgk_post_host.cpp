// The post-processing entries: feature buffers, both denoisers, the noise estimate, tile selection, the round fold, temporal reuse and
// guided upsampling and the display output (kernels: rgk_post.hip), and the output files made on the device (kernels: rgk_pack.hip).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "rgk_scene_impl.h"
#include "rgk_adapt.h"
#include "rgk_display.h"
#include "rgk_pack.h"

namespace {
// HIP events (the scene's pool, from its first) around the launches of one post call, when the scene's "time_post" switch is on.
struct PostTimer {
    rgk_scene* s;
    size_t n = 0; // marks so far
    int mark() { // between two launches
        if (!s->tune.time_post) return 0;
        hipEvent_t e;
        if (int rc = scene_event(s, n, e)) return rc;
        n++;
        HIPCHK(hipEventRecord(e, s->stream));
        return 0;
    }
    int fold(std::vector<double>& out) const { // after the stream has been waited for
        out.clear();
        for (size_t i = 0; i + 1 < n; i++) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, s->events[i], s->events[i + 1]));
            out.push_back(ms);
        }
        return 0;
    }
};

// A post call once the entry's own argument checks have passed: refused while a round is in flight; the slot's old times go; with no
// `work` to do that is all, and the device is not touched.  Else body(tm) -- the entry's allocations and its launches on the scene's
// stream, tm.mark() between them -- then a wait for the stream, and the launch times go into the slot.
template <class Body>
int post_call(rgk_scene* s, const char* entry, PostSlot slot, bool work, Body&& body) {
    if (s->prog_busy.load()) return fail(RGK_ERR_INVALID, "%s while a round is in flight on this scene", entry);
    s->post_ms[slot].clear();
    if (!work) return RGK_OK;
    HIPCHK(hipSetDevice(s->device));
    PostTimer tm{s};
    if (int rc = body(tm)) return rc;
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipGetLastError());
    return tm.fold(s->post_ms[slot]);
}

// (every check before the scene or the device is touched; `toff`: tile_offsets)
int check_aov_args(const rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, std::vector<uint32_t>& toff) {
    if (!s || !camera || !prm || (!tiles && n_tiles)) return fail(RGK_ERR_INVALID, "null argument");
    if (int rc = check_frame_size(prm->xres, prm->yres)) return rc;
    return tile_offsets(prm, tiles, n_tiles, "feature pass", toff);
}
// What both denoise entries check besides their own parameter ranges, without touching the scene.  The fixed-sigma filter has no
// half-buffer and no variance plane (NULL here); `p`: its parameters too, with albedo_floor 0 (sigma_k belongs to the entry).
int check_denoise_args(const rgk_scene* s, uint32_t xres, uint32_t yres, const float* accum_rgb, const uint32_t* accum_count, const float* half_rgb,
                       const uint32_t* half_count, const float* albedo, const float* normal, const float* depth, const rgk_denoise_var_params& p,
                       const float* out_rgb, const float* out_variance) {
    if (!s || !accum_rgb || !accum_count || !normal || !depth || !out_rgb) return fail(RGK_ERR_INVALID, "null argument");
    if (p.demodulate && !albedo) return fail(RGK_ERR_INVALID, "demodulate without an albedo plane");
    if (int rc = check_frame_size(xres, yres)) return rc;
    if (p.iterations > 16 || p.normal_power_log2 > 16) return fail(RGK_ERR_INVALID, "iterations and normal_power_log2 must be <= 16");
    const void* ins[] = {accum_rgb, accum_count, half_rgb, half_count, albedo, normal, depth};
    for (const void* in : ins)
        if (in && (in == out_rgb || in == out_variance)) return fail(RGK_ERR_INVALID, "an output plane must not be one of the inputs");
    if (out_rgb == out_variance) return fail(RGK_ERR_INVALID, "out_rgb and out_variance must differ");
    return RGK_OK;
}
// A whole denoise call once the entry's own checks have passed: the shared ones, then prepare -> [prefilter] -> iterations -> finish ->
// [variance copy] on the scene's stream, waited for.  `wc[i]`: iteration i's colour-weight constant (sigma_i^2 / sigma_k^2).
int denoise(rgk_scene* s, const char* entry, PostSlot slot, uint32_t xres, uint32_t yres, const float* accum_rgb, const uint32_t* accum_count, const float* half_rgb,
            const uint32_t* half_count, const float* albedo, const float* normal, const float* depth, const rgk_denoise_var_params& p, const float* wc,
            float* out_rgb, float* out_variance) {
    int rc;
    if ((rc = check_denoise_args(s, xres, yres, accum_rgb, accum_count, half_rgb, half_count, albedo, normal, depth, p, out_rgb, out_variance))) return rc;
    return post_call(s, entry, slot, true, [&](PostTimer& tm) -> int {
        const size_t P = (size_t)xres * yres;
        const uint32_t it = p.iterations, demod = (it && p.demodulate) ? 1u : 0u; // no iteration: out = c, variance = v, nothing to demodulate for
        const RgkDnMode mode = half_rgb ? RGK_DN_VARIANCE_GUIDED : RGK_DN_FIXED_SIGMA;
        if ((rc = s->dn_col[0].alloc(P)) || (it && ((rc = s->dn_col[1].alloc(P)) || (rc = s->dn_guide.alloc(P))))) return rc;
        hipStream_t st = s->stream;
        uint32_t cur = 0; // the plane that holds the current image
        const auto filter = [&](RgkDnMode m, uint32_t step, float c) {
            rgk_launch_dn_atrous(st, m, xres, yres, step, c, p.sigma_depth, p.normal_power_log2, s->dn_guide.p, s->dn_col[cur].p, s->dn_col[cur ^ 1u].p);
            cur ^= 1u;
            return tm.mark();
        };
        if ((rc = tm.mark())) return rc;
        rgk_launch_dn_prepare(st, P, accum_rgb, accum_count, half_rgb, half_count, albedo, normal, depth, demod, p.albedo_floor, s->dn_col[0].p, it ? s->dn_guide.p : nullptr);
        if ((rc = tm.mark())) return rc;
        if (it && mode == RGK_DN_VARIANCE_GUIDED && (rc = filter(RGK_DN_VARIANCE_MEAN, 1u, 0.0f))) return rc;
        for (uint32_t i = 0; i < it; i++)
            if ((rc = filter(mode, 1u << i, wc[i]))) return rc;
        rgk_launch_dn_finish(st, P, s->dn_col[cur].p, albedo, demod, p.albedo_floor, out_rgb);
        if ((rc = tm.mark())) return rc;
        if (!out_variance) return 0;
        rgk_launch_nz_finish(st, P, s->dn_col[cur].p, out_variance);
        return tm.mark();
    });
}

// ---- temporal reuse
// (both entries check every member, whichever of them they read: a parameter set is good or bad, not good for one call)
int check_temporal_params(const rgk_temporal_params* p) {
    if (!p) return fail(RGK_ERR_INVALID, "null argument");
    const float all[5] = {p->plane_tol, p->normal_cos, p->alpha_min, p->max_len, p->albedo_floor};
    for (float v : all)
        if (!std::isfinite(v)) return fail(RGK_ERR_INVALID, "temporal parameters must be finite");
    if (!(p->plane_tol >= 0.0f)) return fail(RGK_ERR_INVALID, "plane_tol must be >= 0");
    if (!(p->normal_cos >= -1.0f && p->normal_cos <= 1.0f)) return fail(RGK_ERR_INVALID, "normal_cos must be in [-1, 1]");
    if (!(p->alpha_min > 0.0f && p->alpha_min <= 1.0f)) return fail(RGK_ERR_INVALID, "alpha_min must be in (0, 1]");
    if (!(p->max_len >= 1.0f)) return fail(RGK_ERR_INVALID, "max_len must be >= 1");
    if (!(p->albedo_floor >= 0.0f)) return fail(RGK_ERR_INVALID, "albedo_floor must be >= 0");
    return RGK_OK;
}
// no output is an input or another output (`ins` may hold NULLs)
int check_outputs_apart(const void* const* ins, size_t n_in, const void* const* outs, size_t n_out) {
    for (size_t o = 0; o < n_out; o++) {
        for (size_t i = 0; i < n_in; i++)
            if (ins[i] && ins[i] == outs[o]) return fail(RGK_ERR_INVALID, "an output plane must not be one of the inputs");
        for (size_t k = o + 1; k < n_out; k++)
            if (outs[k] == outs[o]) return fail(RGK_ERR_INVALID, "the output planes must be different buffers");
    }
    return RGK_OK;
}
// One launch between two marks.  The temporal slot holds {reproject, blend}: `half`'s entry is replaced, the other one kept.
template <class Launch>
int temporal_call(rgk_scene* s, const char* entry, int half, Launch&& launch) {
    std::vector<double> pair = s->post_ms[POST_TEMPORAL];
    const int rc = post_call(s, entry, POST_TEMPORAL, true, [&](PostTimer& tm) -> int {
        if (int rc = tm.mark()) return rc;
        launch(s->stream);
        return tm.mark();
    });
    std::vector<double>& v = s->post_ms[POST_TEMPORAL];
    if (rc || v.empty()) return rc; // ("time_post" is off: nothing recorded)
    pair.resize(2, 0.0);
    pair[half] = v[0];
    v = pair;
    return RGK_OK;
}

// ---- display output
struct DisplayTable {
    float T[RGK_DISPLAY_BINS];
    DisplayTable() { rgk_display_build_table(T); }
};
const float* display_table() {
    static const DisplayTable t; // built once, by the first caller
    return t.T;
}
// (every check before the scene or the device is touched)
int check_display_args(const rgk_scene* s, uint32_t xres, uint32_t yres, const float* d_rgb, const rgk_display_params* p) {
    if (!s || !d_rgb || !p) return fail(RGK_ERR_INVALID, "null argument");
    if (int rc = check_frame_size(xres, yres)) return rc;
    if (const char* why = rgk_display_check_params(p)) return fail(RGK_ERR_INVALID, "display parameters: %s", why);
    return RGK_OK;
}

// ---- output files made on the device
struct PackCrcTable {
    uint32_t t[256];
    PackCrcTable() { rgk_pack_crc_table(t); }
};
const uint32_t* pack_crc_table() {
    static const PackCrcTable t; // built once, by the first caller
    return t.t;
}
// The scene's pinned buffer with room for `bytes`; it only grows.  (The caller has waited for every copy into the old one.)
int pinned_room(rgk_scene* s, size_t bytes) {
    if (s->out_pin && s->out_pin_n >= bytes) return 0;
    if (s->out_pin) (void)hipHostFree(s->out_pin);
    s->out_pin = nullptr; s->out_pin_n = 0;
    hipError_t e = hipHostMalloc((void**)&s->out_pin, bytes);
    if (e != hipSuccess) { s->out_pin = nullptr; return fail(RGK_ERR_OOM, "hipHostMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); }
    s->out_pin_n = bytes;
    return 0;
}
// one fwrite of a finished file image; the host writers' two errors
int write_file(const char* entry, const char* path, const uint8_t* image, size_t bytes) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(RGK_ERR_INVALID, "%s: cannot open the output file", entry);
    const size_t w = std::fwrite(image, 1, bytes, f);
    const int rc = std::fclose(f);
    if (w != bytes || rc != 0) return fail(RGK_ERR_DEVICE, "%s: short write", entry);
    return RGK_OK;
}
} // namespace

extern "C" {

int rgk_render_aov_device(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, float* d_albedo,
                          float* d_normal, float* d_depth, int32_t* d_tri) {
    int rc;
    std::vector<uint32_t> toff; // (read by a queued copy: lives until the stream has been waited for)
    if ((rc = check_aov_args(s, camera, prm, tiles, n_tiles, toff))) return rc;
    const uint32_t n = toff[n_tiles];
    return post_call(s, "rgk_render_aov_device", POST_AOV, n != 0, [&](PostTimer& tm) -> int {
        // The round's own buffers: its pixel list (rebuilt by every round before it is read), two ray planes and the hit plane of
        // the workspace (written by every pass before they are read).  The frame's cached lists -- entry nodes, their caps, the
        // light-side entries -- are neither read nor written here, so the rounds of a frame compute the same with or without this call.
        if ((rc = ensure_workspace(s, n))) return rc;
        hipStream_t st = s->stream;
        DevCamera cam;
        make_camera(camera, cam);
        cam.lens_size = 0.0f; // every feature ray leaves from the camera's origin
        if ((rc = tm.mark()) || (rc = queue_pixel_list(s, tiles, n_tiles, toff))) return rc;
        rgk_launch_init_counters(st, s->counters.p, n);
        rgk_launch_aov_raygen(st, cam, prm->xres, prm->yres, s->pix_xy.p, n, s->rayA[0].p, s->rayB[0].p);
        if ((rc = tm.mark())) return rc;
        rgk_launch_trace_closest(st, s->dev, s->tcfg, false, s->rayA[0].p, s->rayB[0].p, nullptr, s->hit.p, {n, s->counters.p + RGK_CNT_QUEUE, s->counters.p + RGK_CNT_FETCH_T}, s->stats.p);
        if ((rc = tm.mark())) return rc;
        rgk_launch_aov_gather(st, s->dev, prm->bumpmap_scale, prm->xres, s->pix_xy.p, n, s->rayA[0].p, s->rayB[0].p, s->hit.p, d_albedo, d_normal, d_depth, d_tri);
        return tm.mark();
    });
}

int rgk_render_aov(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, float* albedo, float* normal,
                   float* depth, int32_t* tri) {
    int rc;
    std::vector<uint32_t> toff;
    if ((rc = check_aov_args(s, camera, prm, tiles, n_tiles, toff))) return rc;
    HIPCHK(hipSetDevice(s->device));
    const size_t P = (size_t)prm->xres * prm->yres;
    DevBuf<float> d_alb, d_nrm, d_z;
    DevBuf<int32_t> d_tri;
    // (the planes go up first: pixels outside the tiles keep what the caller had there)
    if ((albedo && (rc = d_alb.upload(albedo, 3 * P))) || (normal && (rc = d_nrm.upload(normal, 3 * P))) || (depth && (rc = d_z.upload(depth, P))) || (tri && (rc = d_tri.upload(tri, P))))
        return rc;
    if ((rc = rgk_render_aov_device(s, camera, prm, tiles, n_tiles, albedo ? d_alb.p : nullptr, normal ? d_nrm.p : nullptr, depth ? d_z.p : nullptr, tri ? d_tri.p : nullptr))) return rc;
    if ((albedo && (rc = down(albedo, d_alb, 3 * P))) || (normal && (rc = down(normal, d_nrm, 3 * P))) || (depth && (rc = down(depth, d_z, P))) || (tri && (rc = down(tri, d_tri, P)))) return rc;
    return RGK_OK;
}

int rgk_render_aov_chain_device(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, uint32_t max_hops,
                                float* d_albedo, float* d_normal, float* d_depth, int32_t* d_tri, uint8_t* d_hops) {
    int rc;
    std::vector<uint32_t> toff; // (read by a queued copy: lives until the stream has been waited for)
    if (max_hops > RGK_AOV_MAX_HOPS) return fail(RGK_ERR_INVALID, "max_hops %u: at most %d", max_hops, RGK_AOV_MAX_HOPS);
    if ((rc = check_aov_args(s, camera, prm, tiles, n_tiles, toff))) return rc;
    const uint32_t n = toff[n_tiles];
    return post_call(s, "rgk_render_aov_chain_device", POST_AOV_CHAIN, n != 0, [&](PostTimer& tm) -> int {
        // The buffers of rgk_render_aov_device, with the same argument: the round's pixel list, both pairs of ray planes (hop k reads
        // pair k & 1 and fills the other), the hit plane, and the path-state plane for {T.rgb, L} -- every pass writes a slot's state
        // (its first vertex) before a later vertex reads it.  The counters are the round's: every pass initialises them first.
        // Nothing is read back between the hops: walker and hop kernel of hop k take the queue's length from the device counter.
        if ((rc = ensure_workspace(s, n))) return rc;
        hipStream_t st = s->stream;
        DevCamera cam;
        make_camera(camera, cam);
        cam.lens_size = 0.0f; // every feature ray leaves from the camera's origin
        if ((rc = tm.mark()) || (rc = queue_pixel_list(s, tiles, n_tiles, toff))) return rc;
        rgk_launch_init_counters(st, s->counters.p, n);
        rgk_launch_aov_raygen(st, cam, prm->xres, prm->yres, s->pix_xy.p, n, s->rayA[0].p, s->rayB[0].p);
        if ((rc = tm.mark())) return rc;
        for (uint32_t k = 0; k <= max_hops; k++) {
            const uint32_t cur = k & 1u;
            rgk_launch_trace_closest(st, s->dev, s->tcfg, false, s->rayA[cur].p, s->rayB[cur].p, nullptr, s->hit.p,
                                     {n, s->counters.p + RGK_CNT_QUEUE + k, s->counters.p + RGK_CNT_FETCH_T + k}, s->stats.p);
            if ((rc = tm.mark())) return rc;
            rgk_launch_aov_hop(st, s->dev, prm->bumpmap_scale, prm->xres, s->pix_xy.p, n, k, max_hops, s->rayA[cur].p, s->rayB[cur].p, s->hit.p, s->thr.p,
                               s->rayA[cur ^ 1u].p, s->rayB[cur ^ 1u].p, s->counters.p, d_albedo, d_normal, d_depth, d_tri, d_hops);
            if ((rc = tm.mark())) return rc;
        }
        return 0;
    });
}

int rgk_render_aov_chain(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, uint32_t max_hops, float* albedo,
                         float* normal, float* depth, int32_t* tri, uint8_t* hops) {
    int rc;
    std::vector<uint32_t> toff;
    if (max_hops > RGK_AOV_MAX_HOPS) return fail(RGK_ERR_INVALID, "max_hops %u: at most %d", max_hops, RGK_AOV_MAX_HOPS);
    if ((rc = check_aov_args(s, camera, prm, tiles, n_tiles, toff))) return rc;
    HIPCHK(hipSetDevice(s->device));
    const size_t P = (size_t)prm->xres * prm->yres;
    DevBuf<float> d_alb, d_nrm, d_z;
    DevBuf<int32_t> d_tri;
    DevBuf<uint8_t> d_hops;
    // (the planes go up first: pixels outside the tiles keep what the caller had there)
    if ((albedo && (rc = d_alb.upload(albedo, 3 * P))) || (normal && (rc = d_nrm.upload(normal, 3 * P))) || (depth && (rc = d_z.upload(depth, P))) ||
        (tri && (rc = d_tri.upload(tri, P))) || (hops && (rc = d_hops.upload(hops, P))))
        return rc;
    if ((rc = rgk_render_aov_chain_device(s, camera, prm, tiles, n_tiles, max_hops, albedo ? d_alb.p : nullptr, normal ? d_nrm.p : nullptr, depth ? d_z.p : nullptr,
                                          tri ? d_tri.p : nullptr, hops ? d_hops.p : nullptr)))
        return rc;
    if ((albedo && (rc = down(albedo, d_alb, 3 * P))) || (normal && (rc = down(normal, d_nrm, 3 * P))) || (depth && (rc = down(depth, d_z, P))) ||
        (tri && (rc = down(tri, d_tri, P))) || (hops && (rc = down(hops, d_hops, P))))
        return rc;
    return RGK_OK;
}

int rgk_denoise_device(rgk_scene* s, uint32_t xres, uint32_t yres, const float* d_accum_rgb, const uint32_t* d_accum_count, const float* d_albedo,
                       const float* d_normal, const float* d_depth, const rgk_denoise_params* dp, float* d_out_rgb) {
    if (!dp) return fail(RGK_ERR_INVALID, "null argument");
    if (!(dp->sigma_color > 0.0f) || !(dp->sigma_depth >= 0.0f) || std::isinf(dp->sigma_color) || std::isinf(dp->sigma_depth)) return fail(RGK_ERR_INVALID, "sigma_color must be > 0 and sigma_depth >= 0, both finite");
    float sigma2[16];
    for (uint32_t i = 0; i < dp->iterations && i < 16; i++) { // (iterations <= 16 is checked with what both entries share)
        const float si = dp->sigma_color * std::ldexp(1.0f, -(int)i); // sigma_color * 2^-i
        sigma2[i] = si * si;
        if (!(sigma2[i] > 0.0f) || std::isinf(sigma2[i])) return fail(RGK_ERR_INVALID, "sigma_color^2 leaves the float range at iteration %u", i);
    }
    const rgk_denoise_var_params p = {dp->iterations, 0.0f, dp->sigma_depth, dp->normal_power_log2, dp->demodulate, 0.0f};
    return denoise(s, "rgk_denoise_device", POST_DENOISE, xres, yres, d_accum_rgb, d_accum_count, nullptr, nullptr, d_albedo, d_normal, d_depth, p, sigma2, d_out_rgb, nullptr);
}

int rgk_noise_estimate_device(rgk_scene* s, uint32_t xres, uint32_t yres, uint32_t tile_size, const float* d_accum_rgb, const uint32_t* d_accum_count,
                              const float* d_half_rgb, const uint32_t* d_half_count, rgk_noise_tile* tiles, float* d_variance) {
    // (every check before the scene or the device is touched)
    if (!s || !d_accum_rgb || !d_accum_count || !d_half_rgb || !d_half_count || !tiles) return fail(RGK_ERR_INVALID, "null argument");
    if (int rc = check_frame_size(xres, yres)) return rc;
    if (tile_size == 0) return fail(RGK_ERR_INVALID, "tile_size must be >= 1");
    if (d_variance && (d_variance == d_accum_rgb || d_variance == d_half_rgb || (const void*)d_variance == d_accum_count || (const void*)d_variance == d_half_count))
        return fail(RGK_ERR_INVALID, "variance must not be one of the inputs");
    if (d_half_rgb == d_accum_rgb || d_half_count == d_accum_count) return fail(RGK_ERR_INVALID, "the half-buffer must not be the accumulator");
    const RgkGrid2 g = rgk_nz_tile_grid(xres, yres, tile_size);
    const int rc = post_call(s, "rgk_noise_estimate_device", POST_NOISE, true, [&](PostTimer& tm) -> int {
        int rc;
        if ((rc = s->nz_tiles.alloc(g.count())) || (rc = tm.mark())) return rc;
        rgk_launch_nz_tile_sums(s->stream, xres, yres, tile_size, d_accum_rgb, d_accum_count, d_half_rgb, d_half_count, s->nz_tiles.p, d_variance);
        return tm.mark();
    });
    return rc ? rc : down(tiles, s->nz_tiles, g.count());
}

int rgk_denoise_variance_device(rgk_scene* s, uint32_t xres, uint32_t yres, const float* d_accum_rgb, const uint32_t* d_accum_count, const float* d_half_rgb,
                                const uint32_t* d_half_count, const float* d_albedo, const float* d_normal, const float* d_depth,
                                const rgk_denoise_var_params* dp, float* d_out_rgb, float* d_out_variance) {
    if (!dp || !d_half_rgb || !d_half_count) return fail(RGK_ERR_INVALID, "null argument");
    if (!(dp->sigma_k > 0.0f) || !(dp->sigma_depth >= 0.0f) || !(dp->albedo_floor >= 0.0f) || std::isinf(dp->sigma_k) || std::isinf(dp->sigma_depth) || std::isinf(dp->albedo_floor))
        return fail(RGK_ERR_INVALID, "sigma_k must be > 0, sigma_depth and albedo_floor >= 0, all finite");
    float k2[16];
    std::fill(k2, k2 + 16, dp->sigma_k * dp->sigma_k);
    if (!(k2[0] > 0.0f) || std::isinf(k2[0])) return fail(RGK_ERR_INVALID, "sigma_k^2 leaves the float range");
    if (d_half_rgb == d_accum_rgb || d_half_count == d_accum_count) return fail(RGK_ERR_INVALID, "the half-buffer must not be the accumulator");
    return denoise(s, "rgk_denoise_variance_device", POST_DENOISE_VARIANCE, xres, yres, d_accum_rgb, d_accum_count, d_half_rgb, d_half_count, d_albedo, d_normal, d_depth,
                   *dp, k2, d_out_rgb, d_out_variance);
}

int rgk_adapt_select(const rgk_noise_tile* tiles, const uint32_t* visits, uint32_t xres, uint32_t yres, uint32_t tile_size, const rgk_adapt_params* prm,
                     uint8_t* live, uint32_t* n_live, uint32_t* done) {
    if (const char* why = rgk_adapt_check(tiles, visits, xres, yres, tile_size, prm, live)) return fail(RGK_ERR_INVALID, "rgk_adapt_select: %s", why);
    const RgkAdaptResult r = rgk_adapt_rule(tiles, visits, xres, yres, tile_size, *prm, live);
    if (n_live) *n_live = r.n_live;
    if (done) *done = r.done ? 1u : 0u;
    return RGK_OK;
}

int rgk_round_fold_device(rgk_scene* s, uint32_t xres, uint32_t yres, const rgk_tile* tiles, uint32_t n_tiles, const uint8_t* to_half, float* d_round_rgb,
                          uint32_t* d_round_count, float* d_total_rgb, uint32_t* d_total_count, float* d_half_rgb, uint32_t* d_half_count) {
    // (every check before the scene or the device is touched)
    if (!s || (n_tiles && (!tiles || !to_half)) || !d_round_rgb || !d_round_count || !d_total_rgb || !d_total_count || !d_half_rgb || !d_half_count)
        return fail(RGK_ERR_INVALID, "null argument");
    if (int rc = check_frame_size(xres, yres)) return rc;
    const void* planes[6] = {d_round_rgb, d_round_count, d_total_rgb, d_total_count, d_half_rgb, d_half_count};
    for (int i = 0; i < 6; i++)
        for (int j = i + 1; j < 6; j++)
            if (planes[i] == planes[j]) return fail(RGK_ERR_INVALID, "the six planes must be six different buffers");
    uint32_t max_height = 0, bad = 0;
    if (const char* why = rgk_fold_check_tiles(tiles, n_tiles, xres, yres, max_height, bad)) return fail(RGK_ERR_INVALID, "round fold: %s (tile %u)", why, bad);
    return post_call(s, "rgk_round_fold_device", POST_FOLD, n_tiles != 0, [&](PostTimer& tm) -> int {
        int rc;
        if ((rc = s->fold_buf.alloc((size_t)n_tiles * 5 + (n_tiles + 3u) / 4u)) || (rc = tm.mark())) return rc;
        hipStream_t st = s->stream;
        // (queued copies of the caller's arrays: they are the caller's until this call returns, and it waits for the stream first)
        uint8_t* d_flags = reinterpret_cast<uint8_t*>(s->fold_buf.p + (size_t)n_tiles * 5);
        HIPCHK(hipMemcpyAsync(s->fold_buf.p, tiles, (size_t)n_tiles * sizeof(rgk_tile), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_flags, to_half, n_tiles, hipMemcpyHostToDevice, st));
        if ((rc = tm.mark())) return rc;
        rgk_launch_round_fold(st, xres, reinterpret_cast<const rgk_tile*>(s->fold_buf.p), d_flags, n_tiles, max_height, d_round_rgb, d_round_count, d_total_rgb,
                              d_total_count, d_half_rgb, d_half_count);
        return tm.mark();
    });
}

int rgk_temporal_reproject_device(rgk_scene* s, uint32_t xres, uint32_t yres, const rgk_camera* cam_cur, const rgk_camera* cam_prev, const float* d_depth_cur,
                                  const float* d_normal_cur, const int32_t* d_tri_cur, const float* d_depth_prev, const float* d_normal_prev,
                                  const int32_t* d_tri_prev, const float* d_hist_rgb_prev, const float* d_hist_len_prev, const rgk_temporal_params* tp,
                                  float* d_hist_rgb, float* d_hist_len) {
    // (every check before the scene or the device is touched)
    const void* ins[8] = {d_depth_cur, d_normal_cur, d_tri_cur, d_depth_prev, d_normal_prev, d_tri_prev, d_hist_rgb_prev, d_hist_len_prev};
    const void* outs[2] = {d_hist_rgb, d_hist_len};
    if (!s || !cam_cur || !cam_prev || !d_hist_rgb || !d_hist_len) return fail(RGK_ERR_INVALID, "null argument");
    for (const void* in : ins)
        if (!in) return fail(RGK_ERR_INVALID, "null argument");
    int rc;
    if ((rc = check_temporal_params(tp)) || (rc = check_frame_size(xres, yres)) || (rc = check_outputs_apart(ins, 8, outs, 2))) return rc;
    DevCamera cur, prev;
    make_camera(cam_cur, cur);
    make_camera(cam_prev, prev);
    cur.lens_size = prev.lens_size = 0.0f; // the feature planes' rays: from the cameras' origins
    const rgk_temporal_params p = *tp;
    return temporal_call(s, "rgk_temporal_reproject_device", 0, [&](hipStream_t st) {
        rgk_launch_tp_reproject(st, s->dev, s->n_triangles, cur, prev, xres, yres, d_depth_cur, d_normal_cur, d_tri_cur, d_depth_prev, d_normal_prev, d_tri_prev,
                                d_hist_rgb_prev, d_hist_len_prev, p.plane_tol, p.normal_cos, d_hist_rgb, d_hist_len);
    });
}

int rgk_temporal_blend_device(rgk_scene* s, uint32_t xres, uint32_t yres, const float* d_accum_rgb, const uint32_t* d_accum_count, const float* d_albedo,
                              const float* d_hist_rgb, const float* d_hist_len, const rgk_temporal_params* tp, float* d_out_hist_rgb, float* d_out_hist_len,
                              float* d_out_rgb) {
    // (every check before the scene or the device is touched)
    if (!s || !d_accum_rgb || !d_accum_count || !d_hist_rgb || !d_hist_len || !d_out_hist_rgb || !d_out_hist_len || !d_out_rgb)
        return fail(RGK_ERR_INVALID, "null argument");
    int rc;
    if ((rc = check_temporal_params(tp))) return rc;
    if (tp->demodulate && !d_albedo) return fail(RGK_ERR_INVALID, "demodulate without an albedo plane");
    const void* ins[5] = {d_accum_rgb, d_accum_count, d_albedo, d_hist_rgb, d_hist_len};
    const void* outs[3] = {d_out_hist_rgb, d_out_hist_len, d_out_rgb};
    if ((rc = check_frame_size(xres, yres)) || (rc = check_outputs_apart(ins, 5, outs, 3))) return rc;
    const rgk_temporal_params p = *tp;
    return temporal_call(s, "rgk_temporal_blend_device", 1, [&](hipStream_t st) {
        rgk_launch_tp_blend(st, (size_t)xres * yres, d_accum_rgb, d_accum_count, d_albedo, d_hist_rgb, d_hist_len, p.alpha_min, p.max_len, p.demodulate ? 1u : 0u,
                            p.albedo_floor, d_out_hist_rgb, d_out_hist_len, d_out_rgb);
    });
}

int rgk_upsample_device(rgk_scene* s, uint32_t xres, uint32_t yres, const rgk_camera* cam, const float* d_albedo, const float* d_normal, const float* d_depth,
                        uint32_t xl, uint32_t yl, const rgk_camera* cam_low, const float* d_low_accum_rgb, const uint32_t* d_low_accum_count, const float* d_low_albedo,
                        const float* d_low_normal, const float* d_low_depth, const rgk_upsample_params* up, float* d_out_rgb, uint8_t* d_out_support) {
    // (every check before the scene or the device is touched)
    if (!s || !cam || !cam_low || !d_normal || !d_depth || !d_low_accum_rgb || !d_low_accum_count || !d_low_normal || !d_low_depth || !up || !d_out_rgb)
        return fail(RGK_ERR_INVALID, "null argument");
    const float all[3] = {up->plane_tol, up->normal_cos, up->albedo_floor};
    for (float v : all)
        if (!std::isfinite(v)) return fail(RGK_ERR_INVALID, "upsample parameters must be finite");
    if (!(up->plane_tol >= 0.0f)) return fail(RGK_ERR_INVALID, "plane_tol must be >= 0");
    if (!(up->normal_cos >= -1.0f && up->normal_cos <= 1.0f)) return fail(RGK_ERR_INVALID, "normal_cos must be in [-1, 1]");
    if (!(up->albedo_floor >= 0.0f)) return fail(RGK_ERR_INVALID, "albedo_floor must be >= 0");
    if (up->demodulate && (!d_albedo || !d_low_albedo)) return fail(RGK_ERR_INVALID, "demodulate without both albedo planes");
    int rc;
    if ((rc = check_frame_size(xres, yres)) || (rc = check_frame_size(xl, yl))) return rc;
    if (cam->xsize != (int32_t)xres || cam->ysize != (int32_t)yres || cam_low->xsize != (int32_t)xl || cam_low->ysize != (int32_t)yl)
        return fail(RGK_ERR_INVALID, "a camera's xsize / ysize is not its grid's resolution");
    const void* ins[8] = {d_albedo, d_normal, d_depth, d_low_accum_rgb, d_low_accum_count, d_low_albedo, d_low_normal, d_low_depth};
    const void* outs[2] = {d_out_rgb, d_out_support};
    if ((rc = check_outputs_apart(ins, 8, outs, d_out_support ? 2 : 1))) return rc;
    DevCamera full, low;
    make_camera(cam, full);
    make_camera(cam_low, low);
    full.lens_size = low.lens_size = 0.0f; // the feature planes' rays: from the cameras' origins
    const rgk_upsample_params p = *up;
    const uint32_t demod = p.demodulate ? 1u : 0u;
    return post_call(s, "rgk_upsample_device", POST_UPSAMPLE, true, [&](PostTimer& tm) -> int {
        // The record planes are the entry's own (the library's allocation path: RGK_POISON covers them); nothing a round reads or writes.
        if ((rc = s->us_rec.alloc(3 * (size_t)xl * yl)) || (rc = tm.mark())) return rc;
        rgk_launch_us_prepare(s->stream, low, xl, yl, d_low_accum_rgb, d_low_accum_count, d_low_albedo, d_low_normal, d_low_depth, demod, p.albedo_floor, s->us_rec.p);
        if ((rc = tm.mark())) return rc;
        rgk_launch_us_gather(s->stream, full, low, xres, yres, xl, yl, d_albedo, d_normal, d_depth, d_low_accum_rgb, d_low_accum_count, s->us_rec.p, p.plane_tol,
                             p.normal_cos, demod, p.albedo_floor, d_out_rgb, d_out_support);
        return tm.mark();
    });
}

int rgk_remodulate_device(rgk_scene* s, uint32_t xres, uint32_t yres, const float* d_in_rgb, const float* d_div_rgb, const uint32_t* d_div_count, float albedo_floor,
                          float* d_out_rgb) {
    // (every check before the scene or the device is touched)
    if (!s || !d_in_rgb || !d_div_rgb || !d_out_rgb) return fail(RGK_ERR_INVALID, "null argument");
    if (!(albedo_floor >= 0.0f) || std::isinf(albedo_floor)) return fail(RGK_ERR_INVALID, "albedo_floor must be >= 0 and finite");
    int rc;
    const void* ins[3] = {d_in_rgb, d_div_rgb, d_div_count};
    const void* outs[1] = {d_out_rgb};
    if ((rc = check_frame_size(xres, yres)) || (rc = check_outputs_apart(ins, 3, outs, 1))) return rc;
    return post_call(s, "rgk_remodulate_device", POST_REMODULATE, true, [&](PostTimer& tm) -> int {
        if ((rc = tm.mark())) return rc;
        rgk_launch_remodulate(s->stream, (size_t)xres * yres, d_in_rgb, d_div_rgb, d_div_count, albedo_floor, d_out_rgb);
        return tm.mark();
    });
}

const float* rgk_display_table(void) { return display_table(); }

int rgk_display_solve(const uint32_t* hist, uint32_t n_dark, const rgk_display_params* params, rgk_display_stats* stats) {
    if (!hist || !stats) return fail(RGK_ERR_INVALID, "null argument");
    if (const char* why = rgk_display_check_params(params)) return fail(RGK_ERR_INVALID, "display parameters: %s", why);
    if (!rgk_display_solve_hist(hist, n_dark, *params, *stats)) return fail(RGK_ERR_INVALID, "the histogram's counts do not fit 32 bits");
    return RGK_OK;
}

int rgk_display_measure_device(rgk_scene* s, uint32_t xres, uint32_t yres, const float* d_rgb, const uint32_t* d_count, const rgk_display_params* params,
                               rgk_display_stats* stats) {
    int rc;
    if (!stats) return fail(RGK_ERR_INVALID, "null argument");
    if ((rc = check_display_args(s, xres, yres, d_rgb, params))) return rc;
    const rgk_display_params p = *params;
    rc = post_call(s, "rgk_display_measure_device", POST_DISPLAY_MEASURE, true, [&](PostTimer& tm) -> int {
        // The histogram is the entry's own buffer (the library's allocation path: RGK_POISON covers it) and is cleared here, on the
        // stream, before the launch that adds to it; nothing a round reads or writes.
        int rc;
        if ((rc = s->disp_hist.alloc(RGK_DISPLAY_HIST_WORDS)) || (rc = tm.mark())) return rc;
        HIPCHK(hipMemsetAsync(s->disp_hist.p, 0, RGK_DISPLAY_HIST_WORDS * sizeof(uint32_t), s->stream));
        if ((rc = tm.mark())) return rc;
        rgk_launch_display_hist(s->stream, (size_t)xres * yres, d_rgb, d_count, s->disp_hist.p);
        return tm.mark();
    });
    uint32_t h[RGK_DISPLAY_HIST_WORDS];
    if (rc || (rc = down(h, s->disp_hist, RGK_DISPLAY_HIST_WORDS))) return rc;
    if (!rgk_display_solve_hist(h, h[RGK_DISPLAY_BINS], p, *stats)) return fail(RGK_ERR_DEVICE, "the histogram's counts do not fit 32 bits"); // (P < 2^32: not reached)
    return RGK_OK;
}

int rgk_display_encode_device(rgk_scene* s, uint32_t xres, uint32_t yres, const float* d_rgb, const uint32_t* d_count, const rgk_display_params* params,
                              const rgk_display_stats* stats, uint32_t* d_out_rgba) {
    int rc;
    if (!stats || !d_out_rgba) return fail(RGK_ERR_INVALID, "null argument");
    if ((rc = check_display_args(s, xres, yres, d_rgb, params))) return rc;
    if (const char* why = rgk_display_check_scale(stats->exposure, stats->white)) return fail(RGK_ERR_INVALID, "display stats: %s", why);
    const void* ins[2] = {d_rgb, d_count};
    const void* outs[1] = {d_out_rgba};
    if ((rc = check_outputs_apart(ins, 2, outs, 1))) return rc;
    const uint32_t op = params->op;
    const float exposure = stats->exposure, white = stats->white;
    return post_call(s, "rgk_display_encode_device", POST_DISPLAY_ENCODE, true, [&](PostTimer& tm) -> int {
        int rc;
        if (!s->disp_table.p && (rc = s->disp_table.upload(display_table(), RGK_DISPLAY_BINS))) return rc; // (a blocking copy: done before the launch is queued)
        if ((rc = tm.mark())) return rc;
        rgk_launch_display_encode(s->stream, (size_t)xres * yres, d_rgb, d_count, s->disp_table.p, op, exposure, white, d_out_rgba);
        return tm.mark();
    });
}

// ---- output files made on the device (kernels: rgk_pack.hip; arithmetic and file layout: rgk_pack.h)
// Both entries: the pack kernels fill the scene's output byte buffer, ONE copy brings the file's device-made region -- and, behind
// it, the scale word or the checksum pieces -- into the scene's pinned buffer, where the host has written or then writes the bytes
// around it; one fwrite.  The buffers are the entries' own: nothing a round reads or writes.

int rgk_output_write_exr_device(rgk_scene* s, const char* path, uint32_t xres, uint32_t yres, const float* d_rgb, const uint32_t* d_count, float output_scale,
                                float* scale_used) {
    if (!s || !path || !d_rgb) return fail(RGK_ERR_INVALID, "rgk_output_write_exr_device: null argument");
    if (int rc = check_frame_size(xres, yres)) return rc;
    if (!d_count && !(std::isfinite(output_scale) && output_scale > 0.0f))
        return fail(RGK_ERR_INVALID, "rgk_output_write_exr_device: without a count plane output_scale must be > 0 and finite");
    const bool automatic = d_count && output_scale <= 0.0f; // (the host's `val <= 0`: a NaN scale is applied as it is, there and here)
    const size_t head = rgk_pack_exr_data_at(yres), data = rgk_pack_exr_data_bytes(xres, yres);
    const size_t val_at = data, partial_at = (data + 4 + 15) & ~(size_t)15; // in the device buffer; data is a multiple of 8
    const size_t copy = automatic ? data + 4 : data;
    const size_t pad = (64 - head % 64) % 64; // the pinned image starts here, so that the copy lands on a 64-byte boundary
    int rc = post_call(s, "rgk_output_write_exr_device", POST_OUTPUT_EXR, true, [&](PostTimer& tm) -> int {
        int rc;
        if ((rc = s->out_dev.alloc(partial_at + RGK_OUT_MAX_WGS * sizeof(float))) || (rc = pinned_room(s, pad + head + data + 4))) return rc;
        uint8_t* const d = s->out_dev.p;
        float* const d_val = (float*)(d + val_at);
        if ((rc = tm.mark())) return rc;
        if (automatic) {
            rgk_launch_out_max(s->stream, (size_t)xres * yres, d_rgb, d_count, (float*)(d + partial_at), d_val);
            if ((rc = tm.mark())) return rc;
        }
        rgk_launch_out_pack_exr(s->stream, xres, yres, d_rgb, d_count, output_scale, automatic ? d_val : nullptr, d);
        if ((rc = tm.mark())) return rc;
        HIPCHK(hipMemcpyAsync(s->out_pin + pad + head, d, copy, hipMemcpyDeviceToHost, s->stream));
        rgk_pack_exr_head(s->out_pin + pad, xres, yres); // (host bytes in front of the region the copy fills)
        return 0;
    });
    if (rc) return rc;
    std::vector<double>& ms = s->post_ms[POST_OUTPUT_EXR];
    if (!automatic && !ms.empty()) ms.insert(ms.begin(), 0.0); // {k_out_max or 0, pack}
    float val = output_scale;
    if (automatic) std::memcpy(&val, s->out_pin + pad + head + data, 4);
    if (scale_used) *scale_used = val;
    return write_file("rgk_output_write_exr_device", path, s->out_pin + pad, head + data);
}

int rgk_output_write_png_device(rgk_scene* s, const char* path, uint32_t xres, uint32_t yres, const uint32_t* d_rgba) {
    if (!s || !path || !d_rgba) return fail(RGK_ERR_INVALID, "rgk_output_write_png_device: null argument");
    if (int rc = check_frame_size(xres, yres)) return rc;
    if (!rgk_pack_png_fits(xres, yres)) return fail(RGK_ERR_INVALID, "rgk_output_write_png_device: the image does not fit one IDAT chunk");
    const uint32_t raw = (uint32_t)rgk_pack_png_raw_bytes(xres, yres), payload = (uint32_t)rgk_pack_png_payload_bytes(raw);
    const uint32_t n_adler = rgk_pack_pieces(raw, RGK_PACK_SEGMENT), n_crc = rgk_pack_pieces((uint64_t)payload + 4u, RGK_PACK_SEGMENT);
    const size_t sums_at = ((size_t)payload + 3) & ~(size_t)3, n_sums = (size_t)2 * n_adler + n_crc; // the kernel writes zeros up to sums_at
    const size_t copy = sums_at + 4 * n_sums;
    const size_t pad = (64 - RGK_PACK_PNG_LEAD % 64) % 64;
    int rc = post_call(s, "rgk_output_write_png_device", POST_OUTPUT_PNG, true, [&](PostTimer& tm) -> int {
        int rc;
        if ((rc = s->out_dev.alloc(copy)) || (rc = pinned_room(s, pad + RGK_PACK_PNG_LEAD + copy + RGK_PACK_PNG_TAIL))) return rc;
        uint8_t* const d = s->out_dev.p;
        if ((rc = tm.mark())) return rc;
        rgk_launch_out_pack_png(s->stream, xres, yres, d_rgba, d);
        if ((rc = tm.mark())) return rc;
        rgk_launch_out_png_sums(s->stream, xres, yres, d, (uint32_t*)(d + sums_at));
        if ((rc = tm.mark())) return rc;
        HIPCHK(hipMemcpyAsync(s->out_pin + pad + RGK_PACK_PNG_LEAD, d, copy, hipMemcpyDeviceToHost, s->stream));
        rgk_pack_png_lead(s->out_pin + pad, pack_crc_table(), xres, yres, payload);
        return 0;
    });
    if (rc) return rc;
    uint8_t* const image = s->out_pin + pad;
    std::vector<uint32_t> sums(n_sums); // (out of the way of the tail, which is written where they arrived)
    std::memcpy(sums.data(), image + RGK_PACK_PNG_LEAD + sums_at, 4 * n_sums);
    RgkPackAdler adler;
    for (uint32_t k = 0; k < n_adler; k++) {
        const uint32_t left = raw - k * RGK_PACK_SEGMENT;
        adler.add(sums[2 * k], sums[2 * k + 1], left < RGK_PACK_SEGMENT ? left : RGK_PACK_SEGMENT);
    }
    const uint32_t crc = rgk_pack_crc_fold(sums.data() + 2 * (size_t)n_adler, (uint64_t)payload + 4u, RGK_PACK_SEGMENT);
    rgk_pack_png_tail(image + RGK_PACK_PNG_LEAD + payload, pack_crc_table(), adler.value(), crc);
    return write_file("rgk_output_write_png_device", path, image, RGK_PACK_PNG_LEAD + (size_t)payload + RGK_PACK_PNG_TAIL);
}

int rgk_scene_get_post_timing(const rgk_scene* s, uint32_t which, double* ms, uint32_t* n) {
    if (!s || !n || which >= POST_SLOTS || (!ms && *n)) return fail(RGK_ERR_INVALID, "bad argument");
    if (s->magic != RGK_SCENE_MAGIC) return fail(RGK_ERR_INVALID, "not a live scene handle");
    const std::vector<double>& v = s->post_ms[which];
    for (uint32_t i = 0; i < *n && i < v.size(); i++) ms[i] = v[i];
    *n = (uint32_t)v.size();
    return RGK_OK;
}

} // extern "C"
