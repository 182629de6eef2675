// The round driver: tiles -> per-pixel seeds (a2) -> passes of paths resident in HBM -> raygen / trace / shade / shadow / resolve
// launches on one HIP stream.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rgk_scene_impl.h"

#ifndef RGK_SAMPLE_GROUP_DEFAULT
#define RGK_SAMPLE_GROUP_DEFAULT 3 // 8 samples of a pixel side by side: swept 0..6 on the Sponza proxy (154.2, -, 149.6, 148.4, 148.1, 150.3, 150.0 ms per round)
#endif

// what rgk_round_plan.h restates of rgk_kernels.h
static_assert(RGK_RP_CNT_QUEUE == RGK_CNT_QUEUE && RGK_RP_CNT_SHADOW == RGK_CNT_SHADOW && RGK_RP_CNT_HITS == RGK_CNT_HITS && RGK_RP_CNT_SRAYS == RGK_CNT_SRAYS &&
                  RGK_RP_CNT_CONN == RGK_CNT_CONN && RGK_RP_CNT_TOTAL == RGK_CNT_TOTAL && RGK_RP_LV_FLOAT4 == RGK_LV_FLOAT4,
              "rgk_round_plan.h and rgk_kernels.h disagree");

int queue_pixel_list(rgk_scene* s, const rgk_tile* tiles, uint32_t n_tiles, const std::vector<uint32_t>& toff) {
    const size_t P = toff[n_tiles];
    hipStream_t st = s->stream;
    int rc;
    if ((rc = s->pix_xy.alloc(P)) || (rc = s->pix_seed.alloc(P)) || (rc = s->tile_buf.alloc((size_t)n_tiles * 5 + n_tiles + 1))) return rc;
    HIPCHK(hipMemcpyAsync(s->tile_buf.p, tiles, (size_t)n_tiles * sizeof(rgk_tile), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->tile_buf.p + (size_t)n_tiles * 5, toff.data(), (n_tiles + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    rgk_launch_build_pixel_list(st, reinterpret_cast<const rgk_tile*>(s->tile_buf.p), s->tile_buf.p + (size_t)n_tiles * 5, n_tiles, s->pix_xy.p, s->pix_seed.p);
    return 0;
}

namespace {
// Paths resident per pass.  The path state is sized for the machine, not for a cache: by default
// 96 GB of the 288 GB HBM3E (measured on Sponza 1080p x 256 spp: 2^25 paths/pass 2235 Mpaths/s, 2^27 2398,
// 2^28 2440 -- fewer, longer launches and shorter tails; 48 -> 96 GB: +1.4 % there, +6 % on the bidirectional
// configuration whose paths carry 3.5x the state).  RGK_WORKSPACE_GB / RGK_BATCH_PATHS override.
size_t batch_paths(const RgkTuning& tune, uint32_t reverse) {
    if (tune.batch_paths) return tune.batch_paths;
    const size_t per_path = rgk_workspace_bytes_per_path(reverse); // the planes ensure_workspace allocates
    const bool g = tune.workspace_gb > 0;
    double gb = g ? tune.workspace_gb : (reverse ? 160.0 : 96.0); // bidirectional paths carry 3.5x the state: 765 -> 781 Mpaths/s
    if (!g) { // a shared or smaller card: never plan for more than 60 % of what is free right now
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) gb = std::min(gb, 0.6 * (double)free_b / 1e9);
    }
    size_t b = (size_t)(gb * 1e9 / (double)per_path);
    return std::min<size_t>(std::max<size_t>(b, 1024), (size_t)1 << 30);
}

// ------------------------------------------------------------------ the round driver
// rgk_render_round_device: the round's pixel list (prepare_round_lists), a plan of passes the workspace holds (plan_passes), and
// per pass -- pixels [j0, j0 + npix) of the list x samples [s0, s0 + ns) -- its launches queued on the scene's stream
// (queue_pass), a wait, and its queue counters added to the round's totals (rgk_round_plan.h rgk_add_pass_counters).

// Per-kernel records of a round (rgk_counters::kernel and the four class sums).  RGK_FLAG_TIME_KERNELS: a pair of events around
// every launch.  RGK_FLAG_COUNT_TRAVERSAL: the traversal counters (stats[0..3]: closest nodes / triangles, shadow nodes /
// triangles) are read back after every traversal launch, so that each kernel gets its own share (stream-ordered copies; nobody
// times a counting round).  The pass code names the kernel class of each launch: run(class, launch).
struct KernelLog {
    rgk_scene* s;
    bool timing, count_stats;
    struct Ev { int cls; hipEvent_t a, b; };
    std::vector<Ev> evs;
    size_t ev_used = 0; // events of the scene's pool taken by this round
    std::vector<RgkStatSnap> snaps;

    KernelLog(rgk_scene* s_, uint32_t flags)
        : s(s_), timing((flags & RGK_FLAG_TIME_KERNELS) != 0), count_stats((flags & RGK_FLAG_COUNT_TRAVERSAL) != 0) {
        if (count_stats) snaps.reserve(4096);
    }
    int event(hipEvent_t& e) { return scene_event(s, ev_used++, e); }
    template <class Launch>
    int run(int cls, Launch&& launch) {
        Ev ev{cls, nullptr, nullptr};
        if (timing) {
            int rc;
            if ((rc = event(ev.a)) || (rc = event(ev.b))) return rc;
            HIPCHK(hipEventRecord(ev.a, s->stream));
        }
        launch();
        if (timing) {
            HIPCHK(hipEventRecord(ev.b, s->stream));
            evs.push_back(ev);
        }
        if (count_stats && rgk_kernel_traverses(cls)) {
            snaps.push_back(RgkStatSnap{cls, {}});
            HIPCHK(hipMemcpyAsync(snaps.back().v, s->stats.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
            HIPCHK(hipStreamSynchronize(s->stream));
        }
        return 0;
    }
    int fold(rgk_counters& c) const {
        std::vector<RgkLaunchTime> times(evs.size());
        for (size_t i = 0; i < evs.size(); i++) {
            times[i] = {evs[i].cls, 0.f};
            HIPCHK(hipEventElapsedTime(&times[i].ms, evs[i].a, evs[i].b));
        }
        rgk_fold_kernel_log(times.data(), times.size(), snaps.data(), snaps.size(), c);
        return 0;
    }
};

// Deep path loops (depth > 12): the length of the next queue is read back every other bounce from the fourth on; it bounds the
// grids of the following launches (queues only shrink) and ends the loop once no path is left.  The copy lands in pinned memory;
// polling it costs microseconds where hipStreamSynchronize was measured at 2-3 ms per call (blocking wait), more than the
// launches it saves.
int queue_len(rgk_scene* s, const uint32_t* dptr, uint32_t& out) {
    volatile uint32_t* h = s->h_counters;
    h[0] = 0xffffffffu; // never a queue length (queues hold < 2^30 entries)
    HIPCHK(hipMemcpyAsync(s->h_counters, dptr, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    for (uint64_t spins = 0; h[0] == 0xffffffffu; spins++) {
        if ((spins & 0xfffff) != 0xfffff) continue;
        // every ~1 M polls ask the stream: not-ready means keep polling, success means the copy has landed (re-read), anything
        // else is a sticky launch / device error that would otherwise spin here for ever
        const hipError_t q = hipStreamQuery(s->stream);
        if (q == hipErrorNotReady) continue;
        if (q != hipSuccess) return fail(RGK_ERR_DEVICE, "queue-length read-back: %s", hipGetErrorString(q));
        if (h[0] == 0xffffffffu) HIPCHK(hipStreamSynchronize(s->stream));
        if (h[0] == 0xffffffffu) return fail(RGK_ERR_DEVICE, "queue-length read-back never landed");
        break;
    }
    out = h[0];
    return 0;
}

// The round's pixel list and the camera rays' entry nodes per pixel group.  P: the round's pixels (0: nothing queued).  `toff`:
// see queue_pixel_list.
int prepare_round_lists(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles,
                        std::vector<uint32_t>& toff, size_t& P) {
    int rc;
    if ((rc = tile_offsets(prm, tiles, n_tiles, "round", toff))) return rc;
    P = toff[n_tiles];
    if (P == 0) return 0;
    if ((rc = queue_pixel_list(s, tiles, n_tiles, toff))) return rc;
    if (!s->tune.entry_points) { // (off: every camera ray starts at the root)
        s->entry.release(); s->entry_cap.release();
        return 0;
    }
    // the entry nodes depend on the camera and on which pixels the list holds in which order -- not on the seeds: a frame's
    // rounds share them (0.7 ms per round at 1080p otherwise)
    const uint64_t key = rgk_frame_list_key(*camera, prm->xres, prm->yres, tiles, n_tiles);
    const size_t n_entry = ((size_t)P + RGK_ENTRY_PIX - 1) / RGK_ENTRY_PIX * RGK_ENTRY_K;
    if (s->entry.p && s->entry_n == n_entry && s->entry_key == key) return 0;
    if ((rc = s->entry.alloc(n_entry)) || (rc = s->entry_cap.alloc(n_entry / RGK_ENTRY_K + 1)) || (rc = s->trange.alloc((n_entry / RGK_ENTRY_K + 1) * 2))) return rc;
    DevCamera cam0;
    make_camera(camera, cam0);
    rgk_launch_entry_points(s->stream, s->dev, cam0, prm->xres, prm->yres, s->pix_xy.p, (uint32_t)P, 0u, (uint32_t)(n_entry / RGK_ENTRY_K), nullptr, s->entry.p, s->entry_cap.p);
    s->entry_key = key; s->entry_n = n_entry;
    s->entry_capped = 0; s->lentry_done = 0; // a new frame: capped / light-side lists are rebuilt as its first passes finish
    return 0;
}

// The pass plan: pixel ranges of npix_pass pixels x equal-sized sample passes of ns_pass samples, and the workspace for them.
// Paths per pass: what the card has room for now (an existing workspace counts as room); halved on an allocation failure.
int plan_passes(rgk_scene* s, const rgk_params* prm, size_t P, uint32_t R, RgkPassPlan& plan) {
    size_t B = batch_paths(s->tune, R);
    if (!s->tune.batch_paths && s->batch_reverse >= R) B = std::max(B, s->batch); // (an explicit batch size is taken literally)
    int rc;
    for (;;) {
        plan = rgk_plan_passes(P, prm->multisample, B);
        rc = ensure_workspace(s, plan.npix_pass * plan.ns_pass, R);
        if (rc != RGK_ERR_OOM || B <= ((size_t)1 << 20)) break;
        (void)hipGetLastError();
        B /= 2;
    }
    if (rc) return rc;
    return s->pixsum.alloc(P);
}

// Behind bounce 0's trace, once per frame and pixel range (later rounds and sample ranges reuse them): how far the first hits of
// each pixel group lie -> the camera rays' entry lists capped behind them, and where the group's shadow rays can go (light-side
// entry nodes and their boxes, which pp points to from here on).
int queue_first_hit_lists(rgk_scene* s, KernelLog& kl, const DevCamera& cam, PassParams& pp, uint32_t P, bool cap_entries, bool light_entry) {
    hipStream_t st = s->stream;
    const size_t end = (size_t)pp.j0 + pp.npix;
    const RgkGroupRange groups = rgk_group_range(pp.j0, pp.npix);
    const bool need_cap = cap_entries && end > s->entry_capped;
    const bool need_light = light_entry && end > s->lentry_done;
    int rc;
    if ((need_cap || need_light) && (rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_group_trange(st, pp, s->hit.p, s->trange.p); }))) return rc;
    if (need_cap) {
        if ((rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_entry_points(st, s->dev, cam, pp.xres, pp.yres, s->pix_xy.p, P, groups.first, groups.count(), s->trange.p, s->entry.p, s->entry_cap.p); })))
            return rc;
        s->entry_capped = end;
    }
    if (!light_entry) return 0;
    pp.lentry = s->lentry.p; pp.lbox = s->lbox.p;
    if (!need_light) return 0;
    if ((rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_light_entry_points(st, s->dev, cam, pp, P, s->trange.p, s->lentry.p, s->lbox.p); }))) return rc;
    s->lentry_done = end;
    if (s->tune.debug_bvh) { // how many pixel groups got light-side entry nodes below the root
        const size_t g0 = groups.first, g1 = groups.last;
        std::vector<int> he((g1 - g0) * RGK_ENTRY_K);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(he.data(), s->lentry.p + g0 * RGK_ENTRY_K, he.size() * sizeof(int), hipMemcpyDeviceToHost));
        size_t below = 0, total_e = 0;
        for (size_t g = 0; g < g1 - g0; g++) { if (he[g * RGK_ENTRY_K] != 0) below++; for (int k = 0; k < RGK_ENTRY_K; k++) total_e += he[g * RGK_ENTRY_K + k] != 0x7fffffff; }
        std::fprintf(stderr, "[rgk] light-side entry nodes: %zu of %zu pixel groups start below the root, %.2f entries per group\n", below, g1 - g0, (double)total_e / (double)(g1 - g0));
    }
    return 0;
}

// What a demodulated round has beside the accumulator (rgk.h rgk_render_round_demod_device).
// `timed` (the scene's "time_post" switch): event pairs around the two extra launches of every pass, {divisor, resolve} alternating.
struct DemodPlanes {
    float* demod_rgb; float* div_rgb; float albedo_floor;
    bool timed = false;
    std::vector<hipEvent_t> evs = {};
};

// One pass, queued on the scene's stream: the light sub-path (reverse > 0), the camera path's bounces, the resolve into the
// accumulator, a progress mark behind every bounce (`stage`: the round's stages before this pass), and the copy of the pass's
// counter blocks into h_counters.
// `dm` (a demodulated round, else null): behind bounce 0's walk the divisor of every slot, behind the resolve the second one.  Neither
// launch goes through the kernel log: the counters of a demodulated round are the plain round's.
int queue_pass(rgk_scene* s, KernelLog& kl, const DevCamera& cam, PassParams& pp, size_t P, bool light_entry, bool const_light, float* d_accum_rgb,
               uint32_t* d_accum_count, uint32_t stage, DemodPlanes* dm) {
    hipStream_t st = s->stream;
    const RgkTraceCfg& tc = s->tcfg;
    const bool count_stats = kl.count_stats, cap_entries = s->entry.p != nullptr && s->tune.entry_cap;
    const bool track = pp.depth > 12; // queue lengths read back (queue_len): measured, depth 10 loses 4 % to the read-backs, depth 40 gains 4 %
    const uint32_t R = pp.reverse, n0 = pp.npix * pp.ns;
    // the slot order, and the bundle walk for passes whose entry lists are not capped yet -- a frame's first round (rgk_plan.h)
    pp.gshift = rgk_plan_gshift(s->tune.sample_group, RGK_SAMPLE_GROUP_DEFAULT, pp.ns);
    pp.beam = rgk_beam_wanted(s->tune.beam, cap_entries && (size_t)pp.j0 + pp.npix <= s->entry_capped) ? 1u : 0u;
    float4* const rayA[2] = {s->rayA[0].p, s->rayA[1].p};
    float4* const rayB[2] = {s->rayB[0].p, s->rayB[1].p};
    float4 *const hit = s->hit.p, *const thr = s->thr.p, *const tot = s->tot.p, *const shA = s->shA.p, *const shB = s->shB.p, *const shC = s->shC.p;
    uint32_t* const cn = s->counters.p;      // camera-phase counters
    uint32_t* const cl = cn + RGK_CNT_TOTAL; // light-phase counters
    int rc;
    const auto demod_launch = [&](auto&& launch) -> int { // outside the kernel log; between two events of the scene's pool when timed
        hipEvent_t a = nullptr, b = nullptr;
        if (dm->timed) {
            if ((rc = kl.event(a)) || (rc = kl.event(b))) return rc;
            HIPCHK(hipEventRecord(a, st));
        }
        launch();
        if (dm->timed) {
            HIPCHK(hipEventRecord(b, st));
            dm->evs.push_back(a); dm->evs.push_back(b);
        }
        return 0;
    };
    if (R > 0) {
        // light sub-path first (its sampler dimensions are fixed), splats straight into the accumulator
        if ((rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_init_counters(st, cl, 0u); })) || // (k_raygen_light queues the light rays that can touch the scene's box)
            (rc = kl.run(RGK_K_LIGHT_SHADE, [&] { rgk_launch_raygen_light(st, s->dev, cam, pp, rayA[0], rayB[0], thr, cl); })))
            return rc;
        for (uint32_t k = 0; k < R; k++) {
            const int q = k & 1;
            if ((rc = kl.run(RGK_K_LIGHT_TRACE, [&] { rgk_launch_trace_closest(st, s->dev, tc, count_stats, rayA[q], rayB[q], nullptr, hit, {n0, cl + RGK_CNT_QUEUE + k, cl + RGK_CNT_FETCH_T + k}, s->stats.p); })) ||
                (rc = kl.run(RGK_K_LIGHT_SHADE, [&] { rgk_launch_list_hits(st, hit, cl + RGK_CNT_QUEUE + k, s->hitlist.p, cl + RGK_CNT_HITS + k, n0); })) ||
                (rc = kl.run(RGK_K_LIGHT_SHADE, [&] { rgk_launch_shade_light(st, s->dev, cam, pp, k, rayA[q], rayB[q], hit, thr, rayA[q ^ 1], rayB[q ^ 1], shA, shB, shC, cl, n0); })) ||
                (rc = kl.run(RGK_K_LIGHT_SPLAT, [&] { rgk_launch_trace_shadow(st, s->dev, tc, count_stats, shA, shB, shC, nullptr, nullptr, RGK_SHADOW_SPLAT, d_accum_rgb,
                                                                              {n0, cl + RGK_CNT_SHADOW + k, cl + RGK_CNT_FETCH_S + k}, s->stats.p); })))
                return rc;
        }
    }
    // the camera path: the same pipeline for uni- and bidirectional rounds (R > 0: vertices with connections take the record
    // route -- k_shade<BDPT> -> k_connect -> k_trace_shadow_jobs -- beside the plain NEE rays)
    if ((rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_init_counters(st, cn, n0); }))) return rc;
    uint32_t ub = n0; // upper bound on bounce b's queues: every launch of the bounce sizes its grid by it
    for (uint32_t b = 0; b < pp.depth && ub > 0; b++) {
        const int q = b & 1;
        const RgkWalk wq = {ub, cn + RGK_CNT_QUEUE + b, cn + RGK_CNT_FETCH_T + b}, ws = {ub, cn + RGK_CNT_SHADOW + b, cn + RGK_CNT_FETCH_S + b};
        if (b == 0) // no ray queue at bounce 0: the camera ray of slot i is made where it is traced and shaded
            rc = kl.run(RGK_K_TRACE_CAMERA, [&] { rgk_launch_trace_camera(st, s->dev, cam, pp, tc, count_stats, hit, wq, s->stats.p); });
        else
            rc = kl.run(RGK_K_TRACE_CLOSEST, [&] { rgk_launch_trace_closest(st, s->dev, tc, count_stats, rayA[q], rayB[q], nullptr, hit, wq, s->stats.p); });
        if (rc || (b == 0 && (rc = queue_first_hit_lists(s, kl, cam, pp, (uint32_t)P, cap_entries, light_entry)))) return rc;
        if (dm && b == 0 && (rc = demod_launch([&] { rgk_launch_demod_divisor(st, s->dev, cam, pp, hit, dm->albedo_floor, s->demod_div.p); }))) return rc;
        if ((rc = kl.run(b == 0 ? RGK_K_SHADE_FIRST : RGK_K_SHADE, [&] { rgk_launch_shade(st, s->dev, cam, pp, b, rayA[q], rayB[q], hit, thr, tot, rayA[q ^ 1], rayB[q ^ 1], shA, shB, shC, cn, ub, R > 0, const_light, s->tune.last_vertex); })) ||
            (R > 0 && (rc = kl.run(RGK_K_CONNECT, [&] { rgk_launch_connect(st, s->dev, pp, b, s->jobs.p, s->rads.p, cn, ub); }))))
            return rc;
        // (the constant-light route: the shading launches above left 32-byte records, shA = {d, far}, shB = {radiance, slot})
        const bool first = b == 0 && light_entry, rec32 = const_light && rgk_const_light_records();
        rc = kl.run(first ? RGK_K_SHADOW_FIRST : RGK_K_SHADOW, [&] { rgk_launch_trace_shadow(st, s->dev, tc, count_stats, shA, shB, shC, tot, nullptr, RGK_SHADOW_ADD, nullptr, ws, s->stats.p, first ? &pp : nullptr, rec32); });
        // (the vertex queue after the plain rays: both add into the slot sums, a slot has a vertex in ONE of the two queues)
        if (rc || (R > 0 && (rc = kl.run(RGK_K_SHADOW_JOBS, [&] { rgk_launch_trace_shadow_jobs(st, s->dev, pp, tc, count_stats, s->jobs.p, s->rads.p, tot, {ub, cn + RGK_CNT_CONN + b, cn + RGK_CNT_FETCH_J + b}, s->stats.p); }))))
            return rc;
        rgk_launch_stage_mark(st, s->h_stage, stage + b + 1);
        if (track && b >= 3 && (b & 1) && b + 1 < pp.depth && (rc = queue_len(s, cn + RGK_CNT_QUEUE + b + 1, ub))) return rc;
    }
    if ((rc = kl.run(RGK_K_RESOLVE, [&] { rgk_launch_resolve(st, pp, tot, s->pixsum.p, d_accum_rgb, d_accum_count); }))) return rc;
    if (dm && (rc = demod_launch([&] { rgk_launch_resolve_demod(st, pp, tot, s->demod_div.p, s->demod_pixsum.p, dm->demod_rgb, dm->div_rgb); }))) return rc;
    rgk_launch_stage_mark(st, s->h_stage, stage + std::max(1u, pp.depth)); // (all of the pass's stages: bounces that never ran count too)
    HIPCHK(hipMemcpyAsync(s->h_counters, cn, 2 * RGK_CNT_TOTAL * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return 0;
}

// The body of both round entries.  dm == null: rgk_render_round_device, as it was before the demodulated round existed.
int render_round(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, float* d_accum_rgb, uint32_t* d_accum_count,
                 rgk_counters* counters, DemodPlanes* dm) {
    if (!s || !camera || !prm || (!tiles && n_tiles) || !d_accum_rgb || !d_accum_count) return fail(RGK_ERR_INVALID, "null argument");
    if (int rc = check_frame_size(prm->xres, prm->yres)) return rc;
    if (prm->multisample == 0) return fail(RGK_ERR_INVALID, "multisample must be >= 1");
    if (prm->depth > RGK_MAX_DEPTH) return fail(RGK_ERR_UNSUPPORTED, "recursion depth %u > %d", prm->depth, RGK_MAX_DEPTH);
    if (prm->reverse > 7) return fail(RGK_ERR_UNSUPPORTED, "reverse %u > 7 light sub-path vertices", prm->reverse);
    if (prm->sampler != RGK_SAMPLER_HALTON) return fail(RGK_ERR_UNSUPPORTED, "the HIP path implements the Halton sampler only");
    HIPCHK(hipSetDevice(s->device));
    if (counters) std::memset(counters, 0, sizeof(*counters));
    std::vector<uint32_t> toff; // (read by a queued copy: it lives to the end of this call, which synchronises the stream before returning)
    size_t P = 0;
    RgkPassPlan plan{};
    int rc;
    if ((rc = prepare_round_lists(s, camera, prm, tiles, n_tiles, toff, P))) return rc;
    if (P == 0) return RGK_OK;
    // no light at all: TracePath builds no light sub-path (`reverse > 0 && valid light`), same as reverse == 0
    const uint32_t R = (s->dev.total_point_power + s->dev.total_areal_power > 0.0f) ? prm->reverse : 0u;
    if ((rc = plan_passes(s, prm, P, R, plan))) return rc;
    if (dm && ((rc = s->demod_div.alloc(s->batch)) || (rc = s->demod_pixsum.alloc(2 * P)))) return rc;

    DevCamera cam;
    make_camera(camera, cam);
    HIPCHK(hipMemsetAsync(s->stats.p, 0, 8 * sizeof(unsigned long long), s->stream));
    KernelLog kl(s, prm->flags);
    // progress: one stage per bounce per pass; a one-thread kernel queued behind each bounce writes the stage number into pinned
    // host memory when the DEVICE gets there (a host function in the stream did the same but stalls the stream for a host
    // round trip per mark)
    const uint32_t pass_stages = std::max(1u, prm->depth);
    {
        const uint32_t n_pix_passes = (uint32_t)((P + plan.npix_pass - 1) / plan.npix_pass), n_s_passes = (prm->multisample + plan.ns_pass - 1) / plan.ns_pass;
        *(volatile uint32_t*)s->h_stage = 0; s->prog_stages = n_pix_passes * n_s_passes * pass_stages;
        s->prog_pixels = P; s->prog_paths = (uint64_t)P * prm->multisample; s->prog_busy = 1;
    }
    struct Done { rgk_scene* s; ~Done() { *(volatile uint32_t*)s->h_stage = s->prog_stages.load(); s->prog_busy = 0; } } done_guard{s};
    PassParams pp{};
    pp.multisample = prm->multisample; pp.depth = prm->depth; pp.xres = prm->xres; pp.yres = prm->yres;
    pp.clamp = prm->clamp; pp.russian = prm->russian; pp.bumpmap_scale = prm->bumpmap_scale; pp.reverse = R;
    pp.lstart = s->lstart.p; pp.lv = s->lv.p; pp.hitlist = s->hitlist.p; pp.lvmask = s->lvmask.p; pp.conn = s->conn.p; pp.connlist = s->connlist.p;
    pp.batch = (uint32_t)s->batch;
    pp.pix_xy = s->pix_xy.p; pp.pix_seed = s->pix_seed.p; pp.light = s->light.p; pp.generic = s->generic.p;
    pp.entry = s->entry.p; // (null when switched off; only the unidirectional bounce-0 launch reads it)
    pp.entry_cap = s->entry_cap.p;
    // one point / sphere light and nothing else that emits: every first-vertex shadow ray starts there (k_entry_points_light)
    const bool light_entry = s->entry.p && s->tune.light_entry && s->dev.n_pointlights == 1 && s->dev.n_areal == 0;
    // ... and if that light is provably every path's light, at its own position, a unidirectional round takes it as a constant
    const bool const_light = s->info.const_light == 1 && s->tune.const_light && R == 0;
    if (light_entry) {
        const size_t groups = ((size_t)P + RGK_ENTRY_PIX - 1) / RGK_ENTRY_PIX + 1;
        if ((rc = s->lentry.alloc(groups * RGK_ENTRY_K)) || (rc = s->trange.alloc(groups * 2)) || (rc = s->lbox.alloc(groups * 2))) return rc;
    }
    if ((rc = s->htab.alloc((size_t)192 * prm->multisample))) return rc;
    if ((rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_build_halton_table(s->stream, s->dev, prm->multisample, s->htab.p); }))) return rc;
    pp.htab = s->htab.p;

    rgk_counters tot{};
    uint32_t stage = 0; // progress stages of the passes before this one
    for (size_t j0 = 0; j0 < P; j0 += plan.npix_pass) {
        pp.j0 = (uint32_t)j0;
        pp.npix = (uint32_t)std::min(plan.npix_pass, P - j0);
        for (uint32_t s0 = 0; s0 < prm->multisample; s0 += plan.ns_pass, stage += pass_stages) {
            pp.s0 = s0;
            pp.ns = std::min(plan.ns_pass, prm->multisample - s0);
            if ((rc = queue_pass(s, kl, cam, pp, P, light_entry, const_light, d_accum_rgb, d_accum_count, stage, dm))) return rc;
            HIPCHK(hipStreamSynchronize(s->stream));
            rgk_add_pass_counters(s->h_counters, s->h_counters + RGK_CNT_TOTAL, pp.depth, pp.reverse, pp.npix * pp.ns, light_entry, tot);
        }
    }
    HIPCHK(hipGetLastError());
    s->prog_rounds++;
    if (dm) { // rgk_scene_get_post_timing(9): {the round's k_demod_divisor launches, its k_resolve_demod launches}, summed over the passes
        std::vector<double>& ms = s->post_ms[POST_DEMOD_ROUND];
        ms.clear();
        if (dm->timed) ms.assign(2, 0.0);
        for (size_t i = 0; i + 1 < dm->evs.size(); i += 2) {
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, dm->evs[i], dm->evs[i + 1]));
            ms[(i / 2) & 1] += t;
        }
    }
    if (counters) {
        tot.paths = (uint64_t)P * prm->multisample;
        if (kl.count_stats) {
            unsigned long long h[8];
            if ((rc = read_stats(s, h))) return rc;
            tot.node_visits = h[0]; tot.tri_tests = h[1]; tot.shadow_node_visits = h[2]; tot.shadow_tri_tests = h[3];
        }
        if ((rc = kl.fold(tot))) return rc;
        *counters = tot;
    }
    return RGK_OK;
}
} // namespace

extern "C" {

int rgk_render_round_device(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles,
                            float* d_accum_rgb, uint32_t* d_accum_count, rgk_counters* counters) {
    return render_round(s, camera, prm, tiles, n_tiles, d_accum_rgb, d_accum_count, counters, nullptr);
}

int rgk_render_round_demod_device(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, float* d_accum_rgb,
                                  uint32_t* d_accum_count, float* d_demod_rgb, float* d_div_rgb, float albedo_floor, rgk_counters* counters) {
    // (its own checks first, like the shared ones before the scene or the device is touched)
    if (!d_demod_rgb || !d_div_rgb) return fail(RGK_ERR_INVALID, "null argument");
    if (!(albedo_floor >= 0.0f) || std::isinf(albedo_floor)) return fail(RGK_ERR_INVALID, "albedo_floor must be >= 0 and finite");
    if (d_demod_rgb == d_div_rgb || d_demod_rgb == d_accum_rgb || d_div_rgb == d_accum_rgb || (const void*)d_demod_rgb == d_accum_count || (const void*)d_div_rgb == d_accum_count)
        return fail(RGK_ERR_INVALID, "the four planes must be four different buffers");
    if (prm && prm->reverse > 0) return fail(RGK_ERR_UNSUPPORTED, "a demodulated round cannot be bidirectional (reverse %u): a light-tracing splat has no path slot", prm->reverse);
    if (prm && prm->depth == 0) return fail(RGK_ERR_UNSUPPORTED, "a demodulated round needs depth >= 1: without a bounce there is no first hit");
    DemodPlanes dm = {d_demod_rgb, d_div_rgb, albedo_floor};
    if (s && s->magic == RGK_SCENE_MAGIC) {
        dm.timed = s->tune.time_post;
        if (!s->prog_busy.load()) s->post_ms[POST_DEMOD_ROUND].clear(); // (a round that ends early, with no pixel, leaves no earlier round's times)
    }
    return render_round(s, camera, prm, tiles, n_tiles, d_accum_rgb, d_accum_count, counters, &dm);
}

int rgk_render_round(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles,
                     float* accum_rgb, uint32_t* accum_count, rgk_counters* counters) {
    if (!s || !prm || !accum_rgb || !accum_count) return fail(RGK_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(s->device));
    const size_t P = (size_t)prm->xres * prm->yres;
    DevBuf<float> d_rgb;
    DevBuf<uint32_t> d_cnt;
    int rc;
    if ((rc = d_rgb.upload(accum_rgb, 3 * P)) || (rc = d_cnt.upload(accum_count, P))) return rc;
    if ((rc = rgk_render_round_device(s, camera, prm, tiles, n_tiles, d_rgb.p, d_cnt.p, counters))) return rc;
    if ((rc = down(accum_rgb, d_rgb, 3 * P)) || (rc = down(accum_count, d_cnt, P))) return rc;
    return RGK_OK;
}

} // extern "C"
