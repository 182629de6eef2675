// The unit-level entries the parity tests call: traversal, visibility, BxDFs, textures, libm and the sampler, one kernel each.
#include <cstring>

#include "rgk_scene_impl.h"

namespace {
// One probe call on a scene: every host array of `ins` goes up, `launch(in, out)` runs on the scene's stream and is waited for,
// every array of `outs` comes down.  n == 0: nothing to do; else no array may be null, and `check()` (the indices) runs before
// the device is touched.  `what`: the kernel, for the error text.
struct ProbeIn { const void* host; size_t bytes; };
struct ProbeOut { void* host; size_t bytes; };
using ProbeDev = DevBuf<unsigned char>;
template <class T> T* as(ProbeDev& b) { return reinterpret_cast<T*>(b.p); }
template <size_t NI, size_t NO, class Check, class Launch>
int probe_call(rgk_scene* s, uint32_t n, const char* what, const ProbeIn (&ins)[NI], const ProbeOut (&outs)[NO], Check&& check, Launch&& launch) {
    if (!s) return fail(RGK_ERR_INVALID, "null argument");
    if (n == 0) return RGK_OK;
    for (const ProbeIn& a : ins) if (!a.host) return fail(RGK_ERR_INVALID, "null argument");
    for (const ProbeOut& a : outs) if (!a.host) return fail(RGK_ERR_INVALID, "null argument");
    int rc;
    if ((rc = check())) return rc;
    HIPCHK(hipSetDevice(s->device));
    ProbeDev in[NI], out[NO];
    for (size_t i = 0; i < NI; i++) if ((rc = in[i].upload((const unsigned char*)ins[i].host, ins[i].bytes))) return rc;
    for (size_t i = 0; i < NO; i++) if ((rc = out[i].alloc(outs[i].bytes))) return rc;
    launch(in, out);
    if (hipStreamSynchronize(s->stream) != hipSuccess) return fail(RGK_ERR_DEVICE, "%s kernel failed", what);
    for (size_t i = 0; i < NO; i++) if ((rc = down((unsigned char*)outs[i].host, out[i], outs[i].bytes))) return rc;
    return RGK_OK;
}
template <class T>
int check_below(const T* v, uint32_t n, T limit, const char* what) {
    for (uint32_t i = 0; i < n; i++) if (v[i] >= limit) return fail(RGK_ERR_INVALID, "%s index out of range", what);
    return 0;
}
// The entries that take no scene need a device all the same.
int need_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RGK_ERR_NO_DEVICE, "no HIP device visible");
    return 0;
}
} // namespace

extern "C" {

int rgk_trace_closest(rgk_scene* s, uint32_t n, const float* rays, const int32_t* ignore, rgk_hit* hits, rgk_counters* counters) {
    if (!s || (!rays && n) || (!hits && n)) return fail(RGK_ERR_INVALID, "null argument");
    if (counters) std::memset(counters, 0, sizeof(*counters));
    if (n == 0) return RGK_OK;
    HIPCHK(hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_workspace(s, n)) || (rc = s->nearfar.alloc(n)) || (rc = s->scratch_f.alloc((size_t)8 * n)) || (rc = s->scratch_u.alloc((size_t)5 * n)))
        return rc;
    hipStream_t st = s->stream;
    HIPCHK(hipMemcpyAsync(s->scratch_f.p, rays, (size_t)8 * n * sizeof(float), hipMemcpyHostToDevice, st));
    int32_t* d_ign = nullptr;
    if (ignore) {
        d_ign = (int32_t*)s->scratch_u.p;
        HIPCHK(hipMemcpyAsync(d_ign, ignore, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemsetAsync(s->stats.p, 0, 8 * sizeof(unsigned long long), st));
    rgk_launch_init_counters(st, s->counters.p, n);
    rgk_launch_pack_rays(st, n, s->scratch_f.p, d_ign, s->rayA[0].p, s->rayB[0].p, s->nearfar.p);
    const RgkWalk w = {n, s->counters.p + RGK_CNT_QUEUE, s->counters.p + RGK_CNT_FETCH_T};
    hipEvent_t e0 = nullptr, e1 = nullptr; // kernel time of the traversal alone, for counters->ms_trace
    if (counters) {
        if ((rc = scene_event(s, 0, e0)) || (rc = scene_event(s, 1, e1))) return rc;
        HIPCHK(hipEventRecord(e0, st));
    }
    rgk_launch_trace_closest(st, s->dev, s->tcfg, false, s->rayA[0].p, s->rayB[0].p, s->nearfar.p, s->hit.p, w, s->stats.p);
    if (counters) {
        HIPCHK(hipEventRecord(e1, st));
        // the counting variant runs separately so that the timed launch is the kernel a round runs
        rgk_launch_init_counters(st, s->counters.p, n);
        rgk_launch_trace_closest(st, s->dev, s->tcfg, true, s->rayA[0].p, s->rayB[0].p, s->nearfar.p, s->hit.p, w, s->stats.p);
    }
    rgk_hit* d_hits = (rgk_hit*)s->scratch_u.p; // 5 dwords per hit; reuses the ignore buffer after the trace
    rgk_launch_unpack_hits(st, n, s->hit.p, d_hits);
    HIPCHK(hipMemcpyAsync(hits, d_hits, (size_t)n * sizeof(rgk_hit), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (counters) {
        unsigned long long h[8];
        if ((rc = read_stats(s, h))) return rc;
        counters->node_visits = h[0]; counters->tri_tests = h[1]; counters->path_rays = n;
        if (s->tune.debug_util) // lane occupancy per phase of the walker: lane-visits / (64 x wave iterations)
            std::fprintf(stderr, "[rgk util] rays %u  node visits %llu in %llu wave iterations (%.3f of lanes)  triangle tests %llu in %llu (%.3f)  outer iterations %llu  refills %llu\n",
                         n, h[0], h[4], h[4] ? (double)h[0] / (64.0 * (double)h[4]) : 0.0, h[1], h[5], h[5] ? (double)h[1] / (64.0 * (double)h[5]) : 0.0, h[6], h[7]);
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        counters->ms_trace = ms; counters->n_trace_launches = 1;
    }
    return RGK_OK;
}

int rgk_trace_visibility(rgk_scene* s, uint32_t n, const float* a, const float* b, uint8_t* visible, rgk_counters* counters) {
    if (!s || (n && (!a || !b || !visible))) return fail(RGK_ERR_INVALID, "null argument");
    if (counters) std::memset(counters, 0, sizeof(*counters));
    if (n == 0) return RGK_OK;
    HIPCHK(hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_workspace(s, n)) || (rc = s->scratch_f.alloc((size_t)6 * n)) || (rc = s->scratch_u.alloc(n))) return rc;
    hipStream_t st = s->stream;
    HIPCHK(hipMemcpyAsync(s->scratch_f.p, a, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->scratch_f.p + (size_t)3 * n, b, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(s->stats.p, 0, 8 * sizeof(unsigned long long), st));
    rgk_launch_init_counters(st, s->counters.p, n);
    rgk_launch_pack_visibility(st, s->dev, n, s->scratch_f.p, s->scratch_f.p + (size_t)3 * n, s->shA.p, s->shB.p, s->shC.p);
    rgk_launch_trace_shadow(st, s->dev, s->tcfg, counters != nullptr, s->shA.p, s->shB.p, s->shC.p, s->tot.p, (uint8_t*)s->scratch_u.p,
                            RGK_SHADOW_ADD, nullptr, {n, s->counters.p + RGK_CNT_QUEUE, s->counters.p + RGK_CNT_FETCH_S}, s->stats.p);
    HIPCHK(hipMemcpyAsync(visible, s->scratch_u.p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (counters) {
        unsigned long long h[8];
        if ((rc = read_stats(s, h))) return rc;
        counters->shadow_node_visits = h[2]; counters->shadow_tri_tests = h[3]; counters->shadow_rays = n;
    }
    return RGK_OK;
}

int rgk_bxdf_value(rgk_scene* s, uint32_t n, uint32_t route, const uint32_t* mat, const float* Vi, const float* Vr, const float* uv, float* out_rgb) {
    const size_t f = (size_t)n * sizeof(float);
    return probe_call(s, n, "bxdf value", {{mat, (size_t)n * sizeof(uint32_t)}, {Vi, 3 * f}, {Vr, 3 * f}, {uv, 2 * f}}, {{out_rgb, 3 * f}},
                      [&] { return check_below(mat, n, s->n_materials, "material"); },
                      [&](ProbeDev* in, ProbeDev* out) { rgk_launch_bxdf_value(s->stream, s->dev, n, route, as<uint32_t>(in[0]), as<float>(in[1]), as<float>(in[2]), as<float>(in[3]), as<float>(out[0])); });
}

int rgk_bxdf_sample(rgk_scene* s, uint32_t n, uint32_t route, const uint32_t* mat, const float* Vi, const float* uv, const float* u, float* out_dir,
                    float* out_weight, uint8_t* may_leak) {
    const size_t f = (size_t)n * sizeof(float);
    return probe_call(s, n, "bxdf sample", {{mat, (size_t)n * sizeof(uint32_t)}, {Vi, 3 * f}, {uv, 2 * f}, {u, 2 * f}}, {{out_dir, 3 * f}, {out_weight, 3 * f}, {may_leak, n}},
                      [&] { return check_below(mat, n, s->n_materials, "material"); },
                      [&](ProbeDev* in, ProbeDev* out) {
                          rgk_launch_bxdf_sample(s->stream, s->dev, n, route, as<uint32_t>(in[0]), as<float>(in[1]), as<float>(in[2]), as<float>(in[3]), as<float>(out[0]), as<float>(out[1]), as<uint8_t>(out[2]));
                      });
}

int rgk_texture_sample(rgk_scene* s, uint32_t n, const int32_t* tex, const float* uv, float* rgb, float* slope_right, float* slope_bottom) {
    const size_t f = (size_t)n * sizeof(float);
    return probe_call(s, n, "texture sample", {{tex, (size_t)n * sizeof(int32_t)}, {uv, 2 * f}}, {{rgb, 3 * f}, {slope_right, f}, {slope_bottom, f}},
                      [&] { return check_below(tex, n, (int32_t)s->n_textures, "texture"); },
                      [&](ProbeDev* in, ProbeDev* out) { rgk_launch_texture_sample(s->stream, s->dev, n, s->texrefs.p, as<int32_t>(in[0]), as<float>(in[1]), as<float>(out[0]), as<float>(out[1]), as<float>(out[2])); });
}

int rgk_libm_eval(int fn, uint32_t n, const float* a, const float* b, float* out) {
    if (n && (!a || !out || (fn == 4 && !b))) return fail(RGK_ERR_INVALID, "null argument");
    if (fn < 0 || fn > 4) return fail(RGK_ERR_INVALID, "unknown function");
    if (n == 0) return RGK_OK;
    DevBuf<float> da, db, dout;
    int rc;
    if ((rc = need_device()) || (rc = da.upload(a, n)) || (rc = db.upload(b ? b : a, n)) || (rc = dout.alloc(n))) return rc;
    rgk_launch_libm_eval(nullptr, fn, n, da.p, db.p, dout.p);
    return down(out, dout, n);
}

int rgk_sampler_eval(uint32_t n, const uint32_t* seed, const uint32_t* index, const uint32_t* dim, int is2d, float* out) {
    if (n && (!seed || !index || !dim || !out)) return fail(RGK_ERR_INVALID, "null argument");
    if (n == 0) return RGK_OK;
    if (int rc = need_device()) return rc;
    std::vector<DevHaltonDim> hd;
    std::vector<uint16_t> hp;
    build_halton(hd, hp);
    DevBuf<DevHaltonDim> dh;
    DevBuf<uint16_t> dp;
    DevBuf<uint32_t> ds_, di, dd;
    DevBuf<float> dout;
    int rc;
    if ((rc = dh.upload(hd.data(), hd.size())) || (rc = dp.upload(hp.data(), hp.size())) || (rc = ds_.upload(seed, n)) || (rc = di.upload(index, n)) ||
        (rc = dd.upload(dim, n)) || (rc = dout.alloc((size_t)2 * n)))
        return rc;
    DevScene sc{};
    sc.hdims = dh.p; sc.hperm = dp.p;
    rgk_launch_sampler_eval(nullptr, sc, n, ds_.p, di.p, dd.p, is2d, dout.p);
    hipError_t e = hipMemcpy(out, dout.p, (size_t)2 * n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RGK_ERR_DEVICE, "sampler eval: %s", hipGetErrorString(e));
    return RGK_OK;
}

} // extern "C"
