// The kernels behind the unit-level entries of the parity tests (rgk_probe.cpp).  No round launches them.
#pragma once
#include <hip/hip_runtime.h>
#include "rgk_device.h"
#include "rgk_kernels.h"
#include "rgk_shade.h" // the queue records

// rays given as 8 floats {o, d, near, far} (rgk_trace_closest API) -> the ray queue's records
__global__ void k_pack_rays(uint32_t n, const float* __restrict__ rays, const int32_t* __restrict__ ignore, float4* rayA, float4* rayB, float2* nearfar) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float* r = rays + 8 * (size_t)i;
        const f3 o = mk3(r[0], r[1], r[2]), d = mk3(r[3], r[4], r[5]);
        rayA[i] = ray_rec_a(o, d);
        rayB[i] = ray_rec_b(d, __int_as_float(ignore ? ignore[i] : -1), i);
        nearfar[i] = make_float2(r[6], r[7]);
    }
}
// Ray(a, b, 20 eps) for Scene::Visibility(a, b)
__global__ void k_pack_visibility(const DevScene sc, uint32_t n, const float* __restrict__ a, const float* __restrict__ b, float4* shA, float4* shB, float4* shC) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        f3 pa = mk3(a[3 * i], a[3 * i + 1], a[3 * i + 2]), pb = mk3(b[3 * i], b[3 * i + 1], b[3 * i + 2]);
        f3 diff = pb - pa;
        f3 d = norm3(diff);
        float e = sc.epsilon * 20.0f;
        shA[i] = shadow_rec_a(pa, d);
        shB[i] = shadow_rec_b(d, len3(diff) - e, i);
        shC[i] = shadow_rec_c(mk3(0.f, 0.f, 0.f), 0.0f + e);
    }
}
__global__ void k_unpack_hits(uint32_t n, const float4* __restrict__ hit, rgk_hit* out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float4 h = hit[i];
        rgk_hit r;
        r.t = h.x; r.tri = __float_as_int(h.w);
        r.a = 1.0f - h.y - h.z; r.b = h.y; r.c = h.z;
        if (r.tri < 0) { r.a = 0.f; r.b = 0.f; r.c = 0.f; }
        out[i] = r;
    }
}
__global__ void k_sampler_eval(const DevScene sc, uint32_t n, const uint32_t* seed, const uint32_t* index, const uint32_t* dim, int is2d, float* out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (is2d) { float2 v = sample2d(sc, seed[i], index[i], dim[i]); out[2 * i] = v.x; out[2 * i + 1] = v.y; }
        else { out[2 * i] = sample1d(sc, seed[i], index[i], dim[i]); out[2 * i + 1] = 0.f; }
    }
}

// ------------------------------------------------------------------ unit-level seams: BxDF::value / sample, texture lookups
// route 0: the generic code (bxdf_value / bxdf_sample: every material kind, mixes included);
// route 1: what k_shade runs for diffuse / LTC materials (mat_prepare + mat_value / mat_sample with the shared fetches), generic otherwise.
__global__ __launch_bounds__(256) void k_bxdf_value(const DevScene sc, uint32_t n, uint32_t route, const uint32_t* __restrict__ mat, const float* __restrict__ Vi,
                                                    const float* __restrict__ Vr, const float* __restrict__ uv, float* __restrict__ out) {
    lut_lds_fill(sc);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const f3 vi = mk3(Vi[3 * i], Vi[3 * i + 1], Vi[3 * i + 2]), vr = mk3(Vr[3 * i], Vr[3 * i + 1], Vr[3 * i + 2]);
        const float2 t = make_float2(uv[2 * i], uv[2 * i + 1]);
        f3 v;
        const DevMaterial m = mat_load(sc, mat[i]);
        if (route == 1u && mat_is_fast(m.kind)) {
            MatPrep mp;
            mat_prepare(sc, m, t, vr, false, mp);
            v = mat_value<false>(sc, (int)mat[i], m, mp, vi, vr, t);
        } else v = bxdf_value(sc, (int)mat[i], vi, vr, t);
        out[3 * i] = v.x; out[3 * i + 1] = v.y; out[3 * i + 2] = v.z;
    }
}
__global__ __launch_bounds__(256) void k_bxdf_sample(const DevScene sc, uint32_t n, uint32_t route, const uint32_t* __restrict__ mat, const float* __restrict__ Vi,
                                                     const float* __restrict__ uv, const float* __restrict__ u, float* __restrict__ out_dir,
                                                     float* __restrict__ out_w, uint8_t* __restrict__ leak) {
    lut_lds_fill(sc);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const f3 vi = mk3(Vi[3 * i], Vi[3 * i + 1], Vi[3 * i + 2]);
        const float2 t = make_float2(uv[2 * i], uv[2 * i + 1]), uu = make_float2(u[2 * i], u[2 * i + 1]);
        f3 d, w;
        bool ml;
        const DevMaterial m = mat_load(sc, mat[i]);
        if (route == 1u && mat_is_fast(m.kind)) {
            MatPrep mp;
            mat_prepare(sc, m, t, vi, true, mp);
            mat_sample<false>(sc, (int)mat[i], m, mp, vi, t, uu, d, w, ml);
        } else bxdf_sample(sc, (int)mat[i], vi, t, uu, d, w, ml);
        out_dir[3 * i] = d.x; out_dir[3 * i + 1] = d.y; out_dir[3 * i + 2] = d.z;
        out_w[3 * i] = w.x; out_w[3 * i + 1] = w.y; out_w[3 * i + 2] = w.z;
        leak[i] = ml ? 1 : 0;
    }
}
__global__ __launch_bounds__(256) void k_texture_sample(const DevScene sc, uint32_t n, const TexRef* __restrict__ refs, const int32_t* __restrict__ tex,
                                                        const float* __restrict__ uv, float* __restrict__ rgb, float* __restrict__ sr, float* __restrict__ sb) {
    lut_lds_fill(sc);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        TexRef t;
        t.kind = RGK_TEXREF_NONE; t.a = t.b = t.c = 0;
        if (tex[i] >= 0) t = refs[tex[i]];
        const float2 p = make_float2(uv[2 * i], uv[2 * i + 1]);
        const f3 c = tex_get(sc, t, p);
        float r, b;
        tex_slopes(sc, t, p, r, b);
        rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
        sr[i] = r; sb[i] = b;
    }
}
// the pinned transcendental functions (include/rgk_libm.h) evaluated on the device: fn 0 sin, 1 cos, 2 acos, 3 asin, 4 atan2(a, b)
__global__ void k_libm_eval(int fn, uint32_t n, const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float r = 0.f;
        if (fn == 0) r = rgk_sinf(a[i]);
        else if (fn == 1) r = rgk_cosf(a[i]);
        else if (fn == 2) r = rgk_acosf(a[i]);
        else if (fn == 3) r = rgk_asinf(a[i]);
        else r = rgk_atan2f(a[i], b[i]);
        out[i] = r;
    }
}
