// Post-processing kernels for gfx950 (MI355X): first-hit feature buffers and the guided a-trous denoiser (include/rgk.h).
//
//   k_aov_raygen    one primary ray per listed pixel through the pixel centre, in the closest-hit walker's queue layout
//   k_aov_gather    surface_point() + the material's albedo at the walker's hit -> albedo / normal / depth / triangle planes
//   k_dn_prepare    accumulator -> colour plane (float4, demodulated on request), features -> guide plane {n.xyz, z}
//   k_dn_atrous     one iteration of the edge-avoiding 5 x 5 a-trous filter, ping-ponging two colour planes
//   k_dn_finish     colour plane (float4) -> out_rgb (3 floats per pixel), remodulated on request
//
// The traversal between raygen and gather is the round's own k_trace_closest (rgk_launch_trace_closest): no second walker.
// Every formula of the filter is + - * / max in float32 with contraction off, so a numpy restatement in the same order gives
// the same bits (tests/post_ref.py).
#include <hip/hip_runtime.h>
#include "rgk_device.h"
#include "rgk_kernels.h"
#include "rgk_trace.h" // camera_ray

// ------------------------------------------------------------------ feature pass
__global__ __launch_bounds__(256) void k_aov_raygen(const DevCamera cam, uint32_t xres, uint32_t yres, const uint32_t* __restrict__ pix_xy, uint32_t n,
                                                     float4* __restrict__ rayA, float4* __restrict__ rayB) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t pix = pix_xy[i];
    f3 o, d; // (cam.lens_size == 0 here: the host passes a pinhole copy of the camera)
    camera_ray(cam, (int)(pix & 0xffffu), (int)(pix >> 16), (int)xres, (int)yres, make_float2(0.5f, 0.5f), make_float2(0.f, 0.f), o, d);
    rayA[i] = make_float4(o.x, o.y, o.z, d.x);
    rayB[i] = make_float4(d.y, d.z, __int_as_float(-1), __uint_as_float(i)); // {.., ignored triangle: none, slot}
}

// The colour a material reflects at uv, leaf kinds (rgk.h rgk_render_aov_device).
__device__ __forceinline__ f3 albedo_leaf(const DevScene& sc, const DevMaterial& m, float2 uv) {
    switch (m.kind) {
    case RGK_BXDF_DIFFUSE: return tex_get(sc, m.t_diffuse, uv);
    case RGK_BXDF_LTC_BECKMANN:
    case RGK_BXDF_LTC_GGX: return tex_get(sc, m.t_color, uv);
    case RGK_BXDF_LTC_BECKMANN_DIFFUSE:
    case RGK_BXDF_LTC_GGX_DIFFUSE: return tex_get(sc, m.t_diffuse, uv) + tex_get(sc, m.t_color, uv);
    case RGK_BXDF_MIRROR:
    case RGK_BXDF_DIELECTRIC:
    case RGK_BXDF_TRANSPARENT: return mk3(1.f, 1.f, 1.f);
    default: return mk3(0.f, 0.f, 0.f);
    }
}
// ... and mixes, to the two levels bxdf_value evaluates (a third level counts as black there too)
__device__ __forceinline__ f3 albedo_of(const DevScene& sc, const DevMaterial& m, float2 uv) {
    if (m.kind != RGK_BXDF_MIX) return albedo_leaf(sc, m, uv);
    f3 s[2];
    const int ch[2] = {m.mix_m1, m.mix_m2};
    for (int k = 0; k < 2; k++) {
        const DevMaterial c = gld_rec<DevMaterial>(sc.materials, ch[k] * (uint32_t)sizeof(DevMaterial));
        if (c.kind != RGK_BXDF_MIX) s[k] = albedo_leaf(sc, c, uv);
        else {
            const DevMaterial c1 = gld_rec<DevMaterial>(sc.materials, c.mix_m1 * (uint32_t)sizeof(DevMaterial));
            const DevMaterial c2 = gld_rec<DevMaterial>(sc.materials, c.mix_m2 * (uint32_t)sizeof(DevMaterial));
            const f3 v1 = (c1.kind == RGK_BXDF_MIX) ? mk3(0.f, 0.f, 0.f) : albedo_leaf(sc, c1, uv);
            const f3 v2 = (c2.kind == RGK_BXDF_MIX) ? mk3(0.f, 0.f, 0.f) : albedo_leaf(sc, c2, uv);
            s[k] = c.amount * v1 + (1.0f - c.amount) * v2;
        }
    }
    return m.amount * s[0] + (1.0f - m.amount) * s[1];
}

__global__ __launch_bounds__(256) void k_aov_gather(const DevScene sc, float bumpmap_scale, uint32_t xres, const uint32_t* __restrict__ pix_xy, uint32_t n,
                                                     const float4* __restrict__ rayA, const float4* __restrict__ rayB, const float4* __restrict__ hit,
                                                     float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ depth, int32_t* __restrict__ tri_out) {
    lut_lds_fill(sc); // (a barrier: before any lane leaves)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t pix = pix_xy[i];
    const size_t p = (size_t)(pix >> 16) * xres + (pix & 0xffffu);
    const float4 h = hit[i];
    const int tri = __float_as_int(h.w);
    f3 nrm = mk3(0.f, 0.f, 0.f), alb = nrm;
    float z = 0.f;
    if (tri >= 0) {
        const float4 a = rayA[i], b = rayB[i];
        Vertex v;
        surface_point(sc, bumpmap_scale, mk3(a.x, a.y, a.z), mk3(a.w, b.x, b.y), h, v);
        z = h.x;
        if (v.ok) {
            nrm = v.lightN;
            alb = albedo_of(sc, v.mat, v.uv);
        }
    }
    if (tri_out) tri_out[p] = tri < 0 ? -1 : tri;
    if (depth) depth[p] = z;
    if (normal) { normal[3 * p] = nrm.x; normal[3 * p + 1] = nrm.y; normal[3 * p + 2] = nrm.z; }
    if (albedo) { albedo[3 * p] = alb.x; albedo[3 * p + 1] = alb.y; albedo[3 * p + 2] = alb.z; }
}

void rgk_launch_aov_raygen(hipStream_t st, const DevCamera& cam, uint32_t xres, uint32_t yres, const uint32_t* pix_xy, uint32_t n, float4* rayA, float4* rayB) {
    k_aov_raygen<<<(n + 255u) / 256u, 256, 0, st>>>(cam, xres, yres, pix_xy, n, rayA, rayB);
}
void rgk_launch_aov_gather(hipStream_t st, const DevScene& sc, float bumpmap_scale, uint32_t xres, const uint32_t* pix_xy, uint32_t n, const float4* rayA,
                           const float4* rayB, const float4* hit, float* albedo, float* normal, float* depth, int32_t* tri) {
    k_aov_gather<<<(n + 255u) / 256u, 256, RGK_LDS_SHADE_BYTES, st>>>(sc, bumpmap_scale, xres, pix_xy, n, rayA, rayB, hit, albedo, normal, depth, tri);
}

// ------------------------------------------------------------------ denoiser
__device__ __forceinline__ float demod_div(float a) { return a > 0.0f ? a : 1.0f; }
__device__ __forceinline__ float demod_div(float a, float floor_) { return a > 0.0f ? fmaxf(a, floor_) : 1.0f; }

__global__ __launch_bounds__(256) void k_dn_prepare(size_t P, const float* __restrict__ accum_rgb, const uint32_t* __restrict__ accum_count,
                                                     const float* __restrict__ albedo, const float* __restrict__ normal, const float* __restrict__ depth,
                                                     uint32_t demodulate, float4* __restrict__ col, float4* __restrict__ guide) {
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= P) return;
    const uint32_t cnt = accum_count[p];
    f3 c = mk3(0.f, 0.f, 0.f);
    if (cnt) c = mk3(accum_rgb[3 * p], accum_rgb[3 * p + 1], accum_rgb[3 * p + 2]) / (float)cnt;
    if (demodulate) { c.x = c.x / demod_div(albedo[3 * p]); c.y = c.y / demod_div(albedo[3 * p + 1]); c.z = c.z / demod_div(albedo[3 * p + 2]); }
    col[p] = make_float4(c.x, c.y, c.z, 0.f);
    if (guide) guide[p] = make_float4(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], depth[p]);
}

// One iteration.  A workgroup is RGK_DN_BX x RGK_DN_BY pixels = four waves of 32 x 2 pixels: a tap of a wave is two rows of
// 32 x 16 B = 512 contiguous bytes in each plane.  Every tap is two 16-byte loads per lane (guide, then colour only where
// the guide lets the tap in).  The kernel is bound by the VALU, not by these loads: the weights' four IEEE divisions per tap
// are half of its 91 vector instructions per tap, and 2.07 M pixels x 2281 instructions at the chip's 39 T lane-instructions
// per second are the 0.12 ms it takes.
#define RGK_DN_BX 32
#define RGK_DN_BY 8
// One tap: its weight and what it adds to the sums (rgk.h rgk_denoise_params), shared by both forms of the kernel.
struct DnSums {
    float r, g, b, w;
};
__device__ __forceinline__ void dn_tap(const float4 gp, const float4 cp, const float4 gq, const float4 cq, float hh, float sigma2, float sigma_depth, uint32_t npow, DnSums& s) {
    float wn = fmaxf(0.0f, (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z);
    for (uint32_t k = 0; k < npow; k++) wn = wn * wn;
    const float r = fabsf(gp.w - gq.w) / (sigma_depth * (gp.w + gq.w) + 1e-20f);
    const float wz = 1.0f / (1.0f + r * r);
    const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
    const float d2 = (dr * dr + dg * dg) + db * db;
    const float wc = 1.0f / (1.0f + d2 / sigma2);
    const float w = ((hh * wn) * wz) * wc;
    s.r = s.r + w * cq.x; s.g = s.g + w * cq.y; s.b = s.b + w * cq.z;
    s.w = s.w + w;
}
__device__ __forceinline__ bool dn_no_normal(const float4 g) { return g.x == 0.0f && g.y == 0.0f && g.z == 0.0f; }
// (the centre tap has w > 0 unless the inputs hold NaN / infinity; such a pixel passes through)
__device__ __forceinline__ float4 dn_result(const DnSums& s, const float4 cp) { return s.w > 0.0f ? make_float4(s.r / s.w, s.g / s.w, s.b / s.w, 0.f) : cp; }

__global__ __launch_bounds__(RGK_DN_BX * RGK_DN_BY) void k_dn_atrous(int xres, int yres, int step, float sigma2, float sigma_depth, uint32_t npow,
                                                                     const float4* __restrict__ guide, const float4* __restrict__ src, float4* __restrict__ dst) {
    const int x = (int)(blockIdx.x * RGK_DN_BX + threadIdx.x), y = (int)(blockIdx.y * RGK_DN_BY + threadIdx.y);
    if (x >= xres || y >= yres) return;
    const size_t p = (size_t)y * (size_t)xres + (size_t)x;
    const float4 cp = src[p], gp = guide[p];
    if (dn_no_normal(gp)) { dst[p] = cp; return; }
    const float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    DnSums sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + step * dy;
        if (qy < 0 || qy >= yres) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + step * dx;
            if (qx < 0 || qx >= xres) continue;
            const size_t q = (size_t)qy * (size_t)xres + (size_t)qx;
            const float4 gq = guide[q];
            if (dn_no_normal(gq)) continue;
            dn_tap(gp, cp, gq, src[q], hk[dy + 2] * hk[dx + 2], sigma2, sigma_depth, npow, sum);
        }
    }
    dst[p] = dn_result(sum, cp);
}

// The same iteration with the workgroup's tile and its halo of 2 * STEP pixels staged in LDS first (both planes): every pixel of
// the tile is then fetched from memory once per workgroup instead of up to 25 times.  A halo pixel outside the frame gets a
// zero normal, which skips it exactly like the frame test above; same taps in the same order, same bits.
template <int STEP>
__global__ __launch_bounds__(RGK_DN_BX * RGK_DN_BY) void k_dn_atrous_lds(int xres, int yres, float sigma2, float sigma_depth, uint32_t npow,
                                                                         const float4* __restrict__ guide, const float4* __restrict__ src, float4* __restrict__ dst) {
    constexpr int HALO = 2 * STEP, TW = RGK_DN_BX + 2 * HALO, TH = RGK_DN_BY + 2 * HALO;
    __shared__ float4 s_g[TH * TW], s_c[TH * TW];
    const int bx0 = (int)(blockIdx.x * RGK_DN_BX) - HALO, by0 = (int)(blockIdx.y * RGK_DN_BY) - HALO;
    for (int k = (int)(threadIdx.y * RGK_DN_BX + threadIdx.x); k < TH * TW; k += RGK_DN_BX * RGK_DN_BY) {
        const int ty = k / TW, tx = k - ty * TW, gx = bx0 + tx, gy = by0 + ty;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f), c = g;
        if (gx >= 0 && gx < xres && gy >= 0 && gy < yres) {
            const size_t q = (size_t)gy * (size_t)xres + (size_t)gx;
            g = guide[q]; c = src[q];
        }
        s_g[k] = g; s_c[k] = c;
    }
    __syncthreads();
    const int x = (int)(blockIdx.x * RGK_DN_BX + threadIdx.x), y = (int)(blockIdx.y * RGK_DN_BY + threadIdx.y);
    if (x >= xres || y >= yres) return;
    const size_t p = (size_t)y * (size_t)xres + (size_t)x;
    const int t0 = ((int)threadIdx.y + HALO) * TW + (int)threadIdx.x + HALO;
    const float4 cp = s_c[t0], gp = s_g[t0];
    if (dn_no_normal(gp)) { dst[p] = cp; return; }
    const float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    DnSums sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int t = t0 + STEP * dy * TW + STEP * dx;
            const float4 gq = s_g[t];
            if (dn_no_normal(gq)) continue;
            dn_tap(gp, cp, gq, s_c[t], hk[dy + 2] * hk[dx + 2], sigma2, sigma_depth, npow, sum);
        }
    }
    dst[p] = dn_result(sum, cp);
}

// (albedo_floor: 0 for the fixed-sigma filter -- max(a, 0) == a for a > 0 -- and the variance-guided filter's floor on its divisor)
__global__ __launch_bounds__(256) void k_dn_finish(size_t P, const float4* __restrict__ col, const float* __restrict__ albedo, uint32_t demodulate, float albedo_floor,
                                                    float* __restrict__ out_rgb) {
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= P) return;
    const float4 c = col[p];
    f3 o = mk3(c.x, c.y, c.z);
    if (demodulate) { o.x = o.x * demod_div(albedo[3 * p], albedo_floor); o.y = o.y * demod_div(albedo[3 * p + 1], albedo_floor); o.z = o.z * demod_div(albedo[3 * p + 2], albedo_floor); }
    out_rgb[3 * p] = o.x; out_rgb[3 * p + 1] = o.y; out_rgb[3 * p + 2] = o.z;
}

void rgk_launch_dn_prepare(hipStream_t st, size_t P, const float* accum_rgb, const uint32_t* accum_count, const float* albedo, const float* normal, const float* depth,
                           uint32_t demodulate, float4* col, float4* guide) {
    k_dn_prepare<<<(unsigned)((P + 255) / 256), 256, 0, st>>>(P, accum_rgb, accum_count, albedo, normal, depth, demodulate, col, guide);
}
void rgk_launch_dn_atrous(hipStream_t st, uint32_t xres, uint32_t yres, uint32_t step, float sigma2, float sigma_depth, uint32_t npow, const float4* guide,
                          const float4* src, float4* dst) {
    const dim3 grid((xres + RGK_DN_BX - 1) / RGK_DN_BX, (yres + RGK_DN_BY - 1) / RGK_DN_BY), block(RGK_DN_BX, RGK_DN_BY);
    // steps 1 and 2 from LDS (measured at 1080p: 0.116 / 0.119 ms against 0.128 / 0.128 as gathers, same bits); from step 4 on the
    // halo is larger than the tile and the gathers are as fast (0.128 against 0.130)
    if (step == 1) { k_dn_atrous_lds<1><<<grid, block, 0, st>>>((int)xres, (int)yres, sigma2, sigma_depth, npow, guide, src, dst); return; }
    if (step == 2) { k_dn_atrous_lds<2><<<grid, block, 0, st>>>((int)xres, (int)yres, sigma2, sigma_depth, npow, guide, src, dst); return; }
    k_dn_atrous<<<grid, block, 0, st>>>((int)xres, (int)yres, (int)step, sigma2, sigma_depth, npow, guide, src, dst);
}
void rgk_launch_dn_finish(hipStream_t st, size_t P, const float4* col, const float* albedo, uint32_t demodulate, float albedo_floor, float* out_rgb) {
    k_dn_finish<<<(unsigned)((P + 255) / 256), 256, 0, st>>>(P, col, albedo, demodulate, albedo_floor, out_rgb);
}

// ------------------------------------------------------------------ noise estimate and the variance-guided filter
//   k_nz_tile_sums  accumulator + the odd rounds' half-buffer -> per tile {sum of v, sum of |c|^2, estimable pixels} (doubles), raw v plane
//   k_nz_prepare    the same two buffers -> colour plane {c.rgb, v} (demodulated with a floored divisor on request), guide plane
//   k_nz_prefilter  5 x 5, step 1: v -> the guide-weighted mean of its neighbourhood
//   k_nz_atrous     one iteration: the a-trous taps with wc from the two pixels' variances, variance carried in the plane's 4th float
//   k_nz_finish     the plane's 4th float -> a plane of P floats (the image itself leaves through k_dn_finish)
// Formulas: rgk.h rgk_noise_estimate_device / rgk_denoise_variance_device; the numpy restatement is tests/noise_ref.py.
struct NzPixel {
    f3 c, a, b; // mean of all rounds, of the even rounds, of the odd rounds
    float f;    // n_A * n_B / n^2
    bool est;   // both halves hold samples
};
__device__ __forceinline__ NzPixel nz_pixel(size_t p, const float* __restrict__ accum_rgb, const uint32_t* __restrict__ accum_count,
                                            const float* __restrict__ half_rgb, const uint32_t* __restrict__ half_count) {
    NzPixel r;
    r.c = r.a = r.b = mk3(0.f, 0.f, 0.f);
    r.f = 0.f;
    const uint32_t n = accum_count[p], nB = half_count[p];
    r.est = nB > 0u && nB < n;
    if (n) {
        const f3 S = mk3(accum_rgb[3 * p], accum_rgb[3 * p + 1], accum_rgb[3 * p + 2]);
        r.c = S / (float)n;
        if (r.est) {
            const f3 SB = mk3(half_rgb[3 * p], half_rgb[3 * p + 1], half_rgb[3 * p + 2]);
            const uint32_t nA = n - nB;
            r.a = (S - SB) / (float)nA;
            r.b = SB / (float)nB;
            r.f = ((float)nA * (float)nB) / ((float)n * (float)n);
        }
    }
    return r;
}
__device__ __forceinline__ float nz_variance(f3 a, f3 b, float f) {
    const f3 h = a - b;
    return ((h.x * h.x + h.y * h.y) + h.z * h.z) * f;
}

// One workgroup per tile.  Lane t takes the tile's pixels t, t + 256, ... (row-major inside the tile) into double partial sums; the
// 256 partials are then folded in LDS in a fixed order (s[t] += s[t + 128], + 64, ... + 1): no atomics, the same bits every run.
__global__ __launch_bounds__(RGK_NZ_BLOCK) void k_nz_tile_sums(uint32_t xres, uint32_t yres, uint32_t tile_size, const float* __restrict__ accum_rgb,
                                                                const uint32_t* __restrict__ accum_count, const float* __restrict__ half_rgb,
                                                                const uint32_t* __restrict__ half_count, rgk_noise_tile* __restrict__ tiles,
                                                                float* __restrict__ variance) {
    __shared__ double s_v[RGK_NZ_BLOCK], s_q[RGK_NZ_BLOCK];
    __shared__ unsigned long long s_n[RGK_NZ_BLOCK];
    const uint64_t x0 = (uint64_t)blockIdx.x * tile_size, y0 = (uint64_t)blockIdx.y * tile_size; // (< xres, yres: the grid is ceil(res / tile_size))
    const uint64_t tw = min((uint64_t)tile_size, (uint64_t)xres - x0), th = min((uint64_t)tile_size, (uint64_t)yres - y0);
    double sv = 0.0, sq = 0.0;
    unsigned long long ne = 0;
    for (uint64_t k = threadIdx.x; k < tw * th; k += RGK_NZ_BLOCK) {
        const uint64_t ty = k / tw, tx = k - ty * tw;
        const size_t p = (size_t)(y0 + ty) * xres + (size_t)(x0 + tx);
        const NzPixel px = nz_pixel(p, accum_rgb, accum_count, half_rgb, half_count);
        const float v = px.est ? nz_variance(px.a, px.b, px.f) : 0.0f;
        if (variance) variance[p] = v;
        if (px.est) {
            sv += (double)v;
            sq += (double)((px.c.x * px.c.x + px.c.y * px.c.y) + px.c.z * px.c.z);
            ne++;
        }
    }
    s_v[threadIdx.x] = sv; s_q[threadIdx.x] = sq; s_n[threadIdx.x] = ne;
    __syncthreads();
    for (uint32_t stride = RGK_NZ_BLOCK / 2; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride) {
            s_v[threadIdx.x] += s_v[threadIdx.x + stride];
            s_q[threadIdx.x] += s_q[threadIdx.x + stride];
            s_n[threadIdx.x] += s_n[threadIdx.x + stride];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        rgk_noise_tile t;
        t.sum_var = s_v[0]; t.sum_sq = s_q[0]; t.n_estimable = s_n[0];
        tiles[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(RGK_NZ_BLOCK) void k_nz_prepare(size_t P, const float* __restrict__ accum_rgb, const uint32_t* __restrict__ accum_count,
                                                              const float* __restrict__ half_rgb, const uint32_t* __restrict__ half_count,
                                                              const float* __restrict__ albedo, const float* __restrict__ normal, const float* __restrict__ depth,
                                                              uint32_t demodulate, float albedo_floor, float4* __restrict__ col, float4* __restrict__ guide) {
    const size_t p = (size_t)blockIdx.x * RGK_NZ_BLOCK + threadIdx.x;
    if (p >= P) return;
    NzPixel px = nz_pixel(p, accum_rgb, accum_count, half_rgb, half_count);
    if (demodulate) {
        const float dx = demod_div(albedo[3 * p], albedo_floor), dy = demod_div(albedo[3 * p + 1], albedo_floor), dz = demod_div(albedo[3 * p + 2], albedo_floor);
        px.c = mk3(px.c.x / dx, px.c.y / dy, px.c.z / dz);
        px.a = mk3(px.a.x / dx, px.a.y / dy, px.a.z / dz);
        px.b = mk3(px.b.x / dx, px.b.y / dy, px.b.z / dz);
    }
    col[p] = make_float4(px.c.x, px.c.y, px.c.z, px.est ? nz_variance(px.a, px.b, px.f) : 0.0f);
    if (guide) guide[p] = make_float4(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], depth[p]);
}

// The workgroup's tile and its halo of HALO pixels, both planes, into LDS; a pixel outside the frame gets a zero normal (k_dn_atrous_lds).
template <int HALO>
__device__ __forceinline__ void nz_stage(int xres, int yres, const float4* __restrict__ guide, const float4* __restrict__ src, float4* s_g, float4* s_c) {
    constexpr int TW = RGK_NZ_BX + 2 * HALO, TH = RGK_NZ_BY + 2 * HALO;
    const int bx0 = (int)(blockIdx.x * RGK_NZ_BX) - HALO, by0 = (int)(blockIdx.y * RGK_NZ_BY) - HALO;
    for (int k = (int)(threadIdx.y * RGK_NZ_BX + threadIdx.x); k < TH * TW; k += RGK_NZ_BX * RGK_NZ_BY) {
        const int ty = k / TW, tx = k - ty * TW, gx = bx0 + tx, gy = by0 + ty;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f), c = g;
        if (gx >= 0 && gx < xres && gy >= 0 && gy < yres) {
            const size_t q = (size_t)gy * (size_t)xres + (size_t)gx;
            g = guide[q]; c = src[q];
        }
        s_g[k] = g; s_c[k] = c;
    }
    __syncthreads();
}
// wn * wz of a tap (dn_tap's two guide weights)
__device__ __forceinline__ float nz_guide_weight(const float4 gp, const float4 gq, float sigma_depth, uint32_t npow) {
    float wn = fmaxf(0.0f, (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z);
    for (uint32_t k = 0; k < npow; k++) wn = wn * wn;
    const float r = fabsf(gp.w - gq.w) / (sigma_depth * (gp.w + gq.w) + 1e-20f);
    const float wz = 1.0f / (1.0f + r * r);
    return wn * wz;
}

__global__ __launch_bounds__(RGK_NZ_BX * RGK_NZ_BY) void k_nz_prefilter(int xres, int yres, float sigma_depth, uint32_t npow, const float4* __restrict__ guide,
                                                                        const float4* __restrict__ src, float4* __restrict__ dst) {
    constexpr int HALO = 2, TW = RGK_NZ_BX + 2 * HALO, TH = RGK_NZ_BY + 2 * HALO;
    __shared__ float4 s_g[TH * TW], s_c[TH * TW];
    nz_stage<HALO>(xres, yres, guide, src, s_g, s_c);
    const int x = (int)(blockIdx.x * RGK_NZ_BX + threadIdx.x), y = (int)(blockIdx.y * RGK_NZ_BY + threadIdx.y);
    if (x >= xres || y >= yres) return;
    const size_t p = (size_t)y * (size_t)xres + (size_t)x;
    const int t0 = ((int)threadIdx.y + HALO) * TW + (int)threadIdx.x + HALO;
    const float4 cp = s_c[t0], gp = s_g[t0];
    if (dn_no_normal(gp)) { dst[p] = cp; return; }
    float sv = 0.f, sw = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int t = t0 + dy * TW + dx;
            const float4 gq = s_g[t];
            if (dn_no_normal(gq)) continue;
            const float w = nz_guide_weight(gp, gq, sigma_depth, npow);
            sv = sv + w * s_c[t].w;
            sw = sw + w;
        }
    }
    dst[p] = make_float4(cp.x, cp.y, cp.z, sw > 0.0f ? sv / sw : cp.w);
}

struct NzSums {
    float r, g, b, w, v;
};
__device__ __forceinline__ void nz_tap(const float4 gp, const float4 cp, const float4 gq, const float4 cq, float hh, float k2, float sigma_depth, uint32_t npow, NzSums& s) {
    float wn = fmaxf(0.0f, (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z);
    for (uint32_t k = 0; k < npow; k++) wn = wn * wn;
    const float r = fabsf(gp.w - gq.w) / (sigma_depth * (gp.w + gq.w) + 1e-20f);
    const float wz = 1.0f / (1.0f + r * r);
    const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
    const float d2 = (dr * dr + dg * dg) + db * db;
    const float wc = 1.0f / (1.0f + d2 / (k2 * (cp.w + cq.w) + 1e-20f));
    const float w = ((hh * wn) * wz) * wc;
    s.r = s.r + w * cq.x; s.g = s.g + w * cq.y; s.b = s.b + w * cq.z;
    s.w = s.w + w;
    s.v = s.v + (w * w) * cq.w;
}
__device__ __forceinline__ float4 nz_result(const NzSums& s, const float4 cp) {
    return s.w > 0.0f ? make_float4(s.r / s.w, s.g / s.w, s.b / s.w, s.v / (s.w * s.w)) : cp;
}

__global__ __launch_bounds__(RGK_NZ_BX * RGK_NZ_BY) void k_nz_atrous(int xres, int yres, int step, float k2, float sigma_depth, uint32_t npow,
                                                                     const float4* __restrict__ guide, const float4* __restrict__ src, float4* __restrict__ dst) {
    const int x = (int)(blockIdx.x * RGK_NZ_BX + threadIdx.x), y = (int)(blockIdx.y * RGK_NZ_BY + threadIdx.y);
    if (x >= xres || y >= yres) return;
    const size_t p = (size_t)y * (size_t)xres + (size_t)x;
    const float4 cp = src[p], gp = guide[p];
    if (dn_no_normal(gp)) { dst[p] = cp; return; }
    const float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    NzSums sum = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + step * dy;
        if (qy < 0 || qy >= yres) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + step * dx;
            if (qx < 0 || qx >= xres) continue;
            const size_t q = (size_t)qy * (size_t)xres + (size_t)qx;
            const float4 gq = guide[q];
            if (dn_no_normal(gq)) continue;
            nz_tap(gp, cp, gq, src[q], hk[dy + 2] * hk[dx + 2], k2, sigma_depth, npow, sum);
        }
    }
    dst[p] = nz_result(sum, cp);
}

template <int STEP>
__global__ __launch_bounds__(RGK_NZ_BX * RGK_NZ_BY) void k_nz_atrous_lds(int xres, int yres, float k2, float sigma_depth, uint32_t npow,
                                                                         const float4* __restrict__ guide, const float4* __restrict__ src, float4* __restrict__ dst) {
    constexpr int HALO = 2 * STEP, TW = RGK_NZ_BX + 2 * HALO, TH = RGK_NZ_BY + 2 * HALO;
    __shared__ float4 s_g[TH * TW], s_c[TH * TW];
    nz_stage<HALO>(xres, yres, guide, src, s_g, s_c);
    const int x = (int)(blockIdx.x * RGK_NZ_BX + threadIdx.x), y = (int)(blockIdx.y * RGK_NZ_BY + threadIdx.y);
    if (x >= xres || y >= yres) return;
    const size_t p = (size_t)y * (size_t)xres + (size_t)x;
    const int t0 = ((int)threadIdx.y + HALO) * TW + (int)threadIdx.x + HALO;
    const float4 cp = s_c[t0], gp = s_g[t0];
    if (dn_no_normal(gp)) { dst[p] = cp; return; }
    const float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    NzSums sum = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int t = t0 + STEP * dy * TW + STEP * dx;
            const float4 gq = s_g[t];
            if (dn_no_normal(gq)) continue;
            nz_tap(gp, cp, gq, s_c[t], hk[dy + 2] * hk[dx + 2], k2, sigma_depth, npow, sum);
        }
    }
    dst[p] = nz_result(sum, cp);
}

__global__ __launch_bounds__(RGK_NZ_BLOCK) void k_nz_finish(size_t P, const float4* __restrict__ col, float* __restrict__ out_variance) {
    const size_t p = (size_t)blockIdx.x * RGK_NZ_BLOCK + threadIdx.x;
    if (p >= P) return;
    out_variance[p] = col[p].w;
}

void rgk_launch_nz_tile_sums(hipStream_t st, uint32_t xres, uint32_t yres, uint32_t tile_size, const float* accum_rgb, const uint32_t* accum_count,
                             const float* half_rgb, const uint32_t* half_count, rgk_noise_tile* tiles, float* variance) {
    const RgkGrid2 g = rgk_nz_tile_grid(xres, yres, tile_size);
    k_nz_tile_sums<<<dim3(g.x, g.y), RGK_NZ_BLOCK, 0, st>>>(xres, yres, tile_size, accum_rgb, accum_count, half_rgb, half_count, tiles, variance);
}
void rgk_launch_nz_prepare(hipStream_t st, size_t P, const float* accum_rgb, const uint32_t* accum_count, const float* half_rgb, const uint32_t* half_count,
                           const float* albedo, const float* normal, const float* depth, uint32_t demodulate, float albedo_floor, float4* col, float4* guide) {
    k_nz_prepare<<<rgk_nz_pixel_grid(P), RGK_NZ_BLOCK, 0, st>>>(P, accum_rgb, accum_count, half_rgb, half_count, albedo, normal, depth, demodulate, albedo_floor, col, guide);
}
void rgk_launch_nz_prefilter(hipStream_t st, uint32_t xres, uint32_t yres, float sigma_depth, uint32_t npow, const float4* guide, const float4* src, float4* dst) {
    const RgkGrid2 g = rgk_nz_filter_grid(xres, yres);
    k_nz_prefilter<<<dim3(g.x, g.y), dim3(RGK_NZ_BX, RGK_NZ_BY), 0, st>>>((int)xres, (int)yres, sigma_depth, npow, guide, src, dst);
}
void rgk_launch_nz_atrous(hipStream_t st, uint32_t xres, uint32_t yres, uint32_t step, float k2, float sigma_depth, uint32_t npow, const float4* guide,
                          const float4* src, float4* dst) {
    const RgkGrid2 g = rgk_nz_filter_grid(xres, yres);
    const dim3 grid(g.x, g.y), block(RGK_NZ_BX, RGK_NZ_BY);
    // the LDS form for steps 1 and 2, gathers above, as rgk_launch_dn_atrous
    if (step == 1) { k_nz_atrous_lds<1><<<grid, block, 0, st>>>((int)xres, (int)yres, k2, sigma_depth, npow, guide, src, dst); return; }
    if (step == 2) { k_nz_atrous_lds<2><<<grid, block, 0, st>>>((int)xres, (int)yres, k2, sigma_depth, npow, guide, src, dst); return; }
    k_nz_atrous<<<grid, block, 0, st>>>((int)xres, (int)yres, (int)step, k2, sigma_depth, npow, guide, src, dst);
}
void rgk_launch_nz_finish(hipStream_t st, size_t P, const float4* col, float* out_variance) {
    k_nz_finish<<<rgk_nz_pixel_grid(P), RGK_NZ_BLOCK, 0, st>>>(P, col, out_variance);
}
