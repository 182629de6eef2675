// Post-processing kernels for gfx950 (MI355X): first-hit feature buffers and the guided a-trous denoiser (include/rgk.h).
//
//   k_aov_raygen    one primary ray per listed pixel through the pixel centre, in the closest-hit walker's queue layout
//   k_aov_gather    surface_point() + the material's albedo at the walker's hit -> albedo / normal / depth / triangle planes
//   k_dn_prepare<HALVES>     accumulator [+ the odd rounds' half-buffer] -> colour plane {c.rgb, v} (demodulated on request; v = 0
//                            without halves), features -> guide plane {n.xyz, z}
//   k_dn_atrous<Mode, STEP>  one pass of the edge-avoiding 5 x 5 a-trous filter, ping-ponging two colour planes.  Mode: FixedSigma,
//                            VarianceGuided (wc from the two pixels' variances, carried in the plane's 4th float) or VarianceMean
//                            (its prefilter: v -> the guide-weighted mean of its neighbourhood).  STEP 1, 2: taps from a tile in
//                            LDS; 0: gathered at the run-time step
//   k_dn_finish              colour plane (float4) -> out_rgb (3 floats per pixel), remodulated on request
//   k_nz_finish              the plane's 4th float -> a plane of P floats
//   k_nz_tile_sums           accumulator + half-buffer -> per tile {sum of v, sum of |c|^2, estimable pixels} (doubles), raw v plane
//   k_round_fold             the listed tiles of a per-round accumulator -> += into the frame's, per tile into the half-buffer, and cleared
//   k_tp_reproject           the previous frame's history {rgb, length} -> the current frame's pixels: four taps, each tested against the
//                            previous frame's feature planes
//   k_tp_blend               accumulator + reprojected history -> the next frame's history and the image to filter
//   k_aov_hop                one hop of the feature planes that follow mirrors and glass: a terminal vertex, miss or dropped vertex
//                            -> the planes, a delta vertex -> the continuation ray, compacted into the next hop's queue
//   k_us_prepare             a low-resolution accumulator and its feature planes -> 16-byte tap records {m.rgb, flags}, {x_q}, {n_q}
//   k_us_gather              the full grid's pixels projected into the low grid: ring 1 (bilinear), ring 2 (4 x 4), nearest
//   k_display_hist           an image's luminances -> a 256-bin histogram, 8 bins per octave, and the count of black pixels
//   k_display_encode         an image -> exposure, tone curve, sRGB transfer table -> one R, G, B, 255 word per pixel
// (tests/noise_ref.py's k_nz_prepare, k_nz_prefilter and k_nz_atrous are k_dn_prepare<true> and k_dn_atrous<VarianceMean / VarianceGuided>)
//
// The traversal between raygen and gather is the round's own k_trace_closest (rgk_launch_trace_closest): no second walker.
// Every formula of the filter is + - * / max in float32 with contraction off, so a numpy restatement in the same order gives
// the same bits (tests/post_ref.py, tests/noise_ref.py).
#include <hip/hip_runtime.h>
#include "rgk_device.h"
#include "rgk_display.h"
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
// Both filters of rgk.h -- fixed sigma (rgk_denoise_device) and variance guided with its prefilter (rgk_denoise_variance_device) --
// and the noise estimate's tile statistics (rgk_noise_estimate_device).
// (FLOORED false: the fixed-sigma filter's divisor -- what a floor of 0 gives, max(a, 0) == a for a > 0, without the max)
template <bool FLOORED = true>
__device__ __forceinline__ float demod_div(float a, float floor_) { return a > 0.0f ? (FLOORED ? fmaxf(a, floor_) : a) : 1.0f; }

struct NzPixel {
    f3 c, a, b; // mean of all rounds, of the even rounds, of the odd rounds
    float f;    // n_A * n_B / n^2
    bool est;   // both halves hold samples
};
// (HALVES false: no half-buffer, nothing is estimable and half_rgb / half_count are not read)
template <bool HALVES>
__device__ __forceinline__ NzPixel nz_pixel(size_t p, const float* __restrict__ accum_rgb, const uint32_t* __restrict__ accum_count,
                                            const float* __restrict__ half_rgb, const uint32_t* __restrict__ half_count) {
    NzPixel r;
    r.c = r.a = r.b = mk3(0.f, 0.f, 0.f);
    r.f = 0.f;
    const uint32_t n = accum_count[p], nB = HALVES ? half_count[p] : 0u;
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
__global__ __launch_bounds__(RGK_POST_BLOCK) void k_nz_tile_sums(uint32_t xres, uint32_t yres, uint32_t tile_size, const float* __restrict__ accum_rgb,
                                                                  const uint32_t* __restrict__ accum_count, const float* __restrict__ half_rgb,
                                                                  const uint32_t* __restrict__ half_count, rgk_noise_tile* __restrict__ tiles,
                                                                  float* __restrict__ variance) {
    __shared__ double s_v[RGK_POST_BLOCK], s_q[RGK_POST_BLOCK];
    __shared__ unsigned long long s_n[RGK_POST_BLOCK];
    const uint64_t x0 = (uint64_t)blockIdx.x * tile_size, y0 = (uint64_t)blockIdx.y * tile_size; // (< xres, yres: the grid is ceil(res / tile_size))
    const uint64_t tw = min((uint64_t)tile_size, (uint64_t)xres - x0), th = min((uint64_t)tile_size, (uint64_t)yres - y0);
    double sv = 0.0, sq = 0.0;
    unsigned long long ne = 0;
    for (uint64_t k = threadIdx.x; k < tw * th; k += RGK_POST_BLOCK) {
        const uint64_t ty = k / tw, tx = k - ty * tw;
        const size_t p = (size_t)(y0 + ty) * xres + (size_t)(x0 + tx);
        const NzPixel px = nz_pixel<true>(p, accum_rgb, accum_count, half_rgb, half_count);
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
    for (uint32_t stride = RGK_POST_BLOCK / 2; stride > 0; stride >>= 1) {
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

// Accumulator [+ the odd rounds' half-buffer] -> colour plane {c.rgb, v}, features -> guide plane.  Without a half-buffer no pixel is
// estimable: v = 0, and a and b are never formed; albedo_floor belongs to the variance-guided filter and is not read either.
template <bool HALVES>
__global__ __launch_bounds__(RGK_POST_BLOCK) void k_dn_prepare(size_t P, const float* __restrict__ accum_rgb, const uint32_t* __restrict__ accum_count,
                                                                const float* __restrict__ half_rgb, const uint32_t* __restrict__ half_count,
                                                                const float* __restrict__ albedo, const float* __restrict__ normal, const float* __restrict__ depth,
                                                                uint32_t demodulate, float albedo_floor, float4* __restrict__ col, float4* __restrict__ guide) {
    const size_t p = (size_t)blockIdx.x * RGK_POST_BLOCK + threadIdx.x;
    if (p >= P) return;
    NzPixel px = nz_pixel<HALVES>(p, accum_rgb, accum_count, half_rgb, half_count);
    if (demodulate) {
        const float dx = demod_div<HALVES>(albedo[3 * p], albedo_floor), dy = demod_div<HALVES>(albedo[3 * p + 1], albedo_floor), dz = demod_div<HALVES>(albedo[3 * p + 2], albedo_floor);
        px.c = mk3(px.c.x / dx, px.c.y / dy, px.c.z / dz);
        px.a = mk3(px.a.x / dx, px.a.y / dy, px.a.z / dz);
        px.b = mk3(px.b.x / dx, px.b.y / dy, px.b.z / dz);
    }
    col[p] = make_float4(px.c.x, px.c.y, px.c.z, px.est ? nz_variance(px.a, px.b, px.f) : 0.0f);
    if (guide) guide[p] = make_float4(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], depth[p]);
}

// ---- the a-trous filter: the weights every mode shares ...
__device__ __forceinline__ bool dn_no_normal(const float4 g) { return g.x == 0.0f && g.y == 0.0f && g.z == 0.0f; }
struct GuideWeights {
    float wn, wz;
};
__device__ __forceinline__ GuideWeights dn_guide_weights(const float4 gp, const float4 gq, float sigma_depth, uint32_t npow) {
    float wn = fmaxf(0.0f, (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z);
    for (uint32_t k = 0; k < npow; k++) wn = wn * wn;
    const float r = fabsf(gp.w - gq.w) / (sigma_depth * (gp.w + gq.w) + 1e-20f);
    return {wn, 1.0f / (1.0f + r * r)};
}
__device__ __forceinline__ float dn_color_d2(const float4 cp, const float4 cq) {
    const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
    return (dr * dr + dg * dg) + db * db;
}
// ... and the three modes: a pixel's sums, what one tap adds to them (`hh`: the tap's h[dy] * h[dx], `c`: the launch's constant) and
// what the pixel becomes.  The centre tap has w > 0 unless the inputs hold NaN / infinity; such a pixel passes through.
struct FixedSigma { // c = sigma_i^2
    float r = 0.f, g = 0.f, b = 0.f, w = 0.f;
    __device__ __forceinline__ void tap(const GuideWeights gw, float hh, float c, const float4 cp, const float4 cq) {
        const float wc = 1.0f / (1.0f + dn_color_d2(cp, cq) / c);
        const float t = ((hh * gw.wn) * gw.wz) * wc;
        r = r + t * cq.x; g = g + t * cq.y; b = b + t * cq.z;
        w = w + t;
    }
    __device__ __forceinline__ float4 result(const float4 cp) const { return w > 0.0f ? make_float4(r / w, g / w, b / w, 0.f) : cp; }
};
struct VarianceGuided { // c = sigma_k^2; the plane's 4th float carries the variance
    float r = 0.f, g = 0.f, b = 0.f, w = 0.f, v = 0.f;
    __device__ __forceinline__ void tap(const GuideWeights gw, float hh, float c, const float4 cp, const float4 cq) {
        const float wc = 1.0f / (1.0f + dn_color_d2(cp, cq) / (c * (cp.w + cq.w) + 1e-20f));
        const float t = ((hh * gw.wn) * gw.wz) * wc;
        r = r + t * cq.x; g = g + t * cq.y; b = b + t * cq.z;
        w = w + t;
        v = v + (t * t) * cq.w;
    }
    __device__ __forceinline__ float4 result(const float4 cp) const { return w > 0.0f ? make_float4(r / w, g / w, b / w, v / (w * w)) : cp; }
};
struct VarianceMean { // the prefilter (step 1 only): variance -> the guide-weighted mean of its neighbourhood, the colour passes through
    float sv = 0.f, sw = 0.f;
    __device__ __forceinline__ void tap(const GuideWeights gw, float, float, const float4, const float4 cq) {
        const float t = gw.wn * gw.wz;
        sv = sv + t * cq.w;
        sw = sw + t;
    }
    __device__ __forceinline__ float4 result(const float4 cp) const { return make_float4(cp.x, cp.y, cp.z, sw > 0.0f ? sv / sw : cp.w); }
};

// The workgroup's tile and its halo of HALO pixels, both planes, into LDS; a pixel outside the frame gets a zero normal.
template <int HALO>
__device__ __forceinline__ void dn_stage(int xres, int yres, const float4* __restrict__ guide, const float4* __restrict__ src, float4* s_g, float4* s_c) {
    constexpr int TW = RGK_POST_BX + 2 * HALO, TH = RGK_POST_BY + 2 * HALO;
    const int bx0 = (int)(blockIdx.x * RGK_POST_BX) - HALO, by0 = (int)(blockIdx.y * RGK_POST_BY) - HALO;
    for (int k = (int)(threadIdx.y * RGK_POST_BX + threadIdx.x); k < TH * TW; k += RGK_POST_BX * RGK_POST_BY) {
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

// One iteration of one mode: 5 x 5 taps `step` pixels apart, dy outer, dx inner.  A workgroup is RGK_POST_BX x RGK_POST_BY pixels =
// four waves of 32 x 2 pixels: a tap of a wave is two rows of 32 x 16 B = 512 contiguous bytes in each plane.  Every tap is two
// 16-byte loads per lane (guide, then colour only where the guide lets the tap in).  The kernel is bound by the VALU, not by these
// loads: the weights' four IEEE divisions per tap are half of its 91 vector instructions per tap, and 2.07 M pixels x 2281
// instructions at the chip's 39 T lane-instructions per second are the 0.12 ms it takes.
//   STEP 0     the taps are gathered from the planes, `step` apart; a tap outside the frame is skipped
//   STEP 1, 2  the tile and its halo of 2 * STEP pixels are staged in LDS first (both planes): every pixel of the tile is then fetched
//              from memory once per workgroup instead of up to 25 times.  A zero normal skips a halo pixel outside the frame exactly
//              like the frame test; same taps in the same order, same bits.  (`step` is not read.)
template <class Mode, int STEP>
__global__ __launch_bounds__(RGK_POST_BX * RGK_POST_BY) void k_dn_atrous(int xres, int yres, int step, float c, float sigma_depth, uint32_t npow,
                                                                         const float4* __restrict__ guide, const float4* __restrict__ src, float4* __restrict__ dst) {
    constexpr bool LDS = STEP > 0;
    constexpr int HALO = 2 * STEP, TW = RGK_POST_BX + 2 * HALO, TH = RGK_POST_BY + 2 * HALO;
    __shared__ float4 s_g[LDS ? TH * TW : 1], s_c[LDS ? TH * TW : 1];
    if constexpr (LDS) dn_stage<HALO>(xres, yres, guide, src, s_g, s_c);
    const int x = (int)(blockIdx.x * RGK_POST_BX + threadIdx.x), y = (int)(blockIdx.y * RGK_POST_BY + threadIdx.y);
    if (x >= xres || y >= yres) return;
    const size_t p = (size_t)y * (size_t)xres + (size_t)x;
    const int t0 = ((int)threadIdx.y + HALO) * TW + (int)threadIdx.x + HALO;
    const float4 cp = LDS ? s_c[t0] : src[p], gp = LDS ? s_g[t0] : guide[p];
    if (dn_no_normal(gp)) { dst[p] = cp; return; }
    const float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    Mode sum;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + step * dy;
        if (!LDS && (qy < 0 || qy >= yres)) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + step * dx;
            if (!LDS && (qx < 0 || qx >= xres)) continue;
            const int t = t0 + STEP * dy * TW + STEP * dx;                   // in the tile
            const size_t q = (size_t)qy * (size_t)xres + (size_t)qx;         // in the planes
            const float4 gq = LDS ? s_g[t] : guide[q];
            if (dn_no_normal(gq)) continue;
            const float4 cq = LDS ? s_c[t] : src[q]; // (asked for before the weights: the squaring loop hides the gather's latency)
            sum.tap(dn_guide_weights(gp, gq, sigma_depth, npow), hk[dy + 2] * hk[dx + 2], c, cp, cq);
        }
    }
    dst[p] = sum.result(cp);
}

// (albedo_floor: 0 for the fixed-sigma filter -- max(a, 0) == a for a > 0 -- and the variance-guided filter's floor on its divisor)
__global__ __launch_bounds__(RGK_POST_BLOCK) void k_dn_finish(size_t P, const float4* __restrict__ col, const float* __restrict__ albedo, uint32_t demodulate, float albedo_floor,
                                                               float* __restrict__ out_rgb) {
    const size_t p = (size_t)blockIdx.x * RGK_POST_BLOCK + threadIdx.x;
    if (p >= P) return;
    const float4 c = col[p];
    f3 o = mk3(c.x, c.y, c.z);
    if (demodulate) { o.x = o.x * demod_div(albedo[3 * p], albedo_floor); o.y = o.y * demod_div(albedo[3 * p + 1], albedo_floor); o.z = o.z * demod_div(albedo[3 * p + 2], albedo_floor); }
    out_rgb[3 * p] = o.x; out_rgb[3 * p + 1] = o.y; out_rgb[3 * p + 2] = o.z;
}
__global__ __launch_bounds__(RGK_POST_BLOCK) void k_nz_finish(size_t P, const float4* __restrict__ col, float* __restrict__ out_variance) {
    const size_t p = (size_t)blockIdx.x * RGK_POST_BLOCK + threadIdx.x;
    if (p >= P) return;
    out_variance[p] = col[p].w;
}

void rgk_launch_nz_tile_sums(hipStream_t st, uint32_t xres, uint32_t yres, uint32_t tile_size, const float* accum_rgb, const uint32_t* accum_count,
                             const float* half_rgb, const uint32_t* half_count, rgk_noise_tile* tiles, float* variance) {
    const RgkGrid2 g = rgk_nz_tile_grid(xres, yres, tile_size);
    k_nz_tile_sums<<<dim3(g.x, g.y), RGK_POST_BLOCK, 0, st>>>(xres, yres, tile_size, accum_rgb, accum_count, half_rgb, half_count, tiles, variance);
}
void rgk_launch_dn_prepare(hipStream_t st, size_t P, const float* accum_rgb, const uint32_t* accum_count, const float* half_rgb, const uint32_t* half_count,
                           const float* albedo, const float* normal, const float* depth, uint32_t demodulate, float albedo_floor, float4* col, float4* guide) {
    const uint32_t grid = rgk_post_pixel_grid(P);
    if (half_rgb) k_dn_prepare<true><<<grid, RGK_POST_BLOCK, 0, st>>>(P, accum_rgb, accum_count, half_rgb, half_count, albedo, normal, depth, demodulate, albedo_floor, col, guide);
    else k_dn_prepare<false><<<grid, RGK_POST_BLOCK, 0, st>>>(P, accum_rgb, accum_count, nullptr, nullptr, albedo, normal, depth, demodulate, albedo_floor, col, guide);
}
struct DnAtrousLaunch {
    hipStream_t st;
    uint32_t xres, yres, step;
    float c, sigma_depth;
    uint32_t npow;
    const float4 *guide, *src;
    float4* dst;
};
template <class Mode, int STEP>
static void launch_atrous(const DnAtrousLaunch& a) {
    const RgkGrid2 g = rgk_post_filter_grid(a.xres, a.yres);
    k_dn_atrous<Mode, STEP><<<dim3(g.x, g.y), dim3(RGK_POST_BX, RGK_POST_BY), 0, a.st>>>((int)a.xres, (int)a.yres, (int)a.step, a.c, a.sigma_depth, a.npow, a.guide, a.src, a.dst);
}
template <class Mode>
static void launch_atrous_by_step(const DnAtrousLaunch& a) {
    // steps 1 and 2 from LDS (measured at 1080p: 0.116 / 0.119 ms against 0.128 / 0.128 as gathers, same bits); from step 4 on the
    // halo is larger than the tile and the gathers are as fast (0.128 against 0.130)
    if (a.step == 1) launch_atrous<Mode, 1>(a);
    else if (a.step == 2) launch_atrous<Mode, 2>(a);
    else launch_atrous<Mode, 0>(a);
}
void rgk_launch_dn_atrous(hipStream_t st, RgkDnMode mode, uint32_t xres, uint32_t yres, uint32_t step, float c, float sigma_depth, uint32_t npow,
                          const float4* guide, const float4* src, float4* dst) {
    const DnAtrousLaunch a = {st, xres, yres, step, c, sigma_depth, npow, guide, src, dst};
    switch (mode) {
    case RGK_DN_FIXED_SIGMA: launch_atrous_by_step<FixedSigma>(a); break;
    case RGK_DN_VARIANCE_GUIDED: launch_atrous_by_step<VarianceGuided>(a); break;
    case RGK_DN_VARIANCE_MEAN: launch_atrous<VarianceMean, 1>(a); break; // (the prefilter: step 1 whatever `step` says)
    }
}
void rgk_launch_dn_finish(hipStream_t st, size_t P, const float4* col, const float* albedo, uint32_t demodulate, float albedo_floor, float* out_rgb) {
    k_dn_finish<<<rgk_post_pixel_grid(P), RGK_POST_BLOCK, 0, st>>>(P, col, albedo, demodulate, albedo_floor, out_rgb);
}
void rgk_launch_nz_finish(hipStream_t st, size_t P, const float4* col, float* out_variance) {
    k_nz_finish<<<rgk_post_pixel_grid(P), RGK_POST_BLOCK, 0, st>>>(P, col, out_variance);
}

// ------------------------------------------------------------------ the round fold (rgk.h rgk_round_fold_device)
// One plane pair of one band (rgk_plan.h: which elements, in which order): total += round, half += round where the tile's flag
// says so, round = 0.  One float32 / uint32 addition per element, nothing contracted: the bits of the whole-frame additions it stands
// in for.  Pure streaming -- per element 2 or 3 loads and as many stores of 4 bytes, a wave's instruction 256 contiguous bytes -- and
// nothing outside the band is touched.  (The planes are six different buffers: the host has checked.)
template <uint32_t C, class T>
__device__ __forceinline__ void fold_band(uint32_t xres, uint32_t x0, uint32_t y, uint32_t tw, uint32_t rows, bool to_half, T* __restrict__ round_,
                                          T* __restrict__ total, T* __restrict__ half) {
    const uint32_t n = rows * tw * C;
    for (uint32_t k = threadIdx.x; k < n; k += RGK_POST_BLOCK) {
        const size_t e = rgk_fold_element(xres, x0, y, tw, C, k);
        const T r = round_[e];
        total[e] = total[e] + r;
        if (to_half) half[e] = half[e] + r; // (the same for a whole workgroup)
        round_[e] = (T)0;
    }
}
__global__ __launch_bounds__(RGK_POST_BLOCK) void k_round_fold(uint32_t xres, const rgk_tile* __restrict__ tiles, const uint8_t* __restrict__ to_half,
                                                                float* __restrict__ round_rgb, uint32_t* __restrict__ round_count, float* __restrict__ total_rgb,
                                                                uint32_t* __restrict__ total_count, float* __restrict__ half_rgb, uint32_t* __restrict__ half_count) {
    const rgk_tile t = tiles[blockIdx.x];
    const RgkRowRange rr = rgk_fold_band(blockIdx.y, t.y1 - t.y0);
    if (rr.r0 == rr.r1) return; // a band below this tile's last row
    const bool h = to_half[blockIdx.x] != 0;
    const uint32_t tw = t.x1 - t.x0, y = t.y0 + rr.r0, rows = rr.r1 - rr.r0;
    fold_band<3u>(xres, t.x0, y, tw, rows, h, round_rgb, total_rgb, half_rgb);
    fold_band<1u>(xres, t.x0, y, tw, rows, h, round_count, total_count, half_count);
}
void rgk_launch_round_fold(hipStream_t st, uint32_t xres, const rgk_tile* tiles, const uint8_t* to_half, uint32_t n_tiles, uint32_t max_tile_height,
                           float* round_rgb, uint32_t* round_count, float* total_rgb, uint32_t* total_count, float* half_rgb, uint32_t* half_count) {
    const RgkGrid2 g = rgk_fold_grid(n_tiles, max_tile_height);
    k_round_fold<<<dim3(g.x, g.y), RGK_POST_BLOCK, 0, st>>>(xres, tiles, to_half, round_rgb, round_count, total_rgb, total_count, half_rgb, half_count);
}

// ------------------------------------------------------------------ temporal reuse (rgk.h rgk_temporal_reproject_device / _blend_device)
// One pixel of the current frame per lane; every formula in rgk.h's order, float32, nothing contracted (tests/temporal_ref.py gives
// the same bits).  Streaming gathers: a lane reads 20 B of the current planes, the 4 B of its triangle's material index and that
// material's kind, and per tap {length 4, triangle 4, depth 4, normal 12, colour 12 B} -- the feature planes only where the length
// lets the tap in, the colour only where the features do -- and writes 16 B.  A wave's taps are two rows of up to 65 neighbouring
// pixels of the previous frame wherever the motion is a shift, so the gathers are coalesced like the a-trous filter's at step 1.
// (Both are templates for one reason: the compiler emits a template's code where it is first used, here after every other kernel
// of this file, whose assembly -- the numbers in its labels included -- then stays what it was: tools/device_code_diff.sh compares text.)
__device__ __forceinline__ f3 ld3(const float* __restrict__ a, size_t p) { return mk3(a[3 * p], a[3 * p + 1], a[3 * p + 2]); }

template <int = 0>
__global__ __launch_bounds__(RGK_POST_BLOCK) void k_tp_reproject(const DevScene sc, uint32_t n_triangles, const DevCamera cam, const DevCamera prev, int xres, int yres,
                                                                  const float* __restrict__ depth, const float* __restrict__ normal, const int32_t* __restrict__ tri,
                                                                  const float* __restrict__ depth_prev, const float* __restrict__ normal_prev,
                                                                  const int32_t* __restrict__ tri_prev, const float* __restrict__ hist_rgb_prev,
                                                                  const float* __restrict__ hist_len_prev, float plane_tol, float normal_cos,
                                                                  float* __restrict__ hist_rgb, float* __restrict__ hist_len) {
    const size_t p = (size_t)blockIdx.x * RGK_POST_BLOCK + threadIdx.x;
    if (p >= (size_t)xres * (size_t)yres) return;
    const int y = (int)(p / (size_t)xres), x = (int)(p - (size_t)y * (size_t)xres);
    f3 o, d; // (lens_size == 0 in both cameras: the host passes pinhole copies)
    camera_ray(cam, x, y, xres, yres, make_float2(0.5f, 0.5f), make_float2(0.f, 0.f), o, d);
    const int t = tri[p];
    const bool hit = t >= 0;
    const f3 o_prev = mk3(prev.origin[0], prev.origin[1], prev.origin[2]);
    const f3 xp = o + d * depth[p];
    const f3 v = hit ? xp - o_prev : d;
    const f3 np = ld3(normal, p);
    bool ok = true;
    if (hit) {
        ok = (uint32_t)t < n_triangles && !is_zero3(np);
        if (ok) { // the tables k_aov_gather reads: the triangle's shading record names its material
            const uint32_t mat = gld_u32(sc.tri_shade, (uint32_t)t * (uint32_t)sizeof(TriShade) + 96u);
            const uint32_t kind = gld_u32(sc.materials, mat * (uint32_t)sizeof(DevMaterial));
            ok = !(kind == RGK_BXDF_MIRROR || kind == RGK_BXDF_DIELECTRIC || kind == RGK_BXDF_TRANSPARENT);
        }
    }
    const f3 N = mk3(prev.direction[0], prev.direction[1], prev.direction[2]);
    const float q = dot3(v, N);
    float sr = 0.f, sg = 0.f, sb = 0.f, sl = 0.f, sw = 0.f;
    if (ok && q > 0.0f) {
        const f3 vs = mk3(prev.viewscreen[0], prev.viewscreen[1], prev.viewscreen[2]);
        const f3 vx = mk3(prev.viewscreen_x[0], prev.viewscreen_x[1], prev.viewscreen_x[2]);
        const f3 vy = mk3(prev.viewscreen_y[0], prev.viewscreen_y[1], prev.viewscreen_y[2]);
        const float s = dot3(vs - o_prev, N) / q;
        const f3 w = (o_prev + v * s) - vs;
        const float a = dot3(w, vx) / dot3(vx, vx), b = dot3(w, vy) / dot3(vy, vy);
        const float fx = a * (float)xres - 0.5f, fy = b * (float)yres - 0.5f;
        if (fx > -1.0f && fx < (float)xres && fy > -1.0f && fy < (float)yres) { // (false for NaN)
            const float flx = floorf(fx), fly = floorf(fy);
            const int ix = (int)flx, iy = (int)fly;
            const float tx = fx - flx, ty = fy - fly;
            const float wt[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
            const float tol = plane_tol * len3(v);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int qx = ix + (k & 1), qy = iy + (k >> 1);
                if (qx < 0 || qx >= xres || qy < 0 || qy >= yres) continue;
                const size_t qi = (size_t)qy * (size_t)xres + (size_t)qx;
                const float lq = hist_len_prev[qi];
                if (!(lq > 0.0f)) continue;
                const bool hq = tri_prev[qi] >= 0;
                if (hq != hit) continue;
                if (hit) {
                    const f3 nq = ld3(normal_prev, qi);
                    if (!(dot3(np, nq) >= normal_cos)) continue;
                    f3 oq, dq;
                    camera_ray(prev, qx, qy, xres, yres, make_float2(0.5f, 0.5f), make_float2(0.f, 0.f), oq, dq);
                    if (!(fabsf(dot3(xp - (o_prev + dq * depth_prev[qi]), nq)) <= tol)) continue;
                }
                const f3 c = ld3(hist_rgb_prev, qi);
                sr = sr + wt[k] * c.x; sg = sg + wt[k] * c.y; sb = sb + wt[k] * c.z;
                sl = sl + wt[k] * lq;
                sw = sw + wt[k];
            }
        }
    }
    const bool have = sw > 0.0f; // (sum(w) == 0, and everything that never reached the taps: no history)
    hist_rgb[3 * p] = have ? sr / sw : 0.0f; hist_rgb[3 * p + 1] = have ? sg / sw : 0.0f; hist_rgb[3 * p + 2] = have ? sb / sw : 0.0f;
    hist_len[p] = have ? sl / sw : 0.0f;
}

template <int = 0>
__global__ __launch_bounds__(RGK_POST_BLOCK) void k_tp_blend(size_t P, const float* __restrict__ accum_rgb, const uint32_t* __restrict__ accum_count,
                                                              const float* __restrict__ albedo, const float* __restrict__ hist_rgb, const float* __restrict__ hist_len,
                                                              float alpha_min, float max_len, uint32_t demodulate, float albedo_floor,
                                                              float* __restrict__ out_hist_rgb, float* __restrict__ out_hist_len, float* __restrict__ out_rgb) {
    const size_t p = (size_t)blockIdx.x * RGK_POST_BLOCK + threadIdx.x;
    if (p >= P) return;
    const uint32_t n = accum_count[p];
    const f3 h = ld3(hist_rgb, p);
    const float L = hist_len[p];
    f3 div = mk3(1.f, 1.f, 1.f);
    if (demodulate) div = mk3(demod_div(albedo[3 * p], albedo_floor), demod_div(albedo[3 * p + 1], albedo_floor), demod_div(albedo[3 * p + 2], albedo_floor));
    f3 m = h;
    float Ln = L;
    if (n) {
        const f3 c = ld3(accum_rgb, p) / (float)n;
        m = mk3(c.x / div.x, c.y / div.y, c.z / div.z);
        Ln = 1.0f;
        if (L > 0.0f) {
            const float alpha = fmaxf(1.0f / (L + 1.0f), alpha_min);
            m = (m - h) * alpha + h;
            Ln = fminf(L + 1.0f, max_len);
        }
    }
    out_hist_rgb[3 * p] = m.x; out_hist_rgb[3 * p + 1] = m.y; out_hist_rgb[3 * p + 2] = m.z;
    out_hist_len[p] = Ln;
    out_rgb[3 * p] = m.x * div.x; out_rgb[3 * p + 1] = m.y * div.y; out_rgb[3 * p + 2] = m.z * div.z;
}

void rgk_launch_tp_reproject(hipStream_t st, const DevScene& sc, uint32_t n_triangles, const DevCamera& cam, const DevCamera& prev, uint32_t xres, uint32_t yres,
                             const float* depth, const float* normal, const int32_t* tri, const float* depth_prev, const float* normal_prev, const int32_t* tri_prev,
                             const float* hist_rgb_prev, const float* hist_len_prev, float plane_tol, float normal_cos, float* hist_rgb, float* hist_len) {
    k_tp_reproject<0><<<rgk_post_pixel_grid((size_t)xres * yres), RGK_POST_BLOCK, 0, st>>>(sc, n_triangles, cam, prev, (int)xres, (int)yres, depth, normal, tri, depth_prev, normal_prev,
                                                                                       tri_prev, hist_rgb_prev, hist_len_prev, plane_tol, normal_cos, hist_rgb, hist_len);
}
void rgk_launch_tp_blend(hipStream_t st, size_t P, const float* accum_rgb, const uint32_t* accum_count, const float* albedo, const float* hist_rgb, const float* hist_len,
                         float alpha_min, float max_len, uint32_t demodulate, float albedo_floor, float* out_hist_rgb, float* out_hist_len, float* out_rgb) {
    k_tp_blend<0><<<rgk_post_pixel_grid(P), RGK_POST_BLOCK, 0, st>>>(P, accum_rgb, accum_count, albedo, hist_rgb, hist_len, alpha_min, max_len, demodulate, albedo_floor,
                                                                 out_hist_rgb, out_hist_len, out_rgb);
}

// ------------------------------------------------------------------ feature planes through delta chains (rgk.h rgk_render_aov_chain_device)
// One hop of the chain: a lane per entry of hop k's queue.  The entry is the ray the walker has just traced (A / B as every ray
// queue, the pixel's slot in B.w) and its hit; per slot {T.rgb, L} -- the product of the delta weights and the length of the chain
// so far -- in one float4 plane, implicit {1, 1, 1 | 0} at hop 0.  A lane either writes its pixel's planes (miss, dropped vertex,
// terminal vertex) or appends the ray the integrator would continue with to hop k + 1's queue: wave ballot + prefix, the four
// waves add up through LDS, one atomic per workgroup on counters[RGK_CNT_QUEUE + k + 1] (written out here: the shared
// block_append of rgk_shade.h is sized for another workgroup).  Every output is indexed by the slot, so the order of the queue
// does not show in the planes.
// The three delta kinds are sampled with the statements bxdf_sample (rgk_device.h) runs for them at u = U = (0x1.fffffep-1f, 0);
// the LTC and diffuse cases are not in this kernel.  (A template for the reason k_tp_reproject is one.)
__device__ __forceinline__ bool aov_is_delta(uint32_t kind) { return kind == RGK_BXDF_MIRROR || kind == RGK_BXDF_DIELECTRIC || kind == RGK_BXDF_TRANSPARENT; }
__device__ __forceinline__ void aov_delta_sample(const DevScene& sc, const DevMaterial& m, f3 Vi, float2 uv, f3& dir, f3& weight, bool& may_leak) {
    may_leak = false;
    if (m.kind == RGK_BXDF_MIRROR) {
        dir = mk3(-Vi.x, -Vi.y, Vi.z);
        weight = tex_get(sc, m.t_color, uv);
    } else if (m.kind == RGK_BXDF_DIELECTRIC) {
        float eta = (Vi.z < 0) ? m.ior : (float)(1.0 / (double)m.ior);
        float R, cosT;
        fresnel_dielectric(eta, fabsf(Vi.z), R, cosT);
        weight = tex_get(sc, m.t_color, uv);
        float ux = 0x1.fffffep-1f;
        if (decide_and_rescale(ux, R)) { dir = mk3(-Vi.x, -Vi.y, Vi.z); return; }
        cosT = fabsf(cosT);
        dir = mk3(-Vi.x * eta, -Vi.y * eta, (Vi.z > 0) ? -cosT : cosT);
        may_leak = true;
    } else { // RGK_BXDF_TRANSPARENT
        dir = mk3(-Vi.x, -Vi.y, -Vi.z);
        weight = mk3(1.f, 1.f, 1.f);
        may_leak = true;
    }
}

template <int = 0>
__global__ __launch_bounds__(256) void k_aov_hop(const DevScene sc, float bumpmap_scale, uint32_t xres, const uint32_t* __restrict__ pix_xy, uint32_t n, uint32_t hop,
                                                  uint32_t max_hops, const float4* __restrict__ rayA, const float4* __restrict__ rayB, const float4* __restrict__ hit,
                                                  float4* __restrict__ state, float4* __restrict__ nextA, float4* __restrict__ nextB, uint32_t* __restrict__ counters,
                                                  float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ depth, int32_t* __restrict__ tri_out,
                                                  uint8_t* __restrict__ hops_out) {
    __shared__ uint32_t s_cnt[4];
    __shared__ uint32_t s_base;
    lut_lds_fill(sc);
    // (a queue never holds more entries than the call has pixels -- an entry leaves at most one -- and every plane here has n elements)
    const uint32_t queued = counters[RGK_CNT_QUEUE + hop], count = queued < n ? queued : n;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // workgroup-uniform trip count (the compaction synchronises the workgroup)
    for (uint32_t base = blockIdx.x * 256u; base < count; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        bool cont = false;
        float4 nA = make_float4(0, 0, 0, 0), nB = nA, nS = nA;
        uint32_t slot = 0;
        if (i < count) {
            const float4 a = rayA[i], b = rayB[i], h = hit[i];
            slot = __float_as_uint(b.w);
            if (slot < n) { // (always: raygen numbered the slots 0 .. n - 1)
                const uint32_t pix = pix_xy[slot];
                const size_t p = (size_t)(pix >> 16) * xres + (pix & 0xffffu);
                f3 T = mk3(1.f, 1.f, 1.f);
                float L = 0.f;
                if (hop) { const float4 s = state[slot]; T = mk3(s.x, s.y, s.z); L = s.w; }
                const int tri = __float_as_int(h.w);
                f3 nrm = mk3(0.f, 0.f, 0.f), alb = nrm;
                float z = 0.f;
                if (tri >= 0) {
                    Vertex v;
                    surface_point(sc, bumpmap_scale, mk3(a.x, a.y, a.z), mk3(a.w, b.x, b.y), h, v);
                    z = L + h.x;
                    if (v.ok) {
                        if (aov_is_delta(v.mat.kind) && hop < max_hops) {
                            f3 dirL, weight; bool may_leak;
                            aov_delta_sample(sc, v.mat, v.VrL, v.uv, dirL, weight, may_leak);
                            const f3 dir = qrot(qinverse(v.g2l), dirL);
                            if (!(!(dot3(dir, v.faceN) * dot3(v.Vr, v.faceN) > 0) && !may_leak)) { // the integrator's leak rule (path_step, rgk_shade.h)
                                cont = true;
                                T = T * weight;
                                const f3 no = v.pos + v.faceN * sc.epsilon * 10.0f * (dirL.z < 0 ? -1.0f : 1.0f);
                                const f3 nd = norm3(norm3(dir));
                                nA = make_float4(no.x, no.y, no.z, nd.x);
                                nB = make_float4(nd.y, nd.z, __int_as_float(tri), __uint_as_float(slot));
                                nS = make_float4(T.x, T.y, T.z, z);
                            }
                        }
                        if (!cont) {
                            nrm = v.lightN;
                            alb = T * albedo_of(sc, v.mat, v.uv);
                        }
                    }
                }
                if (!cont) {
                    if (tri_out) tri_out[p] = tri < 0 ? -1 : tri;
                    if (depth) depth[p] = z;
                    if (normal) { normal[3 * p] = nrm.x; normal[3 * p + 1] = nrm.y; normal[3 * p + 2] = nrm.z; }
                    if (albedo) { albedo[3 * p] = alb.x; albedo[3 * p + 1] = alb.y; albedo[3 * p + 2] = alb.z; }
                    if (hops_out) hops_out[p] = (uint8_t)hop;
                }
            }
        }
        const unsigned long long m = __ballot(cont);
        if (lane == 0) s_cnt[w] = __popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int k = 0; k < 4; k++) { const uint32_t c = s_cnt[k]; s_cnt[k] = t; t += c; }
            s_base = t ? atomicAdd(&counters[RGK_CNT_QUEUE + hop + 1], t) : 0u;
        }
        __syncthreads();
        if (cont) {
            const uint32_t q = s_base + s_cnt[w] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (q < n) { // (always: see `count`)
                nextA[q] = nA; nextB[q] = nB;
                state[slot] = nS;
            }
        }
        __syncthreads(); // s_cnt / s_base are rewritten by the next trip
    }
}

void rgk_launch_aov_hop(hipStream_t st, const DevScene& sc, float bumpmap_scale, uint32_t xres, const uint32_t* pix_xy, uint32_t n, uint32_t hop, uint32_t max_hops,
                        const float4* rayA, const float4* rayB, const float4* hit, float4* state, float4* nextA, float4* nextB, uint32_t* counters, float* albedo,
                        float* normal, float* depth, int32_t* tri, uint8_t* hops) {
    k_aov_hop<0><<<rgk_aov_hop_grid(n), 256, RGK_LDS_SHADE_BYTES, st>>>(sc, bumpmap_scale, xres, pix_xy, n, hop, max_hops, rayA, rayB, hit, state, nextA, nextB, counters, albedo,
                                                                        normal, depth, tri, hops);
}

// ------------------------------------------------------------------ guided upsampling (rgk.h rgk_upsample_device)
// A low-resolution accumulator reconstructed on a finer grid, guided by the feature planes of both grids; every formula in rgk.h's
// order, float32, nothing contracted (tests/upsample_ref.py gives the same bits).  (Templates for the reason k_tp_reproject is one.)
//   k_us_prepare   a lane per LOW pixel: three 16-byte records in three planes of `rec` -- [q] {m.rgb, flags: 1 live, 2 flat},
//                  [Pl + q] {x_q.xyz, 0}, [2 Pl + q] {n_q.xyz, 0} -- so a tap is up to three dwordx4 loads (the flags decide whether
//                  the other two are needed) and x_q, its camera ray included, is formed once per low pixel instead of once per tap.
//                  Reads 32 B (44 with the albedo), writes 48 B per low pixel.
//   k_us_gather    a lane per FULL pixel, a workgroup per RGK_POST_BX x RGK_POST_BY tile: at ratio 4 its ring-1 taps lie in a 9 x 3
//                  patch of the low grid, ring 2 in 11 x 5, i.e. a few cache lines per record plane.  Reads its own 16 B (28 with
//                  the albedo), writes 12 B + 1 B.  Ring 2 is a branch: a wave none of whose lanes needs it skips it.
constexpr uint32_t RGK_US_LIVE = 1u, RGK_US_FLAT = 2u;

template <int = 0>
__global__ __launch_bounds__(RGK_POST_BLOCK) void k_us_prepare(const DevCamera low, int xl, int yl, const float* __restrict__ accum_rgb,
                                                                const uint32_t* __restrict__ accum_count, const float* __restrict__ albedo,
                                                                const float* __restrict__ normal, const float* __restrict__ depth, uint32_t demodulate,
                                                                float albedo_floor, float4* __restrict__ rec) {
    const size_t Pl = (size_t)xl * (size_t)yl;
    const size_t q = (size_t)blockIdx.x * RGK_POST_BLOCK + threadIdx.x;
    if (q >= Pl) return;
    const int y = (int)(q / (size_t)xl), x = (int)(q - (size_t)y * (size_t)xl);
    const uint32_t n = accum_count[q];
    f3 c = mk3(0.f, 0.f, 0.f);
    if (n) c = ld3(accum_rgb, q) / (float)n;
    f3 div = mk3(1.f, 1.f, 1.f);
    if (demodulate) div = mk3(demod_div(albedo[3 * q], albedo_floor), demod_div(albedo[3 * q + 1], albedo_floor), demod_div(albedo[3 * q + 2], albedo_floor));
    const f3 nq = ld3(normal, q);
    f3 o, d; // (lens_size == 0: the host passes a pinhole copy)
    camera_ray(low, x, y, xl, yl, make_float2(0.5f, 0.5f), make_float2(0.f, 0.f), o, d);
    const f3 xq = o + d * depth[q];
    const uint32_t flags = (n ? RGK_US_LIVE : 0u) | (is_zero3(nq) ? RGK_US_FLAT : 0u);
    rec[q] = make_float4(c.x / div.x, c.y / div.y, c.z / div.z, __uint_as_float(flags));
    rec[Pl + q] = make_float4(xq.x, xq.y, xq.z, 0.f);
    rec[2 * Pl + q] = make_float4(nq.x, nq.y, nq.z, 0.f);
}

// One tap of either ring: adds w * m_q to (A, W) when q counts.
struct UsPixel { f3 xp, np; float tol, normal_cos; bool flat; };
__device__ __forceinline__ void us_tap(const UsPixel& px, const float4* __restrict__ rec, size_t Pl, int xl, int yl, int qx, int qy, float w, f3& A, float& W) {
    if (qx < 0 || qx >= xl || qy < 0 || qy >= yl) return;
    const size_t qi = (size_t)qy * (size_t)xl + (size_t)qx;
    const float4 r0 = rec[qi];
    const uint32_t flags = __float_as_uint(r0.w);
    if (!(flags & RGK_US_LIVE) || ((flags & RGK_US_FLAT) != 0u) != px.flat) return;
    if (!px.flat) {
        const float4 rn = rec[2 * Pl + qi];
        if (!(dot3(px.np, mk3(rn.x, rn.y, rn.z)) >= px.normal_cos)) return;
        const float4 rx = rec[Pl + qi];
        if (!(fabsf(dot3(mk3(rx.x, rx.y, rx.z) - px.xp, px.np)) <= px.tol)) return;
    }
    W = W + w;
    A = mk3(A.x + w * r0.x, A.y + w * r0.y, A.z + w * r0.z);
}

template <int = 0>
__global__ __launch_bounds__(RGK_POST_BX * RGK_POST_BY) void k_us_gather(const DevCamera cam, const DevCamera low, int xres, int yres, int xl, int yl,
                                                                         const float* __restrict__ albedo, const float* __restrict__ normal,
                                                                         const float* __restrict__ depth, const float* __restrict__ low_rgb,
                                                                         const uint32_t* __restrict__ low_count, const float4* __restrict__ rec, float plane_tol,
                                                                         float normal_cos, uint32_t demodulate, float albedo_floor, float* __restrict__ out_rgb,
                                                                         uint8_t* __restrict__ out_support) {
    const int x = (int)(blockIdx.x * RGK_POST_BX + threadIdx.x % RGK_POST_BX), y = (int)(blockIdx.y * RGK_POST_BY + threadIdx.x / RGK_POST_BX);
    if (x >= xres || y >= yres) return;
    const size_t p = (size_t)y * (size_t)xres + (size_t)x, Pl = (size_t)xl * (size_t)yl;
    f3 o, d; // (lens_size == 0 in both cameras: the host passes pinhole copies)
    camera_ray(cam, x, y, xres, yres, make_float2(0.5f, 0.5f), make_float2(0.f, 0.f), o, d);
    UsPixel px;
    px.np = ld3(normal, p);
    px.flat = is_zero3(px.np);
    px.xp = o + d * depth[p];
    px.normal_cos = normal_cos;
    const f3 o_low = mk3(low.origin[0], low.origin[1], low.origin[2]);
    const f3 v = px.flat ? d : px.xp - o_low;
    const f3 N = mk3(low.direction[0], low.direction[1], low.direction[2]);
    const float qd = dot3(v, N);
    f3 out = mk3(0.f, 0.f, 0.f);
    uint32_t support = 0;
    if (qd > 0.0f) {
        const f3 vs = mk3(low.viewscreen[0], low.viewscreen[1], low.viewscreen[2]);
        const f3 vx = mk3(low.viewscreen_x[0], low.viewscreen_x[1], low.viewscreen_x[2]);
        const f3 vy = mk3(low.viewscreen_y[0], low.viewscreen_y[1], low.viewscreen_y[2]);
        const float s = dot3(vs - o_low, N) / qd;
        const f3 w = (o_low + v * s) - vs;
        const float a = dot3(w, vx) / dot3(vx, vx), b = dot3(w, vy) / dot3(vy, vy);
        const float fx = a * (float)xl - 0.5f, fy = b * (float)yl - 0.5f;
        if (fx > -2.0f && fx < (float)(xl + 1) && fy > -2.0f && fy < (float)(yl + 1)) { // (false for NaN)
            const float flx = floorf(fx), fly = floorf(fy);
            const int ix = (int)flx, iy = (int)fly;
            const float tx = fx - flx, ty = fy - fly;
            px.tol = plane_tol * len3(px.xp - o);
            f3 A = mk3(0.f, 0.f, 0.f);
            float W = 0.f;
            const float wt[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
#pragma unroll
            for (int k = 0; k < 4; k++) us_tap(px, rec, Pl, xl, yl, ix + (k & 1), iy + (k >> 1), wt[k], A, W);
            support = 1;
            if (!(W > 0.0f)) { // ring 2: only where ring 1 found nothing
                A = mk3(0.f, 0.f, 0.f);
                W = 0.f;
                for (int dy = -1; dy <= 2; dy++)
                    for (int dx = -1; dx <= 2; dx++) {
                        const int qx = ix + dx, qy = iy + dy;
                        const float ex = fx - (float)qx, ey = fy - (float)qy;
                        us_tap(px, rec, Pl, xl, yl, qx, qy, 1.0f / (1.0f + (ex * ex + ey * ey)), A, W);
                    }
                support = 2;
            }
            if (W > 0.0f) {
                f3 div = mk3(1.f, 1.f, 1.f);
                if (demodulate) div = mk3(demod_div(albedo[3 * p], albedo_floor), demod_div(albedo[3 * p + 1], albedo_floor), demod_div(albedo[3 * p + 2], albedo_floor));
                out = mk3((A.x / W) * div.x, (A.y / W) * div.y, (A.z / W) * div.z);
            } else { // nearest: the plain image of the closest low pixel
                support = 0;
                const int nx = min(max((int)floorf(fx + 0.5f), 0), xl - 1), ny = min(max((int)floorf(fy + 0.5f), 0), yl - 1);
                const size_t q0 = (size_t)ny * (size_t)xl + (size_t)nx;
                const uint32_t n0 = low_count[q0];
                if (n0) out = ld3(low_rgb, q0) / (float)n0;
            }
        }
    }
    out_rgb[3 * p] = out.x; out_rgb[3 * p + 1] = out.y; out_rgb[3 * p + 2] = out.z;
    if (out_support) out_support[p] = (uint8_t)support;
}

void rgk_launch_us_prepare(hipStream_t st, const DevCamera& low, uint32_t xl, uint32_t yl, const float* accum_rgb, const uint32_t* accum_count, const float* albedo,
                           const float* normal, const float* depth, uint32_t demodulate, float albedo_floor, float4* rec) {
    k_us_prepare<0><<<rgk_post_pixel_grid((size_t)xl * yl), RGK_POST_BLOCK, 0, st>>>(low, (int)xl, (int)yl, accum_rgb, accum_count, albedo, normal, depth, demodulate, albedo_floor, rec);
}
void rgk_launch_us_gather(hipStream_t st, const DevCamera& cam, const DevCamera& low, uint32_t xres, uint32_t yres, uint32_t xl, uint32_t yl, const float* albedo,
                          const float* normal, const float* depth, const float* low_rgb, const uint32_t* low_count, const float4* rec, float plane_tol, float normal_cos,
                          uint32_t demodulate, float albedo_floor, float* out_rgb, uint8_t* out_support) {
    const RgkGrid2 g = rgk_post_filter_grid(xres, yres);
    k_us_gather<0><<<dim3(g.x, g.y), RGK_POST_BX * RGK_POST_BY, 0, st>>>(cam, low, (int)xres, (int)yres, (int)xl, (int)yl, albedo, normal, depth, low_rgb, low_count, rec,
                                                                         plane_tol, normal_cos, demodulate, albedo_floor, out_rgb, out_support);
}

// ------------------------------------------------------------------ per-sample demodulated accumulation (rgk.h rgk_render_round_demod_device)
// Beside the accumulator S = sum of L_s a demodulated round keeps D = sum of L_s / div_s and A = sum of div_s, div_s the albedo at the
// first hit of sample s's OWN camera ray (jitter and lens included) through the floor rule of demod_div.  No shading kernel or walker
// takes part: at bounce 0 hit[] is indexed by path slot -- every walker writes the record of every slot below npix * ns, misses
// included (k_trace_camera at the lane's retirement, k_trace_camera_beam when it sets the sample up), which k_shade<FIRST> relies on
// as well -- camera_ray_of_slot re-derives the ray from the slot number, and tot[slot] holds the finished sample until the resolve.
//   k_demod_divisor  a lane per slot (a bounded grid of 256-lane workgroups striding over the slots), behind bounce 0's walk and before its shading (later bounces index hit[] by queue position):
//                    surface_point() + albedo_of() as k_aov_gather has them -> div[slot] = {div.rgb, 0}.  Reads 16 B, writes 16 B per path.
//   k_resolve_demod  behind k_resolve, over the same pass: per pixel, in sample order, Dsum += v_s / div_s and Asum += div_s with v_s
//                    the value resolve_add adds (resolve_value, rgk_device.h: the clamp comes before the division); carried across
//                    sample passes in pixsum2[2 * pixel] / [2 * pixel + 1]; added to the two planes with the pixel's last sample.
//                    gshift > 0: the sample blocks of tot and div are staged through LDS as k_resolve_tiled stages tot.
//   k_remodulate     a lane per pixel: out = in * dbar, dbar = A / n (1 where n == 0) or the floor rule of an albedo plane.
// Float32, + * / max only, nothing contracted, sums in sample order: tests/demod_ref.py gives the same bits.
// (Templates for the reason k_tp_reproject is one; last in the file, so every earlier kernel keeps its text.)
template <int = 0>
__global__ __launch_bounds__(256) void k_demod_divisor(const DevScene sc, const DevCamera cam, const PassParams pp, const float4* __restrict__ hit, float albedo_floor,
                                                        float4* __restrict__ div) {
    lut_lds_fill(sc); // (a barrier: before any lane leaves; once per workgroup, which is why the grid is bounded and the lanes stride)
    const uint32_t n = pp.npix * pp.ns;
    for (uint32_t slot = blockIdx.x * 256u + threadIdx.x; slot < n; slot += gridDim.x * 256u) {
        const float4 h = hit[slot];
        f3 dv = mk3(1.f, 1.f, 1.f);
        if (__float_as_int(h.w) >= 0) {
            f3 o, d;
            camera_ray_of_slot(cam, pp, slot, o, d);
            Vertex v;
            surface_point(sc, pp.bumpmap_scale, o, d, h, v);
            if (v.ok) {
                const f3 a = albedo_of(sc, v.mat, v.uv);
                dv = mk3(demod_div(a.x, albedo_floor), demod_div(a.y, albedo_floor), demod_div(a.z, albedo_floor));
            }
        }
        div[slot] = make_float4(dv.x, dv.y, dv.z, 0.f);
    }
}

__device__ __forceinline__ void demod_add(float4& D, float4& A, float4 t, float4 dv, float clamp) {
    const f3 v = resolve_value(t, clamp);
    D.x = D.x + v.x / dv.x; D.y = D.y + v.y / dv.y; D.z = D.z + v.z / dv.z;
    A.x = A.x + dv.x; A.y = A.y + dv.y; A.z = A.z + dv.z;
}
// One wave per PT <= 64 pixels, lane p owns pixel p.  gshift == 0: consecutive lanes read consecutive slots, nothing to stage.
template <int = 0>
__global__ __launch_bounds__(64) void k_resolve_demod(const PassParams pp, const float4* __restrict__ tot, const float4* __restrict__ div, float4* __restrict__ pixsum2,
                                                       float* __restrict__ demod_rgb, float* __restrict__ div_rgb, const uint32_t PT) {
    extern __shared__ float4 tile[]; // gshift > 0: [2][PT pixels][G + 1] -- tot, then div
    const uint32_t G = 1u << pp.gshift, lane = threadIdx.x;
    for (uint32_t jb = blockIdx.x * PT; jb < pp.npix; jb += gridDim.x * PT) {
        const uint32_t np = min(PT, pp.npix - jb), j = jb + lane;
        float4 D = make_float4(0.f, 0.f, 0.f, 0.f), A = D;
        if (lane < np && pp.s0 != 0) { D = pixsum2[2 * (size_t)(pp.j0 + j)]; A = pixsum2[2 * (size_t)(pp.j0 + j) + 1]; }
        if (pp.gshift == 0) {
            if (lane < np)
                for (uint32_t srel = 0; srel < pp.ns; srel++) {
                    const size_t slot = (size_t)srel * pp.npix + j; // slot_of at gshift 0
                    demod_add(D, A, tot[slot], div[slot], pp.clamp);
                }
        } else {
            float4* const tile_d = tile + PT * (G + 1u);
            for (uint32_t sb = 0; sb < (pp.ns >> pp.gshift); sb++) {
                const size_t base = (size_t)(sb * pp.npix + jb) << pp.gshift; // np * G consecutive slots
                for (uint32_t k = 0; k * 64u < np * G; k++) {
                    const uint32_t idx = k * 64u + lane;
                    if (idx < np * G) {
                        const uint32_t at = (idx >> pp.gshift) * (G + 1u) + (idx & (G - 1u));
                        tile[at] = tot[base + idx];
                        tile_d[at] = div[base + idx];
                    }
                }
                __syncthreads();
                if (lane < np)
                    for (uint32_t g = 0; g < G; g++) demod_add(D, A, tile[lane * (G + 1u) + g], tile_d[lane * (G + 1u) + g], pp.clamp);
                __syncthreads();
            }
        }
        if (lane < np) {
            if (pp.s0 + pp.ns >= pp.multisample) {
                const uint32_t pix = pp.pix_xy[pp.j0 + j];
                const size_t p = (size_t)(pix >> 16) * pp.xres + (pix & 0xffffu);
                demod_rgb[3 * p] += D.x; demod_rgb[3 * p + 1] += D.y; demod_rgb[3 * p + 2] += D.z;
                div_rgb[3 * p] += A.x; div_rgb[3 * p + 1] += A.y; div_rgb[3 * p + 2] += A.z;
            } else {
                pixsum2[2 * (size_t)(pp.j0 + j)] = D;
                pixsum2[2 * (size_t)(pp.j0 + j) + 1] = A;
            }
        }
    }
}

template <int = 0>
__global__ __launch_bounds__(RGK_POST_BLOCK) void k_remodulate(size_t P, const float* __restrict__ in_rgb, const float* __restrict__ div_rgb,
                                                                const uint32_t* __restrict__ div_count, float albedo_floor, float* __restrict__ out_rgb) {
    const size_t p = (size_t)blockIdx.x * RGK_POST_BLOCK + threadIdx.x;
    if (p >= P) return;
    f3 dbar = mk3(1.f, 1.f, 1.f);
    const f3 a = ld3(div_rgb, p);
    if (div_count) {
        const uint32_t n = div_count[p];
        if (n) dbar = a / (float)n;
    } else dbar = mk3(demod_div(a.x, albedo_floor), demod_div(a.y, albedo_floor), demod_div(a.z, albedo_floor));
    const f3 c = ld3(in_rgb, p);
    out_rgb[3 * p] = c.x * dbar.x; out_rgb[3 * p + 1] = c.y * dbar.y; out_rgb[3 * p + 2] = c.z * dbar.z;
}

void rgk_launch_demod_divisor(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, const float4* hit, float albedo_floor, float4* div) {
    k_demod_divisor<0><<<rgk_demod_divisor_grid(pp.npix * pp.ns), 256, RGK_LDS_SHADE_BYTES, st>>>(sc, cam, pp, hit, albedo_floor, div);
}
void rgk_launch_resolve_demod(hipStream_t st, const PassParams& pp, const float4* tot, const float4* div, float4* pixsum2, float* demod_rgb, float* div_rgb) {
    const RgkResolvePlan r = rgk_resolve_demod_plan(pp.npix, pp.gshift);
    k_resolve_demod<0><<<r.grid, 64, r.lds, st>>>(pp, tot, div, pixsum2, demod_rgb, div_rgb, r.PT);
}
void rgk_launch_remodulate(hipStream_t st, size_t P, const float* in_rgb, const float* div_rgb, const uint32_t* div_count, float albedo_floor, float* out_rgb) {
    k_remodulate<0><<<rgk_post_pixel_grid(P), RGK_POST_BLOCK, 0, st>>>(P, in_rgb, div_rgb, div_count, albedo_floor, out_rgb);
}

// ------------------------------------------------------------------ display output (rgk.h rgk_display_measure_device / rgk_display_encode_device)
// From radiance to 8-bit sRGB: a luminance histogram for the exposure, then exposure, tone curve and transfer function per pixel.
// The arithmetic is rgk_display.h's, which the host and the CPU harness include too; float32, + - * / min max and comparisons,
// nothing contracted, no transcendental function (tests/display_ref.py gives the same bits).
//   k_display_hist    a bounded grid of 256-lane workgroups striding over the frame (rgk_plan.h: one per CU).  A per-workgroup histogram in LDS (256 bins
//                     and the dark count), integer LDS adds, then one integer add per non-empty bin per workgroup into the scene's
//                     histogram, which the host cleared on the stream: integers only, so the order of the adds does not matter.
//                     Reads 16 B per pixel (12 without a count plane).
//   k_display_encode  the same striding; the table T in 1 KB of LDS, filled once per workgroup; per channel the curve and the
//                     8-step search of rgk_display_byte in T.  Reads 16 B, writes 4 B per pixel.
// VEC: a lane takes four consecutive pixels at a time -- three 16-byte loads of the rgb plane, one of the counts, and for the
// encode one 16-byte store -- when every plane's base is 16-byte aligned; the frame's last P % 4 pixels, and every pixel of a
// frame whose planes are not aligned, are taken one per lane.  An item is a group of four or one such pixel.
// (Templates for the reason k_tp_reproject is one; last in the file, so every earlier kernel keeps its text.)
struct DisplayItems {
    size_t groups, items;
    __device__ DisplayItems(size_t P, bool vec) : groups(vec ? P / 4 : 0), items(groups + (P - 4 * groups)) {}
};

__device__ __forceinline__ void display_hist_add(uint32_t* s_hist, float r, float g, float b, bool counted, uint32_t n) {
    const float Y = rgk_display_lum(rgk_display_colour(r, g, b, counted, n));
    atomicAdd(&s_hist[Y > 0.0f ? rgk_display_bin(Y) : RGK_DISPLAY_BINS], 1u);
}

template <bool VEC>
__global__ __launch_bounds__(RGK_POST_BLOCK) void k_display_hist(size_t P, const float* __restrict__ rgb, const uint32_t* __restrict__ count, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[RGK_DISPLAY_HIST_WORDS];
    static_assert(RGK_POST_BLOCK == RGK_DISPLAY_BINS, "a lane per bin");
    s_hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_hist[RGK_DISPLAY_BINS] = 0;
    __syncthreads();
    const DisplayItems it(P, VEC);
    const bool counted = count != nullptr;
    for (size_t i = (size_t)blockIdx.x * RGK_POST_BLOCK + threadIdx.x; i < it.items; i += (size_t)gridDim.x * RGK_POST_BLOCK) {
        if (VEC && i < it.groups) {
            const float4* q = reinterpret_cast<const float4*>(rgb) + 3 * i;
            const float4 a = q[0], b = q[1], c = q[2];
            const uint4 n = counted ? reinterpret_cast<const uint4*>(count)[i] : make_uint4(0u, 0u, 0u, 0u);
            display_hist_add(s_hist, a.x, a.y, a.z, counted, n.x);
            display_hist_add(s_hist, a.w, b.x, b.y, counted, n.y);
            display_hist_add(s_hist, b.z, b.w, c.x, counted, n.z);
            display_hist_add(s_hist, c.y, c.z, c.w, counted, n.w);
        } else {
            const size_t p = 4 * it.groups + (i - it.groups);
            display_hist_add(s_hist, rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], counted, counted ? count[p] : 0u);
        }
    }
    __syncthreads();
    const uint32_t v = s_hist[threadIdx.x];
    if (v) atomicAdd(&hist[threadIdx.x], v);
    if (threadIdx.x == 0 && s_hist[RGK_DISPLAY_BINS]) atomicAdd(&hist[RGK_DISPLAY_BINS], s_hist[RGK_DISPLAY_BINS]);
}

__device__ __forceinline__ uint32_t display_encode_pixel(const float* s_T, float r, float g, float b, bool counted, uint32_t n, uint32_t op, float exposure, float white) {
    return rgk_display_word(s_T, rgk_display_curve(op, rgk_display_colour(r, g, b, counted, n), exposure, white));
}

template <bool VEC>
__global__ __launch_bounds__(RGK_POST_BLOCK) void k_display_encode(size_t P, const float* __restrict__ rgb, const uint32_t* __restrict__ count, const float* __restrict__ table,
                                                                    uint32_t op, float exposure, float white, uint32_t* __restrict__ out) {
    __shared__ float s_T[RGK_DISPLAY_BINS];
    static_assert(RGK_POST_BLOCK == RGK_DISPLAY_BINS, "a lane per threshold");
    s_T[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const DisplayItems it(P, VEC);
    const bool counted = count != nullptr;
    for (size_t i = (size_t)blockIdx.x * RGK_POST_BLOCK + threadIdx.x; i < it.items; i += (size_t)gridDim.x * RGK_POST_BLOCK) {
        if (VEC && i < it.groups) {
            const float4* q = reinterpret_cast<const float4*>(rgb) + 3 * i;
            const float4 a = q[0], b = q[1], c = q[2];
            const uint4 n = counted ? reinterpret_cast<const uint4*>(count)[i] : make_uint4(0u, 0u, 0u, 0u);
            uint4 w;
            w.x = display_encode_pixel(s_T, a.x, a.y, a.z, counted, n.x, op, exposure, white);
            w.y = display_encode_pixel(s_T, a.w, b.x, b.y, counted, n.y, op, exposure, white);
            w.z = display_encode_pixel(s_T, b.z, b.w, c.x, counted, n.z, op, exposure, white);
            w.w = display_encode_pixel(s_T, c.y, c.z, c.w, counted, n.w, op, exposure, white);
            reinterpret_cast<uint4*>(out)[i] = w;
        } else {
            const size_t p = 4 * it.groups + (i - it.groups);
            out[p] = display_encode_pixel(s_T, rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], counted, counted ? count[p] : 0u, op, exposure, white);
        }
    }
}

void rgk_launch_display_hist(hipStream_t st, size_t P, const float* rgb, const uint32_t* count, uint32_t* hist) {
    if (rgk_display_vec(rgb, count, nullptr)) k_display_hist<true><<<rgk_display_grid(P, true, RGK_DISPLAY_HIST_WGS), RGK_POST_BLOCK, 0, st>>>(P, rgb, count, hist);
    else k_display_hist<false><<<rgk_display_grid(P, false, RGK_DISPLAY_HIST_WGS), RGK_POST_BLOCK, 0, st>>>(P, rgb, count, hist);
}
void rgk_launch_display_encode(hipStream_t st, size_t P, const float* rgb, const uint32_t* count, const float* table, uint32_t op, float exposure, float white, uint32_t* out) {
    if (rgk_display_vec(rgb, count, out)) k_display_encode<true><<<rgk_display_grid(P, true, RGK_DISPLAY_ENCODE_WGS), RGK_POST_BLOCK, 0, st>>>(P, rgb, count, table, op, exposure, white, out);
    else k_display_encode<false><<<rgk_display_grid(P, false, RGK_DISPLAY_ENCODE_WGS), RGK_POST_BLOCK, 0, st>>>(P, rgb, count, table, op, exposure, white, out);
}
