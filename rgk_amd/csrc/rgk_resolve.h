// Resolve and the round's lists: the slot sums folded into the accumulator (K9), the pixel list and the Halton table of a round,
// the queue counters.
#pragma once
#include <hip/hip_runtime.h>
#include "rgk_device.h"
#include "rgk_kernels.h"

// ------------------------------------------------------------------ K9: resolve
// final clamp + NaN/negative scrub (path_tracer.cpp:502-507), per-pixel sum over the pass's
// samples in sample order (RenderPixel :64), then AddPixel when the pixel's last sample is in.
__device__ __forceinline__ float4 resolve_add(float4 acc, float4 t, float clamp) {
    const f3 v = resolve_value(t, clamp);
    acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z;
    return acc;
}
// AddPixel: a pixel's finished sum of n samples into the accumulator
__device__ __forceinline__ void add_pixel(uint32_t pix, uint32_t xres, float4 acc, uint32_t n, float* accum_rgb, uint32_t* accum_count) {
    size_t p = (size_t)(pix >> 16) * xres + (pix & 0xffff);
    accum_rgb[3 * p + 0] += acc.x;
    accum_rgb[3 * p + 1] += acc.y;
    accum_rgb[3 * p + 2] += acc.z;
    accum_count[p] += n;
}
__global__ __launch_bounds__(256) void k_resolve(const PassParams pp, const float4* __restrict__ tot, float4* __restrict__ pixsum,
                                                  float* __restrict__ accum_rgb, uint32_t* __restrict__ accum_count) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < pp.npix; j += gridDim.x * blockDim.x) {
        float4 acc = (pp.s0 == 0) ? make_float4(0.f, 0.f, 0.f, 0.f) : pixsum[pp.j0 + j];
        for (uint32_t srel = 0; srel < pp.ns; srel++) {
            float4 t = tot[slot_of(pp, j, srel)];
            acc = resolve_add(acc, t, pp.clamp);
        }
        if (pp.s0 + pp.ns >= pp.multisample) add_pixel(pp.pix_xy[pp.j0 + j], pp.xres, acc, pp.multisample, accum_rgb, accum_count);
        else pixsum[pp.j0 + j] = acc;
    }
}

// The same for gshift > 0, where the 2^g samples of a pixel are contiguous (a thread walking its pixel's samples would stride
// 2^g * 16 bytes against its neighbours): one wave per PT pixels stages each sample block through LDS with coalesced loads, then
// lane p sums pixel p's samples in sample order -- the same additions in the same order as above.
__global__ __launch_bounds__(64) void k_resolve_tiled(const PassParams pp, const float4* __restrict__ tot, float4* __restrict__ pixsum,
                                                       float* __restrict__ accum_rgb, uint32_t* __restrict__ accum_count, const uint32_t PT) {
    extern __shared__ float4 tile[]; // [PT pixels][G + 1], PT <= 64
    const uint32_t G = 1u << pp.gshift, lane = threadIdx.x;
    for (uint32_t jb = blockIdx.x * PT; jb < pp.npix; jb += gridDim.x * PT) {
        const uint32_t np = min(PT, pp.npix - jb), j = jb + lane;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < np && pp.s0 != 0) acc = pixsum[pp.j0 + j];
        for (uint32_t sb = 0; sb < (pp.ns >> pp.gshift); sb++) {
            const float4* __restrict__ src = tot + ((size_t)(sb * pp.npix + jb) << pp.gshift); // np * G consecutive slots
            for (uint32_t k = 0; k * 64u < np * G; k++) {
                const uint32_t idx = k * 64u + lane;
                if (idx < np * G) tile[(idx >> pp.gshift) * (G + 1u) + (idx & (G - 1u))] = src[idx];
            }
            __syncthreads();
            if (lane < np)
                for (uint32_t g = 0; g < G; g++) {
                    const float4 t = tile[lane * (G + 1u) + g];
                    acc = resolve_add(acc, t, pp.clamp);
                }
            __syncthreads();
        }
        if (lane < np) {
            if (pp.s0 + pp.ns >= pp.multisample) add_pixel(pp.pix_xy[pp.j0 + j], pp.xres, acc, pp.multisample, accum_rgb, accum_count);
            else pixsum[pp.j0 + j] = acc;
        }
    }
}

// The round's pixel list in Tracer::Render order with the per-pixel seeds (a1, a2), built on the device from the tile list
// (2040 tiles at 1080p: a few KB up instead of 16 MB of host-built lists every round).  The seed of a pixel is fixed by its
// row-major rank k inside the task (RenderPixel is called in that order, tracer.cpp:8-9, and bumps the seed first,
// path_tracer.cpp:47).  The ORDER in which pixels occupy path slots is free: 8x8 blocks, so the 64 lanes of a wave start as
// a compact bundle of camera rays instead of two 32-pixel row segments (coherent traversal and shading).
__global__ __launch_bounds__(256) void k_build_pixel_list(const rgk_tile* __restrict__ tiles, const uint32_t* __restrict__ tile_off, uint32_t n_tiles,
                                                           uint32_t* __restrict__ pix_xy, uint32_t* __restrict__ pix_seed) {
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const rgk_tile tl = tiles[t];
        const uint32_t tw = tl.x1 - tl.x0, th = tl.y1 - tl.y0, base = tile_off[t];
        for (uint32_t q = threadIdx.x; q < tw * th; q += blockDim.x) {
            // slot q of the tile in 8x8-block order -> (x, y) inside the tile
            const uint32_t nbr = (th + 7u) >> 3, nbc = (tw + 7u) >> 3;
            uint32_t r = q / (8u * tw);
            if (r > nbr - 1u) r = nbr - 1u;
            const uint32_t rem = q - r * 8u * tw;
            const uint32_t bh = (th - 8u * r) < 8u ? (th - 8u * r) : 8u;
            uint32_t c = rem / (bh * 8u);
            if (c > nbc - 1u) c = nbc - 1u;
            const uint32_t rem2 = rem - c * bh * 8u;
            const uint32_t bw = (tw - 8u * c) < 8u ? (tw - 8u * c) : 8u;
            const uint32_t y = 8u * r + rem2 / bw, x = 8u * c + rem2 % bw; // (Z order inside the block: no difference measured)
            const uint32_t k = y * tw + x;
            pix_xy[base + q] = (tl.x0 + x) | ((tl.y0 + y) << 16);
            pix_seed[base + q] = tl.seed + (k + 1u) * 0x42424242u;
        }
    }
}

// halton_raw tabulated once per round: htab[hdim * S + s]
__global__ void k_build_halton_table(const DevScene sc, uint32_t S, float* __restrict__ htab) {
    const uint32_t n = 192u * S;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t hdim = i / S, s = i - hdim * S;
        htab[i] = halton_raw(sc, hdim, s);
    }
}

__global__ void k_init_counters(uint32_t* counters, uint32_t n0) {
    for (uint32_t i = threadIdx.x; i < RGK_CNT_TOTAL; i += blockDim.x) counters[i] = (i == RGK_CNT_QUEUE) ? n0 : 0u;
}
