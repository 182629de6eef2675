// The device side of the output path (rgk.h rgk_output_write_exr_device / rgk_output_write_png_device): the bytes of an EXR's
// pixel-data region and of a PNG's IDAT payload, and the pieces of the PNG's two checksums, made where the image is.  The
// arithmetic is rgk_pack.h's, shared with the host; every byte equals what rgk_output.cpp's host writers produce.
//   k_out_max        accumulator -> per-workgroup maxima of data / count (rgk_pack_max: no float atomics)
//   k_out_max_fold   one workgroup: the maxima -> the scale 1 / max
//   k_out_pack_exr   per line {y, 8 * xres, A, B, G, R planes of halves}; a workgroup is 512 consecutive x of one line, a lane two
//                    adjacent pixels, so a wave's store per plane is 256 contiguous bytes.  Even xres: every plane is 4-byte aligned
//                    and a lane stores one dword per plane; odd xres: planes B and R sit 2 bytes off, and lanes store halves.
//   k_out_pack_png   a lane makes four consecutive payload bytes, each by rgk_pack_png_payload_byte -- zlib header, stored-block
//                    headers and raw bytes alike, so the handful of header bytes belong to whichever lane covers them -- and stores
//                    one dword; the last dword's bytes behind the payload are zeros
//   k_out_png_sums   a lane per piece of RGK_PACK_SEGMENT bytes: the Adler lanes read the raw stream back from the payload, the CRC
//                    lanes the payload behind the chunk type; the CRC table is built in LDS by the workgroup's 256 lanes
// Every byte of the regions the host copies is written: nothing depends on what the buffer held (RGK_POISON).
#include <hip/hip_runtime.h>

#include "rgk_kernels.h"
#include "rgk_pack.h"

namespace {
constexpr int OUT_BLOCK = 256;

// the workgroup's maximum into lane 0 (every lane calls)
__device__ float block_max(float m, float* lds) {
    lds[threadIdx.x] = m;
    __syncthreads();
    for (int step = OUT_BLOCK / 2; step; step >>= 1) {
        if ((int)threadIdx.x < step) lds[threadIdx.x] = rgk_pack_max(lds[threadIdx.x], lds[threadIdx.x + step]);
        __syncthreads();
    }
    return lds[0];
}

__global__ __launch_bounds__(OUT_BLOCK) void k_out_max(size_t P, const float* __restrict__ rgb, const uint32_t* __restrict__ count, float* __restrict__ partial) {
    __shared__ float lds[OUT_BLOCK];
    float m = 0.0f;
    for (size_t p = (size_t)blockIdx.x * OUT_BLOCK + threadIdx.x; p < P; p += (size_t)gridDim.x * OUT_BLOCK)
        m = rgk_pack_max_pixel(m, rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], count[p]);
    m = block_max(m, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

__global__ __launch_bounds__(OUT_BLOCK) void k_out_max_fold(uint32_t n, const float* __restrict__ partial, float* __restrict__ val) {
    __shared__ float lds[OUT_BLOCK];
    float m = 0.0f;
    for (uint32_t i = threadIdx.x; i < n; i += OUT_BLOCK) m = rgk_pack_max(m, partial[i]);
    m = block_max(m, lds);
    if (threadIdx.x == 0) *val = rgk_pack_scale_of_max(m);
}

template <bool ACCUM>
__global__ __launch_bounds__(OUT_BLOCK) void k_out_pack_exr(uint32_t xres, const float* __restrict__ rgb, const uint32_t* __restrict__ count, float val,
                                                             const float* __restrict__ d_val, uint8_t* __restrict__ out) {
    const uint32_t y = blockIdx.y, x0 = 2u * (blockIdx.x * OUT_BLOCK + threadIdx.x);
    if (x0 >= xres) return;
    const float s = d_val ? *d_val : val;
    const uint32_t n_px = x0 + 1u < xres ? 2u : 1u;
    uint32_t h[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}}; // [pixel][R, G, B]
    for (uint32_t i = 0; i < n_px; i++) {
        const size_t p = (size_t)y * xres + x0 + i;
        const uint32_t n = ACCUM ? count[p] : 0u;
        for (int k = 0; k < 3; k++) {
            const float v = rgb[3 * p + k];
            h[i][k] = rgk_pack_half(ACCUM ? rgk_pack_accum_value(v, n, s) : rgk_pack_image_value(v, s));
        }
    }
    uint8_t* const line = out + rgk_pack_exr_line_stride(xres) * y;
    if (x0 == 0) {
        int32_t* head = (int32_t*)line; // 8-byte aligned: the stride is a multiple of 8
        head[0] = (int32_t)y;
        head[1] = (int32_t)(8u * xres);
    }
    const size_t plane = (size_t)2 * xres; // bytes
    uint8_t* const at = line + 8 + (size_t)2 * x0;
    if ((xres & 1u) == 0u) { // two pixels, every plane dword aligned
        *(uint32_t*)(at) = RGK_PACK_HALF_ONE | (RGK_PACK_HALF_ONE << 16);
        *(uint32_t*)(at + plane) = h[0][2] | (h[1][2] << 16);
        *(uint32_t*)(at + 2 * plane) = h[0][1] | (h[1][1] << 16);
        *(uint32_t*)(at + 3 * plane) = h[0][0] | (h[1][0] << 16);
    } else {
        for (uint32_t i = 0; i < n_px; i++) {
            *(uint16_t*)(at + 2 * i) = (uint16_t)RGK_PACK_HALF_ONE;
            *(uint16_t*)(at + plane + 2 * i) = (uint16_t)h[i][2];
            *(uint16_t*)(at + 2 * plane + 2 * i) = (uint16_t)h[i][1];
            *(uint16_t*)(at + 3 * plane + 2 * i) = (uint16_t)h[i][0];
        }
    }
}

__global__ __launch_bounds__(OUT_BLOCK) void k_out_pack_png(uint32_t xres, uint32_t raw_bytes, uint32_t payload_bytes, const uint32_t* __restrict__ rgba,
                                                             uint8_t* __restrict__ out) {
    const uint32_t j = 4u * (blockIdx.x * OUT_BLOCK + threadIdx.x); // (payload_bytes < 2^31: no wrap)
    if (j >= payload_bytes) return;
    uint32_t w = 0u; // the last dword's bytes behind the payload are 0: the host's one copy takes whole dwords
    for (uint32_t k = 0; k < 4u; k++)
        if (j + k < payload_bytes) w |= rgk_pack_png_payload_byte(rgba, xres, raw_bytes, j + k) << (8u * k);
    *(uint32_t*)(out + j) = w;
}

__global__ __launch_bounds__(OUT_BLOCK) void k_out_png_sums(uint32_t raw_bytes, uint32_t payload_bytes, uint32_t n_adler, uint32_t n_crc,
                                                             const uint8_t* __restrict__ payload, uint32_t* __restrict__ sums) {
    __shared__ uint32_t table[256];
    {
        uint32_t c = threadIdx.x;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
        table[threadIdx.x] = c; // (OUT_BLOCK == 256)
    }
    __syncthreads();
    const uint32_t t = blockIdx.x * OUT_BLOCK + threadIdx.x;
    if (t < n_adler) {
        const uint32_t start = t * RGK_PACK_SEGMENT, left = raw_bytes - start;
        uint32_t s1, s2;
        rgk_pack_adler_piece([&](uint32_t i) -> uint32_t { return payload[rgk_pack_png_pos(i)]; }, start, left < RGK_PACK_SEGMENT ? left : RGK_PACK_SEGMENT, s1, s2);
        sums[2u * t] = s1;
        sums[2u * t + 1u] = s2;
    } else if (t - n_adler < n_crc) {
        const uint32_t k = t - n_adler, start = k * RGK_PACK_SEGMENT, left = payload_bytes + 4u - start;
        sums[2u * n_adler + k] = rgk_pack_crc_piece(table, [&](uint32_t j) -> uint32_t { return j < 4u ? rgk_pack_idat_type_byte(j) : payload[j - 4u]; }, start,
                                                    left < RGK_PACK_SEGMENT ? left : RGK_PACK_SEGMENT);
    }
}
} // namespace

void rgk_launch_out_max(hipStream_t st, size_t P, const float* rgb, const uint32_t* count, float* partial, float* val) {
    const size_t need = (P + OUT_BLOCK - 1) / OUT_BLOCK;
    const uint32_t wgs = (uint32_t)(need < RGK_OUT_MAX_WGS ? need : RGK_OUT_MAX_WGS);
    k_out_max<<<wgs, OUT_BLOCK, 0, st>>>(P, rgb, count, partial);
    k_out_max_fold<<<1, OUT_BLOCK, 0, st>>>(wgs, partial, val);
}

void rgk_launch_out_pack_exr(hipStream_t st, uint32_t xres, uint32_t yres, const float* rgb, const uint32_t* count, float val, const float* d_val, uint8_t* out) {
    const dim3 grid((xres + 2 * OUT_BLOCK - 1) / (2 * OUT_BLOCK), yres); // (yres <= 65535: check_frame_size)
    if (count) k_out_pack_exr<true><<<grid, OUT_BLOCK, 0, st>>>(xres, rgb, count, val, d_val, out);
    else k_out_pack_exr<false><<<grid, OUT_BLOCK, 0, st>>>(xres, rgb, count, val, d_val, out);
}

void rgk_launch_out_pack_png(hipStream_t st, uint32_t xres, uint32_t yres, const uint32_t* rgba, uint8_t* out) {
    const uint32_t raw = (uint32_t)rgk_pack_png_raw_bytes(xres, yres), payload = (uint32_t)rgk_pack_png_payload_bytes(raw);
    const uint32_t lanes = (payload + 3u) / 4u;
    k_out_pack_png<<<(lanes + OUT_BLOCK - 1) / OUT_BLOCK, OUT_BLOCK, 0, st>>>(xres, raw, payload, rgba, out);
}

void rgk_launch_out_png_sums(hipStream_t st, uint32_t xres, uint32_t yres, const uint8_t* payload, uint32_t* sums) {
    const uint32_t raw = (uint32_t)rgk_pack_png_raw_bytes(xres, yres), bytes = (uint32_t)rgk_pack_png_payload_bytes(raw);
    const uint32_t n_adler = rgk_pack_pieces(raw, RGK_PACK_SEGMENT), n_crc = rgk_pack_pieces((uint64_t)bytes + 4u, RGK_PACK_SEGMENT);
    k_out_png_sums<<<(n_adler + n_crc + OUT_BLOCK - 1) / OUT_BLOCK, OUT_BLOCK, 0, st>>>(raw, bytes, n_adler, n_crc, payload, sums);
}
