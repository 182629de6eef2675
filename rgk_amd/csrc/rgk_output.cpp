// Output path, the host writers: normalise the accumulator the way RenderFrame does after every round and write
// the half-float RGBA OpenEXR file; and the PNG container of the display stage's bytes.  Host code on host buffers, no device work,
// as the reference does it (src/render_driver.cpp:229-247).  A frame that lives on the device does not come through here any more:
// rgk_output_write_exr_device / rgk_output_write_png_device (rgk_post_host.cpp, kernels rgk_pack.hip, arithmetic rgk_pack.h) assemble
// the same files, byte for byte, where the image is.  These writers stay as they are: they serve host buffers and CPU tensors, and
// they are the reference the device path is tested against.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rgk.h"

extern "C" int rgk_internal_fail(int code, const char* msg); // rgk_commit.cpp: sets rgk_last_error

// float -> half with round-to-nearest-even, denormals, overflow to infinity, NaN kept: the value half(float)
// of OpenEXR's half class produces.
extern "C" uint16_t rgk_float_to_half(float v) {
    uint32_t f;
    std::memcpy(&f, &v, 4);
    const uint32_t sign = (f >> 16) & 0x8000u;
    const uint32_t a = f & 0x7fffffffu;
    if (a >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (a > 0x7f800000u ? (0x0200u | ((a >> 13) & 0x3ffu)) : 0u)); // inf / NaN
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);   // rounds to >= 65520: overflow to infinity
    if (a < 0x33000001u) return (uint16_t)sign;                 // < 2^-25 (or exactly 2^-25, a tie to even 0): zero
    int e = (int)(a >> 23) - 127;
    uint32_t m = (a & 0x7fffffu) | 0x800000u;
    int shift;
    uint32_t base;
    if (e < -14) { shift = 13 + (-14 - e); base = 0; }          // half denormal: value = m * 2^(e-23), unit 2^-24
    else { shift = 13; base = (uint32_t)(e + 15) << 10; m &= 0x7fffffu; }
    uint32_t h = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (h & 1u))) h++;           // may carry into the exponent: still correct
    return (uint16_t)(sign | (base + h));
}

extern "C" int rgk_output_normalize(const float* accum_rgb, const uint32_t* accum_count, uint32_t xres, uint32_t yres, float output_scale,
                                    float* out_rgb, float* scale_used) {
    if (!accum_rgb || !accum_count || !out_rgb || xres == 0 || yres == 0) return rgk_internal_fail(RGK_ERR_INVALID, "rgk_output_normalize: null or empty argument");
    const size_t P = (size_t)xres * yres;
    float val = output_scale;
    if (val <= 0.0f) { // texture.cpp:381-391
        float m = 0.0f;
        for (size_t p = 0; p < P; p++) {
            if (accum_count[p] == 0) continue;
            const float n = (float)accum_count[p];
            m = std::max(m, accum_rgb[3 * p] / n);
            m = std::max(m, accum_rgb[3 * p + 1] / n);
            m = std::max(m, accum_rgb[3 * p + 2] / n);
        }
        val = 1.0f / m;
    }
    for (size_t p = 0; p < P; p++) { // out.data *= val (:393-398), then GetPixel = data / count (:349-354)
        const uint32_t c = accum_count[p];
        for (int k = 0; k < 3; k++) out_rgb[3 * p + k] = c ? (accum_rgb[3 * p + k] * val) / (float)c : 0.0f;
    }
    if (scale_used) *scale_used = val;
    return RGK_OK;
}

namespace {
struct Out {
    std::vector<uint8_t> b;
    void raw(const void* p, size_t n) { const uint8_t* q = (const uint8_t*)p; b.insert(b.end(), q, q + n); }
    void str(const char* s) { raw(s, std::strlen(s) + 1); }
    void i32(int32_t v) { raw(&v, 4); }
    void u64(uint64_t v) { raw(&v, 8); }
    void f32(float v) { raw(&v, 4); }
    void attr(const char* name, const char* type, int32_t size) { str(name); str(type); i32(size); }
};
} // namespace

extern "C" int rgk_output_write_exr(const char* path, uint32_t xres, uint32_t yres, const float* rgb) {
    if (!path || !rgb || xres == 0 || yres == 0) return rgk_internal_fail(RGK_ERR_INVALID, "rgk_output_write_exr: null or empty argument");
    Out o;
    o.i32(20000630); // magic
    o.i32(2);        // version 2, single-part scan-line
    // channels: A, B, G, R (alphabetical), HALF, linear, sampling 1 x 1
    o.attr("channels", "chlist", 4 * (2 + 4 + 4 + 4 + 4) + 1);
    for (const char* c : {"A", "B", "G", "R"}) { o.str(c); o.i32(1); o.b.push_back(0); o.b.push_back(0); o.b.push_back(0); o.b.push_back(0); o.i32(1); o.i32(1); }
    o.b.push_back(0);
    o.attr("compression", "compression", 1); o.b.push_back(0); // NO_COMPRESSION
    o.attr("dataWindow", "box2i", 16); o.i32(0); o.i32(0); o.i32((int32_t)xres - 1); o.i32((int32_t)yres - 1);
    o.attr("displayWindow", "box2i", 16); o.i32(0); o.i32(0); o.i32((int32_t)xres - 1); o.i32((int32_t)yres - 1);
    o.attr("lineOrder", "lineOrder", 1); o.b.push_back(0); // INCREASING_Y
    o.attr("pixelAspectRatio", "float", 4); o.f32(1.0f);
    o.attr("screenWindowCenter", "v2f", 8); o.f32(0.0f); o.f32(0.0f);
    o.attr("screenWindowWidth", "float", 4); o.f32(1.0f);
    o.b.push_back(0); // end of header
    const size_t line_bytes = (size_t)xres * 4 * 2, table_at = o.b.size();
    const uint64_t first = table_at + (uint64_t)8 * yres;
    for (uint32_t y = 0; y < yres; y++) o.u64(first + (uint64_t)y * (8 + line_bytes));
    std::vector<uint16_t> line((size_t)xres * 4);
    const uint16_t one = rgk_float_to_half(1.0f);
    for (uint32_t y = 0; y < yres; y++) {
        const float* src = rgb + (size_t)y * xres * 3;
        for (uint32_t x = 0; x < xres; x++) {
            line[x] = one;                                            // A
            line[(size_t)xres + x] = rgk_float_to_half(src[3 * x + 2]);     // B
            line[(size_t)2 * xres + x] = rgk_float_to_half(src[3 * x + 1]); // G
            line[(size_t)3 * xres + x] = rgk_float_to_half(src[3 * x]);     // R
        }
        o.i32((int32_t)y);
        o.i32((int32_t)line_bytes);
        o.raw(line.data(), line_bytes);
    }
    FILE* f = std::fopen(path, "wb");
    if (!f) return rgk_internal_fail(RGK_ERR_INVALID, "rgk_output_write_exr: cannot open the output file");
    const size_t w = std::fwrite(o.b.data(), 1, o.b.size(), f);
    const int rc = std::fclose(f);
    if (w != o.b.size() || rc != 0) return rgk_internal_fail(RGK_ERR_DEVICE, "rgk_output_write_exr: short write");
    return RGK_OK;
}

// ---- PNG (rgk.h rgk_output_write_png): 8-bit truecolour, filter 0, stored deflate blocks; the two checksums are the file's own
namespace {
uint32_t crc32_of(const uint8_t* p, size_t n, uint32_t crc = 0) { // ISO 3309 / PNG annex D, bit by bit into a table built once
    static const struct Table {
        uint32_t t[256];
        Table() {
            for (uint32_t i = 0; i < 256; i++) {
                uint32_t c = i;
                for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
                t[i] = c;
            }
        }
    } tab;
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = tab.t[(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
    return ~crc;
}
uint32_t adler32_of(const uint8_t* p, size_t n) { // RFC 1950; 5552: the most bytes whose sums cannot overflow 32 bits before the modulo
    uint32_t a = 1, b = 0;
    while (n) {
        const size_t k = n < 5552 ? n : 5552;
        for (size_t i = 0; i < k; i++) { a += p[i]; b += a; }
        a %= 65521u; b %= 65521u;
        p += k; n -= k;
    }
    return (b << 16) | a;
}
void be32(std::vector<uint8_t>& o, uint32_t v) { for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(v >> s)); }
// length, type, data, CRC of type + data
void png_chunk(std::vector<uint8_t>& o, const char type[4], const std::vector<uint8_t>& data) {
    be32(o, (uint32_t)data.size());
    const size_t at = o.size();
    o.insert(o.end(), type, type + 4);
    o.insert(o.end(), data.begin(), data.end());
    be32(o, crc32_of(o.data() + at, o.size() - at));
}
} // namespace

extern "C" int rgk_output_write_png(const char* path, uint32_t xres, uint32_t yres, const uint32_t* rgba) {
    if (!path || !rgba || xres == 0 || yres == 0 || xres > 0x7fffffffu || yres > 0x7fffffffu)
        return rgk_internal_fail(RGK_ERR_INVALID, "rgk_output_write_png: null argument, or a side that is 0 or above 2^31 - 1");
    const uint64_t raw_bytes = ((uint64_t)xres * 3 + 1) * yres; // a filter byte and the row's R, G, B bytes, row after row
    const uint64_t blocks = (raw_bytes + 65534) / 65535;
    if (2 + raw_bytes + 5 * blocks + 4 > 0x7fffffffull) return rgk_internal_fail(RGK_ERR_INVALID, "rgk_output_write_png: the image does not fit one IDAT chunk");
    std::vector<uint8_t> raw;
    raw.reserve((size_t)raw_bytes);
    for (uint32_t y = 0; y < yres; y++) {
        raw.push_back(0); // filter 0: none
        const uint32_t* src = rgba + (size_t)y * xres;
        for (uint32_t x = 0; x < xres; x++) {
            raw.push_back((uint8_t)(src[x] & 0xffu));
            raw.push_back((uint8_t)((src[x] >> 8) & 0xffu));
            raw.push_back((uint8_t)((src[x] >> 16) & 0xffu));
        }
    }
    std::vector<uint8_t> z;
    z.reserve(raw.size() + 5 * (size_t)blocks + 6);
    z.push_back(0x78); z.push_back(0x01); // zlib header: deflate, 32 K window, no preset dictionary (0x7801 is a multiple of 31)
    for (size_t at = 0; at < raw.size();) {
        const size_t n = raw.size() - at < 65535 ? raw.size() - at : 65535;
        z.push_back(at + n == raw.size() ? 1 : 0); // BFINAL, BTYPE 00: stored
        z.push_back((uint8_t)(n & 0xff)); z.push_back((uint8_t)(n >> 8));
        z.push_back((uint8_t)(~n & 0xff)); z.push_back((uint8_t)((~n >> 8) & 0xff));
        z.insert(z.end(), raw.begin() + at, raw.begin() + at + n);
        at += n;
    }
    be32(z, adler32_of(raw.data(), raw.size()));
    std::vector<uint8_t> o = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a}, ihdr;
    be32(ihdr, xres); be32(ihdr, yres);
    for (uint8_t v : {8, 2, 0, 0, 0}) ihdr.push_back(v); // bit depth 8, colour type 2 (truecolour), deflate, adaptive filtering, no interlace
    png_chunk(o, "IHDR", ihdr);
    png_chunk(o, "IDAT", z);
    png_chunk(o, "IEND", {});
    FILE* f = std::fopen(path, "wb");
    if (!f) return rgk_internal_fail(RGK_ERR_INVALID, "rgk_output_write_png: cannot open the output file");
    const size_t w = std::fwrite(o.data(), 1, o.size(), f);
    const int rc = std::fclose(f);
    if (w != o.size() || rc != 0) return rgk_internal_fail(RGK_ERR_DEVICE, "rgk_output_write_png: short write");
    return RGK_OK;
}
