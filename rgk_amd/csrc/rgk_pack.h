// The device output path's arithmetic (rgk.h "output path on the device"), written once for the kernels (rgk_pack.hip: k_out_max,
// k_out_pack_exr, k_out_pack_png, k_out_png_sums) and the host (rgk_post_host.cpp: the file images around what the kernels fill, the
// folds of the partial maxima and of the checksum pieces).  Like rgk_display.h: pure functions marked RGK_HD (rgk_libm.h) that call
// nothing of the HIP runtime, so the unit builds with any host compiler and what the device runs here is the source
// tests/cpp/pack_main.cpp runs under sanitizers.  Plain integer and float32 operations, compiled without contraction on both sides;
// every byte is the one rgk_output.cpp's host writers produce, which stay the reference.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/rgk_libm.h"

// ------------------------------------------------------------------ float -> half, the integer sequence of rgk_float_to_half
RGK_HD uint32_t rgk_pack_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
// round to nearest even, half denormals, overflow to infinity from 0x477ff000 on, NaN kept (0x0200 and the payload's top ten bits),
// 2^-25 and below to signed zero
RGK_HD uint32_t rgk_pack_half(float v) {
    const uint32_t f = rgk_pack_bits(v);
    const uint32_t sign = (f >> 16) & 0x8000u;
    const uint32_t a = f & 0x7fffffffu;
    if (a >= 0x7f800000u) return sign | 0x7c00u | (a > 0x7f800000u ? (0x0200u | ((a >> 13) & 0x3ffu)) : 0u);
    if (a >= 0x477ff000u) return sign | 0x7c00u;
    if (a < 0x33000001u) return sign;
    const int e = (int)(a >> 23) - 127;
    uint32_t m = (a & 0x7fffffu) | 0x800000u;
    uint32_t shift = 13u, base = 0u;
    if (e < -14) shift = 13u + (uint32_t)(-14 - e);      // half denormal: unit 2^-24; shift <= 24 here (a > 2^-25)
    else { base = (uint32_t)(e + 15) << 10; m &= 0x7fffffu; }
    uint32_t h = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (h & 1u))) h++;    // may carry into the exponent: still correct
    return sign | (base + h);
}
constexpr uint32_t RGK_PACK_HALF_ONE = 0x3c00u; // rgk_pack_half(1.0f): the A plane

// ------------------------------------------------------------------ the pixel values
// accumulator mode (rgk_output_normalize): multiply first, then an IEEE divide; 0 where no sample fell
RGK_HD float rgk_pack_accum_value(float a, uint32_t n, float val) { return n ? (a * val) / (float)n : 0.0f; }
// image mode: the one multiply torch's (image * val) does
RGK_HD float rgk_pack_image_value(float v, float val) { return v * val; }

// ------------------------------------------------------------------ auto scale
// The host loop's std::max(m, x): a NaN x never wins, -0 never wins over +0.  Every partial starts at +0.0f and what remains is a
// maximum of ordinary values, so any tree of these merges gives the loop's bits.
RGK_HD float rgk_pack_max(float m, float x) { return (m < x) ? x : m; }
RGK_HD float rgk_pack_max_pixel(float m, float r, float g, float b, uint32_t n) {
    if (n == 0) return m;
    const float fn = (float)n;
    m = rgk_pack_max(m, r / fn);
    m = rgk_pack_max(m, g / fn);
    return rgk_pack_max(m, b / fn);
}
RGK_HD float rgk_pack_scale_of_max(float m) { return 1.0f / m; } // (+inf for a frame with no positive value, as the host)

// ------------------------------------------------------------------ EXR layout (rgk_output_write_exr)
// header, offset table (8 * yres bytes), then per line {int32 y, int32 8 * xres, A plane, B, G, R}, xres halves each
constexpr size_t RGK_PACK_EXR_HEADER = 331; // bytes before the offset table (checked against the writer by tests/cpp/pack_main.cpp)
RGK_HD size_t rgk_pack_exr_line_stride(uint32_t xres) { return 8u + (size_t)8 * xres; }
RGK_HD size_t rgk_pack_exr_data_at(uint32_t yres) { return RGK_PACK_EXR_HEADER + (size_t)8 * yres; } // `first`: where line 0 starts
RGK_HD size_t rgk_pack_exr_data_bytes(uint32_t xres, uint32_t yres) { return rgk_pack_exr_line_stride(xres) * yres; }
// inside the data region: where plane c (0 A, 1 B, 2 G, 3 R) of line y starts
RGK_HD size_t rgk_pack_exr_plane_at(uint32_t xres, uint32_t y, uint32_t c) { return rgk_pack_exr_line_stride(xres) * y + 8u + (size_t)2 * xres * c; }

// ------------------------------------------------------------------ PNG layout (rgk_output_write_png)
// The raw stream: per row a filter byte 0, then R, G, B per pixel.  The IDAT payload built on the device: the two zlib header bytes,
// then per 65535 raw bytes a five-byte stored-block header and the bytes; the Adler word behind it is the host's.
constexpr uint32_t RGK_PACK_BLOCK = 65535u;
RGK_HD uint64_t rgk_pack_png_raw_bytes(uint32_t xres, uint32_t yres) { return ((uint64_t)xres * 3u + 1u) * yres; }
RGK_HD uint64_t rgk_pack_png_blocks(uint64_t raw_bytes) { return (raw_bytes + (RGK_PACK_BLOCK - 1u)) / RGK_PACK_BLOCK; }
RGK_HD uint64_t rgk_pack_png_payload_bytes(uint64_t raw_bytes) { return 2u + raw_bytes + 5u * rgk_pack_png_blocks(raw_bytes); }
// what rgk_output_write_png refuses: the IDAT chunk's data (payload + Adler word) must stay below 2^31
RGK_HD bool rgk_pack_png_fits(uint32_t xres, uint32_t yres) {
    if (xres == 0 || yres == 0 || xres > 0x7fffffffu || yres > 0x7fffffffu) return false;
    return rgk_pack_png_payload_bytes(rgk_pack_png_raw_bytes(xres, yres)) + 4u <= 0x7fffffffull;
}
// payload position of raw byte i
RGK_HD uint32_t rgk_pack_png_pos(uint32_t i) { return 2u + 5u * (i / RGK_PACK_BLOCK + 1u) + i; }
// raw byte i of the image (rgba: one R, G, B, x word per pixel, little endian)
RGK_HD uint32_t rgk_pack_png_raw_byte(const uint32_t* rgba, uint32_t xres, uint32_t i) {
    const uint32_t row_bytes = 3u * xres + 1u, y = i / row_bytes, c = i - y * row_bytes;
    if (c == 0) return 0u; // filter 0: none
    const uint32_t x = (c - 1u) / 3u, k = (c - 1u) - 3u * x;
    return (rgba[(size_t)y * xres + x] >> (8u * k)) & 0xffu;
}
// Byte j of the payload (j < rgk_pack_png_payload_bytes(raw_bytes) < 2^31) is either one of the stream's own bytes -- true, and
// `v` is its value -- or a raw byte -- false, and `v` is its index in the raw stream.
RGK_HD bool rgk_pack_png_stream_byte(uint32_t raw_bytes, uint32_t j, uint32_t& v) {
    if (j < 2u) { v = j == 0u ? 0x78u : 0x01u; return true; } // zlib header: deflate, 32 K window, no preset dictionary
    const uint32_t q = j - 2u, blk = q / (RGK_PACK_BLOCK + 5u), r = q - blk * (RGK_PACK_BLOCK + 5u);
    if (r >= 5u) { v = blk * RGK_PACK_BLOCK + (r - 5u); return false; }
    const uint32_t left = raw_bytes - blk * RGK_PACK_BLOCK, n = left < RGK_PACK_BLOCK ? left : RGK_PACK_BLOCK; // LEN of this block
    if (r == 0u) v = left <= RGK_PACK_BLOCK ? 1u : 0u; // BFINAL, BTYPE 00: stored
    else if (r == 1u) v = n & 0xffu;
    else if (r == 2u) v = n >> 8;
    else if (r == 3u) v = ~n & 0xffu;
    else v = (~n >> 8) & 0xffu;
    return true;
}
RGK_HD uint32_t rgk_pack_png_payload_byte(const uint32_t* rgba, uint32_t xres, uint32_t raw_bytes, uint32_t j) {
    uint32_t v;
    return rgk_pack_png_stream_byte(raw_bytes, j, v) ? v : rgk_pack_png_raw_byte(rgba, xres, v);
}

// ------------------------------------------------------------------ checksums from pieces
// A piece is RGK_PACK_SEGMENT bytes of the stream being summed (the last one what is left).  4 KiB: a piece's second Adler sum
// stays below 2^32 (255 * 4096 * 4097 / 2 = 2,139,586,560), so a lane sums in 32 bits with no modulo, and a 1920 x 1080 picture is
// about 1500 pieces per checksum -- 3000 lanes of latency-bound work, which is what the byte-serial CRC recurrence needs to hide.
constexpr uint32_t RGK_PACK_SEGMENT = 4096u;
RGK_HD uint32_t rgk_pack_pieces(uint64_t bytes, uint32_t seg) { return (uint32_t)((bytes + seg - 1u) / seg); }
// Adler-32 piece of `len` bytes b_0 .. b_{len-1} (len <= 4096): s1 = sum of b_j, s2 = sum of (len - j) * b_j
template <class ByteAt>
RGK_HD void rgk_pack_adler_piece(ByteAt byte_at, uint32_t start, uint32_t len, uint32_t& s1, uint32_t& s2) {
    uint32_t a = 0u, b = 0u;
    for (uint32_t j = 0; j < len; j++) { a += byte_at(start + j); b += a; }
    s1 = a; s2 = b;
}
// CRC-32 (ISO 3309) of a piece on its own: initial value and final complement as for a whole message
template <class ByteAt>
RGK_HD uint32_t rgk_pack_crc_piece(const uint32_t* table, ByteAt byte_at, uint32_t start, uint32_t len) {
    uint32_t crc = 0xffffffffu;
    for (uint32_t j = 0; j < len; j++) crc = table[(crc ^ byte_at(start + j)) & 0xffu] ^ (crc >> 8);
    return ~crc;
}
// byte j of the IDAT chunk's summed stream without the Adler word: the type, then the payload
RGK_HD uint32_t rgk_pack_idat_type_byte(uint32_t j) { return j == 0u ? 0x49u : (j == 1u ? 0x44u : (j == 2u ? 0x41u : 0x54u)); } // "IDAT"

// ------------------------------------------------------------------ host only: the table, the folds, the file images
inline void rgk_pack_crc_table(uint32_t* t /*256*/) {
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
        t[i] = c;
    }
}
// Adler-32 of a stream from its pieces in order: (a, b) starts at (1, 0); a piece of len bytes adds s1 to a and len * a + s2 to b
struct RgkPackAdler {
    uint64_t a = 1, b = 0;
    void add(uint32_t s1, uint32_t s2, uint32_t len) {
        b = (b + (uint64_t)len * a + s2) % 65521u;
        a = (a + s1) % 65521u;
    }
    uint32_t value() const { return (uint32_t)((b << 16) | a); }
};
// The GF(2) operator that carries a CRC register over `len` zero bytes: crc(A || B) = shift_|B|(crc(A)) ^ crc(B) for the complemented
// CRCs of rgk_pack_crc_piece.  32 columns; built by squaring the one-bit operator log2(8 * len) times.
struct RgkPackCrcShift {
    uint32_t col[32];
    static uint32_t times(const uint32_t* m, uint32_t v) {
        uint32_t s = 0;
        for (int i = 0; v; v >>= 1, i++)
            if (v & 1u) s ^= m[i];
        return s;
    }
    static void square(uint32_t* out, const uint32_t* m) {
        for (int i = 0; i < 32; i++) out[i] = times(m, m[i]);
    }
    explicit RgkPackCrcShift(uint64_t len) {
        uint32_t odd[32], even[32];
        odd[0] = 0xedb88320u; // one zero bit
        for (int i = 1; i < 32; i++) odd[i] = 1u << (i - 1);
        square(even, odd);  // two bits
        square(odd, even);  // four bits
        for (int i = 0; i < 32; i++) col[i] = 1u << i; // identity
        uint32_t* p = odd; uint32_t* q = even; // *q: the operator of 8 << k bits after k rounds
        for (; len; len >>= 1) {
            square(q, p);
            if (len & 1u) {
                uint32_t next[32];
                for (int i = 0; i < 32; i++) next[i] = times(q, col[i]);
                for (int i = 0; i < 32; i++) col[i] = next[i];
            }
            uint32_t* t = p; p = q; q = t;
        }
    }
    uint32_t apply(uint32_t crc) const { return times(col, crc); }
};
// CRC-32 of a stream of `bytes` bytes from the CRCs of its pieces of `seg` bytes (the last one shorter or equal)
inline uint32_t rgk_pack_crc_fold(const uint32_t* piece_crc, uint64_t bytes, uint32_t seg) {
    const uint32_t n = rgk_pack_pieces(bytes, seg);
    if (n == 0) return 0u;
    const uint64_t last = bytes - (uint64_t)(n - 1u) * seg;
    const RgkPackCrcShift full(seg), tail(last);
    uint32_t crc = piece_crc[0];
    for (uint32_t k = 1; k < n; k++) crc = (k + 1u == n ? tail : full).apply(crc) ^ piece_crc[k];
    return crc;
}
// ... and carried on over a few more bytes (the Adler word behind the payload)
inline uint32_t rgk_pack_crc_more(const uint32_t* table, uint32_t crc, const uint8_t* p, size_t n) {
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
    return ~crc;
}

inline void rgk_pack_be32(uint8_t* o, uint32_t v) { o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v; }

// The EXR header and offset table: rgk_pack_exr_data_at(yres) bytes at `o`.
inline void rgk_pack_exr_head(uint8_t* o, uint32_t xres, uint32_t yres) {
    uint8_t* const o0 = o;
    const auto raw = [&](const void* p, size_t n) { __builtin_memcpy(o, p, n); o += n; };
    const auto i32 = [&](int32_t v) { raw(&v, 4); };
    const auto f32 = [&](float v) { raw(&v, 4); };
    const auto str = [&](const char* s) { size_t n = 0; while (s[n]) n++; raw(s, n + 1); };
    const auto byte = [&](uint8_t v) { *o++ = v; };
    const auto attr = [&](const char* name, const char* type, int32_t size) { str(name); str(type); i32(size); };
    i32(20000630); // magic
    i32(2);        // version 2, single-part scan-line
    attr("channels", "chlist", 4 * (2 + 4 + 4 + 4 + 4) + 1); // A, B, G, R (alphabetical), HALF, linear, sampling 1 x 1
    for (const char* c : {"A", "B", "G", "R"}) { str(c); i32(1); byte(0); byte(0); byte(0); byte(0); i32(1); i32(1); }
    byte(0);
    attr("compression", "compression", 1); byte(0); // NO_COMPRESSION
    attr("dataWindow", "box2i", 16); i32(0); i32(0); i32((int32_t)xres - 1); i32((int32_t)yres - 1);
    attr("displayWindow", "box2i", 16); i32(0); i32(0); i32((int32_t)xres - 1); i32((int32_t)yres - 1);
    attr("lineOrder", "lineOrder", 1); byte(0); // INCREASING_Y
    attr("pixelAspectRatio", "float", 4); f32(1.0f);
    attr("screenWindowCenter", "v2f", 8); f32(0.0f); f32(0.0f);
    attr("screenWindowWidth", "float", 4); f32(1.0f);
    byte(0); // end of header
    (void)o0; // (o - o0 == RGK_PACK_EXR_HEADER: tests/cpp/pack_main.cpp)
    const uint64_t first = rgk_pack_exr_data_at(yres);
    for (uint32_t y = 0; y < yres; y++) { const uint64_t at = first + (uint64_t)y * rgk_pack_exr_line_stride(xres); raw(&at, 8); }
}

// The PNG file around the payload: RGK_PACK_PNG_LEAD bytes (signature, IHDR chunk, the IDAT chunk's length and type) in front of it,
// RGK_PACK_PNG_TAIL bytes (Adler word, the IDAT chunk's CRC, the IEND chunk) behind.
constexpr size_t RGK_PACK_PNG_LEAD = 8 + 25 + 8, RGK_PACK_PNG_TAIL = 4 + 4 + 12;
inline void rgk_pack_png_lead(uint8_t* o, const uint32_t* table, uint32_t xres, uint32_t yres, uint64_t payload_bytes) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    __builtin_memcpy(o, sig, 8);
    rgk_pack_be32(o + 8, 13);
    __builtin_memcpy(o + 12, "IHDR", 4);
    rgk_pack_be32(o + 16, xres);
    rgk_pack_be32(o + 20, yres);
    const uint8_t rest[5] = {8, 2, 0, 0, 0}; // bit depth 8, colour type 2 (truecolour), deflate, adaptive filtering, no interlace
    __builtin_memcpy(o + 24, rest, 5);
    rgk_pack_be32(o + 29, rgk_pack_crc_more(table, 0u, o + 12, 17));
    rgk_pack_be32(o + 33, (uint32_t)(payload_bytes + 4u));
    __builtin_memcpy(o + 37, "IDAT", 4);
}
// adler: of the raw stream; crc_to_payload_end: CRC of "IDAT" + payload
inline void rgk_pack_png_tail(uint8_t* o, const uint32_t* table, uint32_t adler, uint32_t crc_to_payload_end) {
    rgk_pack_be32(o, adler);
    rgk_pack_be32(o + 4, rgk_pack_crc_more(table, crc_to_payload_end, o, 4));
    rgk_pack_be32(o + 8, 0);
    __builtin_memcpy(o + 12, "IEND", 4);
    rgk_pack_be32(o + 16, rgk_pack_crc_more(table, 0u, o + 12, 4));
}
