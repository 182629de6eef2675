// The device output path's GPU-free parts on the CPU: this file includes rgk_amd/csrc/rgk_pack.h -- the functions the four kernels
// call, the folds and the file images the host entries build -- and rgk_amd/csrc/rgk_output.cpp, the host writers that are the
// reference for every comparison here.  Nothing needs the HIP runtime; the program links without it.  Every bar is equality of bytes.
// Usage: pack_main <case> [directory for the files the exr and png cases write]; exit status 0 = every condition held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rgk_amd/csrc/rgk_pack.h"
#include "../../rgk_amd/csrc/rgk_output.cpp"

extern "C" int rgk_internal_fail(int code, const char*) { return code; } // (rgk_commit.cpp's in the library)

static int failures = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        if (!(c)) { if (failures < 20) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
    } while (0)

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint64_t rng_state = 0x9e3779b97f4a7c15ull; // splitmix64, fixed seed
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static std::vector<uint8_t> read_file(const std::string& path) {
    std::vector<uint8_t> b;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return b;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + n);
    std::fclose(f);
    return b;
}

// ------------------------------------------------------------------ half conversion
static uint64_t halves_checked = 0;
static void half_of(uint32_t bits) {
    const float f = from_bits(bits);
    CHECK(rgk_pack_half(f) == (uint32_t)rgk_float_to_half(f));
    halves_checked++;
}
static void around(uint32_t bits) { // a float and its two neighbours, both signs
    for (uint32_t s : {0u, 0x80000000u})
        for (uint32_t d : {0xffffffffu, 0u, 1u}) half_of(((bits + d) & 0x7fffffffu) | s);
}
// the float that equals a finite half (h < 0x7c00); 0x7c00 stands for 65536, the value the largest half's upper midpoint is taken to
static float half_value(uint32_t h) {
    const uint32_t e = h >> 10, m = h & 0x3ffu;
    if (e == 0) return std::ldexp((float)m, -24);
    return std::ldexp((float)(m | 0x400u), (int)e - 25);
}
static void half() {
    for (uint32_t h = 0; h < 0x7c00u; h++) {
        const float f = half_value(h), g = half_value(h + 1u), mid = 0.5f * f + 0.5f * g; // exact: eleven or twelve significant bits
        CHECK((uint32_t)rgk_float_to_half(f) == h);
        around(rgk_pack_bits(f));
        around(rgk_pack_bits(mid)); // the midpoint to the next half up; it is the next half's midpoint down
    }
    for (uint32_t h = 0x7c00u; h < 0x8000u; h++) around(0x7f800000u | ((h & 0x3ffu) << 13)); // infinity and every NaN half
    for (uint32_t b : {0x33000000u, 0x33000001u, 0x477fefffu, 0x477ff000u}) around(b);
    for (uint32_t b : {0u, 0x7f800000u, 0x7fc00000u, 0x7fc00001u, 0x7fffffffu, 0x7fe00000u, 0x7f800001u, 0x7f801fffu, 0x7f802000u, 0x7fbfffffu, 0x7fa00000u}) around(b);
    CHECK(rgk_pack_half(1.0f) == RGK_PACK_HALF_ONE && rgk_float_to_half(1.0f) == RGK_PACK_HALF_ONE);
    for (int i = 0; i < (1 << 20); i++) half_of((uint32_t)rnd());
    CHECK(halves_checked > 1400000);
}

// ------------------------------------------------------------------ the two pixel expressions
static void pixel() {
    const uint32_t counts[] = {0u, 1u, 3u, 256u, (1u << 24) + 1u, 0xffffffffu, 7u};
    std::vector<float> acc;
    std::vector<uint32_t> cnt;
    const float specials[] = {0.0f, -0.0f, 1.0f, -2.5f, 1e-40f, 3e38f, INFINITY, -INFINITY, NAN, 0.1f, 65504.0f, 5.9604645e-8f};
    for (uint32_t n : counts)
        for (int rep = 0; rep < 64; rep++) {
            for (int k = 0; k < 3; k++) acc.push_back(rep < 12 ? specials[(rep + k) % 12] : from_bits((uint32_t)rnd()));
            cnt.push_back(n);
        }
    const uint32_t P = (uint32_t)cnt.size();
    std::vector<float> want(acc.size());
    for (float val : {1.0f, 0.0573f, 3.7e-5f, 2.0f, INFINITY}) {
        float used = 0.0f;
        CHECK(rgk_output_normalize(acc.data(), cnt.data(), P, 1, val, want.data(), &used) == RGK_OK && rgk_pack_bits(used) == rgk_pack_bits(val));
        for (uint32_t p = 0; p < P; p++)
            for (int k = 0; k < 3; k++) {
                CHECK(rgk_pack_bits(rgk_pack_accum_value(acc[3 * p + k], cnt[p], val)) == rgk_pack_bits(want[3 * p + k]));
                volatile float v = acc[3 * p + k], s = val; // the single multiply, not folded by the compiler
                const float prod = v * s;
                CHECK(rgk_pack_bits(rgk_pack_image_value(acc[3 * p + k], val)) == rgk_pack_bits(prod));
            }
    }
    // (float)n rounds at 2^24 + 1: the divisor is 2^24
    CHECK(rgk_pack_accum_value(16777216.0f, (1u << 24) + 1u, 1.0f) == 1.0f && rgk_pack_accum_value(3.0f, 0u, 2.0f) == 0.0f);
}

// ------------------------------------------------------------------ the auto-scale fold
static float fold_chunks(const std::vector<float>& a, const std::vector<uint32_t>& n, size_t chunk, bool strided, bool pairwise) {
    const size_t P = n.size(), parts = (P + chunk - 1) / chunk;
    std::vector<float> part(parts, 0.0f);
    for (size_t p = 0; p < P; p++) {
        float& m = part[strided ? p % parts : p / chunk];
        m = rgk_pack_max_pixel(m, a[3 * p], a[3 * p + 1], a[3 * p + 2], n[p]);
    }
    if (pairwise) // a tree, as a workgroup folds
        for (size_t step = 1; step < parts; step *= 2)
            for (size_t i = 0; i + step < parts; i += 2 * step) part[i] = rgk_pack_max(part[i], part[i + step]);
    else // ... or from the back
        for (size_t i = parts - 1; i > 0; i--) part[0] = rgk_pack_max(part[0], part[i]);
    return rgk_pack_scale_of_max(part[0]);
}
static void scale() {
    const size_t P = 67 * 45;
    for (int kind = 0; kind < 6; kind++) {
        std::vector<float> a(3 * P);
        std::vector<uint32_t> n(P);
        for (size_t p = 0; p < P; p++) {
            n[p] = (uint32_t)(rnd() % 5u) * (uint32_t)(rnd() % 3u); // many zeros
            for (int k = 0; k < 3; k++) {
                float v = (float)(rnd() % 100000u) * 1e-3f;
                if (kind == 1) v = 0.0f;                                   // nothing positive: the scale is +inf
                if (kind == 2) v = -v - 1.0f;                              // all negative
                if (kind == 3 && rnd() % 7u == 0) v = NAN;                 // NaNs never win
                if (kind == 4) v = rnd() % 2u ? -0.0f : 0.0f;              // -0 never wins over +0
                if (kind == 5 && p == 1234 && k == 1) v = INFINITY;        // +inf wins: the scale is 0
                a[3 * p + k] = v;
            }
        }
        if (kind == 3) { a[0] = NAN; n[0] = 1; a[3 * (P - 1)] = NAN; n[P - 1] = 2; }
        std::vector<float> out(3 * P);
        float want = 0.0f;
        CHECK(rgk_output_normalize(a.data(), n.data(), 67, 45, -1.0f, out.data(), &want) == RGK_OK);
        const float got[3] = {fold_chunks(a, n, 1, false, true), fold_chunks(a, n, 7, false, false), fold_chunks(a, n, 256, true, true)};
        for (float g : got) CHECK(rgk_pack_bits(g) == rgk_pack_bits(want));
        if (kind == 1 || kind == 2 || kind == 4) CHECK(rgk_pack_bits(want) == 0x7f800000u);
        if (kind == 5) CHECK(rgk_pack_bits(want) == 0u);
    }
}

// ------------------------------------------------------------------ the EXR layout
static void exr(const std::string& dir) {
    const uint32_t sizes[3][2] = {{1, 1}, {3, 2}, {67, 45}};
    for (const auto& sz : sizes) {
        const uint32_t W = sz[0], H = sz[1];
        std::vector<float> rgb((size_t)3 * W * H);
        for (float& v : rgb) v = from_bits((uint32_t)rnd());
        const std::string path = dir + "/ref.exr";
        CHECK(rgk_output_write_exr(path.c_str(), W, H, rgb.data()) == RGK_OK);
        const std::vector<uint8_t> want = read_file(path);
        const size_t head = rgk_pack_exr_data_at(H), data = rgk_pack_exr_data_bytes(W, H);
        std::vector<uint8_t> got(head + data + 8, 0xA5);
        rgk_pack_exr_head(got.data(), W, H);
        CHECK(got[head] == 0xA5); // the header and the table end where the data region starts
        uint8_t* const d = got.data() + head;
        for (uint32_t y = 0; y < H; y++) { // what k_out_pack_exr stores
            const int32_t line[2] = {(int32_t)y, (int32_t)(8 * W)};
            std::memcpy(d + rgk_pack_exr_line_stride(W) * y, line, 8);
            for (uint32_t x = 0; x < W; x++)
                for (uint32_t c = 0; c < 4; c++) {
                    const uint16_t h = c == 0 ? (uint16_t)RGK_PACK_HALF_ONE : (uint16_t)rgk_pack_half(rgk_pack_image_value(rgb[3 * ((size_t)y * W + x) + (3 - c)], 1.0f));
                    std::memcpy(d + rgk_pack_exr_plane_at(W, y, c) + 2 * x, &h, 2);
                }
        }
        for (size_t i = head + data; i < got.size(); i++) CHECK(got[i] == 0xA5);
        got.resize(head + data);
        CHECK(want.size() == head + data && got == want);
    }
}

// ------------------------------------------------------------------ the PNG layout and the checksums from pieces
static void stream_of(const std::vector<uint8_t>& raw, std::vector<uint8_t>& z) { // rgk_output_write_png's loop
    z.clear();
    z.push_back(0x78); z.push_back(0x01);
    for (size_t at = 0; at < raw.size();) {
        const size_t n = raw.size() - at < 65535 ? raw.size() - at : 65535;
        z.push_back(at + n == raw.size() ? 1 : 0);
        z.push_back((uint8_t)(n & 0xff)); z.push_back((uint8_t)(n >> 8));
        z.push_back((uint8_t)(~n & 0xff)); z.push_back((uint8_t)((~n >> 8) & 0xff));
        z.insert(z.end(), raw.begin() + at, raw.begin() + at + n);
        at += n;
    }
}
static void checksums() {
    uint32_t table[256];
    rgk_pack_crc_table(table);
    const uint32_t L = RGK_PACK_SEGMENT;
    const uint32_t sizes[] = {1, L - 1, L, L + 1, 65535, 65536, 2 * 65535 + 7};
    const uint32_t segs[] = {L, L - 1, 1000, 4369, 7, 1, 5803}; // 4369 divides 65535, 5803: the longest piece whose sums fit 32 bits
    for (uint32_t size : sizes) {
        std::vector<uint8_t> raw(size), z;
        for (uint8_t& b : raw) b = (uint8_t)(rnd() % 3u ? rnd() : 0xff);
        stream_of(raw, z);
        // layout: the stream's own bytes and where the raw bytes land
        CHECK(rgk_pack_png_payload_bytes(size) == z.size() && rgk_pack_png_blocks(size) == (size + 65534) / 65535);
        size_t raws = 0;
        for (uint32_t j = 0; j < (uint32_t)z.size(); j++) {
            uint32_t v = 0;
            if (rgk_pack_png_stream_byte(size, j, v)) CHECK(v == z[j]);
            else { CHECK(v < size && rgk_pack_png_pos(v) == j && raw[v] == z[j]); raws++; }
        }
        CHECK(raws == size);
        for (uint32_t seg : segs) {
            if (seg == 1 && size > 70000) continue;
            // Adler-32 of the raw stream from pieces read back out of the payload, as the kernel reads them
            RgkPackAdler ad;
            for (uint32_t k = 0; k < rgk_pack_pieces(size, seg); k++) {
                const uint32_t start = k * seg, len = size - start < seg ? size - start : seg;
                uint32_t s1, s2;
                rgk_pack_adler_piece([&](uint32_t i) -> uint32_t { return z[rgk_pack_png_pos(i)]; }, start, len, s1, s2);
                uint64_t w1 = 0, w2 = 0; // the definition: sum of b_j, sum of (len - j) * b_j
                for (uint32_t j = 0; j < len; j++) { w1 += raw[start + j]; w2 += (uint64_t)(len - j) * raw[start + j]; }
                CHECK(s1 == w1 && s2 == w2);
                ad.add(s1, s2, len);
            }
            CHECK(ad.value() == adler32_of(raw.data(), raw.size()));
            // CRC-32 of "IDAT" + payload from pieces
            std::vector<uint8_t> chunk = {'I', 'D', 'A', 'T'};
            chunk.insert(chunk.end(), z.begin(), z.end());
            std::vector<uint32_t> crcs;
            for (uint32_t k = 0; k < rgk_pack_pieces(chunk.size(), seg); k++) {
                const uint32_t start = k * seg, left = (uint32_t)chunk.size() - start;
                crcs.push_back(rgk_pack_crc_piece(table, [&](uint32_t j) -> uint32_t { return j < 4u ? rgk_pack_idat_type_byte(j) : z[j - 4u]; }, start, left < seg ? left : seg));
                CHECK(crcs.back() == crc32_of(chunk.data() + start, left < seg ? left : seg));
            }
            const uint32_t crc = rgk_pack_crc_fold(crcs.data(), chunk.size(), seg);
            CHECK(crc == crc32_of(chunk.data(), chunk.size()));
            const uint8_t more[4] = {1, 2, 0xfe, 0xff};
            chunk.insert(chunk.end(), more, more + 4);
            CHECK(rgk_pack_crc_more(table, crc, more, 4) == crc32_of(chunk.data(), chunk.size()));
        }
    }
    for (uint64_t len : {0ull, 1ull, 4096ull, 0x7fffffffull}) { // the operator against zero bytes fed to the register
        const RgkPackCrcShift op(len);
        if (len > 4096) continue; // (built: no shift count out of range)
        const std::vector<uint8_t> a = {'a', 'b', 'c'}, zeros((size_t)len, 0);
        std::vector<uint8_t> both = a;
        both.insert(both.end(), zeros.begin(), zeros.end());
        CHECK((op.apply(crc32_of(a.data(), 3)) ^ crc32_of(zeros.data(), zeros.size())) == crc32_of(both.data(), both.size()));
    }
}
static void png(const std::string& dir) {
    uint32_t table[256];
    rgk_pack_crc_table(table);
    const uint32_t sizes[][2] = {{1, 1}, {3, 2}, {67, 45}, {150, 150}, {28, 772}, {21845, 1}};
    for (const auto& sz : sizes) {
        const uint32_t W = sz[0], H = sz[1];
        std::vector<uint32_t> rgba((size_t)W * H);
        for (uint32_t& w : rgba) w = (uint32_t)rnd();
        const std::string path = dir + "/ref.png";
        CHECK(rgk_output_write_png(path.c_str(), W, H, rgba.data()) == RGK_OK);
        const std::vector<uint8_t> want = read_file(path);
        CHECK(rgk_pack_png_fits(W, H));
        const uint32_t raw = (uint32_t)rgk_pack_png_raw_bytes(W, H), payload = (uint32_t)rgk_pack_png_payload_bytes(raw);
        std::vector<uint8_t> got(RGK_PACK_PNG_LEAD + payload + RGK_PACK_PNG_TAIL + 8, 0xA5);
        rgk_pack_png_lead(got.data(), table, W, H, payload);
        uint8_t* const z = got.data() + RGK_PACK_PNG_LEAD;
        for (uint32_t j = 0; j < payload; j++) z[j] = (uint8_t)rgk_pack_png_payload_byte(rgba.data(), W, raw, j); // k_out_pack_png
        RgkPackAdler ad; // k_out_png_sums and the host's folds
        for (uint32_t k = 0; k < rgk_pack_pieces(raw, RGK_PACK_SEGMENT); k++) {
            const uint32_t start = k * RGK_PACK_SEGMENT, len = raw - start < RGK_PACK_SEGMENT ? raw - start : RGK_PACK_SEGMENT;
            uint32_t s1, s2;
            rgk_pack_adler_piece([&](uint32_t i) -> uint32_t { return z[rgk_pack_png_pos(i)]; }, start, len, s1, s2);
            ad.add(s1, s2, len);
        }
        std::vector<uint32_t> crcs;
        for (uint32_t k = 0; k < rgk_pack_pieces((uint64_t)payload + 4u, RGK_PACK_SEGMENT); k++) {
            const uint32_t start = k * RGK_PACK_SEGMENT, left = payload + 4u - start;
            crcs.push_back(rgk_pack_crc_piece(table, [&](uint32_t j) -> uint32_t { return j < 4u ? rgk_pack_idat_type_byte(j) : z[j - 4u]; }, start,
                                              left < RGK_PACK_SEGMENT ? left : RGK_PACK_SEGMENT));
        }
        rgk_pack_png_tail(z + payload, table, ad.value(), rgk_pack_crc_fold(crcs.data(), (uint64_t)payload + 4u, RGK_PACK_SEGMENT));
        for (size_t i = RGK_PACK_PNG_LEAD + payload + RGK_PACK_PNG_TAIL; i < got.size(); i++) CHECK(got[i] == 0xA5);
        got.resize(RGK_PACK_PNG_LEAD + payload + RGK_PACK_PNG_TAIL);
        CHECK(got == want);
    }
    // raw byte 65535 of 28 x 772 is a filter byte: 85 divides 65535
    CHECK(65535u % (3u * 28u + 1u) == 0u);
    // the limits of rgk_output_write_png
    const uint32_t one = 0;
    CHECK(!rgk_pack_png_fits(0, 1) && !rgk_pack_png_fits(1, 0) && !rgk_pack_png_fits(0x80000000u, 1) && !rgk_pack_png_fits(26800, 26800) && rgk_pack_png_fits(26700, 26700));
    CHECK(rgk_output_write_png((dir + "/big.png").c_str(), 26800, 26800, &one) == RGK_ERR_INVALID);
}

int main(int argc, char** argv) {
    const std::string which = argc > 1 ? argv[1] : "", dir = argc > 2 ? argv[2] : ".";
    if (which == "half") half();
    else if (which == "pixel") pixel();
    else if (which == "scale") scale();
    else if (which == "exr") exr(dir);
    else if (which == "checksums") checksums();
    else if (which == "png") png(dir);
    else { std::fprintf(stderr, "usage: pack_main half|pixel|scale|exr|checksums|png [directory]\n"); return 2; }
    if (failures) std::fprintf(stderr, "%d condition(s) failed\n", failures);
    return failures ? 1 : 0;
}
