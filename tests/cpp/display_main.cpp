// The display stage's GPU-free parts on the CPU: this file includes rgk_amd/csrc/rgk_display.h -- the functions the two kernels call,
// the table and the solve -- and rgk_amd/csrc/rgk_output.cpp (the PNG writer with its two checksums), nothing that needs the HIP
// runtime, and links without it.  Expected values are written out by hand from the definition in include/rgk.h.
// Usage: display_main <case> [directory for the files the png case writes]; exit status 0 = every condition held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rgk_amd/csrc/rgk_display.h"
#include "../../rgk_amd/csrc/rgk_output.cpp"

extern "C" int rgk_internal_fail(int code, const char*) { return code; } // (rgk_commit.cpp's in the library)

static int failures = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
    } while (0)

static bool same(float a, float b) { return rgk_display_bits(a) == rgk_display_bits(b); }
static float below(float x) { return rgk_display_float(rgk_display_bits(x) - 1u); } // x > 0

static rgk_display_params params(float exposure = 0.0f, float white = 0.0f, uint32_t permille = 995) { return {RGK_DISPLAY_REINHARD, exposure, 0.18f, permille, white}; }

static void colour() {
    const float inf = INFINITY, nan = NAN;
    RgkDisplayRgb c = rgk_display_colour(nan, -1.0f, inf, false, 7);
    CHECK(same(c.r, 0.0f) && same(c.g, 0.0f) && c.b == inf);
    c = rgk_display_colour(3.0f, 6.0f, 9.0f, true, 3);
    CHECK(c.r == 1.0f && c.g == 2.0f && c.b == 3.0f);
    c = rgk_display_colour(3.0f, nan, inf, true, 0);
    CHECK(same(c.r, 0.0f) && same(c.g, 0.0f) && same(c.b, 0.0f));
    c = rgk_display_colour(-0.0f, 1e-30f, -inf, true, 1);
    CHECK(same(c.r, 0.0f) && c.g == 1e-30f && same(c.b, 0.0f));
    CHECK(same(rgk_display_lum({1.0f, 1.0f, 1.0f}), (0.2126f + 0.7152f) + 0.0722f));
    CHECK(rgk_display_lum({0.0f, 0.0f, inf}) == inf);
    // bins: 8 per octave from 2^-20; the edges are where the exponent or the mantissa's top three bits change
    CHECK(rgk_display_bin(1.0f) == 160 && rgk_display_bin(below(1.0f)) == 159 && rgk_display_bin(1.125f) == 161 && rgk_display_bin(below(1.125f)) == 160);
    CHECK(rgk_display_bin(std::ldexp(1.0f, -20)) == 0 && rgk_display_bin(below(std::ldexp(1.0f, -20))) == 0 && rgk_display_bin(1e-30f) == 0 && rgk_display_bin(1e-45f) == 0);
    CHECK(rgk_display_bin(std::ldexp(1.125f, -20)) == 1);
    CHECK(rgk_display_bin(4096.0f) == 255 && rgk_display_bin(below(4096.0f)) == 255 && rgk_display_bin(3840.0f) == 255 && rgk_display_bin(below(3840.0f)) == 254);
    CHECK(rgk_display_bin(1e30f) == 255 && rgk_display_bin(inf) == 255);
    CHECK(rgk_display_edge(0) == std::ldexp(1.0f, -20) && rgk_display_edge(160) == 1.0f && rgk_display_edge(161) == 1.125f && rgk_display_edge(255) == 3840.0f && rgk_display_edge(256) == 4096.0f);
    for (int b = 0; b < 256; b++) CHECK(rgk_display_bin(rgk_display_edge(b)) == b && (b == 0 || rgk_display_bin(below(rgk_display_edge(b))) == b - 1));
    // curves
    CHECK(rgk_display_expose(2.0f, inf) == 65504.0f && rgk_display_expose(0.5f, 3.0f) == 1.5f);
    CHECK(rgk_display_linear(2.0f) == 1.0f && rgk_display_linear(0.25f) == 0.25f);
    CHECK(same(rgk_display_filmic(0.0f), 0.0f) && rgk_display_filmic(65504.0f) == 1.0f);
    CHECK(same(rgk_display_filmic(0.5f), (0.5f * (2.51f * 0.5f + 0.03f)) / (0.5f * (2.43f * 0.5f + 0.59f) + 0.14f)));
    const float L1 = (0.2126f + 0.7152f) + 0.0722f;
    CHECK(same(rgk_display_reinhard_scale({1.0f, 1.0f, 1.0f}, 2.0f), (1.0f + L1 / 4.0f) / (1.0f + L1)));
    RgkDisplayRgb v = rgk_display_curve(RGK_DISPLAY_REINHARD, {1.0f, 0.0f, inf}, 1.0f, 1e30f); // white^2 overflows: L / inf == 0
    const float L2 = (0.2126f * 1.0f + 0.7152f * 0.0f) + 0.0722f * 65504.0f;
    CHECK(same(v.r, 1.0f * (1.0f / (1.0f + L2))) && same(v.g, 0.0f) && v.b == 1.0f);
    v = rgk_display_curve(RGK_DISPLAY_LINEAR, {0.25f, 2.0f, 0.0f}, 2.0f, 1.0f);
    CHECK(v.r == 0.5f && v.g == 1.0f && same(v.b, 0.0f));
}

static void solve() {
    rgk_display_stats st;
    uint32_t h[256];
    auto clear = [&] { std::memset(h, 0, sizeof h); std::memset(&st, 0xAB, sizeof st); };
    // one pixel, luminance in [1, 1.125): both ranks are 1; the median is the middle of the bin
    clear(); h[160] = 1;
    CHECK(rgk_display_solve_hist(h, 5, params(), st));
    CHECK(st.n_lit == 1 && st.n_dark == 5 && st.hist[160] == 1 && st.hist[0] == 0 && st.hist[255] == 0);
    CHECK(st.y_median == 1.0625f && st.y_white == 1.125f && same(st.exposure, 0.18f / 1.0625f) && st.white == 1.0f);
    // all pixels in one bin: rank 500 of 1000 lies 499.5 / 1000 into it; the white rank 995 is in the same bin
    clear(); h[160] = 1000;
    CHECK(rgk_display_solve_hist(h, 0, params(), st));
    CHECK(st.n_lit == 1000 && same(st.y_median, 1.0f + 0.125f * (499.5f / 1000.0f)) && st.y_white == 1.125f);
    CHECK(same(st.exposure, 0.18f / st.y_median) && st.white == 1.0f);
    // bin 0, what lies below 2^-20 too: edges 2^-20 and 1.125 * 2^-20; rank 2 of 4 is 1.5 / 4 into it
    clear(); h[0] = 4;
    CHECK(rgk_display_solve_hist(h, 0, params(), st));
    CHECK(st.y_median == std::ldexp(1.046875f, -20) && st.y_white == std::ldexp(1.125f, -20) && same(st.exposure, 0.18f / std::ldexp(1.046875f, -20)) && st.white == 1.0f);
    // bin 255: edges 3840 and 4096; rank 1 of 2 is a quarter into it; the white rank (2 * 995 + 999) / 1000 = 2
    clear(); h[255] = 2;
    CHECK(rgk_display_solve_hist(h, 0, params(), st));
    CHECK(st.y_median == 3904.0f && st.y_white == 4096.0f && same(st.exposure, 0.18f / 3904.0f) && st.white == 1.0f);
    // two equal halves: the median rank 10 of 20 is the LAST pixel of the lower half (bin 100: 1.5 * 2^-8 .. 1.625 * 2^-8),
    // the white rank 20 is in the upper (bin 200, upper edge 36)
    clear(); h[100] = 10; h[200] = 10;
    CHECK(rgk_display_solve_hist(h, 0, params(), st));
    const float lo = std::ldexp(1.5f, -8), hi = std::ldexp(1.625f, -8), ym = lo + (hi - lo) * (9.5f / 10.0f);
    CHECK(same(st.y_median, ym) && st.y_white == 36.0f && same(st.exposure, 0.18f / ym) && same(st.white, (0.18f / ym) * 36.0f) && st.white > 1000.0f);
    CHECK(rgk_display_solve_hist(h, 0, params(0.0f, 0.0f, 500), st)); // half the lit pixels at or below white: rank 10, the lower bin
    CHECK(st.y_white == hi && same(st.y_median, ym) && st.white == 1.0f);
    CHECK(rgk_display_solve_hist(h, 0, params(0.0f, 0.0f, 1), st));   // rank max(1, (20 + 999) / 1000) = 1
    CHECK(st.y_white == hi);
    CHECK(rgk_display_solve_hist(h, 0, params(0.25f, 0.0f), st));     // a fixed exposure: the measurement is reported, the white follows the exposure
    CHECK(st.exposure == 0.25f && same(st.y_median, ym) && st.white == 9.0f);
    CHECK(rgk_display_solve_hist(h, 0, params(0.25f, 3.5f), st));
    CHECK(st.exposure == 0.25f && st.white == 3.5f);
    // nothing lit
    clear();
    CHECK(rgk_display_solve_hist(h, 9, params(), st));
    CHECK(st.n_lit == 0 && st.n_dark == 9 && same(st.y_median, 0.0f) && same(st.y_white, 0.0f) && st.exposure == 1.0f && st.white == 1.0f);
    CHECK(rgk_display_solve_hist(h, 9, params(2.0f, 3.0f), st));
    CHECK(st.exposure == 2.0f && st.white == 3.0f);
    // counts beyond 32 bits in all are refused; 64-bit ranks below that
    clear(); h[3] = 0xffffffffu; h[4] = 1;
    CHECK(!rgk_display_solve_hist(h, 0, params(), st));
    h[4] = 0;
    CHECK(rgk_display_solve_hist(h, 0, params(), st) && st.n_lit == 0xffffffffu && st.y_white == rgk_display_edge(4));
    // the checks
    rgk_display_params p = params();
    CHECK(rgk_display_check_params(&p) == nullptr && rgk_display_check_params(nullptr) != nullptr);
    p.op = 3; CHECK(rgk_display_check_params(&p)); p = params();
    p.key = 0.0f; CHECK(rgk_display_check_params(&p)); p.key = NAN; CHECK(rgk_display_check_params(&p)); p.key = INFINITY; CHECK(rgk_display_check_params(&p)); p = params();
    p.exposure = NAN; CHECK(rgk_display_check_params(&p)); p.exposure = -INFINITY; CHECK(rgk_display_check_params(&p)); p.exposure = -1.0f; CHECK(!rgk_display_check_params(&p)); p = params();
    p.white = INFINITY; CHECK(rgk_display_check_params(&p)); p = params();
    p.white_permille = 0; CHECK(rgk_display_check_params(&p)); p.white_permille = 1001; CHECK(rgk_display_check_params(&p)); p.white_permille = 1000; CHECK(!rgk_display_check_params(&p));
    CHECK(!rgk_display_check_scale(1.0f, 1.0f) && rgk_display_check_scale(0.0f, 1.0f) && rgk_display_check_scale(1.0f, -1.0f) && rgk_display_check_scale(NAN, 1.0f) && rgk_display_check_scale(1.0f, INFINITY));
}

static void byte() {
    float T[256];
    rgk_display_build_table(T);
    CHECK(same(T[0], 0.0f));
    for (int k = 1; k < 256; k++) {
        CHECK(T[k] > T[k - 1]);
        CHECK(rgk_display_byte(T, T[k]) == (uint32_t)k);         // at the threshold: the byte is k
        CHECK(rgk_display_byte(T, below(T[k])) == (uint32_t)k - 1); // the float just below it: k - 1
    }
    CHECK(rgk_display_byte(T, 0.0f) == 0 && rgk_display_byte(T, 1.0f) == 255 && rgk_display_byte(T, 65504.0f) == 255);
    CHECK(same(T[1], (float)(0.5 / 255.0 / 12.92)) && T[255] < 1.0f && T[255] > 0.99f);
    CHECK(rgk_display_byte(T, 0.5f) == 188 && rgk_display_byte(T, 0.18f) == 118); // round(255 * srgb(0.5)) = 188, of 0.18: 118
    CHECK(rgk_display_word(T, {0.0f, 1.0f, 0.5f}) == 0xffbcff00u);
}

static void checksums() {
    CHECK(crc32_of((const uint8_t*)"IEND", 4) == 0xAE426082u);
    CHECK(adler32_of((const uint8_t*)"Wikipedia", 9) == 0x11E60398u);
    CHECK(crc32_of(nullptr, 0) == 0 && adler32_of(nullptr, 0) == 1);
    CHECK(crc32_of((const uint8_t*)"123456789", 9) == 0xCBF43926u); // the check value of CRC-32/ISO-HDLC
    std::vector<uint8_t> big(100000, 0xff);                         // past 5552 bytes: the sums are reduced in time
    uint32_t a = 1, b = 0;
    for (uint8_t v : big) { a = (a + v) % 65521u; b = (b + a) % 65521u; }
    CHECK(adler32_of(big.data(), big.size()) == ((b << 16) | a));
}

static std::vector<uint8_t> slurp(const std::string& path) {
    std::vector<uint8_t> v;
    if (FILE* f = std::fopen(path.c_str(), "rb")) {
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
        std::fclose(f);
    }
    return v;
}
static uint32_t be(const std::vector<uint8_t>& v, size_t at) { return ((uint32_t)v[at] << 24) | ((uint32_t)v[at + 1] << 16) | ((uint32_t)v[at + 2] << 8) | v[at + 3]; }

static void png(const std::string& dir) {
    // 1 x 1: signature 8, IHDR 25, IDAT 12 + (2 + 5 + 4 + 4), IEND 12
    const uint32_t one = 0x7f332211u; // R 0x11, G 0x22, B 0x33; the fourth byte is dropped
    const std::string p1 = dir + "/one.png";
    CHECK(rgk_output_write_png(p1.c_str(), 1, 1, &one) == RGK_OK);
    const std::vector<uint8_t> f = slurp(p1);
    CHECK(f.size() == 72);
    if (f.size() == 72) {
        const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
        CHECK(!std::memcmp(f.data(), sig, 8));
        CHECK(be(f, 8) == 13 && !std::memcmp(&f[12], "IHDR", 4) && be(f, 16) == 1 && be(f, 20) == 1);
        const uint8_t rest[5] = {8, 2, 0, 0, 0};
        CHECK(!std::memcmp(&f[24], rest, 5) && be(f, 29) == crc32_of(&f[12], 17));
        // zlib header, one final stored block of 4 bytes (LEN 4, NLEN ~4), the filter byte and R, G, B
        const uint8_t idat[11] = {0x78, 0x01, 0x01, 0x04, 0x00, 0xfb, 0xff, 0x00, 0x11, 0x22, 0x33};
        CHECK(be(f, 33) == 15 && !std::memcmp(&f[37], "IDAT", 4) && !std::memcmp(&f[41], idat, 11));
        // Adler-32 of {0, 0x11, 0x22, 0x33}: a runs 1, 0x12, 0x34, 0x67; b is their sum 0xae
        CHECK(be(f, 52) == 0x00ae0067u);
        CHECK(be(f, 56) == crc32_of(&f[37], 19));
        CHECK(be(f, 60) == 0 && !std::memcmp(&f[64], "IEND", 4) && be(f, 68) == 0xAE426082u);
    }
    // 21845 x 1: the row is 1 + 65535 bytes, one more than a stored block holds
    const uint32_t W = 21845;
    std::vector<uint32_t> row(W);
    for (uint32_t x = 0; x < W; x++) row[x] = x * 2654435761u;
    const std::string p2 = dir + "/wide.png";
    CHECK(rgk_output_write_png(p2.c_str(), W, 1, row.data()) == RGK_OK);
    const std::vector<uint8_t> g = slurp(p2);
    const size_t zlen = 2 + 5 + 65535 + 5 + 1 + 4;
    CHECK(g.size() == 8 + 25 + 12 + zlen + 12);
    if (g.size() == 8 + 25 + 12 + zlen + 12) {
        CHECK(be(g, 16) == W && be(g, 20) == 1 && be(g, 33) == zlen);
        const size_t z = 41;
        const uint8_t first[5] = {0x00, 0xff, 0xff, 0x00, 0x00}, last[5] = {0x01, 0x01, 0x00, 0xfe, 0xff};
        CHECK(g[z] == 0x78 && g[z + 1] == 0x01 && !std::memcmp(&g[z + 2], first, 5) && g[z + 7] == 0 /* the filter byte */);
        CHECK(!std::memcmp(&g[z + 7 + 65535], last, 5));
        CHECK(g[z + 8] == (row[0] & 0xff) && g[z + 7 + 65535 + 5] == ((row[W - 1] >> 16) & 0xff)); // first R; last B, alone in the second block
        std::vector<uint8_t> raw(1, 0);
        for (uint32_t x = 0; x < W; x++) for (int s = 0; s < 24; s += 8) raw.push_back((uint8_t)(row[x] >> s));
        CHECK(be(g, z + zlen - 4) == adler32_of(raw.data(), raw.size()));
        CHECK(be(g, z + zlen) == crc32_of(&g[37], 4 + zlen));
    }
    // refusals
    CHECK(rgk_output_write_png((dir + "/no-such-directory/x.png").c_str(), 1, 1, &one) == RGK_ERR_INVALID);
    CHECK(rgk_output_write_png(nullptr, 1, 1, &one) == RGK_ERR_INVALID && rgk_output_write_png(p1.c_str(), 1, 1, nullptr) == RGK_ERR_INVALID);
    CHECK(rgk_output_write_png(p1.c_str(), 0, 1, &one) == RGK_ERR_INVALID && rgk_output_write_png(p1.c_str(), 1, 0, &one) == RGK_ERR_INVALID);
    CHECK(rgk_output_write_png(p1.c_str(), 0x80000000u, 1, &one) == RGK_ERR_INVALID);
    CHECK(rgk_output_write_png(p1.c_str(), 40000, 40000, &one) == RGK_ERR_INVALID); // 4.8 GB: refused before a pixel is read
}

int main(int argc, char** argv) {
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "colour") colour();
    else if (c == "solve") solve();
    else if (c == "byte") byte();
    else if (c == "checksums") checksums();
    else if (c == "png" && argc > 2) png(argv[2]);
    else { std::fprintf(stderr, "usage: %s colour|solve|byte|checksums|png <directory>\n", argv[0]); return 2; }
    if (failures) std::fprintf(stderr, "%d condition(s) failed\n", failures);
    return failures ? 1 : 0;
}
