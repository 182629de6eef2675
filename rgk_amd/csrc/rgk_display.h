// The display stage's arithmetic (rgk.h "display output"), written once for the kernels (rgk_post.hip: k_display_hist,
// k_display_encode) and the host (rgk_post_host.cpp: the solve, the table, the argument checks).  Like rgk_tree.h: pure functions
// marked RGK_HD (rgk_libm.h) that call nothing of the HIP runtime, so the unit builds with any host compiler and what the device
// runs here is the source tests/cpp/display_main.cpp runs under sanitizers.  Float32, + - * / and comparisons only, compiled
// without contraction on both sides; the one transcendental call, pow in the table, is host code in double.
#pragma once
#include <stdint.h>

#include <cmath> // the host part at the end: pow for the table, isfinite for the checks

#include "../../include/rgk.h"
#include "../../include/rgk_libm.h"

constexpr int RGK_DISPLAY_BINS = 256;
constexpr int RGK_DISPLAY_BIAS = (127 - 20) << 3; // bits >> 20 of 2^-20: bin 0's lower edge
constexpr uint32_t RGK_DISPLAY_HIST_WORDS = RGK_DISPLAY_BINS + 1; // the device histogram: the bins, then n_dark
constexpr float RGK_DISPLAY_MAX = 65504.0f;       // the largest exposed value a curve is given (the largest half)

RGK_HD uint32_t rgk_display_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
RGK_HD float rgk_display_float(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
RGK_HD float rgk_display_min(float a, float b) { return a < b ? a : b; }

// ------------------------------------------------------------------ the input colour
struct RgkDisplayRgb {
    float r, g, b;
};
RGK_HD float rgk_display_pos(float c) { return c > 0.0f ? c : 0.0f; } // NaN, negatives and -0 -> +0
// `counted`: the image comes with a count plane (n its pixel's count); else it is a mean already and n is not read
RGK_HD RgkDisplayRgb rgk_display_colour(float r, float g, float b, bool counted, uint32_t n) {
    if (counted) {
        if (n == 0) return {0.0f, 0.0f, 0.0f};
        const float fn = (float)n;
        r = r / fn; g = g / fn; b = b / fn;
    }
    return {rgk_display_pos(r), rgk_display_pos(g), rgk_display_pos(b)};
}
RGK_HD float rgk_display_lum(RgkDisplayRgb c) {
    const float tr = 0.2126f * c.r, tg = 0.7152f * c.g, tb = 0.0722f * c.b;
    return (tr + tg) + tb;
}

// ------------------------------------------------------------------ the histogram's bins
// Y > 0 (+inf too); 8 bins per octave: the exponent and the mantissa's top three bits
RGK_HD int rgk_display_bin(float Y) {
    const int b = (int)(rgk_display_bits(Y) >> 20) - RGK_DISPLAY_BIAS;
    return b < 0 ? 0 : (b > RGK_DISPLAY_BINS - 1 ? RGK_DISPLAY_BINS - 1 : b);
}
// lower edge of bin 0 .. 256 (256: the upper edge of the last bin, 4096)
RGK_HD float rgk_display_edge(int bin) { return rgk_display_float((uint32_t)(bin + RGK_DISPLAY_BIAS) << 20); }

// ------------------------------------------------------------------ the curves: an exposed colour x -> v in [0, 1]
RGK_HD float rgk_display_expose(float exposure, float c) { return rgk_display_min(exposure * c, RGK_DISPLAY_MAX); }
RGK_HD float rgk_display_linear(float x) { return rgk_display_min(x, 1.0f); }
RGK_HD float rgk_display_filmic(float x) {
    const float num = x * (2.51f * x + 0.03f), den = x * (2.43f * x + 0.59f) + 0.14f;
    return rgk_display_min(num / den, 1.0f);
}
// the factor all three channels of a pixel share
RGK_HD float rgk_display_reinhard_scale(RgkDisplayRgb x, float white) {
    const float L = rgk_display_lum(x);
    return (1.0f + L / (white * white)) / (1.0f + L);
}
RGK_HD RgkDisplayRgb rgk_display_curve(uint32_t op, RgkDisplayRgb c, float exposure, float white) {
    const RgkDisplayRgb x = {rgk_display_expose(exposure, c.r), rgk_display_expose(exposure, c.g), rgk_display_expose(exposure, c.b)};
    if (op == RGK_DISPLAY_LINEAR) return {rgk_display_linear(x.r), rgk_display_linear(x.g), rgk_display_linear(x.b)};
    if (op == RGK_DISPLAY_FILMIC) return {rgk_display_filmic(x.r), rgk_display_filmic(x.g), rgk_display_filmic(x.b)};
    const float s = rgk_display_reinhard_scale(x, white);
    return {rgk_display_min(x.r * s, 1.0f), rgk_display_min(x.g * s, 1.0f), rgk_display_min(x.b * s, 1.0f)};
}

// ------------------------------------------------------------------ the byte
// The number of k in 1 .. 255 with v >= T[k], T increasing: the largest such k, by eight halvings (128 + 64 + .. + 1 = 255, so no
// step looks past the table).  v is never NaN: a curve's input is finite and >= 0.
RGK_HD uint32_t rgk_display_byte(const float* T, float v) {
    uint32_t k = 0;
    for (uint32_t step = 128; step; step >>= 1)
        if (v >= T[k + step]) k += step;
    return k;
}
// bytes R, G, B, 255 in memory order (little endian)
RGK_HD uint32_t rgk_display_word(const float* T, RgkDisplayRgb v) {
    return rgk_display_byte(T, v.r) | (rgk_display_byte(T, v.g) << 8) | (rgk_display_byte(T, v.b) << 16) | 0xff000000u;
}

// ------------------------------------------------------------------ host only: the table, the checks, the solve
inline void rgk_display_build_table(float* T /*256*/) {
    T[0] = 0.0f;
    for (int k = 1; k < 256; k++) {
        const double s = ((double)k - 0.5) / 255.0;
        T[k] = (float)(s <= 0.04045 ? s / 12.92 : std::pow((s + 0.055) / 1.055, 2.4));
    }
}

// NULL, or what is wrong with a parameter set
inline const char* rgk_display_check_params(const rgk_display_params* p) {
    if (!p) return "null argument";
    if (p->op != RGK_DISPLAY_LINEAR && p->op != RGK_DISPLAY_REINHARD && p->op != RGK_DISPLAY_FILMIC) return "op must be one of RGK_DISPLAY_LINEAR, _REINHARD, _FILMIC";
    if (!std::isfinite(p->exposure) || !std::isfinite(p->white)) return "exposure and white must be finite";
    if (!std::isfinite(p->key) || !(p->key > 0.0f)) return "key must be > 0 and finite";
    if (p->white_permille < 1 || p->white_permille > 1000) return "white_permille must be 1 .. 1000";
    return nullptr;
}
// ... with the two numbers an encode runs with
inline const char* rgk_display_check_scale(float exposure, float white) {
    if (!std::isfinite(exposure) || !(exposure > 0.0f) || !std::isfinite(white) || !(white > 0.0f)) return "the exposure and the white point must be > 0 and finite";
    return nullptr;
}

// The first bin whose running sum reaches `rank` (1 <= rank <= the sum of all bins); *before: the sum below that bin.
inline int rgk_display_rank_bin(const uint32_t* hist, uint64_t rank, uint64_t* before) {
    uint64_t sum = 0;
    for (int b = 0; b < RGK_DISPLAY_BINS; b++) {
        if (sum + hist[b] >= rank) { *before = sum; return b; }
        sum += hist[b];
    }
    *before = sum - hist[RGK_DISPLAY_BINS - 1];
    return RGK_DISPLAY_BINS - 1; // (not reached for a rank in range)
}

// rgk.h's solve; `p` checked by the caller.  false: the counts do not fit n_lit.
inline bool rgk_display_solve_hist(const uint32_t* hist, uint32_t n_dark, const rgk_display_params& p, rgk_display_stats& st) {
    uint64_t N = 0;
    for (int b = 0; b < RGK_DISPLAY_BINS; b++) { st.hist[b] = hist[b]; N += hist[b]; }
    if (N > 0xffffffffull) return false;
    st.n_lit = (uint32_t)N;
    st.n_dark = n_dark;
    st.y_median = st.y_white = 0.0f;
    float exposure = 1.0f, white = 1.0f;
    if (N) {
        const uint64_t rank_m = (N + 1) / 2;
        uint64_t rank_w = (N * p.white_permille + 999) / 1000;
        if (rank_w < 1) rank_w = 1;
        uint64_t before = 0;
        st.y_white = rgk_display_edge(rgk_display_rank_bin(hist, rank_w, &before) + 1);
        const int b = rgk_display_rank_bin(hist, rank_m, &before);
        const float lo = rgk_display_edge(b), hi = rgk_display_edge(b + 1);
        const float t = ((float)(rank_m - before) - 0.5f) / (float)hist[b];
        st.y_median = lo + (hi - lo) * t;
        exposure = p.key / st.y_median;
    }
    if (p.exposure > 0.0f) exposure = p.exposure;
    if (N) white = exposure * st.y_white > 1.0f ? exposure * st.y_white : 1.0f;
    if (p.white > 0.0f) white = p.white;
    st.exposure = exposure;
    st.white = white;
    return true;
}
