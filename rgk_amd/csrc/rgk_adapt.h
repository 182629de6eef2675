// Adaptive tile sampling, the part that needs no device: which tiles of a frame the next round still renders.
// Plain C++17 over the noise estimate's per-tile statistics (rgk.h rgk_noise_tile) -- no call into the HIP runtime -- so the unit
// builds with any host compiler and runs under sanitizers (tests/cpp/adapt_main.cpp includes it and rgk_plan.h alone).
// tests/adapt_ref.py restates the rule in numpy; the two agree mask for mask.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/rgk.h" // rgk_noise_tile, rgk_adapt_params

// What is wrong with a call's arguments (the text rgk_last_error then gives), or nullptr.
inline const char* rgk_adapt_check(const rgk_noise_tile* tiles, const uint32_t* visits, uint32_t xres, uint32_t yres, uint32_t tile_size,
                                   const rgk_adapt_params* prm, const uint8_t* live) {
    if (!tiles || !visits || !prm || !live) return "null argument";
    if (xres == 0 || yres == 0 || xres > 65535 || yres > 65535) return "resolution out of range";
    if (tile_size == 0) return "tile_size must be >= 1";
    if (!std::isfinite(prm->target) || !(prm->target >= 0.0f)) return "target must be finite and >= 0";
    if (prm->min_visits < 2) return "min_visits must be >= 2 (a tile is not estimable before its second visit)";
    return nullptr;
}

struct RgkAdaptResult { uint32_t n_live; bool done; };

// The rule, on checked arguments.  All arithmetic in double; the tiles are added in row-major order, as RenderDriver.noise() adds them.
//   SV = sum of sum_var, SQ = sum of sum_sq, NE = sum of n_estimable
//   done:   NE > 0 and SV <= target^2 * SQ                      (rel <= target: the criterion of --until-noise)
//   live_t: visits_t < min_visits,  or  n_estimable_t == 0 (every tile of the grid has pixels),
//           or  sum_var_t > (target^2 * SQ) * (n_estimable_t / NE)
// The allowance is the frame's, shared out by estimable pixels: a tile is live while its mean per-pixel variance is above the
// frame-wide per-pixel allowance.  Normalised by the frame's energy, not the tile's own: a dark tile retires, and in a black frame
// (SQ == 0) nothing is live beyond min_visits.  Nothing live: done, whatever the last place of SV says (the allowances sum to
// target^2 * SQ only up to rounding).  Stateless: a tile retired for one round is judged afresh after it.
inline RgkAdaptResult rgk_adapt_rule(const rgk_noise_tile* tiles, const uint32_t* visits, uint32_t xres, uint32_t yres, uint32_t tile_size,
                                     const rgk_adapt_params& prm, uint8_t* live) {
    const size_t n = (size_t)(((uint64_t)xres + tile_size - 1) / tile_size) * (size_t)(((uint64_t)yres + tile_size - 1) / tile_size);
    double SV = 0.0, SQ = 0.0;
    uint64_t NE = 0;
    for (size_t t = 0; t < n; t++) { SV += tiles[t].sum_var; SQ += tiles[t].sum_sq; NE += tiles[t].n_estimable; }
    const double allowance = ((double)prm.target * (double)prm.target) * SQ;
    RgkAdaptResult r = {0u, NE > 0 && SV <= allowance};
    for (size_t t = 0; t < n; t++) {
        const bool l = visits[t] < prm.min_visits || tiles[t].n_estimable == 0 ||
                       tiles[t].sum_var > allowance * ((double)tiles[t].n_estimable / (double)NE); // (n_estimable_t > 0 here, so NE > 0)
        live[t] = l ? 1 : 0;
        r.n_live += l ? 1u : 0u;
    }
    if (r.n_live == 0) r.done = true;
    return r;
}

// ------------------------------------------------------------------ the tile list of a round fold (rgk_round_fold_device)
// Every tile in the frame and non-empty, no two overlapping: what is wrong (`bad`: the tile it was found at), or nullptr.
// `max_height`: the list's highest tile, which sizes the grid (rgk_plan.h rgk_fold_grid).  Sorted by top row, a tile can only overlap
// the ones that start above its bottom row: a frame's tile grid costs its tiles times a tile row's length, not their square.
inline const char* rgk_fold_check_tiles(const rgk_tile* tiles, uint32_t n_tiles, uint32_t xres, uint32_t yres, uint32_t& max_height, uint32_t& bad) {
    max_height = 0;
    for (uint32_t i = 0; i < n_tiles; i++) {
        const rgk_tile& t = tiles[i];
        bad = i;
        if (t.x1 > xres || t.y1 > yres || t.x0 > t.x1 || t.y0 > t.y1) return "tile outside the frame";
        if (t.x0 == t.x1 || t.y0 == t.y1) return "empty tile";
        max_height = std::max(max_height, t.y1 - t.y0);
    }
    std::vector<uint32_t> order(n_tiles);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return tiles[a].y0 != tiles[b].y0 ? tiles[a].y0 < tiles[b].y0 : a < b; });
    for (uint32_t i = 0; i < n_tiles; i++) {
        const rgk_tile& a = tiles[order[i]];
        for (uint32_t j = i + 1; j < n_tiles && tiles[order[j]].y0 < a.y1; j++) {
            const rgk_tile& b = tiles[order[j]];
            if (a.x0 < b.x1 && b.x0 < a.x1) { bad = std::max(order[i], order[j]); return "tile overlaps an earlier one"; }
        }
    }
    return nullptr;
}
