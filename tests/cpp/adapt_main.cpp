// The adaptive-sampling unit (rgk_amd/csrc/rgk_adapt.h) and the round fold's grid (rgk_plan.h) on the CPU: this file includes those
// two headers and nothing else of the library, and links without the HIP runtime.  The expected masks are written out by hand from
// the rule's definition (include/rgk.h) on numbers chosen so that every product and quotient is exact in double.
// Usage: adapt_main <case>; exit status 0 = every condition held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../rgk_amd/csrc/rgk_adapt.h"
#include "../../rgk_amd/csrc/rgk_plan.h"

static int failures = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
    } while (0)

struct Frame {
    uint32_t xres, yres, ts;
    std::vector<rgk_noise_tile> tiles;
    std::vector<uint32_t> visits;
    std::vector<uint8_t> live; // one entry more than the frame has tiles: a sentinel the rule must leave alone
    Frame(uint32_t x, uint32_t y, uint32_t t, double sum_var, double sum_sq, uint64_t ne, uint32_t v) : xres(x), yres(y), ts(t) {
        const size_t n = (size_t)((x + t - 1) / t) * ((y + t - 1) / t);
        tiles.assign(n, rgk_noise_tile{sum_var, sum_sq, ne});
        visits.assign(n, v);
        live.assign(n + 1, 0xAB);
    }
    size_t n() const { return tiles.size(); }
    RgkAdaptResult run(float target, uint32_t min_visits) {
        const rgk_adapt_params p = {target, min_visits};
        CHECK(rgk_adapt_check(tiles.data(), visits.data(), xres, yres, ts, &p, live.data()) == nullptr);
        const RgkAdaptResult r = rgk_adapt_rule(tiles.data(), visits.data(), xres, yres, ts, p, live.data());
        CHECK(live[n()] == 0xAB);
        uint32_t c = 0;
        for (size_t i = 0; i < n(); i++) { CHECK(live[i] <= 1); c += live[i]; }
        CHECK(c == r.n_live);
        return r;
    }
    bool only(size_t t) const { // tile t is live and no other
        for (size_t i = 0; i < n(); i++) if (live[i] != (i == t ? 1 : 0)) return false;
        return true;
    }
};

// target 0.5: target^2 = 0.25 exactly
static void known() {
    { // 2 x 2 tiles of 1024 estimable pixels, sum_sq 100 each: allowance 0.25 * 400 = 100, a tile's share 100 * (1024 / 4096) = 25
        Frame f(64, 64, 32, 1.0, 100.0, 1024, 4);
        RgkAdaptResult r = f.run(0.5f, 4); // all retired: done
        CHECK(r.done && r.n_live == 0);
        f.tiles[2].sum_var = 300.0; // one hot tile among cold ones: SV = 303 > 100
        r = f.run(0.5f, 4);
        CHECK(!r.done && r.n_live == 1 && f.only(2));
        f.tiles[2].sum_var = 25.0; // exactly its share: not above it
        r = f.run(0.5f, 4);
        CHECK(r.done && r.n_live == 0);
        f.tiles[2].sum_var = std::nextafter(25.0, 26.0);
        r = f.run(0.5f, 4);
        CHECK(r.done && r.n_live == 1 && f.only(2)); // (the frame as a whole is below the target: done although a tile is above its share)
        f.tiles[2].sum_var = 1.0;
        f.tiles[0].sum_var = 97.0; // SV = 100 exactly: done; SV one place above: not
        r = f.run(0.5f, 4);
        CHECK(r.done && f.only(0));
        f.tiles[0].sum_var = std::nextafter(97.0, 98.0);
        r = f.run(0.5f, 4);
        CHECK(!r.done && f.only(0));
        // visits < min_visits overrides everything
        f.tiles[0].sum_var = 1.0;
        f.visits[3] = 3;
        r = f.run(0.5f, 4);
        CHECK(r.done && r.n_live == 1 && f.only(3));
        r = f.run(0.5f, 3);
        CHECK(r.done && r.n_live == 0);
        r = f.run(0.5f, 5);
        CHECK(r.n_live == 4);
        // target 0: everything with variance is live, and the frame is not done
        r = f.run(0.0f, 2);
        CHECK(!r.done && r.n_live == 4);
    }
    { // a black frame: no energy, no variance -- done, and nothing is live beyond min_visits
        Frame f(96, 96, 32, 0.0, 0.0, 1024, 4);
        RgkAdaptResult r = f.run(0.5f, 4);
        CHECK(r.done && r.n_live == 0);
        f.visits.assign(f.n(), 3);
        r = f.run(0.5f, 4);
        CHECK(r.done && r.n_live == 9);
    }
    { // a tile without an estimable pixel is live however often it was visited
        Frame f(96, 96, 32, 1.0, 100.0, 1024, 9);
        f.tiles[5] = rgk_noise_tile{0.0, 0.0, 0};
        RgkAdaptResult r = f.run(0.5f, 4);
        CHECK(r.n_live == 1 && f.only(5) && r.done); // (SV = 8 <= 0.25 * 800)
        // no estimable pixel anywhere: every tile is live and the frame is not done
        Frame g(96, 96, 32, 0.0, 0.0, 0, 9);
        r = g.run(0.5f, 4);
        CHECK(!r.done && r.n_live == 9);
    }
    { // ragged 67 x 45: 3 x 2 tiles of 32, 14 x 9 tiles of 5; the hot tile is the last one
        Frame f(67, 45, 32, 1.0, 100.0, 64, 4);
        CHECK(f.n() == 6);
        f.tiles[5].sum_var = 1000.0;
        RgkAdaptResult r = f.run(0.5f, 4);
        CHECK(!r.done && r.n_live == 1 && f.only(5));
        Frame g(67, 45, 5, 1.0, 100.0, 64, 4);
        CHECK(g.n() == 126);
        g.tiles[125].sum_var = 1e6;
        r = g.run(0.5f, 4);
        CHECK(!r.done && r.n_live == 1 && g.only(125));
    }
    { // 1 x 1
        Frame f(1, 1, 32, 1.0, 1.0, 1, 4);
        RgkAdaptResult r = f.run(0.5f, 4); // 1 > 0.25
        CHECK(!r.done && r.n_live == 1);
        r = f.run(1.0f, 4);
        CHECK(r.done && r.n_live == 0);
    }
}

static void refuse() {
    Frame f(64, 64, 32, 1.0, 100.0, 1024, 4);
    const auto bad = [&](float target, uint32_t mv) {
        const rgk_adapt_params p = {target, mv};
        return rgk_adapt_check(f.tiles.data(), f.visits.data(), 64, 64, 32, &p, f.live.data()) != nullptr;
    };
    CHECK(!bad(0.5f, 2) && !bad(0.0f, 4));
    CHECK(bad(0.5f, 0) && bad(0.5f, 1));
    CHECK(bad(std::numeric_limits<float>::quiet_NaN(), 4) && bad(std::numeric_limits<float>::infinity(), 4) && bad(-0.5f, 4));
    const rgk_adapt_params p = {0.5f, 4};
    CHECK(rgk_adapt_check(nullptr, f.visits.data(), 64, 64, 32, &p, f.live.data()));
    CHECK(rgk_adapt_check(f.tiles.data(), nullptr, 64, 64, 32, &p, f.live.data()));
    CHECK(rgk_adapt_check(f.tiles.data(), f.visits.data(), 64, 64, 32, nullptr, f.live.data()));
    CHECK(rgk_adapt_check(f.tiles.data(), f.visits.data(), 64, 64, 32, &p, nullptr));
    CHECK(rgk_adapt_check(f.tiles.data(), f.visits.data(), 64, 64, 0, &p, f.live.data()));
    CHECK(rgk_adapt_check(f.tiles.data(), f.visits.data(), 0, 64, 32, &p, f.live.data()));
    CHECK(rgk_adapt_check(f.tiles.data(), f.visits.data(), 64, 65536, 32, &p, f.live.data()));
}

// Every workgroup and thread of the fold's grid, as k_round_fold walks them, over planes of C values per pixel: each element of a
// listed tile exactly once, nothing else at all.
static void cover(uint32_t xres, uint32_t yres, const std::vector<rgk_tile>& list) {
    uint32_t max_h = 0, bad = 0;
    CHECK(rgk_fold_check_tiles(list.data(), (uint32_t)list.size(), xres, yres, max_h, bad) == nullptr);
    const RgkGrid2 g = rgk_fold_grid((uint32_t)list.size(), max_h);
    CHECK(g.x == list.size() && (uint64_t)g.y * RGK_FOLD_ROWS >= max_h && (g.y == 0 || (uint64_t)(g.y - 1) * RGK_FOLD_ROWS < max_h));
    for (uint32_t C = 1; C <= 3; C += 2) {
        std::vector<uint8_t> hits((size_t)xres * yres * C, 0), want(hits.size(), 0);
        for (const rgk_tile& t : list)
            for (uint32_t y = t.y0; y < t.y1; y++)
                for (uint32_t x = t.x0; x < t.x1; x++)
                    for (uint32_t c = 0; c < C; c++) want[((size_t)y * xres + x) * C + c] = 1;
        for (uint32_t bx = 0; bx < g.x; bx++)
            for (uint32_t by = 0; by < g.y; by++) {
                const rgk_tile& t = list[bx];
                const RgkRowRange rr = rgk_fold_band(by, t.y1 - t.y0);
                CHECK(rr.r0 <= rr.r1 && rr.r1 <= t.y1 - t.y0 && rr.r1 - rr.r0 <= RGK_FOLD_ROWS);
                const uint32_t tw = t.x1 - t.x0, n = (rr.r1 - rr.r0) * tw * C;
                for (uint32_t th = 0; th < (uint32_t)RGK_POST_BLOCK; th++)
                    for (uint32_t k = th; k < n; k += RGK_POST_BLOCK) {
                        const size_t e = rgk_fold_element(xres, t.x0, t.y0 + rr.r0, tw, C, k);
                        if (e >= hits.size()) { CHECK(e < hits.size()); return; }
                        hits[e]++;
                    }
            }
        CHECK(hits == want);
    }
}

static std::vector<rgk_tile> grid_tiles(uint32_t xres, uint32_t yres, uint32_t ts) {
    std::vector<rgk_tile> v;
    for (uint32_t y = 0; y < yres; y += ts)
        for (uint32_t x = 0; x < xres; x += ts) v.push_back(rgk_tile{x, std::min(xres, x + ts), y, std::min(yres, y + ts), 0u});
    return v;
}

static void fold() {
    const uint32_t sizes[3][2] = {{96, 96}, {67, 45}, {1, 1}};
    for (const auto& s : sizes) {
        std::vector<rgk_tile> all = grid_tiles(s[0], s[1], 32);
        cover(s[0], s[1], all);
        std::vector<rgk_tile> some; // every second tile, last first
        for (size_t i = all.size(); i-- > 0;) if (i % 2 == 0) some.push_back(all[i]);
        cover(s[0], s[1], some);
        cover(s[0], s[1], grid_tiles(s[0], s[1], 5));
        cover(s[0], s[1], {});
    }
    cover(67, 45, {rgk_tile{3, 67, 1, 45, 0u}, rgk_tile{0, 3, 0, 45, 0u}, rgk_tile{3, 4, 0, 1, 0u}}); // tiles of no grid; one higher than a band, one of a pixel
    // the list's check
    uint32_t max_h = 0, bad = 99;
    std::vector<rgk_tile> l = grid_tiles(96, 96, 32);
    CHECK(rgk_fold_check_tiles(l.data(), 9, 96, 96, max_h, bad) == nullptr && max_h == 32);
    CHECK(rgk_fold_check_tiles(l.data(), 9, 96, 95, max_h, bad) != nullptr && bad == 6); // below the frame
    CHECK(rgk_fold_check_tiles(l.data(), 9, 95, 96, max_h, bad) != nullptr && bad == 2); // right of it
    l.push_back(rgk_tile{31, 33, 70, 71, 0u}); // overlaps tiles 6 and 7
    CHECK(rgk_fold_check_tiles(l.data(), 10, 96, 96, max_h, bad) != nullptr && bad == 9);
    l[9] = l[4]; // a tile twice
    CHECK(rgk_fold_check_tiles(l.data(), 10, 96, 96, max_h, bad) != nullptr && bad == 9);
    l[9] = rgk_tile{10, 10, 0, 5, 0u}; // empty
    CHECK(rgk_fold_check_tiles(l.data(), 10, 96, 96, max_h, bad) != nullptr && bad == 9);
    l[9] = rgk_tile{12, 10, 0, 5, 0u}; // inside out
    CHECK(rgk_fold_check_tiles(l.data(), 10, 96, 96, max_h, bad) != nullptr && bad == 9);
    const rgk_tile touching[2] = {{0, 10, 0, 10, 0u}, {10, 20, 0, 10, 0u}}; // sharing an edge is no overlap
    CHECK(rgk_fold_check_tiles(touching, 2, 20, 10, max_h, bad) == nullptr && max_h == 10);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: adapt_main known|refuse|fold\n"); return 2; }
    if (!std::strcmp(argv[1], "known")) known();
    else if (!std::strcmp(argv[1], "refuse")) refuse();
    else if (!std::strcmp(argv[1], "fold")) fold();
    else { std::fprintf(stderr, "unknown case %s\n", argv[1]); return 2; }
    return failures ? 1 : 0;
}
