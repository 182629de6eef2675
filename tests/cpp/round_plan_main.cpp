// The host runtime's GPU-free arithmetic (rgk_amd/csrc/rgk_round_plan.h) on the CPU: this file includes that header (which pulls
// in rgk_plan.h and rgk.h) and nothing else of the library, and links without the HIP runtime.  Every expected value below is
// written out from the formulas rgk_host.cpp carried before the unit existed -- never computed by the unit itself.
// Usage: round_plan_main <case>; exit status 0 = every condition held.  `print-tasks` prints the task list of 67 x 45.
#include <cstdio>
#include <cstring>

#include "../../rgk_amd/csrc/rgk_round_plan.h"

static int failures = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
    } while (0)

static const RgkWorkspacePlane* plane(const char* name) {
    for (const RgkWorkspacePlane& pl : RGK_WORKSPACE)
        if (!std::strcmp(pl.name, name)) return &pl;
    std::fprintf(stderr, "no workspace plane '%s'\n", name);
    failures++;
    return &RGK_WORKSPACE[0];
}
static void workspace() {
    // the literal batch_paths carried (6: RGK_LV_FLOAT4)
    const auto before = [](size_t reverse) -> size_t { return 180 + (reverse ? 16 + 16 * 6 * reverse + 12 + 16 * (6 + 4 + reverse + 1) : 0); };
    CHECK(rgk_workspace_bytes_per_path(0) == 180);
    CHECK(rgk_workspace_bytes_per_path(1) == 496 && before(1) == 496);
    CHECK(rgk_workspace_bytes_per_path(3) == 720 && before(3) == 720);
    CHECK(rgk_workspace_bytes_per_path(7) == 1168 && before(7) == 1168);
    for (int i = 0; i < RGK_WS_PLANES; i++) CHECK(RGK_WORKSPACE[i].id == i); // (ensure_workspace allocates in this order)
    // ensure_workspace's alloc arguments for `paths` paths, and the element each plane's buffer holds (float4: 16, uint32_t: 4)
    const size_t paths = 1000;
    const char* one16[] = {"rayA0", "rayB0", "rayA1", "rayB1", "hit", "thr", "tot", "shA", "shB", "shC", "light"};
    for (uint32_t reverse : {0u, 3u, 7u}) {
        for (const char* n : one16) CHECK(rgk_plane_elems(*plane(n), paths, reverse) == paths && plane(n)->bytes == 16 && !plane(n)->bidir);
        CHECK(rgk_plane_elems(*plane("generic"), paths, reverse) == paths && plane("generic")->bytes == 4 && !plane("generic")->bidir);
        const char* bidir[] = {"lstart", "lv", "hitlist", "lvmask", "connlist", "conn", "jobs", "rads"};
        for (const char* n : bidir) CHECK(plane(n)->bidir);
        if (reverse == 0) {
            for (const char* n : bidir) CHECK(rgk_plane_elems(*plane(n), paths, 0) == 0);
            continue;
        }
        CHECK(rgk_plane_elems(*plane("lstart"), paths, reverse) == paths && plane("lstart")->bytes == 16);
        CHECK(rgk_plane_elems(*plane("lv"), paths, reverse) == paths * 6 * reverse && plane("lv")->bytes == 16);
        CHECK(rgk_plane_elems(*plane("hitlist"), paths, reverse) == paths && plane("hitlist")->bytes == 4);
        CHECK(rgk_plane_elems(*plane("lvmask"), paths, reverse) == paths && plane("lvmask")->bytes == 4);
        CHECK(rgk_plane_elems(*plane("connlist"), paths, reverse) == paths && plane("connlist")->bytes == 4);
        CHECK(rgk_plane_elems(*plane("conn"), paths, reverse) == paths * 6 && plane("conn")->bytes == 16);
        CHECK(rgk_plane_elems(*plane("jobs"), paths, reverse) == paths * 4 && plane("jobs")->bytes == 16);
        CHECK(rgk_plane_elems(*plane("rads"), paths, reverse) == paths * (reverse + 1) && plane("rads")->bytes == 16);
    }
    CHECK(rgk_plane_elems(*plane("lv"), (size_t)1 << 30, 7) == ((size_t)42 << 30)); // no 32-bit overflow
}

// Two counter blocks with a different value in every word the host reads, and junk in the others (work-fetch cursors, the
// generic lists).  Offsets as rgk_kernels.h has them: queue 0, shadow 64, hits 320, shadow rays 384, connections 448 of 576.
static void fill_blocks(uint32_t (&cam)[576], uint32_t (&light)[576]) {
    for (uint32_t i = 0; i < 576; i++) cam[i] = light[i] = 0xdead0000u + i;
    for (uint32_t b = 0; b < 64; b++) {
        cam[0 + b] = 1000 - 100 * b; cam[64 + b] = 500 - 50 * b; cam[384 + b] = 7 + b; cam[448 + b] = 30 + b;
        light[0 + b] = 900 - 10 * b; light[320 + b] = 800 - 10 * b; light[64 + b] = 700 - 10 * b;
    }
}
static void counters() {
    static_assert(RGK_RP_CNT_TOTAL == 576, "two blocks of 576 words");
    uint32_t cam[576], light[576];
    fill_blocks(cam, light);
    const uint32_t n0 = 1000;
    auto units = [](const rgk_counters& c, int k) { return c.kernel[k].units; };
    for (int le = 0; le < 2; le++) {
        // depth 1, unidirectional
        rgk_counters c{};
        rgk_add_pass_counters(cam, light, 1, 0, n0, le != 0, c);
        CHECK(c.path_rays == 1000 && c.shadow_rays == 500 + 7);
        CHECK(units(c, RGK_K_TRACE_CAMERA) == 1000 && units(c, RGK_K_SHADE_FIRST) == 1000 && units(c, RGK_K_TRACE_CLOSEST) == 0 && units(c, RGK_K_SHADE) == 0);
        CHECK(units(c, RGK_K_SHADOW_FIRST) == (le ? 500u : 0u) && units(c, RGK_K_SHADOW) == (le ? 0u : 500u));
        CHECK(units(c, RGK_K_SHADOW_JOBS) == 30 && units(c, RGK_K_CONNECT) == 30 && units(c, RGK_K_RESOLVE) == 1000);
        CHECK(units(c, RGK_K_LIGHT_TRACE) == 0 && units(c, RGK_K_LIGHT_SHADE) == 0 && units(c, RGK_K_LIGHT_SPLAT) == 0 && units(c, RGK_K_OTHER) == 0);
        // depth 5, unidirectional: queues 1000 .. 600, shadow 500 .. 300, traced shadow rays 7 .. 11, connections 30 .. 34
        c = rgk_counters{};
        rgk_add_pass_counters(cam, light, 5, 0, n0, le != 0, c);
        CHECK(c.path_rays == 4000 && c.shadow_rays == 2000 + 45);
        CHECK(units(c, RGK_K_TRACE_CAMERA) == 1000 && units(c, RGK_K_SHADE_FIRST) == 1000 && units(c, RGK_K_TRACE_CLOSEST) == 3000 && units(c, RGK_K_SHADE) == 3000);
        CHECK(units(c, RGK_K_SHADOW_FIRST) == (le ? 500u : 0u) && units(c, RGK_K_SHADOW) == (le ? 1500u : 2000u));
        CHECK(units(c, RGK_K_SHADOW_JOBS) == 160 && units(c, RGK_K_CONNECT) == 160 && units(c, RGK_K_RESOLVE) == 1000);
        CHECK(units(c, RGK_K_LIGHT_TRACE) == 0 && units(c, RGK_K_LIGHT_SHADE) == 0 && units(c, RGK_K_LIGHT_SPLAT) == 0);
        // depth 5, three light vertices: light queues 900, 890, 880, hits 800 .. 780, splats 700 .. 680.  The culled-light-ray
        // rule: light ray 0 counts once per path (n0 = 1000), not the 900 that reached the queue.
        c = rgk_counters{};
        rgk_add_pass_counters(cam, light, 5, 3, n0, le != 0, c);
        CHECK(c.path_rays == 4000 + 1000 + 890 + 880 && c.shadow_rays == 2045 + 2070);
        CHECK(units(c, RGK_K_LIGHT_TRACE) == 2670 && units(c, RGK_K_LIGHT_SHADE) == 2370 && units(c, RGK_K_LIGHT_SPLAT) == 2070);
        CHECK(units(c, RGK_K_TRACE_CLOSEST) == 3000 && units(c, RGK_K_SHADOW) == (le ? 1500u : 2000u) && units(c, RGK_K_RESOLVE) == 1000);
        // depth 1, three light vertices; a second pass adds to the first
        c = rgk_counters{};
        rgk_add_pass_counters(cam, light, 1, 3, n0, le != 0, c);
        CHECK(c.path_rays == 1000 + 2770 && c.shadow_rays == 507 + 2070);
        rgk_add_pass_counters(cam, light, 1, 3, n0, le != 0, c);
        CHECK(c.path_rays == 2 * 3770 && c.shadow_rays == 2 * 2577 && units(c, RGK_K_RESOLVE) == 2000 && units(c, RGK_K_LIGHT_TRACE) == 2 * 2670);
        // reverse 1: only the per-path light ray
        c = rgk_counters{};
        rgk_add_pass_counters(cam, light, 1, 1, n0, le != 0, c);
        CHECK(c.path_rays == 1000 + 1000 && units(c, RGK_K_LIGHT_TRACE) == 900);
        CHECK(c.paths == 0 && c.node_visits == 0 && c.ms_trace == 0.0); // (not this function's)
    }
}

static void fold() {
    // classes
    const int closest[] = {RGK_K_TRACE_CAMERA, RGK_K_TRACE_CLOSEST, RGK_K_LIGHT_TRACE}, shadow[] = {RGK_K_SHADOW_FIRST, RGK_K_SHADOW, RGK_K_SHADOW_JOBS, RGK_K_LIGHT_SPLAT};
    const int shade[] = {RGK_K_SHADE_FIRST, RGK_K_SHADE, RGK_K_CONNECT, RGK_K_LIGHT_SHADE}, other[] = {RGK_K_RESOLVE, RGK_K_OTHER};
    static_assert(RGK_K_COUNT == 13, "every kernel id is in one of the four lists");
    for (int k : closest) CHECK(rgk_kernel_class(k) == RGK_CLASS_CLOSEST && rgk_kernel_traverses(k));
    for (int k : shadow) CHECK(rgk_kernel_class(k) == RGK_CLASS_SHADOW && rgk_kernel_traverses(k));
    for (int k : shade) CHECK(rgk_kernel_class(k) == RGK_CLASS_SHADE && !rgk_kernel_traverses(k));
    for (int k : other) CHECK(rgk_kernel_class(k) == RGK_CLASS_OTHER && !rgk_kernel_traverses(k));
    // two launches per class (times exact in binary), and one kernel launched twice
    const RgkLaunchTime times[] = {{RGK_K_OTHER, 0.25f},       {RGK_K_TRACE_CAMERA, 1.5f}, {RGK_K_SHADE_FIRST, 3.0f}, {RGK_K_SHADOW_FIRST, 0.75f}, {RGK_K_TRACE_CLOSEST, 2.25f},
                                   {RGK_K_SHADE, 4.0f},        {RGK_K_SHADOW, 1.25f},      {RGK_K_RESOLVE, 0.125f},   {RGK_K_SHADE, 4.5f}};
    rgk_counters c{};
    rgk_fold_kernel_log(times, 9, nullptr, 0, c);
    CHECK(c.ms_trace == 3.75 && c.n_trace_launches == 2);
    CHECK(c.ms_shadow == 2.0 && c.n_shadow_launches == 2);
    CHECK(c.ms_shade == 11.5 && c.n_shade_launches == 3);
    CHECK(c.ms_other == 0.375);
    CHECK(c.kernel[RGK_K_SHADE].ms == 8.5 && c.kernel[RGK_K_SHADE].launches == 2);
    CHECK(c.kernel[RGK_K_TRACE_CAMERA].ms == 1.5 && c.kernel[RGK_K_TRACE_CAMERA].launches == 1);
    CHECK(c.kernel[RGK_K_RESOLVE].ms == 0.125 && c.kernel[RGK_K_OTHER].launches == 1 && c.kernel[RGK_K_CONNECT].launches == 0);
    double sum = 0.0;
    for (int k = 0; k < RGK_K_COUNT; k++) sum += c.kernel[k].ms;
    CHECK(sum == c.ms_trace + c.ms_shadow + c.ms_shade + c.ms_other); // the class sums are sums of the kernels'
    // read-backs behind alternating closest and shadow launches: running totals {closest nodes, triangles, shadow nodes, triangles}
    const RgkStatSnap snaps[] = {{RGK_K_TRACE_CAMERA, {100, 40, 0, 0}}, {RGK_K_SHADOW_FIRST, {100, 40, 50, 20}}, {RGK_K_TRACE_CLOSEST, {160, 70, 50, 20}},
                                 {RGK_K_SHADOW, {160, 70, 85, 33}},     {RGK_K_TRACE_CLOSEST, {200, 90, 85, 33}}};
    c = rgk_counters{};
    rgk_fold_kernel_log(nullptr, 0, snaps, 5, c);
    CHECK(c.kernel[RGK_K_TRACE_CAMERA].node_visits == 100 && c.kernel[RGK_K_TRACE_CAMERA].tri_tests == 40);
    CHECK(c.kernel[RGK_K_SHADOW_FIRST].node_visits == 50 && c.kernel[RGK_K_SHADOW_FIRST].tri_tests == 20);
    CHECK(c.kernel[RGK_K_TRACE_CLOSEST].node_visits == 60 + 40 && c.kernel[RGK_K_TRACE_CLOSEST].tri_tests == 30 + 20);
    CHECK(c.kernel[RGK_K_SHADOW].node_visits == 35 && c.kernel[RGK_K_SHADOW].tri_tests == 13);
    CHECK(c.node_visits == 0 && c.ms_trace == 0.0 && c.n_trace_launches == 0); // (the round's totals come from the final read-back)
}

static const rgk_tile TASKS_67x45[6] = {{32, 64, 0, 32, 142}, {0, 32, 0, 32, 143}, {32, 64, 32, 45, 144}, {0, 32, 32, 45, 145}, {64, 67, 0, 32, 146}, {64, 67, 32, 45, 147}};
static bool same_tile(const rgk_tile& a, const rgk_tile& b) { return a.x0 == b.x0 && a.x1 == b.x1 && a.y0 == b.y0 && a.y1 == b.y1 && a.seed == b.seed; }
static void tiles() {
    std::vector<uint32_t> toff;
    uint32_t bad = 99;
    CHECK(rgk_tile_offsets(67, 45, nullptr, 0, toff, bad) == RGK_TILES_OK && toff.size() == 1 && toff[0] == 0);
    const rgk_tile some[] = {{0, 32, 0, 32, 1}, {64, 67, 32, 45, 2}, {5, 5, 0, 10, 3}, {0, 67, 0, 45, 4}};
    CHECK(rgk_tile_offsets(67, 45, some, 4, toff, bad) == RGK_TILES_OK && toff.size() == 5);
    CHECK(toff[0] == 0 && toff[1] == 1024 && toff[2] == 1063 && toff[3] == 1063 && toff[4] == 1063 + 3015);
    const rgk_tile backwards[] = {{0, 32, 0, 32, 1}, {33, 32, 0, 32, 2}}, upside[] = {{0, 32, 9, 8, 1}};
    CHECK(rgk_tile_offsets(67, 45, backwards, 2, toff, bad) == RGK_TILES_OUTSIDE && bad == 1);
    CHECK(rgk_tile_offsets(67, 45, upside, 1, toff, bad) == RGK_TILES_OUTSIDE && bad == 0);
    const rgk_tile right[] = {{60, 68, 0, 45, 1}}, below[] = {{0, 67, 40, 46, 1}};
    CHECK(rgk_tile_offsets(67, 45, right, 1, toff, bad) == RGK_TILES_OUTSIDE && bad == 0);
    CHECK(rgk_tile_offsets(67, 45, below, 1, toff, bad) == RGK_TILES_OUTSIDE && bad == 0);
    // 2^30 + (2^30 - 32768) + 32767 = 2^31 - 1 pixels are a list; one more pixel is not, and neither are two tiles of 2^30
    const rgk_tile big[] = {{0, 32768, 0, 32768, 1}, {0, 32768, 0, 32767, 2}, {0, 32767, 0, 1, 3}, {7, 8, 7, 8, 4}};
    CHECK(rgk_tile_offsets(65535, 65535, big, 3, toff, bad) == RGK_TILES_OK && toff[3] == 0x7fffffffu);
    CHECK(rgk_tile_offsets(65535, 65535, big, 4, toff, bad) == RGK_TILES_TOO_MANY_PIXELS && bad == 3);
    const rgk_tile two[] = {{0, 32768, 0, 32768, 1}, {0, 32768, 0, 32768, 2}};
    CHECK(rgk_tile_offsets(65535, 65535, two, 2, toff, bad) == RGK_TILES_TOO_MANY_PIXELS && bad == 1);
    const rgk_tile whole[] = {{0, 65535, 0, 65535, 1}}; // 4294836225 pixels: the 64-bit product, not its low word
    CHECK(rgk_tile_offsets(65535, 65535, whole, 1, toff, bad) == RGK_TILES_TOO_MANY_PIXELS && bad == 0);

    // 67 x 45 in tiles of 32 around (33.5, 22.5): squared distances of the six midpoints, row-major, 348.5, 252.5, 1066.25 /
    // 562.25, 466.25, 1280 -> tiles 1, 0, 4, 3, 2, 5; seeds seedstart + seedcount_base + i
    std::vector<rgk_tile> tl = rgk_task_list(32, 67, 45, 33.5f, 22.5f, 42u + 100u);
    CHECK(tl.size() == 6);
    for (size_t i = 0; i < tl.size() && i < 6; i++) CHECK(same_tile(tl[i], TASKS_67x45[i]));
    // equal distances keep the row-major order (a stable sort)
    tl = rgk_task_list(32, 64, 64, 32.0f, 32.0f, 0u);
    const rgk_tile ties[4] = {{0, 32, 0, 32, 0}, {32, 64, 0, 32, 1}, {0, 32, 32, 64, 2}, {32, 64, 32, 64, 3}};
    CHECK(tl.size() == 4);
    for (size_t i = 0; i < tl.size() && i < 4; i++) CHECK(same_tile(tl[i], ties[i]));
    CHECK(rgk_task_list(32, 0, 45, 0.f, 0.f, 0u).empty());

    // the key of a frame's lists: camera, resolution, every tile's rectangle -- not the seeds
    rgk_camera cam;
    std::memset(&cam, 0, sizeof(cam)); // (the key reads the struct's bytes)
    cam.origin[0] = 1.0f; cam.direction[2] = -1.0f; cam.xsize = 67; cam.ysize = 45;
    rgk_tile t[6];
    std::memcpy(t, TASKS_67x45, sizeof(t));
    const uint64_t key = rgk_frame_list_key(cam, 67, 45, t, 6);
    CHECK(key == rgk_frame_list_key(cam, 67, 45, t, 6));
    for (rgk_tile& x : t) x.seed += 1000;
    CHECK(rgk_frame_list_key(cam, 67, 45, t, 6) == key);
    rgk_camera cam2 = cam;
    cam2.origin[0] = 1.5f;
    CHECK(rgk_frame_list_key(cam2, 67, 45, t, 6) != key);
    cam2 = cam; cam2.lens_size = 0.01f;
    CHECK(rgk_frame_list_key(cam2, 67, 45, t, 6) != key);
    CHECK(rgk_frame_list_key(cam, 68, 45, t, 6) != key && rgk_frame_list_key(cam, 67, 46, t, 6) != key && rgk_frame_list_key(cam, 45, 67, t, 6) != key);
    CHECK(rgk_frame_list_key(cam, 67, 45, t, 5) != key);
    for (int w = 0; w < 4; w++) { // one word of one tile's rectangle
        rgk_tile u[6];
        std::memcpy(u, t, sizeof(u));
        uint32_t words[5];
        std::memcpy(words, &u[3], sizeof(words));
        words[w] ^= 1u;
        std::memcpy(&u[3], words, sizeof(words));
        CHECK(rgk_frame_list_key(cam, 67, 45, u, 6) != key);
    }
    std::swap(t[0], t[1]); // the order of the pixels in the list
    CHECK(rgk_frame_list_key(cam, 67, 45, t, 6) != key);
    // FNV-1a, 64 bit: no tiles, an all-zero camera and resolution 0 x 0 hash sizeof(rgk_camera) + 8 zero bytes: offset * prime^n
    rgk_camera zero;
    std::memset(&zero, 0, sizeof(zero));
    uint64_t expect = 1469598103934665603ull;
    for (size_t i = 0; i < sizeof(rgk_camera) + 8; i++) expect *= 1099511628211ull;
    CHECK(rgk_frame_list_key(zero, 0, 0, nullptr, 0) == expect);
}

static void stack() {
    static_assert(RGK_ENTRY_K == 6, "a camera ray starts with 6 entry nodes");
    RgkStackPlan p{};
    // 10 + 1 + 6 = 17 entries: all in LDS where the overflow is switched off ...
    CHECK(rgk_stack_plan(10, false, 16, p) && p.stack == 32 && p.lds == 32 && p.ovf_per_lane == 0);
    CHECK(rgk_stack_plan(25, false, 16, p) && p.stack == 32 && p.lds == 32 && p.ovf_per_lane == 0);   // 32 entries: the last that fit
    CHECK(rgk_stack_plan(26, false, 16, p) && p.stack == 256 && p.lds == 16 && p.ovf_per_lane == 25); // 33 - 8
    // ... and by default 256/16 with room for all but the 8 entries the beam walker keeps in LDS
    CHECK(rgk_stack_plan(10, true, 16, p) && p.stack == 256 && p.lds == 16 && p.ovf_per_lane == 9);
    CHECK(rgk_stack_plan(40, true, 16, p) && p.stack == 256 && p.lds == 16 && p.ovf_per_lane == 39); // 47 - 8
    CHECK(rgk_stack_plan(40, true, 32, p) && p.stack == 256 && p.lds == 32 && p.ovf_per_lane == 39);
    CHECK(rgk_stack_plan(40, false, 32, p) && p.stack == 256 && p.lds == 32 && p.ovf_per_lane == 39);
    CHECK(rgk_stack_plan(0, true, 16, p) && p.ovf_per_lane == 1); // 7 - 8: at least one entry
    CHECK(rgk_stack_plan(249, true, 16, p) && p.stack == 256 && p.ovf_per_lane == 248); // 256 entries: the deepest tree
    CHECK(!rgk_stack_plan(250, true, 16, p));
    CHECK(!rgk_stack_plan(252, true, 16, p) && !rgk_stack_plan(252, false, 32, p));
    // the area the host allocates: lanes of a full trace grid (rgk_plan.h) x entries per lane
    CHECK((size_t)rgk_trace_grid(16) * RGK_TRACE_BLOCK * 39 == (size_t)2048 * 256 * 39);
}

int main(int argc, char** argv) {
    const char* c = argc > 1 ? argv[1] : "";
    if (!std::strcmp(c, "workspace")) workspace();
    else if (!std::strcmp(c, "counters")) counters();
    else if (!std::strcmp(c, "fold")) fold();
    else if (!std::strcmp(c, "tiles")) tiles();
    else if (!std::strcmp(c, "stack")) stack();
    else if (!std::strcmp(c, "print-tasks")) {
        for (const rgk_tile& t : rgk_task_list(32, 67, 45, 33.5f, 22.5f, 42u)) std::printf("%u %u %u %u %u\n", t.x0, t.x1, t.y0, t.y1, t.seed);
    } else { std::fprintf(stderr, "unknown case '%s'\n", c); return 2; }
    if (failures) std::fprintf(stderr, "%d condition(s) failed in case %s\n", failures, c);
    return failures ? 1 : 0;
}
