// CPU harness of the GPU-free commit unit (rgk_amd/csrc/rgk_commit.cpp), linked with nothing else of the library and
// run under ASan + UBSan by tests/test_commit_cpu.py:  commit_main <case> [--digest]
//   geom-default | geom-leaf1 | geom-leaf16 | geom-nosplit | geom-noopt | geom-single | refit-pieces | textures |
//   pool-tables | pool-limits | pool-bits | pool-small | small
// Inputs come from a fixed LCG seed, no file is read.  Exit status 0: every condition of the case held.
// --digest: an FNV-1a digest per output table on stdout (a refactor of the unit must leave them as they are).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../rgk_amd/csrc/rgk_commit.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                \
            std::fprintf(stderr, "\n");                                       \
            g_failed++;                                                       \
        }                                                                     \
    } while (0)

static bool g_digest = false;
template <typename T>
static void digest(const char* name, const std::vector<T>& v) {
    if (!g_digest) return;
    uint64_t x = 1469598103934665603ull;
    const unsigned char* b = (const unsigned char*)v.data();
    for (size_t i = 0; i < v.size() * sizeof(T); i++) { x ^= b[i]; x *= 1099511628211ull; }
    std::printf("[digest] %s %zu %016llx\n", name, v.size(), (unsigned long long)x);
}
template <typename T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// ------------------------------------------------------------------ inputs
struct Lcg {
    uint32_t s = 12345u;
    uint32_t next() { s = s * 1664525u + 1013904223u; return s >> 8; }
    float unit() { return (float)next() / 16777216.0f; } // [0, 1)
};

struct Geometry {
    std::vector<float> v;    // three vertices of its own per triangle
    std::vector<uint32_t> idx;
    std::set<uint32_t> degenerate;
    uint32_t nt() const { return (uint32_t)(idx.size() / 3); }
    void tri(const float a[3], const float b[3], const float c[3]) {
        for (const float* p : {a, b, c}) { idx.push_back((uint32_t)(v.size() / 3)); v.insert(v.end(), p, p + 3); }
    }
};

// 647 triangles: 600 small random ones in the unit cube, 2 spanning the cube (pre-splitting), 5 with two equal vertices
// (NaN plane), 40 identical copies of one small triangle (coincident centroids: the builder's median split).
static Geometry make_geometry() {
    Geometry g;
    Lcg r;
    const float a = 0.05f / (2.0f * 1.7320508f); // offsets within +-a per axis: every edge <= 0.05
    auto small = [&](float o[3][3]) {
        float c[3] = {0.02f + 0.96f * r.unit(), 0.02f + 0.96f * r.unit(), 0.02f + 0.96f * r.unit()};
        for (int k = 0; k < 3; k++) for (int x = 0; x < 3; x++) o[k][x] = c[x] + a * (2.0f * r.unit() - 1.0f);
    };
    float t[3][3];
    for (int i = 0; i < 600; i++) { small(t); g.tri(t[0], t[1], t[2]); }
    const float big[2][3][3] = {{{0.f, 0.f, 0.5f}, {1.f, 0.f, 0.4f}, {0.f, 1.f, 0.6f}}, {{1.f, 1.f, 0.f}, {0.f, 1.f, 1.f}, {1.f, 0.f, 1.f}}};
    for (int i = 0; i < 2; i++) g.tri(big[i][0], big[i][1], big[i][2]);
    for (int i = 0; i < 5; i++) { small(t); g.degenerate.insert(g.nt()); g.tri(t[0], t[0], t[2]); }
    small(t);
    for (int i = 0; i < 40; i++) g.tri(t[0], t[1], t[2]);
    return g;
}

static Geometry make_single_leaf() {
    Geometry g; // three small triangles far apart: none is pre-split, and three references fit one leaf
    Lcg r;
    const float centre[3][3] = {{0.1f, 0.1f, 0.1f}, {0.9f, 0.5f, 0.2f}, {0.4f, 0.9f, 0.8f}};
    for (int i = 0; i < 3; i++) {
        float t[3][3];
        for (int k = 0; k < 3; k++) for (int x = 0; x < 3; x++) t[k][x] = centre[i][x] + 0.02f * (2.0f * r.unit() - 1.0f);
        g.tri(t[0], t[1], t[2]);
    }
    return g;
}

// The six textures of the texture case and a small scene around them.
struct TextureScene {
    std::vector<float> tex[6], lut3;
    std::vector<uint8_t> bytes3;
    std::vector<rgk_texture> textures;
    std::vector<rgk_material> materials;
    std::vector<rgk_pointlight> lights;
    std::vector<float> v, n, tg, uv, ltc;
    std::vector<uint32_t> idx, mat, areal_off, areal_tris;
    rgk_scene_desc d;
};
static void make_texture_scene(TextureScene& s) {
    Lcg r;
    auto image = [&](std::vector<float>& out, uint32_t w, uint32_t h, const std::vector<float>& vals) { // every value at least once, then any
        out.resize((size_t)3 * w * h);
        for (size_t k = 0; k < out.size(); k++) out[k] = vals[k < vals.size() ? k : r.next() % vals.size()];
    };
    std::vector<float> v0 = {0.0f, -0.0f, std::nanf("")}, v1, v2, v4;
    while (v0.size() < 200) v0.push_back(0.001f + 0.004f * (float)v0.size());
    for (int k = 0; k < 40; k++) v1.push_back(2.0f + 0.01f * (float)k);
    for (int k = 10; k < 30; k++) v1.push_back(v0[(size_t)k]);
    for (int k = 0; k < 257; k++) v2.push_back(100.0f + (float)k);
    s.lut3.resize(256);
    for (int k = 0; k < 256; k++) s.lut3[(size_t)k] = ((float)k / 255.0f) * ((float)k / 255.0f);
    for (int k = 0; k < 256; k += 3) v4.push_back(s.lut3[(size_t)k]);
    image(s.tex[0], 16, 12, v0); image(s.tex[1], 9, 5, v1); image(s.tex[2], 10, 9, v2); image(s.tex[4], 11, 3, v4);
    s.bytes3.resize(3 * 5 * 7);
    for (uint8_t& b : s.bytes3) b = (uint8_t)(r.next() & 255u);
    const uint32_t dims[6][2] = {{16, 12}, {9, 5}, {10, 9}, {5, 7}, {11, 3}, {0, 0}};
    s.textures.assign(6, rgk_texture{});
    for (int i = 0; i < 6; i++) {
        rgk_texture& t = s.textures[(size_t)i];
        t.kind = i == 5 ? RGK_TEX_SOLID : (i == 3 ? RGK_TEX_RGB8 : RGK_TEX_RGB32F);
        t.width = dims[i][0]; t.height = dims[i][1];
        if (t.kind == RGK_TEX_RGB32F) t.texels = s.tex[i].data();
    }
    s.textures[3].texels8 = s.bytes3.data(); s.textures[3].lut = s.lut3.data();
    s.textures[5].color[0] = 0.25f; s.textures[5].color[1] = -0.0f; s.textures[5].color[2] = 3.5f;
    s.materials.assign(2, rgk_material{});
    s.materials[0].tex_diffuse = 0; s.materials[0].tex_color = 3; s.materials[0].tex_bump = -1; s.materials[0].mix_m1 = s.materials[0].mix_m2 = -1;
    s.materials[1].tex_diffuse = 5; s.materials[1].tex_color = 2; s.materials[1].tex_bump = 4; s.materials[1].mix_m1 = s.materials[1].mix_m2 = -1;
    s.materials[1].emission[0] = 1.f; s.materials[1].emission[1] = 2.f; s.materials[1].emission[2] = 0.5f;
    s.materials[0].roughness = 0.3f; s.materials[0].ior = 1.5f; s.materials[0].amount = 0.25f;
    // three right triangles in the plane z = 0 with legs (1, 1), (2, 1), (2, 3): areas 0.5, 1, 3 -- one emissive object
    const float legs[3][2] = {{1.f, 1.f}, {2.f, 1.f}, {2.f, 3.f}};
    for (uint32_t i = 0; i < 3; i++) {
        const float o = 4.0f * (float)i;
        const float p[9] = {o, 0.f, 0.f, o + legs[i][0], 0.f, 0.f, o, legs[i][1], 0.f};
        s.v.insert(s.v.end(), p, p + 9);
        for (uint32_t k = 0; k < 3; k++) {
            s.idx.push_back(3 * i + k);
            const float nn[3] = {0.f, 0.f, 1.f}, tt[3] = {1.f, 0.f, 0.f}, cc[2] = {r.unit(), r.unit()};
            s.n.insert(s.n.end(), nn, nn + 3); s.tg.insert(s.tg.end(), tt, tt + 3); s.uv.insert(s.uv.end(), cc, cc + 2);
        }
        s.mat.push_back(1);
        s.areal_tris.push_back(i);
    }
    s.areal_off = {0, 3};
    s.lights.assign(1, rgk_pointlight{});
    s.lights[0].pos[0] = 1.f; s.lights[0].pos[1] = 2.f; s.lights[0].pos[2] = 3.f;
    s.lights[0].color[0] = s.lights[0].color[1] = s.lights[0].color[2] = 1.f;
    s.lights[0].intensity = 7.5f; s.lights[0].size = 0.f;
    s.ltc.resize(4096 * 5);
    for (float& f : s.ltc) f = r.unit();
    rgk_scene_desc& d = s.d;
    std::memset(&d, 0, sizeof(d));
    d.n_vertices = 9; d.vertices = s.v.data(); d.normals = s.n.data(); d.tangents = s.tg.data(); d.texcoords = s.uv.data();
    d.n_triangles = 3; d.tri_indices = s.idx.data(); d.tri_material = s.mat.data();
    d.n_materials = 2; d.materials = s.materials.data();
    d.n_textures = 6; d.textures = s.textures.data();
    d.n_pointlights = 1; d.pointlights = s.lights.data();
    d.n_areal_lights = 1; d.areal_offsets = s.areal_off.data(); d.areal_tris = s.areal_tris.data();
    d.ltc_ggx = s.ltc.data(); d.ltc_beckmann = nullptr;
    d.sky_texture = -1;
}

// ------------------------------------------------------------------ geometry cases
struct GeomOut {
    std::vector<TriIsect> recs;
    std::vector<Prim> prims; // as commit_triangles left them
    HostAccel acc;
};
static int run_geometry(const Geometry& g, const BuildOptions& opt, GeomOut& o) {
    float mn[3], mx[3], eps;
    int rc = commit_bounds(g.v.data(), g.idx.data(), g.nt(), mn, mx, &eps);
    if (rc) return rc;
    commit_triangles(g.v.data(), g.idx.data(), g.nt(), split_threshold(opt, eps), o.recs, o.prims);
    std::vector<Prim> work = o.prims; // the builder shuffles its input
    return build_host_accel(work, o.recs, eps, opt, o.acc);
}

static bool inside(const QNode& q, int i, const float p[3]) {
    const float s[3] = {q.sx, q.sy, q.sz};
    for (int a = 0; a < 3; a++) { // the kernels' decode
        const float lo = std::fmaf((float)q.qlo[a][i], s[a], q.p[a]), hi = std::fmaf((float)q.qhi[a][i], s[a], q.p[a]);
        if (!(lo <= p[a] && p[a] <= hi)) return false;
    }
    return true;
}

static void check_geometry(const Geometry& g, const BuildOptions& opt, bool expect_split) {
    GeomOut o, again;
    CHECK(run_geometry(g, opt, o) == 0, "%s", rgk_last_error());
    if (g_failed) return;
    const HostAccel& A = o.acc;
    const uint32_t nt = g.nt(), n_refs = (uint32_t)A.leaf_recs.size(), n_finite = nt - (uint32_t)g.degenerate.size();
    digest("recs", o.recs); digest("prims", o.prims); digest("qnodes", A.qnodes); digest("leaf_recs", A.leaf_recs); digest("leaf_pb", A.leaf_pb);
    if (g_digest) std::printf("[digest] max_depth %u max_stack %u n_refs %u\n", A.max_depth, A.max_stack, n_refs);
    CHECK(A.leaf_pb.size() == n_refs && o.prims.size() == n_refs, "leaf_pb %zu prims %zu refs %u", A.leaf_pb.size(), o.prims.size(), n_refs);
    CHECK(n_refs <= 2 * nt, "%u refs of %u triangles", n_refs, nt);
    if (expect_split) CHECK(n_refs > n_finite, "%u refs, %u finite triangles: nothing was pre-split", n_refs, n_finite);
    else CHECK(n_refs == n_finite, "%u refs, %u finite triangles", n_refs, n_finite);
    std::set<uint32_t> listed;
    for (const TriIsect& r : A.leaf_recs) listed.insert(r.tri);
    CHECK(listed.size() == n_finite, "%zu triangles listed, %u finite", listed.size(), n_finite);
    for (uint32_t t = 0; t < nt; t++) {
        const bool nan_plane = o.recs[t].n[0] != o.recs[t].n[0];
        CHECK(nan_plane == (g.degenerate.count(t) != 0), "triangle %u: plane %g", t, o.recs[t].n[0]);
        CHECK((listed.count(t) != 0) == !nan_plane, "triangle %u: listed %d, NaN plane %d", t, (int)listed.count(t), (int)nan_plane);
    }
    // the leaves reached from node 0 cover [0, n_refs) exactly once; the deepest inner node is max_depth
    std::vector<uint32_t> covered(n_refs, 0u);
    uint32_t deepest = 0;
    std::vector<std::pair<int, uint32_t>> stack = {{0, 0u}};
    size_t visited = 0;
    while (!stack.empty() && visited++ <= A.qnodes.size()) {
        const int node = stack.back().first; const uint32_t depth = stack.back().second;
        stack.pop_back();
        deepest = std::max(deepest, depth);
        for (int i = 0; i < 4; i++) {
            const int32_t c = A.qnodes[(size_t)node].child[i];
            if (c == RGK_QNODE_EMPTY) continue;
            if (c >= 0) { CHECK((size_t)c < A.qnodes.size(), "child %d of node %d", c, node); if ((size_t)c < A.qnodes.size()) stack.push_back({c, depth + 1}); continue; }
            const uint32_t code = ~(uint32_t)c, first = code >> 4, count = (code & 15u) + 1u;
            CHECK(first + count <= n_refs, "leaf [%u, +%u) of %u refs", first, count, n_refs);
            for (uint32_t k = first; k < first + count && k < n_refs; k++) covered[k]++;
        }
    }
    CHECK(visited == A.qnodes.size(), "%zu nodes visited of %zu", visited, A.qnodes.size());
    size_t once = 0;
    for (uint32_t c : covered) once += c == 1u;
    CHECK(once == n_refs, "%zu of %u references covered exactly once", once, n_refs);
    CHECK(deepest == A.max_depth, "deepest inner node %u, max_depth %u", deepest, A.max_depth);
    // point location: every lattice point of every finite triangle is in a leaf that lists the triangle, through decoded boxes only
    size_t points = 0, misses = 0;
    std::vector<int> walk;
    for (uint32_t t = 0; t < nt; t++) {
        if (g.degenerate.count(t)) continue;
        const float *v0 = &g.v[3 * (size_t)g.idx[3 * t]], *v1 = &g.v[3 * (size_t)g.idx[3 * t + 1]], *v2 = &g.v[3 * (size_t)g.idx[3 * t + 2]];
        for (int bi = 0; bi <= 12; bi++)
            for (int ci = 0; bi + ci <= 12; ci++) {
                const float b = (float)bi / 12.0f, c = (float)ci / 12.0f;
                float p[3];
                for (int a = 0; a < 3; a++) p[a] = v0[a] + b * (v1[a] - v0[a]) + c * (v2[a] - v0[a]);
                bool found = false;
                walk.assign(1, 0);
                while (!walk.empty() && !found) {
                    const QNode& q = A.qnodes[(size_t)walk.back()];
                    walk.pop_back();
                    for (int i = 0; i < 4 && !found; i++) {
                        const int32_t ch = q.child[i];
                        if (ch == RGK_QNODE_EMPTY || !inside(q, i, p)) continue;
                        if (ch >= 0) { walk.push_back(ch); continue; }
                        const uint32_t code = ~(uint32_t)ch, first = code >> 4, count = (code & 15u) + 1u;
                        for (uint32_t k = first; k < first + count && k < n_refs; k++) found = found || A.leaf_recs[k].tri == t;
                    }
                }
                points++;
                misses += !found;
            }
    }
    if (g_digest) std::printf("[points] %zu located, %zu missed\n", points, misses);
    CHECK(points == (size_t)91 * n_finite && misses == 0, "%zu of %zu points in no leaf of their triangle", misses, points);
    // a second run: byte-identical tables
    CHECK(run_geometry(g, opt, again) == 0, "%s", rgk_last_error());
    CHECK(same_bytes(o.recs, again.recs) && same_bytes(o.prims, again.prims) && same_bytes(A.qnodes, again.acc.qnodes) && same_bytes(A.leaf_recs, again.acc.leaf_recs) &&
              same_bytes(A.leaf_pb, again.acc.leaf_pb) && A.max_depth == again.acc.max_depth && A.max_stack == again.acc.max_stack,
          "two runs on the same input differ");
}

static void check_single_leaf() {
    const Geometry g = make_single_leaf();
    check_geometry(g, BuildOptions{}, false);
    GeomOut o;
    CHECK(run_geometry(g, BuildOptions{}, o) == 0 && o.acc.qnodes.size() == 1, "%zu nodes", o.acc.qnodes.size());
}

// ------------------------------------------------------------------ the box of a moved piece
// rgk_scene_refit re-boxes a pre-split reference with piece_box (rgk_tree.h) from the moved triangle and the piece's parameter
// box.  For every proper piece of the 647-triangle geometry and three affine moves of its triangle -- none, a rotation with a
// scale and a shift of order 1, and scales of 1e3 and 1e-3 with a shift of 1e4 -- every point of a 13 x 13 lattice over the
// parameter box that lies in the triangle (b + c <= 1), evaluated in double from the moved float vertices and rounded to
// float, is in the box: tolerance zero.
static void check_refit_pieces() {
    const Geometry g = make_geometry();
    GeomOut o;
    CHECK(run_geometry(g, BuildOptions{}, o) == 0, "%s", rgk_last_error());
    if (g_failed) return;
    const double rot[3][3] = {{0.36, 0.48, -0.8}, {-0.8, 0.6, 0.0}, {0.48, 0.64, 0.6}}; // orthonormal
    const auto move = [&](int map, const float* v) {
        double w[3] = {v[0], v[1], v[2]};
        if (map == 1) for (int a = 0; a < 3; a++) w[a] = 1.3 * (rot[a][0] * v[0] + rot[a][1] * v[1] + rot[a][2] * v[2]) + (a == 0 ? 0.3 : (a == 1 ? -0.2 : 0.5));
        if (map == 2) { w[0] = 1e3 * v[0] + 1e4; w[1] = v[1] + 1e4; w[2] = 1e-3 * v[2] + 1e4; }
        return V3{(float)w[0], (float)w[1], (float)w[2]};
    };
    size_t pieces = 0, points = 0, outside = 0;
    for (const Prim& p : o.prims) {
        if (whole_triangle(p.pb[0], p.pb[1], p.pb[2], p.pb[3])) continue;
        for (int map = 0; map < 3; map++) {
            V3 v[3];
            for (int k = 0; k < 3; k++) v[k] = move(map, &g.v[3 * (size_t)g.idx[3 * p.tri + k]]);
            const Box box = piece_box(v[0], v[1], v[2], p.pb[0], p.pb[1], p.pb[2], p.pb[3]);
            pieces++;
            for (int bi = 0; bi <= 12; bi++)
                for (int ci = 0; ci <= 12; ci++) {
                    const double b = p.pb[0] + ((double)p.pb[1] - p.pb[0]) * bi / 12.0, c = p.pb[2] + ((double)p.pb[3] - p.pb[2]) * ci / 12.0;
                    if (b + c > 1.0) continue;
                    points++;
                    bool in = true;
                    for (int a = 0; a < 3; a++) {
                        const double v0 = comp(v[0], a), v1 = comp(v[1], a), v2 = comp(v[2], a);
                        const float x = (float)(v0 + b * (v1 - v0) + c * (v2 - v0));
                        in = in && box.mn[a] <= x && x <= box.mx[a];
                    }
                    outside += !in;
                }
        }
    }
    if (g_digest) std::printf("[pieces] %zu pieces, %zu points, %zu outside\n", pieces, points, outside);
    CHECK(pieces > 0, "the geometry has no pre-split piece");
    CHECK(outside == 0, "%zu of %zu points outside the box of their piece (%zu pieces)", outside, points, pieces);
}

// ------------------------------------------------------------------ texture case
static void digest_tables(const ShadingTables& t) {
    digest("tri_shade", t.tri_shade); digest("texels", t.tex.texels); digest("texels8", t.tex.texels8); digest("luts", t.tex.luts); digest("texrefs", t.tex.refs);
    digest("materials", t.materials); digest("pointlights", t.pointlights); digest("areal", t.areal); digest("areal_tris", t.areal_tris);
    digest("hdims", t.hdims); digest("hperm", t.hperm); digest("ltc", t.ltc);
    if (g_digest) std::printf("[digest] total_point %08x total_areal %08x n_float %u n_palettized %u\n", bits(t.total_point_power), bits(t.total_areal_power), t.tex.n_float, t.tex.n_palettized);
}

static void check_textures() {
    TextureScene s;
    make_texture_scene(s);
    CHECK(validate_desc(&s.d) == 0, "%s", rgk_last_error());
    ShadingTables t, again;
    CHECK(build_shading_tables(&s.d, t) == 0, "%s", rgk_last_error());
    if (g_failed) return;
    digest_tables(t);
    const std::vector<TexRef>& R = t.tex.refs;
    CHECK(t.tex.n_float == 4 && t.tex.n_palettized == 3, "%u float textures, %u palettized", t.tex.n_float, t.tex.n_palettized);
    const uint32_t kinds[6] = {RGK_TEX_RGB8, RGK_TEX_RGB8, RGK_TEX_RGB32F, RGK_TEX_RGB8, RGK_TEX_RGB8, RGK_TEX_SOLID};
    for (int i = 0; i < 6; i++) CHECK(R[(size_t)i].kind == kinds[i], "T%d: kind %u", i, R[(size_t)i].kind);
    CHECK(R[1].c == R[0].c, "T1 table at %u, T0's at %u", R[1].c, R[0].c);
    CHECK(R[4].c == R[3].c, "T4 table at %u, T3's at %u", R[4].c, R[3].c);
    CHECK(R[0].c != R[3].c, "T0 in the caller's table");
    CHECK(std::memcmp(&t.tex.luts[R[3].c], s.lut3.data(), 1024) == 0, "T3: not the caller's table");
    CHECK(R[5].a == bits(0.25f) && R[5].b == bits(-0.0f) && R[5].c == bits(3.5f), "T5: %08x %08x %08x", R[5].a, R[5].b, R[5].c);
    for (int i = 0; i < 5; i++) {
        const rgk_texture& x = s.textures[(size_t)i];
        const TexRef& r = R[(size_t)i];
        CHECK(r.a == (x.width | (x.height << 16)), "T%d: size word %08x", i, r.a);
        size_t bad = 0;
        if (r.kind == RGK_TEX_RGB8) {
            CHECK(r.b % 32 == 0, "T%d: byte texels at %u", i, r.b);
            const size_t tiles_x = (x.width + 7) / 8, tiles_y = (x.height + 3) / 4;
            CHECK(r.b + tiles_x * tiles_y * 32 <= t.tex.texels8.size() && r.c + 256 <= t.tex.luts.size(), "T%d: outside its pools", i);
            for (size_t y = 0; y < x.height; y++)
                for (size_t xx = 0; xx < x.width; xx++) {
                    const uint32_t w = t.tex.texels8[r.b + ((y >> 2) * tiles_x + (xx >> 3)) * 32 + ((y & 3) << 3) + (xx & 7)];
                    for (int ch = 0; ch < 3; ch++) {
                        const size_t k = 3 * (y * x.width + xx) + (size_t)ch;
                        const uint32_t byte = (w >> (8 * ch)) & 255u;
                        const float want = i == 3 ? s.lut3[s.bytes3[k]] : s.tex[i][k];
                        bad += bits(t.tex.luts[r.c + byte]) != bits(want);
                    }
                }
        } else {
            CHECK(r.b + (size_t)x.width * x.height <= t.tex.texels.size(), "T%d: outside the float pool", i);
            for (size_t k = 0; k < (size_t)x.width * x.height; k++) {
                const float4 f = t.tex.texels[r.b + k];
                bad += bits(f.x) != bits(s.tex[i][3 * k]) || bits(f.y) != bits(s.tex[i][3 * k + 1]) || bits(f.z) != bits(s.tex[i][3 * k + 2]) || bits(f.w) != 0u;
            }
        }
        CHECK(bad == 0, "T%d: %zu texels differ from the source", i, bad);
    }
    CHECK(t.materials[0].t_diffuse.b == R[0].b && t.materials[0].t_bump.kind == RGK_TEXREF_NONE && t.materials[1].t_color.kind == RGK_TEX_RGB32F, "material texture references");
    CHECK(build_shading_tables(&s.d, again) == 0, "%s", rgk_last_error());
    CHECK(same_bytes(t.tri_shade, again.tri_shade) && same_bytes(t.tex.texels, again.tex.texels) && same_bytes(t.tex.texels8, again.tex.texels8) && same_bytes(t.tex.luts, again.tex.luts) &&
              same_bytes(t.tex.refs, again.tex.refs) && same_bytes(t.materials, again.materials) && same_bytes(t.pointlights, again.pointlights) && same_bytes(t.areal, again.areal) &&
              same_bytes(t.areal_tris, again.areal_tris) && same_bytes(t.hdims, again.hdims) && same_bytes(t.hperm, again.hperm) && same_bytes(t.ltc, again.ltc),
          "two runs on the same input differ");
}

// ------------------------------------------------------------------ texture pool cases
// assign_palettes + pack_texels on descriptors that hold textures only: where the tables land (the kernels decode a table
// through LDS while its offset + 256 <= RGK_LDS_LUT_FLOATS = 512, rgk_device.h), the 256 / 257 value limit, values told apart
// by their bits, and the tiled byte layout at its smallest shapes.
struct Pool {
    std::vector<Palette> palettes;
    std::vector<int> tex_palette;
    TexturePools pools;
};
static int run_pool(const std::vector<rgk_texture>& tex, uint32_t flags, Pool& p) {
    rgk_scene_desc d;
    std::memset(&d, 0, sizeof(d));
    d.n_textures = (uint32_t)tex.size(); d.textures = tex.data(); d.build_flags = flags;
    assign_palettes(&d, p.palettes, p.tex_palette, p.pools);
    return pack_texels(&d, p.palettes, p.tex_palette, p.pools);
}
static rgk_texture float_texture(uint32_t w, uint32_t h, const std::vector<float>& texels) {
    rgk_texture t{};
    t.kind = RGK_TEX_RGB32F; t.width = w; t.height = h; t.texels = texels.data();
    return t;
}
static rgk_texture byte_texture(uint32_t w, uint32_t h, const std::vector<uint8_t>& bytes, const std::vector<float>& lut) {
    rgk_texture t{};
    t.kind = RGK_TEX_RGB8; t.width = w; t.height = h; t.texels8 = bytes.data(); t.lut = lut.data();
    return t;
}
static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
// tex_row / tex_col of rgk_device.h for a byte texture of width w, restated
static uint32_t row_of(uint32_t w, uint32_t y) { return (y >> 2) * (((w + 7u) >> 3) << 5) + ((y & 3u) << 3); }
static uint32_t col_of(uint32_t x) { return ((x >> 3) << 5) + (x & 7u); }

// Three caller tables (1 x 1 byte textures) and two few-valued float textures whose union fits one table: the callers' tables
// at 0, 256, 512 in the order of their first appearance -- a repeated table takes no new place --, the shared one at 768.
static void check_pool_tables() {
    std::vector<float> lut[3];
    for (int k = 0; k < 3; k++) for (int i = 0; i < 256; i++) lut[k].push_back((float)(k + 2) * (float)((i * 37 + k) & 255));
    const std::vector<uint8_t> px[4] = {{1, 2, 3}, {4, 5, 6}, {7, 8, 9}, {10, 11, 12}};
    std::vector<float> a, b;
    for (int i = 0; i < 3 * 8 * 6; i++) a.push_back(1000.5f + (float)(i % 120));          // 120 values
    for (int i = 0; i < 3 * 5 * 10; i++) b.push_back(1000.5f + (float)(60 + i % 130));     // 130 values, 60 of them a's: a union of 190
    const std::vector<rgk_texture> tex = {byte_texture(1, 1, px[0], lut[0]), float_texture(8, 6, a), byte_texture(1, 1, px[1], lut[1]), byte_texture(1, 1, px[3], lut[0]),
                                          byte_texture(1, 1, px[2], lut[2]), float_texture(5, 10, b)};
    Pool p;
    CHECK(run_pool(tex, 0u, p) == 0, "%s", rgk_last_error());
    const std::vector<TexRef>& R = p.pools.refs;
    CHECK(R.size() == 6 && p.pools.luts.size() == 4 * 256, "%zu refs, %zu table floats", R.size(), p.pools.luts.size());
    if (g_failed) return;
    CHECK(R[0].c == 0 && R[2].c == 256 && R[4].c == 512 && R[3].c == 0, "callers' tables at %u %u %u, the repeated one at %u", R[0].c, R[2].c, R[4].c, R[3].c);
    CHECK(R[1].c == 768 && R[5].c == 768, "shared table at %u and %u", R[1].c, R[5].c);
    CHECK(p.pools.n_float == 2 && p.pools.n_palettized == 2, "%u float, %u palettized", p.pools.n_float, p.pools.n_palettized);
    for (int k = 0; k < 3; k++) CHECK(std::memcmp(&p.pools.luts[256 * (size_t)k], lut[k].data(), 1024) == 0, "table %d is not the caller's", k);
    size_t bad = 0;
    for (int i : {1, 5}) {
        const rgk_texture& x = tex[(size_t)i];
        CHECK(R[(size_t)i].kind == RGK_TEX_RGB8, "T%d kind %u", i, R[(size_t)i].kind);
        for (uint32_t y = 0; y < x.height; y++)
            for (uint32_t xx = 0; xx < x.width; xx++) {
                const uint32_t w = p.pools.texels8[R[(size_t)i].b + row_of(x.width, y) + col_of(xx)];
                for (int ch = 0; ch < 3; ch++) bad += bits(p.pools.luts[768 + ((w >> (8 * ch)) & 255u)]) != bits(x.texels[3 * (y * x.width + xx) + (uint32_t)ch]);
            }
    }
    CHECK(bad == 0, "%zu channel values decode wrong through the shared table", bad);
    Pool keep; // RGK_BUILD_KEEP_FLOAT_TEXTURES: the callers' tables stay where they are, no table of the scene's own
    CHECK(run_pool(tex, RGK_BUILD_KEEP_FLOAT_TEXTURES, keep) == 0, "%s", rgk_last_error());
    CHECK(keep.pools.luts.size() == 3 * 256 && keep.pools.n_float == 2 && keep.pools.n_palettized == 0 && keep.pools.refs[1].kind == RGK_TEX_RGB32F && keep.pools.refs[4].c == 512,
          "keep-float: %zu table floats, %u palettized", keep.pools.luts.size(), keep.pools.n_palettized);
}

// Exactly 256 distinct values: bytes + table.  257: stays float.
static void check_pool_limits() {
    for (int n_vals : {256, 257}) {
        std::vector<float> t;
        for (int i = 0; i < 3 * 16 * 6; i++) t.push_back(-7.25f + 0.5f * (float)(i < n_vals ? i : (i * 7) % n_vals)); // 288 channel values
        std::set<uint32_t> distinct;
        for (float f : t) distinct.insert(bits(f));
        CHECK((int)distinct.size() == n_vals, "%zu distinct values", distinct.size());
        Pool p;
        CHECK(run_pool({float_texture(16, 6, t)}, 0u, p) == 0, "%s", rgk_last_error());
        if (g_failed) return;
        const TexRef& r = p.pools.refs[0];
        if (n_vals == 256) {
            CHECK(r.kind == RGK_TEX_RGB8 && p.pools.n_palettized == 1 && p.pools.luts.size() == 256 && p.pools.texels.empty(), "256 values: kind %u, %zu table floats", r.kind, p.pools.luts.size());
            size_t bad = 0;
            for (uint32_t y = 0; y < 6 && r.kind == RGK_TEX_RGB8; y++)
                for (uint32_t x = 0; x < 16; x++) {
                    const uint32_t w = p.pools.texels8[r.b + row_of(16, y) + col_of(x)];
                    for (int ch = 0; ch < 3; ch++) bad += bits(p.pools.luts[r.c + ((w >> (8 * ch)) & 255u)]) != bits(t[3 * (y * 16 + x) + (uint32_t)ch]);
                }
            CHECK(bad == 0, "%zu channel values decode wrong", bad);
        } else {
            CHECK(r.kind == RGK_TEX_RGB32F && p.pools.n_float == 1 && p.pools.n_palettized == 0 && p.pools.luts.empty() && p.pools.texels8.empty() && p.pools.texels.size() == 96,
                  "257 values: kind %u, %zu table floats, %zu byte texels", r.kind, p.pools.luts.size(), p.pools.texels8.size());
        }
    }
}

// +0.0, -0.0 and NaNs of different payloads and signs are different values: every texel decodes to its own bits.
static void check_pool_bits() {
    const uint32_t special[] = {0x00000000u, 0x80000000u, 0x7fc00000u, 0x7fc12345u, 0xffc00001u, 0x7f800000u, 0xff800000u, 0x00000001u, 0x80000001u, 0x3f800000u};
    const size_t ns = sizeof(special) / sizeof(special[0]);
    Lcg r;
    std::vector<float> t;
    for (size_t i = 0; i < 3 * 9 * 5; i++) t.push_back(from_bits(special[i < ns ? i : r.next() % ns]));
    for (size_t i = 0; i < ns; i++) CHECK(bits(t[i]) == special[i], "value %zu did not keep its bits on the way in: %08x", i, bits(t[i]));
    Pool p;
    CHECK(run_pool({float_texture(9, 5, t)}, 0u, p) == 0, "%s", rgk_last_error());
    if (g_failed) return;
    const TexRef& rr = p.pools.refs[0];
    CHECK(rr.kind == RGK_TEX_RGB8 && p.palettes.size() == 1 && p.palettes[0].vals.size() == ns, "kind %u, %zu values in the table", rr.kind, p.palettes.empty() ? (size_t)0 : p.palettes[0].vals.size());
    if (g_failed) return;
    size_t bad = 0;
    std::set<uint32_t> used;
    for (uint32_t y = 0; y < 5; y++)
        for (uint32_t x = 0; x < 9; x++) {
            const uint32_t w = p.pools.texels8[rr.b + row_of(9, y) + col_of(x)];
            for (int ch = 0; ch < 3; ch++) {
                const uint32_t byte = (w >> (8 * ch)) & 255u;
                used.insert(byte);
                bad += bits(p.pools.luts[rr.c + byte]) != bits(t[3 * (y * 9 + x) + (uint32_t)ch]);
            }
        }
    CHECK(bad == 0, "%zu channel values decode to other bits", bad);
    CHECK(used.size() == ns, "%zu table entries in use for %zu values", used.size(), ns);
}

// The smallest shapes of the tiled layout, (height, width) 1 x 1, 1 x 5, 9 x 1, 4 x 8, 5 x 9, 4 x 16, 3 x 7, each as a byte texture
// and as a few-valued float texture, one after the other in one pool: texel (x, y) lies at tex_row(y) + tex_col(x), everything
// else inside the texture's whole tiles is zero, and each texture starts on the 32-dword boundary where the one before ended.
static void check_pool_small() {
    const uint32_t sizes[7][2] = {{1, 1}, {1, 5}, {9, 1}, {4, 8}, {5, 9}, {4, 16}, {3, 7}};
    Lcg r;
    std::vector<float> lut(256), fvals;
    for (int i = 0; i < 256; i++) lut[(size_t)i] = 0.25f * (float)i - 3.0f;
    for (int i = 0; i < 100; i++) fvals.push_back(50.0625f + 0.125f * (float)i); // none of them in `lut`: a table of the scene's own
    std::vector<std::vector<uint8_t>> bytes(7);
    std::vector<std::vector<float>> floats(7);
    std::vector<rgk_texture> tex;
    for (int s = 0; s < 7; s++) {
        const uint32_t h = sizes[s][0], w = sizes[s][1];
        for (uint32_t k = 0; k < 3 * w * h; k++) { bytes[(size_t)s].push_back((uint8_t)(1u + r.next() % 255u)); floats[(size_t)s].push_back(fvals[1 + r.next() % 99]); } // no zero word: padding shows
        floats[(size_t)s][0] = fvals[0];
    }
    for (int s = 0; s < 7; s++) {
        tex.push_back(byte_texture(sizes[s][1], sizes[s][0], bytes[(size_t)s], lut));
        tex.push_back(float_texture(sizes[s][1], sizes[s][0], floats[(size_t)s]));
    }
    Pool p;
    CHECK(run_pool(tex, 0u, p) == 0, "%s", rgk_last_error());
    if (g_failed) return;
    CHECK(p.pools.n_float == 7 && p.pools.n_palettized == 7 && p.pools.luts.size() == 512 && p.pools.texels.empty(), "%u float, %u palettized, %zu table floats", p.pools.n_float,
          p.pools.n_palettized, p.pools.luts.size());
    size_t at = 0;
    for (size_t i = 0; i < tex.size(); i++) {
        const rgk_texture& x = tex[i];
        const TexRef& rr = p.pools.refs[i];
        const size_t span = ((x.width + 7) / 8) * ((x.height + 3) / 4) * 32;
        CHECK(rr.kind == RGK_TEX_RGB8 && rr.a == (x.width | (x.height << 16)) && rr.c == (x.kind == RGK_TEX_RGB8 ? 0u : 256u), "T%zu: kind %u size %08x table %u", i, rr.kind, rr.a, rr.c);
        CHECK(rr.b == at && rr.b % 32 == 0, "T%zu (%u x %u) starts at %u, the one before ended at %zu", i, x.height, x.width, rr.b, at);
        CHECK(rr.b + span <= p.pools.texels8.size(), "T%zu: outside the pool", i);
        if (g_failed) return;
        std::vector<uint8_t> texel(span, 0);
        size_t bad = 0, twice = 0, pad_nonzero = 0;
        for (uint32_t y = 0; y < x.height; y++)
            for (uint32_t xx = 0; xx < x.width; xx++) {
                const uint32_t k = row_of(x.width, y) + col_of(xx);
                CHECK(k < span, "T%zu: texel (%u, %u) at %u of %zu", i, xx, y, k, span);
                if (k >= span) return;
                twice += texel[k]++;
                const uint32_t w = p.pools.texels8[rr.b + k];
                bad += (w >> 24) != 0;
                for (int ch = 0; ch < 3; ch++) {
                    const size_t src = 3 * ((size_t)y * x.width + xx) + (size_t)ch;
                    const uint32_t byte = (w >> (8 * ch)) & 255u;
                    if (x.kind == RGK_TEX_RGB8) bad += byte != x.texels8[src] || bits(p.pools.luts[rr.c + byte]) != bits(lut[x.texels8[src]]);
                    else bad += bits(p.pools.luts[rr.c + byte]) != bits(x.texels[src]);
                }
            }
        for (size_t k = 0; k < span; k++) pad_nonzero += !texel[k] && p.pools.texels8[rr.b + k] != 0u;
        CHECK(bad == 0 && twice == 0 && pad_nonzero == 0, "T%zu (%u x %u): %zu texels wrong, %zu places used twice, %zu padding words not zero", i, x.height, x.width, bad, twice, pad_nonzero);
        at += span;
    }
    CHECK(at == p.pools.texels8.size(), "pool of %zu dwords, textures cover %zu", p.pools.texels8.size(), at);
    CHECK(p.pools.refs[13].b == p.pools.refs[12].b + 32 && p.pools.refs[12].b % 32 == 0, "the texture after the 3 x 7 one starts at %u, the 3 x 7 one at %u", p.pools.refs[13].b, p.pools.refs[12].b);
}

// ------------------------------------------------------------------ small cases
static uint32_t eligible(const std::vector<rgk_pointlight>& lights, float areal_power) {
    rgk_scene_desc d;
    std::memset(&d, 0, sizeof(d));
    d.n_pointlights = (uint32_t)lights.size(); d.pointlights = lights.data();
    DevScene ds;
    std::memset(&ds, 0, sizeof(ds));
    const std::vector<DevPointLight> pls = build_point_lights(&d, ds.total_point_power);
    ds.n_pointlights = (uint32_t)pls.size(); ds.n_areal = areal_power > 0.f ? 1u : 0u; ds.total_areal_power = areal_power;
    return const_light_eligible(ds, pls.data());
}

static void check_small() {
    {   // commit_bounds
        const Geometry g = make_single_leaf();
        float mn[3], mx[3], eps = -1.f, wmn[3] = {1e30f, 1e30f, 1e30f}, wmx[3] = {-1e30f, -1e30f, -1e30f};
        for (size_t k = 0; k < g.v.size(); k++) { wmn[k % 3] = std::min(wmn[k % 3], g.v[k]); wmx[k % 3] = std::max(wmx[k % 3], g.v[k]); }
        CHECK(commit_bounds(g.v.data(), g.idx.data(), g.nt(), mn, mx, &eps) == 0, "%s", rgk_last_error());
        const float xs = wmx[0] - wmn[0], ys = wmx[1] - wmn[1], zs = wmx[2] - wmn[2];
        CHECK(std::memcmp(mn, wmn, 12) == 0 && std::memcmp(mx, wmx, 12) == 0, "box");
        CHECK(bits(eps) == bits(0.00001f * std::sqrt(xs * xs + ys * ys + zs * zs)), "epsilon %g", eps);
        Geometry h = g;
        h.v[4] = INFINITY;
        CHECK(commit_bounds(h.v.data(), h.idx.data(), h.nt(), mn, mx, &eps) == RGK_ERR_INVALID, "an infinite coordinate was accepted");
        CHECK(std::string(rgk_last_error()) == "non-finite vertex coordinates", "%s", rgk_last_error());
    }
    {   // const_light_eligible
        rgk_pointlight l{};
        l.pos[0] = 1.f; l.pos[1] = 2.f; l.pos[2] = 3.f; l.color[0] = l.color[1] = l.color[2] = 1.f; l.intensity = 7.5f; l.size = 0.f;
        rgk_pointlight sized = l, negzero = l;
        sized.size = 0.1f; negzero.pos[1] = -0.0f;
        CHECK(eligible({l}, 0.f) == 1, "one point light of size 0");
        CHECK(eligible({sized}, 0.f) == 0, "a sized light");
        CHECK(eligible({l, l}, 0.f) == 0, "two lights");
        CHECK(eligible({l}, 2.f) == 0, "a light plus an emitter");
        CHECK(eligible({negzero}, 0.f) == 0, "a -0.0 coordinate");
    }
    {   // build_areal_tables: the texture scene's emissive object, triangles of areas 0.5, 1, 3
        TextureScene s;
        make_texture_scene(s);
        std::vector<DevArealLight> als;
        std::vector<DevArealTri> ats;
        float total = -1.f;
        build_areal_tables(s.d.vertices, s.d.normals, s.d.tri_indices, s.d.tri_material, s.d.materials, 1, s.d.areal_offsets, s.d.areal_tris, als, ats, total);
        CHECK(als.size() == 1 && ats.size() == 3, "%zu lights, %zu triangles", als.size(), ats.size());
        if (als.size() == 1 && ats.size() == 3) {
            CHECK(ats[0].tri == 2 && ats[1].tri == 1 && ats[2].tri == 0, "order %u %u %u", ats[0].tri, ats[1].tri, ats[2].tri);
            CHECK(ats[0].area == 3.f && ats[1].area == 1.f && ats[2].area == 0.5f, "areas %g %g %g", ats[0].area, ats[1].area, ats[2].area);
            CHECK(als[0].total_area == 4.5f && als[0].power == 4.5f * (1.f + 2.f + 0.5f) && total == als[0].power, "area %g power %g total %g", als[0].total_area, als[0].power, total);
            CHECK(als[0].first == 0 && als[0].count == 3 && ats[0].a[0] == 8.f && ats[0].normal_a[2] == 1.f, "table layout");
        }
    }
    if (g_digest) { // the environment's switches, as read_build_options sees them
        const BuildOptions o = read_build_options();
        std::printf("[options] split %g max_leaf %d c_isect %g opt %d max_leaf_dev %d stack_ovf %d stack_lds %d walk_q %u rotate %d ploc %d morton_bits %d\n", o.split, o.max_leaf, o.c_isect,
                    o.opt_rounds, o.max_leaf_dev, (int)o.stack_ovf, o.stack_lds, o.walk_q, o.lbvh_rotate, o.lbvh_ploc, o.lbvh_morton_bits);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: commit_main <case> [--digest]\n"); return 2; }
    const std::string c = argv[1];
    g_digest = argc > 2 && std::string(argv[2]) == "--digest";
    BuildOptions o; // the defaults, whatever the environment says
    if (c == "geom-default") check_geometry(make_geometry(), o, true);
    else if (c == "geom-leaf1") { o.max_leaf = 1; check_geometry(make_geometry(), o, true); }
    else if (c == "geom-leaf16") { o.max_leaf = 16; check_geometry(make_geometry(), o, true); }
    else if (c == "geom-nosplit") { o.split = 0.f; check_geometry(make_geometry(), o, false); }
    else if (c == "geom-noopt") { o.opt_rounds = 0; check_geometry(make_geometry(), o, true); }
    else if (c == "geom-single") check_single_leaf();
    else if (c == "refit-pieces") check_refit_pieces();
    else if (c == "textures") check_textures();
    else if (c == "pool-tables") check_pool_tables();
    else if (c == "pool-limits") check_pool_limits();
    else if (c == "pool-bits") check_pool_bits();
    else if (c == "pool-small") check_pool_small();
    else if (c == "small") check_small();
    else { std::fprintf(stderr, "unknown case '%s'\n", c.c_str()); return 2; }
    if (g_failed) std::fprintf(stderr, "%d condition(s) failed in case %s\n", g_failed, c.c_str());
    return g_failed ? 1 : 0;
}
