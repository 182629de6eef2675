// Scene commit on the host (rgk_commit.h): no HIP runtime call in this file.
#include "rgk_commit.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iterator>
#include <limits>
#include <random>
#include <string>

namespace {
thread_local std::string g_err;
const float PI_F = 3.14159265358979323846264338327950288f; // RGK_PI_F
} // namespace

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char* rgk_last_error(void) { return g_err.c_str(); }
extern "C" __attribute__((visibility("hidden"))) int rgk_internal_fail(int code, const char* msg) { return fail(code, "%s", msg); }

// ------------------------------------------------------------------ build switches
BuildOptions read_build_options() {
    BuildOptions o;
    if (const char* e = std::getenv("RGK_BVH_SPLIT")) o.split = (float)std::atof(e);
    if (const char* e = std::getenv("RGK_BVH_MAXLEAF")) o.max_leaf = std::min(16, std::max(1, std::atoi(e)));
    if (const char* e = std::getenv("RGK_BVH_CISECT")) o.c_isect = (float)std::atof(e);
    if (const char* e = std::getenv("RGK_BVH_OPT")) o.opt_rounds = std::atoi(e);
    if (const char* e = std::getenv("RGK_BVH_MAXLEAF_DEV")) o.max_leaf_dev = std::min(16, std::max(1, std::atoi(e)));
    if (const char* e = std::getenv("RGK_STACK_OVF")) o.stack_ovf = e[0] != '0';
    if (const char* e = std::getenv("RGK_STACK_LDS")) o.stack_lds = std::atoi(e) == 32 ? 32 : 16;
    if (const char* e = std::getenv("RGK_WALK_Q")) o.walk_q = (uint32_t)std::atoi(e);
    if (const char* e = std::getenv("RGK_LBVH_ROTATE")) o.lbvh_rotate = std::max(0, std::min(32, std::atoi(e)));
    if (const char* e = std::getenv("RGK_LBVH_PLOC")) o.lbvh_ploc = std::max(0, std::min(256, std::atoi(e)));
    if (const char* e = std::getenv("RGK_LBVH_MORTON_BITS")) o.lbvh_morton_bits = std::max(1, std::atoi(e));
    return o;
}

// ------------------------------------------------------------------ descriptor checks
int validate_desc(const rgk_scene_desc* d) {
    if (!d) return fail(RGK_ERR_INVALID, "null scene descriptor");
    if (d->n_triangles == 0 || d->n_vertices == 0) return fail(RGK_ERR_INVALID, "scene has no geometry");
    if (!d->vertices || !d->normals || !d->tangents || !d->tri_indices || !d->tri_material)
        return fail(RGK_ERR_INVALID, "null geometry pointer");
    if (d->n_materials == 0 || !d->materials) return fail(RGK_ERR_INVALID, "scene has no materials");
    for (uint32_t i = 0; i < d->n_triangles; i++) {
        for (int k = 0; k < 3; k++)
            if (d->tri_indices[3 * i + k] >= d->n_vertices) return fail(RGK_ERR_INVALID, "triangle %u: vertex index out of range", i);
        if (d->tri_material[i] >= d->n_materials) return fail(RGK_ERR_INVALID, "triangle %u: material index out of range", i);
    }
    bool ggx = false, bek = false;
    for (uint32_t i = 0; i < d->n_materials; i++) {
        const rgk_material& m = d->materials[i];
        if (m.kind > RGK_BXDF_LTC_GGX_DIFFUSE) return fail(RGK_ERR_INVALID, "material %u: unknown bxdf kind %u", i, m.kind);
        const int32_t t[3] = {m.tex_diffuse, m.tex_color, m.tex_bump};
        for (int k = 0; k < 3; k++)
            if (t[k] >= (int32_t)d->n_textures) return fail(RGK_ERR_INVALID, "material %u: texture index out of range", i);
        if (m.kind == RGK_BXDF_MIX && (m.mix_m1 < 0 || m.mix_m2 < 0 || m.mix_m1 >= (int32_t)d->n_materials || m.mix_m2 >= (int32_t)d->n_materials))
            return fail(RGK_ERR_INVALID, "material %u: mix children out of range", i);
        if (m.kind == RGK_BXDF_LTC_GGX || m.kind == RGK_BXDF_LTC_GGX_DIFFUSE) ggx = true;
        if (m.kind == RGK_BXDF_LTC_BECKMANN || m.kind == RGK_BXDF_LTC_BECKMANN_DIFFUSE) bek = true;
    }
    {   // BxDFMix recurses (bxdf.cpp:235-249); the kernels evaluate a mix of mixes of leaves (two levels) without recursion.
        // Anything deeper, or a mix that reaches itself, is refused here rather than rendered wrong.
        std::vector<int> depth(d->n_materials, -1); // -1 unvisited, -2 on the current walk
        struct Walk {
            const rgk_scene_desc* d; std::vector<int>& depth;
            int go(uint32_t i) {
                if (d->materials[i].kind != RGK_BXDF_MIX) return depth[i] = 0;
                if (depth[i] == -2) return -1; // cycle
                if (depth[i] >= 0) return depth[i];
                depth[i] = -2;
                const int a = go((uint32_t)d->materials[i].mix_m1), b = go((uint32_t)d->materials[i].mix_m2);
                if (a < 0 || b < 0) return -1;
                return depth[i] = 1 + std::max(a, b);
            }
        } walk{d, depth};
        for (uint32_t i = 0; i < d->n_materials; i++) {
            const int k = walk.go(i);
            if (k < 0) return fail(RGK_ERR_INVALID, "material %u: mix materials form a cycle", i);
            if (k > 2) return fail(RGK_ERR_UNSUPPORTED, "material %u: mix nested %d levels deep (at most 2 are evaluated)", i, k);
        }
    }
    if (ggx && !d->ltc_ggx) return fail(RGK_ERR_INVALID, "LTC GGX material without ltc_ggx table");
    if (bek && !d->ltc_beckmann) return fail(RGK_ERR_INVALID, "LTC Beckmann material without ltc_beckmann table");
    for (uint32_t i = 0; i < d->n_textures; i++) {
        const rgk_texture& t = d->textures[i];
        if (t.kind == RGK_TEX_RGB32F && (!t.texels || t.width == 0 || t.height == 0)) return fail(RGK_ERR_INVALID, "texture %u: empty image", i);
        if (t.kind == RGK_TEX_RGB8 && (!t.texels8 || !t.lut || t.width == 0 || t.height == 0)) return fail(RGK_ERR_INVALID, "texture %u: empty 8-bit image", i);
        if (t.kind > RGK_TEX_RGB8) return fail(RGK_ERR_INVALID, "texture %u: unknown kind", i);
    }
    for (uint32_t i = 0; i < d->n_areal_lights; i++)
        for (uint32_t j = d->areal_offsets[i]; j < d->areal_offsets[i + 1]; j++)
            if (d->areal_tris[j] >= d->n_triangles) return fail(RGK_ERR_INVALID, "areal light %u: triangle out of range", i);
    if (d->sky_mode == RGK_SKY_ENVMAP && (d->sky_texture < 0 || d->sky_texture >= (int32_t)d->n_textures))
        return fail(RGK_ERR_INVALID, "sky envmap texture out of range");
    return 0;
}

// RGK_DEBUG_DESC=1: one line per table of the descriptor with an FNV-1a digest of its bytes, on stderr -- lets a host binding
// be checked against a known-good one ("did my flattening hand over the same scene?") without a debugger.
void debug_desc(const rgk_scene_desc* d) {
    auto h = [](const void* p, size_t n) { uint64_t x = 1469598103934665603ull; const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; p && i < n; i++) { x ^= b[i]; x *= 1099511628211ull; } return (unsigned long long)x; };
    std::fprintf(stderr, "[rgk desc] vertices %u %016llx normals %016llx tangents %016llx texcoords %016llx\n", d->n_vertices, h(d->vertices, 12ull * d->n_vertices),
                 h(d->normals, 12ull * d->n_vertices), h(d->tangents, 12ull * d->n_vertices), h(d->texcoords, 8ull * d->n_vertices));
    std::fprintf(stderr, "[rgk desc] triangles %u idx %016llx mat %016llx\n", d->n_triangles, h(d->tri_indices, 12ull * d->n_triangles), h(d->tri_material, 4ull * d->n_triangles));
    for (uint32_t i = 0; i < d->n_materials; i++) {
        const rgk_material& m = d->materials[i];
        std::fprintf(stderr, "[rgk desc] material %u kind %u flags %u emission %g %g %g rough %.9g ior %.9g amount %.9g tex %d %d %d mix %d %d\n", i, m.kind, m.flags, m.emission[0], m.emission[1],
                     m.emission[2], m.roughness, m.ior, m.amount, m.tex_diffuse, m.tex_color, m.tex_bump, m.mix_m1, m.mix_m2);
    }
    for (uint32_t i = 0; i < d->n_textures; i++) {
        const rgk_texture& t = d->textures[i];
        const size_t n = (size_t)t.width * t.height;
        std::fprintf(stderr, "[rgk desc] texture %u kind %u %ux%u color %.9g %.9g %.9g texels %016llx\n", i, t.kind, t.width, t.height, t.color[0], t.color[1], t.color[2],
                     t.kind == RGK_TEX_RGB32F ? h(t.texels, 12 * n) : (t.kind == RGK_TEX_RGB8 ? h(t.texels8, 3 * n) ^ h(t.lut, 1024) : 0ull));
    }
    std::fprintf(stderr, "[rgk desc] pointlights %u %016llx areal %u offsets %016llx tris %016llx\n", d->n_pointlights, h(d->pointlights, sizeof(rgk_pointlight) * (size_t)d->n_pointlights),
                 d->n_areal_lights, h(d->areal_offsets, 4ull * (d->n_areal_lights + 1)), h(d->areal_tris, d->n_areal_lights ? 4ull * d->areal_offsets[d->n_areal_lights] : 0));
    std::fprintf(stderr, "[rgk desc] sky mode %u color %.9g %.9g %.9g intensity %.9g rotate %.9g tex %d ltc %016llx %016llx\n", d->sky_mode, d->sky_color[0], d->sky_color[1], d->sky_color[2],
                 d->sky_intensity, d->sky_rotate, d->sky_texture, h(d->ltc_ggx, 4096 * 20), h(d->ltc_beckmann, 4096 * 20));
}

// ------------------------------------------------------------------ bounds, records, references
int commit_bounds(const float* vertices, const uint32_t* tri_indices, uint32_t n_triangles, float mn[3], float mx[3], float* eps) {
    for (int a = 0; a < 3; a++) { mn[a] = std::numeric_limits<float>::infinity(); mx[a] = -mn[a]; }
    for (size_t k = 0; k < 3 * (size_t)n_triangles; k++) {
        const float* v = vertices + 3 * (size_t)tri_indices[k];
        for (int a = 0; a < 3; a++) { if (v[a] < mn[a]) mn[a] = v[a]; if (v[a] > mx[a]) mx[a] = v[a]; }
    }
    const float xs = mx[0] - mn[0], ys = mx[1] - mn[1], zs = mx[2] - mn[2];
    const float diameter = std::sqrt(xs * xs + ys * ys + zs * zs);
    *eps = 0.00001f * diameter;
    if (!(*eps == *eps) || !(diameter < std::numeric_limits<float>::infinity())) return fail(RGK_ERR_INVALID, "non-finite vertex coordinates");
    return 0;
}

namespace {

// Early split clipping of large triangles (reference-splitting before the build): a triangle whose box is longer
// than `lmax` on some axis enters the build as several references, one per piece of the triangle clipped at the
// box midpoint, each with the tight box of its piece.  The pieces tile the triangle, so every hit point lies in
// the (eps-padded) box of a reference; the leaf records are whole triangles, so a hit is what it was -- the tree
// just stops dragging wall- and floor-sized boxes through its upper levels.
struct RefSplitter {
    struct P3 { double x[3]; };
    float lmax;
    size_t budget; // extra references still allowed
    std::vector<Prim>* out;
    double tv[3][3]; // the triangle being split (for the pieces' parameter boxes)
    void param_box(const std::vector<P3>& poly, float pb[4]) const {
        double e1[3], e2[3], a11 = 0, a12 = 0, a22 = 0;
        for (int k = 0; k < 3; k++) { e1[k] = tv[1][k] - tv[0][k]; e2[k] = tv[2][k] - tv[0][k]; a11 += e1[k] * e1[k]; a12 += e1[k] * e2[k]; a22 += e2[k] * e2[k]; }
        const double det = a11 * a22 - a12 * a12;
        double b0 = 1, b1 = 0, c0 = 1, c1 = 0;
        if (!(det > 0)) { pb[0] = 0.f; pb[1] = 1.f; pb[2] = 0.f; pb[3] = 1.f; return; }
        for (const P3& v : poly) {
            double r1 = 0, r2 = 0;
            for (int k = 0; k < 3; k++) { const double w = v.x[k] - tv[0][k]; r1 += e1[k] * w; r2 += e2[k] * w; }
            const double b = (a22 * r1 - a12 * r2) / det, c = (a11 * r2 - a12 * r1) / det;
            b0 = std::min(b0, b); b1 = std::max(b1, b); c0 = std::min(c0, c); c1 = std::max(c1, c);
        }
        const double pad = 1e-5; // (the solve's rounding; the pieces overlap by this much)
        pb[0] = (float)std::max(0.0, b0 - pad); pb[1] = (float)std::min(1.0, b1 + pad); pb[2] = (float)std::max(0.0, c0 - pad); pb[3] = (float)std::min(1.0, c1 + pad);
    }
    static void clip(const std::vector<P3>& in, int ax, double plane, bool keep_below, std::vector<P3>& res) {
        res.clear();
        const size_t n = in.size();
        for (size_t i = 0; i < n; i++) {
            const P3 &a = in[i], &b = in[(i + 1) % n];
            const bool ia = keep_below ? a.x[ax] <= plane : a.x[ax] >= plane, ib = keep_below ? b.x[ax] <= plane : b.x[ax] >= plane;
            if (ia) res.push_back(a);
            if (ia != ib) {
                const double t = (plane - a.x[ax]) / (b.x[ax] - a.x[ax]);
                P3 m;
                for (int k = 0; k < 3; k++) m.x[k] = a.x[k] + t * (b.x[k] - a.x[k]);
                m.x[ax] = plane;
                res.push_back(m);
            }
        }
    }
    void emit(const std::vector<P3>& poly, const float* bmin, const float* bmax, uint32_t tri, int depth) {
        // tight box of the piece: polygon bounds (outward-rounded to float) within the parent's box
        Prim p;
        for (int a = 0; a < 3; a++) {
            double lo = std::numeric_limits<double>::infinity(), hi = -lo;
            for (const P3& v : poly) { lo = std::min(lo, v.x[a]); hi = std::max(hi, v.x[a]); }
            float fl = (float)lo, fh = (float)hi;
            if ((double)fl > lo) fl = std::nextafterf(fl, -std::numeric_limits<float>::infinity());
            if ((double)fh < hi) fh = std::nextafterf(fh, std::numeric_limits<float>::infinity());
            p.bmin[a] = std::max(fl, bmin[a]); p.bmax[a] = std::min(fh, bmax[a]);
            if (p.bmin[a] > p.bmax[a]) p.bmin[a] = p.bmax[a] = 0.5f * (bmin[a] + bmax[a]);
        }
        int ax = 0;
        for (int a = 1; a < 3; a++) if (p.bmax[a] - p.bmin[a] > p.bmax[ax] - p.bmin[ax]) ax = a;
        if (!(p.bmax[ax] - p.bmin[ax] > lmax) || depth >= 12 || budget == 0 || poly.size() < 3) {
            for (int a = 0; a < 3; a++) p.c[a] = 0.5f * (p.bmin[a] + p.bmax[a]);
            p.tri = tri;
            p.ref = (uint32_t)out->size();
            if (depth == 0) { p.pb[0] = 0.f; p.pb[1] = 1.f; p.pb[2] = 0.f; p.pb[3] = 1.f; } else param_box(poly, p.pb);
            out->push_back(p);
            return;
        }
        budget--;
        const double mid = 0.5 * ((double)p.bmin[ax] + (double)p.bmax[ax]);
        std::vector<P3> lo, hi;
        clip(poly, ax, mid, true, lo);
        clip(poly, ax, mid, false, hi);
        float cmax[3] = {p.bmax[0], p.bmax[1], p.bmax[2]}, cmin[3] = {p.bmin[0], p.bmin[1], p.bmin[2]};
        cmax[ax] = std::nextafterf((float)mid, std::numeric_limits<float>::infinity());
        cmin[ax] = std::nextafterf((float)mid, -std::numeric_limits<float>::infinity());
        if (lo.size() >= 3) emit(lo, p.bmin, cmax, tri, depth + 1);
        if (hi.size() >= 3) emit(hi, cmin, p.bmax, tri, depth + 1);
    }
};

} // namespace

void commit_triangles(const float* vertices, const uint32_t* tri_indices, uint32_t n_triangles, float split_lmax, std::vector<TriIsect>& recs,
                      std::vector<Prim>& prims) {
    auto vert = [&](uint32_t i) { return V3{vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]}; };
    recs.assign(n_triangles, TriIsect{});
    prims.clear();
    prims.reserve(n_triangles);
    RefSplitter splitter;
    splitter.lmax = split_lmax;
    splitter.budget = (size_t)n_triangles; // at most 2x references
    splitter.out = &prims;
    for (uint32_t i = 0; i < n_triangles; i++) {
        V3 v0 = vert(tri_indices[3 * i]), v1 = vert(tri_indices[3 * i + 1]), v2 = vert(tri_indices[3 * i + 2]);
        const TriIsect& r = recs[i] = tri_isect_record(v0, v1, v2, i);
        if (r.n[0] == r.n[0] && r.n[1] == r.n[1] && r.n[2] == r.n[2]) { // a NaN plane can never be hit (primitives.cpp:90)
            Prim p;
            const Box b = tri_box(v0, v1, v2);
            for (int a = 0; a < 3; a++) { p.bmin[a] = b.mn[a]; p.bmax[a] = b.mx[a]; p.c[a] = 0.5f * (p.bmin[a] + p.bmax[a]); }
            p.tri = i;
            p.pb[0] = 0.f; p.pb[1] = 1.f; p.pb[2] = 0.f; p.pb[3] = 1.f;
            if (splitter.lmax > 0.f) {
                std::vector<RefSplitter::P3> poly(3);
                for (int a = 0; a < 3; a++) { poly[0].x[a] = comp(v0, a); poly[1].x[a] = comp(v1, a); poly[2].x[a] = comp(v2, a); }
                for (int c = 0; c < 3; c++) for (int a = 0; a < 3; a++) splitter.tv[c][a] = poly[c].x[a];
                splitter.emit(poly, p.bmin, p.bmax, i, 0);
            } else {
                p.ref = (uint32_t)prims.size();
                prims.push_back(p);
            }
        }
    }
}

// ------------------------------------------------------------------ BVH build
namespace {

struct BvhBuilder {
    std::vector<Prim>& prims;
    std::vector<BvhNode> nodes;
    std::vector<uint32_t> order; // reference numbers (Prim::ref) in leaf order
    uint32_t max_depth = 0;
    float pad;
    static constexpr int NBINS = 16;
    int MAX_LEAF;                          // leaf encoding allows up to 16
    float C_TRAV = 1.0f, C_ISECT;          // SAH: one node step vs one triangle test (swept on MI355X: 1.0 best)
    BvhBuilder(std::vector<Prim>& p, float pad_, const BuildOptions& o) : prims(p), pad(pad_), MAX_LEAF(o.max_leaf), C_ISECT(o.c_isect) {}

    int make_leaf(size_t b, size_t e) {
        uint32_t first = order.size();
        for (size_t i = b; i < e; i++) order.push_back(prims[i].ref);
        return leaf_code(first, (uint32_t)(e - b));
    }
    // returns the child code for prims[b,e) and its (padded) box
    int build(size_t b, size_t e, uint32_t depth, Box& box) {
        max_depth = std::max(max_depth, depth);
        box.reset();
        Box cb;
        cb.reset();
        for (size_t i = b; i < e; i++) { box.grow(prims[i].bmin, prims[i].bmax); cb.grow(prims[i].c, prims[i].c); }
        size_t n = e - b;
        size_t mid = 0;
        bool leaf = (n == 1);
        if (!leaf) {
            float best = std::numeric_limits<float>::infinity();
            int best_axis = -1, best_bin = -1;
            float parent_area = box.area();
            for (int ax = 0; ax < 3; ax++) {
                float lo = cb.mn[ax], hi = cb.mx[ax];
                if (!(hi > lo)) continue;
                Box bb[NBINS];
                uint32_t cnt[NBINS] = {0};
                for (auto& x : bb) x.reset();
                float k = NBINS / (hi - lo);
                for (size_t i = b; i < e; i++) {
                    int bi = std::min(NBINS - 1, std::max(0, (int)((prims[i].c[ax] - lo) * k)));
                    cnt[bi]++;
                    bb[bi].grow(prims[i].bmin, prims[i].bmax);
                }
                float ra[NBINS];
                uint32_t rc[NBINS];
                Box acc;
                acc.reset();
                uint32_t c = 0;
                for (int i = NBINS - 1; i > 0; i--) { acc.grow(bb[i]); c += cnt[i]; ra[i] = acc.area(); rc[i] = c; }
                acc.reset();
                c = 0;
                for (int i = 0; i < NBINS - 1; i++) {
                    acc.grow(bb[i]);
                    c += cnt[i];
                    if (c == 0 || rc[i + 1] == 0) continue;
                    float cost = C_TRAV + C_ISECT * (acc.area() * c + ra[i + 1] * rc[i + 1]) / std::max(parent_area, 1e-30f);
                    if (cost < best) { best = cost; best_axis = ax; best_bin = i; }
                }
            }
            if (best_axis >= 0 && (n > (size_t)MAX_LEAF || best < C_ISECT * n)) {
                float lo = cb.mn[best_axis], hi = cb.mx[best_axis];
                float k = NBINS / (hi - lo);
                auto it = std::partition(prims.begin() + b, prims.begin() + e, [&](const Prim& p) {
                    int bi = std::min(NBINS - 1, std::max(0, (int)((p.c[best_axis] - lo) * k)));
                    return bi <= best_bin;
                });
                mid = it - prims.begin();
                if (mid == b || mid == e) best_axis = -1;
            } else if (best_axis >= 0) {
                leaf = true; // SAH prefers a leaf and it fits
                best_axis = 0;
            }
            if (!leaf && best_axis < 0) {
                if (n <= (size_t)MAX_LEAF) leaf = true;
                else { // coincident centroids: median split by index
                    int ax = 0;
                    float ex = -1;
                    for (int a = 0; a < 3; a++) if (box.mx[a] - box.mn[a] > ex) { ex = box.mx[a] - box.mn[a]; ax = a; }
                    mid = b + n / 2;
                    std::nth_element(prims.begin() + b, prims.begin() + mid, prims.begin() + e,
                                     [ax](const Prim& p, const Prim& q) { return p.c[ax] < q.c[ax]; });
                }
            }
        }
        box.pad(pad);
        if (leaf) return make_leaf(b, e);
        int idx = (int)nodes.size();
        nodes.emplace_back();
        Box lb, rb;
        int l = build(b, mid, depth + 1, lb);
        int r = build(mid, e, depth + 1, rb);
        BvhNode& nd = nodes[idx];
        for (int i = 0; i < 3; i++) { nd.lmin[i] = lb.mn[i]; nd.lmax[i] = lb.mx[i]; nd.rmin[i] = rb.mn[i]; nd.rmax[i] = rb.mx[i]; }
        nd.left = l; nd.right = r; nd.pad[0] = nd.pad[1] = 0;
        return idx;
    }
};

// ------------------------------------------------------------------ BVH2 optimisation by reinsertion
// The binned top-down build decides every split with local information; afterwards single subtrees are taken out and put back
// where the surface-area cost of the whole tree grows least (insertion-based optimisation, Bittner, Hapala, Havran 2013, in its
// simplest form: the largest nodes first, branch-and-bound search from the root).  Same triangles, same leaves, so the same
// hits; on the Sponza proxy 8 rounds over half of the nodes cut the surface-area cost by 4 % and the node visits per ray by
// 4 % (diffuse bounce rays) to 9 % (camera rays) -- tools/probe_wide_bvh.py measures it on the CPU.
static void optimise_bvh2(std::vector<BvhNode>& nodes, std::vector<uint32_t>& order, int rounds, float frac) {
    const int NI = (int)nodes.size();
    if (NI < 8 || rounds <= 0) return;
    std::vector<Box> box; std::vector<int> l, r, par, leaf_codes;
    box.reserve(2 * NI + 1); l.assign(NI, -1); r.assign(NI, -1);
    box.resize(NI);
    auto side_box = [](const BvhNode& n, bool left) { Box b; for (int a = 0; a < 3; a++) { b.mn[a] = left ? n.lmin[a] : n.rmin[a]; b.mx[a] = left ? n.lmax[a] : n.rmax[a]; } return b; };
    for (int i = 0; i < NI; i++) {
        for (int sd = 0; sd < 2; sd++) {
            const int code = sd == 0 ? nodes[i].left : nodes[i].right;
            const Box b = side_box(nodes[i], sd == 0);
            int id;
            if (code >= 0) { id = code; box[id] = b; }
            else { id = (int)box.size(); box.push_back(b); l.push_back(-1); r.push_back(-1); leaf_codes.resize(box.size(), 0); leaf_codes[id] = code; }
            (sd == 0 ? l[i] : r[i]) = id;
        }
    }
    leaf_codes.resize(box.size(), 0);
    const int N = (int)box.size();
    par.assign(N, -1);
    for (int i = 0; i < NI; i++) { par[l[i]] = i; par[r[i]] = i; }
    box[0] = box[l[0]]; box[0].grow(box[r[0]]);
    auto refit_up = [&](int n) { while (n >= 0) { Box b = box[l[n]]; b.grow(box[r[n]]); box[n] = b; n = par[n]; } };
    std::mt19937 rng(7);
    const auto heap_cmp = [](const std::pair<float, int>& a, const std::pair<float, int>& b) { return a.first > b.first; };
    std::vector<std::pair<float, int>> pq;
    for (int it = 0; it < rounds; it++) {
        std::vector<int> cand;
        const auto larger = [&](int a, int b) { const float x = box[a].area(), y = box[b].area(); return x > y || (x == y && a < b); };
        if (!(it & 1)) { // the largest nodes (they cost the most); bounded work per round: a 1 M-triangle tree moves its largest nodes only
            for (int i = 1; i < N; i++) if (par[i] > 0) cand.push_back(i);
            const size_t take = std::min<size_t>((size_t)(cand.size() * frac), 65536);
            std::nth_element(cand.begin(), cand.begin() + take, cand.end(), larger);
            cand.resize(take);
            std::sort(cand.begin(), cand.end(), larger);
        } else { // every other round: any nodes
            const size_t take = std::min<size_t>((size_t)(N * frac), 65536);
            for (size_t k = 0; k < take; k++) { const int i = (int)(rng() % (uint32_t)N); if (par[i] > 0) cand.push_back(i); }
        }
        for (int n : cand) {
            const int p = par[n];
            if (p <= 0) continue;
            const int g = par[p];
            const int sib = l[p] == n ? r[p] : l[p];
            (l[g] == p ? l[g] : r[g]) = sib; // n and its parent leave the tree: the sibling moves up
            par[sib] = g;
            refit_up(g);
            const Box nb = box[n];
            const float na = nb.area();
            float best = std::numeric_limits<float>::infinity();
            int bx = sib;
            pq.clear(); pq.push_back({0.f, 0});
            while (!pq.empty()) {
                std::pop_heap(pq.begin(), pq.end(), heap_cmp);
                const float ind = pq.back().first; const int x = pq.back().second;
                pq.pop_back();
                if (ind + na >= best) break;
                Box u = box[x]; u.grow(nb);
                const float total = ind + u.area();
                if (total < best && par[x] >= 0) { best = total; bx = x; } // (not above the root: node 0 stays the root)
                const float child_ind = total - box[x].area();
                if (l[x] >= 0 && child_ind + na < best) {
                    pq.push_back({child_ind, l[x]}); std::push_heap(pq.begin(), pq.end(), heap_cmp);
                    pq.push_back({child_ind, r[x]}); std::push_heap(pq.begin(), pq.end(), heap_cmp);
                }
            }
            const int xp = par[bx]; // p becomes the parent of (bx, n) where bx was
            (l[xp] == bx ? l[xp] : r[xp]) = p;
            par[p] = xp; l[p] = bx; r[p] = n; par[bx] = p; par[n] = p;
            refit_up(p);
        }
    }
    // back to the builder's form: inner nodes in depth-first order from node 0, leaves re-listed in that order
    std::vector<BvhNode> out; out.reserve(NI);
    std::vector<uint32_t> new_order; new_order.reserve(order.size());
    std::function<int(int)> emit = [&](int n) -> int {
        if (l[n] < 0) {
            const uint32_t code = ~(uint32_t)leaf_codes[n], first = leaf_first(code), cnt = leaf_count(code);
            const uint32_t nf = (uint32_t)new_order.size();
            for (uint32_t k = 0; k < cnt; k++) new_order.push_back(order[first + k]);
            return leaf_code(nf, cnt);
        }
        const int idx = (int)out.size();
        out.emplace_back();
        const int a = emit(l[n]), b = emit(r[n]);
        BvhNode& nd = out[idx];
        for (int k = 0; k < 3; k++) { nd.lmin[k] = box[l[n]].mn[k]; nd.lmax[k] = box[l[n]].mx[k]; nd.rmin[k] = box[r[n]].mn[k]; nd.rmax[k] = box[r[n]].mx[k]; }
        nd.left = a; nd.right = b; nd.pad[0] = nd.pad[1] = 0;
        return idx;
    };
    emit(0);
    nodes.swap(out);
    order.swap(new_order);
}

// ------------------------------------------------------------------ BVH2 -> quantised BVH4
// Collapse the binary tree (always open the inner child with the largest surface until four
// children) and quantise each child box to 8 bits per plane relative to the node's box (quantise_axis, rgk_tree.h).
struct QbvhBuilder {
    const std::vector<BvhNode>& bn;
    std::vector<QNode> out;
    uint32_t max_stack = 0, max_depth = 0;
    explicit QbvhBuilder(const std::vector<BvhNode>& b) : bn(b) {}
    struct Child { int ref; Box box; };

    static bool valid(const Box& b) { return b.mn[0] <= b.mx[0] && b.mn[1] <= b.mx[1] && b.mn[2] <= b.mx[2]; }
    void children_of(int node, Child& l, Child& r) const {
        const BvhNode& n = bn[node];
        l.ref = n.left; r.ref = n.right;
        for (int a = 0; a < 3; a++) { l.box.mn[a] = n.lmin[a]; l.box.mx[a] = n.lmax[a]; r.box.mn[a] = n.rmin[a]; r.box.mx[a] = n.rmax[a]; }
    }
    // `stack_before`: entries a traversal may already hold when it reaches this node
    int collapse(int node, uint32_t depth, uint32_t stack_before) {
        std::vector<Child> ch(2);
        children_of(node, ch[0], ch[1]);
        ch.erase(std::remove_if(ch.begin(), ch.end(), [](const Child& c) { return !valid(c.box); }), ch.end());
        while (ch.size() < 4) {
            int best = -1;
            float best_area = -1.f;
            for (size_t i = 0; i < ch.size(); i++)
                if (ch[i].ref >= 0 && ch[i].box.area() > best_area) { best_area = ch[i].box.area(); best = (int)i; }
            if (best < 0) break;
            Child a, b;
            children_of(ch[best].ref, a, b);
            ch.erase(ch.begin() + best);
            if (valid(a.box)) ch.push_back(a);
            if (valid(b.box)) ch.push_back(b);
        }
        int idx = (int)out.size();
        out.emplace_back();
        max_depth = std::max(max_depth, depth);
        const uint32_t pushed = (uint32_t)ch.size() - 1;
        max_stack = std::max(max_stack, stack_before + pushed);
        Box nb;
        nb.reset();
        for (auto& c : ch) nb.grow(c.box);
        QNode q;
        std::memset(&q, 0, sizeof(q));
        Box cb[4];
        for (size_t i = 0; i < ch.size(); i++) cb[i] = ch[i].box;
        for (int a = 0; a < 3; a++) {
            q.p[a] = nb.mn[a];
            quantise_axis(cb, (int)ch.size(), a, q.p[a], nb.mx[a] - nb.mn[a], a == 0 ? q.sx : (a == 1 ? q.sy : q.sz), q.qlo[a], q.qhi[a]);
        }
        for (size_t i = 0; i < 4; i++) q.child[i] = RGK_QNODE_EMPTY;
        out[idx] = q;
        for (size_t i = 0; i < ch.size(); i++) {
            int ref = ch[i].ref;
            if (ref >= 0) ref = collapse(ref, depth + 1, stack_before + pushed);
            out[idx].child[i] = ref;
        }
        return idx;
    }
};

} // namespace

int build_host_accel(std::vector<Prim>& prims, const std::vector<TriIsect>& recs, float pad, const BuildOptions& opt, HostAccel& out) {
    std::vector<uint32_t> ref_tri(prims.size());
    std::vector<float4> ref_pb(prims.size());
    for (const Prim& p : prims) { ref_tri[p.ref] = p.tri; ref_pb[p.ref] = make_float4(p.pb[0], p.pb[1], p.pb[2], p.pb[3]); }
    BvhBuilder bb(prims, pad, opt);
    Box rootbox;
    bb.nodes.reserve(prims.size());
    bb.nodes.emplace_back(); // node 0 = root, filled below if the whole scene is one leaf
    int code;
    if (prims.size() <= (size_t)bb.MAX_LEAF) {
        code = bb.build(0, prims.size(), 1, rootbox);
        BvhNode& r = bb.nodes[0];
        for (int a = 0; a < 3; a++) {
            r.lmin[a] = rootbox.mn[a]; r.lmax[a] = rootbox.mx[a];
            r.rmin[a] = std::numeric_limits<float>::infinity(); r.rmax[a] = -std::numeric_limits<float>::infinity();
        }
        r.left = code; r.right = code; r.pad[0] = r.pad[1] = 0;
    } else {
        bb.nodes.pop_back();
        code = bb.build(0, prims.size(), 0, rootbox);
        if (code != 0) return fail(RGK_ERR_DEVICE, "internal: BVH root is not node 0");
        optimise_bvh2(bb.nodes, bb.order, opt.opt_rounds, 0.5f);
    }
    out.leaf_recs.clear(); out.leaf_pb.clear();
    out.leaf_recs.reserve(bb.order.size());
    out.leaf_pb.reserve(bb.order.size());
    for (uint32_t r : bb.order) { out.leaf_recs.push_back(recs[ref_tri[r]]); out.leaf_pb.push_back(ref_pb[r]); }
    QbvhBuilder qb(bb.nodes);
    qb.out.reserve(bb.nodes.size() / 2 + 1);
    if (qb.collapse(0, 0, 0) != 0) return fail(RGK_ERR_DEVICE, "internal: QBVH root is not node 0");
    out.qnodes.swap(qb.out);
    out.max_depth = qb.max_depth; out.max_stack = qb.max_stack;
    return 0;
}

// ------------------------------------------------------------------ shading tables
std::vector<TriShade> build_tri_shade(const rgk_scene_desc* d) {
    std::vector<TriShade> tsh(d->n_triangles);
    for (uint32_t i = 0; i < d->n_triangles; i++) {
        TriShade& t = tsh[i];
        std::memset(&t, 0, sizeof(t));
        const uint32_t v[3] = {d->tri_indices[3 * i], d->tri_indices[3 * i + 1], d->tri_indices[3 * i + 2]};
        float uvs[6];
        for (int k = 0; k < 3; k++) {
            for (int a = 0; a < 3; a++) { t.q[k][a] = d->normals[3 * v[k] + a]; t.q[3 + k][a] = d->tangents[3 * v[k] + a]; }
            uvs[2 * k] = d->texcoords ? d->texcoords[2 * v[k]] : 0.f;
            uvs[2 * k + 1] = d->texcoords ? d->texcoords[2 * v[k] + 1] : 0.f;
        }
        for (int k = 0; k < 6; k++) t.q[k][3] = uvs[k]; // uvA.x uvA.y uvB.x uvB.y uvC.x uvC.y
        t.mat = d->tri_material[i];
    }
    return tsh;
}

// ------------------------------------------------------------------ textures
// Image texels go into one float4 pool (float textures) or one dword pool + byte -> float tables (8-bit ones).
// A float texture whose channel values are at most 256 distinct floats is what a loader leaves that decodes an 8-bit
// file to floats and keeps only those (the reference: Color(byte / 255).gammaDecode(2.2) per channel,
// src/texture.cpp:203,252-254, every FileTexture it holds).  Such a texture is stored as bytes + the table of its values --
// bit-identical by construction (the table holds the very floats), a quarter of the texel traffic, and the table sits in LDS.
// Textures share a table while the union of their value sets fits 256 entries (one table for all of Sponza's 17 images).
namespace {

uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// The caller-supplied table equal to `lut` (256 floats), or null.
const Palette* find_fixed_palette(const std::vector<Palette>& palettes, const std::vector<float>& luts, const float* lut) {
    for (const Palette& p : palettes)
        if (p.fixed && std::memcmp(&luts[p.lut_off], lut, 256 * sizeof(float)) == 0) return &p;
    return nullptr;
}

// The distinct channel values of a float texture, sorted; false at the 257th (open addressing, 1024 slots).
bool distinct_values(const rgk_texture& t, std::vector<uint32_t>& vals) {
    std::vector<uint32_t> slots(1024, 0u);
    std::vector<uint8_t> used(1024, 0);
    const size_t n = (size_t)3 * t.width * t.height;
    for (size_t k = 0; k < n; k++) {
        const uint32_t u = bits_of(t.texels[k]);
        uint32_t h = (u * 2654435761u) >> 22;
        while (used[h] && slots[h] != u) h = (h + 1) & 1023u;
        if (!used[h]) { used[h] = 1; slots[h] = u; vals.push_back(u); if (vals.size() > 256) return false; }
    }
    std::sort(vals.begin(), vals.end());
    return true;
}

} // namespace

void assign_palettes(const rgk_scene_desc* d, std::vector<Palette>& palettes, std::vector<int>& tex_palette, TexturePools& pools) {
    std::vector<float>& luts = pools.luts;
    tex_palette.assign(d->n_textures, -1);
    for (uint32_t i = 0; i < d->n_textures; i++) { // caller-supplied tables first: a float texture whose values all occur in one shares it
        const rgk_texture& t = d->textures[i];
        if (t.kind != RGK_TEX_RGB8 || find_fixed_palette(palettes, luts, t.lut)) continue;
        Palette p; p.fixed = true; p.lut_off = (uint32_t)luts.size();
        luts.insert(luts.end(), t.lut, t.lut + 256);
        for (int k = 0; k < 256; k++) p.vals.push_back(bits_of(t.lut[k]));
        std::sort(p.vals.begin(), p.vals.end());
        p.vals.erase(std::unique(p.vals.begin(), p.vals.end()), p.vals.end());
        palettes.push_back(std::move(p));
    }
    if (!(d->build_flags & RGK_BUILD_KEEP_FLOAT_TEXTURES))
        for (uint32_t i = 0; i < d->n_textures; i++) {
            const rgk_texture& t = d->textures[i];
            if (t.kind != RGK_TEX_RGB32F || t.width > 65535 || t.height > 65535) continue;
            std::vector<uint32_t> vals;
            if (!distinct_values(t, vals)) continue;
            int pick = -1;
            for (size_t p = 0; p < palettes.size() && pick < 0; p++) // all of it already in a table?
                if (std::includes(palettes[p].vals.begin(), palettes[p].vals.end(), vals.begin(), vals.end())) pick = (int)p;
            for (size_t p = 0; p < palettes.size() && pick < 0; p++) { // a table of this scene's that can take the new values?
                if (palettes[p].fixed) continue;
                std::vector<uint32_t> u;
                std::set_union(palettes[p].vals.begin(), palettes[p].vals.end(), vals.begin(), vals.end(), std::back_inserter(u));
                if (u.size() <= 256) { palettes[p].vals.swap(u); pick = (int)p; }
            }
            if (pick < 0) { Palette p; p.fixed = false; p.lut_off = 0; p.vals = vals; palettes.push_back(std::move(p)); pick = (int)palettes.size() - 1; }
            tex_palette[i] = pick;
        }
    for (Palette& p : palettes) // this scene's own tables: the sorted values, padded with zeros
        if (!p.fixed) {
            p.lut_off = (uint32_t)luts.size();
            for (size_t k = 0; k < 256; k++) { float f = 0.f; if (k < p.vals.size()) std::memcpy(&f, &p.vals[k], 4); luts.push_back(f); }
        }
}

int pack_texels(const rgk_scene_desc* d, const std::vector<Palette>& palettes, const std::vector<int>& tex_palette, TexturePools& pools) {
    std::vector<float4>& pool = pools.texels;
    std::vector<uint32_t>& pool8 = pools.texels8;
    const std::vector<float>& luts = pools.luts;
    pools.refs.resize(d->n_textures);
    for (uint32_t i = 0; i < d->n_textures; i++) {
        const rgk_texture& t = d->textures[i];
        TexRef& o = pools.refs[i];
        o.kind = t.kind; o.a = o.b = o.c = 0;
        if (t.kind == RGK_TEX_SOLID) {
            std::memcpy(&o.a, &t.color[0], 4); std::memcpy(&o.b, &t.color[1], 4); std::memcpy(&o.c, &t.color[2], 4);
            continue;
        }
        if (t.width > 65535 || t.height > 65535) return fail(RGK_ERR_UNSUPPORTED, "texture %u larger than 65535 texels on a side", i);
        const size_t n = (size_t)t.width * t.height;
        o.a = t.width | (t.height << 16);
        if (t.kind == RGK_TEX_RGB8 || tex_palette[i] >= 0) {
            // byte texels lie in tiles of 8 x 4 (one 128-byte line; rgk_device.h tex_row / tex_col), the image padded up to whole tiles
            const size_t tiles_x = ((size_t)t.width + 7) / 8, tiles_y = ((size_t)t.height + 3) / 4, n_padded = RGK_TEX_TILED ? tiles_x * tiles_y * 32 : n;
            if (pool8.size() + n_padded >= (1ull << 30)) return fail(RGK_ERR_UNSUPPORTED, "8-bit texel pool exceeds 2^30 texels"); // 32-bit byte offsets
            o.kind = RGK_TEX_RGB8;
            while (pool8.size() % 32) pool8.push_back(0u); // a tile = a line: the pool itself is 128-byte aligned
            o.b = (uint32_t)pool8.size();
            const size_t pool_at = pool8.size();
            pool8.resize(pool_at + n_padded, 0u);
            auto put = [&](size_t k, uint32_t w) { // texel k = y * width + x  ->  its place in the tiled order
                const size_t x = k % t.width, y = k / t.width;
                pool8[pool_at + (RGK_TEX_TILED ? ((y >> 2) * tiles_x + (x >> 3)) * 32 + ((y & 3) << 3) + (x & 7) : k)] = w;
            };
            if (t.kind == RGK_TEX_RGB8) {
                if (const Palette* p = find_fixed_palette(palettes, luts, t.lut)) o.c = p->lut_off;
                for (size_t k = 0; k < n; k++)
                    put(k, (uint32_t)t.texels8[3 * k] | ((uint32_t)t.texels8[3 * k + 1] << 8) | ((uint32_t)t.texels8[3 * k + 2] << 16));
            } else { // a float texture with few distinct values: its texels as indices into the table (the first entry holding the value)
                pools.n_float++; pools.n_palettized++;
                const Palette& p = palettes[(size_t)tex_palette[i]];
                o.c = p.lut_off;
                std::vector<std::pair<uint32_t, uint8_t>> idx; // (bit pattern, table index), sorted by pattern
                for (int k = 255; k >= 0; k--) idx.push_back({bits_of(luts[p.lut_off + (size_t)k]), (uint8_t)k});
                std::stable_sort(idx.begin(), idx.end(), [](const std::pair<uint32_t, uint8_t>& a, const std::pair<uint32_t, uint8_t>& b) { return a.first < b.first || (a.first == b.first && a.second < b.second); });
                auto index_of = [&](float f) -> uint32_t {
                    const uint32_t u = bits_of(f);
                    auto it = std::lower_bound(idx.begin(), idx.end(), std::make_pair(u, (uint8_t)0));
                    return it->second; // present by construction
                };
                for (size_t k = 0; k < n; k++)
                    put(k, index_of(t.texels[3 * k]) | (index_of(t.texels[3 * k + 1]) << 8) | (index_of(t.texels[3 * k + 2]) << 16));
            }
        } else {
            pools.n_float++;
            if (pool.size() + n >= (1ull << 28)) return fail(RGK_ERR_UNSUPPORTED, "float texel pool exceeds 2^28 texels"); // 32-bit byte offsets
            o.b = (uint32_t)pool.size();
            pool.reserve(pool.size() + n);
            for (size_t k = 0; k < n; k++) pool.push_back(make_float4(t.texels[3 * k], t.texels[3 * k + 1], t.texels[3 * k + 2], 0.f));
        }
    }
    return 0;
}

TexRef tex_ref(const std::vector<TexRef>& refs, int32_t id) {
    TexRef r;
    r.kind = RGK_TEXREF_NONE; r.a = r.b = r.c = 0;
    return id < 0 ? r : refs[id];
}

std::vector<DevMaterial> build_materials(const rgk_scene_desc* d, const std::vector<TexRef>& refs) {
    std::vector<DevMaterial> mats(d->n_materials);
    for (uint32_t i = 0; i < d->n_materials; i++) {
        const rgk_material& m = d->materials[i];
        DevMaterial& o = mats[i];
        std::memset(&o, 0, sizeof(o));
        o.kind = m.kind; o.flags = m.flags;
        for (int k = 0; k < 3; k++) o.emission[k] = m.emission[k];
        o.roughness = m.roughness; o.ior = m.ior; o.amount = m.amount;
        o.t_diffuse = tex_ref(refs, m.tex_diffuse); o.t_color = tex_ref(refs, m.tex_color); o.t_bump = tex_ref(refs, m.tex_bump);
        o.mix_m1 = m.mix_m1; o.mix_m2 = m.mix_m2;
    }
    return mats;
}

// Point lights and their total power (scene.cpp:323-344)
std::vector<DevPointLight> build_point_lights(const rgk_scene_desc* d, float& total_power) {
    std::vector<DevPointLight> pls(d->n_pointlights);
    total_power = 0.f;
    for (uint32_t i = 0; i < d->n_pointlights; i++) {
        const rgk_pointlight& l = d->pointlights[i];
        DevPointLight& o = pls[i];
        for (int k = 0; k < 3; k++) { o.pos[k] = l.pos[k]; o.color[k] = l.color[k]; }
        o.intensity = l.intensity; o.size = l.size;
        total_power += l.intensity * 4.0f * PI_F;
    }
    return pls;
}

// Scene::Commit's areal-light tables (src/scene.cpp:323-344): per emissive object its triangles sorted by area (descending), the
// total area, power = area * (r + g + b).  Used by rgk_scene_create and, for moved vertices, by rgk_scene_refit.
void build_areal_tables(const float* vertices, const float* normals, const uint32_t* tri_indices, const uint32_t* tri_material, const rgk_material* materials,
                               uint32_t n_areal, const uint32_t* areal_offsets, const uint32_t* areal_tris, std::vector<DevArealLight>& als,
                               std::vector<DevArealTri>& ats, float& total_areal) {
    auto vert = [&](uint32_t i) { return V3{vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]}; };
    als.clear(); ats.clear(); total_areal = 0.f;
    for (uint32_t i = 0; i < n_areal; i++) {
        uint32_t b = areal_offsets[i], e = areal_offsets[i + 1];
        if (e <= b) continue;
        std::vector<std::pair<float, uint32_t>> twa;
        float total_area = 0.f;
        for (uint32_t j = b; j < e; j++) {
            uint32_t t = areal_tris[j];
            V3 A = vert(tri_indices[3 * t]), B = vert(tri_indices[3 * t + 1]), C = vert(tri_indices[3 * t + 2]);
            V3 c = crossv(sub(A, B), sub(C, B)); // Triangle::GetArea primitives.cpp:38-45
            float area = 0.5f * std::sqrt(dotv(c, c));
            twa.push_back({area, t});
            total_area += area;
        }
        const rgk_material& m0 = materials[tri_material[twa[0].second]];
        std::sort(twa.rbegin(), twa.rend()); // descending by (area, index)
        DevArealLight al{};
        al.total_area = total_area;
        for (int k = 0; k < 3; k++) al.emission[k] = m0.emission[k];
        al.power = total_area * (m0.emission[0] + m0.emission[1] + m0.emission[2]);
        al.first = (uint32_t)ats.size();
        al.count = (uint32_t)twa.size();
        for (auto& p : twa) {
            DevArealTri at{};
            at.area = p.first; at.tri = p.second; at.light = (uint32_t)als.size();
            uint32_t ia = tri_indices[3 * p.second], ib = tri_indices[3 * p.second + 1], ic = tri_indices[3 * p.second + 2];
            for (int k = 0; k < 3; k++) {
                at.a[k] = vertices[3 * ia + k]; at.b[k] = vertices[3 * ib + k]; at.c[k] = vertices[3 * ic + k];
                at.normal_a[k] = normals[3 * ia + k];
            }
            ats.push_back(at);
        }
        total_areal += al.power;
        als.push_back(al);
    }
}

void build_halton(std::vector<DevHaltonDim>& dims, std::vector<uint16_t>& perm) {
    // Faure permutations: the standard recursive construction the reference uses
    // (external/halton_sampler.h:574-604), one permutation per prime base.
    const unsigned max_base = 1619u;
    std::vector<std::vector<uint16_t>> perms(max_base + 1);
    for (unsigned k = 1; k <= 3; ++k) { perms[k].resize(k); for (unsigned i = 0; i < k; ++i) perms[k][i] = i; }
    for (unsigned base = 4; base <= max_base; ++base) {
        perms[base].resize(base);
        unsigned b = base / 2;
        if (base & 1) {
            for (unsigned i = 0; i + 1 < base; ++i) {
                uint16_t v = perms[base - 1][i];
                perms[base][i + (i >= b)] = v + (v >= b);
            }
            perms[base][b] = b;
        } else {
            for (unsigned i = 0; i < b; ++i) { perms[base][i] = 2 * perms[b][i]; perms[base][b + i] = 2 * perms[b][i] + 1; }
        }
    }
    for (unsigned p = 2; dims.size() < 256; p++) {
        bool prime = true;
        for (unsigned d = 2; d * d <= p; d++) if (p % d == 0) { prime = false; break; }
        if (!prime) continue;
        DevHaltonDim hd{};
        hd.base = p;
        uint64_t bk = p; unsigned k = 1;
        while (bk * p <= 500) { bk *= p; k++; }  // digits per table lookup in the reference
        uint64_t tot = bk; unsigned G = 1;
        while (tot * bk < (1ull << 32)) { tot *= bk; G++; } // lookups per sample
        hd.digits = k * G;
        hd.scale = float(0x1.fffffcp-1 / (double)tot);
        hd.perm_off = (uint32_t)perm.size();
        if (p > 2) { // exact u32 division by p: q = (t + ((n - t) >> 1)) >> (l - 1), t = mulhi(m, n)
            unsigned l = 0;
            while ((1u << l) < p) l++;
            hd.magic = (uint32_t)(((1ull << 32) * ((1ull << l) - p)) / p + 1);
            hd.shift = l - 1;
        }
        perm.insert(perm.end(), perms[p].begin(), perms[p].end());
        dims.push_back(hd);
    }
}

std::vector<float4> build_ltc_table(const float* ltc_ggx, const float* ltc_beckmann) {
    std::vector<float4> t(2 * 2 * 4096, make_float4(0.f, 0.f, 0.f, 0.f));
    const float* src[2] = {ltc_ggx, ltc_beckmann};
    for (int w = 0; w < 2; w++)
        for (int k = 0; src[w] && k < 4096; k++) {
            t[(size_t)w * 8192 + 2 * k] = make_float4(src[w][5 * k], src[w][5 * k + 1], src[w][5 * k + 2], src[w][5 * k + 3]);
            t[(size_t)w * 8192 + 2 * k + 1] = make_float4(src[w][5 * k + 4], 0.f, 0.f, 0.f);
        }
    return t;
}

// The constant-light route's eligibility (rgk.h rgk_scene_info::const_light): does random_light (rgk_device.h) return point
// light 0, at its own position, for EVERY sample?  One point light of size 0 and no areal light; no -0.0 in the position
// (light_code's pos + 0 * v would make it +0.0 for some v); and random_light's own two comparisons, in float with its own
// expressions, select light 0 for the largest `choice.x` the sampler returns, 1 - 2^-24.  Rounding is monotone: choice.x *
// total_power does not grow when choice.x shrinks, nor does q - intensity * 4 pi when q shrinks, so every smaller sample passes
// both comparisons too.  (A NaN or infinite power fails them and stays on the per-path route.)
uint32_t const_light_eligible(const DevScene& ds, const DevPointLight* pls) {
    if (ds.n_pointlights != 1 || ds.n_areal != 0) return 0;
    const DevPointLight& pl = pls[0];
    if (pl.size != 0.0f) return 0;
    for (int k = 0; k < 3; k++)
        if (pl.pos[k] == 0.0f && std::signbit(pl.pos[k])) return 0;
    volatile float total_power = ds.total_point_power + ds.total_areal_power; // (volatile: each step rounded to float, as on the device)
    if (total_power <= 0.0f) return 0;
    const float choice_max = 0x1.fffffep-1f;
    volatile float q = choice_max * total_power;
    if (!(q < ds.total_point_power)) return 0;
    volatile float step = pl.intensity * 4.0f;
    step = step * PI_F;
    q = q - step;
    if (!(q <= 0.0f)) return 0;
    return 1;
}

int build_shading_tables(const rgk_scene_desc* d, ShadingTables& out) {
    out.tri_shade = build_tri_shade(d);
    std::vector<Palette> palettes;
    std::vector<int> tex_palette;
    assign_palettes(d, palettes, tex_palette, out.tex);
    if (int rc = pack_texels(d, palettes, tex_palette, out.tex)) return rc;
    out.materials = build_materials(d, out.tex.refs);
    out.pointlights = build_point_lights(d, out.total_point_power);
    build_areal_tables(d->vertices, d->normals, d->tri_indices, d->tri_material, d->materials, d->n_areal_lights, d->areal_offsets, d->areal_tris, out.areal,
                       out.areal_tris, out.total_areal_power);
    build_halton(out.hdims, out.hperm);
    out.ltc = build_ltc_table(d->ltc_ggx, d->ltc_beckmann);
    return 0;
}
