// The pieces of the accelerator that the host builder (rgk_commit.cpp) and the device builder and refit (rgk_build.hip) both
// compute, written once: the box, the leaf child code, the 8-bit child-box quantiser, a triangle's intersection record and the
// box of a reference.  Like rgk_plan.h: pure functions -- no call into the HIP runtime -- marked RGK_HD (rgk_libm.h), so a
// kernel calls them too and the unit builds with any host compiler: what the device runs here is the source that
// tests/cpp/commit_main.cpp runs under sanitizers.  Math goes through __builtin_* (one spelling for both compilers, no <cmath>
// overload to resolve differently in device code) and rgk_sqrtf_ieee; everything is compiled without contraction.
#pragma once
#include <stdint.h>

#include "../../include/rgk_libm.h"
#include "device_types.h"

// ------------------------------------------------------------------ vectors
struct V3 {
    float x, y, z;
};
RGK_HD V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
RGK_HD V3 crossv(V3 x, V3 y) { return {x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y}; }
RGK_HD float dotv(V3 a, V3 b) {
    float tx = a.x * b.x, ty = a.y * b.y, tz = a.z * b.z;
    return tx + ty + tz;
}
RGK_HD V3 scale(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
RGK_HD V3 normv(V3 v) { return scale(v, 1.0f / rgk_sqrtf_ieee(dotv(v, v))); }
RGK_HD float comp(V3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }

// ------------------------------------------------------------------ the box
// std::min / std::max as comparisons, the host builder's spelling: of two equal operands (+0.0 and -0.0) the first is kept, and
// every host table keeps its bits.  The device build used fminf / fmaxf before; the two differ only in the sign of a zero -- a
// byte of QNode::p, never a hit or a visit (fma(q, s, -0.0) and fma(q, s, +0.0) decode to the same plane for every q).
RGK_HD float minf(float a, float b) { return b < a ? b : a; }
RGK_HD float maxf(float a, float b) { return a < b ? b : a; }

struct Box {
    float mn[3], mx[3];
    RGK_HD void reset() { for (int i = 0; i < 3; i++) { mn[i] = __builtin_inff(); mx[i] = -mn[i]; } }
    RGK_HD void grow(const float* a, const float* b) { for (int i = 0; i < 3; i++) { mn[i] = minf(mn[i], a[i]); mx[i] = maxf(mx[i], b[i]); } }
    RGK_HD void grow(const Box& o) { grow(o.mn, o.mx); }
    RGK_HD void pad(float e) { for (int i = 0; i < 3; i++) { mn[i] -= e; mx[i] += e; } }
    RGK_HD float area() const {
        float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
        if (dx < 0 || dy < 0 || dz < 0) return 0.f;
        return 2.f * (dx * dy + dy * dz + dz * dx);
    }
};
RGK_HD Box unite(Box a, const Box& b) { a.grow(b); return a; }

// ------------------------------------------------------------------ leaf child code
// A negative QNode / BvhNode child is a leaf: ~child = (first << 4) | (count - 1), `first` indexing the records in leaf order,
// count 1..16.  leaf_first / leaf_count take ~child.
RGK_HD int32_t leaf_code(uint32_t first, uint32_t count) { return (int32_t)~((first << 4) | (count - 1u)); }
RGK_HD uint32_t leaf_first(const uint32_t code) { return code >> 4; }
RGK_HD uint32_t leaf_count(const uint32_t code) { return (code & 15u) + 1u; }

// ------------------------------------------------------------------ 8-bit child boxes
// Quantise axis `a` of up to four child boxes against the node box [p, p + ext]: the smallest power-of-two step whose
// outward-rounded codes fit 8 bits, verified with the kernels' decode fma(q, step, p) -- a decoded box contains its child box.
// Slots from nch on get the inverted box (255, 0).  The search ends at 2^127; a box that fits not even there (a NaN or an
// infinity in it) gets the whole range.
RGK_HD void quantise_axis(const Box* ch, int nch, int a, float p, float ext, float& step, uint8_t* qlo, uint8_t* qhi) {
    int e = -126;
    if (ext > 0.f) (void)__builtin_frexpf(ext / 255.0f, &e);
    for (;; e++) {
        if (e < -126) e = -126;
        const float s = __builtin_ldexpf(1.0f, e);
        bool ok = true;
        uint8_t lo[4] = {0, 0, 0, 0}, hi[4] = {255, 255, 255, 255};
        for (int i = 0; i < nch; i++) {
            float fl = __builtin_floorf((ch[i].mn[a] - p) / s), fh = __builtin_ceilf((ch[i].mx[a] - p) / s);
            if (fl < 0.f) fl = 0.f;
            while (fl > 0.f && __builtin_fmaf(fl, s, p) > ch[i].mn[a]) fl -= 1.f;
            while (fh <= 255.f && __builtin_fmaf(fh, s, p) < ch[i].mx[a]) fh += 1.f;
            if (fh > 255.f || fl > 255.f) { ok = false; break; }
            lo[i] = (uint8_t)fl; hi[i] = (uint8_t)fh;
        }
        if (!ok && e < 127) continue;
        step = s;
        for (int i = 0; i < 4; i++) { qlo[i] = i < nch ? lo[i] : 255; qhi[i] = i < nch ? hi[i] : 0; }
        return;
    }
}

// ------------------------------------------------------------------ a triangle's record and a reference's box
// The plane (Triangle::CalculatePlane, primitives.cpp:24-36), the dominant axes and the vertex differences that
// TestIntersection (primitives.cpp:75-166) would recompute per call.  One sequence of IEEE operations for rgk_scene_create
// (host) and rgk_scene_refit (device), so a refitted scene holds the bits a fresh one would.
RGK_HD TriIsect tri_isect_record(V3 v0, V3 v1, V3 v2, uint32_t tri) {
    V3 d0 = sub(v1, v0), d1 = sub(v2, v0);
    V3 n = normv(crossv(d1, d0));
    TriIsect r;
    r.n[0] = n.x; r.n[1] = n.y; r.n[2] = n.z; r.d = -dotv(n, v0);
    int i1, i2;
    float ax = __builtin_fabsf(n.x), ay = __builtin_fabsf(n.y), az = __builtin_fabsf(n.z);
    if (ax > ay && ax > az) { i1 = 1; i2 = 2; }
    else if (ay > az) { i1 = 0; i2 = 2; }
    else { i1 = 0; i2 = 1; }
    r.v0a = comp(v0, i1); r.v0b = comp(v0, i2);
    r.q1x = comp(v1, i1) - comp(v0, i1); r.q1y = comp(v1, i2) - comp(v0, i2);
    r.q2x = comp(v2, i1) - comp(v0, i1); r.q2y = comp(v2, i2) - comp(v0, i2);
    r.axes = (uint32_t)i1 | ((uint32_t)i2 << 2);
    r.tri = tri;
    return r;
}

RGK_HD Box tri_box(V3 v0, V3 v1, V3 v2) {
    Box b;
    for (int a = 0; a < 3; a++) {
        b.mn[a] = minf(comp(v0, a), minf(comp(v1, a), comp(v2, a)));
        b.mx[a] = maxf(comp(v0, a), maxf(comp(v1, a), comp(v2, a)));
    }
    return b;
}
// The box of the piece {v0 + b (v1 - v0) + c (v2 - v0): b in [pb[0], pb[1]], c in [pb[2], pb[3]]} of a triangle (Prim::pb): a
// triangle moves affinely, so a piece made at build time is still that set over its old parameter box -- a parallelogram whose
// four corners bound it, widened by a few ulps of the coordinates (the corners are rounded), within the triangle's own box.
RGK_HD Box piece_box(V3 v0, V3 v1, V3 v2, float b0, float b1, float c0, float c1) {
    Box b = tri_box(v0, v1, v2);
    for (int a = 0; a < 3; a++) {
        const float o = comp(v0, a), e1 = comp(v1, a) - o, e2 = comp(v2, a) - o;
        const float c00 = o + b0 * e1 + c0 * e2, c10 = o + b1 * e1 + c0 * e2, c01 = o + b0 * e1 + c1 * e2, c11 = o + b1 * e1 + c1 * e2;
        const float m = 4e-6f * (__builtin_fabsf(o) + __builtin_fabsf(e1) + __builtin_fabsf(e2));
        b.mn[a] = maxf(b.mn[a], minf(minf(c00, c10), minf(c01, c11)) - m);
        b.mx[a] = minf(b.mx[a], maxf(maxf(c00, c10), maxf(c01, c11)) + m);
    }
    return b;
}
RGK_HD bool whole_triangle(float b0, float b1, float c0, float c1) { return b0 == 0.f && b1 == 1.f && c0 == 0.f && c1 == 1.f; }
