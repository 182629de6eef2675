// Shading: k_shade (K3 / K4 / K6 / K7) and the pieces the shading kernels of both sub-paths use (k_shade here, k_shade_light and
// k_raygen_light in rgk_bdpt.h): the queue records, the path's sampler coordinates, the workgroup compaction and the sampling half
// of a path vertex.  The geometric half -- Vertex, surface_point(), clamp3 -- is in rgk_device.h: the feature pass (rgk_post.hip)
// and the walkers (rgk_trace.h) use it too.  At the end of the file: k_last_vertex, the last bounce of a unidirectional pass.
#pragma once
#include <hip/hip_runtime.h>
#include "rgk_device.h"
#include "rgk_kernels.h"
#include "rgk_ring.h"
#include "rgk_trace.h" // camera_ray_of_slot, slot_decode

#ifndef RGK_SKIP_DEAD_NEE
#define RGK_SKIP_DEAD_NEE 1
#endif
#ifndef RGK_CL_REC32
#define RGK_CL_REC32 1 // constant-light route: shadow rays queued as 32-byte records (0: the three-array records, for measuring the two parts apart)
#endif

// ------------------------------------------------------------------ queue records: what the shading kernels hand the walkers (rgk_trace.h)
//   ray queue       A = {o.xyz, d.x}     B = {d.y, d.z, w, slot}   w: the triangle the ray leaves (the walker skips it), all ones
//                                                                  for a light ray; the shading kernels read back o, d and slot
//   shadow queue    A = {from.xyz, d.x}  B = {d.y, d.z, far, id}   C = {radiance.rgb, near}   id: the slot, or the pixel of a splat
//   constant light  A = {d.xyz, far}     B = {radiance.rgb, slot}  (RGK_CL_REC32: every ray from sc.cl_pos with near = 20 eps)
// Value functions, one per 16-byte word: a record handed over as a struct or through references changes the kernels' code.
__device__ __forceinline__ float4 ray_rec_a(f3 o, f3 d) { return make_float4(o.x, o.y, o.z, d.x); }
__device__ __forceinline__ float4 ray_rec_b(f3 d, float w, uint32_t slot) { return make_float4(d.y, d.z, w, __uint_as_float(slot)); }
__device__ __forceinline__ f3 ray_rec_o(float4 a) { return mk3(a.x, a.y, a.z); }
__device__ __forceinline__ f3 ray_rec_d(float4 a, float4 b) { return mk3(a.w, b.x, b.y); }
__device__ __forceinline__ uint32_t ray_rec_slot(float4 b) { return __float_as_uint(b.w); }
__device__ __forceinline__ float4 shadow_rec_a(f3 from, f3 d) { return make_float4(from.x, from.y, from.z, d.x); }
__device__ __forceinline__ float4 shadow_rec_b(f3 d, float far, uint32_t id) { return make_float4(d.y, d.z, far, __uint_as_float(id)); }
__device__ __forceinline__ float4 shadow_rec_c(f3 rad, float near) { return make_float4(rad.x, rad.y, rad.z, near); }
__device__ __forceinline__ float4 cl_rec_a(f3 d, float far) { return make_float4(d.x, d.y, d.z, far); }
__device__ __forceinline__ float4 cl_rec_b(f3 rad, uint32_t slot) { return make_float4(rad.x, rad.y, rad.z, __uint_as_float(slot)); }

// Where a path reads its sampler: the pixel's seed, the sample's index and the first 2-D dimension behind the camera's own.
struct PathSampler { uint32_t seed, s, base2d; };
__device__ __forceinline__ PathSampler path_sampler(const PassParams& pp, const DevCamera& cam, uint32_t slot) {
    uint32_t srel, j; slot_decode(pp, slot, j, srel);
    PathSampler ps;
    ps.seed = pp.pix_seed[pp.j0 + j];
    ps.s = pp.s0 + srel;
    ps.base2d = (cam.lens_size != 0.0f) ? 2u : 1u;
    return ps;
}

// ------------------------------------------------------------------ workgroup compaction
// this lane's rank among the set lanes of a ballot
__device__ __forceinline__ uint32_t lane_rank(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// Workgroup-level append: returns this lane's position in the queue behind `counter` (valid only
// when flag).  Two barriers; every thread of the workgroup must call it the same number of times.
__device__ __forceinline__ uint32_t block_append(bool flag, uint32_t* counter, uint32_t* s_cnt, uint32_t* s_base) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) s_cnt[w] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int k = 0; k < RGK_LIGHT_BLOCK / 64; k++) { uint32_t a = s_cnt[k]; s_cnt[k] = t; t += a; }
        *s_base = t ? atomicAdd(counter, t) : 0u;
    }
    __syncthreads();
    const uint32_t p = *s_base + s_cnt[w] + lane_rank(m, lane);
    __syncthreads();
    return p;
}

// k_shade's four queues at once -- next rays, shadow rays, deferred vertices, connection records (BDPT): between the compaction's
// two barriers one thread turns the per-wave counts s_cnt[q][] into the waves' offsets and reserves each queue's range with one
// atomic, so that s_base[q] + s_cnt[q][w] is the place of wave w's first entry in queue q.
template <uint32_t BLK, bool BDPT>
__device__ __forceinline__ void block_reserve4(uint32_t (*s_cnt)[BLK / 64], uint32_t* s_base, uint32_t* counters, uint32_t bounce) {
    if (threadIdx.x == 0) {
        uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
        for (int k = 0; k < (int)(BLK / 64); k++) {
            uint32_t a = s_cnt[0][k], b = s_cnt[1][k], c = s_cnt[2][k];
            s_cnt[0][k] = t0; s_cnt[1][k] = t1; s_cnt[2][k] = t2;
            t0 += a; t1 += b; t2 += c;
            if (BDPT) { uint32_t e = s_cnt[3][k]; s_cnt[3][k] = t3; t3 += e; }
        }
        s_base[0] = t0 ? atomicAdd(&counters[RGK_CNT_QUEUE + bounce + 1], t0) : 0u;
        s_base[1] = t1 ? atomicAdd(&counters[RGK_CNT_SHADOW + bounce], t1) : 0u;
        s_base[2] = t2 ? atomicAdd(&counters[RGK_CNT_GENERIC + bounce], t2) : 0u;
        if (BDPT) s_base[3] = t3 ? atomicAdd(&counters[RGK_CNT_CONN + bounce], t3) : 0u;
    }
}

// The sampling half of a GeneratePath iteration (path_tracer.cpp:239-300), as k_shade_light calls it.  THERE ARE TWO COPIES: k_shade
// below has the same steps inline -- BxDF sample, leak rule, roulette, next ray -- around its NEE.  Value functions for the leak,
// the roulette coefficient and the next ray, called from both, change the code of all fourteen shading kernels
// (profiles/shade_pieces_device_code.txt), so neither copy has them.  A change to one copy belongs in the other.
struct Step {
    bool go;
    f3 cum, no, nd;
};
template <bool GENERIC>
__device__ __forceinline__ void path_step(const DevScene& sc, const SamplerTab& tb, const Vertex& v, const MatPrep& mp, uint32_t seed, uint32_t s,
                                 uint32_t dim2d, uint32_t n, uint32_t depth, float russian, f3 cum, uint32_t& c1, Step& st) {
    st.go = false; st.cum = cum; st.no = st.nd = mk3(0.f, 0.f, 0.f);
    if (!(n < depth)) return; // last vertex: nothing sampled here can be observed
    const quatf l2g = qinverse(v.g2l);
    float2 u = sample2d_t(tb, seed, s, dim2d);
    f3 dirL, weight; bool may_leak;
    mat_sample<GENERIC>(sc, (int)v.mat_id, v.mat, mp, v.VrL, v.uv, u, dirL, weight, may_leak);
    const bool inside = dirL.z < 0;
    const f3 dir = qrot(l2g, dirL);
    uint32_t n_eff = n;
    if (!(dot3(dir, v.faceN) * dot3(v.Vr, v.faceN) > 0) && !may_leak) n_eff += 10000u;
    const bool no_russian = (v.mat.flags & RGK_MAT_NO_RUSSIAN) != 0;
    const float rc = (!no_russian && russian > 0.0f && n_eff > 1u) ? 1.0f / russian : 1.0f;
    cum = cum * rc;
    cum = cum * weight;
    st.cum = cum;
    bool go = !(max3c(cum) < 0.001f);
    if (go && !no_russian && russian >= 0.0f) {
        float r = sample1d_t(tb, seed, s, c1);
        c1++;
        if (r > russian) go = false;
    }
    if (go && !(n_eff < depth)) go = false;
    if (go) {
        st.no = v.pos + v.faceN * sc.epsilon * 10.0f * (inside ? -1.0f : 1.0f);
        st.nd = norm3(norm3(dir));
    }
    st.go = go;
}

// A vertex's own addition to its slot's sum (sky, emission).  START: the fast launch of the first vertices, where the sum starts --
// the addition goes to the value the kernel writes once at the end; elsewhere the sum is read, added to and written back.
template <bool START>
__device__ __forceinline__ f3 slot_add(float4* tot, uint32_t slot, f3 tot0, f3 add) {
    if (START) return mk3(0.f + add.x, 0.f + add.y, 0.f + add.z);
    float4 t = tot[slot];
    t.x = t.x + add.x; t.y = t.y + add.y; t.z = t.z + add.z;
    tot[slot] = t;
    return tot0;
}

// An emitting vertex that is also lit: the oracle adds ONE term, A = clamp(NEE + emission) * contribution if the light is visible and
// B = clamp(emission) * contribution if not, to the sum `prev` of the vertices before.  Here B is added when the vertex is shaded and the
// shadow ray, if it gets through, adds the rest -- which is (prev + A) - (prev + B) in float32, not A - B: then
// (prev + B) + rest == prev + A to the bit (A >= B >= 0 channel by channel; above half of prev + A the difference is exact, below it
// its rounding error stays under half a unit of prev + A), where (prev + B) + (A - B) can end one bit off.
// Adds B to the slot's sum as slot_add does; `prev`, `now`: the sum before and behind the addition.
template <bool START>
__device__ __forceinline__ f3 slot_add_keep(float4* tot, uint32_t slot, f3 tot0, f3 add, f3& prev, f3& now) {
    if (START) { prev = mk3(0.f, 0.f, 0.f); now = mk3(0.f + add.x, 0.f + add.y, 0.f + add.z); return now; }
    float4 t = tot[slot];
    prev = mk3(t.x, t.y, t.z);
    t.x = t.x + add.x; t.y = t.y + add.y; t.z = t.z + add.z;
    tot[slot] = t;
    now = mk3(t.x, t.y, t.z);
    return tot0;
}
__device__ __forceinline__ f3 lit_emitter_rest(f3 prev, f3 now, f3 A) { return (prev + A) - now; }

// ------------------------------------------------------------------ K1: ray generation (camera_ray, camera_ray_of_slot: rgk_trace.h)
// (Unidirectional rounds have no ray-generation kernel: bounce 0 derives the camera ray from the slot number in the traversal
// kernel and again in the shading kernel, and the first vertex samples the path's light and starts its sum -- see
// k_trace_camera and k_shade<GENERIC, FIRST = true>.  The bidirectional kernels keep theirs, rgk_bdpt.h.)

// ------------------------------------------------------------------ K3+K4+K6+K7: shade

// FIRST = true: bounce 0.  Queue index == path slot, the ray is the slot's camera ray (not stored anywhere), the path state is
// implicit {1, 1, 1 | n = 0, 1-D counter = 1}, the path's ONE light is sampled here (TracePath: areal_sample, (lightdir_sample),
// GetRandomLight(Get2D, Get1D, areal_sample) -- path_tracer.cpp:315-322) and kept per slot for the later bounces of paths that
// go on, and the slot's radiance sum STARTS here (written, not read-modified: nothing zeroes it beforehand).
// BDPT = true: a camera-path vertex of a bidirectional round (reverse > 0).  The same vertex code; but where the slot's light
// sub-path has vertices to connect to (pp.lvmask) or the vertex emits, its total is clamp(NEE + connections + emission) -- the
// clamp spans all of them (path_tracer.cpp:422-496) -- so instead of its own shadow ray the vertex leaves a RECORD
// (pp.conn[c * batch + i], i = its queue index, listed in pp.connlist) for k_connect (rgk_bdpt.h), which evaluates the
// connections and queues the vertex for k_trace_shadow_jobs.  Most slots have no light vertex (a light far outside the
// geometry: its first ray must hit the scene at all), and those vertices are shaded exactly like a unidirectional one.
// CL = true: the constant-light route of a unidirectional round (rgk.h rgk_scene_info::const_light).  "The path's light" is the
// same {pointlights[0].pos, code 0} for every path -- the host has checked that the pick below can have no other outcome -- so
// it is neither picked (five sampler dimensions, the selection loop, sphere_uniform times size == 0) nor kept per slot nor
// looked up through a per-lane code: position, colour and intensity come from the kernel arguments (sc.cl_*, SGPRs), the DLight
// has the member values light_from_code would have filled in, and everything computed from it is computed as before.  The shadow
// ray leaves as {d.xyz, far}{radiance.rgb, slot}: its origin and near distance are the same for every ray (k_trace_shadow<CL>).
// Both launches of a pass, fast and GENERIC, take the same route: nobody writes pp.light on this one.
template <bool GENERIC, bool FIRST, bool BDPT = false, bool CL = false>
__global__ __launch_bounds__((FIRST ? RGK_SHADE_BLOCK : RGK_SHADE_BLOCK_LATER), RGK_SHADE_WAVES) void k_shade(const DevScene sc, const DevCamera cam, const PassParams pp, const uint32_t bounce,
                                                            const float4* __restrict__ rayA, const float4* __restrict__ rayB,
                                                            const float4* __restrict__ hit, float4* __restrict__ thr, float4* __restrict__ tot,
                                                            float4* __restrict__ nextA, float4* __restrict__ nextB, float4* __restrict__ shA,
                                                            float4* __restrict__ shB, float4* __restrict__ shC, uint32_t* __restrict__ counters) {
    // GENERIC = false: every vertex whose material takes the fast route (diffuse, LTC); the others (mirror, dielectric,
    // transparent, mix) are only LISTED here and shaded by the GENERIC = true launch that follows, which walks that
    // list with the full BxDF code.  Keeping the rare, big generic route out of this kernel takes its scratch from
    // 136 to 24 bytes per thread -- and the kernel is bound by the bytes it moves.
    const uint32_t count = counters[(GENERIC ? RGK_CNT_GENERIC : RGK_CNT_QUEUE) + bounce];
    const int lane = threadIdx.x & 63;
    const float eps = sc.epsilon;
    const SamplerTab tb = {pp.htab, pp.multisample};
    // workgroup size: 512 for the first vertices, 256 for the later ones -- their lanes diverge (0.59 of them busy), and with four
    // waves instead of eight behind each of the compaction's two barriers the launch is 5.6 % shorter (21.35 -> 20.15 ms; the first
    // vertices, whose waves run alike, lose 1.7 % that way and keep 512)
    constexpr uint32_t BLK = FIRST ? RGK_SHADE_BLOCK : RGK_SHADE_BLOCK_LATER;
    __shared__ uint32_t s_cnt[4][BLK / 64];
    __shared__ uint32_t s_base[4];
    lut_lds_fill(sc);
    // workgroup-uniform trip count (the compaction below synchronises the workgroup)
    for (uint32_t base = blockIdx.x * BLK; base < count; base += gridDim.x * BLK) {
        const bool valid = base + threadIdx.x < count;
        const uint32_t i = !valid ? 0u : (GENERIC ? pp.generic[base + threadIdx.x] : base + threadIdx.x);
        bool cont = false, shadow = false, defer = false, conn = false;
        float4 nA = make_float4(0, 0, 0, 0), nB = nA, sA = nA, sB = nA, sC = nA;
        if (valid) {
            const float4 h = hit[i];
            uint32_t slot;
            f3 o, d;
            if (FIRST) { slot = i; camera_ray_of_slot(cam, pp, slot, o, d); }
            else {
                const float4 a = rayA[i], b = rayB[i];
                slot = ray_rec_slot(b);
                o = ray_rec_o(a); d = ray_rec_d(a, b);
            }
            const float4 st = FIRST ? make_float4(1.f, 1.f, 1.f, __uint_as_float(1u << 16)) : thr[slot];
            const float4 li_slot = (FIRST || CL) ? make_float4(0.f, 0.f, 0.f, 0.f) : pp.light[slot]; // (asked for with the path state, not where it is first used: later vertices 21.75 -> 21.3 ms)
            f3 tot0 = mk3(0.f, 0.f, 0.f); // FIRST, fast launch: what this vertex adds to the (so far empty) sum of its slot
            float4 li_keep = make_float4(0.f, 0.f, 0.f, 0.f);
            f3 cum = mk3(st.x, st.y, st.z);
            uint32_t bits = __float_as_uint(st.w);
            uint32_t n = (bits & 0xffffu) + 1u; // n++ at loop top, reference path_tracer.cpp:123
            uint32_t c1 = bits >> 16;
            const int tri = __float_as_int(h.w);
            // (path_sampler() written out: through the function, in any of three forms, the two FIRST && CL kernels come out different)
            uint32_t srel, j; slot_decode(pp, slot, j, srel);
            const uint32_t seed = pp.pix_seed[pp.j0 + j];
            const uint32_t s = pp.s0 + srel;
            const uint32_t base2d = (cam.lens_size != 0.0f) ? 2u : 1u;
            const f3 Vr = -d;
            if (tri < 0) {
                // sky vertex: path_total += contribution * sky, reference path_tracer.cpp:137-146,409-415
                f3 sky = skybox(sc, Vr);
                f3 add = cum * sky;
                tot0 = slot_add<FIRST && !GENERIC>(tot, slot, tot0, add);
            } else {
                // (from here to VrL: the inline copy of surface_point(), rgk_device.h, around this kernel's `defer` test)
                // one 128-byte line per triangle: {nA,uvA.x}{nB,uvA.y}{nC,uvB.x}{tA,uvB.y}{tB,uvC.x}{tC,uvC.y}{mat}
                const uint32_t tsr = (uint32_t)tri * (uint32_t)sizeof(TriShade);
                const float4 g0 = gld_f4(sc.tri_shade, tsr), g1 = gld_f4(sc.tri_shade, tsr + 16u), g2 = gld_f4(sc.tri_shade, tsr + 32u);
                const uint32_t mat_id = gld_u32(sc.tri_shade, tsr + 96u);
                const DevMaterial mat = mat_load(sc, mat_id);
                defer = !GENERIC && !mat_is_fast(mat.kind);
                if (!defer) {
                const float al = h.y, be = h.z;
                const float ia = 1.0f - al - be, ib = al, ic = be; // Intersection::a,b,c scene_intersect.cpp:280-283
                f3 pos = o + h.x * d;
                f3 nA_ = mk3(g0.x, g0.y, g0.z), nB_ = mk3(g1.x, g1.y, g1.z), nC_ = mk3(g2.x, g2.y, g2.z);
                bool ok;
                f3 faceN = face_normal(ia, ib, ic, nA_, nB_, nC_, ok);
                if (ok) {
                    faceN = norm3(faceN);
                    // (asking for the whole 128-byte record at once, before the normal has been checked: measured, nothing -- the line is
                    // in L1 by now)
                    const float4 g3 = gld_f4(sc.tri_shade, tsr + 48u), g4 = gld_f4(sc.tri_shade, tsr + 64u), g5 = gld_f4(sc.tri_shade, tsr + 80u);
                    float2 uv = make_float2(0.f, 0.f);
                    if (sc.has_texcoords) {
                        uv.x = ia * g0.w + ib * g2.w + ic * g4.w;
                        uv.y = ia * g1.w + ib * g3.w + ic * g5.w;
                    }
                    const bool bumped = tex_kind(mat.t_bump) != RGK_TEXREF_NONE;
                    f3 lightN = faceN;
                    if (bumped) { // bump, path_tracer.cpp:204-231
                        float right, bottom;
                        tex_slopes(sc, mat.t_bump, uv, right, bottom);
                        f3 tangent = ia * mk3(g3.x, g3.y, g3.z) + ib * mk3(g4.x, g4.y, g4.z) + ic * mk3(g5.x, g5.y, g5.z);
                        if (!(tangent.x * tangent.x + tangent.y * tangent.y + tangent.z * tangent.z < 0.001f)) {
                            tangent = norm3(tangent);
                            f3 bitangent = norm3(cross3(faceN, tangent));
                            f3 tangent2 = cross3(bitangent, faceN);
                            lightN = norm3(faceN + (tangent2 * right + bitangent * bottom) * pp.bumpmap_scale);
                            if (lightN.x != lightN.x) lightN = faceN;
                        }
                    }
                    // SystemTransform(lightN, +Z), reference src/glm.hpp:21-24
                    const quatf g2l = rotation_between(lightN, mk3(0.f, 0.f, 1.f));
                    const f3 VrL = qrot(g2l, Vr);
                    // The vertex at n == depth is the path's last (while(n < depth__), :122): its sampled direction,
                    // transfer coefficient and roulette draw can never be observed, so they are not computed.
                    const bool last = !(n < pp.depth);
                    const bool no_russian = (mat.flags & RGK_MAT_NO_RUSSIAN) != 0;
                    // `ends`: nothing follows this vertex (it is the last by depth).  Then the sampled direction and its weight can never
                    // be observed and are not computed, and the material is needed for ONE thing, the BxDF value towards the path's
                    // light -- which for the kinds shaded here is exactly 0 when the light or the viewer is below the (bumped)
                    // surface's horizon (bxdf_value_fastkind).  Then neither texels nor tables are fetched: the vertex adds its
                    // emission, if any, and nothing else -- the same zero the long way round gives (0 * G needs G finite: the
                    // vertex is not AT the light).  (Drawing the roulette number first, so that a path it ends counts as ending
                    // here too, is exact as well -- the draw depends on nothing computed here -- but measured slower, 57.9 vs
                    // 55.9 ms of shading per round: the lanes that could stop early wait for their wave anyway.)
                    const bool ends = last;
                    float4 li; // the path's light {pos, code}: sampled by the first vertex, carried in pp.light after it
                    if (CL) li = make_float4(sc.cl_pos[0], sc.cl_pos[1], sc.cl_pos[2], __uint_as_float(0u));
                    else if (FIRST) {
                        f3 lpos;
                        const uint32_t lcode = light_code(sc, sample2d_t(tb, seed, s, base2d + 2u), sample1d_t(tb, seed, s, 0u), sample2d_t(tb, seed, s, base2d), lpos);
                        li = make_float4(lpos.x, lpos.y, lpos.z, __uint_as_float(lcode));
                    } else li = li_slot;
                    bool nee_dead = false;
                    if (RGK_SKIP_DEAD_NEE && ends && !GENERIC) {
                        const DLight L0 = CL ? light_constant(sc) : light_from_code(sc, mk3(li.x, li.y, li.z), __float_as_uint(li.w));
                        if (L0.type < 0) nee_dead = true;
                        else {
                            const f3 df = pos - L0.pos;
                            nee_dead = dot3(df, df) > 0.f && (qrot(g2l, norm3(L0.pos - pos)).z <= 0.f || VrL.z <= 0.f);
                        }
                    }
                    MatPrep mp;
                    if (!nee_dead) mat_prepare(sc, mat, uv, VrL, !ends, mp);
                    else { mp.fast = true; mp.lobe = false; mp.diffc = mp.colorc = mk3(0.f, 0.f, 0.f); }
                    const f3 contribution = cum; // excludes this vertex's own coefficients, :135
                    bool inside = false;
                    f3 dir = mk3(0.f, 0.f, 0.f);
                    uint32_t n_eff = n;
                    if (!ends) {
                        // BxDF sample, path_tracer.cpp:243-250 (from here to `go` below: the inline copy of path_step() above)
                        const quatf l2g = qinverse(g2l);
                        float2 u = sample2d_t(tb, seed, s, base2d + 3u + (n - 1u));
                        f3 dirL, weight; bool may_leak;
                        mat_sample<GENERIC>(sc, (int)mat_id, mat, mp, VrL, uv, u, dirL, weight, may_leak);
                        inside = dirL.z < 0;
                        dir = qrot(l2g, dirL);
                        if (!(dot3(dir, faceN) * dot3(Vr, faceN) > 0) && !may_leak) n_eff += 10000u; // leak, :252-260
                        const float rc = (!no_russian && pp.russian > 0.0f && n_eff > 1u) ? 1.0f / pp.russian : 1.0f;
                        cum = cum * rc;
                        cum = cum * weight;
                    }

                    // ---- phase 3 for this vertex: NEE to the path's light, :427-460,485-496
                    {
                        li_keep = li;
                        const DLight L = CL ? light_constant(sc) : light_from_code(sc, mk3(li.x, li.y, li.z), __float_as_uint(li.w));
                        f3 e_front = mk3(0.f, 0.f, 0.f);
                        if (dot3(faceN, Vr) > 0) e_front = mk3(mat.emission[0], mat.emission[1], mat.emission[2]);
                        const bool has_e = (e_front.x != 0.f) || (e_front.y != 0.f) || (e_front.z != 0.f);
                        // bidirectional: light vertices to connect to (bits 0..6), or an emitting vertex -> the record route
                        if (BDPT) conn = ((pp.lvmask[slot] & 0x7fu) != 0u) || has_e;
                        f3 e_prev = mk3(0.f, 0.f, 0.f), e_now = mk3(0.f, 0.f, 0.f); // the slot's sum before and behind the emission's addition
                        if (has_e && !conn) {
                            const f3 B = clamp3(mk3(0.f, 0.f, 0.f) + e_front, pp.clamp) * contribution;
                            tot0 = slot_add_keep<FIRST && !GENERIC>(tot, slot, tot0, B, e_prev, e_now);
                        }
                        f3 out = mk3(0.f, 0.f, 0.f); // NEE radiance before visibility, clamp and contribution
                        if (L.type >= 0 && !nee_dead) {
                            const f3 diff = pos - L.pos; // Ray(light.pos, p.pos, 20 eps), src/ray.hpp:15-22
                            const f3 sd = norm3(diff);
                            const float slen = len3(diff);
                            const f3 Vi = norm3(L.pos - pos);
                            const f3 f = mat_value<GENERIC>(sc, (int)mat_id, mat, mp, qrot(g2l, Vi), VrL, uv);
                            const float G = fabsf(dot3(lightN, Vi)) / dot3(diff, diff);
                            const float k = L.intensity * light_dir_factor(L, -Vi);
                            const f3 inc = L.color * mk3(k, k, k);
                            out = inc * (f * G);
                            if (!conn) {
                                f3 A = clamp3((mk3(0.f, 0.f, 0.f) + out) + e_front, pp.clamp) * contribution;
                                f3 rad = has_e ? lit_emitter_rest(e_prev, e_now, A) : A;
                                if (rad.x != 0.f || rad.y != 0.f || rad.z != 0.f) {
                                    shadow = true;
                                    if (CL && RGK_CL_REC32) {
                                        sA = cl_rec_a(sd, slen - eps * 20.0f);
                                        sB = cl_rec_b(rad, slot);
                                    } else {
                                        sA = shadow_rec_a(L.pos, sd);
                                        sB = shadow_rec_b(sd, slen - eps * 20.0f, slot);
                                        sC = shadow_rec_c(rad, 0.0f + eps * 20.0f);
                                    }
                                }
                            }
                        }
                        if (BDPT && conn) { // everything k_connect needs to evaluate this vertex's material towards a light vertex
                            const size_t bs = pp.batch;
                            pp.conn[i] = make_float4(pos.x, pos.y, pos.z, __uint_as_float(slot));
                            pp.conn[bs + i] = make_float4(lightN.x, lightN.y, lightN.z, __uint_as_float(mat_id));
                            pp.conn[2 * bs + i] = make_float4(g2l.x, g2l.y, g2l.z, g2l.w);
                            pp.conn[3 * bs + i] = make_float4(VrL.x, VrL.y, VrL.z, uv.x);
                            pp.conn[4 * bs + i] = make_float4(contribution.x, contribution.y, contribution.z, uv.y);
                            pp.conn[5 * bs + i] = make_float4(out.x, out.y, out.z, __uint_as_float(has_e ? 1u : 0u));
                        }
                    }
                    // ---- continuation, path_tracer.cpp:275-300
                    bool go = !ends && !(max3c(cum) < 0.001f);
                    if (go && !no_russian && pp.russian >= 0.0f) {
                        float r = sample1d_t(tb, seed, s, c1);
                        c1++;
                        if (r > pp.russian) go = false;
                    }
                    if (go && n_eff > pp.depth) go = false;
                    if (go && !(n_eff < pp.depth)) go = false; // while(n < depth__)
                    if (go) {
                        const float sgn = inside ? -1.0f : 1.0f;
                        f3 no = pos + faceN * eps * 10.0f * sgn;
                        f3 nd = norm3(norm3(dir)); // normalised by the caller and again by Ray's ctor
                        cont = true;
                        nA = ray_rec_a(no, nd);
                        nB = ray_rec_b(nd, __int_as_float(tri), slot);
                        thr[slot] = make_float4(cum.x, cum.y, cum.z, __uint_as_float((n & 0xffffu) | (c1 << 16)));
                    }
                    // the path's light: later vertices read it (and k_connect, for the NEE ray of a vertex on the record route)
                    if (FIRST && !CL && (go || conn)) pp.light[slot] = li_keep;
                }
                } // !defer
            }
            if (FIRST && !GENERIC) tot[slot] = make_float4(tot0.x, tot0.y, tot0.z, 0.f); // every slot of the pass passes here exactly once
        }
        // ---- K7: compaction into the next queues.
        {
            // Wave ballot + prefix popcount inside the wave, the waves of the workgroup add up through LDS, and ONE
            // atomic per workgroup and queue reserves the range.
            const unsigned long long m = __ballot(cont), ms = __ballot(shadow), md = __ballot(defer), mc = BDPT ? __ballot(conn) : 0ull;
            const int w = threadIdx.x >> 6;
            if (lane == 0) { s_cnt[0][w] = __popcll(m); s_cnt[1][w] = __popcll(ms); s_cnt[2][w] = __popcll(md); if (BDPT) s_cnt[3][w] = __popcll(mc); }
            __syncthreads();
            block_reserve4<BLK, BDPT>(s_cnt, s_base, counters, bounce);
            __syncthreads();
            if (!GENERIC && defer) pp.generic[s_base[2] + s_cnt[2][w] + lane_rank(md, lane)] = i;
            if (BDPT && conn) pp.connlist[s_base[3] + s_cnt[3][w] + lane_rank(mc, lane)] = i;
            if (cont) {
                uint32_t p = s_base[0] + s_cnt[0][w] + lane_rank(m, lane);
                nextA[p] = nA; nextB[p] = nB;
            }
            if (shadow) {
                uint32_t p = s_base[1] + s_cnt[1][w] + lane_rank(ms, lane);
                shA[p] = sA; shB[p] = sB;
                if (!(CL && RGK_CL_REC32)) shC[p] = sC;
            }
            __syncthreads(); // s_cnt / s_base are rewritten by the next iteration
        }
    }
}

// ------------------------------------------------------------------ the last bounce of a unidirectional pass: k_last_vertex
// At bounce b the queue holds the vertices with n == b + 1, so at b + 1 == depth EVERY vertex of the launch is its path's last
// (k_shade's `ends`, there a per-lane test): nothing is sampled, no ray follows, thr[slot] is read and never written.  What is
// left of k_shade<false, false, false, CL> is two halves, and they are the two functions below -- k_shade's expressions in
// k_shade's order (-ffp-contract=off: the same operations on the same operands are the same bits):
//   last_vertex_geometry   hit, ray and path state -> a sky vertex's addition, or the vertex from its triangle record to the
//                          `nee_dead` test, the deferral test (the GENERIC launch that follows is k_shade<true, false, false, CL>
//                          on the list this kernel fills) and the emission's addition; a LIVE vertex -- one whose light is above
//                          both horizons -- leaves a LastVertex;
//   last_vertex_nee        LastVertex -> texels, LTC entry, BxDF value, G, the clamp, a lit emitter's addition (slot_add_keep): the
//                          shadow record, if any.
// Bounce rays scatter, so the 64 vertices of a wave are unrelated and under half of them are live (Sponza: 45 % live, 48 % dead,
// 7 % sky): run back to back per lane -- as k_shade does, and as a one-phase build of this kernel did, which measured no faster than
// k_shade -- the second half has most lanes of every wave masked off.  k_last_vertex runs the halves as two phases of
// the workgroup with a record ring in LDS between them (rgk_ring.h): phase A, a thread per queue entry, appends the live vertices;
// phase B, a thread per record, runs on full waves whenever a workgroup's worth is pending, and once behind the loop.
struct LastVertex {
    f3 pos, lightN, VrL, contribution;
    quatf g2l;
    float2 uv;
    uint32_t slot, matf; // matf: material id | the vertex faces the viewer (bit 31: e_front is the material's emission)
    float4 li;           // the path's light {pos, code} (CL: not read, the launch constant)
};
#define RGK_LV_FRONT 0x80000000u
template <bool CL>
__device__ __forceinline__ DLight last_vertex_light(const DevScene& sc, float4 li) {
    return CL ? light_constant(sc) : light_from_code(sc, mk3(li.x, li.y, li.z), __float_as_uint(li.w));
}
// returns: live.  defer: the vertex goes on the GENERIC list.
template <bool CL>
__device__ __forceinline__ bool last_vertex_geometry(const DevScene& sc, const PassParams& pp, uint32_t i, const float4* __restrict__ rayA, const float4* __restrict__ rayB,
                                                     const float4* __restrict__ hit, const float4* __restrict__ thr, float4* __restrict__ tot, bool& defer, LastVertex& v) {
    const float4 h = hit[i];
    const float4 a = rayA[i], b = rayB[i];
    const uint32_t slot = ray_rec_slot(b);
    const f3 o = ray_rec_o(a), d = ray_rec_d(a, b);
    const float4 st = thr[slot];
    const float4 li = CL ? make_float4(sc.cl_pos[0], sc.cl_pos[1], sc.cl_pos[2], __uint_as_float(0u)) : pp.light[slot];
    const f3 tot0 = mk3(0.f, 0.f, 0.f);
    const f3 cum = mk3(st.x, st.y, st.z);
    const int tri = __float_as_int(h.w);
    const f3 Vr = -d;
    defer = false;
    if (tri < 0) {
        f3 sky = skybox(sc, Vr);
        f3 add = cum * sky;
        slot_add<false>(tot, slot, tot0, add);
        return false;
    }
    const uint32_t tsr = (uint32_t)tri * (uint32_t)sizeof(TriShade);
    const float4 g0 = gld_f4(sc.tri_shade, tsr), g1 = gld_f4(sc.tri_shade, tsr + 16u), g2 = gld_f4(sc.tri_shade, tsr + 32u);
    const uint32_t mat_id = gld_u32(sc.tri_shade, tsr + 96u);
    const DevMaterial mat = mat_load(sc, mat_id);
    defer = !mat_is_fast(mat.kind);
    if (defer) return false;
    const float al = h.y, be = h.z;
    const float ia = 1.0f - al - be, ib = al, ic = be;
    f3 pos = o + h.x * d;
    f3 nA_ = mk3(g0.x, g0.y, g0.z), nB_ = mk3(g1.x, g1.y, g1.z), nC_ = mk3(g2.x, g2.y, g2.z);
    bool ok;
    f3 faceN = face_normal(ia, ib, ic, nA_, nB_, nC_, ok);
    if (!ok) return false;
    faceN = norm3(faceN);
    const float4 g3 = gld_f4(sc.tri_shade, tsr + 48u), g4 = gld_f4(sc.tri_shade, tsr + 64u), g5 = gld_f4(sc.tri_shade, tsr + 80u);
    float2 uv = make_float2(0.f, 0.f);
    if (sc.has_texcoords) {
        uv.x = ia * g0.w + ib * g2.w + ic * g4.w;
        uv.y = ia * g1.w + ib * g3.w + ic * g5.w;
    }
    const bool bumped = tex_kind(mat.t_bump) != RGK_TEXREF_NONE;
    f3 lightN = faceN;
    if (bumped) {
        float right, bottom;
        tex_slopes(sc, mat.t_bump, uv, right, bottom);
        f3 tangent = ia * mk3(g3.x, g3.y, g3.z) + ib * mk3(g4.x, g4.y, g4.z) + ic * mk3(g5.x, g5.y, g5.z);
        if (!(tangent.x * tangent.x + tangent.y * tangent.y + tangent.z * tangent.z < 0.001f)) {
            tangent = norm3(tangent);
            f3 bitangent = norm3(cross3(faceN, tangent));
            f3 tangent2 = cross3(bitangent, faceN);
            lightN = norm3(faceN + (tangent2 * right + bitangent * bottom) * pp.bumpmap_scale);
            if (lightN.x != lightN.x) lightN = faceN;
        }
    }
    const quatf g2l = rotation_between(lightN, mk3(0.f, 0.f, 1.f));
    const f3 VrL = qrot(g2l, Vr);
    const DLight L = last_vertex_light<CL>(sc, li);
    bool nee_dead = false;
    if (RGK_SKIP_DEAD_NEE) {
        if (L.type < 0) nee_dead = true;
        else {
            const f3 df = pos - L.pos;
            nee_dead = dot3(df, df) > 0.f && (qrot(g2l, norm3(L.pos - pos)).z <= 0.f || VrL.z <= 0.f);
        }
    }
    const f3 contribution = cum;
    const bool front = dot3(faceN, Vr) > 0;
    f3 e_front = mk3(0.f, 0.f, 0.f);
    if (front) e_front = mk3(mat.emission[0], mat.emission[1], mat.emission[2]);
    const bool has_e = (e_front.x != 0.f) || (e_front.y != 0.f) || (e_front.z != 0.f);
    const bool live = L.type >= 0 && !nee_dead;
    if (has_e && !live) { // (a live vertex adds its emission in last_vertex_nee, which needs the sum before it: slot_add_keep)
        f3 B = clamp3(mk3(0.f, 0.f, 0.f) + e_front, pp.clamp) * contribution;
        slot_add<false>(tot, slot, tot0, B);
    }
    v.pos = pos; v.lightN = lightN; v.VrL = VrL; v.contribution = contribution; v.g2l = g2l; v.uv = uv;
    v.slot = slot; v.matf = mat_id | (front ? RGK_LV_FRONT : 0u); v.li = li;
    return live;
}
// returns: the vertex leaves a shadow ray, sA / sB (/ sC) its record
template <bool CL>
__device__ __forceinline__ bool last_vertex_nee(const DevScene& sc, const PassParams& pp, const LastVertex& v, float4* __restrict__ tot, float4& sA, float4& sB, float4& sC) {
    const float eps = sc.epsilon;
    const uint32_t mat_id = v.matf & ~RGK_LV_FRONT;
    const DevMaterial mat = mat_load(sc, mat_id);
    const DLight L = last_vertex_light<CL>(sc, v.li);
    MatPrep mp;
    mat_prepare(sc, mat, v.uv, v.VrL, false, mp);
    const f3 pos = v.pos, contribution = v.contribution;
    f3 e_front = mk3(0.f, 0.f, 0.f);
    if (v.matf & RGK_LV_FRONT) e_front = mk3(mat.emission[0], mat.emission[1], mat.emission[2]);
    const bool has_e = (e_front.x != 0.f) || (e_front.y != 0.f) || (e_front.z != 0.f);
    f3 e_prev = mk3(0.f, 0.f, 0.f), e_now = mk3(0.f, 0.f, 0.f);
    if (has_e) slot_add_keep<false>(tot, v.slot, mk3(0.f, 0.f, 0.f), clamp3(mk3(0.f, 0.f, 0.f) + e_front, pp.clamp) * contribution, e_prev, e_now);
    const f3 diff = pos - L.pos;
    const f3 sd = norm3(diff);
    const float slen = len3(diff);
    const f3 Vi = norm3(L.pos - pos);
    const f3 f = mat_value<false>(sc, (int)mat_id, mat, mp, qrot(v.g2l, Vi), v.VrL, v.uv);
    const float G = fabsf(dot3(v.lightN, Vi)) / dot3(diff, diff);
    const float k = L.intensity * light_dir_factor(L, -Vi);
    const f3 inc = L.color * mk3(k, k, k);
    const f3 out = inc * (f * G);
    f3 A = clamp3((mk3(0.f, 0.f, 0.f) + out) + e_front, pp.clamp) * contribution;
    f3 rad = has_e ? lit_emitter_rest(e_prev, e_now, A) : A;
    if (!(rad.x != 0.f || rad.y != 0.f || rad.z != 0.f)) return false;
    if (CL && RGK_CL_REC32) {
        sA = cl_rec_a(sd, slen - eps * 20.0f);
        sB = cl_rec_b(rad, v.slot);
    } else {
        sA = shadow_rec_a(L.pos, sd);
        sB = shadow_rec_b(sd, slen - eps * 20.0f, v.slot);
        sC = shadow_rec_c(rad, 0.0f + eps * 20.0f);
    }
    return true;
}

// A LastVertex in the ring, SoA by field: ring[field * capacity + position], 20 dwords.  The path's light is not among them: off
// the constant-light route phase B reads pp.light[slot] again.  (With the light's four dwords the ring is 48 KB, two workgroups per
// CU instead of three, and the launch measured SLOWER than k_shade on the headline with the route switched off: 21.9 against 20.5 ms.)
constexpr uint32_t RGK_LV_FIELDS = 20;
__device__ __forceinline__ void last_vertex_put(float* ring, uint32_t cap, uint32_t p, const LastVertex& v) {
    const float f[RGK_LV_FIELDS] = {v.pos.x, v.pos.y, v.pos.z, v.lightN.x, v.lightN.y, v.lightN.z, v.VrL.x, v.VrL.y, v.VrL.z,
                                    v.contribution.x, v.contribution.y, v.contribution.z, v.g2l.x, v.g2l.y, v.g2l.z, v.g2l.w, v.uv.x, v.uv.y,
                                    __uint_as_float(v.slot), __uint_as_float(v.matf)};
#pragma unroll
    for (uint32_t k = 0; k < RGK_LV_FIELDS; k++) ring[k * cap + p] = f[k];
}
template <bool CL>
__device__ __forceinline__ void last_vertex_get(const PassParams& pp, const float* ring, uint32_t cap, uint32_t p, LastVertex& v) {
    float f[RGK_LV_FIELDS];
#pragma unroll
    for (uint32_t k = 0; k < RGK_LV_FIELDS; k++) f[k] = ring[k * cap + p];
    v.pos = mk3(f[0], f[1], f[2]); v.lightN = mk3(f[3], f[4], f[5]); v.VrL = mk3(f[6], f[7], f[8]);
    v.contribution = mk3(f[9], f[10], f[11]);
    v.g2l.x = f[12]; v.g2l.y = f[13]; v.g2l.z = f[14]; v.g2l.w = f[15];
    v.uv = make_float2(f[16], f[17]);
    v.slot = __float_as_uint(f[18]); v.matf = __float_as_uint(f[19]);
    v.li = CL ? make_float4(0.f, 0.f, 0.f, 0.f) : pp.light[v.slot];
}

// Three waves per SIMD: the ring (40 KB) beside the 8 KB of tables leaves room for three workgroups per CU.  (shading
// at 3 and at 4 waves per SIMD measured equal.)
template <bool CL>
__global__ __launch_bounds__(RGK_SHADE_BLOCK_LATER, 3) void k_last_vertex(const DevScene sc, const PassParams pp, const uint32_t bounce,
                                                            const float4* __restrict__ rayA, const float4* __restrict__ rayB,
                                                            const float4* __restrict__ hit, const float4* __restrict__ thr, float4* __restrict__ tot,
                                                            float4* __restrict__ shA, float4* __restrict__ shB, float4* __restrict__ shC,
                                                            uint32_t* __restrict__ counters) {
    constexpr uint32_t BLK = RGK_SHADE_BLOCK_LATER, NW = BLK / 64, CAP = rgk_ring_capacity(BLK);
    static_assert((BLK & (BLK - 1)) == 0, "the ring wraps with a mask");
    const uint32_t count = counters[RGK_CNT_QUEUE + bounce];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // per-wave counts of an append, in two sets that alternate (parity): a set is rewritten two appends later, behind the next
    // append's barrier, which every thread reaches only after it has read this one
    __shared__ uint32_t s_live[2][NW], s_defer[2][NW], s_shadow[2][NW];
    __shared__ uint32_t s_gbase[2], s_sbase[2];
    __shared__ float s_ring[RGK_LV_FIELDS * CAP];
    lut_lds_fill(sc);
    uint32_t head = 0, pending = 0, par = 0, parB = 0; // workgroup-uniform: every thread derives them from the same counts
    // workgroup-uniform trip count, and one more trip behind the queue's end (`final`), which only takes what is left in the ring
    for (uint32_t base = blockIdx.x * BLK;; base += gridDim.x * BLK) {
        const bool final = !(base < count);
        if (!final) {
            // ---- phase A: a thread per queue entry
            const bool valid = base + threadIdx.x < count;
            const uint32_t i = valid ? base + threadIdx.x : 0u;
            bool defer = false, live = false;
            LastVertex v;
            if (valid) live = last_vertex_geometry<CL>(sc, pp, i, rayA, rayB, hit, thr, tot, defer, v);
            // append: deferred vertices to the GENERIC list (one atomic per workgroup), live ones to the ring
            const unsigned long long ml = __ballot(live), md = __ballot(defer);
            if (lane == 0) { s_live[par][w] = __popcll(ml); s_defer[par][w] = __popcll(md); }
            __syncthreads();
            uint32_t lbefore = 0, ltotal = 0, dbefore = 0, dtotal = 0;
#pragma unroll
            for (uint32_t k = 0; k < NW; k++) {
                const uint32_t c = s_defer[par][k], l = s_live[par][k];
                if (k < (uint32_t)w) { dbefore += c; lbefore += l; }
                dtotal += c; ltotal += l;
            }
            if (dtotal) { // (workgroup-uniform)
                if (threadIdx.x == 0) s_gbase[par] = atomicAdd(&counters[RGK_CNT_GENERIC + bounce], dtotal);
                __syncthreads();
                if (defer) pp.generic[s_gbase[par] + dbefore + lane_rank(md, lane)] = i;
            }
            par ^= 1u;
            if (live) last_vertex_put(s_ring, CAP, rgk_ring_append_at(head, pending, lbefore + lane_rank(ml, lane), BLK), v);
            pending += ltotal;
        }
        // ---- phase B: a thread per record, for a workgroup's worth of them (behind the queue's end: for what is left)
        const uint32_t n = rgk_ring_take(pending, BLK, final);
        if (n) { // (workgroup-uniform)
            __syncthreads(); // the records are written
            float4 sA = make_float4(0, 0, 0, 0), sB = sA, sC = sA;
            bool shadow = false;
            if (threadIdx.x < n) {
                LastVertex v;
                last_vertex_get<CL>(pp, s_ring, CAP, rgk_ring_read_at(head, threadIdx.x, BLK), v);
                shadow = last_vertex_nee<CL>(sc, pp, v, tot, sA, sB, sC);
            }
            // the workgroup's range of the shadow queue: one atomic
            const unsigned long long ms = __ballot(shadow);
            if (lane == 0) s_shadow[parB][w] = __popcll(ms);
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (uint32_t k = 0; k < NW; k++) { const uint32_t c = s_shadow[parB][k]; if (k < (uint32_t)w) before += c; total += c; }
            if (total) { // (workgroup-uniform)
                if (threadIdx.x == 0) s_sbase[parB] = atomicAdd(&counters[RGK_CNT_SHADOW + bounce], total);
                __syncthreads();
                if (shadow) {
                    const uint32_t p = s_sbase[parB] + before + lane_rank(ms, lane);
                    shA[p] = sA; shB[p] = sB;
                    if (!(CL && RGK_CL_REC32)) shC[p] = sC;
                }
            }
            parB ^= 1u;
            head = rgk_ring_wrap(head + n, BLK); pending -= n;
        }
        if (final) break;
    }
}
