// The camera sub-path's shading kernels, k_shade and k_last_vertex (rgk_shade.h), in a translation unit of their own: it is built
// with -fno-slp-vectorize (rgk_amd/build.py SOURCE_FLAGS), the walkers and everything else in rgk_kernels.hip are not.
//
// Why: under plain -O3 the SLP vectoriser pairs independent fp32 multiplies and adds into v_pk_mul_f32 / v_pk_add_f32.  On gfx950 a
// packed fp32 instruction holds the non-fp32 ("slow") VALU pipe, the most loaded resource of these kernels, for about as long as
// the two plain instructions it replaces hold the issue port, which is not their limit; and the aligned register pairs it needs
// cost moves and registers (profiles/shade_codegen_static.txt).  The operations are the same IEEE operations
// on the same operands either way.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "rgk_device.h"
#include "rgk_kernels.h"
#include "rgk_shade.h" // K3 / K4 / K6 / K7

static void launch_last_vertex(hipStream_t st, const DevScene& sc, const PassParams& pp, uint32_t bounce, const float4* rayA, const float4* rayB, const float4* hit,
                               const float4* thr, float4* tot, float4* shA, float4* shB, float4* shC, uint32_t* counters, uint32_t bound, bool const_light) {
    const int grid = rgk_last_vertex_grid(bound);
    if (const_light) k_last_vertex<true><<<grid, RGK_SHADE_BLOCK_LATER, RGK_LDS_SHADE_BYTES, st>>>(sc, pp, bounce, rayA, rayB, hit, thr, tot, shA, shB, shC, counters);
    else k_last_vertex<false><<<grid, RGK_SHADE_BLOCK_LATER, RGK_LDS_SHADE_BYTES, st>>>(sc, pp, bounce, rayA, rayB, hit, thr, tot, shA, shB, shC, counters);
}

void rgk_launch_shade(hipStream_t st, const DevScene& sc, const DevCamera& cam, const PassParams& pp, uint32_t bounce, const float4* rayA,
                      const float4* rayB, const float4* hit, float4* thr, float4* tot, float4* nextA, float4* nextB, float4* shA,
                      float4* shB, float4* shC, uint32_t* counters, uint32_t bound, bool bdpt, bool const_light, bool last_vertex) {
    const RgkGridPair g = rgk_shade_grids(bounce, bound);
    // every vertex of the launch is its path's last: the fast launch is k_last_vertex, the GENERIC one k_shade on the list it fills
    const bool lv = last_vertex && rgk_last_bounce(bounce, pp.depth, bdpt);
    // the second launch shades the vertices the first one listed (materials on the generic BxDF route); it returns at once when there are none
    auto pair = [&](auto first, auto bd, auto cl) {
        constexpr bool FIRST = decltype(first)::value, BDPT = decltype(bd)::value, CL = decltype(cl)::value;
        if (!lv) k_shade<false, FIRST, BDPT, CL><<<g.fast, g.block, RGK_LDS_SHADE_BYTES, st>>>(sc, cam, pp, bounce, rayA, rayB, hit, thr, tot, nextA, nextB, shA, shB, shC, counters);
        else launch_last_vertex(st, sc, pp, bounce, rayA, rayB, hit, thr, tot, shA, shB, shC, counters, bound, CL);
        k_shade<true, FIRST, BDPT, CL><<<g.generic, g.block, RGK_LDS_SHADE_BYTES, st>>>(sc, cam, pp, bounce, rayA, rayB, hit, thr, tot, nextA, nextB, shA, shB, shC, counters);
    };
    constexpr std::true_type T{}; constexpr std::false_type F{};
    switch ((bounce == 0 ? 4 : 0) | (bdpt ? 2 : (const_light ? 1 : 0))) { // (FIRST, BDPT, CL): a bidirectional round never takes the constant-light route
    case 4 | 2: pair(T, T, F); break;
    case 2: pair(F, T, F); break;
    case 4 | 1: pair(T, F, T); break;
    case 1: pair(F, F, T); break;
    case 4: pair(T, F, F); break;
    default: pair(F, F, F); break;
    }
}
