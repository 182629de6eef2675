// Scene commit, the part that needs no device: everything rgk_scene_create computes on the host before it uploads
// (rgk_commit.cpp).  Plain C++17 over std::vector -- no call into the HIP runtime, no stream, no device buffer -- so the
// unit builds with any host compiler and runs under sanitizers (tests/cpp/commit_main.cpp links it alone).
//
//   * the OUTPUTS of Scene::Commit the hot path reads (reference src/scene.cpp:294-400): triangle planes, areal-light
//     tables sorted by area, light powers, epsilon = 1e-5 * bbox diagonal;
//   * the host accelerator: binned-SAH BVH2 over pre-split references, optimised by reinsertion, collapsed to a
//     quantised 4-wide BVH with one 64-byte line per node -- the reference's kd-tree construction (scene.cpp:431-657)
//     is out of scope, only its nearest-hit semantics are kept;
//   * texture palettes and texel pools, materials, lights, the Halton and LTC tables;
//   * the build switches of the environment (read_build_options) and rgk_last_error.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rgk.h"
#include "device_types.h"
#include "rgk_tree.h" // V3, Box, leaf codes, the quantiser, tri_isect_record: shared with the device builder

// Sets rgk_last_error (per thread) and returns `code`.  Every translation unit reports through this one:
// the others through rgk_internal_fail, its extern "C" form.
int fail(int code, const char* fmt, ...);

// ------------------------------------------------------------------ build switches
// The build-time switches of the environment (nothing here changes a result).  Read ONCE, by read_build_options at the
// top of rgk_scene_create; the builders take this struct or plain values.  -1 in the three RGK_LBVH_* fields: unset (the
// device build's rule "clustering on and rotate unset -> 0 passes" needs "unset" as a value of its own).
struct BuildOptions {
    float split = 0.1f;         // RGK_BVH_SPLIT: longest box side, as a fraction of the scene diagonal, above which a triangle is pre-split
                                // (swept on the Sponza proxy: 0.08..0.15 best, -7 % node visits; finer splits deepen the tree); <= 0: off
    int max_leaf = 4;           // RGK_BVH_MAXLEAF: references per leaf of the host build, 1..16 (the leaf encoding allows up to 16)
    float c_isect = 1.0f;       // RGK_BVH_CISECT: SAH cost of one triangle test in node steps (swept on MI355X: 1.0 best)
    int opt_rounds = 8;         // RGK_BVH_OPT: reinsertion rounds (0 = off)
    // leaves of the device build: at most 2 references (Morton-adjacent triangles make loose leaves: with 4, a ray tests twice the
    // triangles the host tree makes it test -- measured with 1 / 2 / 3 / 4 on the 1.05 M-triangle scene, closest-hit + shadow ms of
    // a round: 7.69 / 7.48 / 7.59 / 8.10, host SAH 7.36: tools/gpu_lbvh_rotate_sweep.py)
    int max_leaf_dev = 2;       // RGK_BVH_MAXLEAF_DEV, 1..16
    bool stack_ovf = true;      // RGK_STACK_OVF=0: the whole traversal stack in LDS, where 32 entries are enough
    int stack_lds = 16;         // RGK_STACK_LDS: 16 or 32 entries per lane in LDS
    uint32_t walk_q = 3;        // RGK_WALK_Q: traversal scheduling knob (rgk_trace.h)
    int lbvh_rotate = -1;       // RGK_LBVH_ROTATE: passes of the rotation step, 0..32; 0: the plain LBVH (for comparisons)
    int lbvh_ploc = -1;         // RGK_LBVH_PLOC: clustering radius, 0..256; 0: the Karras hierarchy
    int lbvh_morton_bits = -1;  // RGK_LBVH_MORTON_BITS: at most this many key bits per axis, >= 1 (experiments: 10 = round 2's keys)
};
BuildOptions read_build_options();

// ------------------------------------------------------------------ descriptor checks
int validate_desc(const rgk_scene_desc* d);
void debug_desc(const rgk_scene_desc* d); // RGK_DEBUG_DESC=1

// ------------------------------------------------------------------ bounds, records, references
// Commit's scalars (scene.cpp:364-395): the box of every referenced vertex and eps = 1e-5 * its diagonal.  The one place
// that computes them: rgk_scene_create and rgk_scene_refit both call it.
int commit_bounds(const float* vertices, const uint32_t* tri_indices, uint32_t n_triangles, float mn[3], float mx[3], float* eps);

struct Prim {
    float bmin[3], bmax[3], c[3];
    uint32_t tri;
    uint32_t ref;  // this reference's number (prims are shuffled by the builders; the leaf order lists these)
    float pb[4];   // the piece of the triangle this reference stands for, as a box in the triangle's own coordinates: P = v0 + b (v1 - v0) + c (v2 - v0)
                   // with b in [pb[0], pb[1]], c in [pb[2], pb[3]] -- (0, 1, 0, 1): the whole triangle.  A moved triangle maps its pieces
                   // affinely, so rgk_scene_refit re-boxes a reference from these four numbers instead of from the whole triangle
};

// The pre-split threshold of RefSplitter: a box side longer than this splits the triangle (0: no pre-splitting).
inline float split_threshold(const BuildOptions& o, float eps) { return o.split > 0.f ? o.split * (eps * 1e5f) : 0.f; } // eps = 1e-5 * diagonal

// Planes + intersection records (primitives.cpp:24-36, 75-166), one per triangle, and the build's references: one or more
// per triangle with a finite plane (a NaN plane can never be hit, primitives.cpp:90), at most 2x the triangles.
void commit_triangles(const float* vertices, const uint32_t* tri_indices, uint32_t n_triangles, float split_lmax, std::vector<TriIsect>& recs,
                      std::vector<Prim>& prims);

// ------------------------------------------------------------------ host accelerator
struct HostAccel {
    std::vector<QNode> qnodes;       // node 0 is the root
    std::vector<TriIsect> leaf_recs; // the records in leaf order, one per reference
    std::vector<float4> leaf_pb;     // per leaf reference: its piece of the triangle in the triangle's own coordinates (Prim::pb), for rgk_scene_refit
    uint32_t max_depth = 0, max_stack = 0;
};
// Binned SAH build over `prims` (shuffled by it), reinsertion, collapse to the quantised BVH4.  `pad`: the scene's epsilon.
int build_host_accel(std::vector<Prim>& prims, const std::vector<TriIsect>& recs, float pad, const BuildOptions& opt, HostAccel& out);

// ------------------------------------------------------------------ shading tables
std::vector<TriShade> build_tri_shade(const rgk_scene_desc* d);

struct Palette { std::vector<uint32_t> vals; bool fixed; uint32_t lut_off; }; // sorted bit patterns; fixed: a caller-supplied table
struct TexturePools {
    std::vector<float4> texels;    // float textures: RGBA float, A unused
    std::vector<uint32_t> texels8; // byte textures: one dword per texel, in tiles of 8 x 4
    std::vector<float> luts;       // byte -> float tables, 256 floats each
    std::vector<TexRef> refs;      // one per descriptor texture
    uint32_t n_float = 0, n_palettized = 0; // float textures of the descriptor; those of them stored as bytes + table
};
// Which textures become bytes + a table, and which table: fills pools.luts and, per texture, its palette (-1: none).
void assign_palettes(const rgk_scene_desc* d, std::vector<Palette>& palettes, std::vector<int>& tex_palette, TexturePools& pools);
// The texels into their pools and a TexRef per texture.
int pack_texels(const rgk_scene_desc* d, const std::vector<Palette>& palettes, const std::vector<int>& tex_palette, TexturePools& pools);
// The TexRef of texture `id`; id < 0: RGK_TEXREF_NONE.
TexRef tex_ref(const std::vector<TexRef>& refs, int32_t id);

std::vector<DevMaterial> build_materials(const rgk_scene_desc* d, const std::vector<TexRef>& refs);
std::vector<DevPointLight> build_point_lights(const rgk_scene_desc* d, float& total_power);
// Scene::Commit's areal-light tables (src/scene.cpp:323-344): per emissive object its triangles sorted by area (descending), the
// total area, power = area * (r + g + b).  Used by rgk_scene_create and, for moved vertices, by rgk_scene_refit.
void build_areal_tables(const float* vertices, const float* normals, const uint32_t* tri_indices, const uint32_t* tri_material, const rgk_material* materials,
                        uint32_t n_areal, const uint32_t* areal_offsets, const uint32_t* areal_tris, std::vector<DevArealLight>& als,
                        std::vector<DevArealTri>& ats, float& total_areal);
void build_halton(std::vector<DevHaltonDim>& dims, std::vector<uint16_t>& perm);
// Both LTC tables in one buffer, {m0,m2,m4,m6}{amp,0,0,0} per entry (two 16-byte loads): GGX, then Beckmann (a null table stays zero).
std::vector<float4> build_ltc_table(const float* ltc_ggx, const float* ltc_beckmann);
uint32_t const_light_eligible(const DevScene& ds, const DevPointLight* pls);

// Everything shading reads, in the order rgk_scene_create uploads it.
struct ShadingTables {
    std::vector<TriShade> tri_shade;
    TexturePools tex;
    std::vector<DevMaterial> materials;
    std::vector<DevPointLight> pointlights;
    std::vector<DevArealLight> areal;
    std::vector<DevArealTri> areal_tris;
    float total_point_power = 0.f, total_areal_power = 0.f;
    std::vector<DevHaltonDim> hdims;
    std::vector<uint16_t> hperm;
    std::vector<float4> ltc;
};
int build_shading_tables(const rgk_scene_desc* d, ShadingTables& out);
