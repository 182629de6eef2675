// Host runtime behind the C ABI of include/rgk.h.
//
//   * scene objects: rgk_scene_create takes what the GPU-free commit unit computes (rgk_commit.h: bounds and epsilon,
//     triangle records, the SAH accelerator, shading tables), or has the accelerator built on the device (rgk_build.h),
//     and uploads it; rgk_scene_refit, tuning, progress;
//   * the round driver: tiles -> per-pixel seeds (a2) -> passes of paths resident in
//     HBM -> raygen / trace / shade / shadow / resolve launches on one HIP stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rgk.h"
#include "device_types.h"
#include "rgk_commit.h"
#include "rgk_kernels.h"
#include "rgk_build.h"
#include "rgk_adapt.h"

namespace {

#define HIPCHK(x)                                                                                     \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess)                                                                         \
            return fail(e_ == hipErrorOutOfMemory ? RGK_ERR_OOM : RGK_ERR_DEVICE, "%s: %s (%s:%d)", #x, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                   \
    } while (0)

// ------------------------------------------------------------------ scene object
// A device allocation with one owner: freed by its destructor, never copied.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int alloc(size_t count) {
        if (count <= n && p) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) return fail(RGK_ERR_OOM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
        n = count;
        // RGK_POISON=1: every fresh device buffer is filled with 0xFF bytes (NaN as float, huge as index), so that any read of
        // memory the pipeline did not write first shows in the results instead of hiding behind zero-filled fresh pages
        static const bool poison = std::getenv("RGK_POISON") != nullptr;
        if (poison) { // (the fill runs on the null stream, the scene's stream is non-blocking: wait for it, or it lands on top of real data)
            (void)hipMemset(p, 0xFF, count * sizeof(T));
            (void)hipDeviceSynchronize();
        }
        return 0;
    }
    int upload(const T* src, size_t count) {
        int rc = alloc(count);
        if (rc) return rc;
        if (count) {
            hipError_t e = hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
            if (e != hipSuccess) return fail(RGK_ERR_DEVICE, "hipMemcpy H2D: %s", hipGetErrorString(e));
        }
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

} // namespace

// Tuning switches of one scene (nothing here changes a result).  Filled ONCE, by read_tuning in rgk_scene_create, from the
// environment (RGK_ENTRY_POINTS, RGK_ENTRY_CAP, RGK_LIGHT_ENTRY, RGK_CONST_LIGHT, RGK_SAMPLE_GROUP, RGK_BATCH_PATHS, RGK_WORKSPACE_GB,
// RGK_BEAM, RGK_DEBUG_BVH, RGK_DEBUG_UTIL); afterwards only rgk_scene_set_tuning changes them -- a round never reads the environment
// (round 2 did, per round: process-global state under a host that may render from two threads).  The build switches are read
// at the same moment, by read_build_options (rgk_commit.h).
struct RgkTuning {
    bool entry_points = true; // camera rays start at their pixel group's entry nodes (k_entry_points)
    bool entry_cap = true;    // ... capped behind the group's first hits from a frame's second round on
    bool light_entry = true;  // first-vertex shadow rays of a single-light scene start at light-side entry nodes
    bool const_light = true;  // eligible scenes (rgk_scene_info::const_light): unidirectional rounds take the light as a launch constant
    int sample_group = -1;    // log2 of the samples of a pixel side by side in the slot order; -1: the compiled default
    size_t batch_paths = 0;   // paths per pass; 0: sized from the memory that is free
    double workspace_gb = 0;  // ... or from this many GB; 0: 96 (160 for bidirectional rounds), at most 60 % of what is free
    int beam = 1;             // pinhole cameras: bounce 0 walks the tree once per pixel for 8 samples (k_trace_camera_beam) -- 1: while the
                              // entry lists are uncapped (a frame's first round), 2: always, 0: never
    bool debug_bvh = false, debug_util = false;
    bool time_post = false;   // feature pass / denoiser: HIP events around their launches (rgk_scene_get_post_timing)
};

// rgk_scene_get_post_timing's `which` (rgk.h): the post-processing call whose launch times a slot holds
enum PostSlot : uint32_t { POST_AOV = 0, POST_DENOISE = 1, POST_DENOISE_VARIANCE = 2, POST_NOISE = 3, POST_FOLD = 4, POST_SLOTS = 5 };
constexpr uint32_t RGK_SCENE_MAGIC = 0x53474b52u; // "RKGS": what a live scene handle starts with (rgk_scene_get_post_timing)
struct rgk_scene {
    uint32_t magic = RGK_SCENE_MAGIC;
    int device = 0;
    RgkTuning tune;
    hipStream_t stream = nullptr;
    rgk_scene_info info{};
    DevScene dev{};
    RgkTraceCfg tcfg{32, 32, nullptr};
    DevBuf<int> ovf; // traversal-stack overflow area (deep trees)
    // scene data
    DevBuf<QNode> nodes;
    DevBuf<TriIsect> tris;
    DevBuf<TriShade> tri_shade;
    DevBuf<DevMaterial> materials;
    DevBuf<float4> texels;
    DevBuf<uint32_t> texels8;
    DevBuf<float> luts;
    DevBuf<DevPointLight> pointlights;
    DevPointLight h_light0{}; // pointlights[0] (const_light_eligible after a refit)
    DevBuf<DevArealLight> areal;
    DevBuf<DevArealTri> areal_tris;
    DevBuf<float4> ltc;
    DevBuf<DevScene> self;    // device-resident copy of `dev` (DevScene::self)
    DevBuf<uint32_t> generic; // queue indices left to the generic-BxDF shade launch
    DevBuf<TexRef> texrefs;   // one TexRef per descriptor texture (rgk_texture_sample)
    // what rgk_scene_refit needs of the descriptor after rgk_scene_create has returned
    DevBuf<uint32_t> d_idx;   // tri_indices on the device
    DevBuf<float4> leaf_pb;   // per leaf reference: its piece of the triangle in the triangle's own coordinates (Prim::pb)
    std::vector<uint32_t> h_idx, h_tri_mat, h_areal_off, h_areal_tris;
    std::vector<rgk_material> h_mats;
    std::vector<float> h_normals;
    uint32_t n_vertices = 0, n_triangles = 0, n_refs = 0, n_nodes = 0;
    uint32_t n_textures = 0, n_materials = 0;
    DevBuf<DevHaltonDim> hdims;
    DevBuf<uint16_t> hperm;
    // workspace
    size_t batch = 0;
    DevBuf<float4> rayA[2], rayB[2], hit, thr, tot, shA, shB, shC, pixsum, light;
    DevBuf<float4> lstart, lv; // bidirectional state (reverse > 0)
    DevBuf<uint32_t> hitlist;  // ... light sub-path: queue indices of the rays that hit (k_list_hits)
    DevBuf<uint32_t> lvmask, connlist; // ... which light vertices a slot has; queue indices of the camera vertices with connections
    DevBuf<float4> conn, jobs, rads;   // ... their records (k_shade<BDPT> -> k_connect) and the vertex queue of k_trace_shadow_jobs
    uint32_t batch_reverse = 0;
    DevBuf<float> htab;
    DevBuf<float2> nearfar;
    DevBuf<uint32_t> counters, pix_xy, pix_seed, tile_buf;
    DevBuf<int> entry; // RGK_ENTRY_K traversal entry nodes per group of RGK_ENTRY_PIX pixels of the round's list
    DevBuf<float> entry_cap;  // ... and up to which distance each list is complete (k_entry_points)
    size_t entry_capped = 0;  // pixels of the round's list whose lists have been rebuilt with this frame's first-hit distances
    DevBuf<int> lentry;       // the same for the first vertex's shadow rays (single-light scenes), rebuilt per pass
    DevBuf<uint32_t> trange;  // per pixel group: nearest / farthest first hit of a block of samples (float bits)
    DevBuf<float4> lbox;      // per pixel group: the box its light-side entry nodes are good for
    size_t lentry_done = 0;   // how many pixels of the round's list the light-side entries of this frame cover so far
    uint64_t entry_key = 0; // camera + tile geometry they were made for
    size_t entry_n = 0;
    DevBuf<unsigned long long> stats;
    DevBuf<float> scratch_f;
    DevBuf<uint32_t> scratch_u;
    DevBuf<float4> dn_col[2], dn_guide; // the denoiser's two colour planes and its guide plane {n.xyz, z}
    DevBuf<rgk_noise_tile> nz_tiles;    // the noise estimate's per-tile sums
    DevBuf<uint32_t> fold_buf;          // the round fold's tile list (5 words per tile), then its flags (a byte per tile)
    std::vector<double> post_ms[POST_SLOTS]; // launch times of the last call of each kind (tuning "time_post")
    std::vector<hipEvent_t> events;
    uint32_t* h_counters = nullptr; // pinned
    // progress, read by rgk_scene_get_progress from any thread
    std::atomic<uint32_t> prog_stages{0}, prog_rounds{0}, prog_busy{0};
    uint32_t* h_stage = nullptr; // pinned word the DEVICE writes (k_stage_mark): stages of the running round that are done
    std::atomic<uint64_t> prog_pixels{0}, prog_paths{0};
    // What is not a DevBuf.  The DevBuf members free themselves after this body has run, and no queued kernel can read one
    // by then: the body waits for the stream first (an entry point waits for the work it queued before it returns, but one
    // that fails halfway may leave some behind).
    ~rgk_scene() {
        magic = 0;
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto e : events) (void)hipEventDestroy(e);
        if (h_counters) (void)hipHostFree(h_counters);
        if (h_stage) (void)hipHostFree(h_stage);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

int ensure_workspace(rgk_scene* s, size_t paths, uint32_t reverse = 0) {
    if (paths <= s->batch && reverse <= s->batch_reverse) return 0;
    if (s->batch) { paths = std::max(paths, s->batch); reverse = std::max(reverse, s->batch_reverse); }
    int rc = 0;
    for (int i = 0; i < 2 && !rc; i++) { rc = s->rayA[i].alloc(paths); if (!rc) rc = s->rayB[i].alloc(paths); }
    if (!rc) rc = s->hit.alloc(paths);
    if (!rc) rc = s->thr.alloc(paths);
    if (!rc) rc = s->tot.alloc(paths);
    // plain shadow queue: one ray {shA, shB, shC} per path and bounce
    if (!rc) rc = s->shA.alloc(paths);
    if (!rc) rc = s->shB.alloc(paths);
    if (!rc) rc = s->shC.alloc(paths);
    if (reverse) {
        if (!rc) rc = s->lstart.alloc(paths);
        if (!rc) rc = s->lv.alloc(paths * RGK_LV_FLOAT4 * reverse);
        if (!rc) rc = s->hitlist.alloc(paths);
        if (!rc) rc = s->lvmask.alloc(paths);
        if (!rc) rc = s->connlist.alloc(paths);
        if (!rc) rc = s->conn.alloc(paths * 6);                  // the record a camera vertex with connections leaves
        if (!rc) rc = s->jobs.alloc(paths * 4);                  // vertex queue: {vertex}{contribution, mask}{emission}{NEE ray start}
        if (!rc) rc = s->rads.alloc(paths * ((size_t)reverse + 1)); // ... and one radiance per ray
    }
    if (!rc) rc = s->light.alloc(paths);
    if (!rc) rc = s->generic.alloc(paths);
    if (!rc) rc = s->counters.alloc(2 * RGK_CNT_TOTAL); // [0] camera phase, [1] light sub-path phase
    if (!rc) rc = s->stats.alloc(8);
    if (rc) { s->batch = 0; s->batch_reverse = 0; return rc; } // some buffers are gone: the next call starts over
    if (!s->h_counters) HIPCHK(hipHostMalloc((void**)&s->h_counters, 2 * RGK_CNT_TOTAL * sizeof(uint32_t)));
    if (!s->h_stage) { HIPCHK(hipHostMalloc((void**)&s->h_stage, sizeof(uint32_t))); *s->h_stage = 0; }
    s->batch = paths;
    s->batch_reverse = reverse;
    return 0;
}

template <typename T>
int down(T* dst, const DevBuf<T>& b, size_t count) {
    if (hipMemcpy(dst, b.p, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return fail(RGK_ERR_DEVICE, "hipMemcpy D2H failed");
    return 0;
}

// Event `i` of the scene's pool, which grows on demand and goes with the scene.  A round and a post call never overlap on a scene
// (prog_busy), so each call counts from 0.
int scene_event(rgk_scene* s, size_t i, hipEvent_t& e) {
    while (s->events.size() <= i) { hipEvent_t n; HIPCHK(hipEventCreate(&n)); s->events.push_back(n); }
    e = s->events[i];
    return 0;
}

// The frame sizes the kernels' 16-bit pixel coordinates can hold.
int check_frame_size(uint32_t xres, uint32_t yres) {
    if (xres == 0 || yres == 0 || xres > 65535 || yres > 65535) return fail(RGK_ERR_INVALID, "resolution out of range");
    return RGK_OK;
}

// The eight traversal-stats words: closest nodes / triangles, shadow nodes / triangles, and the walker's occupancy counters.
int read_stats(const rgk_scene* s, unsigned long long (&h)[8]) { return down(h, s->stats, 8); }

RgkTuning read_tuning() {
    auto off = [](const char* name) { const char* e = std::getenv(name); return e && e[0] == '0'; };
    RgkTuning t;
    t.entry_points = !off("RGK_ENTRY_POINTS"); t.entry_cap = !off("RGK_ENTRY_CAP"); t.light_entry = !off("RGK_LIGHT_ENTRY");
    t.const_light = !off("RGK_CONST_LIGHT");
    if (const char* e = std::getenv("RGK_SAMPLE_GROUP")) t.sample_group = std::min(6, std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("RGK_BATCH_PATHS")) t.batch_paths = std::max<size_t>(1024, strtoull(e, nullptr, 10));
    if (const char* e = std::getenv("RGK_WORKSPACE_GB")) t.workspace_gb = atof(e);
    if (const char* e = std::getenv("RGK_BEAM")) t.beam = std::min(2, std::max(0, std::atoi(e)));
    t.debug_bvh = std::getenv("RGK_DEBUG_BVH") != nullptr; t.debug_util = std::getenv("RGK_DEBUG_UTIL") != nullptr;
    return t;
}

// The per-frame lists (entry nodes, their caps, light-side entries) were made for the old boxes or switches: the next round rebuilds them.
void invalidate_frame_lists(rgk_scene* s) { s->entry_key = 0; s->entry_n = 0; s->entry_capped = 0; s->lentry_done = 0; }

// Epsilon and the epsilon-padded box of commit_bounds, where the kernels and rgk_scene_get_info read them.
void set_bounds(rgk_scene* s, const float mn[3], const float mx[3], float eps) {
    DevScene& ds = s->dev;
    ds.epsilon = eps;
    s->info.epsilon = eps;
    for (int a = 0; a < 3; a++) {
        ds.bb_min[a] = mn[a] - eps; ds.bb_max[a] = mx[a] + eps;
        s->info.bbox_min[a] = ds.bb_min[a]; s->info.bbox_max[a] = ds.bb_max[a];
    }
}

// What rgk_scene_create knows about the tree once it is built, by either builder.
struct AccelInfo {
    uint32_t n_nodes = 0, n_refs = 0, max_depth = 0, max_stack = 0;
    bool on_device = false; // nodes and leaf records are on the device already
};

// LBVH on the GPU (rgk_build.hip): the references go up, nodes and leaf-ordered records stay on the device
int build_accel_device(rgk_scene* s, const std::vector<Prim>& prims, const std::vector<TriIsect>& recs, const float mn[3], const float mx[3], float eps,
                       const BuildOptions& opt, AccelInfo& acc) {
    std::vector<RgkBuildPrim> bp(prims.size());
    for (size_t i = 0; i < prims.size(); i++) {
        for (int a = 0; a < 3; a++) { bp[i].bmin[a] = prims[i].bmin[a]; bp[i].bmax[a] = prims[i].bmax[a]; }
        bp[i].tri = prims[i].tri;
        for (int a = 0; a < 4; a++) bp[i].pb[a] = prims[i].pb[a];
    }
    int rc;
    DevBuf<TriIsect> d_recs;
    if ((rc = d_recs.upload(recs.data(), recs.size())) || (rc = s->nodes.alloc(prims.size())) || (rc = s->tris.alloc(prims.size())) || (rc = s->leaf_pb.alloc(prims.size()))) return rc;
    uint32_t levels = 0;
    const char* err = "";
    acc.n_refs = (uint32_t)prims.size();
    rc = rgk_build_bvh4_device(s->stream, bp.data(), acc.n_refs, mn, mx, eps, (uint32_t)opt.max_leaf_dev, opt.lbvh_rotate, opt.lbvh_ploc, opt.lbvh_morton_bits, d_recs.p,
                               s->nodes.p, s->tris.p, s->leaf_pb.p, &acc.n_nodes, &levels, &err);
    if (rc) return fail(rc, "device BVH build: %s", err);
    acc.max_depth = levels;
    acc.max_stack = 3 * levels; // three pushes per level at most
    acc.on_device = true;
    return 0;
}

#ifndef RGK_BUILD_AUTO_DEVICE_REFS
#define RGK_BUILD_AUTO_DEVICE_REFS 500000
#endif
// Which builder: asked for explicitly, or (RGK_BUILD_AUTO) by size -- from half a million references on, the host's SAH build
// takes seconds (1.5 s at 1.05 M) where the device build takes 0.15 s and traces within 2 % of it.  The host build's tables
// stay in `host` until upload_tables.
int build_accel(rgk_scene* s, uint32_t build_flags, std::vector<Prim>& prims, const std::vector<TriIsect>& recs, const float mn[3], const float mx[3], float eps,
                const BuildOptions& opt, HostAccel& host, AccelInfo& acc) {
    if (prims.empty()) return fail(RGK_ERR_INVALID, "every triangle is degenerate");
    if (prims.size() >= (1u << 25)) return fail(RGK_ERR_UNSUPPORTED, "too many triangles (32-bit byte offsets into the triangle tables: < 2^25)");
    const bool want_device = (build_flags & RGK_BUILD_DEVICE) || (!(build_flags & RGK_BUILD_HOST_SAH) && prims.size() >= (size_t)RGK_BUILD_AUTO_DEVICE_REFS);
    if (want_device && prims.size() > (size_t)opt.max_leaf_dev) return build_accel_device(s, prims, recs, mn, mx, eps, opt, acc);
    if (int rc = build_host_accel(prims, recs, eps, opt, host)) return rc;
    acc.n_nodes = (uint32_t)host.qnodes.size(); acc.n_refs = (uint32_t)host.leaf_recs.size();
    acc.max_depth = host.max_depth; acc.max_stack = host.max_stack;
    return 0;
}

// Traversal stack: 16 entries per lane in LDS + per-lane overflow in global memory (rgk_kernels.hip RGK_TRACE_DISPATCH)
int configure_stack(rgk_scene* s, uint32_t max_stack, const BuildOptions& opt) {
    if (max_stack + 1 + RGK_ENTRY_K > 256) return fail(RGK_ERR_UNSUPPORTED, "BVH needs %u traversal-stack entries (max 256)", max_stack + 1);
    const int need = (int)max_stack + 1 + RGK_ENTRY_K; // (+ the entry nodes a camera ray starts with)
    if (!opt.stack_ovf && need <= 32) { s->tcfg.stack = 32; s->tcfg.lds = 32; }
    else { s->tcfg.stack = 256; s->tcfg.lds = opt.stack_lds; }
    s->tcfg.ovf = nullptr;
    if (s->tcfg.lds < s->tcfg.stack) {
        const size_t per_lane = (size_t)std::max(need - std::min(s->tcfg.lds, 8), 1); // (k_trace_camera_beam keeps 8 entries in LDS)
        if (int rc = s->ovf.alloc((size_t)rgk_trace_grid(s->tcfg.lds) * RGK_TRACE_BLOCK * per_lane)) return rc;
        s->tcfg.ovf = s->ovf.p;
    }
    return 0;
}

// Keeps what rgk_scene_refit needs of the descriptor, then uploads every table; the host build's tree goes up here too.
int upload_tables(rgk_scene* s, const rgk_scene_desc* d, const AccelInfo& acc, const HostAccel& host, const ShadingTables& sh) {
    const uint32_t nt = d->n_triangles;
    s->n_textures = d->n_textures; s->n_materials = d->n_materials;
    s->n_vertices = d->n_vertices; s->n_triangles = nt; s->n_refs = acc.n_refs; s->n_nodes = acc.n_nodes;
    s->h_idx.assign(d->tri_indices, d->tri_indices + 3 * (size_t)nt);
    s->h_tri_mat.assign(d->tri_material, d->tri_material + nt);
    s->h_mats.assign(d->materials, d->materials + d->n_materials);
    s->h_normals.assign(d->normals, d->normals + 3 * (size_t)d->n_vertices);
    if (d->n_areal_lights) {
        s->h_areal_off.assign(d->areal_offsets, d->areal_offsets + d->n_areal_lights + 1);
        s->h_areal_tris.assign(d->areal_tris, d->areal_tris + d->areal_offsets[d->n_areal_lights]);
    }
    int rc;
    if ((rc = s->d_idx.upload(s->h_idx.data(), s->h_idx.size()))) return rc;
    if ((rc = s->texrefs.upload(sh.tex.refs.data(), sh.tex.refs.size()))) return rc;
    if (!acc.on_device && ((rc = s->nodes.upload(host.qnodes.data(), host.qnodes.size())) || (rc = s->tris.upload(host.leaf_recs.data(), host.leaf_recs.size())) ||
                           (rc = s->leaf_pb.upload(host.leaf_pb.data(), host.leaf_pb.size()))))
        return rc;
    if ((rc = s->tri_shade.upload(sh.tri_shade.data(), sh.tri_shade.size())) || (rc = s->materials.upload(sh.materials.data(), sh.materials.size())) ||
        (rc = s->texels.upload(sh.tex.texels.data(), sh.tex.texels.size())) || (rc = s->texels8.upload(sh.tex.texels8.data(), sh.tex.texels8.size())) ||
        (rc = s->luts.upload(sh.tex.luts.data(), sh.tex.luts.size())) || (rc = s->pointlights.upload(sh.pointlights.data(), sh.pointlights.size())) ||
        (rc = s->areal.upload(sh.areal.data(), sh.areal.size())) || (rc = s->areal_tris.upload(sh.areal_tris.data(), sh.areal_tris.size())) ||
        (rc = s->hdims.upload(sh.hdims.data(), sh.hdims.size())) || (rc = s->hperm.upload(sh.hperm.data(), sh.hperm.size())) || (rc = s->ltc.upload(sh.ltc.data(), sh.ltc.size())))
        return rc;
    return 0;
}

// DevScene (host copy and device copy) and the rest of rgk_scene_info, once every table is on the device.
int fill_dev_scene(rgk_scene* s, const rgk_scene_desc* d, const AccelInfo& acc, const ShadingTables& sh, const BuildOptions& opt) {
    DevScene& ds = s->dev;
    ds.nodes = s->nodes.p;
    ds.walk_q = opt.walk_q;
    ds.tris = s->tris.p; ds.tri_shade = s->tri_shade.p;
    ds.materials = s->materials.p; ds.texels = s->texels.p; ds.texels8 = s->texels8.p; ds.luts = s->luts.p; ds.n_lut_floats = (uint32_t)sh.tex.luts.size(); ds.n_materials = (uint32_t)sh.materials.size();
    ds.pointlights = s->pointlights.p; ds.areal = s->areal.p; ds.areal_tris = s->areal_tris.p;
    ds.ltc = s->ltc.p; ds.hdims = s->hdims.p; ds.hperm = s->hperm.p;
    ds.n_pointlights = (uint32_t)sh.pointlights.size(); ds.n_areal = (uint32_t)sh.areal.size();
    ds.total_point_power = sh.total_point_power; ds.total_areal_power = sh.total_areal_power;
    if (!sh.pointlights.empty()) {
        const DevPointLight& l0 = sh.pointlights[0];
        s->h_light0 = l0;
        for (int k = 0; k < 3; k++) { ds.cl_pos[k] = l0.pos[k]; ds.cl_color[k] = l0.color[k]; }
        ds.cl_intensity = l0.intensity;
    }
    ds.has_texcoords = d->texcoords ? 1u : 0u;
    ds.sky_mode = d->sky_mode;
    for (int k = 0; k < 3; k++) ds.sky_color[k] = d->sky_color[k];
    ds.sky_intensity = d->sky_intensity; ds.sky_rotate = d->sky_rotate; ds.sky_tex = tex_ref(sh.tex.refs, d->sky_mode == RGK_SKY_ENVMAP ? d->sky_texture : -1);
    if (int rc = s->self.alloc(1)) return rc;
    ds.self = s->self.p;
    if (hipMemcpy(s->self.p, &ds, sizeof(DevScene), hipMemcpyHostToDevice) != hipSuccess) return fail(RGK_ERR_DEVICE, "hipMemcpy(DevScene)");

    rgk_scene_info& inf = s->info;
    inf.total_areal_power = sh.total_areal_power; inf.total_point_power = sh.total_point_power;
    inf.n_nodes = acc.n_nodes; inf.node_bytes = RGK_NODE_BYTES; inf.tri_bytes = RGK_TRI_BYTES;
    inf.max_depth = acc.max_depth; inf.n_leaf_refs = acc.n_refs;
    inf.n_float_textures = sh.tex.n_float; inf.n_palettized_textures = sh.tex.n_palettized;
    inf.const_light = const_light_eligible(ds, &s->h_light0);
    return 0;
}

} // namespace

extern "C" {

int rgk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

#ifndef RGK_SAMPLE_GROUP_DEFAULT
#define RGK_SAMPLE_GROUP_DEFAULT 3 // 8 samples of a pixel side by side: swept 0..6 on the Sponza proxy (154.2, -, 149.6, 148.4, 148.1, 150.3, 150.0 ms per round)
#endif
int rgk_scene_create(const rgk_scene_desc* d, int device, rgk_scene** out) {
    if (!out) return fail(RGK_ERR_INVALID, "null output pointer");
    *out = nullptr;
    int rc = validate_desc(d);
    if (rc) return rc;
    if (std::getenv("RGK_DEBUG_DESC")) debug_desc(d);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RGK_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(RGK_ERR_INVALID, "device %d out of range (%d visible)", device, ndev);
    HIPCHK(hipSetDevice(device));
    rgk_scene* s = new rgk_scene;
    s->device = device;
    struct Guard { rgk_scene* s; ~Guard() { delete s; } } guard{s};
    HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    s->tune = read_tuning();
    const BuildOptions opt = read_build_options();

    // ---- Commit: bounds, epsilon; planes, intersection records and the build's references
    float mn[3], mx[3], eps;
    if ((rc = commit_bounds(d->vertices, d->tri_indices, d->n_triangles, mn, mx, &eps))) return rc;
    set_bounds(s, mn, mx, eps);
    std::vector<TriIsect> recs;
    std::vector<Prim> prims;
    commit_triangles(d->vertices, d->tri_indices, d->n_triangles, split_threshold(opt, eps), recs, prims);

    // ---- accelerator and its traversal stack
    HostAccel host;
    AccelInfo acc;
    if ((rc = build_accel(s, d->build_flags, prims, recs, mn, mx, eps, opt, host, acc))) return rc;
    if ((rc = configure_stack(s, acc.max_stack, opt))) return rc;

    // ---- shading tables; upload; DevScene
    ShadingTables sh;
    if ((rc = build_shading_tables(d, sh))) return rc;
    if ((rc = upload_tables(s, d, acc, host, sh))) return rc;
    if (s->tune.debug_bvh)
        std::fprintf(stderr, "[rgk] bvh4 (%s) nodes %u max_stack %u max_depth %u refs %u of %u triangles\n", acc.on_device ? "device LBVH" : "host SAH", acc.n_nodes, acc.max_stack,
                     acc.max_depth, acc.n_refs, d->n_triangles);
    if ((rc = fill_dev_scene(s, d, acc, sh, opt))) return rc;
    guard.s = nullptr;
    *out = s;
    return RGK_OK;
}

int rgk_scene_refit(rgk_scene* s, const float* vertices, const float* normals, const float* tangents) {
    if (!s || !vertices) return fail(RGK_ERR_INVALID, "null argument");
    if (s->prog_busy.load()) return fail(RGK_ERR_INVALID, "rgk_scene_refit while a round is in flight on this scene");
    HIPCHK(hipSetDevice(s->device));
    const uint32_t nt = s->n_triangles, nv = s->n_vertices;
    // ---- Commit's scalars for the new positions
    int rc;
    float mn[3], mx[3], eps;
    if ((rc = commit_bounds(vertices, s->h_idx.data(), nt, mn, mx, &eps))) return rc;
    // ---- records, shading normals / tangents, and the tree's boxes: on the device
    if ((rc = s->scratch_f.upload(vertices, 3 * (size_t)nv))) return rc;
    DevBuf<float> d_n, d_t;
    if (normals && (rc = d_n.upload(normals, 3 * (size_t)nv))) return rc;
    if (tangents && (rc = d_t.upload(tangents, 3 * (size_t)nv))) return rc;
    const char* err = "";
    rc = rgk_refit_bvh4_device(s->stream, s->n_refs, s->n_nodes, nt, s->scratch_f.p, normals ? d_n.p : nullptr, tangents ? d_t.p : nullptr, s->d_idx.p, s->leaf_pb.p, eps,
                               s->tris.p, s->nodes.p, s->tri_shade.p, &err);
    if (rc) return fail(rc, "refit: %s", err);
    // ---- areal-light tables (areas, positions, vertex-A normals change with the vertices)
    if (normals) s->h_normals.assign(normals, normals + 3 * (size_t)nv);
    std::vector<DevArealLight> als;
    std::vector<DevArealTri> ats;
    float total_areal = 0.f;
    build_areal_tables(vertices, s->h_normals.data(), s->h_idx.data(), s->h_tri_mat.data(), s->h_mats.data(), (uint32_t)(s->h_areal_off.empty() ? 0 : s->h_areal_off.size() - 1),
                       s->h_areal_off.data(), s->h_areal_tris.data(), als, ats, total_areal);
    if ((rc = s->areal.upload(als.data(), als.size())) || (rc = s->areal_tris.upload(ats.data(), ats.size()))) return rc;
    DevScene& ds = s->dev;
    ds.areal = s->areal.p; ds.areal_tris = s->areal_tris.p; ds.n_areal = (uint32_t)als.size(); ds.total_areal_power = total_areal;
    set_bounds(s, mn, mx, eps);
    if (hipMemcpy(s->self.p, &ds, sizeof(DevScene), hipMemcpyHostToDevice) != hipSuccess) return fail(RGK_ERR_DEVICE, "hipMemcpy(DevScene)");
    s->info.total_areal_power = total_areal;
    s->info.const_light = const_light_eligible(ds, &s->h_light0);
    invalidate_frame_lists(s);
    return RGK_OK;
}

void rgk_scene_destroy(rgk_scene* s) { delete s; }

int rgk_scene_get_info(const rgk_scene* s, rgk_scene_info* out) {
    if (!s || !out) return fail(RGK_ERR_INVALID, "null argument");
    *out = s->info;
    return RGK_OK;
}

int rgk_scene_get_progress(const rgk_scene* s, rgk_progress* out) {
    if (!s || !out) return fail(RGK_ERR_INVALID, "null argument");
    out->stage = s->h_stage ? *(volatile const uint32_t*)s->h_stage : 0u; out->stages = s->prog_stages.load(); out->rounds = s->prog_rounds.load(); out->busy = s->prog_busy.load();
    out->round_pixels = s->prog_pixels.load(); out->round_paths = s->prog_paths.load();
    if (out->stage > out->stages) out->stage = out->stages;
    return RGK_OK;
}

int rgk_scene_set_tuning(rgk_scene* s, const char* key, double value) {
    if (!s || !key) return fail(RGK_ERR_INVALID, "null argument");
    if (s->prog_busy.load()) return fail(RGK_ERR_INVALID, "rgk_scene_set_tuning while a round is in flight on this scene");
    RgkTuning& t = s->tune;
    const std::string k(key);
    if (k == "entry_points") t.entry_points = value != 0;
    else if (k == "entry_cap") t.entry_cap = value != 0;
    else if (k == "light_entry") t.light_entry = value != 0;
    else if (k == "const_light") t.const_light = value != 0;
    else if (k == "sample_group") t.sample_group = value < 0 ? -1 : (int)std::min(6.0, value);
    else if (k == "batch_paths") t.batch_paths = value <= 0 ? 0 : std::max<size_t>(1024, (size_t)value);
    else if (k == "workspace_gb") t.workspace_gb = value <= 0 ? 0.0 : value;
    else if (k == "beam") t.beam = (int)std::min(2.0, std::max(0.0, value));
    else if (k == "time_post") { t.time_post = value != 0; return RGK_OK; } // (no launch of a round depends on it: the frame's lists stay)
    else return fail(RGK_ERR_INVALID, "unknown tuning key '%s'", key);
    invalidate_frame_lists(s);
    return RGK_OK;
}

int rgk_generate_task_list(uint32_t tile_size, uint32_t xres, uint32_t yres, float mid_x, float mid_y, uint32_t seedstart,
                           uint32_t seedcount_base, rgk_tile* tiles, uint32_t* n_tiles) {
    if (!n_tiles || tile_size == 0) return fail(RGK_ERR_INVALID, "bad argument");
    struct T { rgk_tile t; float d; };
    std::vector<T> v;
    for (uint32_t yp = 0; yp < yres; yp += tile_size)
        for (uint32_t xp = 0; xp < xres; xp += tile_size) {
            T t;
            t.t.x0 = xp; t.t.x1 = std::min(xres, xp + tile_size);
            t.t.y0 = yp; t.t.y1 = std::min(yres, yp + tile_size);
            t.t.seed = 0;
            float mx = (t.t.x0 + t.t.x1) / 2.0f, my = (t.t.y0 + t.t.y1) / 2.0f; // RenderTask::midpoint tracer.hpp:18
            float dx = mid_x - mx, dy = mid_y - my;
            t.d = std::sqrt(dx * dx + dy * dy);
            v.push_back(t);
        }
    std::stable_sort(v.begin(), v.end(), [](const T& a, const T& b) { return a.d < b.d; });
    if (tiles) {
        if (*n_tiles < v.size()) return fail(RGK_ERR_INVALID, "tile buffer too small (%u < %zu)", *n_tiles, v.size());
        for (size_t i = 0; i < v.size(); i++) { tiles[i] = v[i].t; tiles[i].seed = seedstart + seedcount_base + (uint32_t)i; }
    }
    *n_tiles = (uint32_t)v.size();
    return RGK_OK;
}

int rgk_camera_init(rgk_camera* o, const float pos[3], const float lookat[3], const float upv[3], float yview, float xview, int32_t xsize,
                    int32_t ysize, float focus_plane, float lens_size) {
    // Camera::Camera, reference src/camera.cpp:7-24
    if (!o || !pos || !lookat || !upv) return fail(RGK_ERR_INVALID, "null argument");
    V3 origin{pos[0], pos[1], pos[2]}, la{lookat[0], lookat[1], lookat[2]}, up{upv[0], upv[1], upv[2]};
    V3 direction = normv(sub(la, origin));
    V3 left = normv(crossv(up, direction));
    up = normv(crossv(left, direction));
    V3 vx = scale(scale(left, -xview), focus_plane);
    V3 vy = scale(scale(up, yview), focus_plane);
    V3 a = {origin.x + direction.x * focus_plane, origin.y + direction.y * focus_plane, origin.z + direction.z * focus_plane};
    V3 hy = scale(vy, 0.5f), hx = scale(vx, 0.5f);
    V3 vs = sub(sub(a, hy), hx);
    auto put = [](float* dst, V3 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; };
    put(o->origin, origin); put(o->direction, direction); put(o->cameraup, up); put(o->cameraleft, left);
    put(o->viewscreen, vs); put(o->viewscreen_x, vx); put(o->viewscreen_y, vy);
    o->lens_size = lens_size; o->xsize = xsize; o->ysize = ysize;
    return RGK_OK;
}

static void make_camera(const rgk_camera* c, DevCamera& o) { // the members RenderRound's `const Camera&` carries, as they are
    for (int k = 0; k < 3; k++) {
        o.origin[k] = c->origin[k]; o.direction[k] = c->direction[k]; o.up[k] = c->cameraup[k]; o.left[k] = c->cameraleft[k];
        o.viewscreen[k] = c->viewscreen[k]; o.viewscreen_x[k] = c->viewscreen_x[k]; o.viewscreen_y[k] = c->viewscreen_y[k];
    }
    o.lens_size = c->lens_size; o.xsize = c->xsize; o.ysize = c->ysize;
}

// Paths resident per pass.  The path state is sized for the machine, not for a cache: by default
// 96 GB of the 288 GB HBM3E (measured on Sponza 1080p x 256 spp: 2^25 paths/pass 2235 Mpaths/s, 2^27 2398,
// 2^28 2440 -- fewer, longer launches and shorter tails; 48 -> 96 GB: +1.4 % there, +6 % on the bidirectional
// configuration whose paths carry 3.5x the state).  RGK_WORKSPACE_GB / RGK_BATCH_PATHS override.
static size_t batch_paths(const RgkTuning& tune, uint32_t reverse) {
    if (tune.batch_paths) return tune.batch_paths;
    // rays 2 x 32, hit 16, state 16, sum 16, light 16, shadow queue 48, generic list 4; bidirectional: + light start 16, light
    // vertices, hit list 4, and the vertex queue's 2 + (1 + reverse) more float4 than a ray's 3
    const size_t per_path = 180 + (reverse ? 16 + 16 * RGK_LV_FLOAT4 * (size_t)reverse + 12 + 16 * (6 + 4 + (size_t)reverse + 1) : 0);
    const bool g = tune.workspace_gb > 0;
    double gb = g ? tune.workspace_gb : (reverse ? 160.0 : 96.0); // bidirectional paths carry 3.5x the state: 765 -> 781 Mpaths/s
    if (!g) { // a shared or smaller card: never plan for more than 60 % of what is free right now
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) gb = std::min(gb, 0.6 * (double)free_b / 1e9);
    }
    size_t b = (size_t)(gb * 1e9 / (double)per_path);
    return std::min<size_t>(std::max<size_t>(b, 1024), (size_t)1 << 30);
}

} // extern "C"

namespace {
// ------------------------------------------------------------------ the round driver
// rgk_render_round_device: the round's pixel list (prepare_round_lists), a plan of passes the workspace holds (plan_passes), and
// per pass -- pixels [j0, j0 + npix) of the list x samples [s0, s0 + ns) -- its launches queued on the scene's stream
// (queue_pass), a wait, and its queue counters added to the round's totals (add_pass_counters).

// Per-kernel records of a round (rgk_counters::kernel and the four class sums).  RGK_FLAG_TIME_KERNELS: a pair of events around
// every launch.  RGK_FLAG_COUNT_TRAVERSAL: the traversal counters (stats[0..3]: closest nodes / triangles, shadow nodes /
// triangles) are read back after every traversal launch, so that each kernel gets its own share (stream-ordered copies; nobody
// times a counting round).  The pass code names the kernel class of each launch: run(class, launch).
struct KernelLog {
    rgk_scene* s;
    bool timing, count_stats;
    struct Ev { int cls; hipEvent_t a, b; };
    std::vector<Ev> evs;
    size_t ev_used = 0; // events of the scene's pool taken by this round
    std::vector<std::pair<int, std::array<unsigned long long, 4>>> snaps;

    KernelLog(rgk_scene* s_, uint32_t flags)
        : s(s_), timing((flags & RGK_FLAG_TIME_KERNELS) != 0), count_stats((flags & RGK_FLAG_COUNT_TRAVERSAL) != 0) {
        if (count_stats) snaps.reserve(4096);
    }
    static bool closest(int k) { return k == RGK_K_TRACE_CAMERA || k == RGK_K_TRACE_CLOSEST || k == RGK_K_LIGHT_TRACE; }
    static bool shadow(int k) { return k == RGK_K_SHADOW_FIRST || k == RGK_K_SHADOW || k == RGK_K_SHADOW_JOBS || k == RGK_K_LIGHT_SPLAT; }
    static bool shade(int k) { return k == RGK_K_SHADE_FIRST || k == RGK_K_SHADE || k == RGK_K_CONNECT || k == RGK_K_LIGHT_SHADE; }
    int event(hipEvent_t& e) { return scene_event(s, ev_used++, e); }
    template <class Launch>
    int run(int cls, Launch&& launch) {
        Ev ev{cls, nullptr, nullptr};
        if (timing) {
            int rc;
            if ((rc = event(ev.a)) || (rc = event(ev.b))) return rc;
            HIPCHK(hipEventRecord(ev.a, s->stream));
        }
        launch();
        if (timing) {
            HIPCHK(hipEventRecord(ev.b, s->stream));
            evs.push_back(ev);
        }
        if (count_stats && (closest(cls) || shadow(cls))) {
            snaps.emplace_back(cls, std::array<unsigned long long, 4>{});
            HIPCHK(hipMemcpyAsync(snaps.back().second.data(), s->stats.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
            HIPCHK(hipStreamSynchronize(s->stream));
        }
        return 0;
    }
    int fold(rgk_counters& c) const {
        for (const Ev& e : evs) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
            rgk_kernel_stat& ks = c.kernel[e.cls];
            ks.ms += ms; ks.launches++;
            if (closest(e.cls)) { c.ms_trace += ms; c.n_trace_launches++; }
            else if (shadow(e.cls)) { c.ms_shadow += ms; c.n_shadow_launches++; }
            else if (shade(e.cls)) { c.ms_shade += ms; c.n_shade_launches++; }
            else c.ms_other += ms;
        }
        std::array<unsigned long long, 4> prev{}; // per-kernel traversal counters: differences between consecutive read-backs
        for (const auto& sn : snaps) {
            rgk_kernel_stat& ks = c.kernel[sn.first];
            const int o = closest(sn.first) ? 0 : 2;
            ks.node_visits += sn.second[o] - prev[o];
            ks.tri_tests += sn.second[o + 1] - prev[o + 1];
            prev = sn.second;
        }
        return 0;
    }
};

// Deep path loops (depth > 12): the length of the next queue is read back every other bounce from the fourth on; it bounds the
// grids of the following launches (queues only shrink) and ends the loop once no path is left.  The copy lands in pinned memory;
// polling it costs microseconds where hipStreamSynchronize was measured at 2-3 ms per call (blocking wait), more than the
// launches it saves.
int queue_len(rgk_scene* s, const uint32_t* dptr, uint32_t& out) {
    volatile uint32_t* h = s->h_counters;
    h[0] = 0xffffffffu; // never a queue length (queues hold < 2^30 entries)
    HIPCHK(hipMemcpyAsync(s->h_counters, dptr, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    for (uint64_t spins = 0; h[0] == 0xffffffffu; spins++) {
        if ((spins & 0xfffff) != 0xfffff) continue;
        // every ~1 M polls ask the stream: not-ready means keep polling, success means the copy has landed (re-read), anything
        // else is a sticky launch / device error that would otherwise spin here for ever
        const hipError_t q = hipStreamQuery(s->stream);
        if (q == hipErrorNotReady) continue;
        if (q != hipSuccess) return fail(RGK_ERR_DEVICE, "queue-length read-back: %s", hipGetErrorString(q));
        if (h[0] == 0xffffffffu) HIPCHK(hipStreamSynchronize(s->stream));
        if (h[0] == 0xffffffffu) return fail(RGK_ERR_DEVICE, "queue-length read-back never landed");
        break;
    }
    out = h[0];
    return 0;
}

// A finished pass's share of the round's totals, from its host counter blocks (camera phase, then light sub-path phase): path
// and shadow rays as the reference counts them, and what each kernel processed (rays / vertices / paths).
void add_pass_counters(const uint32_t* hc, const PassParams& pp, bool light_entry, rgk_counters& c) {
    const uint32_t* hl = hc + RGK_CNT_TOTAL;
    const uint32_t n0 = pp.npix * pp.ns;
    auto units = [&c](int k) -> uint64_t& { return c.kernel[k].units; };
    for (uint32_t b = 0; b < pp.depth; b++) { c.path_rays += hc[RGK_CNT_QUEUE + b]; c.shadow_rays += hc[RGK_CNT_SHADOW + b] + hc[RGK_CNT_SRAYS + b]; }
    units(RGK_K_TRACE_CAMERA) += hc[RGK_CNT_QUEUE]; units(RGK_K_SHADE_FIRST) += hc[RGK_CNT_QUEUE];
    for (uint32_t b = 1; b < pp.depth; b++) { units(RGK_K_TRACE_CLOSEST) += hc[RGK_CNT_QUEUE + b]; units(RGK_K_SHADE) += hc[RGK_CNT_QUEUE + b]; }
    for (uint32_t b = 0; b < pp.depth; b++) {
        units((b == 0 && light_entry) ? RGK_K_SHADOW_FIRST : RGK_K_SHADOW) += hc[RGK_CNT_SHADOW + b];
        units(RGK_K_SHADOW_JOBS) += hc[RGK_CNT_CONN + b]; units(RGK_K_CONNECT) += hc[RGK_CNT_CONN + b];
    }
    for (uint32_t k = 0; k < pp.reverse; k++) {
        units(RGK_K_LIGHT_TRACE) += hl[RGK_CNT_QUEUE + k]; units(RGK_K_LIGHT_SHADE) += hl[RGK_CNT_HITS + k];
        units(RGK_K_LIGHT_SPLAT) += hl[RGK_CNT_SHADOW + k];
    }
    units(RGK_K_RESOLVE) += n0;
    // (light rays: the reference traces and counts one per path, path_tracer.cpp:126,349 -- the ones culled before the queue included)
    for (uint32_t k = 0; k < pp.reverse; k++) { c.path_rays += k == 0 ? n0 : hl[RGK_CNT_QUEUE + k]; c.shadow_rays += hl[RGK_CNT_SHADOW + k]; }
}

// The tiles checked against the frame, and their offsets into the pixel list they make (toff[n_tiles]: its length).  Host only.
// `what`: the caller's unit of work, for the error text.
int tile_offsets(const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, const char* what, std::vector<uint32_t>& toff) {
    toff.assign(n_tiles + 1, 0u);
    for (uint32_t i = 0; i < n_tiles; i++) {
        const rgk_tile& t = tiles[i];
        if (t.x1 > prm->xres || t.y1 > prm->yres || t.x0 > t.x1 || t.y0 > t.y1) return fail(RGK_ERR_INVALID, "tile %u outside the frame", i);
        const uint64_t n = (uint64_t)toff[i] + (uint64_t)(t.x1 - t.x0) * (t.y1 - t.y0);
        if (n >= (1ull << 31)) return fail(RGK_ERR_UNSUPPORTED, "more than 2^31 pixels in one %s", what);
        toff[i + 1] = (uint32_t)n;
    }
    return 0;
}
// ... and that list (toff[n_tiles] > 0 pixels) in Tracer::Render order with its per-pixel seeds (a1, a2), built on the device from
// the tile list.  A queued copy reads `toff`: the caller keeps it until it has synchronised the stream.
int queue_pixel_list(rgk_scene* s, const rgk_tile* tiles, uint32_t n_tiles, const std::vector<uint32_t>& toff) {
    const size_t P = toff[n_tiles];
    hipStream_t st = s->stream;
    int rc;
    if ((rc = s->pix_xy.alloc(P)) || (rc = s->pix_seed.alloc(P)) || (rc = s->tile_buf.alloc((size_t)n_tiles * 5 + n_tiles + 1))) return rc;
    static_assert(sizeof(rgk_tile) == 5 * sizeof(uint32_t), "rgk_tile layout");
    HIPCHK(hipMemcpyAsync(s->tile_buf.p, tiles, (size_t)n_tiles * sizeof(rgk_tile), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->tile_buf.p + (size_t)n_tiles * 5, toff.data(), (n_tiles + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    rgk_launch_build_pixel_list(st, reinterpret_cast<const rgk_tile*>(s->tile_buf.p), s->tile_buf.p + (size_t)n_tiles * 5, n_tiles, s->pix_xy.p, s->pix_seed.p);
    return 0;
}

// The round's pixel list and the camera rays' entry nodes per pixel group.  P: the round's pixels (0: nothing queued).  `toff`:
// see queue_pixel_list.
int prepare_round_lists(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles,
                        std::vector<uint32_t>& toff, size_t& P) {
    int rc;
    if ((rc = tile_offsets(prm, tiles, n_tiles, "round", toff))) return rc;
    P = toff[n_tiles];
    if (P == 0) return 0;
    if ((rc = queue_pixel_list(s, tiles, n_tiles, toff))) return rc;
    if (!s->tune.entry_points) { // (off: every camera ray starts at the root)
        s->entry.release(); s->entry_cap.release();
        return 0;
    }
    // the entry nodes depend on the camera and on which pixels the list holds in which order -- not on the seeds: a frame's
    // rounds share them (0.7 ms per round at 1080p otherwise)
    uint64_t key = 1469598103934665603ull;
    auto mix = [&key](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; i++) { key ^= b[i]; key *= 1099511628211ull; } };
    mix(camera, sizeof(*camera)); mix(&prm->xres, sizeof(prm->xres)); mix(&prm->yres, sizeof(prm->yres));
    for (uint32_t t = 0; t < n_tiles; t++) mix(&tiles[t], 4 * sizeof(uint32_t)); // x0, x1, y0, y1 (the seed is the fifth word)
    const size_t n_entry = ((size_t)P + RGK_ENTRY_PIX - 1) / RGK_ENTRY_PIX * RGK_ENTRY_K;
    if (s->entry.p && s->entry_n == n_entry && s->entry_key == key) return 0;
    if ((rc = s->entry.alloc(n_entry)) || (rc = s->entry_cap.alloc(n_entry / RGK_ENTRY_K + 1)) || (rc = s->trange.alloc((n_entry / RGK_ENTRY_K + 1) * 2))) return rc;
    DevCamera cam0;
    make_camera(camera, cam0);
    rgk_launch_entry_points(s->stream, s->dev, cam0, prm->xres, prm->yres, s->pix_xy.p, (uint32_t)P, 0u, (uint32_t)(n_entry / RGK_ENTRY_K), nullptr, s->entry.p, s->entry_cap.p);
    s->entry_key = key; s->entry_n = n_entry;
    s->entry_capped = 0; s->lentry_done = 0; // a new frame: capped / light-side lists are rebuilt as its first passes finish
    return 0;
}

// The pass plan: pixel ranges of npix_pass pixels x equal-sized sample passes of ns_pass samples, and the workspace for them.
// Paths per pass: what the card has room for now (an existing workspace counts as room); halved on an allocation failure.
int plan_passes(rgk_scene* s, const rgk_params* prm, size_t P, uint32_t R, RgkPassPlan& plan) {
    size_t B = batch_paths(s->tune, R);
    if (!s->tune.batch_paths && s->batch_reverse >= R) B = std::max(B, s->batch); // (an explicit batch size is taken literally)
    int rc;
    for (;;) {
        plan = rgk_plan_passes(P, prm->multisample, B);
        rc = ensure_workspace(s, plan.npix_pass * plan.ns_pass, R);
        if (rc != RGK_ERR_OOM || B <= ((size_t)1 << 20)) break;
        (void)hipGetLastError();
        B /= 2;
    }
    if (rc) return rc;
    return s->pixsum.alloc(P);
}

// Behind bounce 0's trace, once per frame and pixel range (later rounds and sample ranges reuse them): how far the first hits of
// each pixel group lie -> the camera rays' entry lists capped behind them, and where the group's shadow rays can go (light-side
// entry nodes and their boxes, which pp points to from here on).
int queue_first_hit_lists(rgk_scene* s, KernelLog& kl, const DevCamera& cam, PassParams& pp, uint32_t P, bool cap_entries, bool light_entry) {
    hipStream_t st = s->stream;
    const size_t end = (size_t)pp.j0 + pp.npix;
    const RgkGroupRange groups = rgk_group_range(pp.j0, pp.npix);
    const bool need_cap = cap_entries && end > s->entry_capped;
    const bool need_light = light_entry && end > s->lentry_done;
    int rc;
    if ((need_cap || need_light) && (rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_group_trange(st, pp, s->hit.p, s->trange.p); }))) return rc;
    if (need_cap) {
        if ((rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_entry_points(st, s->dev, cam, pp.xres, pp.yres, s->pix_xy.p, P, groups.first, groups.count(), s->trange.p, s->entry.p, s->entry_cap.p); })))
            return rc;
        s->entry_capped = end;
    }
    if (!light_entry) return 0;
    pp.lentry = s->lentry.p; pp.lbox = s->lbox.p;
    if (!need_light) return 0;
    if ((rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_light_entry_points(st, s->dev, cam, pp, P, s->trange.p, s->lentry.p, s->lbox.p); }))) return rc;
    s->lentry_done = end;
    if (s->tune.debug_bvh) { // how many pixel groups got light-side entry nodes below the root
        const size_t g0 = groups.first, g1 = groups.last;
        std::vector<int> he((g1 - g0) * RGK_ENTRY_K);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(he.data(), s->lentry.p + g0 * RGK_ENTRY_K, he.size() * sizeof(int), hipMemcpyDeviceToHost));
        size_t below = 0, total_e = 0;
        for (size_t g = 0; g < g1 - g0; g++) { if (he[g * RGK_ENTRY_K] != 0) below++; for (int k = 0; k < RGK_ENTRY_K; k++) total_e += he[g * RGK_ENTRY_K + k] != 0x7fffffff; }
        std::fprintf(stderr, "[rgk] light-side entry nodes: %zu of %zu pixel groups start below the root, %.2f entries per group\n", below, g1 - g0, (double)total_e / (double)(g1 - g0));
    }
    return 0;
}

// One pass, queued on the scene's stream: the light sub-path (reverse > 0), the camera path's bounces, the resolve into the
// accumulator, a progress mark behind every bounce (`stage`: the round's stages before this pass), and the copy of the pass's
// counter blocks into h_counters.
int queue_pass(rgk_scene* s, KernelLog& kl, const DevCamera& cam, PassParams& pp, size_t P, bool light_entry, bool const_light, float* d_accum_rgb,
               uint32_t* d_accum_count, uint32_t stage) {
    hipStream_t st = s->stream;
    const RgkTraceCfg& tc = s->tcfg;
    const bool count_stats = kl.count_stats, cap_entries = s->entry.p != nullptr && s->tune.entry_cap;
    const bool track = pp.depth > 12; // queue lengths read back (queue_len): measured, depth 10 loses 4 % to the read-backs, depth 40 gains 4 %
    const uint32_t R = pp.reverse, n0 = pp.npix * pp.ns;
    // the slot order, and the bundle walk for passes whose entry lists are not capped yet -- a frame's first round (rgk_plan.h)
    pp.gshift = rgk_plan_gshift(s->tune.sample_group, RGK_SAMPLE_GROUP_DEFAULT, pp.ns);
    pp.beam = rgk_beam_wanted(s->tune.beam, cap_entries && (size_t)pp.j0 + pp.npix <= s->entry_capped) ? 1u : 0u;
    float4* const rayA[2] = {s->rayA[0].p, s->rayA[1].p};
    float4* const rayB[2] = {s->rayB[0].p, s->rayB[1].p};
    float4 *const hit = s->hit.p, *const thr = s->thr.p, *const tot = s->tot.p, *const shA = s->shA.p, *const shB = s->shB.p, *const shC = s->shC.p;
    uint32_t* const cn = s->counters.p;      // camera-phase counters
    uint32_t* const cl = cn + RGK_CNT_TOTAL; // light-phase counters
    int rc;
    if (R > 0) {
        // light sub-path first (its sampler dimensions are fixed), splats straight into the accumulator
        if ((rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_init_counters(st, cl, 0u); })) || // (k_raygen_light queues the light rays that can touch the scene's box)
            (rc = kl.run(RGK_K_LIGHT_SHADE, [&] { rgk_launch_raygen_light(st, s->dev, cam, pp, rayA[0], rayB[0], thr, cl); })))
            return rc;
        for (uint32_t k = 0; k < R; k++) {
            const int q = k & 1;
            if ((rc = kl.run(RGK_K_LIGHT_TRACE, [&] { rgk_launch_trace_closest(st, s->dev, tc, count_stats, rayA[q], rayB[q], nullptr, hit, {n0, cl + RGK_CNT_QUEUE + k, cl + RGK_CNT_FETCH_T + k}, s->stats.p); })) ||
                (rc = kl.run(RGK_K_LIGHT_SHADE, [&] { rgk_launch_list_hits(st, hit, cl + RGK_CNT_QUEUE + k, s->hitlist.p, cl + RGK_CNT_HITS + k, n0); })) ||
                (rc = kl.run(RGK_K_LIGHT_SHADE, [&] { rgk_launch_shade_light(st, s->dev, cam, pp, k, rayA[q], rayB[q], hit, thr, rayA[q ^ 1], rayB[q ^ 1], shA, shB, shC, cl, n0); })) ||
                (rc = kl.run(RGK_K_LIGHT_SPLAT, [&] { rgk_launch_trace_shadow(st, s->dev, tc, count_stats, shA, shB, shC, nullptr, nullptr, RGK_SHADOW_SPLAT, d_accum_rgb,
                                                                              {n0, cl + RGK_CNT_SHADOW + k, cl + RGK_CNT_FETCH_S + k}, s->stats.p); })))
                return rc;
        }
    }
    // the camera path: the same pipeline for uni- and bidirectional rounds (R > 0: vertices with connections take the record
    // route -- k_shade<BDPT> -> k_connect -> k_trace_shadow_jobs -- beside the plain NEE rays)
    if ((rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_init_counters(st, cn, n0); }))) return rc;
    uint32_t ub = n0; // upper bound on bounce b's queues: every launch of the bounce sizes its grid by it
    for (uint32_t b = 0; b < pp.depth && ub > 0; b++) {
        const int q = b & 1;
        const RgkWalk wq = {ub, cn + RGK_CNT_QUEUE + b, cn + RGK_CNT_FETCH_T + b}, ws = {ub, cn + RGK_CNT_SHADOW + b, cn + RGK_CNT_FETCH_S + b};
        if (b == 0) // no ray queue at bounce 0: the camera ray of slot i is made where it is traced and shaded
            rc = kl.run(RGK_K_TRACE_CAMERA, [&] { rgk_launch_trace_camera(st, s->dev, cam, pp, tc, count_stats, hit, wq, s->stats.p); });
        else
            rc = kl.run(RGK_K_TRACE_CLOSEST, [&] { rgk_launch_trace_closest(st, s->dev, tc, count_stats, rayA[q], rayB[q], nullptr, hit, wq, s->stats.p); });
        if (rc || (b == 0 && (rc = queue_first_hit_lists(s, kl, cam, pp, (uint32_t)P, cap_entries, light_entry)))) return rc;
        if ((rc = kl.run(b == 0 ? RGK_K_SHADE_FIRST : RGK_K_SHADE, [&] { rgk_launch_shade(st, s->dev, cam, pp, b, rayA[q], rayB[q], hit, thr, tot, rayA[q ^ 1], rayB[q ^ 1], shA, shB, shC, cn, ub, R > 0, const_light); })) ||
            (R > 0 && (rc = kl.run(RGK_K_CONNECT, [&] { rgk_launch_connect(st, s->dev, pp, b, s->jobs.p, s->rads.p, cn, ub); }))))
            return rc;
        // (the constant-light route: the shading launches above left 32-byte records, shA = {d, far}, shB = {radiance, slot})
        const bool first = b == 0 && light_entry, rec32 = const_light && rgk_const_light_records();
        rc = kl.run(first ? RGK_K_SHADOW_FIRST : RGK_K_SHADOW, [&] {
            if (rec32 && first) rgk_launch_trace_shadow_first_cl(st, s->dev, pp, tc, count_stats, shA, shB, tot, ws, s->stats.p);
            else if (rec32) rgk_launch_trace_shadow_cl(st, s->dev, tc, count_stats, shA, shB, tot, ws, s->stats.p);
            else if (first) rgk_launch_trace_shadow_first(st, s->dev, pp, tc, count_stats, shA, shB, shC, tot, ws, s->stats.p);
            else rgk_launch_trace_shadow(st, s->dev, tc, count_stats, shA, shB, shC, tot, nullptr, RGK_SHADOW_ADD, nullptr, ws, s->stats.p);
        });
        // (the vertex queue after the plain rays: both add into the slot sums, a slot has a vertex in ONE of the two queues)
        if (rc || (R > 0 && (rc = kl.run(RGK_K_SHADOW_JOBS, [&] { rgk_launch_trace_shadow_jobs(st, s->dev, pp, tc, count_stats, s->jobs.p, s->rads.p, tot, {ub, cn + RGK_CNT_CONN + b, cn + RGK_CNT_FETCH_J + b}, s->stats.p); }))))
            return rc;
        rgk_launch_stage_mark(st, s->h_stage, stage + b + 1);
        if (track && b >= 3 && (b & 1) && b + 1 < pp.depth && (rc = queue_len(s, cn + RGK_CNT_QUEUE + b + 1, ub))) return rc;
    }
    if ((rc = kl.run(RGK_K_RESOLVE, [&] { rgk_launch_resolve(st, pp, tot, s->pixsum.p, d_accum_rgb, d_accum_count); }))) return rc;
    rgk_launch_stage_mark(st, s->h_stage, stage + std::max(1u, pp.depth)); // (all of the pass's stages: bounces that never ran count too)
    HIPCHK(hipMemcpyAsync(s->h_counters, cn, 2 * RGK_CNT_TOTAL * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return 0;
}
} // namespace

extern "C" {

int rgk_render_round_device(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles,
                            float* d_accum_rgb, uint32_t* d_accum_count, rgk_counters* counters) {
    if (!s || !camera || !prm || (!tiles && n_tiles) || !d_accum_rgb || !d_accum_count) return fail(RGK_ERR_INVALID, "null argument");
    if (int rc = check_frame_size(prm->xres, prm->yres)) return rc;
    if (prm->multisample == 0) return fail(RGK_ERR_INVALID, "multisample must be >= 1");
    if (prm->depth > RGK_MAX_DEPTH) return fail(RGK_ERR_UNSUPPORTED, "recursion depth %u > %d", prm->depth, RGK_MAX_DEPTH);
    if (prm->reverse > 7) return fail(RGK_ERR_UNSUPPORTED, "reverse %u > 7 light sub-path vertices", prm->reverse);
    if (prm->sampler != RGK_SAMPLER_HALTON) return fail(RGK_ERR_UNSUPPORTED, "the HIP path implements the Halton sampler only");
    HIPCHK(hipSetDevice(s->device));
    if (counters) std::memset(counters, 0, sizeof(*counters));
    std::vector<uint32_t> toff; // (read by a queued copy: it lives to the end of this call, which synchronises the stream before returning)
    size_t P = 0;
    RgkPassPlan plan{};
    int rc;
    if ((rc = prepare_round_lists(s, camera, prm, tiles, n_tiles, toff, P))) return rc;
    if (P == 0) return RGK_OK;
    // no light at all: TracePath builds no light sub-path (`reverse > 0 && valid light`), same as reverse == 0
    const uint32_t R = (s->dev.total_point_power + s->dev.total_areal_power > 0.0f) ? prm->reverse : 0u;
    if ((rc = plan_passes(s, prm, P, R, plan))) return rc;

    DevCamera cam;
    make_camera(camera, cam);
    HIPCHK(hipMemsetAsync(s->stats.p, 0, 8 * sizeof(unsigned long long), s->stream));
    KernelLog kl(s, prm->flags);
    // progress: one stage per bounce per pass; a one-thread kernel queued behind each bounce writes the stage number into pinned
    // host memory when the DEVICE gets there (a host function in the stream did the same but stalls the stream for a host
    // round trip per mark)
    const uint32_t pass_stages = std::max(1u, prm->depth);
    {
        const uint32_t n_pix_passes = (uint32_t)((P + plan.npix_pass - 1) / plan.npix_pass), n_s_passes = (prm->multisample + plan.ns_pass - 1) / plan.ns_pass;
        *(volatile uint32_t*)s->h_stage = 0; s->prog_stages = n_pix_passes * n_s_passes * pass_stages;
        s->prog_pixels = P; s->prog_paths = (uint64_t)P * prm->multisample; s->prog_busy = 1;
    }
    struct Done { rgk_scene* s; ~Done() { *(volatile uint32_t*)s->h_stage = s->prog_stages.load(); s->prog_busy = 0; } } done_guard{s};
    PassParams pp{};
    pp.multisample = prm->multisample; pp.depth = prm->depth; pp.xres = prm->xres; pp.yres = prm->yres;
    pp.clamp = prm->clamp; pp.russian = prm->russian; pp.bumpmap_scale = prm->bumpmap_scale; pp.reverse = R;
    pp.lstart = s->lstart.p; pp.lv = s->lv.p; pp.hitlist = s->hitlist.p; pp.lvmask = s->lvmask.p; pp.conn = s->conn.p; pp.connlist = s->connlist.p;
    pp.batch = (uint32_t)s->batch;
    pp.pix_xy = s->pix_xy.p; pp.pix_seed = s->pix_seed.p; pp.light = s->light.p; pp.generic = s->generic.p;
    pp.entry = s->entry.p; // (null when switched off; only the unidirectional bounce-0 launch reads it)
    pp.entry_cap = s->entry_cap.p;
    // one point / sphere light and nothing else that emits: every first-vertex shadow ray starts there (k_entry_points_light)
    const bool light_entry = s->entry.p && s->tune.light_entry && s->dev.n_pointlights == 1 && s->dev.n_areal == 0;
    // ... and if that light is provably every path's light, at its own position, a unidirectional round takes it as a constant
    const bool const_light = s->info.const_light == 1 && s->tune.const_light && R == 0;
    if (light_entry) {
        const size_t groups = ((size_t)P + RGK_ENTRY_PIX - 1) / RGK_ENTRY_PIX + 1;
        if ((rc = s->lentry.alloc(groups * RGK_ENTRY_K)) || (rc = s->trange.alloc(groups * 2)) || (rc = s->lbox.alloc(groups * 2))) return rc;
    }
    if ((rc = s->htab.alloc((size_t)192 * prm->multisample))) return rc;
    if ((rc = kl.run(RGK_K_OTHER, [&] { rgk_launch_build_halton_table(s->stream, s->dev, prm->multisample, s->htab.p); }))) return rc;
    pp.htab = s->htab.p;

    rgk_counters tot{};
    uint32_t stage = 0; // progress stages of the passes before this one
    for (size_t j0 = 0; j0 < P; j0 += plan.npix_pass) {
        pp.j0 = (uint32_t)j0;
        pp.npix = (uint32_t)std::min(plan.npix_pass, P - j0);
        for (uint32_t s0 = 0; s0 < prm->multisample; s0 += plan.ns_pass, stage += pass_stages) {
            pp.s0 = s0;
            pp.ns = std::min(plan.ns_pass, prm->multisample - s0);
            if ((rc = queue_pass(s, kl, cam, pp, P, light_entry, const_light, d_accum_rgb, d_accum_count, stage))) return rc;
            HIPCHK(hipStreamSynchronize(s->stream));
            add_pass_counters(s->h_counters, pp, light_entry, tot);
        }
    }
    HIPCHK(hipGetLastError());
    s->prog_rounds++;
    if (counters) {
        tot.paths = (uint64_t)P * prm->multisample;
        if (kl.count_stats) {
            unsigned long long h[8];
            if ((rc = read_stats(s, h))) return rc;
            tot.node_visits = h[0]; tot.tri_tests = h[1]; tot.shadow_node_visits = h[2]; tot.shadow_tri_tests = h[3];
        }
        if ((rc = kl.fold(tot))) return rc;
        *counters = tot;
    }
    return RGK_OK;
}

int rgk_render_round(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles,
                     float* accum_rgb, uint32_t* accum_count, rgk_counters* counters) {
    if (!s || !prm || !accum_rgb || !accum_count) return fail(RGK_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(s->device));
    const size_t P = (size_t)prm->xres * prm->yres;
    DevBuf<float> d_rgb;
    DevBuf<uint32_t> d_cnt;
    int rc;
    if ((rc = d_rgb.upload(accum_rgb, 3 * P)) || (rc = d_cnt.upload(accum_count, P))) return rc;
    if ((rc = rgk_render_round_device(s, camera, prm, tiles, n_tiles, d_rgb.p, d_cnt.p, counters))) return rc;
    if ((rc = down(accum_rgb, d_rgb, 3 * P)) || (rc = down(accum_count, d_cnt, P))) return rc;
    return RGK_OK;
}

int rgk_trace_closest(rgk_scene* s, uint32_t n, const float* rays, const int32_t* ignore, rgk_hit* hits, rgk_counters* counters) {
    if (!s || (!rays && n) || (!hits && n)) return fail(RGK_ERR_INVALID, "null argument");
    if (counters) std::memset(counters, 0, sizeof(*counters));
    if (n == 0) return RGK_OK;
    HIPCHK(hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_workspace(s, n)) || (rc = s->nearfar.alloc(n)) || (rc = s->scratch_f.alloc((size_t)8 * n)) || (rc = s->scratch_u.alloc((size_t)5 * n)))
        return rc;
    hipStream_t st = s->stream;
    HIPCHK(hipMemcpyAsync(s->scratch_f.p, rays, (size_t)8 * n * sizeof(float), hipMemcpyHostToDevice, st));
    int32_t* d_ign = nullptr;
    if (ignore) {
        d_ign = (int32_t*)s->scratch_u.p;
        HIPCHK(hipMemcpyAsync(d_ign, ignore, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemsetAsync(s->stats.p, 0, 8 * sizeof(unsigned long long), st));
    rgk_launch_init_counters(st, s->counters.p, n);
    rgk_launch_pack_rays(st, n, s->scratch_f.p, d_ign, s->rayA[0].p, s->rayB[0].p, s->nearfar.p);
    const RgkWalk w = {n, s->counters.p + RGK_CNT_QUEUE, s->counters.p + RGK_CNT_FETCH_T};
    hipEvent_t e0 = nullptr, e1 = nullptr; // kernel time of the traversal alone, for counters->ms_trace
    if (counters) {
        if ((rc = scene_event(s, 0, e0)) || (rc = scene_event(s, 1, e1))) return rc;
        HIPCHK(hipEventRecord(e0, st));
    }
    rgk_launch_trace_closest(st, s->dev, s->tcfg, false, s->rayA[0].p, s->rayB[0].p, s->nearfar.p, s->hit.p, w, s->stats.p);
    if (counters) {
        HIPCHK(hipEventRecord(e1, st));
        // the counting variant runs separately so that the timed launch is the kernel a round runs
        rgk_launch_init_counters(st, s->counters.p, n);
        rgk_launch_trace_closest(st, s->dev, s->tcfg, true, s->rayA[0].p, s->rayB[0].p, s->nearfar.p, s->hit.p, w, s->stats.p);
    }
    rgk_hit* d_hits = (rgk_hit*)s->scratch_u.p; // 5 dwords per hit; reuses the ignore buffer after the trace
    rgk_launch_unpack_hits(st, n, s->hit.p, d_hits);
    HIPCHK(hipMemcpyAsync(hits, d_hits, (size_t)n * sizeof(rgk_hit), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (counters) {
        unsigned long long h[8];
        if ((rc = read_stats(s, h))) return rc;
        counters->node_visits = h[0]; counters->tri_tests = h[1]; counters->path_rays = n;
        if (s->tune.debug_util) // lane occupancy per phase of the walker: lane-visits / (64 x wave iterations)
            std::fprintf(stderr, "[rgk util] rays %u  node visits %llu in %llu wave iterations (%.3f of lanes)  triangle tests %llu in %llu (%.3f)  outer iterations %llu  refills %llu\n",
                         n, h[0], h[4], h[4] ? (double)h[0] / (64.0 * (double)h[4]) : 0.0, h[1], h[5], h[5] ? (double)h[1] / (64.0 * (double)h[5]) : 0.0, h[6], h[7]);
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        counters->ms_trace = ms; counters->n_trace_launches = 1;
    }
    return RGK_OK;
}

int rgk_trace_visibility(rgk_scene* s, uint32_t n, const float* a, const float* b, uint8_t* visible, rgk_counters* counters) {
    if (!s || (n && (!a || !b || !visible))) return fail(RGK_ERR_INVALID, "null argument");
    if (counters) std::memset(counters, 0, sizeof(*counters));
    if (n == 0) return RGK_OK;
    HIPCHK(hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_workspace(s, n)) || (rc = s->scratch_f.alloc((size_t)6 * n)) || (rc = s->scratch_u.alloc(n))) return rc;
    hipStream_t st = s->stream;
    HIPCHK(hipMemcpyAsync(s->scratch_f.p, a, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->scratch_f.p + (size_t)3 * n, b, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(s->stats.p, 0, 8 * sizeof(unsigned long long), st));
    rgk_launch_init_counters(st, s->counters.p, n);
    rgk_launch_pack_visibility(st, s->dev, n, s->scratch_f.p, s->scratch_f.p + (size_t)3 * n, s->shA.p, s->shB.p, s->shC.p);
    rgk_launch_trace_shadow(st, s->dev, s->tcfg, counters != nullptr, s->shA.p, s->shB.p, s->shC.p, s->tot.p, (uint8_t*)s->scratch_u.p,
                            RGK_SHADOW_ADD, nullptr, {n, s->counters.p + RGK_CNT_QUEUE, s->counters.p + RGK_CNT_FETCH_S}, s->stats.p);
    HIPCHK(hipMemcpyAsync(visible, s->scratch_u.p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (counters) {
        unsigned long long h[8];
        if ((rc = read_stats(s, h))) return rc;
        counters->shadow_node_visits = h[2]; counters->shadow_tri_tests = h[3]; counters->shadow_rays = n;
    }
    return RGK_OK;
}

int rgk_bxdf_value(rgk_scene* s, uint32_t n, uint32_t route, const uint32_t* mat, const float* Vi, const float* Vr, const float* uv, float* out_rgb) {
    if (!s || (n && (!mat || !Vi || !Vr || !uv || !out_rgb))) return fail(RGK_ERR_INVALID, "null argument");
    if (n == 0) return RGK_OK;
    for (uint32_t i = 0; i < n; i++) if (mat[i] >= s->n_materials) return fail(RGK_ERR_INVALID, "material index out of range");
    HIPCHK(hipSetDevice(s->device));
    DevBuf<uint32_t> dm; DevBuf<float> dvi, dvr, duv, dout;
    int rc;
    if ((rc = dm.upload(mat, n)) || (rc = dvi.upload(Vi, (size_t)3 * n)) || (rc = dvr.upload(Vr, (size_t)3 * n)) || (rc = duv.upload(uv, (size_t)2 * n)) || (rc = dout.alloc((size_t)3 * n)))
        return rc;
    rgk_launch_bxdf_value(s->stream, s->dev, n, route, dm.p, dvi.p, dvr.p, duv.p, dout.p);
    if (hipStreamSynchronize(s->stream) != hipSuccess) return fail(RGK_ERR_DEVICE, "bxdf value kernel failed");
    return down(out_rgb, dout, (size_t)3 * n);
}

int rgk_bxdf_sample(rgk_scene* s, uint32_t n, uint32_t route, const uint32_t* mat, const float* Vi, const float* uv, const float* u, float* out_dir,
                    float* out_weight, uint8_t* may_leak) {
    if (!s || (n && (!mat || !Vi || !uv || !u || !out_dir || !out_weight || !may_leak))) return fail(RGK_ERR_INVALID, "null argument");
    if (n == 0) return RGK_OK;
    for (uint32_t i = 0; i < n; i++) if (mat[i] >= s->n_materials) return fail(RGK_ERR_INVALID, "material index out of range");
    HIPCHK(hipSetDevice(s->device));
    DevBuf<uint32_t> dm; DevBuf<float> dvi, duv, du, dd, dw; DevBuf<uint8_t> dl;
    int rc;
    if ((rc = dm.upload(mat, n)) || (rc = dvi.upload(Vi, (size_t)3 * n)) || (rc = duv.upload(uv, (size_t)2 * n)) || (rc = du.upload(u, (size_t)2 * n)) ||
        (rc = dd.alloc((size_t)3 * n)) || (rc = dw.alloc((size_t)3 * n)) || (rc = dl.alloc(n)))
        return rc;
    rgk_launch_bxdf_sample(s->stream, s->dev, n, route, dm.p, dvi.p, duv.p, du.p, dd.p, dw.p, dl.p);
    if (hipStreamSynchronize(s->stream) != hipSuccess) return fail(RGK_ERR_DEVICE, "bxdf sample kernel failed");
    if ((rc = down(out_dir, dd, (size_t)3 * n)) || (rc = down(out_weight, dw, (size_t)3 * n))) return rc;
    return down(may_leak, dl, n);
}

int rgk_texture_sample(rgk_scene* s, uint32_t n, const int32_t* tex, const float* uv, float* rgb, float* slope_right, float* slope_bottom) {
    if (!s || (n && (!tex || !uv || !rgb || !slope_right || !slope_bottom))) return fail(RGK_ERR_INVALID, "null argument");
    if (n == 0) return RGK_OK;
    for (uint32_t i = 0; i < n; i++) if (tex[i] >= (int32_t)s->n_textures) return fail(RGK_ERR_INVALID, "texture index out of range");
    HIPCHK(hipSetDevice(s->device));
    DevBuf<int32_t> dt; DevBuf<float> duv, drgb, dr, db;
    int rc;
    if ((rc = dt.upload(tex, n)) || (rc = duv.upload(uv, (size_t)2 * n)) || (rc = drgb.alloc((size_t)3 * n)) || (rc = dr.alloc(n)) || (rc = db.alloc(n))) return rc;
    rgk_launch_texture_sample(s->stream, s->dev, n, s->texrefs.p, dt.p, duv.p, drgb.p, dr.p, db.p);
    if (hipStreamSynchronize(s->stream) != hipSuccess) return fail(RGK_ERR_DEVICE, "texture sample kernel failed");
    if ((rc = down(rgb, drgb, (size_t)3 * n)) || (rc = down(slope_right, dr, n))) return rc;
    return down(slope_bottom, db, n);
}

int rgk_libm_eval(int fn, uint32_t n, const float* a, const float* b, float* out) {
    if (n && (!a || !out || (fn == 4 && !b))) return fail(RGK_ERR_INVALID, "null argument");
    if (fn < 0 || fn > 4) return fail(RGK_ERR_INVALID, "unknown function");
    if (n == 0) return RGK_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RGK_ERR_NO_DEVICE, "no HIP device visible");
    DevBuf<float> da, db, dout;
    int rc;
    if ((rc = da.upload(a, n)) || (rc = db.upload(b ? b : a, n)) || (rc = dout.alloc(n))) return rc;
    rgk_launch_libm_eval(nullptr, fn, n, da.p, db.p, dout.p);
    return down(out, dout, n);
}

int rgk_sampler_eval(uint32_t n, const uint32_t* seed, const uint32_t* index, const uint32_t* dim, int is2d, float* out) {
    if (n && (!seed || !index || !dim || !out)) return fail(RGK_ERR_INVALID, "null argument");
    if (n == 0) return RGK_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RGK_ERR_NO_DEVICE, "no HIP device visible");
    std::vector<DevHaltonDim> hd;
    std::vector<uint16_t> hp;
    build_halton(hd, hp);
    DevBuf<DevHaltonDim> dh;
    DevBuf<uint16_t> dp;
    DevBuf<uint32_t> ds_, di, dd;
    DevBuf<float> dout;
    int rc;
    if ((rc = dh.upload(hd.data(), hd.size())) || (rc = dp.upload(hp.data(), hp.size())) || (rc = ds_.upload(seed, n)) || (rc = di.upload(index, n)) ||
        (rc = dd.upload(dim, n)) || (rc = dout.alloc((size_t)2 * n)))
        return rc;
    DevScene sc{};
    sc.hdims = dh.p; sc.hperm = dp.p;
    rgk_launch_sampler_eval(nullptr, sc, n, ds_.p, di.p, dd.p, is2d, dout.p);
    hipError_t e = hipMemcpy(out, dout.p, (size_t)2 * n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RGK_ERR_DEVICE, "sampler eval: %s", hipGetErrorString(e));
    return RGK_OK;
}

} // extern "C"

// ------------------------------------------------------------------ feature buffers and the denoiser (kernels: rgk_post.hip)
namespace {
// HIP events (the scene's pool, from its first) around the launches of one post call, when the scene's "time_post" switch is on.
struct PostTimer {
    rgk_scene* s;
    size_t n = 0; // marks so far
    int mark() { // between two launches
        if (!s->tune.time_post) return 0;
        hipEvent_t e;
        if (int rc = scene_event(s, n, e)) return rc;
        n++;
        HIPCHK(hipEventRecord(e, s->stream));
        return 0;
    }
    int fold(std::vector<double>& out) const { // after the stream has been waited for
        out.clear();
        for (size_t i = 0; i + 1 < n; i++) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, s->events[i], s->events[i + 1]));
            out.push_back(ms);
        }
        return 0;
    }
};

// A post call once the entry's own argument checks have passed: refused while a round is in flight; the slot's old times go; with no
// `work` to do that is all, and the device is not touched.  Else body(tm) -- the entry's allocations and its launches on the scene's
// stream, tm.mark() between them -- then a wait for the stream, and the launch times go into the slot.
template <class Body>
int post_call(rgk_scene* s, const char* entry, PostSlot slot, bool work, Body&& body) {
    if (s->prog_busy.load()) return fail(RGK_ERR_INVALID, "%s while a round is in flight on this scene", entry);
    s->post_ms[slot].clear();
    if (!work) return RGK_OK;
    HIPCHK(hipSetDevice(s->device));
    PostTimer tm{s};
    if (int rc = body(tm)) return rc;
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipGetLastError());
    return tm.fold(s->post_ms[slot]);
}

// (every check before the scene or the device is touched; `toff`: tile_offsets)
int check_aov_args(const rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, std::vector<uint32_t>& toff) {
    if (!s || !camera || !prm || (!tiles && n_tiles)) return fail(RGK_ERR_INVALID, "null argument");
    if (int rc = check_frame_size(prm->xres, prm->yres)) return rc;
    return tile_offsets(prm, tiles, n_tiles, "feature pass", toff);
}
// What both denoise entries check besides their own parameter ranges, without touching the scene.  The fixed-sigma filter has no
// half-buffer and no variance plane (NULL here); `p`: its parameters too, with albedo_floor 0 (sigma_k belongs to the entry).
int check_denoise_args(const rgk_scene* s, uint32_t xres, uint32_t yres, const float* accum_rgb, const uint32_t* accum_count, const float* half_rgb,
                       const uint32_t* half_count, const float* albedo, const float* normal, const float* depth, const rgk_denoise_var_params& p,
                       const float* out_rgb, const float* out_variance) {
    if (!s || !accum_rgb || !accum_count || !normal || !depth || !out_rgb) return fail(RGK_ERR_INVALID, "null argument");
    if (p.demodulate && !albedo) return fail(RGK_ERR_INVALID, "demodulate without an albedo plane");
    if (int rc = check_frame_size(xres, yres)) return rc;
    if (p.iterations > 16 || p.normal_power_log2 > 16) return fail(RGK_ERR_INVALID, "iterations and normal_power_log2 must be <= 16");
    const void* ins[] = {accum_rgb, accum_count, half_rgb, half_count, albedo, normal, depth};
    for (const void* in : ins)
        if (in && (in == out_rgb || in == out_variance)) return fail(RGK_ERR_INVALID, "an output plane must not be one of the inputs");
    if (out_rgb == out_variance) return fail(RGK_ERR_INVALID, "out_rgb and out_variance must differ");
    return RGK_OK;
}
// A whole denoise call once the entry's own checks have passed: the shared ones, then prepare -> [prefilter] -> iterations -> finish ->
// [variance copy] on the scene's stream, waited for.  `wc[i]`: iteration i's colour-weight constant (sigma_i^2 / sigma_k^2).
int denoise(rgk_scene* s, const char* entry, PostSlot slot, uint32_t xres, uint32_t yres, const float* accum_rgb, const uint32_t* accum_count, const float* half_rgb,
            const uint32_t* half_count, const float* albedo, const float* normal, const float* depth, const rgk_denoise_var_params& p, const float* wc,
            float* out_rgb, float* out_variance) {
    int rc;
    if ((rc = check_denoise_args(s, xres, yres, accum_rgb, accum_count, half_rgb, half_count, albedo, normal, depth, p, out_rgb, out_variance))) return rc;
    return post_call(s, entry, slot, true, [&](PostTimer& tm) -> int {
        const size_t P = (size_t)xres * yres;
        const uint32_t it = p.iterations, demod = (it && p.demodulate) ? 1u : 0u; // no iteration: out = c, variance = v, nothing to demodulate for
        const RgkDnMode mode = half_rgb ? RGK_DN_VARIANCE_GUIDED : RGK_DN_FIXED_SIGMA;
        if ((rc = s->dn_col[0].alloc(P)) || (it && ((rc = s->dn_col[1].alloc(P)) || (rc = s->dn_guide.alloc(P))))) return rc;
        hipStream_t st = s->stream;
        uint32_t cur = 0; // the plane that holds the current image
        const auto filter = [&](RgkDnMode m, uint32_t step, float c) {
            rgk_launch_dn_atrous(st, m, xres, yres, step, c, p.sigma_depth, p.normal_power_log2, s->dn_guide.p, s->dn_col[cur].p, s->dn_col[cur ^ 1u].p);
            cur ^= 1u;
            return tm.mark();
        };
        if ((rc = tm.mark())) return rc;
        rgk_launch_dn_prepare(st, P, accum_rgb, accum_count, half_rgb, half_count, albedo, normal, depth, demod, p.albedo_floor, s->dn_col[0].p, it ? s->dn_guide.p : nullptr);
        if ((rc = tm.mark())) return rc;
        if (it && mode == RGK_DN_VARIANCE_GUIDED && (rc = filter(RGK_DN_VARIANCE_MEAN, 1u, 0.0f))) return rc;
        for (uint32_t i = 0; i < it; i++)
            if ((rc = filter(mode, 1u << i, wc[i]))) return rc;
        rgk_launch_dn_finish(st, P, s->dn_col[cur].p, albedo, demod, p.albedo_floor, out_rgb);
        if ((rc = tm.mark())) return rc;
        if (!out_variance) return 0;
        rgk_launch_nz_finish(st, P, s->dn_col[cur].p, out_variance);
        return tm.mark();
    });
}
} // namespace

extern "C" {

int rgk_render_aov_device(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, float* d_albedo,
                          float* d_normal, float* d_depth, int32_t* d_tri) {
    int rc;
    std::vector<uint32_t> toff; // (read by a queued copy: lives until the stream has been waited for)
    if ((rc = check_aov_args(s, camera, prm, tiles, n_tiles, toff))) return rc;
    const uint32_t n = toff[n_tiles];
    return post_call(s, "rgk_render_aov_device", POST_AOV, n != 0, [&](PostTimer& tm) -> int {
        // The round's own buffers: its pixel list (rebuilt by every round before it is read), two ray planes and the hit plane of
        // the workspace (written by every pass before they are read).  The frame's cached lists -- entry nodes, their caps, the
        // light-side entries -- are neither read nor written here, so the rounds of a frame compute the same with or without this call.
        if ((rc = ensure_workspace(s, n))) return rc;
        hipStream_t st = s->stream;
        DevCamera cam;
        make_camera(camera, cam);
        cam.lens_size = 0.0f; // every feature ray leaves from the camera's origin
        if ((rc = tm.mark()) || (rc = queue_pixel_list(s, tiles, n_tiles, toff))) return rc;
        rgk_launch_init_counters(st, s->counters.p, n);
        rgk_launch_aov_raygen(st, cam, prm->xres, prm->yres, s->pix_xy.p, n, s->rayA[0].p, s->rayB[0].p);
        if ((rc = tm.mark())) return rc;
        rgk_launch_trace_closest(st, s->dev, s->tcfg, false, s->rayA[0].p, s->rayB[0].p, nullptr, s->hit.p, {n, s->counters.p + RGK_CNT_QUEUE, s->counters.p + RGK_CNT_FETCH_T}, s->stats.p);
        if ((rc = tm.mark())) return rc;
        rgk_launch_aov_gather(st, s->dev, prm->bumpmap_scale, prm->xres, s->pix_xy.p, n, s->rayA[0].p, s->rayB[0].p, s->hit.p, d_albedo, d_normal, d_depth, d_tri);
        return tm.mark();
    });
}

int rgk_render_aov(rgk_scene* s, const rgk_camera* camera, const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, float* albedo, float* normal,
                   float* depth, int32_t* tri) {
    int rc;
    std::vector<uint32_t> toff;
    if ((rc = check_aov_args(s, camera, prm, tiles, n_tiles, toff))) return rc;
    HIPCHK(hipSetDevice(s->device));
    const size_t P = (size_t)prm->xres * prm->yres;
    DevBuf<float> d_alb, d_nrm, d_z;
    DevBuf<int32_t> d_tri;
    // (the planes go up first: pixels outside the tiles keep what the caller had there)
    if ((albedo && (rc = d_alb.upload(albedo, 3 * P))) || (normal && (rc = d_nrm.upload(normal, 3 * P))) || (depth && (rc = d_z.upload(depth, P))) || (tri && (rc = d_tri.upload(tri, P))))
        return rc;
    if ((rc = rgk_render_aov_device(s, camera, prm, tiles, n_tiles, albedo ? d_alb.p : nullptr, normal ? d_nrm.p : nullptr, depth ? d_z.p : nullptr, tri ? d_tri.p : nullptr))) return rc;
    if ((albedo && (rc = down(albedo, d_alb, 3 * P))) || (normal && (rc = down(normal, d_nrm, 3 * P))) || (depth && (rc = down(depth, d_z, P))) || (tri && (rc = down(tri, d_tri, P)))) return rc;
    return RGK_OK;
}

int rgk_denoise_device(rgk_scene* s, uint32_t xres, uint32_t yres, const float* d_accum_rgb, const uint32_t* d_accum_count, const float* d_albedo,
                       const float* d_normal, const float* d_depth, const rgk_denoise_params* dp, float* d_out_rgb) {
    if (!dp) return fail(RGK_ERR_INVALID, "null argument");
    if (!(dp->sigma_color > 0.0f) || !(dp->sigma_depth >= 0.0f) || std::isinf(dp->sigma_color) || std::isinf(dp->sigma_depth)) return fail(RGK_ERR_INVALID, "sigma_color must be > 0 and sigma_depth >= 0, both finite");
    float sigma2[16];
    for (uint32_t i = 0; i < dp->iterations && i < 16; i++) { // (iterations <= 16 is checked with what both entries share)
        const float si = dp->sigma_color * std::ldexp(1.0f, -(int)i); // sigma_color * 2^-i
        sigma2[i] = si * si;
        if (!(sigma2[i] > 0.0f) || std::isinf(sigma2[i])) return fail(RGK_ERR_INVALID, "sigma_color^2 leaves the float range at iteration %u", i);
    }
    const rgk_denoise_var_params p = {dp->iterations, 0.0f, dp->sigma_depth, dp->normal_power_log2, dp->demodulate, 0.0f};
    return denoise(s, "rgk_denoise_device", POST_DENOISE, xres, yres, d_accum_rgb, d_accum_count, nullptr, nullptr, d_albedo, d_normal, d_depth, p, sigma2, d_out_rgb, nullptr);
}

int rgk_noise_estimate_device(rgk_scene* s, uint32_t xres, uint32_t yres, uint32_t tile_size, const float* d_accum_rgb, const uint32_t* d_accum_count,
                              const float* d_half_rgb, const uint32_t* d_half_count, rgk_noise_tile* tiles, float* d_variance) {
    // (every check before the scene or the device is touched)
    if (!s || !d_accum_rgb || !d_accum_count || !d_half_rgb || !d_half_count || !tiles) return fail(RGK_ERR_INVALID, "null argument");
    if (int rc = check_frame_size(xres, yres)) return rc;
    if (tile_size == 0) return fail(RGK_ERR_INVALID, "tile_size must be >= 1");
    if (d_variance && (d_variance == d_accum_rgb || d_variance == d_half_rgb || (const void*)d_variance == d_accum_count || (const void*)d_variance == d_half_count))
        return fail(RGK_ERR_INVALID, "variance must not be one of the inputs");
    if (d_half_rgb == d_accum_rgb || d_half_count == d_accum_count) return fail(RGK_ERR_INVALID, "the half-buffer must not be the accumulator");
    const RgkGrid2 g = rgk_nz_tile_grid(xres, yres, tile_size);
    const int rc = post_call(s, "rgk_noise_estimate_device", POST_NOISE, true, [&](PostTimer& tm) -> int {
        int rc;
        if ((rc = s->nz_tiles.alloc(g.count())) || (rc = tm.mark())) return rc;
        rgk_launch_nz_tile_sums(s->stream, xres, yres, tile_size, d_accum_rgb, d_accum_count, d_half_rgb, d_half_count, s->nz_tiles.p, d_variance);
        return tm.mark();
    });
    return rc ? rc : down(tiles, s->nz_tiles, g.count());
}

int rgk_denoise_variance_device(rgk_scene* s, uint32_t xres, uint32_t yres, const float* d_accum_rgb, const uint32_t* d_accum_count, const float* d_half_rgb,
                                const uint32_t* d_half_count, const float* d_albedo, const float* d_normal, const float* d_depth,
                                const rgk_denoise_var_params* dp, float* d_out_rgb, float* d_out_variance) {
    if (!dp || !d_half_rgb || !d_half_count) return fail(RGK_ERR_INVALID, "null argument");
    if (!(dp->sigma_k > 0.0f) || !(dp->sigma_depth >= 0.0f) || !(dp->albedo_floor >= 0.0f) || std::isinf(dp->sigma_k) || std::isinf(dp->sigma_depth) || std::isinf(dp->albedo_floor))
        return fail(RGK_ERR_INVALID, "sigma_k must be > 0, sigma_depth and albedo_floor >= 0, all finite");
    float k2[16];
    std::fill(k2, k2 + 16, dp->sigma_k * dp->sigma_k);
    if (!(k2[0] > 0.0f) || std::isinf(k2[0])) return fail(RGK_ERR_INVALID, "sigma_k^2 leaves the float range");
    if (d_half_rgb == d_accum_rgb || d_half_count == d_accum_count) return fail(RGK_ERR_INVALID, "the half-buffer must not be the accumulator");
    return denoise(s, "rgk_denoise_variance_device", POST_DENOISE_VARIANCE, xres, yres, d_accum_rgb, d_accum_count, d_half_rgb, d_half_count, d_albedo, d_normal, d_depth,
                   *dp, k2, d_out_rgb, d_out_variance);
}

int rgk_adapt_select(const rgk_noise_tile* tiles, const uint32_t* visits, uint32_t xres, uint32_t yres, uint32_t tile_size, const rgk_adapt_params* prm,
                     uint8_t* live, uint32_t* n_live, uint32_t* done) {
    if (const char* why = rgk_adapt_check(tiles, visits, xres, yres, tile_size, prm, live)) return fail(RGK_ERR_INVALID, "rgk_adapt_select: %s", why);
    const RgkAdaptResult r = rgk_adapt_rule(tiles, visits, xres, yres, tile_size, *prm, live);
    if (n_live) *n_live = r.n_live;
    if (done) *done = r.done ? 1u : 0u;
    return RGK_OK;
}

int rgk_round_fold_device(rgk_scene* s, uint32_t xres, uint32_t yres, const rgk_tile* tiles, uint32_t n_tiles, const uint8_t* to_half, float* d_round_rgb,
                          uint32_t* d_round_count, float* d_total_rgb, uint32_t* d_total_count, float* d_half_rgb, uint32_t* d_half_count) {
    // (every check before the scene or the device is touched)
    if (!s || (n_tiles && (!tiles || !to_half)) || !d_round_rgb || !d_round_count || !d_total_rgb || !d_total_count || !d_half_rgb || !d_half_count)
        return fail(RGK_ERR_INVALID, "null argument");
    if (int rc = check_frame_size(xres, yres)) return rc;
    const void* planes[6] = {d_round_rgb, d_round_count, d_total_rgb, d_total_count, d_half_rgb, d_half_count};
    for (int i = 0; i < 6; i++)
        for (int j = i + 1; j < 6; j++)
            if (planes[i] == planes[j]) return fail(RGK_ERR_INVALID, "the six planes must be six different buffers");
    uint32_t max_height = 0, bad = 0;
    if (const char* why = rgk_fold_check_tiles(tiles, n_tiles, xres, yres, max_height, bad)) return fail(RGK_ERR_INVALID, "round fold: %s (tile %u)", why, bad);
    return post_call(s, "rgk_round_fold_device", POST_FOLD, n_tiles != 0, [&](PostTimer& tm) -> int {
        int rc;
        static_assert(sizeof(rgk_tile) == 5 * sizeof(uint32_t), "rgk_tile layout");
        if ((rc = s->fold_buf.alloc((size_t)n_tiles * 5 + (n_tiles + 3u) / 4u)) || (rc = tm.mark())) return rc;
        hipStream_t st = s->stream;
        // (queued copies of the caller's arrays: they are the caller's until this call returns, and it waits for the stream first)
        uint8_t* d_flags = reinterpret_cast<uint8_t*>(s->fold_buf.p + (size_t)n_tiles * 5);
        HIPCHK(hipMemcpyAsync(s->fold_buf.p, tiles, (size_t)n_tiles * sizeof(rgk_tile), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_flags, to_half, n_tiles, hipMemcpyHostToDevice, st));
        if ((rc = tm.mark())) return rc;
        rgk_launch_round_fold(st, xres, reinterpret_cast<const rgk_tile*>(s->fold_buf.p), d_flags, n_tiles, max_height, d_round_rgb, d_round_count, d_total_rgb,
                              d_total_count, d_half_rgb, d_half_count);
        return tm.mark();
    });
}

int rgk_scene_get_post_timing(const rgk_scene* s, uint32_t which, double* ms, uint32_t* n) {
    if (!s || !n || which >= POST_SLOTS || (!ms && *n)) return fail(RGK_ERR_INVALID, "bad argument");
    if (s->magic != RGK_SCENE_MAGIC) return fail(RGK_ERR_INVALID, "not a live scene handle");
    const std::vector<double>& v = s->post_ms[which];
    for (uint32_t i = 0; i < *n && i < v.size(); i++) ms[i] = v[i];
    *n = (uint32_t)v.size();
    return RGK_OK;
}

} // extern "C"
