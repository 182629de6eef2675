// What the host files behind the C ABI of include/rgk.h share: the scene object and the few helpers more than one of them needs.
//   rgk_scene.cpp      create / refit / tuning / progress, the workspace, task list and camera
//   rgk_round.cpp      the round driver (rgk_render_round[_device])
//   rgk_probe.cpp      the unit-level entries the parity tests call
//   rgk_post_host.cpp  feature pass, denoisers, noise estimate, round fold, temporal reuse, upsampling, display output, output files
// The arithmetic that needs no device is in rgk_round_plan.h, rgk_plan.h, rgk_adapt.h and rgk_commit.h.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/rgk.h"
#include "device_types.h"
#include "rgk_commit.h" // fail
#include "rgk_kernels.h"
#include "rgk_poison.h"
#include "rgk_round_plan.h"

#pragma GCC visibility push(hidden) // shared between the host files, not exports of the library (popped at the end)

#define HIPCHK(x)                                                                                    \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess)                                                                         \
            return fail(e_ == hipErrorOutOfMemory ? RGK_ERR_OOM : RGK_ERR_DEVICE, "%s: %s (%s:%d)", #x, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                   \
    } while (0)

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
        rgk_poison_fill(p, count * sizeof(T)); // RGK_POISON=1: 0xFF bytes (rgk_poison.h)
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

template <typename T>
int down(T* dst, const DevBuf<T>& b, size_t count) {
    if (hipMemcpy(dst, b.p, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return fail(RGK_ERR_DEVICE, "hipMemcpy D2H failed");
    return 0;
}

// Tuning switches of one scene (nothing here changes a result).  Filled ONCE, by read_tuning in rgk_scene_create, from the
// environment (RGK_ENTRY_POINTS, RGK_ENTRY_CAP, RGK_LIGHT_ENTRY, RGK_CONST_LIGHT, RGK_LAST_VERTEX, RGK_SAMPLE_GROUP, RGK_BATCH_PATHS, RGK_WORKSPACE_GB,
// RGK_BEAM, RGK_DEBUG_BVH, RGK_DEBUG_UTIL); afterwards only rgk_scene_set_tuning changes them -- a round never reads the environment
// (round 2 did, per round: process-global state under a host that may render from two threads).  The build switches are read
// at the same moment, by read_build_options (rgk_commit.h).
struct RgkTuning {
    bool entry_points = true; // camera rays start at their pixel group's entry nodes (k_entry_points)
    bool entry_cap = true;    // ... capped behind the group's first hits from a frame's second round on
    bool light_entry = true;  // first-vertex shadow rays of a single-light scene start at light-side entry nodes
    bool const_light = true;  // eligible scenes (rgk_scene_info::const_light): unidirectional rounds take the light as a launch constant
    bool last_vertex = true;  // the last bounce of a unidirectional pass is shaded by k_last_vertex (rgk_shade.h); false: by k_shade
    int sample_group = -1;    // log2 of the samples of a pixel side by side in the slot order; -1: the compiled default
    size_t batch_paths = 0;   // paths per pass; 0: sized from the memory that is free
    double workspace_gb = 0;  // ... or from this many GB; 0: 96 (160 for bidirectional rounds), at most 60 % of what is free
    int beam = 1;             // pinhole cameras: bounce 0 walks the tree once per pixel for 8 samples (k_trace_camera_beam) -- 1: while the
                              // entry lists are uncapped (a frame's first round), 2: always, 0: never
    bool debug_bvh = false, debug_util = false;
    bool time_post = false;   // feature pass / denoiser: HIP events around their launches (rgk_scene_get_post_timing)
};

// rgk_scene_get_post_timing's `which` (rgk.h): the post-processing call whose launch times a slot holds
enum PostSlot : uint32_t { POST_AOV = 0, POST_DENOISE = 1, POST_DENOISE_VARIANCE = 2, POST_NOISE = 3, POST_FOLD = 4, POST_TEMPORAL = 5, POST_AOV_CHAIN = 6, POST_UPSAMPLE = 7, POST_REMODULATE = 8, POST_DEMOD_ROUND = 9, POST_DISPLAY_MEASURE = 10, POST_DISPLAY_ENCODE = 11, POST_OUTPUT_EXR = 12, POST_OUTPUT_PNG = 13, POST_SLOTS = 14 };
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
    // ... and of the build: a triangle without a plane (NaN: two equal corners, three on a line) gets no reference, so a refit that
    // gives one of them a plane cannot find it in the old topology and builds the tree again, with the builder and switches kept here
    std::vector<uint8_t> h_no_ref; // per triangle: 1 where the tree holds no reference of it; empty when every triangle has one
    uint32_t build_flags = 0;
    BuildOptions build_opt;
    uint32_t n_textures = 0, n_materials = 0;
    DevBuf<DevHaltonDim> hdims;
    DevBuf<uint16_t> hperm;
    // workspace (the per-path planes: rgk_round_plan.h RGK_WORKSPACE)
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
    DevBuf<float4> us_rec;              // the upsampler's tap records: three planes of the low grid (k_us_prepare)
    // demodulated rounds (rgk_render_round_demod_device), allocated by the first one; beside the workspace, not part of its table
    DevBuf<float4> demod_div;           // per path slot of a pass: the sample's divisor {div.rgb, 0} (k_demod_divisor), `batch` entries
    DevBuf<float4> demod_pixsum;        // per pixel of the round: {Dsum}, {Asum} carried across sample passes (k_resolve_demod)
    // display output (rgk_display_measure_device / rgk_display_encode_device), allocated by the first call of either
    DevBuf<uint32_t> disp_hist;         // 256 bins, then the dark count; cleared on the stream by every measure before its launch
    DevBuf<float> disp_table;           // the 256 thresholds of the sRGB bytes (rgk_display_table), uploaded once
    // device output path (rgk_output_write_exr_device / rgk_output_write_png_device), allocated by the first call of either, grown on demand
    DevBuf<uint8_t> out_dev;            // what the pack kernels write: the file region, then the scale word and partial maxima / the checksum pieces
    uint8_t* out_pin = nullptr;         // pinned: the whole file image, the device's part arriving in one copy
    size_t out_pin_n = 0;
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
        if (out_pin) (void)hipHostFree(out_pin);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// ------------------------------------------------------------------ helpers more than one host file calls
// The workspace for passes of `paths` paths with `reverse` light vertices; it only grows (rgk_scene.cpp).
int ensure_workspace(rgk_scene* s, size_t paths, uint32_t reverse = 0);
// The round's pixel list (toff[n_tiles] > 0 pixels) in Tracer::Render order with its per-pixel seeds (a1, a2), built on the device
// from the tile list.  A queued copy reads `toff`: the caller keeps it until it has synchronised the stream (rgk_round.cpp).
int queue_pixel_list(rgk_scene* s, const rgk_tile* tiles, uint32_t n_tiles, const std::vector<uint32_t>& toff);

// Event `i` of the scene's pool, which grows on demand and goes with the scene.  A round and a post call never overlap on a scene
// (prog_busy), so each call counts from 0.
inline int scene_event(rgk_scene* s, size_t i, hipEvent_t& e) {
    while (s->events.size() <= i) { hipEvent_t n; HIPCHK(hipEventCreate(&n)); s->events.push_back(n); }
    e = s->events[i];
    return 0;
}

// The frame sizes the kernels' 16-bit pixel coordinates can hold.
inline int check_frame_size(uint32_t xres, uint32_t yres) {
    if (xres == 0 || yres == 0 || xres > 65535 || yres > 65535) return fail(RGK_ERR_INVALID, "resolution out of range");
    return RGK_OK;
}

// The eight traversal-stats words: closest nodes / triangles, shadow nodes / triangles, and the walker's occupancy counters.
inline int read_stats(const rgk_scene* s, unsigned long long (&h)[8]) { return down(h, s->stats, 8); }

// The per-frame lists (entry nodes, their caps, light-side entries) were made for the old boxes or switches: the next round rebuilds them.
inline void invalidate_frame_lists(rgk_scene* s) { s->entry_key = 0; s->entry_n = 0; s->entry_capped = 0; s->lentry_done = 0; }

inline void make_camera(const rgk_camera* c, DevCamera& o) { // the members RenderRound's `const Camera&` carries, as they are
    for (int k = 0; k < 3; k++) {
        o.origin[k] = c->origin[k]; o.direction[k] = c->direction[k]; o.up[k] = c->cameraup[k]; o.left[k] = c->cameraleft[k];
        o.viewscreen[k] = c->viewscreen[k]; o.viewscreen_x[k] = c->viewscreen_x[k]; o.viewscreen_y[k] = c->viewscreen_y[k];
    }
    o.lens_size = c->lens_size; o.xsize = c->xsize; o.ysize = c->ysize;
}

// The tiles checked against the frame, and their offsets into the pixel list they make (rgk_round_plan.h rgk_tile_offsets).
// `what`: the caller's unit of work, for the error text.
inline int tile_offsets(const rgk_params* prm, const rgk_tile* tiles, uint32_t n_tiles, const char* what, std::vector<uint32_t>& toff) {
    uint32_t bad = 0;
    switch (rgk_tile_offsets(prm->xres, prm->yres, tiles, n_tiles, toff, bad)) {
    case RGK_TILES_OUTSIDE: return fail(RGK_ERR_INVALID, "tile %u outside the frame", bad);
    case RGK_TILES_TOO_MANY_PIXELS: return fail(RGK_ERR_UNSUPPORTED, "more than 2^31 pixels in one %s", what);
    case RGK_TILES_OK: break;
    }
    return 0;
}
#pragma GCC visibility pop
