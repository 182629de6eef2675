// The scene object behind the C ABI of include/rgk.h: rgk_scene_create takes what the GPU-free commit unit computes (rgk_commit.h:
// bounds and epsilon, triangle records, the SAH accelerator, shading tables), or has the accelerator built on the device
// (rgk_build.h), and uploads it; rgk_scene_refit, tuning, progress; the workspace of a pass; the task list and the camera.
#include <algorithm>
#include <cmath>
#include <string>

#include "rgk_scene_impl.h"
#include "rgk_build.h"

int ensure_workspace(rgk_scene* s, size_t paths, uint32_t reverse) {
    if (paths <= s->batch && reverse <= s->batch_reverse) return 0;
    if (s->batch) { paths = std::max(paths, s->batch); reverse = std::max(reverse, s->batch_reverse); }
    const auto alloc = [s](RgkPlaneId id, size_t n) -> int {
        switch (id) {
        case RGK_WS_RAYA0: return s->rayA[0].alloc(n);
        case RGK_WS_RAYB0: return s->rayB[0].alloc(n);
        case RGK_WS_RAYA1: return s->rayA[1].alloc(n);
        case RGK_WS_RAYB1: return s->rayB[1].alloc(n);
        case RGK_WS_HIT: return s->hit.alloc(n);
        case RGK_WS_THR: return s->thr.alloc(n);
        case RGK_WS_TOT: return s->tot.alloc(n);
        case RGK_WS_SHA: return s->shA.alloc(n);
        case RGK_WS_SHB: return s->shB.alloc(n);
        case RGK_WS_SHC: return s->shC.alloc(n);
        case RGK_WS_LSTART: return s->lstart.alloc(n);
        case RGK_WS_LV: return s->lv.alloc(n);
        case RGK_WS_HITLIST: return s->hitlist.alloc(n);
        case RGK_WS_LVMASK: return s->lvmask.alloc(n);
        case RGK_WS_CONNLIST: return s->connlist.alloc(n);
        case RGK_WS_CONN: return s->conn.alloc(n);
        case RGK_WS_JOBS: return s->jobs.alloc(n);
        case RGK_WS_RADS: return s->rads.alloc(n);
        case RGK_WS_LIGHT: return s->light.alloc(n);
        case RGK_WS_GENERIC: return s->generic.alloc(n);
        case RGK_WS_PLANES: break;
        }
        return fail(RGK_ERR_INVALID, "unknown workspace plane");
    };
    int rc = 0;
    for (const RgkWorkspacePlane& pl : RGK_WORKSPACE)
        if (!rc && (!pl.bidir || reverse)) rc = alloc(pl.id, rgk_plane_elems(pl, paths, reverse));
    if (!rc) rc = s->counters.alloc(2 * RGK_CNT_TOTAL); // [0] camera phase, [1] light sub-path phase
    if (!rc) rc = s->stats.alloc(8);
    if (rc) { s->batch = 0; s->batch_reverse = 0; return rc; } // some buffers are gone: the next call starts over
    if (!s->h_counters) HIPCHK(hipHostMalloc((void**)&s->h_counters, 2 * RGK_CNT_TOTAL * sizeof(uint32_t)));
    if (!s->h_stage) { HIPCHK(hipHostMalloc((void**)&s->h_stage, sizeof(uint32_t))); *s->h_stage = 0; }
    s->batch = paths;
    s->batch_reverse = reverse;
    return 0;
}

namespace {

RgkTuning read_tuning() {
    auto off = [](const char* name) { const char* e = std::getenv(name); return e && e[0] == '0'; };
    RgkTuning t;
    t.entry_points = !off("RGK_ENTRY_POINTS"); t.entry_cap = !off("RGK_ENTRY_CAP"); t.light_entry = !off("RGK_LIGHT_ENTRY");
    t.const_light = !off("RGK_CONST_LIGHT");
    t.last_vertex = !off("RGK_LAST_VERTEX");
    if (const char* e = std::getenv("RGK_SAMPLE_GROUP")) t.sample_group = std::min(6, std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("RGK_BATCH_PATHS")) t.batch_paths = std::max<size_t>(1024, strtoull(e, nullptr, 10));
    if (const char* e = std::getenv("RGK_WORKSPACE_GB")) t.workspace_gb = atof(e);
    if (const char* e = std::getenv("RGK_BEAM")) t.beam = std::min(2, std::max(0, std::atoi(e)));
    t.debug_bvh = std::getenv("RGK_DEBUG_BVH") != nullptr; t.debug_util = std::getenv("RGK_DEBUG_UTIL") != nullptr;
    return t;
}

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
    acc.n_refs = (uint32_t)prims.size();
    rc = rgk_build_bvh4_device(s->stream, bp.data(), acc.n_refs, mn, mx, eps, (uint32_t)opt.max_leaf_dev, opt.lbvh_rotate, opt.lbvh_ploc, opt.lbvh_morton_bits, d_recs.p,
                               s->nodes.p, s->tris.p, s->leaf_pb.p, &acc.n_nodes, &levels);
    if (rc) return rc;
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

// Which triangles the tree holds no reference of (commit_triangles leaves out those without a plane).
void note_unreferenced(rgk_scene* s, const std::vector<Prim>& prims, uint32_t n_triangles) {
    s->h_no_ref.assign(n_triangles, 1);
    size_t left = n_triangles;
    for (const Prim& p : prims)
        if (s->h_no_ref[p.tri]) { s->h_no_ref[p.tri] = 0; left--; }
    if (!left) s->h_no_ref.clear();
}

// Does a triangle that the tree holds no reference of have a plane at the new positions?
bool unreferenced_triangle_gets_a_plane(const rgk_scene* s, const float* vertices) {
    for (size_t t = 0; t < s->h_no_ref.size(); t++) {
        if (!s->h_no_ref[t]) continue;
        V3 v[3];
        for (int c = 0; c < 3; c++) { const float* p = vertices + 3 * (size_t)s->h_idx[3 * t + c]; v[c] = V3{p[0], p[1], p[2]}; }
        const TriIsect r = tri_isect_record(v[0], v[1], v[2], (uint32_t)t);
        if (r.n[0] == r.n[0] && r.n[1] == r.n[1] && r.n[2] == r.n[2]) return true;
    }
    return false;
}

// Traversal stack: the scene's configuration (rgk_round_plan.h rgk_stack_plan) and its overflow area
int configure_stack(rgk_scene* s, uint32_t max_stack, const BuildOptions& opt) {
    RgkStackPlan sp;
    if (!rgk_stack_plan(max_stack, opt.stack_ovf, opt.stack_lds, sp)) return fail(RGK_ERR_UNSUPPORTED, "BVH needs %u traversal-stack entries (max 256)", max_stack + 1);
    s->tcfg = {sp.stack, sp.lds, nullptr};
    if (sp.ovf_per_lane) {
        if (int rc = s->ovf.alloc((size_t)rgk_trace_grid(sp.lds) * RGK_TRACE_BLOCK * sp.ovf_per_lane)) return rc;
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

// The accelerator built again from moved vertices, as rgk_scene_create builds it: rgk_scene_refit's way out when the old topology
// lacks a triangle.  The refit that follows recomputes the records and boxes it leaves (the same bits) and the shading records.
int rebuild_accel(rgk_scene* s, const float* vertices, const float mn[3], const float mx[3], float eps) {
    std::vector<TriIsect> recs;
    std::vector<Prim> prims;
    commit_triangles(vertices, s->h_idx.data(), s->n_triangles, split_threshold(s->build_opt, eps), recs, prims);
    HostAccel host;
    AccelInfo acc;
    int rc;
    if ((rc = build_accel(s, s->build_flags, prims, recs, mn, mx, eps, s->build_opt, host, acc))) return rc;
    if ((rc = configure_stack(s, acc.max_stack, s->build_opt))) return rc;
    if (!acc.on_device && ((rc = s->nodes.upload(host.qnodes.data(), host.qnodes.size())) || (rc = s->tris.upload(host.leaf_recs.data(), host.leaf_recs.size())) ||
                           (rc = s->leaf_pb.upload(host.leaf_pb.data(), host.leaf_pb.size()))))
        return rc;
    s->n_refs = acc.n_refs; s->n_nodes = acc.n_nodes;
    s->dev.nodes = s->nodes.p; s->dev.tris = s->tris.p;
    s->info.n_nodes = acc.n_nodes; s->info.max_depth = acc.max_depth; s->info.n_leaf_refs = acc.n_refs;
    note_unreferenced(s, prims, s->n_triangles);
    return 0;
}

} // namespace

extern "C" {

int rgk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

uint64_t rgk_debug_poisoned_bytes(void) { return rgk_poison_total().load(std::memory_order_relaxed); }

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
    s->build_flags = d->build_flags; s->build_opt = opt;
    note_unreferenced(s, prims, d->n_triangles);

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
    // ---- a triangle the tree has no reference of, and that now has a plane: the tree is built again
    if (unreferenced_triangle_gets_a_plane(s, vertices) && (rc = rebuild_accel(s, vertices, mn, mx, eps))) return rc;
    // ---- records, shading normals / tangents, and the tree's boxes: on the device
    if ((rc = s->scratch_f.upload(vertices, 3 * (size_t)nv))) return rc;
    DevBuf<float> d_n, d_t;
    if (normals && (rc = d_n.upload(normals, 3 * (size_t)nv))) return rc;
    if (tangents && (rc = d_t.upload(tangents, 3 * (size_t)nv))) return rc;
    rc = rgk_refit_bvh4_device(s->stream, s->n_refs, s->n_nodes, nt, s->scratch_f.p, normals ? d_n.p : nullptr, tangents ? d_t.p : nullptr, s->d_idx.p, s->leaf_pb.p, eps,
                               s->tris.p, s->nodes.p, s->tri_shade.p);
    if (rc) return rc;
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
    else if (k == "last_vertex") t.last_vertex = value != 0;
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
    const std::vector<rgk_tile> v = rgk_task_list(tile_size, xres, yres, mid_x, mid_y, seedstart + seedcount_base);
    if (tiles) {
        if (*n_tiles < v.size()) return fail(RGK_ERR_INVALID, "tile buffer too small (%u < %zu)", *n_tiles, v.size());
        std::copy(v.begin(), v.end(), tiles);
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

} // extern "C"
