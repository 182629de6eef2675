/*
 * rgk.h -- C ABI of the MI355X path-tracing core (librgk_hip.so).
 *
 * This is the drop-in boundary for the per-tile body of the reference's
 * RenderDriver::RenderRound (reference src/render_driver.cpp:144-190): the
 * lambda that builds a PathTracer (src/path_tracer.cpp:20-40), calls
 * Tracer::Render (src/tracer.cpp:6-37) on one RenderTask and merges the
 * private EXRTexture into the frame accumulator (src/texture.cpp:403-412).
 *
 * Plain C, plain pointers and sizes.  No C++ or torch types cross it.
 * Every entry point returns RGK_OK (0) or a negative rgk_status; nothing
 * throws across the ABI.  rgk_last_error() gives a thread-local message.
 *
 * All arithmetic on the path is float32 except the two plane dot products of
 * the triangle test (double, reference src/primitives.cpp:85,99-100).
 */
#ifndef RGK_H
#define RGK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rgk_status {
    RGK_OK = 0,
    RGK_ERR_INVALID = -1,   /* bad descriptor / argument                       */
    RGK_ERR_DEVICE = -2,    /* HIP runtime failure (message in rgk_last_error) */
    RGK_ERR_OOM = -3,       /* host or device allocation failed                */
    RGK_ERR_NO_DEVICE = -4, /* no HIP device visible                           */
    RGK_ERR_UNSUPPORTED = -5
} rgk_status;

/* ---- materials: mirrors Material + BxDF subclasses, src/bxdf/bxdf.hpp:19-159,
 *      brdf ids accepted by Material::LoadFromJson src/bxdf/bxdf.cpp:63-84 ---- */
typedef enum rgk_bxdf_kind {
    RGK_BXDF_DIFFUSE = 0,              /* "diffuse"/"diffusecosine"  bxdf.cpp:192-204 */
    RGK_BXDF_MIRROR = 1,               /* "mirror"                   bxdf.cpp:265-276 */
    RGK_BXDF_DIELECTRIC = 2,           /* "dielectric"               bxdf.cpp:332-408 */
    RGK_BXDF_TRANSPARENT = 3,          /* "transparent"              bxdf.cpp:412-423 */
    RGK_BXDF_MIX = 4,                  /* "mix"                      bxdf.cpp:235-249 */
    RGK_BXDF_LTC_BECKMANN = 5,         /* "ltc_beckmann"             bxdf.hpp:107-122 */
    RGK_BXDF_LTC_GGX = 6,              /* "ltc_ggx"                                   */
    RGK_BXDF_LTC_BECKMANN_DIFFUSE = 7, /* "ltc_beckmann_diffuse"     bxdf.hpp:125-159 */
    RGK_BXDF_LTC_GGX_DIFFUSE = 8       /* "ltc_ggx_diffuse"                           */
} rgk_bxdf_kind;

#define RGK_MAT_NO_RUSSIAN 1u /* Material::no_russian, bxdf.hpp:31 */

typedef struct rgk_material {
    uint32_t kind;       /* rgk_bxdf_kind */
    uint32_t flags;      /* RGK_MAT_* */
    float emission[3];   /* Material::emission */
    float roughness;     /* BxDFLTCBase::roughness */
    float ior;           /* BxDFDielectric::ior */
    float amount;        /* BxDFMix::amt1 */
    int32_t tex_diffuse; /* texture id or -1 (EmptyTexture: black, Empty()==true) */
    int32_t tex_color;   /* specular / mirror / dielectric colour texture, or -1 */
    int32_t tex_bump;    /* Material::bumpmap, or -1 */
    int32_t mix_m1;      /* BxDFMix::m1 material index, or -1 */
    int32_t mix_m2;      /* BxDFMix::m2 */
} rgk_material;

/* ---- textures: ReadableTexture family, src/texture.hpp:10-80 ---- */
typedef enum rgk_texture_kind {
    RGK_TEX_SOLID = 0,  /* SolidTexture: constant colour, slopes 0 */
    RGK_TEX_RGB32F = 1, /* FileTexture: width*height Color{r,g,b} float triples, row-major,
                           already gamma-decoded / flipped as the reference loader does -- what a binding to the reference hands
                           over (FileTexture::data).  One whose channels take <= 256 distinct values (every texture the reference
                           decodes from an 8-bit file, src/texture.cpp:203,252-254) is stored like RGK_TEX_RGB8 internally */
    RGK_TEX_RGB8 = 2    /* FileTexture decoded from an 8-bit file (PNG/JPEG, src/texture.cpp:189-292):
                           the bytes as stored (row-major, flipped as the loader does) plus the 256-entry
                           table that turns a byte into the float the reference would hold
                           (Color(byte/255).gammaDecode(2.2)).  Same texel values as RGK_TEX_RGB32F at a
                           quarter of the memory traffic. */
} rgk_texture_kind;

typedef struct rgk_texture {
    uint32_t kind;
    uint32_t width, height;
    float color[3];         /* RGK_TEX_SOLID */
    const float *texels;    /* RGK_TEX_RGB32F: 3*width*height floats */
    const uint8_t *texels8; /* RGK_TEX_RGB8: 3*width*height bytes */
    const float *lut;       /* RGK_TEX_RGB8: 256 floats, byte -> channel value */
} rgk_texture;

/* ---- point / sphere lights: Light{FULL_SPHERE}, src/primitives.hpp:26-43,
 *      filled by ConfigJSON::InstallLights src/config.cpp:372-387 ---- */
typedef struct rgk_pointlight {
    float pos[3];
    float color[3];
    float intensity;
    float size;
} rgk_pointlight;

typedef enum rgk_sky_mode { RGK_SKY_COLOR = 0, RGK_SKY_ENVMAP = 1 } rgk_sky_mode;

/* ---- the immutable Scene as it crosses the seam (src/scene.hpp:76-172) ---- */
typedef struct rgk_scene_desc {
    uint32_t n_vertices;
    const float *vertices;  /* 3*n  Scene::vertices  */
    const float *normals;   /* 3*n  Scene::normals   */
    const float *tangents;  /* 3*n  Scene::tangents  */
    const float *texcoords; /* 2*n  Scene::texcoords */

    uint32_t n_triangles;
    const uint32_t *tri_indices;  /* 3*n  Triangle::va,vb,vc */
    const uint32_t *tri_material; /* n    Triangle::mat as an index */

    uint32_t n_materials;
    const rgk_material *materials;
    uint32_t n_textures;
    const rgk_texture *textures;

    uint32_t n_pointlights;
    const rgk_pointlight *pointlights;

    /* Scene::areal_lights (src/scene.hpp:91-103): one group per emissive
     * primitive / mesh, listing its triangle ids in insertion order.       */
    uint32_t n_areal_lights;
    const uint32_t *areal_offsets; /* n_areal_lights+1 */
    const uint32_t *areal_tris;

    /* sky, Scene::SetSkyboxColor / SetSkyboxEnvmap src/scene.hpp:122-133 */
    uint32_t sky_mode;
    float sky_color[3];
    float sky_intensity;
    float sky_rotate;
    int32_t sky_texture;

    /* LTC fits (src/LTC/ltc_ggx.cpp, ltc_beckmann.cpp): 64*64 entries of
     * {m0,m2,m4,m6,amplitude} as float32 (the only non-constant entries of
     * tabM; m8==1, the rest 0).  Either may be NULL if no material uses it. */
    const float *ltc_ggx;
    const float *ltc_beckmann;

    /* RGK_BUILD_*: how the accelerator is built (results never depend on it: hits come from the triangle records) */
    uint32_t build_flags;
} rgk_scene_desc;

#define RGK_BUILD_AUTO 0u     /* default: the host builder below half a million triangle references, the device builder from there on */
#define RGK_BUILD_HOST_SAH 4u /* binned SAH + reinsertion on the host, collapsed to the 4-wide quantised BVH: the best traversal, seconds
                                 to build at a million triangles                                                              */
#define RGK_BUILD_KEEP_FLOAT_TEXTURES 2u /* store every RGK_TEX_RGB32F texture as float4 texels, even one with <= 256 distinct channel
                                            values (by default such a texture is stored as bytes + the table of its values: the same
                                            texel values, a quarter of the traffic)                                                */
#define RGK_BUILD_DEVICE 1u   /* tree built on the GPU (Morton sort, bottom-up clustering of the sorted references by surface, refit,
                                 collapse + quantisation: all on the device; no rotation pass.  RGK_LBVH_PLOC=0 in the environment:
                                 the Karras prefix hierarchy instead, then refit with tree rotations): a tenth of the host's build
                                 time, traversal within a few per cent of it                                                  */

/* ---- Camera as RenderRound(const Camera&) receives it (src/render_driver.cpp:146): the public data members
 *      of the reference's Camera, src/camera.hpp:27-41, under their own names (`lookat` is not read on the path).
 *      A host that holds a Camera copies the members; a host that only has the constructor arguments
 *      (ConfigJSON::GetCamera, src/config.cpp:332-370) calls rgk_camera_init below. ---- */
typedef struct rgk_camera {
    float origin[3];
    float direction[3];
    float cameraup[3];
    float cameraleft[3];
    float viewscreen[3];
    float viewscreen_x[3];
    float viewscreen_y[3];
    float lens_size;
    int32_t xsize, ysize;
} rgk_camera;

typedef enum rgk_sampler_kind {
    RGK_SAMPLER_HALTON = 0,    /* counter-based Faure-Halton + Cranley-Patterson */
    RGK_SAMPLER_STRATIFIED = 1 /* oracle only: reference StratifiedSampler, src/sampler.cpp:85-116 */
} rgk_sampler_kind;

#define RGK_FLAG_COUNT_TRAVERSAL 1u /* fill node_visits / tri_tests (slower kernels) */
#define RGK_FLAG_TIME_KERNELS 2u    /* bracket every kernel class with HIP events     */

/* ---- PathTracer constructor arguments, src/path_tracer.cpp:20-40 ---- */
typedef struct rgk_params {
    uint32_t xres, yres;
    uint32_t multisample;
    uint32_t depth;
    float clamp;
    float russian;
    float bumpmap_scale;
    uint32_t force_fresnell; /* stored, unused -- as in the reference */
    uint32_t reverse;
    uint32_t sampler; /* rgk_sampler_kind */
    uint32_t flags;   /* RGK_FLAG_* */
} rgk_params;

/* ---- RenderTask (src/tracer.hpp:14-24) + its PathTracer seed
 *      (seedstart + c, src/render_driver.cpp:160,173) ---- */
typedef struct rgk_tile {
    uint32_t x0, x1, y0, y1; /* xrange_start, xrange_end, yrange_start, yrange_end */
    uint32_t seed;
} rgk_tile;

/* The kernels of a round, for the per-kernel records in rgk_counters: RGK_FLAG_TIME_KERNELS / RGK_FLAG_COUNT_TRAVERSAL. */
typedef enum rgk_kernel_id {
    RGK_K_TRACE_CAMERA = 0, /* k_trace_camera: bounce 0, camera rays made where they are traced          */
    RGK_K_TRACE_CLOSEST,    /* k_trace_closest: camera-path bounces >= 1                                 */
    RGK_K_SHADE_FIRST,      /* k_shade<., FIRST = true>: the first vertex of every path                  */
    RGK_K_SHADE,            /* k_shade<., FIRST = false>: later vertices                                 */
    RGK_K_SHADOW_FIRST,     /* k_trace_shadow_first: first-vertex NEE rays from light-side entry nodes   */
    RGK_K_SHADOW,           /* k_trace_shadow: NEE rays                                                  */
    RGK_K_SHADOW_JOBS,      /* k_trace_shadow_jobs: vertices with connections (reverse > 0)              */
    RGK_K_CONNECT,          /* k_connect (reverse > 0)                                                   */
    RGK_K_LIGHT_TRACE,      /* k_trace_closest of the light sub-path (reverse > 0)                       */
    RGK_K_LIGHT_SHADE,      /* k_raygen_light + k_list_hits + k_shade_light                              */
    RGK_K_LIGHT_SPLAT,      /* k_trace_shadow in splat mode: light-tracing side effects                  */
    RGK_K_RESOLVE,          /* k_resolve[_tiled]                                                         */
    RGK_K_OTHER,            /* per-round / per-frame lists, counters, progress marks                     */
    RGK_K_COUNT
} rgk_kernel_id;

typedef struct rgk_kernel_stat {
    double ms;            /* RGK_FLAG_TIME_KERNELS: summed HIP-event time on the scene's stream           */
    uint32_t launches;
    uint32_t reserved;
    uint64_t units;       /* rays (trace kernels) / vertices (shade, connect, jobs) / paths (resolve)     */
    uint64_t node_visits; /* RGK_FLAG_COUNT_TRAVERSAL, trace kernels                                      */
    uint64_t tri_tests;
} rgk_kernel_stat;

typedef struct rgk_counters {
    uint64_t paths;        /* pixels * multisample processed                      */
    uint64_t path_rays;    /* reference semantics: raycount++ path_tracer.cpp:126 */
    uint64_t shadow_rays;  /* Visibility() calls                                  */
    uint64_t node_visits;  /* closest-hit traversal, RGK_FLAG_COUNT_TRAVERSAL     */
    uint64_t tri_tests;
    uint64_t shadow_node_visits;
    uint64_t shadow_tri_tests;
    double ms_trace;       /* RGK_FLAG_TIME_KERNELS: summed HIP-event time, ms    */
    double ms_shadow;
    double ms_shade;
    double ms_other;
    uint32_t n_trace_launches;
    uint32_t n_shadow_launches;
    uint32_t n_shade_launches;
    uint32_t reserved;
    rgk_kernel_stat kernel[RGK_K_COUNT]; /* the same, per kernel (the four class sums above are sums of these) */
} rgk_counters;

typedef struct rgk_scene_info {
    float epsilon;        /* Scene::epsilon, src/scene.cpp:390   */
    float bbox_min[3];    /* xBB/yBB/zBB .first,  scene.cpp:393  */
    float bbox_max[3];
    float total_areal_power, total_point_power; /* scene.cpp:323-344 */
    uint32_t n_nodes;     /* accelerator nodes                    */
    uint32_t node_bytes;  /* s_node of SURVEY 8(d)                */
    uint32_t tri_bytes;   /* s_tri                                */
    uint32_t max_depth;
    uint32_t n_leaf_refs;
    uint32_t n_float_textures;      /* RGK_TEX_RGB32F textures handed over ...                                          */
    uint32_t n_palettized_textures; /* ... and how many of them are stored as bytes + value table (<= 256 distinct values) */
    uint32_t const_light; /* 1: the scene's only light is ONE point light of size 0 that every path provably picks, so unidirectional
                           * rounds take it as a launch constant (see rgk_scene_set_tuning "const_light"); 0: the per-path pick */
} rgk_scene_info;

typedef struct rgk_hit {
    float t;
    int32_t tri; /* triangle index or -1 */
    float a, b, c; /* Intersection::a,b,c  (c'=1-alpha-beta, alpha, beta) scene_intersect.cpp:280-283 */
} rgk_hit;

/* Progress of the round a scene is rendering, for a monitor thread (the reference's FrameMonitorThread reads pixels_done /
 * rays_done every 100 ms, src/render_driver.cpp:49-139).  Fed from the device's side of the stream: a host callback behind every
 * bounce of every pass bumps `stage`.  pixels_done of the reference = round_pixels * stage / stages (+ round_pixels per finished round). */
typedef struct rgk_progress {
    uint32_t stage, stages;      /* bounces finished / bounces in the round (over all passes); stage == stages: round done */
    uint32_t rounds;             /* rounds this scene has finished since it was created                                    */
    uint32_t busy;               /* 1 while a round is in flight                                                            */
    uint64_t round_pixels;       /* pixels of the round in flight (or of the last one)                                      */
    uint64_t round_paths;        /* pixels * multisample                                                                     */
} rgk_progress;

typedef struct rgk_scene rgk_scene;

const char *rgk_last_error(void);
int rgk_device_count(void);
/* Debugging aid.  With RGK_POISON set in the environment (read once per process) every fresh device allocation of the library --
 * a scene's buffers and the device builder's scratch -- is filled with 0xFF bytes, so that a read of memory nothing wrote shows
 * in the results.  This is the number of bytes filled so far in this process; 0 when the switch is off. */
uint64_t rgk_debug_poisoned_bytes(void);

/* Scene::Commit() outputs (src/scene.cpp:294-400) + accelerator build + upload. */
int rgk_scene_create(const rgk_scene_desc *desc, int device, rgk_scene **out);
/* Moved vertices, same triangles (an animated mesh between two frames; SURVEY 8(f) f2 "refit").  What Scene::Commit derives
 * from the positions is recomputed -- triangle planes, epsilon = 1e-5 * diagonal, the padded box, the areal-light tables
 * (src/scene.cpp:294-400) -- and the accelerator is REFIT on the device: its topology stays, every box is recomputed bottom-up
 * (milliseconds at a million triangles, where a rebuild takes 0.15 - 1.5 s).  Hits are those of a freshly created scene with
 * the same vertices (they come from the triangle records; boxes only steer the walk); the walk is as good as the old topology
 * fits the new positions.  vertices: 3 * n_vertices floats; normals / tangents: the same, or NULL = unchanged.  A triangle
 * that was degenerate at creation is not in the tree and stays out.  Not while a round is in flight on this scene. */
int rgk_scene_refit(rgk_scene *scene, const float *vertices, const float *normals, const float *tangents);
void rgk_scene_destroy(rgk_scene *scene);
int rgk_scene_get_info(const rgk_scene *scene, rgk_scene_info *out);

/* Callable from ANY thread while another thread is inside rgk_render_round*: never blocks, touches no device state. */
int rgk_scene_get_progress(const rgk_scene *scene, rgk_progress *out);

/* Tuning switches of ONE scene; none of them changes a result (the tests render with each and compare bits).  Keys:
 * "entry_points", "entry_cap", "light_entry" (0 / 1: where camera rays and first shadow rays start their walk), "sample_group"
 * (log2 of the samples of a pixel that sit side by side in the path-slot order, 0..6; -1: default), "batch_paths" (paths per
 * pass; 0: sized from the free memory), "workspace_gb" (0: default), "beam" (0 / 1: camera rays of a pixel walk the tree together),
 * "const_light" (0 / 1, default 1: in a scene that reports rgk_scene_info.const_light == 1, unidirectional rounds (reverse == 0)
 * do not sample, store and re-read "the path's light" per path -- it is the same {position, light 0} for every path -- but take
 * position, colour and intensity as launch constants, and their shadow rays are queued without the origin and near distance all
 * of them share; 0: the per-path route.  The scene qualifies when it has exactly one point light and no emitting triangle, the
 * light's size is 0, no component of its position is -0.0 (pos + 0 * v must give back pos bit for bit), and GetRandomLight's
 * own two float comparisons, evaluated with its own expressions for the largest number the sampler returns, 1 - 2^-24, select
 * light 0: rounding is monotone, so every smaller sample selects it too.  Same bits either way), "last_vertex" (0 / 1, default 1:
 * the last bounce of a unidirectional pass, whose vertices all end their paths, is shaded by a kernel of its own that neither
 * samples nor queues a ray and evaluates the direct light of the vertices that can receive any on full waves; 0: by the kernel of
 * the other bounces.  Same bits either way; RGK_LAST_VERTEX), "time_post" (0 / 1, default 0: HIP events
 * around the launches of the feature pass and the denoiser, read with rgk_scene_get_post_timing).  Their initial values are read from the environment
 * (RGK_ENTRY_POINTS, RGK_ENTRY_CAP, RGK_LIGHT_ENTRY, RGK_CONST_LIGHT, RGK_LAST_VERTEX, RGK_SAMPLE_GROUP, RGK_BATCH_PATHS, RGK_WORKSPACE_GB) ONCE, in
 * rgk_scene_create; a round never reads the environment.  Not while a round is in flight on this scene. */
int rgk_scene_set_tuning(rgk_scene *scene, const char *key, double value);

/* GenerateTaskList, src/render_driver.cpp:30-46.  Tiles of tile_size, sorted by
 * distance of the tile midpoint to (mid_x, mid_y); ties broken by (y0, x0)
 * (the reference's std::sort leaves ties unspecified).  `seed` of
 * tile i is seedstart + seedcount_base + i.  Call with tiles==NULL for the count. */
int rgk_generate_task_list(uint32_t tile_size, uint32_t xres, uint32_t yres, float mid_x,
                           float mid_y, uint32_t seedstart, uint32_t seedcount_base,
                           rgk_tile *tiles, uint32_t *n_tiles);

/* Camera::Camera(pos, la, up, yview, xview, xsize, ysize, focus_plane, lens_size), src/camera.cpp:7-24: fills the
 * derived members from the constructor arguments, in the reference's operation order (host only, no device needed). */
int rgk_camera_init(rgk_camera *out, const float pos[3], const float lookat[3], const float up[3], float yview,
                    float xview, int32_t xsize, int32_t ysize, float focus_plane, float lens_size);

/* The per-task body of RenderRound for a list of tiles (render_driver.cpp:158-184):
 * accum_rgb[3*(y*xres+x)..] += sum over samples, accum_count[y*xres+x] += multisample.
 * Host buffers; blocking. */
int rgk_render_round(rgk_scene *scene, const rgk_camera *camera, const rgk_params *params,
                     const rgk_tile *tiles, uint32_t n_tiles, float *accum_rgb,
                     uint32_t *accum_count, rgk_counters *counters);

/* Same, adding into DEVICE buffers on the scene's GPU (the per-GPU private
 * accumulator that RCCL then reduces).  Blocking unless the stream is the caller's. */
int rgk_render_round_device(rgk_scene *scene, const rgk_camera *camera,
                            const rgk_params *params, const rgk_tile *tiles, uint32_t n_tiles,
                            float *d_accum_rgb, uint32_t *d_accum_count,
                            rgk_counters *counters);

/* ---- the frame accumulator on the device: EXRTexture total_ob of RenderFrame (src/render_driver.cpp:199,
 *      src/texture.hpp:83-118: `data` = sum of radiance per pixel, `count` = samples per pixel).  A host without HIP
 *      headers keeps its frame here and hands rgk_accum_rgb / rgk_accum_count to rgk_render_round_device. ---- */
typedef struct rgk_accum rgk_accum;
int rgk_accum_create(uint32_t xres, uint32_t yres, int device, rgk_accum **out); /* zeroed */
void rgk_accum_destroy(rgk_accum *acc);
int rgk_accum_clear(rgk_accum *acc);
float *rgk_accum_rgb(rgk_accum *acc);      /* DEVICE pointer, 3 * xres * yres floats */
uint32_t *rgk_accum_count(rgk_accum *acc); /* DEVICE pointer, xres * yres */
int rgk_accum_download(const rgk_accum *acc, float *rgb, uint32_t *count); /* to host buffers (either may be NULL) */
int rgk_accum_upload(rgk_accum *acc, const float *rgb, const uint32_t *count);
/* dst += src (both on the same device): EXRTexture::Accumulate (src/texture.cpp:403-412).  What the root rank does with a
 * round's reduced sum -- see rgk_accum_reduce. */
int rgk_accum_add(rgk_accum *dst, const rgk_accum *src);
/* A digest of what the frame is rendered from (scene, camera, parameters; the host's choice of hash, 0 = none).  rgk_accum_save
 * stores it, rgk_accum_load refuses a file whose tag differs from the accumulator's (either side untagged: not compared). */
int rgk_accum_set_tag(rgk_accum *acc, uint64_t tag);

/* Raw-accumulator checkpoint (the reference cannot resume a frame): the accumulator with the two numbers
 * that make the next round continue the sequence -- rounds done and the running task counter `seedcount`
 * (src/render_driver.cpp:160,222).  Rendering k rounds, saving, loading and rendering m more gives the bits of k + m rounds. */
int rgk_accum_save(const rgk_accum *acc, const char *path, uint32_t rounds_done, uint32_t seedcount);
int rgk_accum_load(rgk_accum *acc, const char *path, uint32_t *rounds_done, uint32_t *seedcount);

/* ---- multi-GPU: one process per GPU, tiles dealt round-robin, ONE exchange per round ---- */
typedef struct rgk_comm rgk_comm;
#define RGK_COMM_ID_BYTES 128
/* Tile i of the centre-out list goes to rank i mod world_size (tiles keep their seeds: the image does not depend on
 * the number of GPUs).  Call with out == NULL for the count. */
int rgk_shard_tiles(const rgk_tile *tiles, uint32_t n_tiles, int rank, int world_size, rgk_tile *out, uint32_t *n_out);
/* RCCL communicator over the node's xGMI links.  Rank 0 makes the id and hands its 128 bytes to the other ranks by the
 * host's own means (a file, an environment variable, MPI, ...).  librccl is bound at run time: single-GPU hosts need none. */
int rgk_comm_get_unique_id(uint8_t id[RGK_COMM_ID_BYTES]);
int rgk_comm_create(const uint8_t id[RGK_COMM_ID_BYTES], int rank, int world_size, int device, rgk_comm **out);
void rgk_comm_destroy(rgk_comm *comm);
/* total_ob.Accumulate(output_buffer) under total_ob_mx (src/render_driver.cpp:177-182) across GPUs: in-place sum-reduce of
 * the per-GPU DEVICE accumulators to `root` (d_accum_count may be NULL when the host derives counts analytically).
 * Collective and blocking: every rank calls it once per round.  IN PLACE means: afterwards the root's buffer holds the sum
 * over all ranks and every other rank's buffer still holds its own contribution -- so what is reduced must be ONE ROUND's
 * accumulator (rgk_accum_clear before the round), which the root then adds to its frame total (rgk_accum_add).  Reducing a
 * buffer that keeps growing over the rounds would count the other ranks' earlier rounds again with every reduce. */
int rgk_accum_reduce(rgk_comm *comm, float *d_accum_rgb, uint32_t *d_accum_count, uint32_t xres, uint32_t yres, int root);

/* Scene::FindIntersectKdOtherThan (src/scene_intersect.cpp:211-327) for n rays.
 * rays: 8 floats each {ox,oy,oz, dx,dy,dz, near, far}; ignore: triangle id or -1. */
int rgk_trace_closest(rgk_scene *scene, uint32_t n, const float *rays, const int32_t *ignore,
                      rgk_hit *hits, rgk_counters *counters);

/* Scene::Visibility (src/scene.cpp:670-673) for n point pairs (3 floats each). */
int rgk_trace_visibility(rgk_scene *scene, uint32_t n, const float *a, const float *b,
                         uint8_t *visible, rgk_counters *counters);

/* BxDF::value(Vi, Vr, texUV) and BxDF::sample(Vi, texUV, sample) (src/bxdf/bxdf.hpp:38-43) of material mat[i], for n
 * inputs, in the local frame (+Z = shading normal).  Unit-level seams for the parity tests.  route 0: the generic code (every
 * material kind, mixes included); route 1: what the shading kernel runs for diffuse / LTC materials (texture colours and LTC
 * table entries fetched once and shared between value and sample).  Vi, Vr, out_*: 3 floats each; uv, u: 2 floats each. */
int rgk_bxdf_value(rgk_scene *scene, uint32_t n, uint32_t route, const uint32_t *mat, const float *Vi, const float *Vr,
                   const float *uv, float *out_rgb);
int rgk_bxdf_sample(rgk_scene *scene, uint32_t n, uint32_t route, const uint32_t *mat, const float *Vi, const float *uv,
                    const float *u, float *out_dir, float *out_weight, uint8_t *may_leak);
/* ReadableTexture::GetPixelInterpolated, GetSlopeRight, GetSlopeBottom (src/texture.cpp:35-102, src/texture.hpp:64-80) of
 * descriptor texture tex[i] (-1: EmptyTexture) at uv[i]. */
int rgk_texture_sample(rgk_scene *scene, uint32_t n, const int32_t *tex, const float *uv, float *rgb, float *slope_right,
                       float *slope_bottom);

/* ---- first-hit feature buffers and the guided denoiser (DESIGN.md "Feature buffers and the a-trous denoiser") ---- */

/* One primary ray per pixel of the listed tiles through the pixel CENTRE (sub-pixel offset (0.5, 0.5)), leaving from
 * camera->origin (the lens is ignored), near 0 / far 10000 as every camera ray; traced by the round's own closest-hit walker.
 * params supplies xres, yres and bumpmap_scale (the sampler is not used).  Planes are row-major from the top row, P = xres * yres;
 * pixels outside the tiles are not written.  Any output may be NULL.  DEVICE buffers on the scene's GPU; blocking.
 *   miss:  tri = -1, depth = 0, normal = albedo = 0
 *   hit:   tri = triangle id, depth = the ray's t, normal = the bump-tilted shading normal the integrator lights with (world
 *          space, NOT flipped towards the viewer); a vertex the integrator drops (NaN / zero face normal) has normal = albedo = 0
 *   albedo by material at the hit's uv: diffuse -> diffuse texture; ltc_* -> colour texture; ltc_*_diffuse -> diffuse + colour;
 *          mirror, dielectric, transparent -> (1, 1, 1); mix -> amount * albedo(m1) + (1 - amount) * albedo(m2), a mix inside a mix
 *          evaluated likewise and a third level as 0 (what the BxDF code does); emission does not enter.
 * Not while a round is in flight on this scene.  A call between two rounds of a frame changes nothing those rounds compute. */
int rgk_render_aov_device(rgk_scene *scene, const rgk_camera *camera, const rgk_params *params, const rgk_tile *tiles,
                          uint32_t n_tiles, float *d_albedo /*3P*/, float *d_normal /*3P*/, float *d_depth /*P*/, int32_t *d_tri /*P*/);
/* Same with HOST buffers (their contents are kept outside the tiles). */
int rgk_render_aov(rgk_scene *scene, const rgk_camera *camera, const rgk_params *params, const rgk_tile *tiles, uint32_t n_tiles,
                   float *albedo, float *normal, float *depth, int32_t *tri);

/* ---- feature planes that follow mirrors and glass to the first non-specular surface ----
 *
 * The planes of rgk_render_aov_device, but a pixel whose centre ray meets a mirror, a dielectric or a transparent surface follows
 * the chain of delta interactions the integrator's path takes and reports the first surface behind it.  Per pixel, float32,
 * contraction off, in this order.  Let U = (0x1.fffffep-1f, 0), T_0 = (1, 1, 1) and L_0 = 0.  ray_0 is the centre ray of
 * rgk_render_aov_device (pinhole copy of the camera, near 0, far 10000, no ignored triangle).  For hop k = 0, 1, ...:
 *   1. Trace ray_k with the round's own closest-hit walker.
 *        Miss: tri = -1, depth = 0, normal = albedo = 0, hops = k.  End.
 *   2. v = the integrator's vertex at the hit (position, face normal, uv, bump-tilted shading normal, local frame g2l) and
 *      L_{k+1} = L_k + t_k.
 *        A vertex the integrator drops (NaN / zero face normal): tri = tri_k, depth = L_{k+1}, normal = albedo = 0, hops = k.  End.
 *   3. TERMINAL means: tri = tri_k, depth = L_{k+1}, normal = v.lightN (world space), albedo = T_k * albedo(v.mat, v.uv) -- the
 *      albedo of rgk_render_aov_device, one multiply per channel -- hops = k.  End.
 *        The vertex is terminal when its TOP-LEVEL material kind is not mirror, dielectric or transparent (a mix ends the chain and
 *        reports its mixed albedo), and when k == max_hops.
 *   4. Otherwise (dirL, weight, may_leak) = the integrator's own BxDF sample of that kind at u = U, in the local frame:
 *        mirror: the reflection; transparent: straight through; dielectric: the refraction unless decide_and_rescale(U.x, R) picks
 *        the reflection (in effect: total internal reflection).
 *      dir = qrot(qinverse(v.g2l), dirL).  The integrator's leak rule: if !(dot(dir, faceN) * dot(Vr, faceN) > 0) && !may_leak its
 *      path would end here, and the vertex is terminal.
 *   5. T_{k+1} = T_k * weight.  ray_{k+1} is the ray the integrator continues with: origin v.pos + v.faceN * epsilon * 10 *
 *      (dirL.z < 0 ? -1 : 1), direction norm3(norm3(dir)), ignored triangle tri_k, near 0, far 10000.
 *      A continuation ray with a non-finite component is queued and traced like every other, as in a round: the walker records no
 *      hit for a ray with a NaN component, so the pixel ends at step 1 of hop k + 1 as a miss.
 * No roulette, no clamp, no throughput cut-off: only geometric ends.  max_hops == 0 gives the planes of rgk_render_aov_device
 * bit for bit and hops = 0 everywhere.  Queue order may vary from run to run, the planes do not.
 * Conventions of rgk_render_aov_device: any output may be NULL; pixels outside the tiles are not written; DEVICE buffers on the
 * scene's GPU; blocking; not while a round is in flight on this scene; a call between two rounds of a frame changes nothing those
 * rounds compute.  Arguments are checked before the scene or the device is touched; max_hops > RGK_AOV_MAX_HOPS is RGK_ERR_INVALID. */
#define RGK_AOV_MAX_HOPS 8
int rgk_render_aov_chain_device(rgk_scene *scene, const rgk_camera *camera, const rgk_params *params, const rgk_tile *tiles,
                                uint32_t n_tiles, uint32_t max_hops, float *d_albedo /*3P*/, float *d_normal /*3P*/,
                                float *d_depth /*P*/, int32_t *d_tri /*P*/, uint8_t *d_hops /*P*/);
/* Same with HOST buffers (their contents are kept outside the tiles). */
int rgk_render_aov_chain(rgk_scene *scene, const rgk_camera *camera, const rgk_params *params, const rgk_tile *tiles,
                         uint32_t n_tiles, uint32_t max_hops, float *albedo, float *normal, float *depth, int32_t *tri,
                         uint8_t *hops);

/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) of the accumulator's image, guided by the feature planes.
 * c = accum_rgb / accum_count (0 where the count is 0); with `demodulate`, c is divided per channel by (albedo > 0 ? albedo : 1)
 * before the filter and multiplied back after it.  Iteration i = 0 .. iterations - 1, step s = 2^i: 5 x 5 taps q = p + s * (dx, dy)
 * (dy outer, dx inner, both -2 .. 2; taps outside the frame are skipped), h = {1/16, 1/4, 3/8, 1/4, 1/16},
 *   w  = (((h[dy] * h[dx]) * wn) * wz) * wc
 *   wn = max(0, n_p . n_q), squared normal_power_log2 times
 *   wz = 1 / (1 + r * r),  r = |z_p - z_q| / (sigma_depth * (z_p + z_q) + 1e-20f)
 *   wc = 1 / (1 + |c_p - c_q|^2 / sigma_i^2),  sigma_i = sigma_color * 2^-i      (sigma_color: in the image's radiance units)
 *   out_p = sum(w * c_q) / sum(w)
 * A pixel whose normal is zero (miss, dropped vertex) passes through unchanged and is never a tap of another pixel.
 * iterations == 0: out = c (nothing is filtered, nothing is demodulated).  Only + - * / max in float32, no contraction: the
 * same operations in the same order give the same bits on a CPU.  iterations, normal_power_log2 <= 16; sigma_color > 0,
 * sigma_depth >= 0.  Arguments are checked before the scene or the device is touched. */
typedef struct rgk_denoise_params {
    uint32_t iterations;
    float sigma_color, sigma_depth;
    uint32_t normal_power_log2;
    uint32_t demodulate;
} rgk_denoise_params;
/* accum_rgb / accum_count as a round leaves them and the three feature planes of rgk_render_aov_device (d_albedo may be NULL
 * when demodulate == 0); out_rgb: 3P floats (not one of the inputs).  All DEVICE pointers on the scene's GPU; whole frame; blocking. */
int rgk_denoise_device(rgk_scene *scene, uint32_t xres, uint32_t yres, const float *d_accum_rgb, const uint32_t *d_accum_count,
                       const float *d_albedo, const float *d_normal, const float *d_depth, const rgk_denoise_params *params,
                       float *d_out_rgb);

/* HIP-event times of the launches of the LAST feature pass (which = 0: pixel list + ray generation, walker, gather) or denoise
 * call (which = 1: preparation, one per iteration, finish), variance-guided denoise call (which = 2: preparation, prefilter, one
 * per iteration, finish [, variance copy]), noise estimate (which = 3: the tile sums) or round fold (which = 4: the copy of the tile
 * list and the fold) on this scene, in ms; recorded only while
 * the tuning key "time_post" is 1. *n: in, room in ms; out, entries the call had (those that fit are written).
 * which = 5: the temporal pair -- {the last rgk_temporal_reproject_device, the last rgk_temporal_blend_device}, one launch each;
 * two entries once either has run with "time_post" on, 0 ms for the one that has not.
 * which = 6: the last rgk_render_aov_chain[_device] -- pixel list + ray generation, then {walker, k_aov_hop} per hop 0 .. max_hops.
 * which = 7: the last rgk_upsample_device -- {k_us_prepare, k_us_gather}.
 * which = 8: the last rgk_remodulate_device -- {k_remodulate}.
 * which = 9: the last rgk_render_round_demod_device -- {its k_demod_divisor launches, its k_resolve_demod launches}, each summed
 * over the round's passes (the round's other launches: rgk_counters with RGK_FLAG_TIME_KERNELS).
 * which = 10: the last rgk_display_measure_device -- {the clear of the histogram, k_display_hist}.
 * which = 11: the last rgk_display_encode_device -- {k_display_encode}.
 * which = 12: the last rgk_output_write_exr_device -- {k_out_max and its fold, or 0 with a given scale; k_out_pack_exr}.
 * which = 13: the last rgk_output_write_png_device -- {k_out_pack_png, k_out_png_sums}. */
int rgk_scene_get_post_timing(const rgk_scene *scene, uint32_t which, double *ms, uint32_t *n);

/* ---- noise estimate from two half-buffers and the variance-guided filter (DESIGN.md "Half-buffer noise estimate") ----
 *
 * The caller keeps, beside the frame's accumulator {S, n}, a second one {S_B, n_B} that received the odd rounds only (n_B <= n).
 * Per pixel, in float32, only + - * / max, no contraction, in the order written:
 *   n_A = n - n_B,  a = (S - S_B) / n_A,  b = S_B / n_B,  c = S / n  (0 where n == 0)
 *   estimable: n_A > 0 and n_B > 0;  f = ((float)n_A * (float)n_B) / ((float)n * (float)n)
 *   v = ((h.r^2 + h.g^2) + h.b^2) * f,  h = a - b;  0 where the pixel is not estimable
 * v is the variance of c (|a - b|^2 / 4 for equal halves).
 *
 * Workspace: both entries use the scene's post-processing planes -- the two colour planes and the guide plane rgk_denoise_device
 * uses, and a tile array of their own -- and nothing else: no buffer, list or counter a round reads or writes.  A call between two
 * rounds of a frame changes nothing those rounds compute; a call overwrites what an earlier post-processing call left in the planes
 * (every entry is blocking and has delivered its outputs by then).  Not while a round is in flight on this scene.  Arguments are
 * checked before the scene or the device is touched. */

/* Statistics of one tile of tile_size x tile_size pixels (ragged at the right and bottom edges) over its ESTIMABLE pixels:
 * sum_var = sum of v, sum_sq = sum of ((c.r^2 + c.g^2) + c.b^2), accumulated in double from the float32 per-pixel terms (no scene
 * features, nothing demodulated).  A frame's relative noise is sqrt(sum of sum_var / sum of sum_sq), tiles added in row-major order:
 * an estimate of |c - converged image| / |c|. */
typedef struct rgk_noise_tile { double sum_var, sum_sq; uint64_t n_estimable; } rgk_noise_tile;
/* per-tile statistics of a frame; tiles: host array of ceil(xres/ts)*ceil(yres/ts), row-major; d_variance (P floats, raw v) may be NULL.
 * The other pointers are DEVICE pointers on the scene's GPU; tile_size >= 1; whole frame; blocking. */
int rgk_noise_estimate_device(rgk_scene *scene, uint32_t xres, uint32_t yres, uint32_t tile_size,
                              const float *d_accum_rgb, const uint32_t *d_accum_count, const float *d_half_rgb,
                              const uint32_t *d_half_count, rgk_noise_tile *tiles, float *d_variance);

/* The a-trous filter of rgk_denoise_device with the colour weight taken from the pixels' own variances instead of one sigma_color.
 * Guide plane, wn, wz, h[], tap order, the live-pixel rule (zero normal: passes through, never a tap), taps outside the frame and
 * "iterations == 0: out = c" are rgk_denoise_device's.  What differs:
 *   div = albedo > 0 ? max(albedo, albedo_floor) : 1 per channel when `demodulate`; a, b and c are each divided by div, v is computed
 *   from the demodulated a and b, and the result is multiplied back by the same div
 *   prefilter, 5 x 5, step 1:  var_p = sum((wn * wz) * v_q) / sum(wn * wz) over the live taps (a pixel that is not live keeps v_p)
 *   iteration i, step 2^i, k2 = sigma_k * sigma_k:
 *     wc = 1 / (1 + d2 / (k2 * (var_p + var_q) + 1e-20f)),  d2 = |c_p - c_q|^2
 *     w  = (((h[dy] * h[dx]) * wn) * wz) * wc
 *     c'_p = sum(w * c_q) / sum(w),   var'_p = sum((w * w) * var_q) / (sum(w) * sum(w))
 * out_variance: the variance plane after the last iteration -- of the filtered image, in the space the filter ran in (divided by
 * div^2 in effect when `demodulate`); with iterations == 0 it is the raw v.  sigma_k > 0, albedo_floor >= 0, sigma_depth >= 0, all
 * finite; iterations, normal_power_log2 <= 16. */
typedef struct rgk_denoise_var_params { uint32_t iterations; float sigma_k, sigma_depth; uint32_t normal_power_log2, demodulate; float albedo_floor; } rgk_denoise_var_params;
/* d_albedo may be NULL when demodulate == 0; out_rgb: 3P floats, out_variance: P floats or NULL, neither one of the inputs.  All DEVICE
 * pointers on the scene's GPU; whole frame; blocking. */
int rgk_denoise_variance_device(rgk_scene *scene, uint32_t xres, uint32_t yres, const float *d_accum_rgb, const uint32_t *d_accum_count,
                                const float *d_half_rgb, const uint32_t *d_half_count, const float *d_albedo, const float *d_normal,
                                const float *d_depth, const rgk_denoise_var_params *params, float *d_out_rgb,
                                float *d_out_variance /* P, the filtered image's variance, may be NULL */);

/* ---- adaptive tile sampling (DESIGN.md "Adaptive tile sampling") ----
 *
 * Which tiles of a frame the next round still renders, from the noise estimate's per-tile statistics.  HOST only: no scene, no
 * device.  tiles / visits / live: ceil(xres/ts)*ceil(yres/ts) entries, row-major as rgk_noise_estimate_device writes them;
 * visits[t]: rounds in which tile t was rendered.  In double, the tiles added in row-major order:
 *   SV = sum of sum_var,  SQ = sum of sum_sq,  NE = sum of n_estimable
 *   *done  = NE > 0 and SV <= target^2 * SQ       (the frame's relative noise is <= target), or no tile is live
 *   live[t] = visits[t] < min_visits  or  n_estimable_t == 0  or  sum_var_t > (target^2 * SQ) * (n_estimable_t / NE)
 * i.e. a tile stays live while its mean per-pixel variance is above the frame-wide per-pixel allowance.  The rule keeps no state: a
 * tile that is not live is left out of the next round only and judged again after it.  target finite and >= 0; min_visits >= 2 (a
 * tile is not estimable before its second visit).  Arguments are checked first; n_live and done may be NULL. */
typedef struct rgk_adapt_params { float target; uint32_t min_visits; } rgk_adapt_params;
int rgk_adapt_select(const rgk_noise_tile *tiles, const uint32_t *visits, uint32_t xres, uint32_t yres, uint32_t tile_size,
                     const rgk_adapt_params *params, uint8_t *live, uint32_t *n_live, uint32_t *done);

/* Folds a round rendered into a per-round accumulator {round} -- all zero outside the pixels the round rendered -- into the frame's
 * accumulator {total} and, tile by tile, into the half-buffer {half}.  For every pixel of every listed tile, rgb and count alike:
 *   total += round;   where to_half[i] != 0: half += round;   round = 0
 * in float32 / uint32, one addition per element.  Pixels outside the listed tiles are neither read nor written in any of the six
 * planes, so a round buffer that starts all zero is all zero again after the fold of the tiles rendered into it and never needs a
 * whole-frame clear.  Tiles must lie in the frame, be non-empty and not overlap each other; the six planes must be six different
 * buffers: checked on the host before the scene or the device is touched (the seed of a tile is not read).  tiles / to_half: HOST
 * arrays of n_tiles; the planes: DEVICE pointers on the scene's GPU, 3P floats / P counts.  One launch on the scene's stream; blocking.
 * Not while a round is in flight on this scene.  Uses a tile buffer of its own and nothing a round reads or writes. */
int rgk_round_fold_device(rgk_scene *scene, uint32_t xres, uint32_t yres, const rgk_tile *tiles, uint32_t n_tiles,
                          const uint8_t *to_half /* n_tiles */, float *d_round_rgb, uint32_t *d_round_count, float *d_total_rgb,
                          uint32_t *d_total_count, float *d_half_rgb, uint32_t *d_half_count);

/* ---- temporal reuse for a moving camera over static geometry (DESIGN.md "Temporal reuse") ----
 *
 * A history image {h.rgb, L} -- the demodulated colour a pixel has gathered over the frames before this one and the number of frames
 * in it, a float -- is carried from the previous frame's pixels to the current frame's (reproject) and the current frame's samples
 * are blended into it (blend).  Both entries: all pointers DEVICE pointers on the scene's GPU, planes row-major from the top row,
 * P = xres * yres; whole frame; one launch on the scene's stream; blocking.  No output may be one of the inputs (or another output).
 * Arguments are checked before the scene or the device is touched; not while a round is in flight on this scene.  They use no
 * buffer, list or counter a round reads or writes, and no workspace of the scene at all.  Everything below is float32, only
 * + - * / max min sqrt floor, no contraction, in the order written; a . b = (a.x * b.x + a.y * b.y) + a.z * b.z, len(a) = sqrt(a . a);
 * sums over taps start at 0 and add the counted taps in tap order. */
typedef struct rgk_temporal_params {
    float plane_tol;     /* >= 0: a tap's surface plane may be this far from the pixel's point, as a share of its distance */
    float normal_cos;    /* in [-1, 1]: the smallest n_p . n_q a tap may have */
    float alpha_min;     /* in (0, 1]: the smallest weight the current frame gets */
    float max_len;       /* >= 1: where the history length stops growing */
    uint32_t demodulate; /* blend only */
    float albedo_floor;  /* >= 0, blend only: rgk_denoise_var_params' floor on the divisor */
} rgk_temporal_params;
/* Per pixel p = (x, y) of the current frame.  The lens of both cameras is ignored, as by rgk_render_aov_device, whose depth /
 * normal / tri planes for the two cameras the six feature planes are.
 *   (o, d) = the ray rgk_render_aov_device traces for p through cam_cur;  hit = tri_cur[p] >= 0
 *   x_p = o + d * z_p;  v = hit ? x_p - o_prev : d         (a miss is a point at infinity: sky is reprojected by direction)
 * No history -- hist_len = 0, hist_rgb = 0 -- for
 *   a hit whose triangle's top-level material is mirror, dielectric or transparent (its radiance depends on the view; a triangle
 *   id that is not the scene's gets none either), a hit whose normal is zero, and !(q > 0) with N = cam_prev->direction, q = v . N.
 * Else into the previous frame, vs / vx / vy = cam_prev's viewscreen, viewscreen_x, viewscreen_y:
 *   s = ((vs - o_prev) . N) / q;   w = (o_prev + v * s) - vs;   a = (w . vx) / (vx . vx);   b = (w . vy) / (vy . vy)
 *   fx = a * xres - 0.5f;  fy = b * yres - 0.5f;   no history unless fx > -1 && fx < xres && fy > -1 && fy < yres
 *   ix = (int)floor(fx), tx = fx - ix, likewise y; taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) with the weights
 *   (1-tx)*(1-ty), tx*(1-ty), (1-tx)*ty, tx*ty
 * A tap q counts when it is inside the frame, hist_len_prev[q] > 0, and
 *   miss:  tri_prev[q] < 0
 *   hit:   tri_prev[q] >= 0,  n_p . n_q >= normal_cos,  |(x_p - (o_prev + d_q * z_q)) . n_q| <= plane_tol * len(v)
 *          (d_q: cam_prev's ray through the centre of q -- the distance to the previous surface's plane)
 *   hist_rgb = sum(w * c_q) / sum(w),  hist_len = sum(w * len_q) / sum(w);  sum(w) == 0: no history.
 * Every member of params is checked by both entries (the ranges beside the members, all finite), whichever of them it reads. */
int rgk_temporal_reproject_device(rgk_scene *scene, uint32_t xres, uint32_t yres, const rgk_camera *cam_cur, const rgk_camera *cam_prev,
                                  const float *d_depth_cur /*P*/, const float *d_normal_cur /*3P*/, const int32_t *d_tri_cur /*P*/,
                                  const float *d_depth_prev, const float *d_normal_prev, const int32_t *d_tri_prev,
                                  const float *d_hist_rgb_prev /*3P*/, const float *d_hist_len_prev /*P floats*/,
                                  const rgk_temporal_params *params, float *d_hist_rgb /*3P out*/, float *d_hist_len /*P out*/);
/* Per pixel: c = accum_rgb / accum_count (0 where the count is 0); per channel div = demodulate ? (albedo > 0 ? max(albedo,
 * albedo_floor) : 1) : 1;  m = c / div;  h = hist_rgb, L = hist_len.
 *   L > 0:  alpha = max(1 / (L + 1), alpha_min);  m' = (m - h) * alpha + h;  L' = min(L + 1, max_len)
 *   else:   m' = m;  L' = 1
 *   a pixel whose count is 0 keeps its history unblended: m' = h, L' = L
 *   out_hist_rgb = m' (demodulated: the next frame's history), out_hist_len = L', out_rgb = m' * div (the image to filter or write)
 * d_albedo may be NULL when demodulate == 0. */
int rgk_temporal_blend_device(rgk_scene *scene, uint32_t xres, uint32_t yres, const float *d_accum_rgb, const uint32_t *d_accum_count,
                              const float *d_albedo, const float *d_hist_rgb, const float *d_hist_len,
                              const rgk_temporal_params *params, float *d_out_hist_rgb /*3P*/, float *d_out_hist_len /*P*/,
                              float *d_out_rgb /*3P*/);

/* ---- guided upsampling of a low-resolution render (DESIGN.md "Guided upsampling") ----
 *
 * The accumulator of a render on a low grid (xl x yl, cam_low) reconstructed on a full grid (xres x yres, cam), guided by the feature
 * planes rgk_render_aov_device makes for the two cameras and re-modulated with the full grid's albedo.  The two cameras need not
 * have the same view rectangle.  All pointers DEVICE pointers on the scene's GPU, planes row-major from the top row, P = xres * yres,
 * Pl = xl * yl; whole frame; two launches on the scene's stream; blocking.  No output may be one of the inputs (or the other
 * output).  Arguments are checked before the scene or the device is touched: every member of params (the ranges beside the members,
 * all finite), xl, yl, xres, yres in 1 .. 65535, cam->xsize == xres, cam->ysize == yres, cam_low->xsize == xl, cam_low->ysize == yl.
 * Not while a round is in flight on this scene.  It uses record planes of its own and no buffer, list or counter a round reads or
 * writes; no scene data is read.  d_albedo and d_low_albedo may be NULL when demodulate == 0.  The lens of both cameras is ignored.
 * Everything below is float32, only + - * / max min sqrt floor, no contraction, in the order written;
 * a . b = (a.x * b.x + a.y * b.y) + a.z * b.z, len(a) = sqrt(a . a); sums over taps start at 0 and add the counted taps in tap order.
 *
 * Per low pixel q:
 *   c_q = S_q / n_q (0 where n_q == 0), live_q = n_q > 0
 *   per channel div_q = demodulate ? (a_q > 0 ? max(a_q, albedo_floor) : 1) : 1,  m_q = c_q / div_q
 *   flat_q: all three normal components == 0 (a miss or a dropped vertex)
 *   x_q = o_low + d_q * z_q, (o_low, d_q) the ray rgk_render_aov_device traces for q through cam_low
 * Per full pixel p = (x, y):
 *   1. (o, d) = the ray rgk_render_aov_device traces for p through cam; flat_p as above; x_p = o + d * z_p;
 *      v = flat_p ? d : x_p - o_low      (a flat pixel is carried by direction, like sky in the reprojection)
 *   2. into the low grid with the formulas of rgk_temporal_reproject_device, cam_low for cam_prev: N = cam_low->direction,
 *      qd = v . N;  s = ((vs - o_low) . N) / qd;  w = (o_low + v * s) - vs;  a = (w . vx) / (vx . vx);  b = (w . vy) / (vy . vy);
 *      fx = a * xl - 0.5f;  fy = b * yl - 0.5f.
 *      If !(qd > 0), or unless fx > -2 && fx < xl + 1 && fy > -2 && fy < yl + 1 (false for NaN): out = 0, support = 0, end.
 *   3. ix = (int)floor(fx), tx = fx - ix, likewise y.  A tap q COUNTS when it is inside the low frame, live_q, flat_q == flat_p and,
 *      for a non-flat p,  n_p . n_q >= normal_cos  and  |(x_q - x_p) . n_p| <= plane_tol * len(x_p - o).
 *   4. ring 1: taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) with the weights (1-tx)*(1-ty), tx*(1-ty), (1-tx)*ty, tx*ty;
 *      W = sum(w), A = sum(w * m_q).  If W > 0: m = A / W, support = 1.
 *   5. else ring 2: the 16 taps ix-1 .. ix+2 x iy-1 .. iy+2 (dy outer, dx inner), the same counting rule,
 *      w = 1 / (1 + ((fx - qx)^2 + (fy - qy)^2)).  If W > 0: m = A / W, support = 2.
 *   6. else nearest: q0 = (min(max((int)floor(fx + 0.5f), 0), xl - 1), likewise y), out = c_q0 (plain: 0 when not live, not
 *      demodulated, not re-modulated), support = 0, end.
 *   7. out = m * div_p, div_p formed from the full-resolution albedo by the rule for div_q. */
typedef struct rgk_upsample_params {
    float plane_tol;     /* >= 0: a tap's point may be this far from the pixel's surface plane, as a share of the pixel's distance */
    float normal_cos;    /* in [-1, 1]: the smallest n_p . n_q a tap may have */
    uint32_t demodulate;
    float albedo_floor;  /* >= 0: the floor on the divisor, as in rgk_temporal_params */
} rgk_upsample_params;
int rgk_upsample_device(rgk_scene *scene, uint32_t xres, uint32_t yres, const rgk_camera *cam,
                        const float *d_albedo /*3P*/, const float *d_normal /*3P*/, const float *d_depth /*P*/,
                        uint32_t xl, uint32_t yl, const rgk_camera *cam_low,
                        const float *d_low_accum_rgb /*3Pl*/, const uint32_t *d_low_accum_count /*Pl*/,
                        const float *d_low_albedo, const float *d_low_normal, const float *d_low_depth,
                        const rgk_upsample_params *params,
                        float *d_out_rgb /*3P*/, uint8_t *d_out_support /*P, may be NULL*/);

/* ---- per-sample demodulated accumulation (DESIGN.md "Per-sample demodulated accumulation") ----
 *
 * The post stages above divide a pixel's MEAN radiance by the albedo of the one ray through the pixel centre, which is the
 * irradiance only where the texture is constant over the pixel's footprint.  A demodulated round keeps, beside the accumulator
 * S = sum of L_s, two more planes of 3P floats:
 *   D = sum over samples s of L_s / div_s      (d_demod_rgb)
 *   A = sum over samples s of div_s            (d_div_rgb, the anti-aliased divisor: D / n is multiplied back with A / n)
 * where div_s belongs to sample s's OWN camera ray -- pixel jitter and lens included, the ray the round's first walk traced.
 * Float32, only + * / max, no contraction, sums in sample order.  Per path slot of a pass (pixel j, sample s):
 *   (o, d) = the camera ray of the slot; h = its first hit as the bounce-0 walk left it
 *   a miss: div = (1, 1, 1).  Else the path vertex at h (hit point, interpolated normal, uv, as the integrator forms it, with
 *   bumpmap_scale); a vertex the integrator drops (no usable normal): div = (1, 1, 1).  Else a = the albedo of the vertex's material
 *   at uv as the feature pass defines it above (mixes to two levels, mirror / dielectric / transparent = 1), and per channel
 *   div_c = a_c > 0 ? max(a_c, albedo_floor) : 1
 *   v_s = the value the round adds to S for the sample: clamped to params->clamp, then NaN and negatives set to 0 (the clamp comes
 *   before the division)
 * Per pixel, in sample order: Dsum += v_s / div_s, Asum += div_s, both from 0, carried across the sample passes of a round the way the
 * radiance sum is; with the pixel's last sample d_demod_rgb[p] += Dsum and d_div_rgb[p] += Asum, one addition per element.
 *
 * d_accum_rgb, d_accum_count and *counters receive exactly what the plain round entry gives them, bit for bit: the two entries share
 * one body, and the plain entry launches, allocates and branches as it did before this one existed.  The extra launches -- the
 * divisors behind the first walk, a second resolve behind the first -- are not entered in counters.  Workspace: 16 B per path of the
 * batch and 32 B per pixel of the round, allocated by the first demodulated round of a scene.
 * RGK_ERR_UNSUPPORTED: params->reverse > 0 (a light-tracing splat has no path slot to demodulate), depth == 0 (no first hit), and
 * everything the plain entry refuses.  RGK_ERR_INVALID: a NULL plane, two of the four planes the same buffer, albedo_floor negative,
 * NaN or infinite, and everything the plain entry refuses as invalid.  All DEVICE pointers on the scene's GPU; blocking. */
int rgk_render_round_demod_device(rgk_scene *scene, const rgk_camera *camera, const rgk_params *params,
                                  const rgk_tile *tiles, uint32_t n_tiles, float *d_accum_rgb, uint32_t *d_accum_count,
                                  float *d_demod_rgb /*3P, +=*/, float *d_div_rgb /*3P, +=*/, float albedo_floor,
                                  rgk_counters *counters);
/* out = in * dbar per pixel and channel, float32, one multiplication:
 *   d_div_count given:  dbar = n > 0 ? A / (float)n : 1      (d_div_rgb is the A plane of demodulated rounds, n its sample count)
 *   d_div_count NULL:   dbar = a > 0 ? max(a, albedo_floor) : 1      (d_div_rgb is an albedo plane of the feature pass)
 * in: 3P floats, e.g. D / n after a filter that ran with demodulate == 0.  The output is not one of the inputs.  albedo_floor >= 0 and
 * finite (read in the second form only, checked in both).  All DEVICE pointers on the scene's GPU; whole frame; one launch on the
 * scene's stream; blocking.  Arguments are checked before the scene or the device is touched; not while a round is in flight on this
 * scene.  Uses no workspace.  The launch's time is which = 8 of the post timing query above. */
int rgk_remodulate_device(rgk_scene *scene, uint32_t xres, uint32_t yres, const float *d_in_rgb /*3P*/,
                          const float *d_div_rgb /*3P*/, const uint32_t *d_div_count /* P, or NULL: d_div_rgb is an albedo plane */,
                          float albedo_floor, float *d_out_rgb /*3P*/);

/* ---- display output: auto exposure, tone mapping, sRGB bytes (DESIGN.md "Display output") ----
 *
 * From a radiance image to a picture a viewer shows: a histogram of the luminances (measure, device), an exposure and a white point
 * from it (solve, host, integers up to the last step), and per pixel the exposure, a tone curve and the sRGB transfer function to
 * 8 bits (encode, device).  Everything on the device is float32 with + - * / min max and integer operations on float bit patterns,
 * no contraction and no transcendental function, so a numpy restatement in the same order gives the same bits
 * (tests/display_ref.py); bits of a float f: its 32-bit pattern as an unsigned integer.
 *
 * Per pixel, the input colour:
 *   with a count plane:  c = rgb / (float)count per channel, 0 where the count is 0
 *   d_count == NULL (an image that is a mean already: a denoised or an upsampled one):  c = rgb
 *   then per channel  c = c > 0 ? c : 0          (NaN and negatives become 0; +inf stays)
 *   Y = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b
 *
 * Measure: a 256-bin histogram of Y, 8 bins per octave over [2^-20, 2^12), from the bits:
 *   Y > 0 (+inf too):  bin = clamp((int)(bits of Y >> 20) - ((127 - 20) << 3), 0, 255), hist[bin] += 1
 *   Y == 0:            not binned, n_dark += 1
 * so luminances below 2^-20 fall into bin 0 and those from 2^12 on into bin 255.  Lower edge of a bin: the float whose bits are
 * (bin + ((127 - 20) << 3)) << 20; upper edge: the lower edge of bin + 1 (4096 for bin 255).  Counts are uint32, added as
 * integers: the histogram does not depend on the order the pixels are visited in.
 *
 * Solve, from the histogram alone:  N = sum of hist (n_lit);  N == 0: y_median = y_white = 0, exposure 1, white 1 -- unless fixed
 * ones are given, below.  Else, in 64-bit integers, rank_m = (N + 1) / 2 and rank_w = max(1, (N * white_permille + 999) / 1000);
 * the bin holding rank r is the first bin b whose running sum hist[0] + .. + hist[b] reaches r.
 *   y_white  = the upper edge of the bin holding rank_w
 *   y_median = lo + (hi - lo) * (((float)(rank_m - before) - 0.5f) / (float)hist[b]),  b the bin holding rank_m, lo / hi its edges,
 *              before = hist[0] + .. + hist[b - 1]
 *   exposure = params->exposure > 0 ? params->exposure : key / y_median
 *   white    = params->white > 0 ? params->white : max(exposure * y_white, 1)
 *
 * Encode, per channel:  x = min(exposure * c, 65504.0f), and the operator takes x to v:
 *   RGK_DISPLAY_LINEAR    v = min(x, 1)
 *   RGK_DISPLAY_REINHARD  L = the luminance of x by the formula of Y;  s = (1 + L / (white * white)) / (1 + L);  v = min(x * s, 1)
 *   RGK_DISPLAY_FILMIC    v = min((x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f), 1)
 *   byte = the number of k in 1 .. 255 with v >= T[k]
 * T is the table of the display entry below: T[0] = 0, T[k] = (float)srgb_to_linear((k - 0.5) / 255) for k = 1 .. 255, built once
 * on the host in double (srgb_to_linear(s) = s <= 0.04045 ? s / 12.92 : pow((s + 0.055) / 1.055, 2.4)): the thresholds at which
 * the rounded sRGB byte changes.  The table IS the transfer function here; the device only compares against it.  Output: one uint32
 * per pixel whose bytes in memory order are R, G, B, 255. */
#define RGK_DISPLAY_LINEAR 0
#define RGK_DISPLAY_REINHARD 1
#define RGK_DISPLAY_FILMIC 2
typedef struct rgk_display_params {
    uint32_t op;             /* RGK_DISPLAY_* */
    float exposure;          /* > 0: this scale; <= 0: automatic, key / y_median.  Finite */
    float key;               /* > 0, finite: the value the median luminance is taken to (0.18) */
    uint32_t white_permille; /* 1 .. 1000: the share of the lit pixels at or below the white point (995) */
    float white;             /* > 0: this white point for RGK_DISPLAY_REINHARD; <= 0: from the measurement.  Finite */
} rgk_display_params;
typedef struct rgk_display_stats {
    uint32_t hist[256];
    uint32_t n_lit, n_dark;  /* pixels binned, pixels with Y == 0 */
    float y_median, y_white, exposure, white;
} rgk_display_stats;
/* T: 256 floats, strictly increasing; the library's own storage, valid for the life of the process.  No device is touched. */
const float *rgk_display_table(void);
/* The solve above on a host histogram of 256 counts; fills every member of *stats (hist and n_dark copied).  HOST only: no scene,
 * no device.  RGK_ERR_INVALID: a NULL pointer, op none of the three, key not finite and > 0, exposure or white not finite,
 * white_permille outside 1 .. 1000, counts whose sum does not fit 32 bits. */
int rgk_display_solve(const uint32_t *hist /*256*/, uint32_t n_dark, const rgk_display_params *params, rgk_display_stats *stats);
/* Measure + solve of a whole frame: d_rgb 3P floats, d_count P counts or NULL, DEVICE pointers on the scene's GPU, P = xres * yres,
 * row-major from the top row; *stats is host memory.  The histogram buffer is the scene's own, cleared on the scene's stream before
 * the one launch that fills it; blocking.  Arguments are checked before the scene or the device is touched (what the solve
 * refuses, NULL scene / d_rgb / stats, xres, yres in 1 .. 65535); not while a round is in flight on this scene.  Uses no buffer, list
 * or counter a round reads or writes. */
int rgk_display_measure_device(rgk_scene *scene, uint32_t xres, uint32_t yres, const float *d_rgb /*3P*/,
                               const uint32_t *d_count /* P, or NULL: d_rgb is a mean */, const rgk_display_params *params,
                               rgk_display_stats *stats);
/* Encode of a whole frame with params->op, stats->exposure and stats->white (no other member of *stats is read; a caller may fill
 * the two by hand): d_out_rgba P uint32 words, a DEVICE pointer, neither d_rgb nor d_count.  One launch on the scene's stream; blocking.
 * Checked first, as above, and: stats->exposure and stats->white finite and > 0.  The table is uploaded to a buffer of the scene
 * by the scene's first call. */
int rgk_display_encode_device(rgk_scene *scene, uint32_t xres, uint32_t yres, const float *d_rgb /*3P*/,
                              const uint32_t *d_count /* P, or NULL */, const rgk_display_params *params,
                              const rgk_display_stats *stats, uint32_t *d_out_rgba /*P*/);

/* The pinned transcendental functions of the path (include/rgk_libm.h) evaluated on the device, for the test that the GPU
 * and the CPU produce the same bits: fn 0 sin, 1 cos, 2 acos, 3 asin, 4 atan2(a[i], b[i]) (b may be NULL otherwise). */
int rgk_libm_eval(int fn, uint32_t n, const float *a, const float *b, float *out);

/* Sampler::Get1D / Get2D of the build's Halton sampler evaluated on the device:
 * out[2*i..] = sample of (seed[i], index[i], dim[i]); is2d selects Get2D. */
int rgk_sampler_eval(uint32_t n, const uint32_t *seed, const uint32_t *index,
                     const uint32_t *dim, int is2d, float *out);

/* ---- output path: what RenderFrame does with total_ob after each round ---------------------- */

/* EXRTexture::Normalize followed by the GetPixel that Write applies (src/texture.cpp:349-354,376-400,
 * src/render_driver.cpp:233,245): out_rgb[p] = (accum_rgb[p] * val) / accum_count[p], 0 where the count is 0.
 * output_scale <= 0 ("auto", the reference's default, config.cpp:303-311): val = 1 / (largest channel of
 * accum/count), so the brightest channel becomes 1.  Host buffers; *scale_used receives val (may be NULL). */
int rgk_output_normalize(const float *accum_rgb, const uint32_t *accum_count, uint32_t xres, uint32_t yres,
                         float output_scale, float *out_rgb, float *scale_used);

/* EXRTexture::Write (src/texture.cpp:356-374): a scan-line OpenEXR file of half-float R, G, B from rgb
 * (xres * yres * 3 floats, row-major from the top row) and A = 1.  float -> half is OpenEXR's conversion (round
 * to nearest even, overflow to infinity).  Written uncompressed; the reference's RgbaOutputFile default is PIZ --
 * the same pixels in another container encoding. */
int rgk_output_write_exr(const char *path, uint32_t xres, uint32_t yres, const float *rgb);

/* An 8-bit truecolour PNG (colour type 2) of rgba -- xres * yres words as rgk_display_encode_device writes them, HOST memory; bytes
 * R, G, B of each word are stored, the fourth is dropped.  Filter 0 on every row; the zlib stream is stored (uncompressed)
 * deflate blocks of at most 65535 bytes, CRC-32 and Adler-32 computed here: no dependency, as the EXR writer above has none, and
 * 3 bytes per pixel on disk.  One IDAT chunk: the stream must stay below 2^31 bytes (about 26,700 x 26,700 pixels).
 * RGK_ERR_INVALID: a NULL pointer, an empty image, a side above 2^31 - 1, an image beyond that size, a path that cannot be
 * opened; RGK_ERR_DEVICE: a short write. */
int rgk_output_write_png(const char *path, uint32_t xres, uint32_t yres, const uint32_t *rgba);

/* float -> IEEE half bits exactly as the writer stores them (exposed for the tests). */
uint16_t rgk_float_to_half(float v);

/* ---- output path on the device (DESIGN.md "Output files made on the device") ----
 * The two files above from DEVICE memory on the scene's GPU, byte for byte what the host writers produce from host copies: the
 * normalisation, the halves and the scan-line blocks, or the IDAT payload and the pieces of its two checksums, are made by kernels
 * on the scene's stream; the finished bytes reach a pinned buffer of the scene in one copy, the host writes the few bytes around
 * them there, and the file leaves in one fwrite.  Blocking; not while a round is in flight on this scene; arguments are checked
 * before the scene, the device or the file is touched.  Each scene keeps one device byte buffer and one pinned host buffer for both
 * entries, grown on demand and freed with the scene; nothing a round reads or writes is used, so a call between two rounds of a
 * frame changes nothing those rounds compute.  RGK_ERR_INVALID: a NULL scene, path or image, xres or yres outside 1 .. 65535, a
 * path that cannot be opened; RGK_ERR_DEVICE: a short write.
 *
 * EXR.  d_count != NULL: accumulator mode, rgk_output_normalize followed by rgk_output_write_exr -- output_scale <= 0 is "auto",
 * and *scale_used (may be NULL) receives the scale applied.  d_count == NULL: image mode, d_rgb is a mean already and every value is
 * multiplied by output_scale, which must be finite and > 0 (RGK_ERR_INVALID otherwise) and is applied also when it is 1. */
int rgk_output_write_exr_device(rgk_scene *scene, const char *path, uint32_t xres, uint32_t yres,
                                const float *d_rgb /*3P*/, const uint32_t *d_count /*P, or NULL*/,
                                float output_scale, float *scale_used /*may be NULL*/);
/* PNG.  d_rgba: the words rgk_display_encode_device writes.  RGK_ERR_INVALID also for an image beyond one IDAT chunk, as the host
 * writer. */
int rgk_output_write_png_device(rgk_scene *scene, const char *path, uint32_t xres, uint32_t yres,
                                const uint32_t *d_rgba /*P*/);

#ifdef __cplusplus
}
#endif
#endif /* RGK_H */
