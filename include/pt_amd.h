/* pt_amd.h — C ABI of the MI355X path tracer (libpt_amd.so).
 *
 * Replaces the reference's render boundary path_tracer/src/pathtrace.h:6-9
 *     void InitDataContainer(GuiDataContainer*);   -> pt_set_flags
 *     void pathtraceInit(Scene*);                  -> pt_create
 *     void pathtraceFree();                        -> pt_destroy
 *     void pathtrace(uchar4* pbo, int frame, int iteration);
 *                                                  -> pt_render_pass (+ pt_preview_rgba for the PBO)
 * the scene loader path_tracer/src/scene.h:17-35 / scene.cpp:16-219 (Scene::Scene, loadFromJSON)
 *                                                  -> pt_scene_load_json / pt_scene_* builders
 * the first-frame camera recompute of main.cpp:59-73,117-136           -> pt_scene_finalize
 * and the image output main.cpp:88-112 + image.cpp:22-42 (saveImage, Image::savePNG)
 *                                                  -> pt_save_png / pt_tonemap
 *
 * Differences from the reference, by design:
 *   - no file-static globals: every render owns a pt_ctx; any number can coexist;
 *   - status codes (PT_OK / PT_ERR_*) instead of exit(); pt_last_error() gives the message;
 *   - explicit stream (hipStream_t passed as void*; NULL = the legacy default stream);
 *   - no per-iteration device->host copy of the image: pt_get_image / pt_copy_image on demand;
 *   - the context renders a pixel TILE (rows y with y % world == rank) and may trace `spp`
 *     consecutive iterations per pass; world == 1, spp == 1 is exactly the reference's
 *     pathtrace() (same RNG keys, same stable compaction order, same accumulation).
 * All structs are plain C with the reference's field order (sceneStructs.h).
 */
#ifndef PT_AMD_H
#define PT_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_OK 0
#define PT_ERR_ARG 1
#define PT_ERR_HIP 2
#define PT_ERR_NOMEM 3
#define PT_ERR_IO 4
#define PT_ERR_PARSE 5
#define PT_ERR_DEVICE 6   /* a device-side check failed (e.g. look-back spin bound hit) */

#define PT_GEOM_SPHERE 0  /* sceneStructs.h:12-17 */
#define PT_GEOM_CUBE 1
#define PT_GEOM_MESH 2

/* Runtime flags: GuiDataContainer (utilities.h:17-34), mirrored into Settings (pathtrace.cu:31-55). */
typedef struct pt_flags {
    int32_t russian_roulette;     /* default 1 */
    int32_t use_bvh;              /* default 1 */
    int32_t use_bbox;             /* default 1 (linear mesh path only) */
    int32_t sort_by_material;     /* default 0: stable material sort before shading */
    int32_t use_thrust_partition; /* default 0: same stable partition either way */
    int32_t ssaa;                 /* default 1 */
    int32_t dof;                  /* default 1 */
    float aperture;               /* default 0.1 */
    float focal_dist;             /* default 10 */
    /* Extension (default 0 = the reference): apply the surface albedo once.  The reference
     * multiplies the path colour by the albedo at interactions.cu:60 AND :83; its own course
     * image (img/REFERENCE_cornell.5000samp.png) matches the single-albedo model. */
    int32_t single_albedo;
    /* Extension (default 0 = the reference): skip BVH nodes whose entry distance exceeds the
     * closest triangle found so far by a 1e-3 relative margin.  BVHIntersectionTest
     * (intersections.cu:170-224) visits every node the ray line crosses.  The closest hit is
     * unchanged unless rounding moves a triangle's computed t by more than the margin
     * (DESIGN.md §4). */
    int32_t bvh_cull;
    /* Another context, stream or process shares the GPU (0 = no).  1 makes every inter-workgroup
     * wait of a render pass safe without co-residency: the split pipeline's look-back compaction
     * claims tiles in order from a ticket (lookback.h), and the material-sorted pipeline scans its
     * histogram with the three-kernel reduce/scan/apply path instead of the single-pass library
     * scan.  With 0, a static-schedule wait that cannot get the whole GPU hits its spin bound and
     * pt_stats reports PT_ERR_DEVICE.  pt_flags_default: 1 if PT_AMD_SCHEDULE=claim, else 0. */
    int32_t shared_gpu;
    /* Extension (default 0 = the reference): key the shading RNG by the path's global pixel index
     * instead of its position in the compacted path array (pathtrace.cu:315).  The image then
     * no longer depends on how pixels are sharded across GPUs or sorted by material: N-GPU output
     * is bitwise equal to 1-GPU output (SURVEY.md §8e's rng_key=pixel mode). */
    int32_t rng_key_pixel;
} pt_flags;

/* Material (sceneStructs.h:43-57), 48 bytes. */
typedef struct pt_material {
    float color[3];
    float spec_exponent;
    float spec_color[3];
    float has_reflective;
    float has_refractive;
    float ior;
    float emittance;
    int32_t texture_id;           /* -1: none */
} pt_material;

/* Geom (sceneStructs.h:25-41), 272 bytes.  Matrices are glm column-major: m[c][r] = a[4c+r]. */
typedef struct pt_geom {
    int32_t type;
    int32_t material_id;
    float translation[3];
    float rotation[3];            /* degrees */
    float scale[3];
    float transform[16];
    float inverse_transform[16];
    float inv_transpose[16];
    int32_t tri_start, tri_end, bbox_idx;
    float min_bound[3], max_bound[3];
} pt_geom;

/* Camera (sceneStructs.h:59-69). */
typedef struct pt_camera {
    int32_t res[2];
    float position[3], look_at[3], view[3], up[3], right[3];
    float fov[2];
    float pixel_length[2];
} pt_camera;

/* Triangle (sceneStructs.h:103-161), 124 bytes, world space. */
typedef struct pt_triangle {
    int32_t id;                   /* original (load-order) index */
    float v[3][3];
    float uv[3][2];
    float n[3][3];
    float bmin[3], bmax[3];
} pt_triangle;

/* Flattened BVH node (BVH_tree.h:54-61), 40 bytes. */
typedef struct pt_bvh_node {
    float bmin[3], bmax[3];
    int32_t sub_areas, axis, first_area_idx, rchild_idx;
} pt_bvh_node;

typedef struct pt_scene pt_scene;
typedef struct pt_ctx pt_ctx;

/* Tile / batching of one context.  rank/world: this context owns image rows y % world == rank.
 * spp: iterations traced together per pass (1 = the reference). */
typedef struct pt_shard {
    int32_t rank, world, spp, reserved;
} pt_shard;

/* Per-context counters (device-side, read back by pt_stats). */
typedef struct pt_stats_t {
    uint64_t segments;            /* sum over bounces of live paths entering intersection */
    uint64_t passes;
    uint64_t bounce_live[64];     /* live paths entering bounce k (k < depth) */
    uint64_t emissive_hits;       /* paths that terminated with non-zero radiance (framebuffer adds) */
    uint64_t bounce_emit[64];     /* of those, per bounce */
    uint32_t device_error;        /* nonzero: a device-side bound was hit */
    uint32_t bound_mismatch;      /* PT_AMD_VERIFY_BOUNDS=1 only: closest hits where the bounded
                                     pass differed from the plain per-geom loop (must stay 0) */
} pt_stats_t;

const char* pt_last_error(void);
void pt_flags_default(pt_flags* f);

/* ---- scene ---------------------------------------------------------------------------- */
int pt_scene_load_json(const char* path, pt_scene** out);   /* Scene::Scene(filename) incl. pt_scene_finalize */
/* Loader extensions, all off by default (pt_scene_load_json == options 0 == the reference's loader).
 * PT_LOAD_REFRACTION: read the material keys REFRACTIVE and IOR, which the reference's
 * Scene::loadFromJSON never reads (scene.cpp:46-56; refraction is unreachable from its files).  A
 * file can also opt in itself with the top-level key "Extensions": {"REFRACTION": true}, which the
 * reference ignores; a reference scene file therefore loads exactly as the reference loads it. */
#define PT_LOAD_REFRACTION 1u
/* PT_LOAD_DEVICE_BVH: build the scene's BVH on the current HIP device (pt_scene_set_bvh_builder). */
#define PT_LOAD_DEVICE_BVH 2u
int pt_scene_load_json_ex(const char* path, uint32_t options, pt_scene** out);
int pt_scene_create(pt_scene** out);
void pt_scene_free(pt_scene* s);
int pt_scene_add_material(pt_scene* s, const pt_material* m, int32_t* id_out);
/* Texture pixels (row-major, `components` bytes per texel; only 3 is shaded, like the reference). */
int pt_scene_add_texture(pt_scene* s, int32_t width, int32_t height, int32_t components,
                         const uint8_t* pixels, int32_t* id_out);
/* JSON scenes reference textures by file (scene.cpp:61-71).  pt_scene_load_json decodes JPEG files
 * with pt_decode_jpeg (below) and fails with PT_ERR_IO where the reference prints "Texture load
 * error!" and exits (missing file, corrupt JPEG).  Files that are not JPEG (no SOI marker: PNG, BMP,
 * TGA, ... which the reference's stbi_load also reads) are NOT decoded here: the texture keeps its
 * path and no pixels, the host fills it with pt_scene_set_texture_pixels (the Python Scene does so
 * for lossless formats, whose texels any decoder reproduces), and pt_create refuses a scene with a
 * texture left unfilled.  pt_scene_set_texture_pixels also replaces a decoded texture's pixels. */
int pt_scene_texture_path(const pt_scene* s, int32_t id, char* buf, int32_t cap);
int pt_scene_set_texture_pixels(pt_scene* s, int32_t id, int32_t width, int32_t height,
                                int32_t components, const uint8_t* pixels);
/* Cube / sphere: builds transform, inverse, inverse-transpose like scene.cpp:80-91. */
int pt_scene_add_geom(pt_scene* s, int32_t type, int32_t material_id, const float t[3],
                      const float r[3], const float sc[3], int32_t* id_out);
/* Mesh: object-space polygon soup, fan-triangulated (tinyobj triangulate=true), pre-transformed
 * to world space (scene.cpp:94-173).  face_sizes[f] vertices per face; idx_* per face-vertex
 * (-1 = absent), positions/normals (xyz), uvs (uv).  PT_ERR_ARG for a world vertex that is not
 * finite or beyond 2^126 in magnitude (the SAH build would recurse without end on it). */
int pt_scene_add_mesh(pt_scene* s, int32_t material_id, const float t[3], const float r[3],
                      const float sc[3], const float* positions, int32_t npos,
                      const float* normals, int32_t nnorm, const float* uvs, int32_t nuv,
                      const int32_t* face_sizes, int32_t nfaces, const int32_t* idx_pos,
                      const int32_t* idx_norm, const int32_t* idx_uv, int32_t* id_out);
int pt_scene_set_camera(pt_scene* s, int32_t res_x, int32_t res_y, float fovy, const float eye[3],
                        const float look_at[3], const float up[3]);
int pt_scene_set_render(pt_scene* s, int32_t iterations, int32_t depth, const char* file);
/* Camera orbit recompute of the first frame (main.cpp:59-73,117-136) + BVH build (scene.cpp:218). */
int pt_scene_finalize(pt_scene* s);
/* Where pt_scene_finalize builds the BVH (BVH_tree.cpp:27-181's SAH tree): 0 (default) on the host,
 * 1 on the current HIP device — the same nodes, byte for byte, and the same triangle order
 * (bvh_build.hip); a tree the device builder leaves to the host (NaN vertex coordinates) is built
 * there.  pt_scene_bvh_build_info: where the last build ran and its wall time in ms. */
int pt_scene_set_bvh_builder(pt_scene* s, int32_t device);
int pt_scene_bvh_build_info(const pt_scene* s, int32_t* on_device, double* ms);
int pt_scene_counts(const pt_scene* s, int32_t* ngeoms, int32_t* nmats, int32_t* ntris,
                    int32_t* nnodes, int32_t* ntex);
int pt_scene_get_camera(const pt_scene* s, pt_camera* out);
int pt_scene_get_render(const pt_scene* s, int32_t* iterations, int32_t* depth, char* file, int32_t cap);
/* The interactive camera of the preview (main.cpp).  pt_scene_get_orbit: the orbit of the loaded
 * camera, phi / theta / zoom as main.cpp:59-73 derives them (pt_scene_finalize computes them).
 * pt_scene_set_orbit: runCuda's camchanged recompute (main.cpp:117-136) for the orbit (phi, theta,
 * zoom) about look_at — position, view, right (= view x (0,1,0), unnormalised) and up; the scene stays
 * finalized, and contexts created after the call render the new camera (the reference re-runs
 * pathtraceInit at iteration 0).  Both need a finalized scene (PT_ERR_ARG otherwise). */
int pt_scene_get_orbit(const pt_scene* s, float* phi, float* theta, float* zoom);
int pt_scene_set_orbit(pt_scene* s, float phi, float theta, float zoom, const float look_at[3]);
/* ---- Environment lighting (extension) -------------------------------------------
 * Without an environment a ray that leaves the scene is worth 0, as in the reference.  With one, it ends
 * the path with throughput x L(direction): L is a bilinear lookup in an octahedral map (y up) of n x n
 * RGBA32F texels, rotated by rotate_deg (Rx Ry Rz, degrees, world to map) and multiplied by scale.  No
 * light sampling: the estimator stays the reference's.  Contexts created AFTER the call render it (fused
 * pipeline only: pt_create / pt_set_flags refuse material-sorted shading and PT_PIPELINE=split, and
 * pt_adaptive_enable refuses the context, each with PT_ERR_ARG); such a context builds no camera masks.
 *   size: the map's n, 1..4096, or 0 for the default (source height / 2, at least 1, at most 2048).
 * pt_scene_set_environment resamples a lat-long image (row 0 = +y, column centre u = 0.5 = -z, u grows
 * towards +x; rgb = width * height * 3 floats) onto the map; a source denser than the map is box-filtered
 * first.  pt_scene_set_environment_octa takes the n x n x 3 texels themselves (row j along z, column i
 * along x, no gutter; params->size is ignored).  pt_scene_load_environment reads a Radiance .hdr file.
 * pt_scene_get_environment: *n (0: none), the parameters, and the padded map, (n + 2)^2 * 4 floats, when
 * rgba_padded is not NULL (cap floats available; PT_ERR_ARG if too few).
 * JSON scenes: "Extensions": {"ENVIRONMENT": {"FILE": name, "SCALE": x, "ROTATE": [x, y, z], "SIZE": n}},
 * FILE relative to <scene dir>/Textures/. */
typedef struct pt_env_params {
    float scale;           /* default 1 */
    float rotate_deg[3];   /* default 0, 0, 0 */
    int32_t size;          /* default 0: derived from the source */
} pt_env_params;
void pt_env_params_default(pt_env_params* p);
int pt_scene_set_environment(pt_scene* s, int32_t width, int32_t height, const float* rgb_latlong,
                             const pt_env_params* params);
int pt_scene_set_environment_octa(pt_scene* s, int32_t n, const float* rgb, const pt_env_params* params);
int pt_scene_load_environment(pt_scene* s, const char* path, const pt_env_params* params);
int pt_scene_clear_environment(pt_scene* s);
int pt_scene_get_environment(const pt_scene* s, int32_t* n, pt_env_params* out, float* rgba_padded, int64_t cap);
/* Radiance HDR reader: "-Y H +X W" files of FORMAT=32-bit_rle_rgbe, new-style run-length coded or flat
 * scanlines.  out = NULL: the size only; else height * width * 3 floats in file order (cap floats
 * available), each mantissa byte m with exponent byte e standing for m * 2^(e - 136), 0 when e = 0.
 * Truncated or malformed input is PT_ERR_PARSE; nothing is read beyond data[size). */
int pt_decode_hdr(const uint8_t* data, int64_t size, int32_t* width, int32_t* height, float* out, int64_t cap);
/* L(d) of the scene's environment for n directions (3 floats each, any length), by the lookup the bounce
 * kernels call: d_dirs / d_rgb are device pointers (n * 3 floats); the map is uploaded for the call, the
 * kernel runs on `stream`, and the call returns when it has completed.  pt_env_eval_host takes host
 * pointers.  PT_ERR_ARG for a scene without an environment. */
int pt_env_eval(const pt_scene* s, int64_t n, const float* d_dirs, float* d_rgb, void* stream);
int pt_env_eval_host(const pt_scene* s, int64_t n, const float* dirs, float* rgb);

/* Getters copy min(count, cap) records and return that number (>= 0), or -PT_ERR_ARG. */
int pt_scene_get_geoms(const pt_scene* s, pt_geom* out, int32_t cap);
int pt_scene_get_materials(const pt_scene* s, pt_material* out, int32_t cap);
int pt_scene_get_triangles(const pt_scene* s, pt_triangle* out, int32_t cap);
int pt_scene_get_bvh(const pt_scene* s, pt_bvh_node* out, int32_t cap);
/* Inspection (host only, used by the tests): the 4-wide layout the BVH walk of mesh scenes runs on
 * (128-byte entries: lo.x, hi.x, lo.y, hi.y, lo.z, hi.z, codes, meta — each 4 slots; layout and
 * codes in pt_layout.h DQuad).  Returns the entry count (0: no 4-wide layout for this tree; the
 * pair walk runs) and copies min(count, cap) entries; *root_code / *stack_bound as pt_create uses. */
int pt_scene_bvh_quads(const pt_scene* s, void* out, int32_t cap, int32_t* root_code, int32_t* stack_bound);
/* Inspection (host only): the 4-wide walk's exact t-cull words, 4 per quad in pt_scene_bvh_quads's
 * order (slot k: binary16 A in bits 0-15, binary16 B in bits 16-31; a slot's children are not entered
 * when A * tau_lo > B + best), and the share of slots with A >= 1/2.  Returns the word
 * count (0: no 4-wide layout) and copies min(count, cap) words. */
int pt_scene_bvh_tcull(const pt_scene* s, uint32_t* words, int32_t cap, double* cullable_frac);
/* Inspection (host only): the room a context created from this scene with these flags (NULL: the
 * defaults) would bound as one group, derived without a device; outputs as pt_ctx_room_info's. */
int pt_scene_room_info(const pt_scene* s, const pt_flags* flags, int32_t* walls, int32_t* faces, float* lo,
                       float* hi);
/* Inspection (host only): the widened bounds of the bounded closest hit that a context
 * created from this scene with these flags (NULL: the defaults) would use, derived without a device.
 * Per geom, min(geom count, cap) rows: the bound kind (0 none, 1 oriented cube, 2 sphere, 3 world-box
 * cube, 4 uniformly scaled sphere), the widened object-space slabs, the widened world box and the tight
 * planes of a world-box cube ((lo, hi) of axis a at tight[2a]; zeros for other kinds; a uniformly
 * scaled sphere keeps its centre in wlo and its squared inverse scale and that value's reciprocal in
 * whi[0], whi[1]), the relative slack and the pull-back constants.  *R: the largest |coordinate| of a ray origin the bounds are sized
 * for; *r_limit: the largest R for which this scene's bound forms cannot overflow; *bounded: 1 when the
 * context runs the bounds pass, 0 when R exceeds r_limit and every geom is exact-tested for every ray
 * (the rows then hold bounds that claim nothing); *abs_slack, *wb_tslack as the kernels read them.  Any
 * pointer may be null. */
typedef struct pt_bound_info {
    int32_t bkind;
    float slo[3], shi[3], wlo[3], whi[3];
    float tight[6];
    float tslack, back, wback;
} pt_bound_info;   /* 88 bytes */
int pt_scene_bound_info(const pt_scene* s, const pt_flags* flags, pt_bound_info* rows, int32_t cap, double* R,
                        double* r_limit, int32_t* bounded, float* abs_slack, float* wb_tslack);

/* ---- render context -------------------------------------------------------------------- */
/* pathtraceInit: uploads the scene to the current HIP device, allocates SoA path buffers for
 * rows_in_tile * width * spp paths.  shard may be NULL (= {0, 1, 1}). */
int pt_create(const pt_scene* s, const pt_flags* flags, const pt_shard* shard, pt_ctx** out);
int pt_destroy(pt_ctx* c);                                  /* pathtraceFree */
/* InitDataContainer / Settings.  Cheap when called every iteration with unchanged camera-ray flags:
 * only a change of ssaa, dof, aperture or focal_dist synchronises the device and rebuilds the
 * first-bounce camera masks (and, for the aperture, the widened geom bounds). */
int pt_set_flags(pt_ctx* c, const pt_flags* flags);
/* Host-side counters of a context: first-bounce camera-mask builds (pt_create builds one) and the
 * pt_set_flags calls that synchronised the device. */
int pt_ctx_counters(const pt_ctx* c, uint64_t* mask_builds, uint64_t* flag_syncs);
/* Inspection: the first-bounce camera masks of a context — built (on), the share of 64-pixel blocks
 * whose mask is empty (no geom reachable: those waves skip raygen and the closest hit), and whether
 * the fused first bounce runs its empty-wave instantiation (chosen when that share is >= 0.2;
 * PT_AMD_SKIP_EMPTY=0/1 forces it).  Results are the same bits either way. */
int pt_ctx_cmask_info(const pt_ctx* c, int32_t* on, double* empty_frac, int32_t* skip_fused);
/* Inspection: the room whose walls the later bounces bound as one group — the number
 * of walls (0: no room), the geom index of the wall of each face -x, +x, -y, +y, -z, +z (faces[6], -1
 * without one) and the box between the walls' facing planes (lo[3], hi[3]; -inf / +inf on a face
 * without a wall).  Results are the same bits with or without a room (PT_AMD_ROOM=0: never one). */
int pt_ctx_room_info(const pt_ctx* c, int32_t* walls, int32_t* faces, float* lo, float* hi);
/* Inspection, PT_AMD_VERIFY_BOUNDS=1 only (zeros otherwise; counted by the verifying kernels of the split
 * and the sorted pipeline since the context's last reset): room — later-bounce rays for which a room
 * wall's tight plane alone called the wall they left a miss (the departure claim, DESIGN.md §4.1;
 * PT_AMD_ROOM_DEPART=0: none); loop_zero — (ray, cube) pairs of the per-cube world-box loop left as
 * candidates with bound 0; loop_depart — those of them whose origin lies beyond the cube's own widened
 * slab with the ray not coming back (what the same claim could remove there).  Waits for the context's
 * queued work.  Any pointer may be null. */
int pt_ctx_depart_counts(pt_ctx* c, uint64_t* room, uint64_t* loop_zero, uint64_t* loop_depart);
/* Inspection, PT_AMD_VERIFY_BOUNDS=1 only (zeros otherwise; counted like pt_ctx_depart_counts): tests —
 * exact tests the bounded closest hit ran (one per ray and candidate geom); tripped — those of them
 * whose range gate tripped, so the whole test ran again through the literal, per-operation-gated path
 * (DESIGN.md §3): an operand of a sqrt, division or normalize that is zero, denormal, infinite, NaN or
 * outside the core's range.  Waits for the context's queued work.  Either pointer may be null. */
int pt_ctx_exact_counts(pt_ctx* c, uint64_t* tests, uint64_t* tripped);
/* Mesh scenes: whether the BVH walk runs on the 4-wide layout, whether its exact t-cull is on, and
 * the share of the layout's slots whose cull margin can pay.  The cull is on when
 * that share is >= 1/4 (PT_AMD_TCULL=0/1 forces it); it never changes a result. */
int pt_ctx_walk_info(const pt_ctx* c, int32_t* quad_walk, int32_t* tcull_on, double* tcull_frac);
/* Mesh scenes, read-only: which BVH walk the context runs under its current flags, as the kernels
 * themselves decide it (the same predicates).  walk — the walk launched ahead of the bounce kernel:
 * PT_WALK_QUADS (k_traverse4), PT_WALK_PAIRS or PT_WALK_NODES (k_traverse's two forms), PT_WALK_NONE
 * when the walk runs inside the bounce kernel (PT_AMD_MESH_INLINE=1, the material-sorted and the split
 * pipeline, more geoms than the LDS table holds).  inline_walk — the walk of that inline form, of the
 * G-buffer and of the rays the 4-wide walk leaves to the bounce kernel: PT_WALK_PAIRS, PT_WALK_NODES
 * (both with the stack in LDS), PT_WALK_NODES_PRIVATE (a tree of depth >= 32: the reference's 64
 * private entries), PT_WALK_NONE without a tree or with the BVH flag off.  bvh_depth — the depth of
 * the deepest interior node; stack_bound — the 4-wide layout's bound on its stack (0 without one).
 * Any pointer may be null. */
enum { PT_WALK_NONE = 0, PT_WALK_QUADS = 1, PT_WALK_PAIRS = 2, PT_WALK_NODES = 3, PT_WALK_NODES_PRIVATE = 4 };
int pt_ctx_walk_kind(const pt_ctx* c, int32_t* walk, int32_t* inline_walk, int32_t* bvh_depth, int32_t* stack_bound);
/* Stream budget.  HIP maps a process's streams of one priority onto GPU_MAX_HW_QUEUES (default 4)
 * hardware queues; streams beyond that share queues and their work runs in submission order.  A
 * context keeps busy: the caller's stream, one stream per extra lane of a batched pass, and the
 * finalize stream of a batched pass.  pt_create caps the lanes it picks by itself so that the busy
 * streams of all live contexts stay within GPU_MAX_HW_QUEUES (PT_AMD_LANES overrides the choice and
 * the cap).  The synchronous entry points copy on a high-priority stream of the context's own, a
 * pool of queues apart from the compute streams.  So one context's passes never wait for another's,
 * and its synchronous reads never queue behind another's passes, while the process's busy
 * normal-priority streams — the library's and the caller's own (torch's stream pool, say) — are at
 * most GPU_MAX_HW_QUEUES; past that, contexts share queues and may serialise (still correct).
 * pt_ctx_stream_info: the context's lanes, its busy streams, the sum over the live contexts, the
 * budget, and whether its lanes were capped. */
int pt_ctx_stream_info(const pt_ctx* c, int32_t* lanes, int32_t* busy_streams, int32_t* process_busy,
                       int32_t* hw_queues, int32_t* lanes_capped);
/* One pass: iterations [iter_first, iter_first + spp) for this tile, accumulated into the tile
 * image.  Asynchronous on `stream`; no host synchronisation inside.  A batched pass (spp > 1)
 * runs its iterations in lanes on internal streams and adds their colours into the image on a
 * finalize stream; `stream` itself is not made to wait for every lane (the next pass starts during
 * this one's tail).  Read the image through pt_copy_image / pt_preview_rgba / pt_reset_image (they
 * wait for the last finalize on their stream) or the synchronising calls.  Passes of one context
 * may go to different streams: a pass on another stream than the previous pass first waits (on the
 * device) for all of the context's queued work; passes on one stream keep their overlap. */
int pt_render_pass(pt_ctx* c, int32_t iter_first, void* stream);
/* Render-ahead for a one-iteration context (spp 1; the drop-in pathtrace() loop): queues the bounces
 * of iteration `iter` on `stream` now, without touching the image, so they run while the caller
 * copies the previous image to the host (pathtrace.cu:524's copy).  A later pt_render_pass(c, iter)
 * with the same flags claims them and only adds their colours into the image (the same bits as
 * rendering then); any other pass — another iteration, changed flags — drops them first.  Counts
 * (pt_stats) include an iteration once it is claimed.  Not synchronising; pt_get_image and the
 * other synchronising calls do not wait for unclaimed ahead work.  Ordering on any streams: the
 * ahead work waits (on the device) for the context's last pass, claim or image call when that went
 * to another stream, and every later pass or ahead waits for the ahead work.  On failure nothing is
 * left to claim and the HIP last-error is cleared (the caller may go on without the overlap). */
int pt_render_ahead(pt_ctx* c, int32_t iter, void* stream);
/* sendImageToPBO (pathtrace.cu:64-86) for the tile: d_rgba = npix * 4 bytes on the device. */
int pt_preview_rgba(pt_ctx* c, int32_t iter, uint8_t* d_rgba, void* stream);
/* pathtrace(pbo, frame, iteration) (pathtrace.h:9, pathtrace.cu:437-525) as one call, under the
 * name SURVEY.md §8b gives it: pt_render_pass for iterations [iter, iter + spp), then, when d_rgba
 * is non-NULL, pt_preview_rgba of the accumulated iter + spp - 1 samples (iterations counted from 1). */
int pt_render_iteration(pt_ctx* c, int32_t iter, uint8_t* d_rgba, void* stream);
int pt_tile_info(const pt_ctx* c, int32_t* width, int32_t* rows, int32_t* npix, int32_t* npaths);
int pt_get_image(pt_ctx* c, float* host_rgb);               /* tile accumulator, npix*3 floats (sync) */
int pt_get_accum(pt_ctx* c, float* host_rgb);               /* §8b name of pt_get_image (pathtrace.cu:524) */
int pt_copy_image(pt_ctx* c, float* d_rgb, void* stream);   /* device-to-device copy */
int pt_reset_image(pt_ctx* c, void* stream);
/* Resume (extension; the reference has none): load a previously saved float accumulator of this
 * context's tile (npix x float3, as pt_get_accum returns it).  Continuing with the next iteration
 * indices reproduces an uninterrupted render bit for bit.  Any -0 is loaded as +0 (the reference's
 * image holds no -0 after a pass: every iteration adds a colour, zero or not, into every pixel). */
int pt_set_accum(pt_ctx* c, const float* host_rgb);
int pt_stats(pt_ctx* c, pt_stats_t* out);                   /* synchronises the context stream */
/* The synchronous calls above (pt_get_image, pt_get_accum, pt_set_accum, pt_stats, and pt_set_flags
 * when it rebuilds device data) and pt_destroy wait for THIS context's enqueued work only — an event
 * recorded after its last pass or image call — and move data on a non-blocking stream of the
 * context's own: another context's passes, or other work on the GPU, are not waited for.
 *
 * Drop-in helpers (host/pathtrace.cpp, the pathtrace.h mirror): page-lock a host buffer that
 * pt_get_image copies into every iteration (the reference's Scene::state.image, pathtrace.cu:524),
 * so the copy runs at the link's DMA rate; and a non-blocking stream for a context's passes, so they
 * neither wait for nor hold up the legacy default stream. */
int pt_host_register(void* host, uint64_t bytes);
int pt_host_unregister(void* host);
int pt_stream_create(void** stream);
int pt_stream_destroy(void* stream);
/* Per-kernel device timing with hipEvents recorded on the launch stream (for the roofline).  When
 * enabled, pt_render_pass brackets every launch with pooled events; pt_profile_read synchronises
 * and returns, per kernel kind, the summed milliseconds and launch counts since the last read. */
#define PT_KIND_FIRST_BOUNCE 0   /* bounce 0: k_bounce<FIRST> (fused), k_trace<FIRST> (split), or the
                                    first k_sort_produce (sorted: raygen + intersection)           */
#define PT_KIND_BOUNCE 1         /* bounces >= 1: k_bounce (fused) or k_trace (split)          */
#define PT_KIND_COMPACT 2        /* split pipeline only: k_compact_paths                        */
#define PT_KIND_SORT 3           /* material-sorted mode, per bounce: histogram scan + producer
                                    (shade bounce b, compact, intersect bounce b + 1)              */
#define PT_KIND_TRAVERSE 4       /* mesh scenes, bounces >= 1: the BVH walk k_traverse[4]       */
#define PT_KIND_FIRST_TRAVERSE 5 /* mesh scenes, bounce 0: the BVH walk of the camera rays       */
#define PT_KIND_COUNT 6
int pt_profile_enable(pt_ctx* c, int32_t on);
/* The first four kinds (pt_profile_read_kinds returns all of them).  These two calls count the BVH
 * walk (kinds 4 and 5) in BOUNCE and FIRST_BOUNCE, as before the walk had kinds of its own.  In the
 * material-sorted pipeline the camera-ray producer counts as FIRST_BOUNCE, not SORT (since round 3). */
int pt_profile_read(pt_ctx* c, double ms[4], uint64_t launches[4]);
/* Same, plus busy_ms[kind]: the length of the union of that kind's launch intervals.  Batched
 * passes of the fused pipeline run two lanes of iterations concurrently (pt_render_pass), so
 * launches of one kind overlap and busy_ms < ms. */
int pt_profile_read_busy(pt_ctx* c, double ms[4], double busy_ms[4], uint64_t launches[4]);
/* Every kind: arrays of nkinds entries (kinds >= PT_KIND_COUNT read 0).  busy_ms may be NULL. */
int pt_profile_read_kinds(pt_ctx* c, int32_t nkinds, double* ms, double* busy_ms, uint64_t* launches);

/* Device self-check of the range-gated correctly rounded sqrt / division cores the kernels use
 * (pt_device.h) against hipcc's library sqrtf and '/': n operand sets from `seed` (random bit
 * patterns over every exponent, a quarter near 1, plus zeros, denormals, infinities and NaNs).
 * *mismatches = operations whose bits differ (NaN == NaN).  Synchronous. */
int pt_selftest_math(uint64_t n, uint32_t seed, uint64_t* mismatches);
/* Device self-check of the exact test's fast path (one range gate) against its literal
 * path: n (ray, geom) pairs from `seed` — cubes and spheres under random affine maps, half of the pairs
 * with ordinary operands and half with pt_selftest_math's operands (every exponent, zeros, denormals,
 * infinities, NaNs) in the ray and the maps.  *mismatches = pairs whose distance bits differ (NaN ==
 * NaN) or, for a hit, whose slab code, object-space point or side differ; *tripped = pairs whose gate
 * tripped; *fast = pairs the fast path answered.  Synchronous. */
int pt_selftest_exact(uint64_t n, uint32_t seed, uint64_t* mismatches, uint64_t* tripped, uint64_t* fast);
/* Device self-check of the renormalisation of unit vectors (pt_device.h renorm_unit_core, the closed form
 * of 1 / sqrt(x) on [1 - 2^-12, 1 + 2^-12]) against the general normalize core, in one launch: every one
 * of the 6,145 floats of that range, the first float outside on each side, zero, denormal, huge, infinite,
 * negative and NaN x, and nvec vectors from `seed` (three of four of unit length), for which the two forms
 * of getPointOnRay are compared as well.  *mismatches = items whose bits differ (NaN == NaN); *in_range =
 * items that took the closed form; *misranged = items whose range test differs from the stated range.
 * Synchronous. */
int pt_selftest_renorm(uint32_t nvec, uint32_t seed, uint64_t* mismatches, uint64_t* in_range, uint64_t* misranged);
/* The closed form itself on the host (no device): out[i] = the bits of 1 / sqrt(x) for the float x with
 * bits[i] and in_range[i] = 1 where x lies in [1 - 2^-12, 1 + 2^-12]; elsewhere in_range[i] = 0 and
 * out[i] = 0 (the kernels run the general normalize there). */
int pt_unit_rnorm_host(const uint32_t* bits, int64_t n, uint32_t* out, uint8_t* in_range);
/* Device self-check of the bounded closest hit's lower bounds, per (ray, geom) pair.
 * The scene is prepared as pt_create prepares it (geom table, widened bounds with the flags' aperture,
 * room, bound order) and uploaded; n rays are generated on the device from `seed`, and every ray is
 * checked against every bounded geom with the functions the render kernels call: where the literal
 * exact test returns t > 0, every bound form the kernels can apply to that geom must be a candidate
 * (tag below +inf's bits) whose bound, less the scene's absolute slack, does not exceed t.  Forms: 0 the
 * tagged form of the geom's kind (world-box cube, oriented cube, uniform sphere), 1 and 2 the float form
 * with early returns and with selects (tagged as the pass tags it), 3 a room wall's slot in the grouped
 * room bound.  Rays take their class from their index (i mod 6) and stay inside the bounds' precondition
 * (every origin coordinate within R, direction length in (0.5, 2), no NaN; others are counted in
 * `skipped`, by class): 0 origin uniform in the scene's box, uniform direction; 1 rays departing from the exact hit
 * of such a ray on a geom, pulled back and lifted as the shader does, half cosine-distributed about the
 * normal and half grazing (|cos| < 1e-3); 2 directions with one or two components exactly +-0 or with a
 * denormal component; 3 rays aimed at a cube's corner or edge or at a sphere's silhouette point, the
 * world-space target moved by 0, +-1 or +-4 ulp per coordinate; 4 origins inside a geom; 5 rays of the
 * scene's camera (lens samples when the flags' DoF is on).  A class-1 ray whose base ray hits nothing
 * counts in class 0.  Scenes the context does not bound (more than 32 geoms, meshes, or beyond the
 * bounds' range: pt_scene_bound_info) are an argument error.  Synchronous. */
typedef struct pt_bounds_report {
    uint64_t pairs[5];        /* pairs with t > 0 per kind: bkind 1, 2, 3, 4, walls of the room */
    uint64_t bad_tagged[5];   /* violations of the tagged form (the room: of the wall's slot) */
    uint64_t bad_float[5];    /* violations of the float forms */
    uint64_t rays[6];         /* rays checked per class */
    uint64_t skipped[6];      /* rays per class that left the precondition, not checked */
    uint32_t has_first;       /* a violation was recorded below (any one of them) */
    uint32_t first_geom, first_form;
    uint32_t first_origin[3], first_dir[3];   /* float bits */
    uint32_t first_bound, first_t;            /* the tag, and t's bits */
    uint32_t pad_;
} pt_bounds_report;   /* 264 bytes */
int pt_selftest_bounds(const pt_scene* s, const pt_flags* flags, uint64_t n, uint32_t seed, pt_bounds_report* report);

/* ---- texture input --------------------------------------------------------------------- */
/* Texture::load (sceneStructs.h:171-175) = stbi_load(file, &w, &h, &comp, 0) for JPEG data:
 * stb_image 2.06's JPEG decoder restated (baseline + progressive, its integer IDCT, triangle-filter
 * chroma upsampling and fixed-point YCbCr->RGB), so texels equal the reference's.  Writes width,
 * height, components (1 or 3); with out != NULL also the w*h*components interleaved bytes (top row
 * first; cap = size of out).  out == NULL: header only. */
int pt_decode_jpeg(const uint8_t* data, int64_t size, int32_t* width, int32_t* height, int32_t* components,
                   uint8_t* out, int64_t cap);

/* ---- image output ---------------------------------------------------------------------- */
/* saveImage + Image::savePNG pixel math: out[3*(y*W + (W-1-x)) + k] = uchar(clamp(rgb/spp,0,1)*255). */
int pt_tonemap(const float* rgb, int32_t width, int32_t height, float samples, uint8_t* out);
/* Writes `path` as an 8-bit RGB PNG of the tonemapped image. */
int pt_save_png(const char* path, const float* rgb, int32_t width, int32_t height, float samples);
/* Image::saveHDR (image.cpp:44-49) via stb_image_write's Radiance RGBE writer (vendored by the
 * reference: external/include/stb_image_write.h:246-387), pixels as saveImage (x-mirrored,
 * accumulated / samples).  pt_encode_hdr writes the file bytes to `out` (NULL: size only). */
int pt_save_hdr(const char* path, const float* rgb, int32_t width, int32_t height, float samples);
int pt_encode_hdr(const float* rgb, int32_t width, int32_t height, float samples, uint8_t* out, int64_t cap,
                  int64_t* size);

/* ---- first-hit G-buffer and denoiser ----------------------------------------------------- */
/* Feature planes of the first hit of the deterministic camera ray (ssaa and dof off, whatever the
 * context's flags), for this context's tile, in pt_get_image's pixel order (npix entries each):
 *   gA  float4: n.x, n.y, n.z, material id as int32 bits; a miss has n = 0 and id -1
 *   gB  float4: P.x, P.y, P.z, t; P = the point shading scatters from (getPointOnRay), t the hit
 *               distance; a miss has P = 0 and t = -1
 *   alb float4: r, g, b, 0: the factor a diffuse first bounce multiplies into the throughput
 *               (texture-or-colour times colour, or texture-or-colour alone with single_albedo);
 *               (1, 1, 1) for emissive materials and misses
 *   uv  float2: the hit's texture coordinates, 0 on a miss (may be NULL)
 * pt_gbuffer is asynchronous on `stream` (device pointers) and orders itself against the context's
 * other work like pt_copy_image; pt_get_gbuffer fills host arrays and synchronises.  Any rank /
 * world / spp. */
int pt_gbuffer(pt_ctx* c, float* d_gA, float* d_gB, float* d_alb, float* d_uv, void* stream);
int pt_get_gbuffer(pt_ctx* c, float* h_gA, float* h_gB, float* h_alb, float* h_uv);

/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) guided by gA / gB, on the colour
 * divided by alb (demodulate) — the exact fp32 definition is DESIGN.md §10.  `levels` in 0..8 (step
 * 2^i at level i; sigma_c halves per level), sigmas finite and > 0.  NaN inputs propagate. */
typedef struct pt_denoise_params {
    int32_t levels;               /* default 5 */
    float sigma_c, sigma_n, sigma_p; /* colour (per-sample, demodulated), normal, plane distance; defaults 1, 0.3, 0.2 */
    int32_t demodulate;           /* default 1 */
    int32_t reserved[3];
} pt_denoise_params;
void pt_denoise_params_default(pt_denoise_params* p);
typedef struct pt_denoiser pt_denoiser;
int pt_denoiser_create(int32_t width, int32_t height, pt_denoiser** out);   /* owns two float4 planes */
int pt_denoiser_destroy(pt_denoiser* d);
/* Asynchronous on `stream`, device pointers.  d_rgb: accumulated W*H float3 of `samples` samples;
 * d_out_rgb: per-sample W*H float3 (pt_tonemap(out, W, H, 1.0f, ...) writes it); must not alias d_rgb.
 * Argument errors (PT_ERR_ARG) are found before any device call. */
int pt_denoiser_run(pt_denoiser* d, const float* d_rgb, float samples, const float* d_gA, const float* d_gB,
                    const float* d_alb, const pt_denoise_params* p, float* d_out_rgb, void* stream);
/* The same on host arrays: allocates, copies, runs, copies back (synchronous). */
int pt_denoise_host(int32_t width, int32_t height, const float* rgb, float samples, const float* gA,
                    const float* gB, const float* alb, const pt_denoise_params* p, float* out_rgb);
/* G-buffer + accumulator of a world == 1 context -> denoised host image (W*H float3, per sample).
 * PT_ERR_ARG when world > 1.  The accumulator is not modified.  Synchronous. */
int pt_denoise_image(pt_ctx* c, float samples, const pt_denoise_params* p, float* host_out_rgb);

/* ---- per-pixel variance and the variance-guided filter -------------------- */
/* Luminance moments of batch means.  The object owns a copy of the accumulator as last seen (prev)
 * and the sums m1, m2 of lum(d) and lum(d)^2 over the updates, d = (rgb - prev) / batch_samples per
 * component (divided by alb where alb.k >= 2^-10 when d_alb is given: npix float4, as pt_gbuffer
 * writes it), lum(c) = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z.  Device pointers, asynchronous on
 * `stream` (the caller orders the calls of one object), no context needed.
 *   reset:    m1 = m2 = 0, batches = 0, prev = d_base_rgb (zeros when NULL)
 *   update:   one batch; batch_samples finite, > 0 and the same as the first update's since the last
 *             reset, else PT_ERR_ARG before any device call
 *   variance: d_var[npix] = max(0, m2/n - (m1/n)^2) * (n * batch_samples) / ((n - 1) * samples): the
 *             variance of the luminance of the per-sample mean of `samples` samples; needs n >= 2
 *             batches and samples > 0 (PT_ERR_ARG)
 *   get:      synchronous, host arrays (npix, npix, npix * 3), any may be NULL (for tests) */
typedef struct pt_moments pt_moments;
int pt_moments_create(int32_t width, int32_t height, pt_moments** out);
int pt_moments_destroy(pt_moments* m);
int pt_moments_reset(pt_moments* m, const float* d_base_rgb, void* stream);
int pt_moments_update(pt_moments* m, const float* d_rgb, float batch_samples, const float* d_alb, void* stream);
int pt_moments_info(const pt_moments* m, int32_t* batches, float* batch_samples);
int pt_moments_variance(pt_moments* m, float samples, float* d_var, void* stream);
int pt_moments_get(pt_moments* m, float* h_m1, float* h_m2, float* h_prev_rgb);

/* The a-trous filter of pt_denoiser_run with the colour term driven by a per-pixel variance of the
 * luminance (which it filters along with the colour) instead of a fixed sigma_c: the exact fp32
 * definition is DESIGN.md §11.  sigma_l scales the standard deviation and is the same at every level. */
typedef struct pt_denoise_var_params {
    int32_t levels;               /* default 5 */
    float sigma_l, sigma_n, sigma_p; /* luminance (in standard deviations), normal, plane distance; defaults 1, 0.3, 0.2 */
    int32_t demodulate;           /* default 1 */
    int32_t reserved[3];
} pt_denoise_var_params;
void pt_denoise_var_params_default(pt_denoise_var_params* p);
/* Like pt_denoiser_run.  d_var: W*H floats, the variance of lum(rgb / samples [/ alb]); d_out_var
 * (may be NULL): the filtered image's variance.  Outputs must not alias inputs. */
int pt_denoiser_run_var(pt_denoiser* d, const float* d_rgb, float samples, const float* d_var, const float* d_gA,
                        const float* d_gB, const float* d_alb, const pt_denoise_var_params* p, float* d_out_rgb,
                        float* d_out_var, void* stream);
int pt_denoise_var_host(int32_t width, int32_t height, const float* rgb, float samples, const float* var,
                        const float* gA, const float* gB, const float* alb, const pt_denoise_var_params* p,
                        float* out_rgb, float* out_var);
/* Variance tracking of a world == 1 context (PT_ERR_ARG otherwise): a pt_moments over its accumulator.
 * pt_track_variance(c, 1) starts from the accumulator as it stands (a no-op when already tracking);
 * (c, 0) frees everything.  pt_variance_update is called after a pass of batch_samples samples (the
 * context's spp); it orders itself like pt_copy_image and, with `demodulate`, divides the batch means
 * by the context's first-hit albedo (computed at the first update after tracking starts or the
 * accumulator is rebased).  pt_render_pass does nothing for tracking.  pt_reset_image and pt_set_accum
 * rebase a tracking context: sums and count to zero, prev = the new accumulator.
 * pt_get_variance: pt_moments_variance into a host array (npix floats; synchronous).
 * pt_denoise_image_var: like pt_denoise_image with the tracked variance (needs >= 2 batches). */
int pt_track_variance(pt_ctx* c, int32_t on);
int pt_variance_update(pt_ctx* c, float batch_samples, int32_t demodulate, void* stream);
int pt_variance_info(const pt_ctx* c, int32_t* on, int32_t* batches, float* batch_samples);
int pt_get_variance(pt_ctx* c, float samples, float* host_var);
int pt_denoise_image_var(pt_ctx* c, float samples, const pt_denoise_var_params* p, float* host_out_rgb);

/* ---- temporal reprojection: denoiser history across camera moves ---------- */
/* A history of a full image (width x height, world == 1 pixel order) that needs no context and outlives
 * any.  Per pixel: the per-sample mean colour (divided by alb where alb.k >= 2^-10 when demodulating)
 * with the history length h in samples, and weighted means of lum(c) and lum(c)^2 over the frames.  The
 * object also keeps the G-buffer, albedo and camera of the frame the history belongs to and the
 * accumulator as last seen.  The planes are allocated at the first frame: argument errors (PT_ERR_ARG)
 * are found before any device call.
 *   max_history  clamp of h in samples (0: unbounded; finite, >= 0, and at least one batch)
 *   min_ndot     a history tap is dropped when dot(N_p, N_q) < min_ndot (finite, in [-1, 1])
 *   plane_tol    ... or when |dot(N_p, P_q - P_p)| > plane_tol * t_p (finite, >= 0)
 *   demodulate   default 1
 *   min_frames   where h < min_frames * batch the resolved variance is spatial (0..2^20; default 4) */
typedef struct pt_temporal_params {
    float max_history;            /* default 32 (DESIGN.md §12's grid) */
    float min_ndot, plane_tol;    /* defaults 0.9, 0.02 */
    int32_t demodulate;
    int32_t min_frames;
    int32_t reserved[3];
} pt_temporal_params;
void pt_temporal_params_default(pt_temporal_params* p);
typedef struct pt_temporal pt_temporal;
#define PT_TEMPORAL_EMPTY 1       /* pt_temporal_info's last_case (0: no frame since the last reset) */
#define PT_TEMPORAL_SAME_VIEW 2
#define PT_TEMPORAL_NEW_VIEW 3
int pt_temporal_create(int32_t width, int32_t height, const pt_temporal_params* params, pt_temporal** out); /* NULL: defaults */
int pt_temporal_destroy(pt_temporal* t);
int pt_temporal_reset(pt_temporal* t);                      /* the next frame finds no history */
int pt_temporal_info(const pt_temporal* t, int32_t* frames, float* batch_samples, int32_t* last_case);
/* One frame: the accumulator d_rgb of `samples` samples (finite, > 0), its G-buffer planes and albedo
 * (npix float4 each, as pt_gbuffer writes them) and the camera they were made with.  Device pointers,
 * asynchronous on `stream` (the caller orders the calls of one object).  Empty (first frame since a
 * reset): batch b = samples, c = rgb / samples.  Same view (cam byte-equal to the stored camera and
 * samples larger than the last frame's): b = samples - the last frame's, c = (rgb - prev) / b, in place;
 * the planes passed in are not read.  New view (anything else): b = samples, c = rgb / samples, and each
 * pixel takes the history of the four bilinear taps around its position in the stored view that lie on
 * its surface.  b must equal the first frame's since the last reset (PT_ERR_ARG otherwise). */
int pt_temporal_frame(pt_temporal* t, const pt_camera* cam, const float* d_rgb, float samples, const float* d_gA,
                      const float* d_gB, const float* d_alb, void* stream);
/* d_out_rgb (W*H float3): the mean, remodulated: per-sample radiance (pt_denoiser_run_var's rgb with
 * samples = 1).  d_out_var (W*H): the variance of lum(mean): max(0, mu2 - mu1^2) * b / h where
 * h >= min_frames * b, else the variance of lum(mean) over the 5 x 5 neighbours of the same material; 0
 * on a miss.  d_out_h (W*H): h.  Any may be NULL; they must not alias.  Needs a frame (PT_ERR_ARG). */
int pt_temporal_resolve(pt_temporal* t, float* d_out_rgb, float* d_out_var, float* d_out_h, void* stream);
/* Host arrays, synchronous (for tests and the Python functions).  pt_temporal_get: the planes of the
 * history as they stand, H0 (npix float4: mean, h), H1 (npix float2), gA, gB, prev (npix float3), alb;
 * any may be NULL. */
int pt_temporal_frame_host(pt_temporal* t, const pt_camera* cam, const float* rgb, float samples, const float* gA,
                           const float* gB, const float* alb);
int pt_temporal_get(pt_temporal* t, float* h_H0, float* h_H1, float* h_gA, float* h_gB, float* h_prev_rgb, float* h_alb);
/* A frame from a world == 1 context of the object's size (PT_ERR_ARG otherwise): its accumulator of
 * `samples` samples, a fresh first-hit G-buffer (none for a same-view frame) and the scene camera it was
 * created with.  Orders itself like pt_copy_image.  The object keeps nothing of the context. */
int pt_temporal_frame_ctx(pt_temporal* t, pt_ctx* c, float samples, void* stream);
/* Resolve, then with var_params pt_denoiser_run_var on the resolved image and variance (samples = 1),
 * then copy to the host: host_rgb (W*H float3), host_var (W*H; the filtered image's with var_params),
 * host_h (W*H); any may be NULL, not all.  Synchronous. */
int pt_temporal_image(pt_temporal* t, const pt_denoise_var_params* var_params, float* host_rgb, float* host_var,
                      float* host_h);

/* ---- adaptive sampling and region rendering through active-block masks ------- */
/* A BLOCK is 64 consecutive pixels in pt_get_image order — one word of the first bounce's camera
 * masks; the last block may be partial and blocks straddle rows when the width is no multiple of 64.
 * pt_adaptive needs no context.  Per pixel it keeps pt_moments' planes (prev, m1, m2) and a byte
 * `hot`; per block nb, the batches the block has received, and act (0 / 1).  Device pointers,
 * asynchronous on `stream` unless stated (the caller orders the calls of one object); the planes are
 * allocated at first use, so argument errors (PT_ERR_ARG) are found before any device call.
 *   reset:    m1 = m2 = 0, nb = 0 and act = 1 everywhere, prev = d_base_rgb (zeros when NULL)
 *   update:   pt_moments_update on the pixels of the blocks with act == 1, whose nb goes up by one;
 *             the pixels of the other blocks are not touched and their d_rgb is not read.
 *             batch_samples as pt_moments_update's
 *   select:   hot = 1 where nb < min_batches, else hot = e > threshold with
 *                 mean = m1 / nb, ex2 = m2 / nb, vm = max(0, ex2 - mean * mean) / (nb - 1),
 *                 e = sqrt(vm) / (mean + floor)        (a NaN is not hot)
 *             for every pixel, those of inactive blocks too; then act[b] = 1 iff some pixel of b has
 *             a hot pixel in the (2 dilate + 1)^2 box around it (clipped to the image).  With
 *             active_blocks / blocks non-NULL the call waits and returns the counts
 *   set_mask: act[b] = host_mask[b] != 0 for the nblocks == blocks bytes (synchronous)
 *   apply:    d_cmask_out[b] = act[b] ? d_cmask_in[b] : 0 for every block
 *   resolve:  d_out_rgb (W*H float3) = d_rgb / (nb * batch_samples), 0 where nb == 0; d_out_var (W*H)
 *             = pt_moments_variance's expression with the block's nb as the batch count and
 *             samples = nb * batch_samples, 0 where nb < 2: pt_denoiser_run_var's inputs with
 *             samples = 1.  Either may be NULL; outputs must not alias d_rgb.  Needs an update
 *   get:      synchronous, host arrays: m1, m2 (npix), prev (npix * 3), nb, act (blocks, uint32), hot
 *             (npix bytes); any may be NULL (for tests) */
typedef struct pt_adaptive_params {
    float threshold;              /* relative standard error of the pixel's mean luminance; finite, >= 0 */
    float floor;                  /* added to the mean in e's divisor; finite, > 0 */
    int32_t min_batches;          /* >= 2: blocks with fewer batches stay active */
    int32_t dilate;               /* 0..2 */
    int32_t reserved[4];
} pt_adaptive_params;
void pt_adaptive_params_default(pt_adaptive_params* p);
typedef struct pt_adaptive pt_adaptive;
int pt_adaptive_obj_create(int32_t width, int32_t height, pt_adaptive** out);
int pt_adaptive_obj_destroy(pt_adaptive* a);
int pt_adaptive_obj_info(const pt_adaptive* a, int32_t* blocks, int32_t* updates, float* batch_samples);
int pt_adaptive_obj_reset(pt_adaptive* a, const float* d_base_rgb, void* stream);
int pt_adaptive_obj_update(pt_adaptive* a, const float* d_rgb, float batch_samples, const float* d_alb, void* stream);
int pt_adaptive_obj_select(pt_adaptive* a, const pt_adaptive_params* p, void* stream, int32_t* active_blocks,
                           int32_t* blocks);
int pt_adaptive_obj_set_mask(pt_adaptive* a, const uint8_t* host_mask, int32_t nblocks, void* stream);
int pt_adaptive_obj_apply(pt_adaptive* a, const uint32_t* d_cmask_in, uint32_t* d_cmask_out, void* stream);
int pt_adaptive_obj_resolve(pt_adaptive* a, const float* d_rgb, float* d_out_rgb, float* d_out_var, void* stream);
int pt_adaptive_obj_get(pt_adaptive* a, float* h_m1, float* h_m2, float* h_prev_rgb, uint32_t* h_nb, uint32_t* h_act,
                        uint8_t* h_hot);

/* Adaptive sampling of a context: a pt_adaptive over its accumulator whose act gates the first
 * bounce.  While enabled the first-bounce kernels read a second mask buffer, word b = act[b] ? the
 * camera mask of block b : 0; a zero word makes the block's camera rays misses that draw no random
 * number and store nothing, so the later bounces hold paths of the active blocks only.  Under
 * rng_key_pixel a pass traced through a mask gives every pixel of an active block the bits of the same
 * pass traced in full and leaves every other pixel's accumulator as it was.
 * pt_adaptive_enable(c, 1) needs all of (PT_ERR_ARG otherwise, the message names the condition):
 *   - world == 1: the object covers the whole image;
 *   - camera masks (an analytic scene of <= 32 geoms without triangles, PT_AMD_NO_CMASK unset): the
 *     mesh walk of the first bounce (k_traverse4<FIRST>) reads no mask;
 *   - the fused or the material-sorted pipeline: the split pipeline (PT_PIPELINE=split) ORs the words
 *     of up to four blocks per wave, so an inactive block beside an active one would be traced;
 *   - PT_AMD_VERIFY_BOUNDS off: the verifying kernels compare against a plain per-geom loop that
 *     ignores the masks;
 *   - no variance tracking (pt_track_variance; and pt_track_variance(c, 1) is refused while adaptive).
 * It starts from the accumulator as it stands, every block active with nb = 0; (c, 0) frees everything
 * and the first bounce reads the camera masks again.
 * pt_adaptive_update: after a pass (batch = the context's spp), like pt_variance_update.
 * pt_adaptive_select / pt_adaptive_set_mask change act: synchronous; they wait for the context's queued
 * work (queued first bounces read the mask), drop unclaimed render-ahead work, rebuild the effective
 * masks and choose the empty-wave first bounce from them as pt_create does from the camera masks.
 * pt_set_flags re-applies act when it rebuilds the camera masks; pt_reset_image resets the object (every
 * block active, nb = 0) and, because that changes the masks, waits for its stream on such a context;
 * pt_set_accum is refused (a saved accumulator carries no per-block counts).  pt_stats' bounce_live[0]
 * still counts every pixel.  pt_preview_rgba divides by one count and is not adaptive-aware.
 * pt_adaptive_image: resolve, then with var_params pt_denoiser_run_var (samples = 1) over a fresh
 * first-hit G-buffer; host_rgb (npix float3), host_var (npix, the filtered variance with var_params);
 * either may be NULL, not both.  Synchronous. */
int pt_adaptive_enable(pt_ctx* c, int32_t on);
int pt_adaptive_update(pt_ctx* c, int32_t demodulate, void* stream);
int pt_adaptive_select(pt_ctx* c, const pt_adaptive_params* p, int32_t* active_blocks, int32_t* blocks);
int pt_adaptive_set_mask(pt_ctx* c, const uint8_t* host_mask, int32_t nblocks);
int pt_adaptive_info(const pt_ctx* c, int32_t* on, int32_t* blocks, int32_t* active_blocks, int32_t* updates,
                     float* batch_samples);
int pt_adaptive_get(pt_ctx* c, float* h_m1, float* h_m2, float* h_prev_rgb, uint32_t* h_nb, uint32_t* h_act,
                    uint8_t* h_hot);
int pt_adaptive_image(pt_ctx* c, const pt_denoise_var_params* var_params, float* host_rgb, float* host_var);

/* ---- baseline JPEG encoding on the device ------------------------------------ */
/* A JFIF file (SOF0, 8-bit, YCbCr 4:4:4 or 4:2:0, the Annex K quantisation tables scaled by the IJG
 * quality rule, the Annex K Huffman tables, one scan, no restart markers) of width x height pixels,
 * encoded on the device in exactly defined int32 arithmetic: the bytes are a function of the input
 * bytes.  mirror_x reads column W-1-x (saveImage's and the preview window's orientation).  The object
 * needs no context; pt_jpeg_enc_create touches no device (argument errors, PT_ERR_ARG, are found before
 * any device call) and the scratch, sized for the worst case, is allocated at the first encode; later
 * encodes neither allocate nor synchronise.  Width and height in 1..65535 with blocks * 1664 < 2^31
 * (blocks: 8x8 blocks of all components, the image padded to whole MCUs). */
#define PT_JPEG_444 0
#define PT_JPEG_420 1
typedef struct pt_jpeg_params {
    int32_t quality;      /* 1..100, default 90 */
    int32_t subsampling;  /* default PT_JPEG_420 */
    int32_t mirror_x;     /* default 0 */
    int32_t reserved[5];
} pt_jpeg_params;
void pt_jpeg_params_default(pt_jpeg_params* p);
typedef struct pt_jpeg_enc pt_jpeg_enc;
int pt_jpeg_enc_create(int32_t width, int32_t height, const pt_jpeg_params* p, pt_jpeg_enc** out);
int pt_jpeg_enc_destroy(pt_jpeg_enc* e);
/* The largest file an encode can write: header (623) + 2 x (blocks * 1664 / 8) + 2.  No device. */
int64_t pt_jpeg_enc_bound(const pt_jpeg_enc* e);
/* Inspection (host only, used by the tests): the file header SOI .. SOS, built at creation.  Returns its
 * length and copies min(length, cap) bytes. */
int64_t pt_jpeg_enc_header(const pt_jpeg_enc* e, uint8_t* out, int64_t cap);
/* Asynchronous on `stream`, device pointers (the caller orders the calls of one object).  d_pix: RGB8 or
 * RGBA8, pixel_stride 3 or 4, alpha ignored.  d_rgb: the float accumulator of `samples` samples (finite,
 * > 0), whose bytes are pt_preview_rgba's.  The file goes to d_out and its size to *d_size (8-byte
 * aligned); a file that does not fit cap leaves the negated size it needs in *d_size, and no byte at or
 * beyond d_out + cap is written. */
int pt_jpeg_enc_pixels(pt_jpeg_enc* e, const uint8_t* d_pix, int32_t pixel_stride,
                       uint8_t* d_out, int64_t cap, int64_t* d_size, void* stream);
int pt_jpeg_enc_accum(pt_jpeg_enc* e, const float* d_rgb, float samples,
                      uint8_t* d_out, int64_t cap, int64_t* d_size, void* stream);
/* Host arrays, synchronous.  A file larger than cap: PT_ERR_ARG, the size it needs in *size. */
int pt_jpeg_encode_host(int32_t width, int32_t height, const uint8_t* pix, int32_t pixel_stride,
                        const pt_jpeg_params* p, uint8_t* out, int64_t cap, int64_t* size);
/* The context's accumulated image of `iter` iterations as pt_preview_rgba converts it, encoded by `e`
 * (whose size must be the tile's, PT_ERR_ARG otherwise).  Orders itself like pt_preview_rgba. */
int pt_preview_jpeg(pt_ctx* c, int32_t iter, pt_jpeg_enc* e, uint8_t* d_out, int64_t cap,
                    int64_t* d_size, void* stream);
/* Stage timing of an encoder (scripts/jpeg_time.py): while on, an encode records events around its
 * stages; read waits for the last encode and returns the milliseconds of blocks, count, scan, emit and
 * stuffing. */
int pt_jpeg_enc_profile(pt_jpeg_enc* e, int32_t on);
int pt_jpeg_enc_profile_read(pt_jpeg_enc* e, float ms[5]);

/* ---- PNG encoding on the device ---------------------------------------------- */
/* An 8-bit RGB PNG (colour type 2, no interlace; signature, IHDR, one IDAT holding one zlib stream, IEND)
 * of width x height pixels, written entirely by kernels: row filtering (a fixed type 0..4, or per row the
 * type with the smallest sum of |signed residual|, ties to the lowest), literals and distance-1 matches
 * within 512-byte lane chunks of the filtered stream, one deflate block per block_bytes coded with the
 * fixed or a dynamic Huffman code (whichever is shorter, ties to fixed; no stored blocks), Adler-32 and
 * CRC-32.  The bytes are a function of the input bytes.  mirror_x reads column W-1-x.  The object needs
 * no context; pt_png_enc_create touches no device (argument errors, PT_ERR_ARG, are found before any
 * device call) and the scratch, sized for the worst case, is allocated at the first encode; later encodes
 * neither allocate nor synchronise.  Sizes whose stream bound 9 N + 10 blocks bits (N = H (1 + 3 W)) does
 * not stay below 2^31 are refused. */
#define PT_PNG_FILTER_ADAPTIVE 5
#define PT_PNG_CONV_PREVIEW 0 /* pt_preview_rgba's bytes: (int)((double)(v / n) * 255.0), clamped */
#define PT_PNG_CONV_SAVE 1    /* pt_tonemap's bytes: float division, clamp to 0..1, (uint8_t)(v * 255.f) */
typedef struct pt_png_params {
    int32_t filter;       /* 0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth, default PT_PNG_FILTER_ADAPTIVE */
    int32_t block_bytes;  /* bytes of the filtered stream per deflate block: a multiple of 512 in
                           * 1024..1048576, default 32768 */
    int32_t conv;         /* how pt_png_enc_accum converts the accumulator, default PT_PNG_CONV_PREVIEW */
    int32_t mirror_x;     /* default 0 */
    int32_t reserved[4];
} pt_png_params;
void pt_png_params_default(pt_png_params* p);
typedef struct pt_png_enc pt_png_enc;
int pt_png_enc_create(int32_t width, int32_t height, const pt_png_params* p, pt_png_enc** out);
int pt_png_enc_destroy(pt_png_enc* e);
/* The largest file an encode can write: (9 N + 10 blocks + 7) / 8 + 63 bytes of framing.  No device. */
int64_t pt_png_enc_bound(const pt_png_enc* e);
/* Asynchronous on `stream`, device pointers (the caller orders the calls of one object).  d_pix: RGB8 or
 * RGBA8, pixel_stride 3 or 4, alpha ignored.  d_rgb: the float accumulator of `samples` samples (finite,
 * > 0), converted as params.conv says.  The file goes to d_out and its size to *d_size (8-byte aligned); a
 * file that does not fit cap leaves the negated size it needs in *d_size, and no byte at or beyond
 * d_out + cap is written. */
int pt_png_enc_pixels(pt_png_enc* e, const uint8_t* d_pix, int32_t pixel_stride,
                      uint8_t* d_out, int64_t cap, int64_t* d_size, void* stream);
int pt_png_enc_accum(pt_png_enc* e, const float* d_rgb, float samples,
                     uint8_t* d_out, int64_t cap, int64_t* d_size, void* stream);
/* Host arrays, synchronous.  A file larger than cap: PT_ERR_ARG, the size it needs in *size. */
int pt_png_encode_host(int32_t width, int32_t height, const uint8_t* pix, int32_t pixel_stride,
                       const pt_png_params* p, uint8_t* out, int64_t cap, int64_t* size);
/* The context's accumulated image divided by `iter`, encoded by `e` (whose size must be the tile's,
 * PT_ERR_ARG otherwise; a sharded context, world > 1, is refused).  Orders itself like pt_preview_rgba. */
int pt_preview_png(pt_ctx* c, int32_t iter, pt_png_enc* e, uint8_t* d_out, int64_t cap,
                   int64_t* d_size, void* stream);
/* Stage timing of an encoder (scripts/png_time.py): while on, an encode records events around its stages;
 * read waits for the last encode and returns the milliseconds of filter, block codes and count, scan,
 * zero and emit, checksums, and the output copy with the framing. */
int pt_png_enc_profile(pt_png_enc* e, int32_t on);
int pt_png_enc_profile_read(pt_png_enc* e, float ms[6]);

/* ---- Radiance HDR encoding on the device ------------------------------------- */
/* The file of pt_encode_hdr, byte for byte, written by kernels from the float accumulator: the same header,
 * RGBE pixels of rgb / samples, and for 8 <= width <= 32767 the per-channel run-length coding of every scanline
 * (flat RGBE rows otherwise).  mirror_x = 1 is pt_encode_hdr's orientation (input column x lands at
 * width-1-x); the default 0 keeps the input's.  The contract covers finite values whose scaled components stay
 * below 2^31 in magnitude (a negative component beside a positive maximum, whose byte C++ leaves undefined in
 * pt_encode_hdr, gets the byte the host library's x86 code gives it: in R and G 0 down to -32768, in B the low
 * byte of the truncation); NaN, infinities and larger values are outside it.  The object
 * needs no context; pt_hdr_enc_create touches no device (argument errors, PT_ERR_ARG, are found before any
 * device call) and the scratch is allocated at the first encode; later encodes neither allocate nor
 * synchronise.  Sizes whose bound reaches 2^31 are refused. */
typedef struct pt_hdr_params {
    int32_t mirror_x;     /* default 0 */
    int32_t reserved[7];
} pt_hdr_params;
void pt_hdr_params_default(pt_hdr_params* p);
typedef struct pt_hdr_enc pt_hdr_enc;
int pt_hdr_enc_create(int32_t width, int32_t height, const pt_hdr_params* p, pt_hdr_enc** out);
int pt_hdr_enc_destroy(pt_hdr_enc* e);
/* The largest file an encode can write: the header + H (4 + 4 (W + ceil(W / 128))) for coded rows, the header
 * + 4 W H (the file's size) for flat ones.  No device. */
int64_t pt_hdr_enc_bound(const pt_hdr_enc* e);
/* Asynchronous on `stream`, device pointers (the caller orders the calls of one object).  d_rgb: the float
 * accumulator of `samples` samples (finite, > 0).  The file goes to d_out and its size to *d_size (8-byte
 * aligned); a file that does not fit cap leaves the negated size it needs in *d_size, and no byte at or beyond
 * d_out + cap is written. */
int pt_hdr_enc_accum(pt_hdr_enc* e, const float* d_rgb, float samples,
                     uint8_t* d_out, int64_t cap, int64_t* d_size, void* stream);
/* A host array, synchronous.  A file larger than cap: PT_ERR_ARG, the size it needs in *size. */
int pt_hdr_encode_host(int32_t width, int32_t height, const float* rgb, float samples,
                       const pt_hdr_params* p, uint8_t* out, int64_t cap, int64_t* size);
/* The context's accumulated image divided by `iter`, encoded by `e` (whose size must be the tile's,
 * PT_ERR_ARG otherwise; a sharded context, world > 1, is refused).  Orders itself like pt_preview_rgba. */
int pt_preview_hdr(pt_ctx* c, int32_t iter, pt_hdr_enc* e, uint8_t* d_out, int64_t cap,
                   int64_t* d_size, void* stream);
/* Stage timing of an encoder (scripts/hdr_time.py): while on, an encode records events around its stages;
 * read waits for the last encode and returns the milliseconds of convert, count, scan and emit. */
int pt_hdr_enc_profile(pt_hdr_enc* e, int32_t on);
int pt_hdr_enc_profile_read(pt_hdr_enc* e, float ms[4]);

/* ---- OpenEXR encoding on the device ------------------------------------------- */
/* A single-part scanline OpenEXR 2.0 file of width x height pixels and 1 to 16 channels, written entirely by
 * kernels from float planes in device memory: uncompressed, or ZIPS / ZIP (one zlib stream per 1 / 16 scanlines
 * over the byte-split, differenced chunk, coded by §15's run-length deflate; the chunk's raw bytes where the
 * stream would not be shorter).  DESIGN.md §18 defines every byte of the file.  The value of channel k at a pixel
 * is plane_k.d[pixel * stride] / divisor (one float32 division; a divisor of 1 is the identity), `pixel` in
 * pt_get_image's order; FLOAT stores its bits, HALF the IEEE round-to-nearest-even half (subnormals kept, overflow
 * to infinity, NaN as sign | 0x7e00), UINT the plane word's 32 bits unchanged (the divisor is ignored).
 * mirror_x reads column W-1-x.  The object needs no context; pt_exr_enc_create touches no device (argument
 * errors, PT_ERR_ARG, are found before any device call) and the scratch is allocated at the first encode; later
 * encodes neither allocate nor synchronise.  Sizes whose bound reaches 2^31, or whose stream bound
 * 16 + 9 n + 10 blocks bits (n the bytes of 1 / 16 scanlines) does, are refused. */
#define PT_EXR_UINT 0
#define PT_EXR_HALF 1
#define PT_EXR_FLOAT 2
#define PT_EXR_NONE 0
#define PT_EXR_ZIPS 2 /* one zlib stream per scanline */
#define PT_EXR_ZIP 3  /* one per 16 scanlines */
typedef struct pt_exr_params {
    int32_t compression;  /* default PT_EXR_ZIP */
    int32_t block_bytes;  /* bytes of a stream per deflate block: a multiple of 512 in 1024..1048576, default 32768 */
    int32_t mirror_x;     /* default 0 */
    int32_t reserved[5];
} pt_exr_params;
void pt_exr_params_default(pt_exr_params* p);
typedef struct pt_exr_channel {
    char name[32];        /* 1 to 31 bytes of [A-Za-z0-9_.], zero-terminated; distinct within a file */
    int32_t type;         /* PT_EXR_UINT, PT_EXR_HALF or PT_EXR_FLOAT */
} pt_exr_channel;
typedef struct pt_exr_plane {
    const float* d;       /* device memory; planes may alias each other, none may overlap the output */
    int32_t stride;       /* floats between two pixels, >= 1 */
    float divisor;        /* finite, > 0 */
} pt_exr_plane;
typedef struct pt_exr_enc pt_exr_enc;
/* The channels in any order: the file lists them sorted by the bytes of their names, and an encode takes its
 * planes in the order given here. */
int pt_exr_enc_create(int32_t width, int32_t height, const pt_exr_channel* channels, int32_t nchannels,
                      const pt_exr_params* p, pt_exr_enc** out);
int pt_exr_enc_destroy(pt_exr_enc* e);
/* The uncompressed file's size, header + 8 chunks + the sum over the chunks of (8 + n): the raw fallback makes it
 * a bound for every compression.  No device. */
int64_t pt_exr_enc_bound(const pt_exr_enc* e);
/* The file from its magic number through the header's final zero byte, to buf (at most cap bytes; NULL: the
 * length only); returns the length.  No device. */
int64_t pt_exr_enc_header(const pt_exr_enc* e, uint8_t* buf, int64_t cap);
/* Asynchronous on `stream`, device pointers (the caller orders the calls of one object): one plane per channel.
 * The file goes to d_out and its size to *d_size (8-byte aligned); a file that does not fit cap leaves the
 * negated size it needs in *d_size, and no byte at or beyond d_out + cap is written. */
int pt_exr_enc_planes(pt_exr_enc* e, const pt_exr_plane* planes, uint8_t* d_out, int64_t cap, int64_t* d_size,
                      void* stream);
/* Host arrays, synchronous: plane k holds width * height * strides[k] floats (strides NULL: all 1; divisors
 * NULL: all 1).  A file larger than cap: PT_ERR_ARG, the size it needs in *size. */
int pt_exr_encode_host(int32_t width, int32_t height, const pt_exr_channel* channels, int32_t nchannels,
                       const float* const* planes, const int32_t* strides, const float* divisors,
                       const pt_exr_params* p, uint8_t* out, int64_t cap, int64_t* size);
/* Stage timing of an encoder: while on, an encode records events around its stages; read waits for the last
 * encode and returns the milliseconds of convert and difference, block codes and count, the per-stream scan, zero
 * and emit, checksums and chunk sizes, and the output copy with the table and header. */
int pt_exr_enc_profile(pt_exr_enc* e, int32_t on);
int pt_exr_enc_profile_read(pt_exr_enc* e, float ms[6]);
/* The layers a render context can write, and their channels:
 *   PT_EXR_BEAUTY    R, G, B                        the accumulator / iter
 *   PT_EXR_ALBEDO    albedo.R, albedo.G, albedo.B   pt_gbuffer's alb
 *   PT_EXR_NORMAL    N.X, N.Y, N.Z                  gA
 *   PT_EXR_POSITION  P.X, P.Y, P.Z                  gB, always FLOAT
 *   PT_EXR_DEPTH     Z                              gB's t (-1 on a miss), always FLOAT
 *   PT_EXR_UV        UV.U, UV.V                     uv
 *   PT_EXR_ID        id                             gA's material id bits, UINT
 * pt_exr_ctx_channels lists the channels of `layers` (a non-empty mask) in this order, FLOAT, or HALF for the
 * layers of `half` that may be HALF (the other bits of `half` are ignored).  No device. */
#define PT_EXR_BEAUTY 1
#define PT_EXR_ALBEDO 2
#define PT_EXR_NORMAL 4
#define PT_EXR_POSITION 8
#define PT_EXR_DEPTH 16
#define PT_EXR_UV 32
#define PT_EXR_ID 64
#define PT_EXR_ALL_LAYERS 127
int pt_exr_ctx_channels(int32_t layers, int32_t half, pt_exr_channel out[16], int32_t* n);
/* The context's layers encoded by `e`, whose size must be the tile's and whose channels must be
 * pt_exr_ctx_channels(layers, half)'s for some `half` (PT_ERR_ARG otherwise; a sharded context, world > 1, is
 * refused).  Layers other than the beauty come from pt_gbuffer into a scratch of 14 floats per pixel that the
 * context keeps until pt_destroy.  Orders itself like pt_preview_rgba. */
int pt_preview_exr(pt_ctx* c, int32_t iter, int32_t layers, pt_exr_enc* e, uint8_t* d_out, int64_t cap,
                   int64_t* d_size, void* stream);

/* ---- display transform on the device ------------------------------------------ */
/* The float accumulator to display bytes (RGB8 or RGBA8 with alpha 0): an exposure multiplier, manual or
 * metered from a luminance histogram, a tone curve, the clamp to 0..1 and a transfer function.  The bytes
 * are an exact function of the input floats (DESIGN.md §17 is the definition; tests/display_ref.py restates
 * it in numpy); the defaults reproduce pt_tonemap's conversion.  The object needs no context;
 * pt_display_create touches no device (argument errors, PT_ERR_ARG, are found before any device call), the
 * scratch is allocated at first use, and later calls neither allocate nor synchronise. */
#define PT_DISPLAY_MANUAL 0
#define PT_DISPLAY_AUTO 1
#define PT_DISPLAY_NONE 0
#define PT_DISPLAY_REINHARD 1 /* extended Reinhard, parameter `white` */
#define PT_DISPLAY_ACES 2     /* Narkowicz's rational fit */
#define PT_DISPLAY_HABLE 3    /* Uncharted 2, W = 11.2 */
#define PT_DISPLAY_LINEAR 0   /* (uint8_t)(c * 255.f): pt_tonemap's byte */
#define PT_DISPLAY_SRGB 1     /* the correctly rounded sRGB byte, floor(255 oetf(c) + 0.5) */
typedef struct pt_display_params {
    int32_t exposure_mode;  /* default PT_DISPLAY_MANUAL */
    float exposure;         /* the multiplier in manual mode, finite and > 0, default 1 */
    float key_value;        /* auto: the luminance the metered level is mapped to, default 0.18 */
    float compensation_ev;  /* auto: added to the target, in stops, -64..64, default 0 */
    float min_ev, max_ev;   /* auto: limits of the exposure in stops, -64 <= min <= max <= 64, default -8, 8 */
    int32_t pct_lo, pct_hi; /* auto: the ranks metered, in 1/1024 of the counted pixels, 0 <= lo < hi <= 1024,
                             * default 102, 922 */
    int32_t rate;           /* auto: the share of the way to the target a metering goes, in 1/256, 1..256,
                             * default 256 (no adaptation) */
    int32_t curve;          /* default PT_DISPLAY_NONE */
    float white;            /* PT_DISPLAY_REINHARD: the radiance mapped to 1, finite and > 0, default 4 */
    int32_t transfer;       /* default PT_DISPLAY_LINEAR */
    int32_t mirror_x;       /* default 0; 1: input column x lands at width-1-x */
    int32_t reserved[3];
} pt_display_params;
void pt_display_params_default(pt_display_params* p);
typedef struct pt_display pt_display;
int pt_display_create(int32_t width, int32_t height, const pt_display_params* p, pt_display** out);
int pt_display_destroy(pt_display* d);
/* Asynchronous on `stream`, device pointers (the caller orders the calls of one object); nothing waits for
 * the host.  d_rgb: the float accumulator of `samples` samples (finite, > 0).
 * meter: the luminance histogram of d_rgb / samples, then the exposure state's step towards its target.
 *        The first metering after create or reset jumps to the target; an image without a counted pixel
 *        changes nothing.
 * apply: the bytes to d_pix (pixel_stride 3 or 4, width * height * pixel_stride bytes, no byte beyond them);
 *        auto mode reads the multiplier the last metering left on the device (1 before any).  d_pix must
 *        not alias d_rgb.
 * frame: meter, then apply.   reset: the next metering jumps again. */
int pt_display_meter(pt_display* d, const float* d_rgb, float samples, void* stream);
int pt_display_apply(pt_display* d, const float* d_rgb, float samples, uint8_t* d_pix,
                     int32_t pixel_stride, void* stream);
int pt_display_frame(pt_display* d, const float* d_rgb, float samples, uint8_t* d_pix,
                     int32_t pixel_stride, void* stream);
int pt_display_reset(pt_display* d, void* stream);
/* A host array, synchronous: one object made, used (frame in auto mode, apply otherwise) and destroyed. */
int pt_display_host(int32_t width, int32_t height, const float* rgb, float samples,
                    const pt_display_params* p, uint8_t* out, int32_t pixel_stride);
/* Inspection (synchronous, for tests): the histogram as last resolved (hist[256]: the uncounted pixels),
 * the exposure state in 1/256 octave, the multiplier apply uses, and whether a metering has set the state
 * since create or reset.  Any pointer may be NULL. */
int pt_display_info(pt_display* d, uint32_t hist[257], int32_t* e, float* mult, int32_t* metered);
/* Host only, no device: the sRGB thresholds T[1..255] (srgb[0] is 0 and not a threshold), P[k] =
 * (float)exp2(k / 256.0), and the Hable curve's divisor f(11.2f). */
void pt_display_tables(float srgb[256], float pow2[256], float* hable_white);
/* The context's accumulated image of `iter` iterations through `d` (metering first in auto mode) into the
 * caller's device buffer.  d's size must be the tile's and world must be 1 (PT_ERR_ARG otherwise).  Orders
 * itself like pt_preview_rgba. */
int pt_preview_display(pt_ctx* c, int32_t iter, pt_display* d, uint8_t* d_pix, int32_t pixel_stride,
                       void* stream);

/* ---- bloom on the device ------------------------------------------------------- */
/* The float accumulator plus its glare, in the accumulator's own unit: a bright pass, a pyramid of K levels
 * through the binomial [1 3 3 1]/8, a 2x tent on the way back up, and out = v + glare * samples.  The output
 * is an exact function of the input floats (DESIGN.md §20 is the definition; tests/bloom_ref.py restates it
 * in numpy).  It feeds whatever takes an accumulator: pt_display_*, the encoders' accum entries.  The object
 * needs no context; pt_bloom_create touches no device (argument errors, PT_ERR_ARG, are found before any
 * device call), the pyramid is allocated at first use, and later calls neither allocate nor synchronise. */
typedef struct pt_bloom_params {
    float threshold;   /* luminance above which a pixel glares, finite and >= 0, default 1 */
    float strength;    /* the glare's weight in the output, finite and >= 0, default 0.25 */
    float spread;      /* the weight of each coarser level relative to the finer, 0 < spread <= 1, default 0.75 */
    float clamp;       /* per-channel ceiling of the bright pass, 0 < clamp <= 65504, default 65504 */
    int32_t levels;    /* default 0: K = clamp(floor(log2(min(width, height))), 1, 6); else K, 1 .. 12 */
    int32_t reserved[3];
} pt_bloom_params;
void pt_bloom_params_default(pt_bloom_params* p);
typedef struct pt_bloom pt_bloom;
int pt_bloom_create(int32_t width, int32_t height, const pt_bloom_params* p, pt_bloom** out);
int pt_bloom_destroy(pt_bloom* b);
/* Asynchronous on `stream`, device pointers aligned to 4 bytes (the caller orders the calls of one object);
 * nothing waits for the host.  d_rgb: the float accumulator of `samples` samples (finite, > 0); d_out: as many
 * floats, d_rgb itself (in place) or memory that does not overlap it (PT_ERR_ARG otherwise). */
int pt_bloom_apply(pt_bloom* b, const float* d_rgb, float samples, float* d_out, void* stream);
/* Host arrays, synchronous: one object made, used and destroyed. */
int pt_bloom_host(int32_t width, int32_t height, const float* rgb, float samples, const pt_bloom_params* p,
                  float* out);
/* The K in use and the sizes of the levels 1 .. K (the other entries 0); no device.  Any pointer may be NULL. */
int pt_bloom_info(pt_bloom* b, int32_t* levels, int32_t widths[12], int32_t heights[12]);
/* The context's accumulated image of `iter` iterations through `b` into the caller's device buffer of as many
 * floats.  b's size must be the tile's and world must be 1 (PT_ERR_ARG otherwise).  Orders itself like
 * pt_preview_rgba. */
int pt_preview_bloom(pt_ctx* c, int32_t iter, pt_bloom* b, float* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PT_AMD_H */
