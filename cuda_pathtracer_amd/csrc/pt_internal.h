// Internal host-side types and checks shared by the scene loader, mesh/BVH builder, image-level objects and render context.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_layout.h"

namespace pt {

extern thread_local std::string g_err;
int fail(int code, const std::string& msg);

struct TextureHost {
    std::string path;            // TEXTURE_FILE of a JSON scene (decoded by the loader, pt_jpeg.cpp)
    int32_t width = 0, height = 0, components = 0;
    std::vector<uint8_t> pixels;
};

// The environment (pt_env.cpp): the padded octahedral map as the device reads it.
struct EnvHost {
    int32_t n = 0;               // 0: none
    pt_env_params params{};      // as given (size: the n in use)
    float rot[9] = {};           // row-major world-to-map rotation of params.rotate_deg
    std::vector<float> rgba;     // (n + 2)^2 * 4
};

struct Scene {
    EnvHost env;
    std::vector<pt_geom> geoms;
    std::vector<pt_material> materials;
    std::vector<pt_triangle> tris_load;     // mesh triangles in load order (ids = index here)
    std::vector<pt_triangle> triangles;     // BVH leaf order, built from tris_load by finalize
    std::vector<pt_bvh_node> bvh;
    std::vector<TextureHost> textures;
    pt_camera camera{};
    float fovy = 45.0f;
    float eye[3] = {0, 0, 0}, look_at[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    float orbit[3] = {0, 0, 0};   // phi, theta, zoom of the loaded camera (main.cpp:59-73), set by finalize
    int32_t iterations = 1, depth = 8;
    std::string file = "render";
    bool camera_set = false;
    bool finalized = false;
    bool bvh_built = false;
    int32_t bvh_builder = 0;     // requested: 0 host (pt_mesh.cpp), 1 device (bvh_build.hip)
    int32_t bvh_on_device = 0;   // the last build ran on the device
    double bvh_ms = 0.0;         // the last build's wall time (host clock)
};

int scene_add_geom(Scene& S, int32_t type, int32_t mat, const float* t, const float* r, const float* s);
int scene_finalize(Scene& S);
// Mesh / BVH (pt_mesh.cpp)
int load_obj_mesh(Scene& S, const std::string& path, int32_t mat, const float* t, const float* r, const float* s);
int add_mesh(Scene& S, int32_t mat, const float* t, const float* r, const float* s, const float* pos, int32_t npos,
             const float* nrm, int32_t nnrm, const float* uv, int32_t nuv, const int32_t* face_sizes, int32_t nfaces,
             const int32_t* ip, const int32_t* in, const int32_t* it, int32_t* id_out);
int build_bvh(Scene& S);
// Device SAH build (bvh_build.hip): PT_OK, 1 = not on the device (the caller builds on the host), or an error.
int build_bvh_device(Scene& S, double* ms);
// JPEG textures (pt_jpeg.cpp): stbi_load(path, ..., req_comp = 0) restated
int decode_jpeg(const uint8_t* data, size_t size, int32_t* width, int32_t* height, int32_t* components,
                std::vector<uint8_t>* pixels);
int load_texture_file(TextureHost& t);
// Environment (pt_env.cpp): a Radiance .hdr file resampled onto the scene's octahedral map
int load_environment_file(Scene& S, const std::string& path, const pt_env_params* params);
// Denoiser (pt_denoise.hip): the argument checks of pt_denoiser_run that need no device
int denoise_check(const pt_denoise_params* p, float samples);
int denoise_var_check(const pt_denoise_var_params* p, float samples);
// pt_moments: the argument checks of pt_moments_update / pt_moments_variance that need no device
int moments_update_check(const pt_moments* m, float batch_samples);
int moments_variance_check(const pt_moments* m, float samples);
// pt_adaptive (pt_adaptive.hip): the argument checks of select and update that need no device
int adaptive_params_check(const pt_adaptive_params* p);
int adaptive_update_check(const pt_adaptive* a, float batch_samples);
// pt_temporal (pt_temporal.hip): the case a frame takes (PT_TEMPORAL_*; < 0: the negated error of its
// argument checks, no device needed), and the object's own planes a frame of that case writes its
// G-buffer and albedo to (a producer fills them and passes them to pt_temporal_frame: no copy)
int temporal_case(const pt_temporal* t, const pt_camera* cam, float samples);
int temporal_staging(pt_temporal* t, int kind, float** gA, float** gB, float** alb);
int temporal_size(const pt_temporal* t, int32_t* width, int32_t* height);
// The device encoders (pt_enc.h): what every object begins with, and the image size one was created for (e not null)
struct EncHead;
const EncHead* enc_head(const pt_jpeg_enc* e);
const EncHead* enc_head(const pt_png_enc* e);
const EncHead* enc_head(const pt_hdr_enc* e);
const EncHead* enc_head(const pt_exr_enc* e);
void enc_size(const EncHead* e, int32_t* width, int32_t* height);
// pt_exr_enc (pt_exr_enc.hip): the channels it was created with, in creation order (e not null)
void exr_channels(const pt_exr_enc* e, const pt_exr_channel** channels, int32_t* n);
// pt_display (pt_display.hip): the image size it was created for and whether its exposure is metered
int display_size(const pt_display* d, int32_t* width, int32_t* height, int32_t* automatic);
// pt_bloom (pt_bloom.hip): the image size it was created for
int bloom_size(const pt_bloom* b, int32_t* width, int32_t* height);

inline float bits_to_float(int32_t v) {
    float f;
    std::memcpy(&f, &v, 4);
    return f;
}
inline int32_t __float_as_int_host(float f) {
    int32_t v;
    std::memcpy(&v, &f, 4);
    return v;
}

// Scene preparation of the bounded closest hit (pt_bounds.cpp; no device needed).  What a context
// keeps on the host to re-derive the bounds when the lens changes (pt_set_flags):
struct BoundsHost {
    std::vector<ptd::DGeom> geoms;   // host copy of the geom table
    std::vector<float> wtight;       // bkind 3: the widened cube's world hull before the pad, rounded outward,
                                     // (lo, hi) of axis r at [6 * geom + 2 * r] (update_bounds; find_room's room.in)
    double scene_ext = 0.0;          // max |coordinate| over every surface and the camera position
    double R = 0.0;                  // update_bounds: the largest |coordinate| of a ray origin the bounds are sized for
    double r_limit = 0.0;            // update_bounds: the largest R for which no bound form of this scene overflows
    bool unbounded = false;          // R > r_limit: every geom carries a bound that claims nothing (update_bounds)
    float abs_slack = 0.0f;          // SceneDev::abs_slack
    float wb_tslack = 0.0f;          // SceneDev::wb_tslack
    ptd::RoomDev room{};             // SceneDev::room
};
BoundsHost make_dgeoms(const Scene& S);
void update_bounds(BoundsHost& B, float aperture);   // (ends with find_room)
void find_room(BoundsHost& B);
void bound_order(const BoundsHost& B, std::vector<ptd::DGeom>& out, int32_t bk[6]);
void camera_masks(const BoundsHost& B, const ptd::CamDev& cam, const ptd::FlagsDev& fl, const ptd::TileDev& T,
                  std::vector<uint32_t>& mask);
void room_info(const ptd::RoomDev& room, int32_t* walls, int32_t* faces, float* lo, float* hi);
// BVH layouts of the walk kernels (pt_bvh_layout.cpp; no device needed)
std::vector<ptd::DNode> to_dnodes(const std::vector<pt_bvh_node>& bvh);
bool leaf_codes_fit(const std::vector<ptd::DNode>& nodes);   // the pair / quad layouts' leaf code holds every leaf
bool make_quads(const std::vector<ptd::DNode>& nodes, std::vector<ptd::DQuad>& quads, int32_t& root_code,
                int32_t& root_occ, std::vector<int32_t>* slot_node = nullptr);
double build_qcull(const std::vector<ptd::DNode>& nodes, const std::vector<pt_triangle>& tris,
                   const std::vector<int32_t>& slot_node, std::vector<uint32_t>& qcull);

}  // namespace pt
