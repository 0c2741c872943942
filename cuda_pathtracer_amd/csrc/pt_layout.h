// Scene-table and kernel-argument layouts of the MI355X path tracer, and the few constants the
// host's scene preparation shares with the device code.  Plain C++ (clang vector types, no HIP
// header, no __device__ function): included by the device code through pt_device.h and by the
// host-only units (pt_bounds.cpp, pt_bvh_layout.cpp) through pt_internal.h.
#pragma once
#include <stdint.h>

namespace ptd {

constexpr float kPI = 3.1415926535897932384626422832795028841971f;       // utilities.h:12
constexpr float kTWO_PI = 6.2831853071795864769252867665590057683943f;   // utilities.h:13
constexpr float kSQRT_1_3 = 0.5773502691896257645091487805019574556476f; // utilities.h:14
constexpr float kFLT_MAX = 3.402823466e+38f;
constexpr float kFLT_EPS = 1.192092896e-07f;

// 1 / sqrt(x) of a float x in [1 - 2^-12, 1 + 2^-12], rounded as sqrt and then as 1 / s (glm's normalize),
// from x's bit pattern u alone: the derivation is in pt_device.h (renorm_unit_core), the exhaustive check
// of all 6,145 values in tests/test_renorm_unit_cpu.py (through pt_renorm.cpp) and, on the device,
// tests/test_renorm_unit_gpu.py.  constexpr: the kernels and the host compile the same lines.
constexpr uint32_t kUnitBits = 0x3f800000u, kUnitBelow = 4096u, kUnitSpan = 6144u;   // 4096 floats below 1, 2048 above
constexpr bool unit_ok_bits(uint32_t u) { return u - (kUnitBits - kUnitBelow) <= kUnitSpan; }
constexpr uint32_t unit_rnorm_bits(uint32_t u) {   // meaningful when unit_ok_bits(u)
    const uint32_t k = u - kUnitBits;   // x's signed distance from 1.0f in ulps, two's complement
    return (int32_t)k < 0 ? kUnitBits + ((3u - k) >> 2) : kUnitBits - (k & ~1u);
}

// Affine 3x4 in glm column order + the exact glm w-term constants.
//   point  (w=1): (c0 x + c1 y) + (c2 z + c3)
//   vector (w=0): (c0 x + c1 y) + (c2 z + z3),  z3 = c3 * 0.0f (a signed zero)
struct Affine {
    float c[4][3];
    float z3[3];
};

// Geoms the bounded closest hit keeps in LDS (LGeom rows, pt_kernels.hip); its tags carry a geom index
// in five bits, so larger scenes take the plain per-geom loop and have no room (find_room).
constexpr int kLdsGeoms = 32;

// Device copy of a Geom: what intersection needs, nothing else (544 bytes, scalar-loaded).
struct DGeom {
    int32_t type, material, tri_start, tri_end;
    Affine inv;      // inverseTransform
    Affine xf;       // transform
    Affine itr;      // invTranspose
    float bmin[3], bmax[3];
    // Conservative bounds test (pt_kernels.hip bound_geom), filled by pt_create: the unit cube's
    // slabs widened to [slo, shi] = [-0.5 - mu_a, 0.5 + mu_a], the sphere's radius^2 widened to
    // r2w = 0.25 + kappa (mu, kappa exceed the rounding of both the exact test and the bounds
    // test for every ray origin in the scene), and tslack < 1, the relative slack that turns a
    // lower bound on the hit parameter into one on the reference's world distance.
    //   A sphere ray whose origin is outside the exact sphere by more than
    // kappa_ray = (|qo|^2 + 1) (kcs |ro|_inf + kc3) and moves away from its centre surely misses
    // (the ray leaving the sphere it just hit; the widened radius alone cannot tell).
    //   Axis-aligned cubes (bkind 3: the Cornell walls, incl. 90-degree rotations) are bounded by
    // their widened WORLD box [wlo, whi] (of the exact inverse of `inv`): a 6-plane slab test on the
    // world ray, with `back` >= 1e-4 * (largest stretch of the transform) for pointOnRay's pull-back.
    float slo[3], shi[3];
    float r2w, tslack;
    float kcs, kc3;
    float wlo[3], whi[3], back;
    int32_t bkind;   // 0: never hit (mesh), 1: oriented cube, 2: sphere, 3: world-box cube,
                     // 4: uniformly scaled sphere (world-space dot products)
    int32_t orig;    // SceneDev::bgeoms rows: index of this geom in SceneDev::geoms
    // Cubes: the world normal of each slab code (axis * 2 + sign) — boxIntersectionTest's
    // normalize(multiplyMV(invTranspose, (n, 0))) of a unit axis vector depends on the geom and
    // the code only, so pt_create evaluates it once with the same float32 operations (glm's
    // association, correctly rounded sqrt and division: the same bits as the per-hit evaluation).
    float nrm[6][3];
    // Cubes: the tangent frame calculateRandomDirectionInHemisphere builds from each of those
    // normals (interactions.cu:23-33: p1 = normalize(cross(n, dnn)), p2 = normalize(cross(n, p1))),
    // also a function of (geom, code) only: frm[code] = (p1, p2), evaluated once by pt_create.
    float frm[6][6];
    // bkind 3: the widened world box with each axis's two planes side by side, (wlo[k], whi[k]) at
    // wbox[2k], so one packed f32 operation (v_pk_add_f32 / v_pk_mul_f32, IEEE per component) takes
    // both planes of an axis from one SGPR pair (pt_kernels.hip bound_wbox_tagged)
    float wbox[6];
    float wback;   // bkind 3: back * SceneDev::wb_tslack rounded up (bound_wbox_tagged)
    float pad_;
};
static_assert(sizeof(Affine) == 60 && sizeof(DGeom) == 544, "geom table row");

struct DMaterial {   // == pt_material
    float color[3];
    float spec_exponent;
    float spec_color[3];
    float has_reflective, has_refractive, ior, emittance;
    int32_t texture_id;
};
static_assert(sizeof(DMaterial) == 48, "material layout");

struct DTexture {
    int32_t width, height, components, pad;
    const uint8_t* data;
};

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

// Triangle hot data, 48 bytes = three 16-byte loads: (v0, id bits), (e1, 0), (e2, 0).  The edges
// e1 = v1 - v0, e2 = v2 - v0 are computed on the host with the same single subtraction glm
// performs, so the per-test arithmetic is unchanged.
struct alignas(16) DTri {
    v4f a, b, c;
};
struct DTriAttr {    // read once for the closest hit
    float n[3][3];
    float uv[3][2];
};
// BVH node, 32 bytes = two 16-byte loads: lo = (bmin, meta), hi = (bmax, link)
//   leaf:     meta = sub_areas (> 0),  link = first triangle
//   interior: meta = -(axis + 1),      link = right child (the left child is this node + 1)
struct alignas(16) DNode {
    v4f lo, hi;
};
static_assert(sizeof(DNode) == 32 && sizeof(DTri) == 48, "packed device layouts");

// Child-pair layout of the same tree: one 64-byte entry per INTERIOR node holding both children's
// boxes and codes, so deciding where to go from a node costs one fetch instead of one per child.
//   code >= 0: interior child, entry index * 4 + its split axis;
//   code <  0: leaf child, -(first triangle * 256 + triangle count) - 1.
// The boxes tested, their outcomes (aabb_hit) and the near-first order are those of bvh_walk:
// a child is tested at its parent instead of after being popped, and only passing children are
// pushed, so the triangles tested, their order and the result are the same; used without the
// bvh_cull extension and when the tree is shallow enough for the LDS stack (no overflow case).
struct alignas(16) DPair {
    v4f lmin, lmax, rmin, rmax;   // .w: left code (lmin.w), unused (lmax.w), right code (rmin.w), unused
};
static_assert(sizeof(DPair) == 64, "pair entry");

// 4-wide layout (k_traverse4): the pair entry of interior node N with each interior child X
// replaced by X's own two children when both boxes lie inside X's box (checked on the host, so a
// grandchild box that the ray hits implies a hit on X's box — the slab test is monotone in the box
// bounds for a finite ray: (b - o) * inv is nondecreasing in b for inv > 0 and nonincreasing for
// inv < 0, so X's slab intervals contain the grandchild's).  The leaves reached, and in the
// near-first order below the triangles tested, are BVHIntersectionTest's (intersections.cu:170-224).
//   Slots 0-1: N's left child's group (X's two children, or the child itself in slot 0), slots 2-3
// the right child's.  meta bits: valid slots (0-3) | N's axis << 4 | left group's axis << 6 |
// right group's axis << 8 (3: a one-slot group, never swapped).  Codes as DPair's, with interior
// codes = quad index.  Boxes are SoA (one v4f per bound and axis) so the four slab tests run two
// slots per packed f32 instruction.
// An interior code carries its quad's meta bits above the index (kQuadMetaShift), so a walk learns
// the order of a quad's slots from the code that led to it and loads 112 of the entry's 128 bytes.
struct alignas(16) DQuad {
    v4f lox, hix, loy, hiy, loz, hiz;
    v4f code;   // int bits
    v4f meta;   // [0]: int bits (above; also in the interior codes that point here)
};
constexpr int kQuadMetaShift = 21;                        // interior code = quad index | meta << 21
constexpr int kQuadIdxMask = (1 << kQuadMetaShift) - 1;   // (a layout of more quads is not built)
static_assert(sizeof(DQuad) == 128, "quad entry");

// The room (find_room, bound_room_tagged): up to six world-box cubes, one per face of the box B they
// enclose, bounded as one group by the later bounces.  They are bgeoms[bk[3] .. bk[3] + n).
struct RoomDev {
    int32_t n;        // walls of the room (0: no room, nothing below is read)
    float pl[6];      // B, an axis's two planes side by side: (L_a, H_a) at [2a] (-inf / +inf: no wall)
    float out[6];     // the box of the walls' widened world boxes, (lowest wlo_a, highest whi_a) at [2a]
    uint32_t tag[6];  // face 2a (-a), 2a + 1 (+a): the wall's geom index, or +inf's bits (a miss) without one
    float wback;      // the largest DGeom::wback of the walls
    float in[6];      // the walls' tight facing planes (Lin_a, Hin_a) at [2a]: the hull of the widened cube
                      // without the pad, rounded outward (+inf / -inf: no wall, or PT_AMD_ROOM_DEPART=0)
};
static_assert(sizeof(RoomDev) == 104 && alignof(RoomDev) == 4, "SceneDev::room keeps the six members' bytes");

struct CamDev {
    float pos[3], view[3], up[3], right[3], pl[2];
    int32_t res[2];
};
struct FlagsDev {
    int32_t rr, bvh, bbox, ssaa, dof;
    float aperture, focal;
    int32_t single_albedo;
    int32_t bvh_cull;
    int32_t claimed;   // tile schedule (lookback.h TileSeq)
    int32_t rng_pixel; // shading RNG keyed by global pixel (pt_flags.rng_key_pixel)
    int32_t verify;    // PT_AMD_VERIFY_BOUNDS=1: re-run the plain closest-hit loop, count differences
};
struct TileDev {
    int32_t W, rank, world, npix, spp, P, depth, iter_first;
    uint64_t wdiv;   // ceil(2^40 / W) when npix * W < 2^40 (then lp / W == lp * wdiv >> 40), else 0
};
static_assert(sizeof(CamDev) == 64 && sizeof(FlagsDev) == 48 && sizeof(TileDev) == 40, "kernel-argument blocks");

// The environment: an octahedral radiance map, y up, of n x n RGBA32F texels inside a
// one-texel gutter, so (n + 2)^2 float4 in all, row-major with row stride n + 2; interior texel (i, j)
// (column along x, row along z) sits at (j + 1) * (n + 2) + (i + 1).  The gutter holds the texels bilinear
// interpolation meets across the fold (pt_env.cpp fill_gutter), so the lookup (pt_env_dev.h) has no edge
// case.  rot is the row-major world-to-map rotation; map == null: no environment.
struct EnvDev {
    const v4f* map;
    int32_t n;
    float scale;
    float rot[9];
    int32_t pad_;
};
static_assert(sizeof(EnvDev) == 56 && alignof(EnvDev) == 8, "kernel-argument block of the environment");

}  // namespace ptd
