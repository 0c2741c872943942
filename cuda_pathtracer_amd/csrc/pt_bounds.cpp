// Scene preparation of the bounded closest hit that needs no device: the geom table
// with its widened slabs, world boxes and tight planes, the room, the order of the bounds pass and the
// first bounce's camera masks.  Double-precision arithmetic on host vectors, compiled as plain C++; the
// context (pt_kernels.hip) uploads the results, and pt_scene_room_info reads them without a device.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pt_internal.h"

using namespace ptd;

namespace pt {

namespace {

Affine to_affine(const float* m) {   // glm column-major 4x4 -> 3x4 + the exact w=0 terms
    Affine a;
    for (int col = 0; col < 4; ++col)
        for (int r = 0; r < 3; ++r) a.c[col][r] = m[4 * col + r];
    for (int r = 0; r < 3; ++r) a.z3[r] = m[12 + r] * 0.0f;
    return a;
}

// The exact inverse X of the linear part of `inv` (q = M p + t, so p = X (q - t)) by adjugate /
// determinant, in double.  Returns the determinant; X is filled when it is not zero.
double invert_linear(const Affine& inv, double X[3][3]) {
    double M[3][3];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) M[r][k] = inv.c[k][r];   // q = M p + t
    const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) -
                       M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                       M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    if (std::fabs(det) > 0.0)
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) {
                const int r1 = (k + 1) % 3, r2 = (k + 2) % 3, k1 = (r + 1) % 3, k2 = (r + 2) % 3;
                X[r][k] = (M[r1][k1] * M[r2][k2] - M[r1][k2] * M[r2][k1]) / det;   // adjugate / det
            }
    return det;
}
// Extends [lo, hi] to the world hull of an object-space box under X: its eight corners take q_k =
// qlo[k] or qhi[k] (the box's planes with inv's translation already subtracted) on each axis.
void corner_hull(const double X[3][3], const double qlo[3], const double qhi[3], double lo[3], double hi[3]) {
    for (int corner = 0; corner < 8; ++corner) {
        double q[3];
        for (int k = 0; k < 3; ++k) q[k] = (corner >> k) & 1 ? qhi[k] : qlo[k];
        for (int r = 0; r < 3; ++r) {
            const double v = X[r][0] * q[0] + X[r][1] * q[1] + X[r][2] * q[2];
            lo[r] = std::min(lo[r], v);
            hi[r] = std::max(hi[r], v);
        }
    }
}

}  // namespace

// The geom table as the device reads it, before the widened bounds (update_bounds), and the scene's
// extent.
BoundsHost make_dgeoms(const Scene& S) {
    BoundsHost B;
    std::vector<DGeom>& dg = B.geoms;
    dg.resize(S.geoms.size());
    for (size_t i = 0; i < S.geoms.size(); ++i) {
        const pt_geom& g = S.geoms[i];
        DGeom& d = dg[i];
        std::memset(&d, 0, sizeof d);
        d.type = g.type;
        d.material = g.material_id;
        d.tri_start = g.tri_start;
        d.tri_end = g.tri_end;
        d.inv = to_affine(g.inverse_transform);
        d.xf = to_affine(g.transform);
        d.itr = to_affine(g.inv_transpose);
        if (d.type == PT_GEOM_CUBE)   // DGeom::nrm: glm's multiplyMV + normalize of each unit axis, in float32
            for (int code = 0; code < 6; ++code) {
                const float sg = (code & 1) ? -1.0f : 1.0f;
                const int a = code >> 1;
                const float n[3] = {a == 0 ? sg : 0.0f, a == 1 ? sg : 0.0f, a == 2 ? sg : 0.0f};
                float v[3];
                for (int r = 0; r < 3; ++r)
                    v[r] = (d.itr.c[0][r] * n[0] + d.itr.c[1][r] * n[1]) + (d.itr.c[2][r] * n[2] + d.itr.z3[r]);
                const float inv = 1.0f / std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
                for (int r = 0; r < 3; ++r) d.nrm[code][r] = v[r] * inv;
                // DGeom::frm: the hemisphere frame of that normal (float32, the device's cross/normalize)
                const float* nn = d.nrm[code];
                float dnn[3] = {0.0f, 0.0f, 1.0f};
                if (std::fabs(nn[0]) < ptd::kSQRT_1_3) { dnn[0] = 1.0f; dnn[2] = 0.0f; }
                else if (std::fabs(nn[1]) < ptd::kSQRT_1_3) { dnn[1] = 1.0f; dnn[2] = 0.0f; }
                auto crs = [](const float* a, const float* b, float* o) {
                    o[0] = a[1] * b[2] - b[1] * a[2];
                    o[1] = a[2] * b[0] - b[2] * a[0];
                    o[2] = a[0] * b[1] - b[0] * a[1];
                };
                auto nrmz = [](float* x) {
                    const float iv = 1.0f / std::sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
                    for (int r = 0; r < 3; ++r) x[r] = x[r] * iv;
                };
                float p1[3], p2[3];
                crs(nn, dnn, p1);
                nrmz(p1);
                crs(nn, p1, p2);
                nrmz(p2);
                for (int r = 0; r < 3; ++r) { d.frm[code][r] = p1[r]; d.frm[code][3 + r] = p2[r]; }
            }
        for (int k = 0; k < 3; ++k) { d.bmin[k] = g.min_bound[k]; d.bmax[k] = g.max_bound[k]; }
    }
    {   // scene extent: every surface point (cube/sphere corners, mesh vertices) and the camera
        double ext = 0.0;
        for (int k = 0; k < 3; ++k) ext = std::max(ext, std::fabs((double)S.camera.position[k]));
        for (const pt_geom& g : S.geoms) {
            if (g.type != PT_GEOM_CUBE && g.type != PT_GEOM_SPHERE) continue;
            for (int corner = 0; corner < 8; ++corner) {
                const double p[3] = {corner & 1 ? 0.5 : -0.5, corner & 2 ? 0.5 : -0.5, corner & 4 ? 0.5 : -0.5};
                for (int r = 0; r < 3; ++r) {
                    double v = g.transform[12 + r];
                    for (int k = 0; k < 3; ++k) v += (double)g.transform[4 * k + r] * p[k];
                    ext = std::max(ext, std::fabs(v));
                }
            }
        }
        for (const pt_triangle& t : S.triangles)
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 3; ++k) ext = std::max(ext, std::fabs((double)t.v[v][k]));
        B.scene_ext = ext;
    }
    return B;
}

// The room of bound_room_tagged: at most one world-box cube (bkind 3) per face -x, +x, -y, +y, -z, +z
// and the box B between the widened planes with which those walls face each other — H_a the low plane
// of the +a wall, L_a the high plane of the -a wall, +-inf for a face without a wall.
//   Per face the candidate is the cube that lies wholly on that side of the centre of the world-box
// cubes' common box and has the largest cross-section there (a cube serves one face only).  A wall
// stays only if its extent on the other two axes covers B's, B ending on an open face where the box
// of the remaining walls ends (their unwidened boxes, which every widened wall of the same extent
// covers); a wall that does not cover its face would send the rays leaving past it through extra
// exact tests — slower, never wrong, since bound_room_tagged's bounds hold for any wall.  The room
// needs three walls (L_a < H_a follows from the selection).  Tags carry five bits, as in the pass
// itself.  PT_AMD_ROOM=0 leaves the walls in the per-cube loop (A/B and tests; the same bits).
void find_room(BoundsHost& B) {
    RoomDev& S = B.room;
    S.n = 0;
    S.wback = 0.0f;
    for (int f = 0; f < 6; ++f) {
        S.pl[f] = (f & 1) ? HUGE_VALF : -HUGE_VALF;
        S.out[f] = (f & 1) ? -HUGE_VALF : HUGE_VALF;
        S.tag[f] = 0x7f800000u;
        S.in[f] = (f & 1) ? -HUGE_VALF : HUGE_VALF;   // no origin is between these: no claim
    }
    const std::vector<DGeom>& G = B.geoms;
    const size_t n = G.size();
    if (n > (size_t)kLdsGeoms || B.unbounded) return;
    if (const char* e = std::getenv("PT_AMD_ROOM"))
        if (std::atoi(e) == 0) return;
    // the cubes' own (unwidened) world boxes
    std::vector<double> elo(3 * n, HUGE_VAL), ehi(3 * n, -HUGE_VAL);
    double alo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, ahi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (size_t i = 0; i < n; ++i) {
        if (G[i].bkind != 3) continue;
        for (int corner = 0; corner < 8; ++corner)
            for (int r = 0; r < 3; ++r) {
                double v = G[i].xf.c[3][r];
                for (int k = 0; k < 3; ++k) v += (double)G[i].xf.c[k][r] * ((corner >> k) & 1 ? 0.5 : -0.5);
                elo[3 * i + r] = std::min(elo[3 * i + r], v);
                ehi[3 * i + r] = std::max(ehi[3 * i + r], v);
            }
        for (int r = 0; r < 3; ++r) {
            alo[r] = std::min(alo[r], elo[3 * i + r]);
            ahi[r] = std::max(ahi[r], ehi[3 * i + r]);
        }
    }
    int face[6];
    std::vector<char> used(n, 0);
    for (int f = 0; f < 6; ++f) {
        const int a = f >> 1, b = (a + 1) % 3, e = (a + 2) % 3;
        const double mid = 0.5 * (alo[a] + ahi[a]);
        double area = -1.0;
        face[f] = -1;
        for (size_t i = 0; i < n; ++i) {
            if (G[i].bkind != 3 || used[i]) continue;
            if (!((f & 1) ? (double)G[i].wlo[a] > mid : (double)G[i].whi[a] < mid)) continue;
            const double ar = ((double)G[i].whi[b] - (double)G[i].wlo[b]) * ((double)G[i].whi[e] - (double)G[i].wlo[e]);
            if (ar > area) { area = ar; face[f] = (int)i; }
        }
        if (face[f] >= 0) used[(size_t)face[f]] = 1;
    }
    float pl[6];
    for (;;) {
        double blo[3], bhi[3];   // B, ended on its open faces
        int walls = 0;
        for (int a = 0; a < 3; ++a) {
            double wl = HUGE_VAL, wh = -HUGE_VAL;
            for (int f = 0; f < 6; ++f)
                if (face[f] >= 0) {
                    wl = std::min(wl, elo[3 * (size_t)face[f] + a]);
                    wh = std::max(wh, ehi[3 * (size_t)face[f] + a]);
                    walls += a == 0;
                }
            pl[2 * a] = face[2 * a] >= 0 ? G[(size_t)face[2 * a]].whi[a] : -HUGE_VALF;
            pl[2 * a + 1] = face[2 * a + 1] >= 0 ? G[(size_t)face[2 * a + 1]].wlo[a] : HUGE_VALF;
            blo[a] = face[2 * a] >= 0 ? (double)pl[2 * a] : wl;
            bhi[a] = face[2 * a + 1] >= 0 ? (double)pl[2 * a + 1] : wh;
        }
        if (walls < 3) return;
        bool dropped = false;
        for (int f = 0; f < 6; ++f) {
            if (face[f] < 0) continue;
            const DGeom& d = G[(size_t)face[f]];
            for (int k = 1; k < 3; ++k) {
                const int b = ((f >> 1) + k) % 3;
                if (!((double)d.wlo[b] <= blo[b] && (double)d.whi[b] >= bhi[b])) { face[f] = -1; dropped = true; break; }
            }
        }
        if (!dropped) break;
    }
    // (L_a < H_a needs no test: a -a wall's high plane is below the centre, a +a wall's low plane above)
    for (int f = 0; f < 6; ++f) {
        S.pl[f] = pl[f];
        if (face[f] < 0) continue;
        S.tag[f] = (uint32_t)face[f];
        S.wback = std::max(S.wback, G[(size_t)face[f]].wback);
        for (int a = 0; a < 3; ++a) {
            S.out[2 * a] = std::min(S.out[2 * a], G[(size_t)face[f]].wlo[a]);
            S.out[2 * a + 1] = std::max(S.out[2 * a + 1], G[(size_t)face[f]].whi[a]);
        }
        ++S.n;
    }
    // The tight facing planes of bound_room_tagged's departure claim: a wall's own hull plane, and for a
    // face without a wall the infinity that leaves the claim to the other face's plane alone (what is
    // claimed a miss there is the missing wall, which is no candidate anyway).  PT_AMD_ROOM_DEPART=0
    // keeps the values no origin lies between (A/B and tests; the same bits).
    bool depart = S.n > 0;
    if (const char* e = std::getenv("PT_AMD_ROOM_DEPART"))
        if (std::atoi(e) == 0) depart = false;
    for (int f = 0; f < 6 && depart; ++f)
        S.in[f] = face[f] >= 0 ? B.wtight[6 * (size_t)face[f] + 2 * (size_t)(f >> 1) + (size_t)(~f & 1)]
                                    : ((f & 1) ? HUGE_VALF : -HUGE_VALF);
}

// Widened bounds of the bounded closest-hit pass (bound_geom), sized from R = the largest
// |coordinate| any ray origin can have: a surface point (+1e-4 offsets) or the camera lens.
//   qo = inv * ro is computed with <= 4 ulp of S_a = sum_i |inv_ia| R + |inv_3a| absolute error by
// either side (exact test, bounds test), the exact slab parameters add <= 5 ulp of (S_a + 0.5):
// mu_a = 2^-18 (S_a + 1) is >= 10x that.  The sphere's b^2 - a c cancels to <= 2^-20 (S + 1)^2:
// kappa = 2^-16 (S + 1)^2.  tslack covers the back-transform (transform * inverse != I in float)
// and the rounding of the reference's length(); abs_slack its absolute part.
//   The range of the forms.  With |ro|_inf <= R and |rd| < 2 the largest finite intermediates are the
// spheres' (bound_geom<2>, <4>, bound_sphere_tagged): |qo_a| <= S_a and |qv_a| <= 2 cs_a give
// q2 <= 3 S^2, |b| <= 6 S cs and a <= 12 cs^2, so b * b and a * (q2 - r2w) stay below
// 36 S^2 cs^2 + 12 cs^2 r2w < 40 (S + 1)^2 (cs + 1)^2 each and their difference below twice that; the
// departing test's (q2 + 1) * (kcs * rinf + kc3) stays below (3 S^2 + 1) 2^-17 (S + 2) < 2^-15 (S + 2)^3;
// bkind 4 takes the dot products in world space first, dot(w, w) <= 12 R^2.  The cubes' forms multiply
// a difference of at most 2 S + 1 (object slabs) or 2 R (1 + 2^-17) (world planes) by a reciprocal of a
// direction component, which is infinite for an axis-parallel ray by design (the slab parameters then
// order as the reference's do), so their only condition is that the differences themselves, and the
// host's constants (mu, the pads, abs_slack), are finite floats.  If a sphere's b * b and a * q2 both
// overflow, disc = inf - inf is a NaN, the tagged form calls a sphere the ray hits a miss, and the
// closest hit is wrong.  bound_range is the largest of these magnitudes at a given R; the scene is
// bounded while it stays within kBoundRange = 2^126, one binade below the first float that rounds to
// infinity, and BoundsHost::r_limit is the R at which it gets there (bisected: every term grows with R).
//   Beyond r_limit the context keeps its kernels and gives every cube and sphere the one bound that
// claims nothing: bkind 3 with an infinite world box, back = wback = 0, tslack = 1, abs_slack = 0 and no
// room.  bound_wbox_tagged then returns E0 = 0, X = +inf, the tag of +0 for every ray (a finite origin
// minus an infinite plane is infinite, times a nonzero or infinite reciprocal still infinite, and never
// NaN), so pass 2 runs the exact test of every geom for every ray: the reference's loop.
constexpr double kBoundRange = 0x1p126;
static double bound_range(const BoundsHost& B, double R) {
    double m = 4.0 * (R + 1.0);
    for (const DGeom& d : B.geoms) {
        if (d.type != PT_GEOM_CUBE && d.type != PT_GEOM_SPHERE) continue;
        double smax = 0.0, cs = 0.0;
        for (int a = 0; a < 3; ++a) {
            double S = std::fabs((double)d.inv.c[3][a]), c = 0.0;
            for (int i = 0; i < 3; ++i) {
                S += std::fabs((double)d.inv.c[i][a]) * R;
                c += std::fabs((double)d.inv.c[i][a]);
            }
            smax = std::max(smax, S);
            cs = std::max(cs, c);
        }
        m = std::max(m, 4.0 * (smax + 1.0));
        if (d.type == PT_GEOM_SPHERE) {
            m = std::max(m, 80.0 * (smax + 1.0) * (smax + 1.0) * (cs + 1.0) * (cs + 1.0));
            m = std::max(m, std::ldexp((smax + 2.0) * (smax + 2.0) * (smax + 2.0), -15));
            m = std::max(m, 16.0 * (R + 1.0) * (R + 1.0));
        }
    }
    return m;   // (+inf or NaN for entries beyond double's own range: not within any limit)
}
static double bound_r_limit(const BoundsHost& B) {
    if (!(bound_range(B, 0.0) <= kBoundRange)) return 0.0;
    double lo = 0.0, hi = 0x1p127;
    for (int it = 0; it < 200; ++it) {
        const double mid = lo == 0.0 ? hi * 0x1p-8 : std::sqrt(lo * hi);
        if (mid == lo || mid == hi) break;
        if (bound_range(B, mid) <= kBoundRange) lo = mid;
        else hi = mid;
        if (lo == 0.0 && hi < 0x1p-1000) break;
    }
    return lo;
}

void update_bounds(BoundsHost& B, float aperture) {
    const double R = B.scene_ext + std::fabs((double)aperture) + 1e-2;
    B.R = R;
    B.r_limit = bound_r_limit(B);
    B.unbounded = !(R <= B.r_limit);
    B.wtight.assign(6 * B.geoms.size(), 0.0f);
    if (B.unbounded) {
        for (DGeom& d : B.geoms) {
            d.bkind = (d.type == PT_GEOM_CUBE || d.type == PT_GEOM_SPHERE) ? 3 : 0;
            for (int k = 0; k < 3; ++k) {
                d.slo[k] = d.wlo[k] = d.wbox[2 * k] = -HUGE_VALF;
                d.shi[k] = d.whi[k] = d.wbox[2 * k + 1] = HUGE_VALF;
            }
            d.r2w = HUGE_VALF;
            d.kcs = d.kc3 = 0.0f;
            d.tslack = 1.0f;
            d.back = d.wback = 0.0f;
        }
        B.abs_slack = 0.0f;
        B.wb_tslack = 1.0f;
        find_room(B);   // (no room: unbounded)
        return;
    }
    for (DGeom& d : B.geoms) {
        double smax = 0.0;
        for (int a = 0; a < 3; ++a) {
            double S = std::fabs((double)d.inv.c[3][a]);
            for (int i = 0; i < 3; ++i) S += std::fabs((double)d.inv.c[i][a]) * R;
            const double mu = std::ldexp(S + 1.0, -18);
            d.slo[a] = (float)(-0.5 - mu);
            d.shi[a] = (float)(0.5 + mu);
            smax = std::max(smax, S);
        }
        d.r2w = (float)(0.25 + std::ldexp((smax + 1.0) * (smax + 1.0), -16));
        // departing-ray test: |qo_exact - qo_bound| <= 2^-21 S_ray (S_ray <= cs |ro|_inf + c3) moves
        // |qo|^2 by <= 2^-20 |qo| S_ray; the dot products add <= 2^-21 |qo|^2.  kappa_ray is >= 6x that.
        double cs = 0.0, c3 = 0.0;
        for (int a = 0; a < 3; ++a) {
            cs = std::max(cs, std::fabs((double)d.inv.c[0][a]) + std::fabs((double)d.inv.c[1][a]) +
                                  std::fabs((double)d.inv.c[2][a]));
            c3 = std::max(c3, std::fabs((double)d.inv.c[3][a]));
        }
        d.kcs = (float)std::ldexp(cs, -18);
        d.kc3 = (float)std::ldexp(c3 + 2.0, -18);
        d.bkind = d.type == PT_GEOM_CUBE ? 1 : (d.type == PT_GEOM_SPHERE ? 2 : 0);
        if (d.type == PT_GEOM_SPHERE) {
            // uniform scale (x rotation): G = L^T L = sigma^2 I up to delta, L = the linear part of inv
            double G[3][3], tr = 0.0, dev = 0.0;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    G[i][j] = 0.0;
                    for (int a = 0; a < 3; ++a) G[i][j] += (double)d.inv.c[i][a] * (double)d.inv.c[j][a];
                }
            for (int i = 0; i < 3; ++i) tr += G[i][i];
            const double s2 = tr / 3.0;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) dev = std::max(dev, std::fabs(G[i][j] - (i == j ? s2 : 0.0)));
            if (s2 > 0.0 && dev <= std::ldexp(s2, -20)) {
                // the world-space dot products differ from the object-space ones by the
                // non-uniformity (<= 2^-20 relative) and the rounding of w = ro - centre (within the
                // 4 ulp of S_a assumed above): margins doubled
                for (int k = 0; k < 3; ++k) d.wlo[k] = d.xf.c[3][k];
                d.whi[0] = (float)s2;
                // bound_sphere_tagged's per-geom constants: 1 / is2 and the pull-back factor
                // 1.0002e-4 / sqrt(is2), rounded up (is2 as the device reads it, a float)
                d.whi[1] = (float)(1.0 / (double)d.whi[0]);
                d.back = std::nextafter((float)(1.0002e-4 / std::sqrt((double)d.whi[0])), HUGE_VALF);
                d.r2w = (float)(0.25 + std::ldexp((smax + 1.0) * (smax + 1.0), -15));
                d.kcs *= 2.0f;
                d.kc3 *= 2.0f;
                d.bkind = 4;
            }
        }
        if (d.type == PT_GEOM_CUBE) {   // world box of the widened cube, if the transform is axis-aligned
            double X[3][3];
            const double det = invert_linear(d.inv, X);
            bool aligned = std::fabs(det) > 0.0;
            if (aligned) {
                for (int r = 0; r < 3 && aligned; ++r) {
                    double big = 0.0;
                    for (int k = 0; k < 3; ++k) big = std::max(big, std::fabs(X[r][k]));
                    int n = 0;
                    // (1e-4 of the row's axis: a 90-degree rotation in float has cos = -4.4e-8, which next
                    // to a 0.01 : 10 scale — the Cornell ceiling and back wall — is 4.4e-5 of the thin axis;
                    // the world box grows by that share of the slab.  Only tightness depends on this bound:
                    // the world box below holds the widened cube at any rotation, and `back` takes the
                    // transform's norm.)
                    for (int k = 0; k < 3; ++k) n += std::fabs(X[r][k]) > 1e-4 * big;
                    aligned = n == 1;
                }
            }
            if (aligned) {
                double stretch = 0.0, lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
                double qlo[3], qhi[3];   // (float differences, as the corners were always taken)
                for (int k = 0; k < 3; ++k) {
                    qlo[k] = d.slo[k] - d.inv.c[3][k];
                    qhi[k] = d.shi[k] - d.inv.c[3][k];
                }
                corner_hull(X, qlo, qhi, lo, hi);
                // the largest stretch ||X||_2 <= sqrt(||X||_1 ||X||_inf): the largest entry when X has one
                // entry per row, and still a bound with the small others the test above lets through
                double n1 = 0.0, ninf = 0.0;
                for (int r = 0; r < 3; ++r) {
                    ninf = std::max(ninf, std::fabs(X[r][0]) + std::fabs(X[r][1]) + std::fabs(X[r][2]));
                    n1 = std::max(n1, std::fabs(X[0][r]) + std::fabs(X[1][r]) + std::fabs(X[2][r]));
                    for (int k = 0; k < 3; ++k) stretch = std::max(stretch, std::fabs(X[r][k]));
                }
                stretch = std::max(stretch, std::sqrt(n1 * ninf));
                const double pad = std::ldexp(R + 1.0, -18);
                for (int r = 0; r < 3; ++r) {
                    d.wlo[r] = (float)(lo[r] - pad - std::ldexp(std::fabs(lo[r]), -18));
                    d.whi[r] = (float)(hi[r] + pad + std::ldexp(std::fabs(hi[r]), -18));
                    // the hull itself, for the departure claim of bound_room_tagged: moved out by 2^-40 (R + 1)
                    // (the rounding of X and of the sums above is a few 2^-53 of the coordinates, also where
                    // the plane itself cancels to nearly 0), then one float further out than the nearest one
                    const double eps = std::ldexp(R + 1.0, -40);
                    float* tg = &B.wtight[6 * (size_t)(&d - B.geoms.data()) + 2 * (size_t)r];
                    tg[0] = std::nextafter((float)(lo[r] - eps), -HUGE_VALF);
                    tg[1] = std::nextafter((float)(hi[r] + eps), HUGE_VALF);
                }
                d.back = (float)(1.0002e-4 * stretch * (1.0 + 1e-5));
                for (int r = 0; r < 3; ++r) {
                    d.wbox[2 * r] = d.wlo[r];
                    d.wbox[2 * r + 1] = d.whi[r];
                }
                d.bkind = 3;
            } else {
                // oriented cube (bkind 1): bound_obox_tagged's pull-back factor, 1.0002e-4 / sigma_min(L)
                // bounded by the Frobenius norm of X = L^-1 (a singular L: +inf, the bound is then 0)
                double fro = HUGE_VAL;
                if (std::fabs(det) > 0.0) {   // (X is computed above exactly then)
                    fro = 0.0;
                    for (int r = 0; r < 3; ++r)
                        for (int k = 0; k < 3; ++k) fro += X[r][k] * X[r][k];
                }
                d.back = std::isfinite(fro) ? std::nextafter((float)(1.0002e-4 * std::sqrt(fro) * (1.0 + 1e-5)), HUGE_VALF)
                                            : HUGE_VALF;
            }
        }
        double dev = 0.0;   // Frobenius norm of xf_lin * inv_lin - I
        for (int r = 0; r < 3; ++r)
            for (int col = 0; col < 3; ++col) {
                double m = 0.0;
                for (int k = 0; k < 3; ++k) m += (double)d.xf.c[k][r] * (double)d.inv.c[col][k];
                m -= r == col ? 1.0 : 0.0;
                dev += m * m;
            }
        d.tslack = (float)(1.0 - 4.0 * std::sqrt(dev) - std::ldexp(1.0, -14));
    }
    B.abs_slack = (float)std::ldexp(R + 1.0, -17);
    // bound_wbox_tagged: one tslack for every world-box cube (their smallest), folded into the pull-back
    float ts = 1.0f;
    for (const DGeom& d : B.geoms)
        if (d.bkind == 3) ts = std::min(ts, d.tslack);
    B.wb_tslack = ts;
    for (DGeom& d : B.geoms)
        d.wback = d.bkind == 3 ? std::nextafter((float)((double)d.back * (double)ts), HUGE_VALF) : 0.0f;
    find_room(B);
}

// SceneDev::bgeoms: the geom table stably ordered by bkind, each row keeping its index in `orig`;
// among the world-box cubes the walls of the room come first (RoomDev::n of them).  bk[k] .. bk[k + 1]
// are the rows of bkind k; a geom of an unknown kind is left out (b.size() < the table's).
void bound_order(const BoundsHost& B, std::vector<DGeom>& b, int32_t bk[6]) {
    b.clear();
    for (int k = 0; k < 6; ++k) bk[k] = 0;
    const RoomDev& S = B.room;
    auto wall = [&](size_t i) {   // a wall of the room (find_room)
        for (int f = 0; f < 6; ++f)
            if (S.n > 0 && S.tag[f] == (uint32_t)i) return true;
        return false;
    };
    for (int k = 0; k < 5; ++k) {
        bk[k] = (int32_t)b.size();
        if (k == 3)   // the room's walls first among the world-box cubes
            for (size_t i = 0; i < B.geoms.size(); ++i)
                if (wall(i)) {
                    b.push_back(B.geoms[i]);
                    b.back().orig = (int32_t)i;
                }
        for (size_t i = 0; i < B.geoms.size(); ++i)
            if (B.geoms[i].bkind == k && !(k == 3 && wall(i))) {
                b.push_back(B.geoms[i]);
                b.back().orig = (int32_t)i;
            }
    }
    bk[5] = (int32_t)b.size();
}

// ---- first-bounce geom masks ----------------------------------------------------------------
// A wave of the first bounce traces 64 consecutive tile pixels of one iteration.  Every camera
// ray of those pixels (any SSAA jitter in [0, 1) pixel, any lens sample within the aperture) is
//   o + s (F - o), s >= 0,   o in cam.pos + [-a, a]^2 x {0},   F in the focal-plane image of the
// pixels' rectangle (DoF; raygen's focus point, pathtrace.cu:203-224), or
//   cam.pos + s v,           v in the span of the rectangle's view vectors (no DoF).
// Bounding o and F - o (or v) by boxes and asking, axis by axis, for a common s >= 0 at which the
// ray box meets a geom's world box gives a conservative "can hit" test (never false for a ray that
// hits).  The geom's box is its test region [slo, shi]^3 (already wider than the exact test's
// rounding, update_bounds) mapped by the exact inverse of `inv`, padded again.  A geom outside the
// mask is skipped by the bounds pass of those rays: the closest hit is unchanged (intersect_bounded).
static bool beam_meets_box(const double olo[3], const double ohi[3], const double dlo[3], const double dhi[3],
                           const double blo[3], const double bhi[3]) {
    double smin = 0.0, smax = HUGE_VAL;
    for (int k = 0; k < 3; ++k) {
        // o_lo + s d_lo <= b_hi  and  o_hi + s d_hi >= b_lo  (the ray box's extent along axis k at s)
        const double c1 = bhi[k] - olo[k], c2 = blo[k] - ohi[k];
        if (dlo[k] > 0.0) smax = std::min(smax, c1 / dlo[k]);
        else if (dlo[k] < 0.0) smin = std::max(smin, c1 / dlo[k]);
        else if (c1 < 0.0) return false;
        if (dhi[k] > 0.0) smin = std::max(smin, c2 / dhi[k]);
        else if (dhi[k] < 0.0) smax = std::min(smax, c2 / dhi[k]);
        else if (c2 > 0.0) return false;
    }
    return smin <= smax * (1.0 + 1e-9) + 1e-12;
}

// The mask of every block of 64 tile pixels (bit g: geom g).  A table of more than kLdsGeoms geoms has
// no bit per geom: every mask is then "all" (the context builds no masks for such a scene).
void camera_masks(const BoundsHost& B, const CamDev& cam, const FlagsDev& fl, const TileDev& T,
                  std::vector<uint32_t>& mask) {
    const int ng = (int)B.geoms.size();
    const size_t nblk = ((size_t)T.npix + 63) / 64;
    if (ng > kLdsGeoms) {
        mask.assign(nblk, ~0u);
        return;
    }
    // world boxes of the geoms' test regions
    std::vector<std::array<double, 6>> gb((size_t)ng);
    std::vector<bool> always((size_t)ng, false);
    for (int g = 0; g < ng; ++g) {
        const DGeom& d = B.geoms[(size_t)g];
        if ((d.type != PT_GEOM_CUBE && d.type != PT_GEOM_SPHERE) || B.unbounded) { always[(size_t)g] = true; continue; }
        double X[3][3];
        const double det = invert_linear(d.inv, X);
        if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) { always[(size_t)g] = true; continue; }
        const double rs = d.type == PT_GEOM_SPHERE ? std::sqrt(std::max(0.0, (double)d.r2w)) : 0.0;
        double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
        double qlo[3], qhi[3];
        for (int k = 0; k < 3; ++k) {
            const double a = std::min((double)d.slo[k], -rs), b = std::max((double)d.shi[k], rs);
            qlo[k] = a * (1.0 + 1e-4) - d.inv.c[3][k];
            qhi[k] = b * (1.0 + 1e-4) - d.inv.c[3][k];
        }
        corner_hull(X, qlo, qhi, lo, hi);
        for (int r = 0; r < 3; ++r) {
            const double pad = 1e-3 + 1e-5 * std::max(std::fabs(lo[r]), std::fabs(hi[r]));
            gb[(size_t)g][r] = lo[r] - pad;
            gb[(size_t)g][3 + r] = hi[r] + pad;
        }
        if (!std::isfinite(gb[(size_t)g][0] + gb[(size_t)g][1] + gb[(size_t)g][2] + gb[(size_t)g][3] +
                           gb[(size_t)g][4] + gb[(size_t)g][5]))
            always[(size_t)g] = true;
    }
    const double pos[3] = {cam.pos[0], cam.pos[1], cam.pos[2]};
    const double jit = fl.ssaa ? 1.0 : 0.0, eps = 0.01;   // pixel units
    const bool dof = fl.dof != 0;
    const double ap = std::fabs((double)fl.aperture), focal = fl.focal;
    // rays of tile row `row`, tile columns [x0, x1]: their geoms
    auto row_mask = [&](int row, int x0, int x1) -> uint32_t {
        const int y = row * T.world + T.rank;
        const double ax0 = x0 - cam.res[0] * 0.5 - eps, ax1 = x1 - cam.res[0] * 0.5 + jit + eps;
        const double ay0 = y - cam.res[1] * 0.5 - eps, ay1 = y - cam.res[1] * 0.5 + jit + eps;
        double v[4][3];
        for (int q = 0; q < 4; ++q) {
            const double ax = q & 1 ? ax1 : ax0, ay = q & 2 ? ay1 : ay0;
            for (int k = 0; k < 3; ++k)
                v[q][k] = (double)cam.view[k] - (double)cam.right[k] * cam.pl[0] * ax - (double)cam.up[k] * cam.pl[1] * ay;
        }
        double olo[3], ohi[3], dlo[3], dhi[3];
        if (!dof) {
            for (int k = 0; k < 3; ++k) {
                olo[k] = pos[k] - 1e-4 * (1.0 + std::fabs(pos[k]));
                ohi[k] = pos[k] + 1e-4 * (1.0 + std::fabs(pos[k]));
                dlo[k] = std::min({v[0][k], v[1][k], v[2][k], v[3][k]});
                dhi[k] = std::max({v[0][k], v[1][k], v[2][k], v[3][k]});
                const double m = 1e-5 * (std::fabs(dlo[k]) + std::fabs(dhi[k]) + 1e-3);
                dlo[k] -= m;
                dhi[k] += m;
            }
        } else {
            double flo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, fhi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
            int sign = 0;
            for (int q = 0; q < 4; ++q) {
                const double n = std::sqrt(v[q][0] * v[q][0] + v[q][1] * v[q][1] + v[q][2] * v[q][2]);
                const int sg = v[q][2] > 0.0 ? 1 : -1;
                if (!(std::fabs(v[q][2]) > 1e-3 * n) || (sign != 0 && sg != sign)) return ~0u;   // focus plane unbounded
                sign = sg;
                for (int k = 0; k < 3; ++k) {
                    const double f = pos[k] + focal * v[q][k] / std::fabs(v[q][2]);
                    flo[k] = std::min(flo[k], f);
                    fhi[k] = std::max(fhi[k], f);
                }
            }
            for (int k = 0; k < 3; ++k) {
                const double fp = 1e-4 * (1.0 + std::fabs(flo[k]) + std::fabs(fhi[k]));
                const double a = k < 2 ? ap * (1.0 + 1e-4) + 1e-6 : 1e-6;
                olo[k] = pos[k] - a - 1e-4 * (1.0 + std::fabs(pos[k]));
                ohi[k] = pos[k] + a + 1e-4 * (1.0 + std::fabs(pos[k]));
                dlo[k] = (flo[k] - fp) - ohi[k];
                dhi[k] = (fhi[k] + fp) - olo[k];
            }
        }
        uint32_t m = 0u;
        for (int g = 0; g < ng; ++g)
            if (always[(size_t)g] || beam_meets_box(olo, ohi, dlo, dhi, &gb[(size_t)g][0], &gb[(size_t)g][3]))
                m |= 1u << g;
        return m;
    };
    mask.assign(nblk, 0u);
    for (size_t b = 0; b < nblk; ++b) {
        const int lp0 = (int)(b * 64), lp1 = std::min(T.npix - 1, lp0 + 63);
        const int r0 = lp0 / T.W, r1 = lp1 / T.W;
        uint32_t m = 0u;
        for (int r = r0; r <= r1; ++r)
            m |= row_mask(r, r == r0 ? lp0 - r * T.W : 0, r == r1 ? lp1 - r * T.W : T.W - 1);
        mask[b] = m;
    }
}

// What pt_ctx_room_info and pt_scene_room_info report of a room.
void room_info(const RoomDev& S, int32_t* walls, int32_t* faces, float* lo, float* hi) {
    if (walls) *walls = S.n;
    for (int f = 0; f < 6 && faces; ++f) faces[f] = S.n > 0 && S.tag[f] < 32u ? (int32_t)S.tag[f] : -1;
    for (int a = 0; a < 3; ++a) {
        if (lo) lo[a] = S.pl[2 * a];
        if (hi) hi[a] = S.pl[2 * a + 1];
    }
}

}  // namespace pt

extern "C" int pt_scene_room_info(const pt_scene* scene, const pt_flags* flags, int32_t* walls, int32_t* faces,
                                  float* lo, float* hi) {
    if (!scene) return pt::fail(PT_ERR_ARG, "null argument");
    const auto& S = *reinterpret_cast<const pt::Scene*>(scene);
    if (!S.finalized) return pt::fail(PT_ERR_ARG, "scene not finalized (pt_scene_finalize)");
    pt_flags f;
    if (flags) f = *flags;
    else pt_flags_default(&f);
    pt::BoundsHost B = pt::make_dgeoms(S);
    pt::update_bounds(B, f.aperture);
    pt::room_info(B.room, walls, faces, lo, hi);
    return PT_OK;
}

extern "C" int pt_scene_bound_info(const pt_scene* scene, const pt_flags* flags, pt_bound_info* rows, int32_t cap,
                                   double* R, double* r_limit, int32_t* bounded, float* abs_slack, float* wb_tslack) {
    if (!scene || (cap > 0 && !rows)) return pt::fail(PT_ERR_ARG, "null argument");
    const auto& S = *reinterpret_cast<const pt::Scene*>(scene);
    if (!S.finalized) return pt::fail(PT_ERR_ARG, "scene not finalized (pt_scene_finalize)");
    pt_flags f;
    if (flags) f = *flags;
    else pt_flags_default(&f);
    pt::BoundsHost B = pt::make_dgeoms(S);
    pt::update_bounds(B, f.aperture);
    for (size_t i = 0; i < B.geoms.size() && (int64_t)i < (int64_t)cap; ++i) {
        const ptd::DGeom& d = B.geoms[i];
        pt_bound_info& o = rows[i];
        o.bkind = d.bkind;
        for (int k = 0; k < 3; ++k) {
            o.slo[k] = d.slo[k];
            o.shi[k] = d.shi[k];
            o.wlo[k] = d.wlo[k];
            o.whi[k] = d.whi[k];
        }
        for (int k = 0; k < 6; ++k) o.tight[k] = B.wtight[6 * i + (size_t)k];
        o.tslack = d.tslack;
        o.back = d.back;
        o.wback = d.wback;
    }
    if (R) *R = B.R;
    if (r_limit) *r_limit = B.r_limit;
    if (bounded) *bounded = (!B.unbounded && B.geoms.size() <= (size_t)ptd::kLdsGeoms) ? 1 : 0;
    if (abs_slack) *abs_slack = B.abs_slack;
    if (wb_tslack) *wb_tslack = B.wb_tslack;
    return PT_OK;
}
