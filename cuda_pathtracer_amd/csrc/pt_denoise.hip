// Edge-avoiding a-trous wavelet denoiser (Dammertz et al. 2010) over the first-hit G-buffer
// (pt_gbuffer), gfx950.  The exact definition of the filter is DESIGN.md §10; tests/denoise_ref.py
// restates it in numpy float32 and the GPU tests compare bit for bit.  Compiled with
// -ffp-contract=off: every operation below is one correctly rounded fp32 operation, in the stated
// order; '/' is div_cr (correctly rounded).  The edge-stopping function is 1 / (1 + x), not exp(-x):
// expf on the device and exp on a host differ in the last bits.
//
// Kernel shape: k_dn_prologue packs rgb / samples (demodulated) into a float4 plane; one k_dn_level
// launch per level ping-pongs two planes, the last one fusing the remodulation and the float3 store.
// A workgroup is a 32 x 8 pixel tile.  Steps 1 and 2 stage the tile plus its halo ((32 + 4s) x (8 + 4s)
// cells of three 16-byte values, 30 KiB at s = 2) in LDS, since neighbouring pixels share most taps;
// from step 4 on the 25 taps of a pixel are shared with no other pixel of the tile, so they are read
// through L2 directly.  Both paths run the same tap arithmetic in the same order (dn_tap), so the
// bits do not depend on the path.  No inter-workgroup waits, no atomics.
//
// The variance-guided variant (k_dnv_*; tests/denoise_var_ref.py) and the per-pixel
// luminance moments that feed it (pt_moments, k_mom_*) follow below under the same contract.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "pt_device.h"
#include "pt_internal.h"
#include "pt_moments_dev.h"

using namespace ptd;

namespace {

constexpr int kTX = 32, kTY = 8, kThreads = kTX * kTY;
constexpr int kLdsStep = 2;                       // largest step staged in LDS
constexpr int kHX = kTX + 4 * kLdsStep, kHY = kTY + 4 * kLdsStep;
constexpr int kMaxLevels = 8;
constexpr int64_t kMaxPixels = (int64_t)1 << 30;

struct DnArgs {
    const v4f* __restrict__ in;     // colour plane of the previous level
    const v4f* __restrict__ gA;     // (n, mat bits)
    const v4f* __restrict__ gB;     // (P, t)
    const v4f* __restrict__ alb;    // LAST: remodulation
    v4f* __restrict__ out;          // !LAST: colour plane
    float* __restrict__ out_rgb;    // LAST: W * H float3
    int32_t W, H, s, demodulate;
    float inv_ci, inv_n, inv_p;
};

__device__ __forceinline__ f3 xyz(v4f v) { return F3(v[0], v[1], v[2]); }

// One tap q of pixel p: adds w * c_q into sum and w into wsum.
__device__ __forceinline__ void dn_tap(float k, f3 cp, f3 np, f3 pp, f3 cq, f3 nq, f3 pq, float inv_ci, float inv_n,
                                       float inv_p, f3& sum, float& wsum) {
    const f3 d = cq - cp;
    const float xc = dot(d, d) * inv_ci;
    const float xn = gmax(0.0f, 1.0f - dot(np, nq)) * inv_n;
    const float e = dot(np, pq - pp);
    const float xp = (e * e) * inv_p;
    const float w = div_cr(k, ((1.0f + xc) * (1.0f + xn)) * (1.0f + xp));
    sum = sum + w * cq;
    wsum = wsum + w;
}

__global__ __launch_bounds__(256) void k_dn_prologue(const float* __restrict__ rgb, const v4f* __restrict__ alb,
                                                      v4f* __restrict__ out, int64_t npix, float samples, int demodulate) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        f3 c = F3(div_cr(rgb[3 * i], samples), div_cr(rgb[3 * i + 1], samples), div_cr(rgb[3 * i + 2], samples));
        if (demodulate) c = dn_modulate(c, alb[i], true);
        out[i] = v4f{c.x, c.y, c.z, 0.0f};
    }
}

// levels == 0: the epilogue alone
__global__ __launch_bounds__(256) void k_dn_epilogue(const v4f* __restrict__ in, const v4f* __restrict__ alb,
                                                      float* __restrict__ out_rgb, int64_t npix, int demodulate) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        f3 c = xyz(in[i]);
        if (demodulate) c = dn_modulate(c, alb[i], false);
        out_rgb[3 * i] = c.x;
        out_rgb[3 * i + 1] = c.y;
        out_rgb[3 * i + 2] = c.z;
    }
}

template <bool LDS, bool LAST>
__global__ __launch_bounds__(kThreads) void k_dn_level(const DnArgs A) {
    __shared__ v4f s_c[LDS ? kHX * kHY : 1], s_a[LDS ? kHX * kHY : 1], s_b[LDS ? kHX * kHY : 1];
    const int W = A.W, H = A.H, s = A.s;
    const int x0 = (int)blockIdx.x * kTX, y0 = (int)blockIdx.y * kTY;
    const int tx = (int)threadIdx.x % kTX, ty = (int)threadIdx.x / kTX;
    const int x = x0 + tx, y = y0 + ty;
    const int hx_n = kTX + 4 * s;   // LDS: the staged footprint (s <= kLdsStep)
    if (LDS) {
        const int hy_n = kTY + 4 * s;
        for (int i = (int)threadIdx.x; i < hx_n * hy_n; i += kThreads) {
            const int hy = i / hx_n, hx = i - hy * hx_n;
            const int gx = x0 - 2 * s + hx, gy = y0 - 2 * s + hy;
            v4f c = {0.f, 0.f, 0.f, 0.f}, a = {0.f, 0.f, 0.f, __int_as_float(-1)}, b = {0.f, 0.f, 0.f, 0.f};
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {   // (a cell outside the image: a tap never taken)
                const size_t g = (size_t)gy * W + gx;
                c = A.in[g];
                a = A.gA[g];
                b = A.gB[g];
            }
            s_c[i] = c;
            s_a[i] = a;
            s_b[i] = b;
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    v4f c4, a4, b4;
    if (LDS) {
        const int l = (ty + 2 * s) * hx_n + (tx + 2 * s);
        c4 = s_c[l];
        a4 = s_a[l];
        b4 = s_b[l];
    } else {
        c4 = A.in[p];
        a4 = A.gA[p];
        b4 = A.gB[p];
    }
    f3 res = xyz(c4);
    if (__float_as_int(a4[3]) >= 0) {
        const f3 cp = xyz(c4), np = xyz(a4), pp = xyz(b4);
        const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
        f3 sum = F3(0.f, 0.f, 0.f);
        float wsum = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const float k = h[dx + 2] * h[dy + 2];
                v4f cq, aq, bq;
                if (LDS) {
                    const int l = (ty + 2 * s + dy * s) * hx_n + (tx + 2 * s + dx * s);
                    aq = s_a[l];
                    if (__float_as_int(aq[3]) < 0) continue;
                    cq = s_c[l];
                    bq = s_b[l];
                } else {
                    const int qx = x + dx * s, qy = y + dy * s;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t q = (size_t)qy * W + qx;
                    aq = A.gA[q];
                    if (__float_as_int(aq[3]) < 0) continue;
                    cq = A.in[q];
                    bq = A.gB[q];
                }
                dn_tap(k, cp, np, pp, xyz(cq), xyz(aq), xyz(bq), A.inv_ci, A.inv_n, A.inv_p, sum, wsum);
            }
        }
        res = F3(div_cr(sum.x, wsum), div_cr(sum.y, wsum), div_cr(sum.z, wsum));
    }
    if (LAST) {
        if (A.demodulate) res = dn_modulate(res, A.alb[p], false);
        A.out_rgb[3 * p] = res.x;
        A.out_rgb[3 * p + 1] = res.y;
        A.out_rgb[3 * p + 2] = res.z;
    } else {
        A.out[p] = v4f{res.x, res.y, res.z, 0.0f};
    }
}

// ---- variance-guided filter ---------------------------------------------------
// The same tile, halo and tap order as k_dn_level, in kernels of their own (k_dn_level's code does not
// change).  The variance of the luminance rides in the colour plane's w; the colour term is the
// luminance difference in units of the 3 x 3-prefiltered standard deviation at the centre pixel.
constexpr int kRX = kTX + 2, kRY = kTY + 2;       // direct path: the tile + 1 ring of (v, mat)

struct DnvArgs {
    const v4f* __restrict__ in;     // (colour, variance) plane of the previous level
    const v4f* __restrict__ gA;
    const v4f* __restrict__ gB;
    const v4f* __restrict__ alb;    // LAST: remodulation
    v4f* __restrict__ out;          // !LAST
    float* __restrict__ out_rgb;    // LAST: W * H float3
    float* __restrict__ out_var;    // LAST: W * H floats, or NULL
    int32_t W, H, s, demodulate;
    float sigma_l, inv_n, inv_p;
};

// One tap q of pixel p: adds w * c_q into sum, w^2 * v_q into vsum and w into wsum.
__device__ __forceinline__ void dnv_tap(float k, float lp, f3 np, f3 pp, v4f cq4, f3 nq, f3 pq, float rl, float inv_n,
                                        float inv_p, f3& sum, float& vsum, float& wsum) {
    const f3 cq = xyz(cq4);
    const float xl = fabsf(lum(cq) - lp) * rl;
    const float xn = gmax(0.0f, 1.0f - dot(np, nq)) * inv_n;
    const float e = dot(np, pq - pp);
    const float xp = (e * e) * inv_p;
    const float w = div_cr(k, ((1.0f + xl) * (1.0f + xn)) * (1.0f + xp));
    sum = sum + w * cq;
    vsum = vsum + (w * w) * cq4[3];
    wsum = wsum + w;
}

__global__ __launch_bounds__(256) void k_dnv_prologue(const float* __restrict__ rgb, const float* __restrict__ var,
                                                       const v4f* __restrict__ alb, v4f* __restrict__ out, int64_t npix,
                                                       float samples, int demodulate) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        f3 c = F3(div_cr(rgb[3 * i], samples), div_cr(rgb[3 * i + 1], samples), div_cr(rgb[3 * i + 2], samples));
        if (demodulate) c = dn_modulate(c, alb[i], true);
        out[i] = v4f{c.x, c.y, c.z, var[i]};
    }
}

// levels == 0
__global__ __launch_bounds__(256) void k_dnv_epilogue(const v4f* __restrict__ in, const v4f* __restrict__ alb,
                                                       float* __restrict__ out_rgb, float* __restrict__ out_var,
                                                       int64_t npix, int demodulate) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const v4f c4 = in[i];
        f3 c = xyz(c4);
        if (demodulate) c = dn_modulate(c, alb[i], false);
        out_rgb[3 * i] = c.x;
        out_rgb[3 * i + 1] = c.y;
        out_rgb[3 * i + 2] = c.z;
        if (out_var) out_var[i] = c4[3];
    }
}

// Direct path: the nine (v, mat) of the prefilter come from an LDS stage of the tile + 1 ring (2.7 KB);
// reading them with 4-byte loads through L2 instead made the direct levels 15-18% slower at 4K.
template <bool LDS, bool LAST>
__global__ __launch_bounds__(kThreads) void k_dnv_level(const DnvArgs A) {
    __shared__ v4f s_c[LDS ? kHX * kHY : 1], s_a[LDS ? kHX * kHY : 1], s_b[LDS ? kHX * kHY : 1];
    __shared__ float s_rv[LDS ? 1 : kRX * kRY];
    __shared__ int s_rm[LDS ? 1 : kRX * kRY];
    const int W = A.W, H = A.H, s = A.s;
    const int x0 = (int)blockIdx.x * kTX, y0 = (int)blockIdx.y * kTY;
    const int tx = (int)threadIdx.x % kTX, ty = (int)threadIdx.x / kTX;
    const int x = x0 + tx, y = y0 + ty;
    const int hx_n = kTX + 4 * s;   // LDS: the staged footprint (s <= kLdsStep)
    if (LDS) {
        const int hy_n = kTY + 4 * s;
        for (int i = (int)threadIdx.x; i < hx_n * hy_n; i += kThreads) {
            const int hy = i / hx_n, hx = i - hy * hx_n;
            const int gx = x0 - 2 * s + hx, gy = y0 - 2 * s + hy;
            v4f c = {0.f, 0.f, 0.f, 0.f}, a = {0.f, 0.f, 0.f, __int_as_float(-1)}, b = {0.f, 0.f, 0.f, 0.f};
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t g = (size_t)gy * W + gx;
                c = A.in[g];
                a = A.gA[g];
                b = A.gB[g];
            }
            s_c[i] = c;
            s_a[i] = a;
            s_b[i] = b;
        }
        __syncthreads();
    } else {
        for (int i = (int)threadIdx.x; i < kRX * kRY; i += kThreads) {
            const int hy = i / kRX, hx = i - hy * kRX;
            const int gx = x0 - 1 + hx, gy = y0 - 1 + hy;
            float v = 0.0f;
            int m = -1;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t g = (size_t)gy * W + gx;
                v = reinterpret_cast<const float*>(A.in)[4 * g + 3];
                m = reinterpret_cast<const int*>(A.gA)[4 * g + 3];
            }
            s_rv[i] = v;
            s_rm[i] = m;
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    v4f c4, a4, b4;
    if (LDS) {
        const int l = (ty + 2 * s) * hx_n + (tx + 2 * s);
        c4 = s_c[l];
        a4 = s_a[l];
        b4 = s_b[l];
    } else {
        c4 = A.in[p];
        a4 = A.gA[p];
        b4 = A.gB[p];
    }
    f3 res = xyz(c4);
    float vres = c4[3];
    if (__float_as_int(a4[3]) >= 0) {
        // the variance at p, prefiltered over the 3 x 3 unit neighbourhood
        const float g3[3] = {0.25f, 0.5f, 0.25f};
        float gs = 0.0f, gw = 0.0f;
#pragma unroll
        for (int ey = -1; ey <= 1; ++ey) {
#pragma unroll
            for (int ex = -1; ex <= 1; ++ex) {
                float vq;
                if (LDS) {
                    const int l = (ty + 2 * s + ey) * hx_n + (tx + 2 * s + ex);
                    if (__float_as_int(s_a[l][3]) < 0) continue;
                    vq = s_c[l][3];
                } else {
                    const int l = (ty + 1 + ey) * kRX + (tx + 1 + ex);
                    if (s_rm[l] < 0) continue;
                    vq = s_rv[l];
                }
                const float kk = g3[ex + 1] * g3[ey + 1];
                gs = gs + kk * vq;
                gw = gw + kk;
            }
        }
        const float g = div_cr(gs, gw);
        const float rl = div_cr(1.0f, A.sigma_l * sqrt_cr(gmax(0.0f, g) + 0x1p-30f));
        const f3 np = xyz(a4), pp = xyz(b4);
        const float lp = lum(xyz(c4));
        const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
        f3 sum = F3(0.f, 0.f, 0.f);
        float vsum = 0.0f, wsum = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const float k = h[dx + 2] * h[dy + 2];
                v4f cq, aq, bq;
                if (LDS) {
                    const int l = (ty + 2 * s + dy * s) * hx_n + (tx + 2 * s + dx * s);
                    aq = s_a[l];
                    if (__float_as_int(aq[3]) < 0) continue;
                    cq = s_c[l];
                    bq = s_b[l];
                } else {
                    const int qx = x + dx * s, qy = y + dy * s;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t q = (size_t)qy * W + qx;
                    aq = A.gA[q];
                    if (__float_as_int(aq[3]) < 0) continue;
                    cq = A.in[q];
                    bq = A.gB[q];
                }
                dnv_tap(k, lp, np, pp, cq, xyz(aq), xyz(bq), rl, A.inv_n, A.inv_p, sum, vsum, wsum);
            }
        }
        res = F3(div_cr(sum.x, wsum), div_cr(sum.y, wsum), div_cr(sum.z, wsum));
        vres = div_cr(vsum, wsum * wsum);
    }
    if (LAST) {
        if (A.demodulate) res = dn_modulate(res, A.alb[p], false);
        A.out_rgb[3 * p] = res.x;
        A.out_rgb[3 * p + 1] = res.y;
        A.out_rgb[3 * p + 2] = res.z;
        if (A.out_var) A.out_var[p] = vres;
    } else {
        A.out[p] = v4f{res.x, res.y, res.z, vres};
    }
}

// ---- luminance moments of batch means (pt_moments) ------------------------------
// pm = (prev.rgb, m1) per pixel, m2 a plane of its own; one update of one pixel is mom_pixel
// (pt_moments_dev.h).

// QUAD: a lane takes four consecutive pixels, so rgb (3 x 16 B) and m2 (16 B) move as whole 16-byte
// vectors like pm and alb (rgb must be 16-byte aligned); the npix % 4 last pixels, or every pixel
// without QUAD, go one per lane.
template <bool QUAD, bool ALB>
__global__ __launch_bounds__(256) void k_mom_update(const float* __restrict__ rgb, const v4f* __restrict__ alb,
                                                     v4f* __restrict__ pm, float* __restrict__ m2, int64_t npix, float bs) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
    const int64_t nquads = QUAD ? npix / 4 : 0;
    for (int64_t q = t0; q < nquads; q += nt) {
        const v4f* r4 = reinterpret_cast<const v4f*>(rgb) + 3 * q;
        const v4f a = r4[0], b = r4[1], c = r4[2];
        const float in[12] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], c[0], c[1], c[2], c[3]};
        v4f mm = reinterpret_cast<v4f*>(m2)[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = 4 * q + j;
            v4f p = pm[i];
            float m = mm[j];
            mom_pixel(in[3 * j], in[3 * j + 1], in[3 * j + 2], p, m, bs, ALB, ALB ? alb[i] : v4f{0.f, 0.f, 0.f, 0.f});
            pm[i] = p;
            mm[j] = m;
        }
        reinterpret_cast<v4f*>(m2)[q] = mm;
    }
    for (int64_t i = 4 * nquads + t0; i < npix; i += nt) {
        v4f p = pm[i];
        float m = m2[i];
        mom_pixel(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], p, m, bs, ALB, ALB ? alb[i] : v4f{0.f, 0.f, 0.f, 0.f});
        pm[i] = p;
        m2[i] = m;
    }
}

__global__ __launch_bounds__(256) void k_mom_reset(const float* __restrict__ base, v4f* __restrict__ pm,
                                                    float* __restrict__ m2, int64_t npix) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        pm[i] = base ? v4f{base[3 * i], base[3 * i + 1], base[3 * i + 2], 0.0f} : v4f{0.f, 0.f, 0.f, 0.f};
        m2[i] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_mom_variance(const v4f* __restrict__ pm, const float* __restrict__ m2,
                                                       float* __restrict__ var, int64_t npix, float nf, float scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const float mean = div_cr(reinterpret_cast<const float*>(pm)[4 * i + 3], nf);
        const float ex2 = div_cr(m2[i], nf);
        var[i] = gmax(0.0f, ex2 - mean * mean) * scale;
    }
}

bool sigma_ok(float v) { return std::isfinite(v) && v > 0.0f; }

#define DN_TRY(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return pt::fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

}  // namespace

struct pt_denoiser {
    int32_t W = 0, H = 0;
    v4f* plane[2] = {nullptr, nullptr};
};

namespace pt {
int denoise_check(const pt_denoise_params* p, float samples) {
    if (!p) return fail(PT_ERR_ARG, "null denoise parameters");
    if (p->levels < 0 || p->levels > kMaxLevels) return fail(PT_ERR_ARG, "denoise levels must be in 0..8");
    if (!sigma_ok(p->sigma_c) || !sigma_ok(p->sigma_n) || !sigma_ok(p->sigma_p))
        return fail(PT_ERR_ARG, "denoise sigmas must be finite and > 0");
    if (!(samples > 0.0f)) return fail(PT_ERR_ARG, "samples must be > 0");
    return PT_OK;
}
int denoise_var_check(const pt_denoise_var_params* p, float samples) {
    if (!p) return fail(PT_ERR_ARG, "null denoise parameters");
    if (p->levels < 0 || p->levels > kMaxLevels) return fail(PT_ERR_ARG, "denoise levels must be in 0..8");
    if (!sigma_ok(p->sigma_l) || !sigma_ok(p->sigma_n) || !sigma_ok(p->sigma_p))
        return fail(PT_ERR_ARG, "denoise sigmas must be finite and > 0");
    if (!(samples > 0.0f)) return fail(PT_ERR_ARG, "samples must be > 0");
    return PT_OK;
}
}  // namespace pt

struct pt_moments {
    int64_t npix = 0;
    v4f* pm = nullptr;        // (prev.rgb, m1)
    float* m2 = nullptr;
    int32_t batches = 0;
    float batch_samples = 0.0f;
    hipEvent_t ev = nullptr;  // after the last queued work (pt_moments_get waits for it)
    bool ev_recorded = false;
};

namespace pt {
int moments_update_check(const pt_moments* m, float batch_samples) {
    if (!m) return fail(PT_ERR_ARG, "null moments object");
    if (!sigma_ok(batch_samples)) return fail(PT_ERR_ARG, "batch_samples must be finite and > 0");
    if (m->batches > 0 && batch_samples != m->batch_samples)
        return fail(PT_ERR_ARG, "batch_samples differs from the first update's since the last reset");
    return PT_OK;
}
int moments_variance_check(const pt_moments* m, float samples) {
    if (!m) return fail(PT_ERR_ARG, "null moments object");
    if (m->batches < 2) return fail(PT_ERR_ARG, "the variance needs at least 2 batches");
    if (!(samples > 0.0f)) return fail(PT_ERR_ARG, "samples must be > 0");
    return PT_OK;
}
}  // namespace pt

namespace {
int lin_grid_of(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 65536); }
int mom_mark(pt_moments* m, hipStream_t st) {
    DN_TRY(hipEventRecord(m->ev, st));
    m->ev_recorded = true;
    return PT_OK;
}
}  // namespace

extern "C" {

void pt_denoise_params_default(pt_denoise_params* p) {
    if (!p) return;
    *p = pt_denoise_params{};
    p->levels = 5;
    p->sigma_c = 1.0f;   // tuned on Cornell 16 spp against 1024 spp
    p->sigma_n = 0.3f;
    p->sigma_p = 0.2f;
    p->demodulate = 1;
}

int pt_denoiser_create(int32_t width, int32_t height, pt_denoiser** out) {
    if (!out || width < 1 || height < 1 || (int64_t)width * height > kMaxPixels)
        return pt::fail(PT_ERR_ARG, "bad denoiser size");
    pt_denoiser* d = new pt_denoiser;
    d->W = width;
    d->H = height;
    const size_t bytes = (size_t)width * height * sizeof(v4f);
    for (int k = 0; k < 2; ++k) {
        if (hipMalloc((void**)&d->plane[k], bytes) != hipSuccess) {
            pt_denoiser_destroy(d);
            return pt::fail(PT_ERR_NOMEM, "hipMalloc (denoiser planes)");
        }
    }
    *out = d;
    return PT_OK;
}

int pt_denoiser_destroy(pt_denoiser* d) {
    if (!d) return PT_OK;
    for (int k = 0; k < 2; ++k)
        if (d->plane[k]) (void)hipFree(d->plane[k]);
    delete d;
    return PT_OK;
}

int pt_denoiser_run(pt_denoiser* d, const float* d_rgb, float samples, const float* d_gA, const float* d_gB,
                    const float* d_alb, const pt_denoise_params* prm, float* d_out_rgb, void* stream) {
    if (!d || !d_rgb || !d_gA || !d_gB || !d_alb || !d_out_rgb) return pt::fail(PT_ERR_ARG, "null argument");
    if (d_out_rgb == d_rgb) return pt::fail(PT_ERR_ARG, "the output must not alias the input");
    if (int rc = pt::denoise_check(prm, samples)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t npix = (int64_t)d->W * d->H;
    const int lin_grid = (int)std::min<int64_t>((npix + 255) / 256, 65536);
    hipLaunchKernelGGL(k_dn_prologue, dim3(lin_grid), dim3(256), 0, st, d_rgb, (const v4f*)d_alb, d->plane[0], npix,
                       samples, prm->demodulate);
    DN_TRY(hipGetLastError());
    if (prm->levels == 0) {
        hipLaunchKernelGGL(k_dn_epilogue, dim3(lin_grid), dim3(256), 0, st, (const v4f*)d->plane[0], (const v4f*)d_alb,
                           d_out_rgb, npix, prm->demodulate);
        DN_TRY(hipGetLastError());
        return PT_OK;
    }
    const float inv_c = 1.0f / (prm->sigma_c * prm->sigma_c);
    DnArgs A{};
    A.gA = (const v4f*)d_gA;
    A.gB = (const v4f*)d_gB;
    A.alb = (const v4f*)d_alb;
    A.out_rgb = d_out_rgb;
    A.W = d->W;
    A.H = d->H;
    A.demodulate = prm->demodulate;
    A.inv_n = 1.0f / (prm->sigma_n * prm->sigma_n);
    A.inv_p = 1.0f / (prm->sigma_p * prm->sigma_p);
    const dim3 grid((d->W + kTX - 1) / kTX, (d->H + kTY - 1) / kTY);
    for (int i = 0; i < prm->levels; ++i) {
        A.in = d->plane[i & 1];
        A.out = d->plane[(i + 1) & 1];
        A.s = 1 << i;
        A.inv_ci = inv_c * (float)(1 << (2 * i));   // sigma_c halves per level
        const bool last = i == prm->levels - 1, lds = A.s <= kLdsStep;
        auto kern = lds ? (last ? k_dn_level<true, true> : k_dn_level<true, false>)
                        : (last ? k_dn_level<false, true> : k_dn_level<false, false>);
        hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, st, A);
        DN_TRY(hipGetLastError());
    }
    return PT_OK;
}

int pt_denoise_host(int32_t width, int32_t height, const float* rgb, float samples, const float* gA, const float* gB,
                    const float* alb, const pt_denoise_params* prm, float* out_rgb) {
    if (width < 1 || height < 1 || (int64_t)width * height > kMaxPixels) return pt::fail(PT_ERR_ARG, "bad image size");
    if (!rgb || !gA || !gB || !alb || !out_rgb) return pt::fail(PT_ERR_ARG, "null argument");
    if (out_rgb == rgb) return pt::fail(PT_ERR_ARG, "the output must not alias the input");
    if (int rc = pt::denoise_check(prm, samples)) return rc;
    const size_t npix = (size_t)width * height;
    float* dev = nullptr;   // rgb | out | gA | gB | alb
    if (hipMalloc((void**)&dev, npix * 18 * sizeof(float)) != hipSuccess) return pt::fail(PT_ERR_NOMEM, "hipMalloc (denoise)");
    float *d_rgb = dev, *d_out = dev + 3 * npix, *d_gA = dev + 6 * npix, *d_gB = dev + 10 * npix, *d_alb = dev + 14 * npix;
    pt_denoiser* dn = nullptr;
    hipStream_t st = nullptr;
    int rc = pt_denoiser_create(width, height, &dn);
    hipError_t e = hipSuccess;
    if (!rc) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (!rc && e == hipSuccess) {
        e = hipMemcpyAsync(d_rgb, rgb, npix * 3 * sizeof(float), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_gA, gA, npix * 4 * sizeof(float), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_gB, gB, npix * 4 * sizeof(float), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_alb, alb, npix * 4 * sizeof(float), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) rc = pt_denoiser_run(dn, d_rgb, samples, d_gA, d_gB, d_alb, prm, d_out, st);
        if (e == hipSuccess && !rc) e = hipMemcpyAsync(out_rgb, d_out, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, st);
        const hipError_t e2 = hipStreamSynchronize(st);
        if (e == hipSuccess) e = e2;
    }
    if (st) (void)hipStreamDestroy(st);
    pt_denoiser_destroy(dn);
    (void)hipFree(dev);
    if (rc) return rc;
    if (e != hipSuccess) return pt::fail(PT_ERR_HIP, std::string("pt_denoise_host: ") + hipGetErrorString(e));
    return PT_OK;
}

// ---- variance-guided filter ---------------------------------------------------------------------
void pt_denoise_var_params_default(pt_denoise_var_params* p) {
    if (!p) return;
    *p = pt_denoise_var_params{};
    p->levels = 5;
    p->sigma_l = 1.0f;   // chosen on Cornell 16 and 256 spp against 1024 spp
    p->sigma_n = 0.3f;
    p->sigma_p = 0.2f;
    p->demodulate = 1;
}

int pt_denoiser_run_var(pt_denoiser* d, const float* d_rgb, float samples, const float* d_var, const float* d_gA,
                        const float* d_gB, const float* d_alb, const pt_denoise_var_params* prm, float* d_out_rgb,
                        float* d_out_var, void* stream) {
    if (!d || !d_rgb || !d_var || !d_gA || !d_gB || !d_alb || !d_out_rgb) return pt::fail(PT_ERR_ARG, "null argument");
    if (d_out_rgb == d_rgb || (d_out_var && d_out_var == d_var))
        return pt::fail(PT_ERR_ARG, "the outputs must not alias the inputs");
    if (int rc = pt::denoise_var_check(prm, samples)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t npix = (int64_t)d->W * d->H;
    const int lin_grid = lin_grid_of(npix);
    hipLaunchKernelGGL(k_dnv_prologue, dim3(lin_grid), dim3(256), 0, st, d_rgb, d_var, (const v4f*)d_alb, d->plane[0], npix,
                       samples, prm->demodulate);
    DN_TRY(hipGetLastError());
    if (prm->levels == 0) {
        hipLaunchKernelGGL(k_dnv_epilogue, dim3(lin_grid), dim3(256), 0, st, (const v4f*)d->plane[0], (const v4f*)d_alb,
                           d_out_rgb, d_out_var, npix, prm->demodulate);
        DN_TRY(hipGetLastError());
        return PT_OK;
    }
    DnvArgs A{};
    A.gA = (const v4f*)d_gA;
    A.gB = (const v4f*)d_gB;
    A.alb = (const v4f*)d_alb;
    A.out_rgb = d_out_rgb;
    A.out_var = d_out_var;
    A.W = d->W;
    A.H = d->H;
    A.demodulate = prm->demodulate;
    A.sigma_l = prm->sigma_l;   // the same at every level: the filtered variance narrows the term
    A.inv_n = 1.0f / (prm->sigma_n * prm->sigma_n);
    A.inv_p = 1.0f / (prm->sigma_p * prm->sigma_p);
    const dim3 grid((d->W + kTX - 1) / kTX, (d->H + kTY - 1) / kTY);
    for (int i = 0; i < prm->levels; ++i) {
        A.in = d->plane[i & 1];
        A.out = d->plane[(i + 1) & 1];
        A.s = 1 << i;
        const bool last = i == prm->levels - 1, lds = A.s <= kLdsStep;
        auto kern = lds ? (last ? k_dnv_level<true, true> : k_dnv_level<true, false>)
                        : (last ? k_dnv_level<false, true> : k_dnv_level<false, false>);
        hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, st, A);
        DN_TRY(hipGetLastError());
    }
    return PT_OK;
}

int pt_denoise_var_host(int32_t width, int32_t height, const float* rgb, float samples, const float* var,
                        const float* gA, const float* gB, const float* alb, const pt_denoise_var_params* prm,
                        float* out_rgb, float* out_var) {
    if (width < 1 || height < 1 || (int64_t)width * height > kMaxPixels) return pt::fail(PT_ERR_ARG, "bad image size");
    if (!rgb || !var || !gA || !gB || !alb || !out_rgb) return pt::fail(PT_ERR_ARG, "null argument");
    if (out_rgb == rgb || (out_var && out_var == var)) return pt::fail(PT_ERR_ARG, "the outputs must not alias the inputs");
    if (int rc = pt::denoise_var_check(prm, samples)) return rc;
    const size_t npix = (size_t)width * height;
    float* dev = nullptr;   // rgb | out | gA | gB | alb | var | out_var
    if (hipMalloc((void**)&dev, npix * 20 * sizeof(float)) != hipSuccess) return pt::fail(PT_ERR_NOMEM, "hipMalloc (denoise)");
    float *d_rgb = dev, *d_out = dev + 3 * npix, *d_gA = dev + 6 * npix, *d_gB = dev + 10 * npix, *d_alb = dev + 14 * npix;
    float *d_var = dev + 18 * npix, *d_ovar = dev + 19 * npix;
    pt_denoiser* dn = nullptr;
    hipStream_t st = nullptr;
    int rc = pt_denoiser_create(width, height, &dn);
    hipError_t e = hipSuccess;
    if (!rc) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (!rc && e == hipSuccess) {
        e = hipMemcpyAsync(d_rgb, rgb, npix * 3 * sizeof(float), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_var, var, npix * sizeof(float), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_gA, gA, npix * 4 * sizeof(float), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_gB, gB, npix * 4 * sizeof(float), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_alb, alb, npix * 4 * sizeof(float), hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            rc = pt_denoiser_run_var(dn, d_rgb, samples, d_var, d_gA, d_gB, d_alb, prm, d_out, out_var ? d_ovar : nullptr, st);
        if (e == hipSuccess && !rc) e = hipMemcpyAsync(out_rgb, d_out, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && !rc && out_var)
            e = hipMemcpyAsync(out_var, d_ovar, npix * sizeof(float), hipMemcpyDeviceToHost, st);
        const hipError_t e2 = hipStreamSynchronize(st);
        if (e == hipSuccess) e = e2;
    }
    if (st) (void)hipStreamDestroy(st);
    pt_denoiser_destroy(dn);
    (void)hipFree(dev);
    if (rc) return rc;
    if (e != hipSuccess) return pt::fail(PT_ERR_HIP, std::string("pt_denoise_var_host: ") + hipGetErrorString(e));
    return PT_OK;
}

// ---- luminance moments of batch means -------------------------------------------------------------
int pt_moments_create(int32_t width, int32_t height, pt_moments** out) {
    if (!out || width < 1 || height < 1 || (int64_t)width * height > kMaxPixels)
        return pt::fail(PT_ERR_ARG, "bad moments size");
    pt_moments* m = new pt_moments;   // (the planes come with the first reset or update: mom_planes)
    m->npix = (int64_t)width * height;
    *out = m;
    return PT_OK;
}

// The device side of the object, allocated at its first use and zeroed on `st`.
static int mom_planes(pt_moments* m, hipStream_t st, bool zero) {
    if (m->pm) return PT_OK;
    // (m2 is read in 16-byte vectors: the allocation is a whole number of them)
    if (hipMalloc((void**)&m->pm, (size_t)m->npix * sizeof(v4f)) != hipSuccess ||
        hipMalloc((void**)&m->m2, (size_t)((m->npix + 3) / 4) * sizeof(v4f)) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev, hipEventDisableTiming) != hipSuccess) {
        if (m->pm) (void)hipFree(m->pm);
        if (m->m2) (void)hipFree(m->m2);
        m->pm = nullptr;
        m->m2 = nullptr;
        return pt::fail(PT_ERR_NOMEM, "hipMalloc (moments planes)");
    }
    if (zero) {
        hipLaunchKernelGGL(k_mom_reset, dim3(lin_grid_of(m->npix)), dim3(256), 0, st, (const float*)nullptr, m->pm, m->m2,
                           m->npix);
        DN_TRY(hipGetLastError());
    }
    return PT_OK;
}

int pt_moments_destroy(pt_moments* m) {
    if (!m) return PT_OK;
    if (m->ev_recorded) (void)hipEventSynchronize(m->ev);
    if (m->ev) (void)hipEventDestroy(m->ev);
    if (m->pm) (void)hipFree(m->pm);
    if (m->m2) (void)hipFree(m->m2);
    delete m;
    return PT_OK;
}

int pt_moments_reset(pt_moments* m, const float* d_base_rgb, void* stream) {
    if (!m) return pt::fail(PT_ERR_ARG, "null moments object");
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = mom_planes(m, st, false)) return rc;
    hipLaunchKernelGGL(k_mom_reset, dim3(lin_grid_of(m->npix)), dim3(256), 0, st, d_base_rgb, m->pm, m->m2, m->npix);
    DN_TRY(hipGetLastError());
    m->batches = 0;
    m->batch_samples = 0.0f;
    return mom_mark(m, st);
}

int pt_moments_update(pt_moments* m, const float* d_rgb, float batch_samples, const float* d_alb, void* stream) {
    if (!m || !d_rgb) return pt::fail(PT_ERR_ARG, "null argument");
    if (int rc = pt::moments_update_check(m, batch_samples)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = mom_planes(m, st, true)) return rc;
    const bool quad = (reinterpret_cast<uintptr_t>(d_rgb) & 15u) == 0;
    const int64_t lanes = quad ? (m->npix + 3) / 4 : m->npix;
    auto kern = quad ? (d_alb ? k_mom_update<true, true> : k_mom_update<true, false>)
                     : (d_alb ? k_mom_update<false, true> : k_mom_update<false, false>);
    hipLaunchKernelGGL(kern, dim3(lin_grid_of(lanes)), dim3(256), 0, st, d_rgb, (const v4f*)d_alb, m->pm, m->m2, m->npix,
                       batch_samples);
    DN_TRY(hipGetLastError());
    m->batches += 1;
    m->batch_samples = batch_samples;
    return mom_mark(m, st);
}

int pt_moments_info(const pt_moments* m, int32_t* batches, float* batch_samples) {
    if (!m) return pt::fail(PT_ERR_ARG, "null moments object");
    if (batches) *batches = m->batches;
    if (batch_samples) *batch_samples = m->batch_samples;
    return PT_OK;
}

int pt_moments_variance(pt_moments* m, float samples, float* d_var, void* stream) {
    if (!m || !d_var) return pt::fail(PT_ERR_ARG, "null argument");
    if (int rc = pt::moments_variance_check(m, samples)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const float nf = (float)m->batches;
    const float scale = (nf * m->batch_samples) / ((nf - 1.0f) * samples);
    hipLaunchKernelGGL(k_mom_variance, dim3(lin_grid_of(m->npix)), dim3(256), 0, st, (const v4f*)m->pm,
                       (const float*)m->m2, d_var, m->npix, nf, scale);
    DN_TRY(hipGetLastError());
    return mom_mark(m, st);
}

int pt_moments_get(pt_moments* m, float* h_m1, float* h_m2, float* h_prev_rgb) {
    if (!m) return pt::fail(PT_ERR_ARG, "null moments object");
    if (int rc = mom_planes(m, nullptr, true)) return rc;
    if (m->ev_recorded) DN_TRY(hipEventSynchronize(m->ev));
    else DN_TRY(hipStreamSynchronize(nullptr));
    const size_t n = (size_t)m->npix;
    if (h_m2) DN_TRY(hipMemcpy(h_m2, m->m2, n * sizeof(float), hipMemcpyDeviceToHost));
    if (h_m1 || h_prev_rgb) {
        std::vector<float> pm(4 * n);
        DN_TRY(hipMemcpy(pm.data(), m->pm, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (h_m1) h_m1[i] = pm[4 * i + 3];
            for (int k = 0; k < 3 && h_prev_rgb; ++k) h_prev_rgb[3 * i + k] = pm[4 * i + k];
        }
    }
    return PT_OK;
}

}  // extern "C"
