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
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "pt_device.h"
#include "pt_internal.h"

using namespace ptd;

namespace {

constexpr int kTX = 32, kTY = 8, kThreads = kTX * kTY;
constexpr int kLdsStep = 2;                       // largest step staged in LDS
constexpr int kHX = kTX + 4 * kLdsStep, kHY = kTY + 4 * kLdsStep;
constexpr float kAlbMin = 0x1p-10f;               // albedo components below are not (de)modulated
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

__device__ __forceinline__ f3 dn_modulate(f3 c, v4f a, bool divide) {
    if (a[0] >= kAlbMin) c.x = divide ? div_cr(c.x, a[0]) : c.x * a[0];
    if (a[1] >= kAlbMin) c.y = divide ? div_cr(c.y, a[1]) : c.y * a[1];
    if (a[2] >= kAlbMin) c.z = divide ? div_cr(c.z, a[2]) : c.z * a[2];
    return c;
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
}  // namespace pt

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

}  // extern "C"
