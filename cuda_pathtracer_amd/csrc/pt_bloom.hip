// Bloom on the device (pt_bloom), gfx950: the float accumulator plus its glare, still in the
// accumulator's unit.  A bright pass, a pyramid of K levels through the binomial [1 3 3 1]/8, a 2x tent on the way
// back up and the composition.  The output is an exact function of the input floats: every operation is one of
// + - * / on floats, a float comparison or index arithmetic (this unit is built with the flags of every other unit:
// no fast-math, no contraction), so tests/bloom_ref.py restates it in numpy and compares with ==.
//
// The pyramid is one allocation made at first use: the levels 1 .. K one after another, RGBA32F texels (16-byte
// loads and stores; the fourth channel is 0).
//   k_bloom_first    (k_bloom_down<FIRST = true>) the 12-byte pixels through the bright pass into level 1: the bright
//                    pass is part of the first down step, level 0 is never stored.
//   k_bloom_down     (k_bloom_down<FIRST = false>) level k to level k + 1.
//   k_bloom_up       U_k = B_k + spread * up(U_k+1), in place over B_k (a lane reads and writes its own texel of
//                    level k, the taps come from level k + 1).
//   k_bloom_compose  out = v + (up(U_1) * gain) * samples; a lane reads only its own pixel of v, so d_out may be d_rgb.
// A workgroup of 256 takes tiles of 32 x 8 output texels; the grid is at most kGrid workgroups, which stride over
// the level's tiles.  No workgroup waits for another.
// The two down kernels stage the 66 x 18 source texels of their tile in LDS (the 64 x 16 under it and a one-texel
// apron, each index clamped to the level, each pixel bright-passed once), filter them horizontally into 32 x 18 sums
// in LDS and vertically out of them.  The direct form (a lane's 16 taps from the cache, which is 16 bright passes a
// texel in k_bloom_first) computes the same bits and was measured slower (0.318 against 0.247 ms at
// 3840 x 2160); it is not kept.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "pt_enc.h"

using namespace pt;

namespace {

constexpr int kGrid = 256;            // workgroups at most
constexpr int kTW = 32, kTH = 8;      // a workgroup's tile of output texels
constexpr int kSW = 2 * kTW + 2, kSH = 2 * kTH + 2;   // the source texels of a down tile
constexpr int kMaxLevels = 12;

typedef float f4 __attribute__((ext_vector_type(4)));

struct BrightK {
    float n, clamp, threshold;
};

__device__ __forceinline__ int clampi(int v, int n) { return min(max(v, 0), n - 1); }

// B0 of the pixel p (step 1)
__device__ __forceinline__ f4 bright(const float* rgb, long long p, const BrightK& k) {
    float c[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float v = rgb[3 * p + j] / k.n;
        v = v > 0.0f ? v : 0.0f;   // (NaN, negatives and -0 to +0)
        c[j] = v < k.clamp ? v : k.clamp;
    }
    const float L = (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2];
    const float w = L > k.threshold ? (L - k.threshold) / L : 0.0f;
    f4 o = {c[0] * w, c[1] * w, c[2] * w, 0.0f};
    return o;
}

__device__ __forceinline__ f4 binom(f4 a, f4 b, f4 c, f4 d) { return (a + d) + 3.0f * (b + c); }

// One tile of a level of dw x dh texels per round; t is uniform over the workgroup
__device__ __forceinline__ int tiles_of(int dw, int dh, int* tiles_x) {
    *tiles_x = (dw + kTW - 1) / kTW;
    return *tiles_x * ((dh + kTH - 1) / kTH);
}

template <bool FIRST>
__device__ __forceinline__ f4 source(const float* rgb, const BrightK& bk, const f4* src, int sw, int x, int y) {
    const long long p = (long long)y * sw + x;
    if (FIRST) return bright(rgb, p, bk);
    return src[p];
}

// Step 2: the level (rgb through the bright pass when FIRST, else src) of sw x sh to dst of dw x dh
template <bool FIRST>
__global__ __launch_bounds__(256) void k_bloom_down(const float* rgb, BrightK bk, const f4* __restrict__ src, int sw, int sh,
                                                    f4* __restrict__ dst, int dw, int dh) {
    __shared__ f4 s_src[kSW * kSH];
    __shared__ f4 s_h[kTW * kSH];
    int tiles_x;
    const int ntiles = tiles_of(dw, dh, &tiles_x);
    const int tid = (int)threadIdx.x, lx = tid & (kTW - 1), ly = tid / kTW;
    for (int t = (int)blockIdx.x; t < ntiles; t += (int)gridDim.x) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x = tx * kTW + lx, y = ty * kTH + ly;
        const int x0 = 2 * tx * kTW - 1, y0 = 2 * ty * kTH - 1;
        for (int i = tid; i < kSW * kSH; i += 256) {
            const int sy = i / kSW, sx = i - sy * kSW;
            s_src[i] = source<FIRST>(rgb, bk, src, sw, clampi(x0 + sx, sw), clampi(y0 + sy, sh));
        }
        __syncthreads();
        for (int i = tid; i < kTW * kSH; i += 256) {
            const f4* r = s_src + (i / kTW) * kSW + 2 * (i & (kTW - 1));
            s_h[i] = binom(r[0], r[1], r[2], r[3]);
        }
        __syncthreads();   // (the next round's writes to s_h come behind its first barrier)
        f4 h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = s_h[(2 * ly + j) * kTW + lx];
        if (x >= dw || y >= dh) continue;
        dst[(long long)y * dw + x] = binom(h[0], h[1], h[2], h[3]) * (1.0f / 64.0f);
    }
}

// up(T) at the fine texel (x, y); T has cw x ch texels (step 3)
__device__ __forceinline__ f4 up_at(const f4* __restrict__ T, int cw, int ch, int x, int y) {
    const int nx = x >> 1, fx = clampi((x & 1) ? nx + 1 : nx - 1, cw);
    const int ny = y >> 1, fy = clampi((y & 1) ? ny + 1 : ny - 1, ch);
    const f4* rn = T + (long long)ny * cw;
    const f4* rf = T + (long long)fy * cw;
    const f4 hn = (3.0f * rn[nx] + rn[fx]) * 0.25f, hf = (3.0f * rf[nx] + rf[fx]) * 0.25f;
    return (3.0f * hn + hf) * 0.25f;
}

__global__ __launch_bounds__(256) void k_bloom_up(f4* __restrict__ fine, int w, int h, const f4* __restrict__ coarse, int cw, int ch,
                                                  float spread) {
    int tiles_x;
    const int ntiles = tiles_of(w, h, &tiles_x);
    const int lx = (int)threadIdx.x & (kTW - 1), ly = (int)threadIdx.x / kTW;
    for (int t = (int)blockIdx.x; t < ntiles; t += (int)gridDim.x) {
        const int ty = t / tiles_x, x = (t - ty * tiles_x) * kTW + lx, y = ty * kTH + ly;
        if (x >= w || y >= h) continue;
        f4* p = fine + (long long)y * w + x;
        *p = *p + spread * up_at(coarse, cw, ch, x, y);
    }
}

// (rgb and out may be the same pointer: no __restrict__ on them)
__global__ __launch_bounds__(256) void k_bloom_compose(const float* rgb, float* out, int w, int h, const f4* __restrict__ coarse, int cw,
                                                       int ch, float gain, float n) {
    int tiles_x;
    const int ntiles = tiles_of(w, h, &tiles_x);
    const int lx = (int)threadIdx.x & (kTW - 1), ly = (int)threadIdx.x / kTW;
    for (int t = (int)blockIdx.x; t < ntiles; t += (int)gridDim.x) {
        const int ty = t / tiles_x, x = (t - ty * tiles_x) * kTW + lx, y = ty * kTH + ly;
        if (x >= w || y >= h) continue;
        const long long p = 3 * ((long long)y * w + x);
        const f4 g = (up_at(coarse, cw, ch, x, y) * gain) * n;
        const float r0 = rgb[p] + g.x, r1 = rgb[p + 1] + g.y, r2 = rgb[p + 2] + g.z;
        out[p] = r0;
        out[p + 1] = r1;
        out[p + 2] = r2;
    }
}

#define BLOOM_TRY(expr)                                                                 \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess)                                                           \
            return fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

}  // namespace

struct pt_bloom {
    int32_t W = 0, H = 0, K = 0;
    pt_bloom_params prm{};
    int32_t lw[kMaxLevels + 1] = {}, lh[kMaxLevels + 1] = {};   // [0]: the image
    size_t off[kMaxLevels + 2] = {};                            // texels before level k (k = 1 .. K); [K + 1]: all
    float gain = 0.0f;
    f4* dev = nullptr;         // the pyramid, one allocation made at first use
    hipEvent_t ev = nullptr;   // after the last queued work (the destructor waits for it)
    bool ev_recorded = false;
    ~pt_bloom() {
        if (ev_recorded) (void)hipEventSynchronize(ev);
        if (ev) (void)hipEventDestroy(ev);
        if (dev) (void)hipFree(dev);
    }
};

int pt::bloom_size(const pt_bloom* b, int32_t* width, int32_t* height) {
    if (!b) return fail(PT_ERR_ARG, "null bloom");
    *width = b->W;
    *height = b->H;
    return PT_OK;
}

namespace {

int params_check(const pt_bloom_params* p) {
    auto finite = [](float v) { return std::isfinite(v); };
    for (int32_t r : p->reserved)
        if (r != 0) return fail(PT_ERR_ARG, "pt_bloom_params.reserved must be zero");
    if (!finite(p->threshold) || !(p->threshold >= 0.0f)) return fail(PT_ERR_ARG, "threshold must be finite and >= 0");
    if (!finite(p->strength) || !(p->strength >= 0.0f)) return fail(PT_ERR_ARG, "strength must be finite and >= 0");
    if (!finite(p->spread) || !(p->spread > 0.0f) || p->spread > 1.0f) return fail(PT_ERR_ARG, "spread must satisfy 0 < spread <= 1");
    if (!finite(p->clamp) || !(p->clamp > 0.0f) || p->clamp > 65504.0f) return fail(PT_ERR_ARG, "clamp must satisfy 0 < clamp <= 65504");
    if (p->levels < 0 || p->levels > kMaxLevels) return fail(PT_ERR_ARG, "levels must be 0 (from the size) or lie in 1 .. 12");
    return PT_OK;
}

int samples_check(float samples) {
    if (!std::isfinite(samples) || !(samples > 0.0f)) return fail(PT_ERR_ARG, "samples must be finite and > 0");
    return PT_OK;
}

int apply_check(const pt_bloom* b, const float* d_rgb, float samples, const float* d_out) {
    if (!b || !d_rgb || !d_out) return fail(PT_ERR_ARG, "null argument");
    const uintptr_t a = (uintptr_t)d_rgb, o = (uintptr_t)d_out;
    if ((a | o) & 3) return fail(PT_ERR_ARG, "d_rgb and d_out must be aligned to 4 bytes");
    const uint64_t bytes = (uint64_t)b->W * b->H * 12;
    if (a != o && a < o + bytes && o < a + bytes) return fail(PT_ERR_ARG, "d_out must be d_rgb itself or not overlap it");
    return samples_check(samples);
}

int bloom_alloc(pt_bloom* b) {
    if (b->dev) return PT_OK;
    if (hipMalloc((void**)&b->dev, b->off[b->K + 1] * sizeof(f4)) != hipSuccess ||
        (!b->ev && hipEventCreateWithFlags(&b->ev, hipEventDisableTiming) != hipSuccess)) {
        if (b->dev) (void)hipFree(b->dev);
        b->dev = nullptr;
        (void)hipGetLastError();
        return fail(PT_ERR_NOMEM, "hipMalloc (bloom pyramid)");
    }
    return PT_OK;
}

int grid_for(int w, int h) {
    const int64_t tiles = (int64_t)((w + kTW - 1) / kTW) * ((h + kTH - 1) / kTH);
    return (int)std::min<int64_t>(tiles, kGrid);
}

int apply(pt_bloom* b, const float* d_rgb, float samples, float* d_out, hipStream_t st) {
    const pt_bloom_params& p = b->prm;
    const BrightK bk{samples, p.clamp, p.threshold};
    const int K = b->K;
    auto level = [&](int k) { return b->dev + b->off[k]; };
    hipLaunchKernelGGL(k_bloom_down<true>, dim3(grid_for(b->lw[1], b->lh[1])), dim3(256), 0, st, d_rgb, bk,
                       (const f4*)nullptr, b->lw[0], b->lh[0], level(1), b->lw[1], b->lh[1]);
    for (int k = 2; k <= K; ++k)
        hipLaunchKernelGGL(k_bloom_down<false>, dim3(grid_for(b->lw[k], b->lh[k])), dim3(256), 0, st,
                           (const float*)nullptr, bk, (const f4*)level(k - 1), b->lw[k - 1], b->lh[k - 1], level(k), b->lw[k], b->lh[k]);
    for (int k = K - 1; k >= 1; --k)
        hipLaunchKernelGGL(k_bloom_up, dim3(grid_for(b->lw[k], b->lh[k])), dim3(256), 0, st, level(k), b->lw[k], b->lh[k],
                           (const f4*)level(k + 1), b->lw[k + 1], b->lh[k + 1], p.spread);
    hipLaunchKernelGGL(k_bloom_compose, dim3(grid_for(b->W, b->H)), dim3(256), 0, st, d_rgb, d_out, b->W, b->H, (const f4*)level(1),
                       b->lw[1], b->lh[1], b->gain, samples);
    BLOOM_TRY(hipGetLastError());
    BLOOM_TRY(hipEventRecord(b->ev, st));
    b->ev_recorded = true;
    return PT_OK;
}

}  // namespace

extern "C" {

void pt_bloom_params_default(pt_bloom_params* p) {
    if (!p) return;
    *p = pt_bloom_params{};
    p->threshold = 1.0f;
    p->strength = 0.25f;
    p->spread = 0.75f;
    p->clamp = 65504.0f;
    p->levels = 0;
}

int pt_bloom_create(int32_t width, int32_t height, const pt_bloom_params* p, pt_bloom** out) {
    if (!out || !p) return fail(PT_ERR_ARG, "null argument");
    if (int rc = params_check(p)) return rc;
    if (width < 1 || height < 1) return fail(PT_ERR_ARG, "bloom width and height must be at least 1");
    if ((int64_t)width * height >= ((int64_t)1 << 31)) return fail(PT_ERR_ARG, "bloom image too large: width * height must stay below 2^31");
    pt_bloom* b = new pt_bloom;   // (the pyramid comes with the first use: bloom_alloc)
    b->W = width;
    b->H = height;
    b->prm = *p;
    int K = p->levels;
    if (K == 0) {
        int lg = 0;
        while ((std::min(width, height) >> (lg + 1)) > 0) ++lg;   // floor(log2(min(W, H)))
        K = std::min(std::max(lg, 1), 6);
    }
    b->K = K;
    b->lw[0] = width;
    b->lh[0] = height;
    size_t at = 0;
    for (int k = 1; k <= K; ++k) {
        b->lw[k] = (b->lw[k - 1] + 1) >> 1;
        b->lh[k] = (b->lh[k - 1] + 1) >> 1;
        b->off[k] = at;
        at += (size_t)b->lw[k] * b->lh[k];
    }
    b->off[K + 1] = at;
    double sum = 0.0, pw = 1.0;
    for (int i = 0; i < K; ++i) {
        sum += pw;
        pw *= (double)p->spread;
    }
    b->gain = (float)((double)p->strength / sum);
    *out = b;
    return PT_OK;
}

int pt_bloom_destroy(pt_bloom* b) {
    delete b;   // (waits for the last queued work)
    return PT_OK;
}

int pt_bloom_info(pt_bloom* b, int32_t* levels, int32_t widths[12], int32_t heights[12]) {
    if (!b) return fail(PT_ERR_ARG, "null bloom");
    if (levels) *levels = b->K;
    for (int k = 1; k <= kMaxLevels; ++k) {
        if (widths) widths[k - 1] = k <= b->K ? b->lw[k] : 0;
        if (heights) heights[k - 1] = k <= b->K ? b->lh[k] : 0;
    }
    return PT_OK;
}

int pt_bloom_apply(pt_bloom* b, const float* d_rgb, float samples, float* d_out, void* stream) {
    if (int rc = apply_check(b, d_rgb, samples, d_out)) return rc;
    if (int rc = bloom_alloc(b)) return rc;
    return apply(b, d_rgb, samples, d_out, (hipStream_t)stream);
}

int pt_bloom_host(int32_t width, int32_t height, const float* rgb, float samples, const pt_bloom_params* p, float* out) {
    if (!rgb || !out) return fail(PT_ERR_ARG, "null argument");
    if (int rc = samples_check(samples)) return rc;
    pt_bloom* b = nullptr;
    if (int rc = pt_bloom_create(width, height, p, &b)) return rc;
    const size_t bytes = (size_t)width * height * 3 * sizeof(float);
    float* dev = nullptr;
    if (hipMalloc((void**)&dev, bytes) != hipSuccess) {
        (void)hipGetLastError();
        delete b;
        return fail(PT_ERR_NOMEM, "hipMalloc (bloom host image)");
    }
    hipError_t he = hipMemcpy(dev, rgb, bytes, hipMemcpyHostToDevice);
    int rc = PT_OK;
    if (he == hipSuccess) rc = pt_bloom_apply(b, dev, samples, dev, nullptr);   // (in place)
    if (he == hipSuccess && !rc) he = hipMemcpy(out, dev, bytes, hipMemcpyDeviceToHost);   // (waits for the kernels)
    delete b;
    (void)hipFree(dev);
    if (rc) return rc;
    if (he != hipSuccess) return fail(PT_ERR_HIP, std::string("pt_bloom_host: ") + hipGetErrorString(he));
    return PT_OK;
}

}  // extern "C"
