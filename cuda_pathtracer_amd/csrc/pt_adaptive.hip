// Adaptive sampling state (pt_adaptive), gfx950: pt_moments' luminance moments kept per
// pixel, a batch count nb and an active flag act per BLOCK of 64 consecutive pixels (one word of the
// first bounce's camera masks), and the selection that turns the moments into the next act.  The
// contract is §10 / §11's: compiled with -ffp-contract=off, every operation below one correctly
// rounded fp32 operation in the stated order ('/' is div_cr, sqrt is sqrt_cr); tests/adaptive_ref.py
// restates it in numpy float32 and the GPU tests compare bit for bit.
//
// Kernel shape: all streaming, no LDS but k_ad_dilate's four count words, no atomics, no
// inter-workgroup waits.  k_ad_update is k_mom_update gated by the pixel's block (a 16-byte group of
// four pixels never straddles a block: blocks are 64-aligned); k_ad_dilate takes one wave per block,
// lane = pixel, and reduces the count of active blocks per workgroup into slots the host sums.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "pt_internal.h"
#include "pt_moments_dev.h"

using namespace ptd;

namespace {

constexpr int64_t kMaxPixels = (int64_t)1 << 30;
constexpr int kDilateGrid = 2048;   // k_ad_dilate's workgroups at most (= count slots)

__global__ __launch_bounds__(256) void k_ad_reset(const float* __restrict__ base, v4f* __restrict__ pm,
                                                   float* __restrict__ m2, uint32_t* __restrict__ nb,
                                                   uint32_t* __restrict__ act, uint8_t* __restrict__ hot, int64_t npix) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        pm[i] = base ? v4f{base[3 * i], base[3 * i + 1], base[3 * i + 2], 0.0f} : v4f{0.f, 0.f, 0.f, 0.f};
        m2[i] = 0.0f;
        hot[i] = 1;
        if ((i & 63) == 0) {
            nb[i >> 6] = 0u;
            act[i >> 6] = 1u;
        }
    }
}

// QUAD as k_mom_update's: four consecutive pixels per lane in whole 16-byte vectors (rgb 16-byte
// aligned), the block's act uniform over 16 lanes; the npix % 4 last pixels, or every pixel without
// QUAD, go one per lane.  The lane that holds a block's first pixel counts the block's batch.
template <bool QUAD, bool ALB>
__global__ __launch_bounds__(256) void k_ad_update(const float* __restrict__ rgb, const v4f* __restrict__ alb,
                                                    v4f* __restrict__ pm, float* __restrict__ m2,
                                                    uint32_t* __restrict__ nb, const uint32_t* __restrict__ act,
                                                    int64_t npix, float bs) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
    const int64_t nquads = QUAD ? npix / 4 : 0;
    for (int64_t q = t0; q < nquads; q += nt) {
        const int64_t blk = q >> 4;
        if (act[blk] == 0u) continue;   // (nothing of the block is read, its rgb included)
        if ((q & 15) == 0) nb[blk] += 1u;
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
        const int64_t blk = i >> 6;
        if (act[blk] == 0u) continue;
        if ((i & 63) == 0) nb[blk] += 1u;
        v4f p = pm[i];
        float m = m2[i];
        mom_pixel(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], p, m, bs, ALB, ALB ? alb[i] : v4f{0.f, 0.f, 0.f, 0.f});
        pm[i] = p;
        m2[i] = m;
    }
}

__global__ __launch_bounds__(256) void k_ad_hot(const v4f* __restrict__ pm, const float* __restrict__ m2,
                                                 const uint32_t* __restrict__ nb, uint8_t* __restrict__ hot, int64_t npix,
                                                 float tau, float floor_, uint32_t min_batches) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const uint32_t n = nb[i >> 6];
        uint8_t h = 1;
        if (n >= min_batches) {
            const float nbf = (float)n;
            const float mean = div_cr(reinterpret_cast<const float*>(pm)[4 * i + 3], nbf);
            const float ex2 = div_cr(m2[i], nbf);
            const float vm = div_cr(gmax(0.0f, ex2 - mean * mean), nbf - 1.0f);
            const float e = div_cr(sqrt_cr(vm), mean + floor_);
            h = e > tau ? 1 : 0;   // (a NaN is not hot)
        }
        hot[i] = h;
    }
}

// One wave per block, lane = pixel: the OR of the hot bytes in the pixel's (2r + 1)^2 box, clipped to
// the image, then the wave's ballot.  slots[workgroup] = the active blocks its waves found.
__global__ __launch_bounds__(256) void k_ad_dilate(const uint8_t* __restrict__ hot, uint32_t* __restrict__ act,
                                                    uint32_t* __restrict__ slots, int W, int H, int64_t npix, int64_t nblk,
                                                    int r) {
    __shared__ uint32_t s_cnt[4];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    uint32_t cnt = 0;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < nblk; b += (int64_t)gridDim.x * 4) {
        const int64_t i = b * 64 + lane;
        uint32_t any = 0;
        if (i < npix) {
            const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
            for (int dy = -r; dy <= r; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= H) continue;
                for (int dx = -r; dx <= r; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= W) continue;
                    any |= hot[(int64_t)yy * W + xx];
                }
            }
        }
        const uint32_t on = __ballot(any != 0u) != 0ull ? 1u : 0u;
        if (lane == 0) act[b] = on;
        cnt += on;
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) slots[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

__global__ __launch_bounds__(256) void k_ad_apply(const uint32_t* __restrict__ act, const uint32_t* __restrict__ in,
                                                   uint32_t* __restrict__ out, int64_t nblk) {
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < nblk; b += (int64_t)gridDim.x * 256)
        out[b] = act[b] ? in[b] : 0u;
}

// scale: pt_moments_variance's (nf * bs) / ((nf - 1) * samples) with samples = nf * bs
__global__ __launch_bounds__(256) void k_ad_resolve(const float* __restrict__ rgb, const v4f* __restrict__ pm,
                                                     const float* __restrict__ m2, const uint32_t* __restrict__ nb,
                                                     float* __restrict__ out_rgb, float* __restrict__ out_var, int64_t npix,
                                                     float bs) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const uint32_t n = nb[i >> 6];
        const float nf = (float)n;
        const float ns = nf * bs;
        if (out_rgb) {
            f3 c = F3(0.0f, 0.0f, 0.0f);
            if (n != 0u) c = F3(div_cr(rgb[3 * i], ns), div_cr(rgb[3 * i + 1], ns), div_cr(rgb[3 * i + 2], ns));
            out_rgb[3 * i] = c.x;
            out_rgb[3 * i + 1] = c.y;
            out_rgb[3 * i + 2] = c.z;
        }
        if (out_var) {
            float v = 0.0f;
            if (n >= 2u) {
                const float scale = div_cr(ns, (nf - 1.0f) * ns);
                const float mean = div_cr(reinterpret_cast<const float*>(pm)[4 * i + 3], nf);
                const float ex2 = div_cr(m2[i], nf);
                v = gmax(0.0f, ex2 - mean * mean) * scale;
            }
            out_var[i] = v;
        }
    }
}

#define AD_TRY(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return pt::fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

int lin_grid_of(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 65536); }

}  // namespace

struct pt_adaptive {
    int32_t W = 0, H = 0;
    int64_t npix = 0, nblk = 0;
    v4f* pm = nullptr;         // (prev.rgb, m1)
    float* m2 = nullptr;
    uint32_t* nb = nullptr;    // nblk batch counts | nblk act words | kDilateGrid count slots
    uint32_t* act = nullptr;
    uint32_t* slots = nullptr;
    uint8_t* hot = nullptr;
    int32_t updates = 0;       // since the last reset
    float batch_samples = 0.0f;
    hipEvent_t ev = nullptr;   // after the last queued work (the synchronous calls wait for it)
    bool ev_recorded = false;
};

namespace pt {
int adaptive_params_check(const pt_adaptive_params* p) {
    if (!p) return fail(PT_ERR_ARG, "null adaptive parameters");
    if (!std::isfinite(p->threshold) || p->threshold < 0.0f) return fail(PT_ERR_ARG, "adaptive threshold must be finite and >= 0");
    if (!std::isfinite(p->floor) || !(p->floor > 0.0f)) return fail(PT_ERR_ARG, "adaptive floor must be finite and > 0");
    if (p->min_batches < 2) return fail(PT_ERR_ARG, "adaptive min_batches must be >= 2");
    if (p->dilate < 0 || p->dilate > 2) return fail(PT_ERR_ARG, "adaptive dilate must be in 0..2");
    return PT_OK;
}
int adaptive_update_check(const pt_adaptive* a, float batch_samples) {
    if (!a) return fail(PT_ERR_ARG, "null adaptive object");
    if (!std::isfinite(batch_samples) || !(batch_samples > 0.0f))
        return fail(PT_ERR_ARG, "batch_samples must be finite and > 0");
    if (a->updates > 0 && batch_samples != a->batch_samples)
        return fail(PT_ERR_ARG, "batch_samples differs from the first update's since the last reset");
    return PT_OK;
}
}  // namespace pt

namespace {
int ad_mark(pt_adaptive* a, hipStream_t st) {
    AD_TRY(hipEventRecord(a->ev, st));
    a->ev_recorded = true;
    return PT_OK;
}
void ad_free(pt_adaptive* a) {
    if (a->pm) (void)hipFree(a->pm);
    if (a->m2) (void)hipFree(a->m2);
    if (a->nb) (void)hipFree(a->nb);
    if (a->hot) (void)hipFree(a->hot);
    a->pm = nullptr;
    a->m2 = nullptr;
    a->nb = a->act = a->slots = nullptr;
    a->hot = nullptr;
}
// The device side of the object, allocated at its first use; `reset`: in the state of a reset without
// a base, on `st`.
int ad_planes(pt_adaptive* a, hipStream_t st, bool reset) {
    if (a->pm) return PT_OK;
    // (m2 is read in 16-byte vectors: the allocation is a whole number of them)
    if (hipMalloc((void**)&a->pm, (size_t)a->npix * sizeof(v4f)) != hipSuccess ||
        hipMalloc((void**)&a->m2, (size_t)((a->npix + 3) / 4) * sizeof(v4f)) != hipSuccess ||
        hipMalloc((void**)&a->nb, (size_t)(2 * a->nblk + kDilateGrid) * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void**)&a->hot, (size_t)a->npix) != hipSuccess ||
        (!a->ev && hipEventCreateWithFlags(&a->ev, hipEventDisableTiming) != hipSuccess)) {
        ad_free(a);
        (void)hipGetLastError();
        return pt::fail(PT_ERR_NOMEM, "hipMalloc (adaptive planes)");
    }
    a->act = a->nb + a->nblk;
    a->slots = a->act + a->nblk;
    if (reset) {
        hipLaunchKernelGGL(k_ad_reset, dim3(lin_grid_of(a->npix)), dim3(256), 0, st, (const float*)nullptr, a->pm, a->m2, a->nb,
                           a->act, a->hot, a->npix);
        AD_TRY(hipGetLastError());
    }
    return PT_OK;
}
}  // namespace

extern "C" {

void pt_adaptive_params_default(pt_adaptive_params* p) {
    if (!p) return;
    *p = pt_adaptive_params{};
    p->threshold = 0.4f;   // the minimiser of scripts/adaptive_tune.py's grid
    p->floor = 0.1f;
    p->min_batches = 4;
    p->dilate = 0;
}

int pt_adaptive_obj_create(int32_t width, int32_t height, pt_adaptive** out) {
    if (!out || width < 1 || height < 1 || (int64_t)width * height > kMaxPixels)
        return pt::fail(PT_ERR_ARG, "bad adaptive size");
    pt_adaptive* a = new pt_adaptive;   // (the planes come with the first use: ad_planes)
    a->W = width;
    a->H = height;
    a->npix = (int64_t)width * height;
    a->nblk = (a->npix + 63) / 64;
    *out = a;
    return PT_OK;
}

int pt_adaptive_obj_destroy(pt_adaptive* a) {
    if (!a) return PT_OK;
    if (a->ev_recorded) (void)hipEventSynchronize(a->ev);
    if (a->ev) (void)hipEventDestroy(a->ev);
    ad_free(a);
    delete a;
    return PT_OK;
}

int pt_adaptive_obj_info(const pt_adaptive* a, int32_t* blocks, int32_t* updates, float* batch_samples) {
    if (!a) return pt::fail(PT_ERR_ARG, "null adaptive object");
    if (blocks) *blocks = (int32_t)a->nblk;
    if (updates) *updates = a->updates;
    if (batch_samples) *batch_samples = a->batch_samples;
    return PT_OK;
}

int pt_adaptive_obj_reset(pt_adaptive* a, const float* d_base_rgb, void* stream) {
    if (!a) return pt::fail(PT_ERR_ARG, "null adaptive object");
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ad_planes(a, st, false)) return rc;
    hipLaunchKernelGGL(k_ad_reset, dim3(lin_grid_of(a->npix)), dim3(256), 0, st, d_base_rgb, a->pm, a->m2, a->nb, a->act,
                       a->hot, a->npix);
    AD_TRY(hipGetLastError());
    a->updates = 0;
    a->batch_samples = 0.0f;
    return ad_mark(a, st);
}

int pt_adaptive_obj_update(pt_adaptive* a, const float* d_rgb, float batch_samples, const float* d_alb, void* stream) {
    if (!a || !d_rgb) return pt::fail(PT_ERR_ARG, "null argument");
    if (int rc = pt::adaptive_update_check(a, batch_samples)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ad_planes(a, st, true)) return rc;
    const bool quad = (reinterpret_cast<uintptr_t>(d_rgb) & 15u) == 0;
    const int64_t lanes = quad ? (a->npix + 3) / 4 : a->npix;
    auto kern = quad ? (d_alb ? k_ad_update<true, true> : k_ad_update<true, false>)
                     : (d_alb ? k_ad_update<false, true> : k_ad_update<false, false>);
    hipLaunchKernelGGL(kern, dim3(lin_grid_of(lanes)), dim3(256), 0, st, d_rgb, (const v4f*)d_alb, a->pm, a->m2, a->nb,
                       (const uint32_t*)a->act, a->npix, batch_samples);
    AD_TRY(hipGetLastError());
    a->updates += 1;
    a->batch_samples = batch_samples;
    return ad_mark(a, st);
}

int pt_adaptive_obj_select(pt_adaptive* a, const pt_adaptive_params* p, void* stream, int32_t* active_blocks,
                           int32_t* blocks) {
    if (!a) return pt::fail(PT_ERR_ARG, "null adaptive object");
    if (int rc = pt::adaptive_params_check(p)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ad_planes(a, st, true)) return rc;
    hipLaunchKernelGGL(k_ad_hot, dim3(lin_grid_of(a->npix)), dim3(256), 0, st, (const v4f*)a->pm, (const float*)a->m2,
                       (const uint32_t*)a->nb, a->hot, a->npix, p->threshold, p->floor, (uint32_t)p->min_batches);
    AD_TRY(hipGetLastError());
    const int grid = (int)std::min<int64_t>((a->nblk + 3) / 4, kDilateGrid);
    hipLaunchKernelGGL(k_ad_dilate, dim3(grid), dim3(256), 0, st, (const uint8_t*)a->hot, a->act, a->slots, a->W, a->H,
                       a->npix, a->nblk, p->dilate);
    AD_TRY(hipGetLastError());
    if (int rc = ad_mark(a, st)) return rc;
    if (blocks) *blocks = (int32_t)a->nblk;
    if (active_blocks) {
        std::vector<uint32_t> s((size_t)grid);
        AD_TRY(hipMemcpyAsync(s.data(), a->slots, s.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        AD_TRY(hipStreamSynchronize(st));
        int64_t n = 0;
        for (uint32_t v : s) n += v;
        *active_blocks = (int32_t)n;
    }
    return PT_OK;
}

int pt_adaptive_obj_set_mask(pt_adaptive* a, const uint8_t* host_mask, int32_t nblocks, void* stream) {
    if (!a || !host_mask) return pt::fail(PT_ERR_ARG, "null argument");
    if ((int64_t)nblocks != a->nblk) return pt::fail(PT_ERR_ARG, "the mask length differs from the number of blocks");
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ad_planes(a, st, true)) return rc;
    std::vector<uint32_t> w((size_t)a->nblk);
    for (size_t b = 0; b < w.size(); ++b) w[b] = host_mask[b] ? 1u : 0u;
    AD_TRY(hipMemcpyAsync(a->act, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    AD_TRY(hipStreamSynchronize(st));
    return ad_mark(a, st);
}

int pt_adaptive_obj_apply(pt_adaptive* a, const uint32_t* d_cmask_in, uint32_t* d_cmask_out, void* stream) {
    if (!a || !d_cmask_in || !d_cmask_out) return pt::fail(PT_ERR_ARG, "null argument");
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ad_planes(a, st, true)) return rc;
    hipLaunchKernelGGL(k_ad_apply, dim3(lin_grid_of(a->nblk)), dim3(256), 0, st, (const uint32_t*)a->act, d_cmask_in,
                       d_cmask_out, a->nblk);
    AD_TRY(hipGetLastError());
    return ad_mark(a, st);
}

int pt_adaptive_obj_resolve(pt_adaptive* a, const float* d_rgb, float* d_out_rgb, float* d_out_var, void* stream) {
    if (!a || !d_rgb || (!d_out_rgb && !d_out_var)) return pt::fail(PT_ERR_ARG, "null argument");
    if (d_out_rgb == d_rgb || (const float*)d_out_var == d_rgb || (d_out_rgb && d_out_rgb == d_out_var))
        return pt::fail(PT_ERR_ARG, "the outputs must not alias the input");
    if (a->updates < 1) return pt::fail(PT_ERR_ARG, "resolve needs an update (the batch size is not known)");
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ad_planes(a, st, true)) return rc;
    hipLaunchKernelGGL(k_ad_resolve, dim3(lin_grid_of(a->npix)), dim3(256), 0, st, d_rgb, (const v4f*)a->pm,
                       (const float*)a->m2, (const uint32_t*)a->nb, d_out_rgb, d_out_var, a->npix, a->batch_samples);
    AD_TRY(hipGetLastError());
    return ad_mark(a, st);
}

int pt_adaptive_obj_get(pt_adaptive* a, float* h_m1, float* h_m2, float* h_prev_rgb, uint32_t* h_nb, uint32_t* h_act,
                        uint8_t* h_hot) {
    if (!a) return pt::fail(PT_ERR_ARG, "null adaptive object");
    if (int rc = ad_planes(a, nullptr, true)) return rc;
    if (a->ev_recorded) AD_TRY(hipEventSynchronize(a->ev));
    else AD_TRY(hipStreamSynchronize(nullptr));
    const size_t n = (size_t)a->npix, nb = (size_t)a->nblk;
    if (h_m2) AD_TRY(hipMemcpy(h_m2, a->m2, n * sizeof(float), hipMemcpyDeviceToHost));
    if (h_nb) AD_TRY(hipMemcpy(h_nb, a->nb, nb * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (h_act) AD_TRY(hipMemcpy(h_act, a->act, nb * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (h_hot) AD_TRY(hipMemcpy(h_hot, a->hot, n, hipMemcpyDeviceToHost));
    if (h_m1 || h_prev_rgb) {
        std::vector<float> pm(4 * n);
        AD_TRY(hipMemcpy(pm.data(), a->pm, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (h_m1) h_m1[i] = pm[4 * i + 3];
            for (int k = 0; k < 3 && h_prev_rgb; ++k) h_prev_rgb[3 * i + k] = pm[4 * i + k];
        }
    }
    return PT_OK;
}

}  // extern "C"
