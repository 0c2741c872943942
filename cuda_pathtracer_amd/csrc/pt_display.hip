// Display transform on the device (pt_display), gfx950: the float accumulator to display bytes
// through a metered or manual exposure, a tone curve and a transfer function.  The bytes are an exact function of
// the input floats: every operation is an integer operation, a float comparison, or one of + - * / on floats (this
// unit is built with the flags of every other unit: no fast-math, no contraction), so tests/display_ref.py restates
// it in numpy and compares with ==.
//
// Metering.  L = (0.2126f r + 0.7152f g) + 0.0722f b of rgb / samples (pt_moments' luminance); a pixel counts iff L
// is finite and >= 2^-16, in bin min(255, (bits(L) - 0x37800000) >> 20): 256 bins of 1/8 octave.  Everything else
// (zeros, denormals, negatives, NaN, infinities) goes to the uncounted bin 256.
//   k_display_meter    a lane takes four pixels (48 contiguous bytes as three 16-byte loads); a workgroup keeps one
//                      private histogram per wave in LDS, filled with per-lane LDS atomics.  A one-colour image
//                      sends all 64 lanes of every atomic to one address; measured (profiles/display_time.txt) it
//                      takes the time of a Cornell frame, 0.044 ms at 3840 x 2160 for both, so same-address LDS
//                      atomics without a return value do not serialise badly here.  Combining equal bins within
//                      the wave first (PT_DISPLAY_PEEL rounds of: the bin of the first pending lane, one ballot
//                      for every lane with that bin, one lane adds their count) was measured at 1, 2 and 4 rounds
//                      and costs more than it saves: 0.058, 0.059 - 0.064 and 0.059 - 0.071 ms.  So the product
//                      combines nothing.  At the end the workgroup sums its four histograms and adds every
//                      non-empty bin to the object's histogram with one vector atomic each.
//   k_display_resolve  one wave, integers only (its own launch: no workgroup waits for another): the trimmed mean
//                      bin of the ranks [a, b), the target exposure, the adaptation step of the state `e` (units of
//                      1/256 octave), the multiplier ldexpf(P[e & 255], e >> 8).  It leaves the histogram in `last`
//                      (pt_display_info) and zeroes it for the next metering.
// Applying.
//   k_display_apply    a lane takes four consecutive output pixels and stores them as one 12- or 16-byte word;
//                      c = (v / samples) * mult, c > 0 ? c : 0, c < 65504 ? c : 65504, the curve, the clamp to
//                      [0, 1], then (uint8_t)(c * 255.f) or, for sRGB, the count of thresholds T[1..255] not above
//                      c by a binary search: three steps against registers, five in the table in LDS.
// No kernel waits for another workgroup; the grid is at most kGrid workgroups, which stride over the image.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "pt_enc.h"

using namespace pt;

namespace {

#ifndef PT_DISPLAY_PEEL
#define PT_DISPLAY_PEEL 0   // bins a wave combines by ballot before its LDS atomics (scripts/display_time.py measured 0, 1, 2, 4)
#endif
constexpr int kGrid = 256;        // workgroups at most: one sweep of a grid is kGrid * 256 * 4 pixels
constexpr int kBins = 257;        // 256 counted bins and the uncounted one
constexpr int kHistPad = 320;     // words of a histogram in device memory
constexpr uint32_t kLumMin = 0x37800000u, kInfBits = 0x7f800000u;   // 2^-16, +inf

typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
struct __attribute__((aligned(4))) U3 { uint32_t a, b, c; };

struct State {      // on the device
    int32_t e;      // the exposure in 1/256 octave
    int32_t has;    // a metering has set it since create / reset
    float mult;     // ldexpf(P[e & 255], e >> 8)
    int32_t pad;
};

struct ResolveK {
    int32_t lo, hi, rate, GC, emin, emax;   // GC: G + C
};

struct ApplyK {
    int32_t W, H, mirror, stride, curve, transfer, automatic, vec_in, word_out;
    float exposure, ww, hable_div;
};

// ---- the curves (host and device: the host evaluates hable_f(11.2f) once) -----------------------------------
__host__ __device__ inline float hable_f(float x) {
    const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
    return (x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F) - E / F;
}

__device__ __forceinline__ float curve_of(float c, const ApplyK& k) {
    switch (k.curve) {
    case PT_DISPLAY_REINHARD: return (c * (1.0f + c / k.ww)) / (1.0f + c);
    case PT_DISPLAY_ACES: return (c * (2.51f * c + 0.03f)) / (c * (2.43f * c + 0.59f) + 0.14f);
    case PT_DISPLAY_HABLE: return hable_f(2.0f * c) / k.hable_div;
    default: return c;
    }
}

// T[32], T[64] .. T[224]: the thresholds of the search's first three steps, wave-uniform, read once per lane
struct TopT { float t[7]; };

__device__ __forceinline__ uint32_t byte_of(float v, float n, float mult, const ApplyK& k, const float* sT, const TopT& top) {
    float c = (v / n) * mult;
    c = c > 0.0f ? c : 0.0f;   // (NaN and negatives to 0)
    c = c < 65504.0f ? c : 65504.0f;
    c = curve_of(c, k);
    c = c > 0.0f ? c : 0.0f;
    c = c < 1.0f ? c : 1.0f;
    if (k.transfer == PT_DISPLAY_LINEAR) return (uint32_t)(uint8_t)(c * 255.f);
    // T is strictly increasing: pos becomes #{b in 1..255 : T[b] <= c}.  Steps 128, 64 and 32 compare with registers
    // (top.t[j] = T[32 (j + 1)]), the other five read the table in LDS.
    int pos = top.t[3] <= c ? 128 : 0;
    pos += (pos ? top.t[5] : top.t[1]) <= c ? 64 : 0;
    const float a = pos & 128 ? top.t[4] : top.t[0], b = pos & 128 ? top.t[6] : top.t[2];
    pos += (pos & 64 ? b : a) <= c ? 32 : 0;
#pragma unroll
    for (int step = 16; step; step >>= 1)
        if (sT[pos + step] <= c) pos += step;   // (pos + step <= 255)
    return (uint32_t)pos;
}

__device__ __forceinline__ int lum_bin(float r, float g, float b, float n) {
    const float L = (0.2126f * (r / n) + 0.7152f * (g / n)) + 0.0722f * (b / n);
    const uint32_t u = __float_as_uint(L);
    if (u < kLumMin || u >= kInfBits) return 256;   // (the sign bit makes every negative larger than both)
    return min(255, (int)((u - kLumMin) >> 20));
}

// The flat pixels 4 g .. 4 g + 3 of the accumulator (cnt of them exist) into v[12].
__device__ __forceinline__ void load_group(const float* __restrict__ rgb, long long g, int cnt, bool vec, float v[12]) {
    const float* p = rgb + 12 * g;
    if (vec && cnt == 4) {
        const f4 a = *reinterpret_cast<const f4*>(p), b = *reinterpret_cast<const f4*>(p + 4), c = *reinterpret_cast<const f4*>(p + 8);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = j < 3 * cnt ? p[j] : 0.0f;
    }
}

// One count per lane with `on` into the wave's histogram h (every lane of the wave calls it).
__device__ __forceinline__ void wave_count(uint32_t* h, int bin, bool on, int lane) {
    unsigned long long todo = __ballot(on);
#pragma unroll
    for (int round = 0; round < PT_DISPLAY_PEEL; ++round) {
        if (!todo) break;   // (wave-uniform)
        const int lead = __shfl(bin, __ffsll((long long)todo) - 1, 64);
        const unsigned long long m = __ballot(on && bin == lead) & todo;
        if (lane == __ffsll((long long)m) - 1) atomicAdd(&h[lead], (uint32_t)__popcll(m));
        todo &= ~m;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&h[bin], 1u);
}

__global__ __launch_bounds__(256) void k_display_meter(const float* __restrict__ rgb, float n, long long npix, int vec,
                                                       uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[4][kBins];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    for (int k = (int)threadIdx.x; k < 4 * kBins; k += 256) (&s_h[0][0])[k] = 0u;
    __syncthreads();
    const long long groups = (npix + 3) / 4;
    // (the bound is the wave's, so that every lane of a wave reaches the ballots)
    for (long long base = ((long long)blockIdx.x * 4 + wave) * 64; base < groups; base += (long long)gridDim.x * 256) {
        const long long g = base + lane;
        const int cnt = g < groups ? (int)min(4LL, npix - 4 * g) : 0;
        float v[12];
        if (cnt) load_group(rgb, g, cnt, vec != 0, v);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool on = q < cnt;
            const int bin = on ? lum_bin(v[3 * q], v[3 * q + 1], v[3 * q + 2], n) : 256;
            wave_count(s_h[wave], bin, on, lane);
        }
    }
    __syncthreads();
    for (int k = (int)threadIdx.x; k < kBins; k += 256) {
        const uint32_t s = s_h[0][k] + s_h[1][k] + s_h[2][k] + s_h[3][k];
        if (s) atomicAdd(&hist[k], s);
    }
}

__global__ __launch_bounds__(64) void k_display_resolve(uint32_t* __restrict__ hist, uint32_t* __restrict__ last,
                                                        State* __restrict__ st, const float* __restrict__ P, ResolveK k) {
    const int lane = (int)threadIdx.x;
    uint32_t c[4];
    long long own = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = hist[4 * lane + j];
        own += c[j];
    }
    long long inc = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    const long long N = __shfl(inc, 63, 64);
    const long long a = (N * k.lo) >> 10, b = (N * k.hi + 1023) >> 10, M = b - a;
    long long run = inc - own, S = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long lo = max(a, run), hi = min(b, run + (long long)c[j]);
        if (hi > lo) S += (long long)(4 * lane + j) * (hi - lo);
        run += c[j];
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) S += __shfl_xor(S, d, 64);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        last[4 * lane + j] = c[j];
        hist[4 * lane + j] = 0u;
    }
    if (lane == 0) {
        last[256] = hist[256];
        hist[256] = 0u;
        if (N > 0) {
            const long long m = (32 * S + M / 2) / M + 16, K = m - 4096;
            long long t = (long long)k.GC - K;
            t = t < k.emin ? k.emin : (t > k.emax ? k.emax : t);
            int32_t e = st->e;
            if (!st->has) {
                e = (int32_t)t;
            } else if (t != e) {
                const long long d = t - e, ad = d < 0 ? -d : d, step = max(1LL, (ad * k.rate) >> 8);
                e += (int32_t)(d < 0 ? -step : step);
            }
            st->e = e;
            st->has = 1;
            // ldexpf(P[e & 255], e >> 8): |e >> 8| <= 64 (the ev limits), so 2^(e >> 8) is a normal float and the
            // product with P in [1, 2) is exact
            st->mult = P[e & 255] * __uint_as_float((uint32_t)((e >> 8) + 127) << 23);
        }
    }
}

__global__ void k_display_reset(State* st) {
    st->e = 0;
    st->has = 0;
    st->mult = 1.0f;
}

__global__ __launch_bounds__(256) void k_display_apply(const float* __restrict__ rgb, float n, ApplyK k, const State* __restrict__ st,
                                                       const float* __restrict__ T, uint8_t* __restrict__ pix) {
    __shared__ float s_T[256];
    TopT top{};
    if (k.transfer == PT_DISPLAY_SRGB) {
        s_T[threadIdx.x] = T[threadIdx.x];
#pragma unroll
        for (int j = 0; j < 7; ++j) top.t[j] = T[32 * (j + 1)];
        __syncthreads();
    }
    const float mult = k.automatic ? st->mult : k.exposure;
    const long long npix = (long long)k.W * k.H, groups = (npix + 3) / 4;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const int cnt = (int)min(4LL, npix - 4 * g);
        float v[12];
        bool rev = false;   // v holds the output pixels 3 .. 0
        if (!k.mirror) {
            load_group(rgb, g, cnt, k.vec_in != 0, v);
        } else if (k.vec_in && (k.W & 3) == 0) {   // a group lies inside one row, and so do its four input pixels
            const long long y = (4 * g) / k.W, X0 = 4 * g - y * k.W;
            load_group(rgb, (y * k.W + (k.W - 4 - X0)) / 4, 4, true, v);
            rev = true;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long o = min(4 * g + q, npix - 1), y = o / k.W, X = o - y * k.W;
                const float* p = rgb + 3 * (y * k.W + (k.W - 1 - X));
                v[3 * q] = p[0];
                v[3 * q + 1] = p[1];
                v[3 * q + 2] = p[2];
            }
        }
        uint32_t px[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int s = rev ? 3 - q : q;
            px[q] = byte_of(v[3 * s], n, mult, k, s_T, top) | (byte_of(v[3 * s + 1], n, mult, k, s_T, top) << 8) |
                    (byte_of(v[3 * s + 2], n, mult, k, s_T, top) << 16);
        }
        uint8_t* o = pix + 4 * g * k.stride;
        if (cnt == 4 && k.word_out) {
            if (k.stride == 4) {
                u4 w = {px[0], px[1], px[2], px[3]};
                *reinterpret_cast<u4*>(o) = w;
            } else {
                U3 w = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
                *reinterpret_cast<U3*>(o) = w;
            }
        } else {
            for (int q = 0; q < cnt; ++q)
                for (int j = 0; j < k.stride; ++j) o[q * k.stride + j] = (uint8_t)(px[q] >> (8 * j));
        }
    }
}

#define DISP_TRY(expr)                                                                  \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess)                                                           \
            return fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

double srgb_eotf(double x) { return x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4); }

long long round_half_up(double v) { return (long long)std::floor(v + 0.5); }

}  // namespace

struct pt_display {
    int32_t W = 0, H = 0;
    pt_display_params prm{};
    ResolveK rk{};
    float ww = 1.0f, hable_div = 1.0f;
    float T[256], P[256];
    // The device side, one allocation made at first use: T | P | state | histogram | the histogram as last resolved
    uint8_t* dev = nullptr;
    float *d_T = nullptr, *d_P = nullptr;
    State* d_state = nullptr;
    uint32_t *d_hist = nullptr, *d_last = nullptr;
    hipEvent_t ev = nullptr;   // after the last queued work (the destructor and pt_display_info wait for it)
    bool ev_recorded = false;
    ~pt_display() {
        if (ev_recorded) (void)hipEventSynchronize(ev);
        if (ev) (void)hipEventDestroy(ev);
        if (dev) (void)hipFree(dev);
    }
};

int pt::display_size(const pt_display* d, int32_t* width, int32_t* height, int32_t* automatic) {
    if (!d) return fail(PT_ERR_ARG, "null display transform");
    *width = d->W;
    *height = d->H;
    *automatic = d->prm.exposure_mode == PT_DISPLAY_AUTO;
    return PT_OK;
}

namespace {

int params_check(const pt_display_params* p) {
    auto finite = [](float v) { return std::isfinite(v); };
    for (int32_t r : p->reserved)
        if (r != 0) return fail(PT_ERR_ARG, "pt_display_params.reserved must be zero");
    if (p->exposure_mode != PT_DISPLAY_MANUAL && p->exposure_mode != PT_DISPLAY_AUTO)
        return fail(PT_ERR_ARG, "unknown exposure_mode");
    if (!finite(p->exposure) || !(p->exposure > 0.0f)) return fail(PT_ERR_ARG, "exposure must be finite and > 0");
    if (!finite(p->key_value) || !(p->key_value > 0.0f)) return fail(PT_ERR_ARG, "key_value must be finite and > 0");
    if (!finite(p->compensation_ev) || std::fabs(p->compensation_ev) > 64.0f)
        return fail(PT_ERR_ARG, "compensation_ev must lie in -64 .. 64");
    if (!finite(p->min_ev) || !finite(p->max_ev) || p->min_ev < -64.0f || p->max_ev > 64.0f || p->min_ev > p->max_ev)
        return fail(PT_ERR_ARG, "the ev limits must satisfy -64 <= min_ev <= max_ev <= 64");
    if (p->pct_lo < 0 || p->pct_lo >= p->pct_hi || p->pct_hi > 1024)
        return fail(PT_ERR_ARG, "the percentiles must satisfy 0 <= pct_lo < pct_hi <= 1024");
    if (p->rate < 1 || p->rate > 256) return fail(PT_ERR_ARG, "rate must lie in 1 .. 256");
    if (p->curve < PT_DISPLAY_NONE || p->curve > PT_DISPLAY_HABLE) return fail(PT_ERR_ARG, "unknown curve");
    if (!finite(p->white) || !(p->white > 0.0f)) return fail(PT_ERR_ARG, "white must be finite and > 0");
    if (p->transfer != PT_DISPLAY_LINEAR && p->transfer != PT_DISPLAY_SRGB) return fail(PT_ERR_ARG, "unknown transfer");
    return PT_OK;
}

int samples_check(float samples) {
    if (!std::isfinite(samples) || !(samples > 0.0f)) return fail(PT_ERR_ARG, "samples must be finite and > 0");
    return PT_OK;
}

int disp_alloc(pt_display* d) {
    if (d->dev) return PT_OK;
    const size_t o_P = align256(sizeof d->T), o_state = o_P + align256(sizeof d->P), o_hist = o_state + 256,
                 o_last = o_hist + align256(kHistPad * 4), total = o_last + align256(kHistPad * 4);
    std::vector<uint8_t> init(total, 0);
    std::memcpy(init.data(), d->T, sizeof d->T);
    std::memcpy(init.data() + o_P, d->P, sizeof d->P);
    const State s0{0, 0, 1.0f, 0};
    std::memcpy(init.data() + o_state, &s0, sizeof s0);
    if (hipMalloc((void**)&d->dev, total) != hipSuccess ||
        (!d->ev && hipEventCreateWithFlags(&d->ev, hipEventDisableTiming) != hipSuccess)) {
        if (d->dev) (void)hipFree(d->dev);
        d->dev = nullptr;
        (void)hipGetLastError();
        return fail(PT_ERR_NOMEM, "hipMalloc (display transform scratch)");
    }
    // synchronous, once per object: a later call on any stream reads it
    const hipError_t he = hipMemcpy(d->dev, init.data(), total, hipMemcpyHostToDevice);
    if (he != hipSuccess) {
        (void)hipFree(d->dev);
        d->dev = nullptr;
        return fail(PT_ERR_HIP, std::string("hipMemcpy (display transform tables): ") + hipGetErrorString(he));
    }
    d->d_T = (float*)d->dev;
    d->d_P = (float*)(d->dev + o_P);
    d->d_state = (State*)(d->dev + o_state);
    d->d_hist = (uint32_t*)(d->dev + o_hist);
    d->d_last = (uint32_t*)(d->dev + o_last);
    return PT_OK;
}

int disp_done(pt_display* d, hipStream_t st) {
    DISP_TRY(hipGetLastError());
    DISP_TRY(hipEventRecord(d->ev, st));
    d->ev_recorded = true;
    return PT_OK;
}

int meter(pt_display* d, const float* d_rgb, float samples, hipStream_t st) {
    const long long npix = (long long)d->W * d->H;
    const int vec = ((uintptr_t)d_rgb & 15) == 0;
    hipLaunchKernelGGL(k_display_meter, dim3(std::min(grid_of((npix + 3) / 4, 256), kGrid)), dim3(256), 0, st, d_rgb, samples,
                       npix, vec, d->d_hist);
    hipLaunchKernelGGL(k_display_resolve, dim3(1), dim3(64), 0, st, d->d_hist, d->d_last, d->d_state, (const float*)d->d_P, d->rk);
    return PT_OK;
}

int apply(pt_display* d, const float* d_rgb, float samples, uint8_t* d_pix, int32_t stride, hipStream_t st) {
    const pt_display_params& p = d->prm;
    const long long npix = (long long)d->W * d->H;
    ApplyK k{};
    k.W = d->W;
    k.H = d->H;
    k.mirror = p.mirror_x ? 1 : 0;
    k.stride = stride;
    k.curve = p.curve;
    k.transfer = p.transfer;
    k.automatic = p.exposure_mode == PT_DISPLAY_AUTO;
    k.vec_in = ((uintptr_t)d_rgb & 15) == 0;
    k.word_out = ((uintptr_t)d_pix & (stride == 4 ? 15 : 3)) == 0;
    k.exposure = p.exposure;
    k.ww = d->ww;
    k.hable_div = d->hable_div;
    hipLaunchKernelGGL(k_display_apply, dim3(std::min(grid_of((npix + 3) / 4, 256), kGrid)), dim3(256), 0, st, d_rgb, samples, k,
                       (const State*)d->d_state, (const float*)d->d_T, d_pix);
    return PT_OK;
}

int apply_check(const pt_display* d, const float* d_rgb, float samples, const uint8_t* d_pix, int32_t stride) {
    if (!d || !d_rgb || !d_pix) return fail(PT_ERR_ARG, "null argument");
    if (stride != 3 && stride != 4) return fail(PT_ERR_ARG, "the pixel stride must be 3 or 4");
    const uintptr_t a = (uintptr_t)d_rgb, b = (uintptr_t)d_pix;
    const uint64_t npix = (uint64_t)d->W * d->H;
    if (a < b + npix * stride && b < a + npix * 12) return fail(PT_ERR_ARG, "d_pix must not alias d_rgb");
    return samples_check(samples);
}

}  // namespace

extern "C" {

void pt_display_params_default(pt_display_params* p) {
    if (!p) return;
    *p = pt_display_params{};
    p->exposure_mode = PT_DISPLAY_MANUAL;
    p->exposure = 1.0f;
    p->key_value = 0.18f;
    p->compensation_ev = 0.0f;
    p->min_ev = -8.0f;
    p->max_ev = 8.0f;
    p->pct_lo = 102;
    p->pct_hi = 922;
    p->rate = 256;
    p->curve = PT_DISPLAY_NONE;
    p->white = 4.0f;
    p->transfer = PT_DISPLAY_LINEAR;
    p->mirror_x = 0;
}

void pt_display_tables(float srgb[256], float pow2[256], float* hable_white) {
    if (srgb) {
        srgb[0] = 0.0f;   // (not a threshold: the count runs over 1..255)
        for (int b = 1; b < 256; ++b) {
            const double t = srgb_eotf((b - 0.5) / 255.0);
            float f = (float)t;
            if ((double)f < t) f = std::nextafterf(f, INFINITY);   // rounded up
            srgb[b] = f;
        }
    }
    if (pow2)
        for (int k = 0; k < 256; ++k) pow2[k] = (float)std::exp2(k / 256.0);
    if (hable_white) *hable_white = hable_f(11.2f);
}

int pt_display_create(int32_t width, int32_t height, const pt_display_params* p, pt_display** out) {
    if (!out || !p) return fail(PT_ERR_ARG, "null argument");
    if (int rc = params_check(p)) return rc;
    if (width < 1 || height < 1) return fail(PT_ERR_ARG, "display width and height must be at least 1");
    if ((int64_t)width * height >= ((int64_t)1 << 31)) return fail(PT_ERR_ARG, "display image too large: width * height must stay below 2^31");
    pt_display* d = new pt_display;   // (the device side comes with the first use: disp_alloc)
    d->W = width;
    d->H = height;
    d->prm = *p;
    pt_display_tables(d->T, d->P, &d->hable_div);
    d->ww = p->white * p->white;
    const long long G = round_half_up(256.0 * std::log2((double)p->key_value)), C = round_half_up(256.0 * (double)p->compensation_ev);
    d->rk = ResolveK{p->pct_lo, p->pct_hi, p->rate, (int32_t)(G + C), (int32_t)round_half_up(256.0 * (double)p->min_ev),
                     (int32_t)round_half_up(256.0 * (double)p->max_ev)};
    *out = d;
    return PT_OK;
}

int pt_display_destroy(pt_display* d) {
    delete d;   // (waits for the last queued work)
    return PT_OK;
}

int pt_display_reset(pt_display* d, void* stream) {
    if (!d) return fail(PT_ERR_ARG, "null display transform");
    if (!d->dev) return PT_OK;   // (nothing metered yet)
    hipLaunchKernelGGL(k_display_reset, dim3(1), dim3(1), 0, (hipStream_t)stream, d->d_state);
    return disp_done(d, (hipStream_t)stream);
}

int pt_display_meter(pt_display* d, const float* d_rgb, float samples, void* stream) {
    if (!d || !d_rgb) return fail(PT_ERR_ARG, "null argument");
    if (int rc = samples_check(samples)) return rc;
    if (int rc = disp_alloc(d)) return rc;
    if (int rc = meter(d, d_rgb, samples, (hipStream_t)stream)) return rc;
    return disp_done(d, (hipStream_t)stream);
}

int pt_display_apply(pt_display* d, const float* d_rgb, float samples, uint8_t* d_pix, int32_t pixel_stride, void* stream) {
    if (int rc = apply_check(d, d_rgb, samples, d_pix, pixel_stride)) return rc;
    if (int rc = disp_alloc(d)) return rc;
    if (int rc = apply(d, d_rgb, samples, d_pix, pixel_stride, (hipStream_t)stream)) return rc;
    return disp_done(d, (hipStream_t)stream);
}

int pt_display_frame(pt_display* d, const float* d_rgb, float samples, uint8_t* d_pix, int32_t pixel_stride, void* stream) {
    if (int rc = apply_check(d, d_rgb, samples, d_pix, pixel_stride)) return rc;
    if (int rc = disp_alloc(d)) return rc;
    if (int rc = meter(d, d_rgb, samples, (hipStream_t)stream)) return rc;
    if (int rc = apply(d, d_rgb, samples, d_pix, pixel_stride, (hipStream_t)stream)) return rc;
    return disp_done(d, (hipStream_t)stream);
}

int pt_display_info(pt_display* d, uint32_t hist[257], int32_t* e, float* mult, int32_t* metered) {
    if (!d) return fail(PT_ERR_ARG, "null display transform");
    State s{0, 0, 1.0f, 0};
    if (hist) std::fill(hist, hist + kBins, 0u);
    if (d->dev) {
        if (d->ev_recorded) DISP_TRY(hipEventSynchronize(d->ev));
        DISP_TRY(hipMemcpy(&s, d->d_state, sizeof s, hipMemcpyDeviceToHost));
        if (hist) DISP_TRY(hipMemcpy(hist, d->d_last, kBins * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (e) *e = s.e;
    if (mult) *mult = d->prm.exposure_mode == PT_DISPLAY_AUTO ? s.mult : d->prm.exposure;
    if (metered) *metered = s.has;
    return PT_OK;
}

int pt_display_host(int32_t width, int32_t height, const float* rgb, float samples, const pt_display_params* p, uint8_t* out,
                    int32_t pixel_stride) {
    if (!rgb || !out) return fail(PT_ERR_ARG, "null argument");
    if (pixel_stride != 3 && pixel_stride != 4) return fail(PT_ERR_ARG, "the pixel stride must be 3 or 4");
    if (int rc = samples_check(samples)) return rc;
    pt_display* d = nullptr;
    if (int rc = pt_display_create(width, height, p, &d)) return rc;
    const size_t in_bytes = (size_t)width * height * 3 * sizeof(float), out_bytes = (size_t)width * height * pixel_stride;
    uint8_t* dev = nullptr;
    const size_t o_out = align256(in_bytes);
    if (hipMalloc((void**)&dev, o_out + out_bytes + 16) != hipSuccess) {
        (void)hipGetLastError();
        delete d;
        return fail(PT_ERR_NOMEM, "hipMalloc (display host transform)");
    }
    hipError_t he = hipMemcpy(dev, rgb, in_bytes, hipMemcpyHostToDevice);
    int rc = PT_OK;
    if (he == hipSuccess)
        rc = p->exposure_mode == PT_DISPLAY_AUTO ? pt_display_frame(d, (const float*)dev, samples, dev + o_out, pixel_stride, nullptr)
                                                 : pt_display_apply(d, (const float*)dev, samples, dev + o_out, pixel_stride, nullptr);
    if (he == hipSuccess && !rc) he = hipMemcpy(out, dev + o_out, out_bytes, hipMemcpyDeviceToHost);   // (waits for the kernels)
    delete d;
    (void)hipFree(dev);
    if (rc) return rc;
    if (he != hipSuccess) return fail(PT_ERR_HIP, std::string("pt_display_host: ") + hipGetErrorString(he));
    return PT_OK;
}

}  // extern "C"
