// Temporal reprojection of the denoiser's history across camera moves (pt_temporal), gfx950.  The exact
// fp32 definition is DESIGN.md §12; tests/temporal_ref.py restates it in numpy float32 and the GPU tests
// compare bit for bit.  The arithmetic rules are pt_denoise.hip's: -ffp-contract=off, every operation
// below is one correctly rounded fp32 operation in the stated order, '/' is div_cr.
//
// The object needs no pt_ctx and outlives any: per pixel it keeps the per-sample mean colour (divided
// by the albedo when demodulating) with the history length h in samples (H0), two weighted means of the
// luminance and its square (H1), the G-buffer of the frame the history belongs to, the accumulator as
// last seen (prev) and that frame's camera.  A frame of the same view integrates in place
// (k_tmp_integrate); a frame of another view looks every pixel's world position up in the old view,
// gathers the four bilinear taps that lie on the same surface and writes the other set of planes
// (k_tmp_reproject).  k_tmp_resolve turns the state into the inputs of pt_denoiser_run_var: the
// remodulated mean and a variance that comes from time where the history is long enough and from the
// 5 x 5 spatial neighbourhood where it is not.  No inter-workgroup waits, no atomics, no LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pt_device.h"
#include "pt_internal.h"

using namespace ptd;

namespace {

constexpr int kTX = 32, kTY = 8, kThreads = kTX * kTY;   // §10's tile: a wave's rows are 512 contiguous bytes
constexpr float kAlbMin = 0x1p-10f;                      // §10's rule: smaller albedo components are not (de)modulated
constexpr int64_t kMaxPixels = (int64_t)1 << 30;
constexpr int32_t kMaxMinFrames = 1 << 20;

__device__ __forceinline__ f3 xyz(v4f v) { return F3(v[0], v[1], v[2]); }
__device__ __forceinline__ float lum(f3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
__device__ __forceinline__ f3 modulate(f3 c, v4f a, bool divide) {
    if (a[0] >= kAlbMin) c.x = divide ? div_cr(c.x, a[0]) : c.x * a[0];
    if (a[1] >= kAlbMin) c.y = divide ? div_cr(c.y, a[1]) : c.y * a[1];
    if (a[2] >= kAlbMin) c.z = divide ? div_cr(c.z, a[2]) : c.z * a[2];
    return c;
}

// The blend of one batch mean c of b samples into a pixel's history.  A pixel without history comes in
// with mean = mu1 = mu2 = h = 0: then a = b / b = 1 and mean = 0 + 1 * (c - 0) = c exactly.
__device__ __forceinline__ void tmp_blend(f3 c, float b, float maxh, f3& mean, float& mu1, float& mu2, float& h) {
    float hn = h + b;
    if (maxh > 0.0f) hn = gmin(hn, maxh);
    const float a = div_cr(b, hn);
    mean = mean + a * (c - mean);
    const float l = lum(c);
    mu1 = mu1 + a * (l - mu1);
    mu2 = mu2 + a * (l * l - mu2);
    h = hn;
}

struct TmpArgs {
    const float* rgb;                 // the accumulator, W * H float3
    const v4f *gA_in, *gB_in, *alb_in; // the new frame's planes (may be the object's own: then not copied)
    const v4f* oH0;                   // the history frame's set
    const v2f* oH1;
    const v4f *ogA, *ogB;
    v4f* nH0;                         // the set this frame writes
    v2f* nH1;
    v4f *ngA, *ngB, *alb;
    float* prev;
    int32_t W, H, demodulate, pad_;
    float samples, b, maxh, min_ndot, plane_tol;
    float pos[3], view[3], right[3], up[3];   // the history frame's camera
    float vv, rr, uu, plx, ply, hw, hh;       // dot(view, view), ..., pixel lengths, W / 2, H / 2
};

// One pixel per lane.  EMPTY: no history anywhere (the first frame): the taps are not looked at.
template <bool EMPTY>
__global__ __launch_bounds__(kThreads) void k_tmp_reproject(const TmpArgs A) {
    const int W = A.W, H = A.H;
    const int x = (int)blockIdx.x * kTX + (int)threadIdx.x % kTX, y = (int)blockIdx.y * kTY + (int)threadIdx.x / kTX;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float r = A.rgb[3 * p], g = A.rgb[3 * p + 1], bl = A.rgb[3 * p + 2];
    const v4f a4 = A.gA_in[p], b4 = A.gB_in[p], al = A.alb_in[p];
    f3 c = F3(div_cr(r, A.samples), div_cr(g, A.samples), div_cr(bl, A.samples));
    if (A.demodulate) c = modulate(c, al, true);
    f3 mean = F3(0.f, 0.f, 0.f);
    float mu1 = 0.0f, mu2 = 0.0f, h = 0.0f;
    const int mat = __float_as_int(a4[3]);
    if (!EMPTY && mat >= 0) {
        const f3 np = xyz(a4), pp = xyz(b4);
        const f3 v = pp - F3(A.pos[0], A.pos[1], A.pos[2]);
        const float z = div_cr(dot(v, F3(A.view[0], A.view[1], A.view[2])), A.vv);
        if (z > 0.0f) {
            const float ax = -div_cr(div_cr(dot(v, F3(A.right[0], A.right[1], A.right[2])), A.rr), A.plx * z);
            const float ay = -div_cr(div_cr(dot(v, F3(A.up[0], A.up[1], A.up[2])), A.uu), A.ply * z);
            const float fx = ax + A.hw, fy = ay + A.hh;
            if (fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H) {   // (else: no tap inside; NaN too)
                const float x0f = floorf(fx), y0f = floorf(fy);
                const int x0 = (int)x0f, y0 = (int)y0f;
                const float tx = fx - x0f, ty = fy - y0f;
                const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty};
                const float tol = A.plane_tol * b4[3];
                f3 sm = F3(0.f, 0.f, 0.f);
                float s1 = 0.0f, s2 = 0.0f, sh = 0.0f, wsum = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {   // (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
                    const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t q = (size_t)qy * W + qx;
                    const v4f aq = A.ogA[q];
                    if (__float_as_int(aq[3]) != mat) continue;
                    if (dot(np, xyz(aq)) < A.min_ndot) continue;
                    const v4f bq = A.ogB[q];
                    if (fabsf(dot(np, xyz(bq) - pp)) > tol) continue;
                    const v4f hq = A.oH0[q];
                    const v2f mq = A.oH1[q];
                    const float w = wx[k & 1] * wy[k >> 1];
                    sm = sm + w * xyz(hq);
                    s1 = s1 + w * mq[0];
                    s2 = s2 + w * mq[1];
                    sh = sh + w * hq[3];
                    wsum = wsum + w;
                }
                if (wsum > 0.0f) {
                    mean = F3(div_cr(sm.x, wsum), div_cr(sm.y, wsum), div_cr(sm.z, wsum));
                    mu1 = div_cr(s1, wsum);
                    mu2 = div_cr(s2, wsum);
                    h = div_cr(sh, wsum);
                }
            }
        }
    }
    tmp_blend(c, A.b, A.maxh, mean, mu1, mu2, h);
    A.nH0[p] = v4f{mean.x, mean.y, mean.z, h};
    A.nH1[p] = v2f{mu1, mu2};
    if (A.gA_in != A.ngA) A.ngA[p] = a4;
    if (A.gB_in != A.ngB) A.ngB[p] = b4;
    if (A.alb_in != A.alb) A.alb[p] = al;
    A.prev[3 * p] = r;
    A.prev[3 * p + 1] = g;
    A.prev[3 * p + 2] = bl;
}

// One same-view update of one pixel, in place: c = (rgb - prev) / b; a miss has no history.
__device__ __forceinline__ void tmp_integrate_pixel(float r, float g, float bl, float& pr, float& pg, float& pb, v4f& h0,
                                                    v2f& h1, int mat, bool use_alb, v4f alb, float b, float maxh) {
    f3 c = F3(div_cr(r - pr, b), div_cr(g - pg, b), div_cr(bl - pb, b));
    if (use_alb) c = modulate(c, alb, true);
    f3 mean = xyz(h0);
    float mu1 = h1[0], mu2 = h1[1], h = h0[3];
    if (mat < 0) {
        mean = F3(0.f, 0.f, 0.f);
        mu1 = mu2 = h = 0.0f;
    }
    tmp_blend(c, b, maxh, mean, mu1, mu2, h);
    h0 = v4f{mean.x, mean.y, mean.z, h};
    h1 = v2f{mu1, mu2};
    pr = r;
    pg = g;
    pb = bl;
}

// QUAD: a lane takes four consecutive pixels, so rgb and prev (3 x 16 B each) and H1 (2 x 16 B) move as
// whole 16-byte vectors like H0 and alb (rgb must be 16-byte aligned); the npix % 4 last pixels, or
// every pixel without QUAD, go one per lane.
template <bool QUAD, bool ALB>
__global__ __launch_bounds__(256) void k_tmp_integrate(const float* __restrict__ rgb, const v4f* __restrict__ gA,
                                                        const v4f* __restrict__ alb, float* __restrict__ prev,
                                                        v4f* __restrict__ H0, v2f* __restrict__ H1, int64_t npix, float b,
                                                        float maxh) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
    const int64_t nquads = QUAD ? npix / 4 : 0;
    const int* mat = reinterpret_cast<const int*>(gA);
    for (int64_t q = t0; q < nquads; q += nt) {
        const v4f* r4 = reinterpret_cast<const v4f*>(rgb) + 3 * q;
        v4f* p4 = reinterpret_cast<v4f*>(prev) + 3 * q;
        v4f* m4 = reinterpret_cast<v4f*>(H1) + 2 * q;
        const v4f ra = r4[0], rb = r4[1], rc = r4[2];
        const v4f pa = p4[0], pb = p4[1], pc = p4[2];
        const v4f ma = m4[0], mb = m4[1];
        const float in[12] = {ra[0], ra[1], ra[2], ra[3], rb[0], rb[1], rb[2], rb[3], rc[0], rc[1], rc[2], rc[3]};
        float pv[12] = {pa[0], pa[1], pa[2], pa[3], pb[0], pb[1], pb[2], pb[3], pc[0], pc[1], pc[2], pc[3]};
        float mv[8] = {ma[0], ma[1], ma[2], ma[3], mb[0], mb[1], mb[2], mb[3]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = 4 * q + j;
            v4f h0 = H0[i];
            v2f h1 = v2f{mv[2 * j], mv[2 * j + 1]};
            tmp_integrate_pixel(in[3 * j], in[3 * j + 1], in[3 * j + 2], pv[3 * j], pv[3 * j + 1], pv[3 * j + 2], h0, h1,
                                mat[4 * i + 3], ALB, ALB ? alb[i] : v4f{0.f, 0.f, 0.f, 0.f}, b, maxh);
            H0[i] = h0;
            mv[2 * j] = h1[0];
            mv[2 * j + 1] = h1[1];
        }
        p4[0] = v4f{pv[0], pv[1], pv[2], pv[3]};
        p4[1] = v4f{pv[4], pv[5], pv[6], pv[7]};
        p4[2] = v4f{pv[8], pv[9], pv[10], pv[11]};
        m4[0] = v4f{mv[0], mv[1], mv[2], mv[3]};
        m4[1] = v4f{mv[4], mv[5], mv[6], mv[7]};
    }
    for (int64_t i = 4 * nquads + t0; i < npix; i += nt) {
        v4f h0 = H0[i];
        v2f h1 = H1[i];
        float pr = prev[3 * i], pg = prev[3 * i + 1], pb = prev[3 * i + 2];
        tmp_integrate_pixel(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], pr, pg, pb, h0, h1, mat[4 * i + 3], ALB,
                            ALB ? alb[i] : v4f{0.f, 0.f, 0.f, 0.f}, b, maxh);
        H0[i] = h0;
        H1[i] = h1;
        prev[3 * i] = pr;
        prev[3 * i + 1] = pg;
        prev[3 * i + 2] = pb;
    }
}

// out_rgb = mean (* alb), out_h = h, out_var = the variance of lum(mean): temporal where h >= thr, else
// the 5 x 5 spatial estimate over the taps of the same material.  A wave none of whose lanes is on the
// spatial branch skips the 25 taps (the branch is taken on the wave's execution mask).
__global__ __launch_bounds__(kThreads) void k_tmp_resolve(const v4f* __restrict__ H0, const v2f* __restrict__ H1,
                                                           const v4f* __restrict__ gA, const v4f* __restrict__ alb,
                                                           float* __restrict__ out_rgb, float* __restrict__ out_var,
                                                           float* __restrict__ out_h, int32_t W, int32_t H, int32_t demodulate,
                                                           float b, float thr) {
    const int x = (int)blockIdx.x * kTX + (int)threadIdx.x % kTX, y = (int)blockIdx.y * kTY + (int)threadIdx.x / kTX;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const v4f h0 = H0[p];
    if (out_rgb) {
        f3 c = xyz(h0);
        if (demodulate) c = modulate(c, alb[p], false);
        out_rgb[3 * p] = c.x;
        out_rgb[3 * p + 1] = c.y;
        out_rgb[3 * p + 2] = c.z;
    }
    if (out_h) out_h[p] = h0[3];
    if (!out_var) return;
    const int* mats = reinterpret_cast<const int*>(gA);
    const int mat = mats[4 * p + 3];
    float var = 0.0f;
    if (mat >= 0) {
        if (h0[3] >= thr) {
            const v2f m = H1[p];
            var = gmax(0.0f, m[1] - m[0] * m[0]) * div_cr(b, h0[3]);
        } else {
            float s1 = 0.0f, s2 = 0.0f, cnt = 0.0f;
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t q = (size_t)qy * W + qx;
                    if (mats[4 * q + 3] != mat) continue;
                    const float l = lum(xyz(H0[q]));
                    s1 = s1 + l;
                    s2 = s2 + l * l;
                    cnt = cnt + 1.0f;
                }
            }
            const float m = div_cr(s1, cnt);
            var = gmax(0.0f, div_cr(s2, cnt) - m * m);
        }
    }
    out_var[p] = var;
}

#define TM_TRY(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return pt::fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

int lin_grid_of(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 65536); }
float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

}  // namespace

struct pt_temporal {
    int32_t W = 0, H = 0;
    int64_t npix = 0;
    pt_temporal_params prm{};
    // device side, allocated at the first frame: two sets (H0, H1, gA, gB) and one alb and prev
    v4f* H0[2] = {nullptr, nullptr};
    v2f* H1[2] = {nullptr, nullptr};
    v4f* gA[2] = {nullptr, nullptr};
    v4f* gB[2] = {nullptr, nullptr};
    v4f* alb = nullptr;
    float* prev = nullptr;
    int cur = 0;                 // the set that holds the history
    int32_t frames = 0;          // since the last reset
    float batch = 0.0f;          // samples per frame, fixed by the first frame since the last reset
    float prev_samples = 0.0f;
    int32_t last_case = 0;
    pt_camera cam{};
    hipEvent_t ev = nullptr;     // after the last queued work (the synchronous calls wait for it)
    bool ev_recorded = false;
};

namespace {

bool params_ok(const pt_temporal_params* p) {
    return std::isfinite(p->max_history) && p->max_history >= 0.0f && std::isfinite(p->min_ndot) && p->min_ndot >= -1.0f &&
           p->min_ndot <= 1.0f && std::isfinite(p->plane_tol) && p->plane_tol >= 0.0f && p->min_frames >= 0 &&
           p->min_frames <= kMaxMinFrames;
}

int tmp_planes(pt_temporal* t) {
    if (t->prev) return PT_OK;
    const size_t n = (size_t)t->npix, n4 = (n + 3) / 4 * 4;   // (H1 and prev are also moved four pixels at a time)
    bool ok = true;
    for (int k = 0; k < 2 && ok; ++k)
        ok = hipMalloc((void**)&t->H0[k], n * sizeof(v4f)) == hipSuccess &&
             hipMalloc((void**)&t->H1[k], n4 * sizeof(v2f)) == hipSuccess &&
             hipMalloc((void**)&t->gA[k], n * sizeof(v4f)) == hipSuccess &&
             hipMalloc((void**)&t->gB[k], n * sizeof(v4f)) == hipSuccess;
    ok = ok && hipMalloc((void**)&t->alb, n * sizeof(v4f)) == hipSuccess &&
         hipEventCreateWithFlags(&t->ev, hipEventDisableTiming) == hipSuccess &&
         hipMalloc((void**)&t->prev, n4 * 3 * sizeof(float)) == hipSuccess;
    if (!ok) {
        for (int k = 0; k < 2; ++k) {
            void** ps[4] = {(void**)&t->H0[k], (void**)&t->H1[k], (void**)&t->gA[k], (void**)&t->gB[k]};
            for (void** q : ps) {
                if (*q) (void)hipFree(*q);
                *q = nullptr;
            }
        }
        if (t->alb) (void)hipFree(t->alb);
        if (t->ev) (void)hipEventDestroy(t->ev);
        t->alb = nullptr;
        t->ev = nullptr;
        return pt::fail(PT_ERR_NOMEM, "hipMalloc (temporal planes)");
    }
    return PT_OK;
}

int tmp_mark(pt_temporal* t, hipStream_t st) {
    TM_TRY(hipEventRecord(t->ev, st));
    t->ev_recorded = true;
    return PT_OK;
}

bool camera_ok(const pt_camera* c) {
    const float vv = dot3(c->view, c->view), rr = dot3(c->right, c->right), uu = dot3(c->up, c->up);
    const float px = c->pixel_length[0], py = c->pixel_length[1];
    bool ok = std::isfinite(vv) && vv > 0.0f && std::isfinite(rr) && rr > 0.0f && std::isfinite(uu) && uu > 0.0f &&
              std::isfinite(px) && px != 0.0f && std::isfinite(py) && py != 0.0f;
    for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(c->position[k]);
    return ok;
}

}  // namespace

namespace pt {
// Which of the three cases a frame takes (PT_TEMPORAL_*), or the negated error of its argument checks.
// Needs no device.
int temporal_case(const pt_temporal* t, const pt_camera* cam, float samples) {
    if (!t || !cam) return -fail(PT_ERR_ARG, "null argument");
    if (!(std::isfinite(samples) && samples > 0.0f)) return -fail(PT_ERR_ARG, "samples must be finite and > 0");
    if (!camera_ok(cam)) return -fail(PT_ERR_ARG, "the camera's axes, pixel lengths and position must be finite and non-zero");
    int kind = PT_TEMPORAL_NEW_VIEW;
    float b = samples;
    if (t->frames == 0) {
        kind = PT_TEMPORAL_EMPTY;
    } else if (std::memcmp(cam, &t->cam, sizeof(pt_camera)) == 0 && samples > t->prev_samples) {
        kind = PT_TEMPORAL_SAME_VIEW;
        b = samples - t->prev_samples;
    }
    if (t->frames > 0 && b != t->batch)
        return -fail(PT_ERR_ARG, "the frame's batch size differs from the first frame's since the last reset");
    if (t->prm.max_history > 0.0f && b > t->prm.max_history)
        return -fail(PT_ERR_ARG, "max_history is smaller than one batch");
    return kind;
}

// The planes a frame of `kind` writes its G-buffer to: a producer may fill them directly and pass them
// to pt_temporal_frame, which then copies nothing.  Allocates the planes.
int temporal_staging(pt_temporal* t, int kind, float** gA, float** gB, float** alb) {
    if (int rc = tmp_planes(t)) return rc;
    const int dst = kind == PT_TEMPORAL_NEW_VIEW ? t->cur ^ 1 : t->cur;
    *gA = (float*)t->gA[dst];
    *gB = (float*)t->gB[dst];
    *alb = (float*)t->alb;
    return PT_OK;
}
int temporal_size(const pt_temporal* t, int32_t* width, int32_t* height) {
    if (!t) return fail(PT_ERR_ARG, "null temporal history");
    *width = t->W;
    *height = t->H;
    return PT_OK;
}
}  // namespace pt

extern "C" {

void pt_temporal_params_default(pt_temporal_params* p) {
    if (!p) return;
    *p = pt_temporal_params{};
    p->max_history = 32.0f;   // chosen on Cornell orbit sequences against 1024 spp
    p->min_ndot = 0.9f;
    p->plane_tol = 0.02f;
    p->demodulate = 1;
    p->min_frames = 4;
}

int pt_temporal_create(int32_t width, int32_t height, const pt_temporal_params* params, pt_temporal** out) {
    if (!out || width < 1 || height < 1 || (int64_t)width * height > kMaxPixels)
        return pt::fail(PT_ERR_ARG, "bad temporal history size");
    pt_temporal_params prm;
    if (params) prm = *params;
    else pt_temporal_params_default(&prm);
    if (!params_ok(&prm))
        return pt::fail(PT_ERR_ARG, "temporal parameters: max_history >= 0, min_ndot in [-1, 1], plane_tol >= 0, "
                                    "min_frames in 0..2^20, all finite");
    pt_temporal* t = new pt_temporal;   // (the planes come with the first frame: tmp_planes)
    t->W = width;
    t->H = height;
    t->npix = (int64_t)width * height;
    t->prm = prm;
    *out = t;
    return PT_OK;
}

int pt_temporal_destroy(pt_temporal* t) {
    if (!t) return PT_OK;
    if (t->ev_recorded) (void)hipEventSynchronize(t->ev);
    if (t->ev) (void)hipEventDestroy(t->ev);
    for (int k = 0; k < 2; ++k) {
        if (t->H0[k]) (void)hipFree(t->H0[k]);
        if (t->H1[k]) (void)hipFree(t->H1[k]);
        if (t->gA[k]) (void)hipFree(t->gA[k]);
        if (t->gB[k]) (void)hipFree(t->gB[k]);
    }
    if (t->alb) (void)hipFree(t->alb);
    if (t->prev) (void)hipFree(t->prev);
    delete t;
    return PT_OK;
}

// Host state only: the next frame takes the empty case, which reads none of the planes.
int pt_temporal_reset(pt_temporal* t) {
    if (!t) return pt::fail(PT_ERR_ARG, "null temporal history");
    t->frames = 0;
    t->batch = 0.0f;
    t->prev_samples = 0.0f;
    t->last_case = 0;
    return PT_OK;
}

int pt_temporal_info(const pt_temporal* t, int32_t* frames, float* batch_samples, int32_t* last_case) {
    if (!t) return pt::fail(PT_ERR_ARG, "null temporal history");
    if (frames) *frames = t->frames;
    if (batch_samples) *batch_samples = t->batch;
    if (last_case) *last_case = t->last_case;
    return PT_OK;
}

int pt_temporal_frame(pt_temporal* t, const pt_camera* cam, const float* d_rgb, float samples, const float* d_gA,
                      const float* d_gB, const float* d_alb, void* stream) {
    if (!t || !cam || !d_rgb || !d_gA || !d_gB || !d_alb) return pt::fail(PT_ERR_ARG, "null argument");
    const int kind = pt::temporal_case(t, cam, samples);
    if (kind < 0) return -kind;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = tmp_planes(t)) return rc;
    const float b = kind == PT_TEMPORAL_SAME_VIEW ? samples - t->prev_samples : samples;
    if (kind == PT_TEMPORAL_SAME_VIEW) {
        // (the view is the stored one: so are its G-buffer and albedo, and the planes passed in are not read)
        const bool quad = (reinterpret_cast<uintptr_t>(d_rgb) & 15u) == 0;
        const int64_t lanes = quad ? (t->npix + 3) / 4 : t->npix;
        const bool al = t->prm.demodulate != 0;
        auto kern = quad ? (al ? k_tmp_integrate<true, true> : k_tmp_integrate<true, false>)
                         : (al ? k_tmp_integrate<false, true> : k_tmp_integrate<false, false>);
        hipLaunchKernelGGL(kern, dim3(lin_grid_of(lanes)), dim3(256), 0, st, d_rgb, (const v4f*)t->gA[t->cur],
                           (const v4f*)t->alb, t->prev, t->H0[t->cur], t->H1[t->cur], t->npix, b, t->prm.max_history);
        TM_TRY(hipGetLastError());
    } else {
        const int src = t->cur, dst = kind == PT_TEMPORAL_NEW_VIEW ? t->cur ^ 1 : t->cur;
        const pt_camera& oc = t->cam;
        TmpArgs A{};
        A.rgb = d_rgb;
        A.gA_in = (const v4f*)d_gA;
        A.gB_in = (const v4f*)d_gB;
        A.alb_in = (const v4f*)d_alb;
        A.oH0 = t->H0[src];
        A.oH1 = t->H1[src];
        A.ogA = t->gA[src];
        A.ogB = t->gB[src];
        A.nH0 = t->H0[dst];
        A.nH1 = t->H1[dst];
        A.ngA = t->gA[dst];
        A.ngB = t->gB[dst];
        A.alb = t->alb;
        A.prev = t->prev;
        A.W = t->W;
        A.H = t->H;
        A.demodulate = t->prm.demodulate;
        A.samples = samples;
        A.b = b;
        A.maxh = t->prm.max_history;
        A.min_ndot = t->prm.min_ndot;
        A.plane_tol = t->prm.plane_tol;
        if (kind == PT_TEMPORAL_NEW_VIEW) {
            for (int k = 0; k < 3; ++k) {
                A.pos[k] = oc.position[k];
                A.view[k] = oc.view[k];
                A.right[k] = oc.right[k];
                A.up[k] = oc.up[k];
            }
            A.vv = dot3(oc.view, oc.view);
            A.rr = dot3(oc.right, oc.right);
            A.uu = dot3(oc.up, oc.up);
            A.plx = oc.pixel_length[0];
            A.ply = oc.pixel_length[1];
            A.hw = (float)t->W * 0.5f;
            A.hh = (float)t->H * 0.5f;
        }
        const dim3 grid((t->W + kTX - 1) / kTX, (t->H + kTY - 1) / kTY);
        auto kern = kind == PT_TEMPORAL_EMPTY ? k_tmp_reproject<true> : k_tmp_reproject<false>;
        hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, st, A);
        TM_TRY(hipGetLastError());
        t->cur = dst;
    }
    // The kernel is queued (a same-view frame rewrites the planes in place), so the host state follows
    // it whatever the event record below returns: an error from there leaves the object describing what
    // the device holds, and the synchronous calls fall back to the previous event.
    t->cam = *cam;
    t->prev_samples = samples;
    t->batch = b;
    t->frames += 1;
    t->last_case = kind;
    return tmp_mark(t, st);
}

int pt_temporal_resolve(pt_temporal* t, float* d_out_rgb, float* d_out_var, float* d_out_h, void* stream) {
    if (!t) return pt::fail(PT_ERR_ARG, "null temporal history");
    if ((d_out_rgb && (d_out_rgb == d_out_var || d_out_rgb == d_out_h)) || (d_out_var && d_out_var == d_out_h))
        return pt::fail(PT_ERR_ARG, "the outputs must not alias each other");
    if (t->frames < 1) return pt::fail(PT_ERR_ARG, "the history holds no frame");
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((t->W + kTX - 1) / kTX, (t->H + kTY - 1) / kTY);
    hipLaunchKernelGGL(k_tmp_resolve, grid, dim3(kThreads), 0, st, (const v4f*)t->H0[t->cur], (const v2f*)t->H1[t->cur],
                       (const v4f*)t->gA[t->cur], (const v4f*)t->alb, d_out_rgb, d_out_var, d_out_h, t->W, t->H,
                       t->prm.demodulate, t->batch, (float)t->prm.min_frames * t->batch);
    TM_TRY(hipGetLastError());
    return tmp_mark(t, st);
}

int pt_temporal_frame_host(pt_temporal* t, const pt_camera* cam, const float* rgb, float samples, const float* gA,
                           const float* gB, const float* alb) {
    if (!t || !cam || !rgb || !gA || !gB || !alb) return pt::fail(PT_ERR_ARG, "null argument");
    const int kind = pt::temporal_case(t, cam, samples);
    if (kind < 0) return -kind;
    const size_t n = (size_t)t->npix;
    float* dev = nullptr;   // rgb | gA | gB | alb
    if (hipMalloc((void**)&dev, (n * 15 + 4) * sizeof(float)) != hipSuccess) return pt::fail(PT_ERR_NOMEM, "hipMalloc (temporal frame)");
    float *d_gA = dev + 4 * ((3 * n + 3) / 4), *d_gB = d_gA + 4 * n, *d_alb = d_gB + 4 * n;   // (16-byte aligned)
    hipStream_t st = nullptr;
    int rc = PT_OK;
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess && t->ev_recorded) e = hipStreamWaitEvent(st, t->ev, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(dev, rgb, n * 3 * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_gA, gA, n * 4 * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_gB, gB, n * 4 * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_alb, alb, n * 4 * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) rc = pt_temporal_frame(t, cam, dev, samples, d_gA, d_gB, d_alb, st);
    if (st) {
        const hipError_t e2 = hipStreamSynchronize(st);
        if (e == hipSuccess) e = e2;
        (void)hipStreamDestroy(st);
    }
    (void)hipFree(dev);
    if (rc) return rc;
    if (e != hipSuccess) return pt::fail(PT_ERR_HIP, std::string("pt_temporal_frame_host: ") + hipGetErrorString(e));
    return PT_OK;
}

int pt_temporal_get(pt_temporal* t, float* h_H0, float* h_H1, float* h_gA, float* h_gB, float* h_prev_rgb, float* h_alb) {
    if (!t) return pt::fail(PT_ERR_ARG, "null temporal history");
    if (t->frames < 1) return pt::fail(PT_ERR_ARG, "the history holds no frame");
    if (t->ev_recorded) TM_TRY(hipEventSynchronize(t->ev));
    const size_t n = (size_t)t->npix;
    const int c = t->cur;
    if (h_H0) TM_TRY(hipMemcpy(h_H0, t->H0[c], n * sizeof(v4f), hipMemcpyDeviceToHost));
    if (h_H1) TM_TRY(hipMemcpy(h_H1, t->H1[c], n * sizeof(v2f), hipMemcpyDeviceToHost));
    if (h_gA) TM_TRY(hipMemcpy(h_gA, t->gA[c], n * sizeof(v4f), hipMemcpyDeviceToHost));
    if (h_gB) TM_TRY(hipMemcpy(h_gB, t->gB[c], n * sizeof(v4f), hipMemcpyDeviceToHost));
    if (h_prev_rgb) TM_TRY(hipMemcpy(h_prev_rgb, t->prev, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (h_alb) TM_TRY(hipMemcpy(h_alb, t->alb, n * sizeof(v4f), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_temporal_image(pt_temporal* t, const pt_denoise_var_params* var_params, float* host_rgb, float* host_var,
                      float* host_h) {
    if (!t) return pt::fail(PT_ERR_ARG, "null temporal history");
    if (!host_rgb && !host_var && !host_h) return pt::fail(PT_ERR_ARG, "null argument");
    if ((host_rgb && ((void*)host_rgb == (void*)host_var || (void*)host_rgb == (void*)host_h)) ||
        (host_var && host_var == host_h))
        return pt::fail(PT_ERR_ARG, "the outputs must not alias each other");
    if (var_params)
        if (int rc = pt::denoise_var_check(var_params, 1.0f)) return rc;
    if (t->frames < 1) return pt::fail(PT_ERR_ARG, "the history holds no frame");
    const size_t n = (size_t)t->npix;
    float* dev = nullptr;   // rgb | out rgb | var | out var | h   (rgb and out rgb: whole 16-byte vectors)
    const size_t n3 = 4 * ((3 * n + 3) / 4);
    if (hipMalloc((void**)&dev, (2 * n3 + 3 * n) * sizeof(float)) != hipSuccess)
        return pt::fail(PT_ERR_NOMEM, "hipMalloc (temporal image)");
    float *d_rgb = dev, *d_out = dev + n3, *d_var = dev + 2 * n3, *d_ovar = d_var + n, *d_h = d_ovar + n;
    pt_denoiser* dn = nullptr;
    hipStream_t st = nullptr;
    int rc = var_params ? pt_denoiser_create(t->W, t->H, &dn) : PT_OK;
    hipError_t e = hipSuccess;
    if (!rc) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (!rc && e == hipSuccess) {
        if (t->ev_recorded) e = hipStreamWaitEvent(st, t->ev, 0);
        if (e == hipSuccess) rc = pt_temporal_resolve(t, d_rgb, d_var, d_h, st);
        const int c = t->cur;
        if (e == hipSuccess && !rc && var_params)
            rc = pt_denoiser_run_var(dn, d_rgb, 1.0f, d_var, (const float*)t->gA[c], (const float*)t->gB[c],
                                     (const float*)t->alb, var_params, d_out, d_ovar, st);
        if (e == hipSuccess && !rc && host_rgb)
            e = hipMemcpyAsync(host_rgb, var_params ? d_out : d_rgb, n * 3 * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && !rc && host_var)
            e = hipMemcpyAsync(host_var, var_params ? d_ovar : d_var, n * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && !rc && host_h) e = hipMemcpyAsync(host_h, d_h, n * sizeof(float), hipMemcpyDeviceToHost, st);
        const hipError_t e2 = hipStreamSynchronize(st);
        if (e == hipSuccess) e = e2;
    }
    if (st) (void)hipStreamDestroy(st);
    pt_denoiser_destroy(dn);
    (void)hipFree(dev);
    if (rc) return rc;
    if (e != hipSuccess) return pt::fail(PT_ERR_HIP, std::string("pt_temporal_image: ") + hipGetErrorString(e));
    return PT_OK;
}

}  // extern "C"
