// The image-level entry points of a render context: its accumulator, the G-buffer readback, the denoisers,
// variance tracking, adaptive sampling and temporal frames.  Host code: the kernels it runs are other units',
// behind their C entry points, and it sees the context through pt_ctx.h (`ctx` the context, `c` its head).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "pt_ctx.h"

using namespace pt;

void CtxHead::release() {
    if (ad) (void)pt_adaptive_obj_destroy(ad);
    if (ad_cmask) (void)hipFree(ad_cmask);
    if (mom) (void)pt_moments_destroy(mom);
    if (planes) (void)hipFree(planes);
    ad = nullptr;
    ad_cmask = nullptr;
    mom = nullptr;
    planes = nullptr;
    planes_valid = false;
}

CtxHead::~CtxHead() {
    if (exr_planes) (void)hipFree(exr_planes);
}

int pt::adaptive_apply(pt_ctx* ctx) {
    CtxHead* c = ctx_head(ctx);
    const CameraMasks m = camera_masks(ctx);
    if (int rc = pt_adaptive_obj_apply(c->ad, m.dev, c->ad_cmask, c->io_stream)) return rc;
    std::vector<uint32_t> act(m.blocks);
    if (int rc = pt_adaptive_obj_get(c->ad, nullptr, nullptr, nullptr, nullptr, act.data(), nullptr)) return rc;
    c->ad_active = (int32_t)(act.size() - std::count(act.begin(), act.end(), 0u));
    point_cmask(ctx, c->ad_cmask, act.data());
    return PT_OK;
}

namespace {

// The accumulator was just replaced or cleared on `st`: the feature that is on starts again from it (adaptive: every
// block active with no batch; nothing of the context is queued behind the caller's wait, so the masks are rebuilt at once).
int rebase(pt_ctx* ctx, CtxHead* c, hipStream_t st) {
    c->planes_valid = false;
    if (c->mom) return pt_moments_reset(c->mom, c->image, st);
    if (!c->ad) return PT_OK;
    if (int rc = pt_adaptive_obj_reset(c->ad, c->image, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = adaptive_quiesce(ctx)) return rc;
    return adaptive_apply(ctx);
}

// The context's first-hit planes, on st (pt_gbuffer orders and marks itself).
int fill_planes(pt_ctx* ctx, CtxHead* c, hipStream_t st) {
    if (int rc = pt_gbuffer(ctx, c->planes, c->planes + 4 * c->npix, c->planes + 8 * c->npix, nullptr, st)) return rc;
    c->planes_valid = true;
    return PT_OK;
}

// The end of a synchronous readback through scratch `d` (allocated before anything was queued) and perhaps a
// denoiser: rc is the result of queueing the producing work on the io stream.  Zero: that work is the context's
// last, and the copies follow it.  The stream is drained before the scratch is freed, whatever failed.
struct Copy { float* host; const float* dev; size_t floats; };   // (host null: not asked for)
int read_back(CtxHead* c, const char* who, int rc, float* d, pt_denoiser* dn, std::initializer_list<Copy> copies) {
    hipError_t e = hipSuccess;
    if (!rc) rc = mark_ctx(c, c->io_stream);
    if (!rc)
        for (const Copy& k : copies)
            if (k.host && e == hipSuccess)
                e = hipMemcpyAsync(k.host, k.dev, k.floats * sizeof(float), hipMemcpyDeviceToHost, c->io_stream);
    const hipError_t e2 = hipStreamSynchronize(c->io_stream);
    if (e == hipSuccess) e = e2;
    pt_denoiser_destroy(dn);
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return pt::fail(PT_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return PT_OK;
}

// The accumulator as a file of encoder `e` (of `iter` iterations), on the stream and behind the context's passes.
// whole: the refusal of a context that renders one tile of several, or null.
template <class Enc>
int preview_file(pt_ctx* ctx, int32_t iter, Enc* e, int (*accum)(Enc*, const float*, float, uint8_t*, int64_t, int64_t*, void*),
                 const char* name, const char* whole, uint8_t* d_out, int64_t cap, int64_t* d_size, void* stream) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !e || !d_out || !d_size || iter <= 0) return pt::fail(PT_ERR_ARG, "bad argument");
    if (whole && c->world > 1) return pt::fail(PT_ERR_ARG, whole);
    int32_t ew = 0, eh = 0;
    pt::enc_size(pt::enc_head(e), &ew, &eh);
    if (ew != c->W || (int64_t)ew * eh != (int64_t)c->npix)
        return pt::fail(PT_ERR_ARG, std::string("the ") + name + " encoder and the context's tile differ in size");
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = wait_finalize(c, st)) return rc;
    if (int rc = accum(e, c->image, (float)iter, d_out, cap, d_size, st)) return rc;
    return mark_ctx(c, st);
}

}  // namespace

extern "C" {

int pt_get_image(pt_ctx* ctx, float* host_rgb) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !host_rgb) return pt::fail(PT_ERR_ARG, "null argument");
    if (int rc = wait_ctx(c)) return rc;   // this context's passes only (pathtrace.cu:524's copy)
    HIP_TRY(io_copy(c, host_rgb, c->image, c->npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_get_accum(pt_ctx* ctx, float* host_rgb) { return pt_get_image(ctx, host_rgb); }

int pt_host_register(void* host, uint64_t bytes) {
    if (!host || !bytes) return pt::fail(PT_ERR_ARG, "null argument");
    const hipError_t e = hipHostRegister(host, (size_t)bytes, hipHostRegisterDefault);
    if (e != hipSuccess) {
        // a caller may go on without the page lock (the copies still work, staged): leave no sticky
        // last-error behind for the next launch's hipGetLastError check to report
        (void)hipGetLastError();
        return pt::fail(PT_ERR_DEVICE, std::string("hipHostRegister: ") + hipGetErrorString(e));
    }
    return PT_OK;
}

int pt_host_unregister(void* host) {
    if (!host) return pt::fail(PT_ERR_ARG, "null argument");
    HIP_TRY(hipHostUnregister(host));
    return PT_OK;
}

int pt_stream_create(void** stream) {
    if (!stream) return pt::fail(PT_ERR_ARG, "null argument");
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return PT_OK;
}

int pt_stream_destroy(void* stream) {
    if (stream) HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return PT_OK;
}

// The accumulator is loaded with every -0 replaced by +0.  The reference adds every iteration's colour
// (zero or not) into every pixel, so after any pass its image holds no -0 (-0 + 0 = +0); the passes here
// skip the additions of zero colours (retire, k_finalize_spp), which are identities on every value but -0.
// A +0 loaded in place of -0 makes the two agree bit for bit from the first pass on.
int pt_set_accum(pt_ctx* ctx, const float* host_rgb) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !host_rgb) return pt::fail(PT_ERR_ARG, "null argument");
    if (c->ad) return pt::fail(PT_ERR_ARG, "pt_set_accum on an adaptive context: a saved accumulator carries no per-block counts");
    if (int rc = wait_ctx(c)) return rc;
    const size_t n = c->npix * 3;
    std::vector<float> img(host_rgb, host_rgb + n);
    for (float& v : img)
        if (v == 0.0f) v = 0.0f;   // (-0 == 0: both zeros become +0)
    HIP_TRY(io_copy(c, c->image, img.data(), n * sizeof(float), hipMemcpyHostToDevice));
    if (!c->mom) return PT_OK;
    if (int rc = rebase(ctx, c, c->io_stream)) return rc;
    return mark_ctx(c, c->io_stream);
}

int pt_copy_image(pt_ctx* ctx, float* d_rgb, void* stream) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !d_rgb) return pt::fail(PT_ERR_ARG, "null argument");
    if (int rc = wait_finalize(c, (hipStream_t)stream)) return rc;
    HIP_TRY(hipMemcpyAsync(d_rgb, c->image, c->npix * 3 * sizeof(float), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return mark_ctx(c, (hipStream_t)stream);
}

int pt_get_gbuffer(pt_ctx* ctx, float* h_gA, float* h_gB, float* h_alb, float* h_uv) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !h_gA || !h_gB || !h_alb) return pt::fail(PT_ERR_ARG, "null argument");
    const size_t npix = c->npix;
    float* d = nullptr;   // gA | gB | alb | uv
    if (hipMalloc((void**)&d, npix * 14 * sizeof(float)) != hipSuccess) return pt::fail(PT_ERR_NOMEM, "hipMalloc (G-buffer)");
    const int rc = pt_gbuffer(ctx, d, d + 4 * npix, d + 8 * npix, h_uv ? d + 12 * npix : nullptr, c->io_stream);
    return read_back(c, "pt_get_gbuffer", rc, d, nullptr, {{h_gA, d, 4 * npix}, {h_gB, d + 4 * npix, 4 * npix},
                                                           {h_alb, d + 8 * npix, 4 * npix}, {h_uv, d + 12 * npix, 2 * npix}});
}

// G-buffer + accumulator -> denoised host image: everything on the context's io stream, the filter
// reading the accumulator in place (it is not modified).
int pt_denoise_image(pt_ctx* ctx, float samples, const pt_denoise_params* prm, float* host_out_rgb) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !host_out_rgb) return pt::fail(PT_ERR_ARG, "null argument");
    if (c->world > 1) return pt::fail(PT_ERR_ARG, "pt_denoise_image needs the whole image (world == 1)");
    if (int rc = pt::denoise_check(prm, samples)) return rc;
    const size_t npix = c->npix;
    float* d = nullptr;   // gA | gB | alb | out
    if (hipMalloc((void**)&d, npix * 15 * sizeof(float)) != hipSuccess) return pt::fail(PT_ERR_NOMEM, "hipMalloc (denoise)");
    pt_denoiser* dn = nullptr;
    int rc = pt_denoiser_create(c->W, (int32_t)(c->npix / c->W), &dn);
    if (!rc) rc = pt_gbuffer(ctx, d, d + 4 * npix, d + 8 * npix, nullptr, c->io_stream);
    if (!rc) rc = pt_denoiser_run(dn, c->image, samples, d, d + 4 * npix, d + 8 * npix, prm, d + 12 * npix, c->io_stream);
    return read_back(c, "pt_denoise_image", rc, d, dn, {{host_out_rgb, d + 12 * npix, npix * 3}});
}

int pt_reset_image(pt_ctx* ctx, void* stream) {
    CtxHead* c = ctx_head(ctx);
    if (!c) return pt::fail(PT_ERR_ARG, "null context");
    if (int rc = wait_finalize(c, (hipStream_t)stream)) return rc;
    HIP_TRY(hipMemsetAsync(c->image, 0, c->npix * 3 * sizeof(float), (hipStream_t)stream));
    if (int rc = rebase(ctx, c, (hipStream_t)stream)) return rc;
    return mark_ctx(c, (hipStream_t)stream);
}

// ---- variance tracking ---------------------------------------------------------
int pt_track_variance(pt_ctx* ctx, int32_t on) {
    CtxHead* c = ctx_head(ctx);
    if (!c) return pt::fail(PT_ERR_ARG, "null context");
    if (c->world > 1) return pt::fail(PT_ERR_ARG, "variance tracking needs the whole image (world == 1)");
    if (on && c->ad) return pt::fail(PT_ERR_ARG, "variance tracking on an adaptive context (pt_adaptive_enable keeps its own moments)");
    if (int rc = wait_ctx(c)) return rc;
    if (!on && c->mom) c->release();
    if (!on || c->mom) return PT_OK;
    if (int rc = pt_moments_create(c->W, (int32_t)(c->npix / c->W), &c->mom)) return rc;
    if (hipMalloc((void**)&c->planes, c->npix * 12 * sizeof(float)) != hipSuccess) {
        c->release();
        return pt::fail(PT_ERR_NOMEM, "hipMalloc (variance tracking)");
    }
    if (int rc = rebase(ctx, c, c->io_stream)) return rc;
    return mark_ctx(c, c->io_stream);
}

int pt_variance_update(pt_ctx* ctx, float batch_samples, int32_t demodulate, void* stream) {
    CtxHead* c = ctx_head(ctx);
    if (!c) return pt::fail(PT_ERR_ARG, "null context");
    if (!c->mom) return pt::fail(PT_ERR_ARG, "variance tracking is off (pt_track_variance)");
    if (int rc = pt::moments_update_check(c->mom, batch_samples)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = wait_finalize(c, st)) return rc;
    if (demodulate && !c->planes_valid)
        if (int rc = fill_planes(ctx, c, st)) return rc;
    const float* alb = demodulate ? c->planes + 8 * c->npix : nullptr;
    if (int rc = pt_moments_update(c->mom, c->image, batch_samples, alb, st)) return rc;
    return mark_ctx(c, st);
}

int pt_variance_info(const pt_ctx* ctx, int32_t* on, int32_t* batches, float* batch_samples) {
    const CtxHead* c = ctx_head(const_cast<pt_ctx*>(ctx));
    if (!c) return pt::fail(PT_ERR_ARG, "null context");
    if (on) *on = c->mom ? 1 : 0;
    if (batches) *batches = 0;
    if (batch_samples) *batch_samples = 0.0f;
    return c->mom ? pt_moments_info(c->mom, batches, batch_samples) : PT_OK;
}

int pt_get_variance(pt_ctx* ctx, float samples, float* host_var) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !host_var) return pt::fail(PT_ERR_ARG, "null argument");
    if (!c->mom) return pt::fail(PT_ERR_ARG, "variance tracking is off (pt_track_variance)");
    if (int rc = pt::moments_variance_check(c->mom, samples)) return rc;
    float* d = nullptr;
    if (hipMalloc((void**)&d, c->npix * sizeof(float)) != hipSuccess) return pt::fail(PT_ERR_NOMEM, "hipMalloc (variance)");
    int rc = wait_finalize(c, c->io_stream);
    if (!rc) rc = pt_moments_variance(c->mom, samples, d, c->io_stream);
    return read_back(c, "pt_get_variance", rc, d, nullptr, {{host_var, d, c->npix}});
}

// Like pt_denoise_image, with the tracked variance: fresh first-hit planes (into the context's own),
// the variance of `samples` samples, the filter and the copy, all on the io stream.
int pt_denoise_image_var(pt_ctx* ctx, float samples, const pt_denoise_var_params* prm, float* host_out_rgb) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !host_out_rgb) return pt::fail(PT_ERR_ARG, "null argument");
    if (c->world > 1) return pt::fail(PT_ERR_ARG, "pt_denoise_image_var needs the whole image (world == 1)");
    if (!c->mom) return pt::fail(PT_ERR_ARG, "variance tracking is off (pt_track_variance)");
    if (int rc = pt::denoise_var_check(prm, samples)) return rc;
    if (int rc = pt::moments_variance_check(c->mom, samples)) return rc;
    const size_t npix = c->npix;
    float* d = nullptr;   // var | out
    if (hipMalloc((void**)&d, npix * 4 * sizeof(float)) != hipSuccess) return pt::fail(PT_ERR_NOMEM, "hipMalloc (denoise)");
    pt_denoiser* dn = nullptr;
    int rc = pt_denoiser_create(c->W, (int32_t)(c->npix / c->W), &dn);
    if (!rc) rc = fill_planes(ctx, c, c->io_stream);
    if (!rc) rc = pt_moments_variance(c->mom, samples, d, c->io_stream);
    if (!rc) rc = pt_denoiser_run_var(dn, c->image, samples, d, c->planes, c->planes + 4 * npix, c->planes + 8 * npix, prm,
                                      d + npix, nullptr, c->io_stream);
    return read_back(c, "pt_denoise_image_var", rc, d, dn, {{host_out_rgb, d + npix, npix * 3}});
}

// ---- adaptive sampling ---------------------------------------------------------
int pt_adaptive_enable(pt_ctx* ctx, int32_t on) {
    CtxHead* c = ctx_head(ctx);
    if (!c) return pt::fail(PT_ERR_ARG, "null context");
    if (!on) {
        if (!c->ad) return PT_OK;
        if (int rc = adaptive_quiesce(ctx)) return rc;
        c->release();
        point_cmask(ctx, nullptr, nullptr);
        return PT_OK;
    }
    if (c->world > 1) return pt::fail(PT_ERR_ARG, "adaptive sampling needs the whole image (world == 1)");
    if (const char* why = adaptive_refusal(ctx)) return pt::fail(PT_ERR_ARG, why);
    if (c->mom) return pt::fail(PT_ERR_ARG, "adaptive sampling on a context that tracks variance (pt_track_variance)");
    if (c->ad) return PT_OK;
    if (int rc = adaptive_quiesce(ctx)) return rc;
    if (int rc = pt_adaptive_obj_create(c->W, (int32_t)(c->npix / c->W), &c->ad)) return rc;
    if (hipMalloc((void**)&c->ad_cmask, std::max<size_t>(camera_masks(ctx).blocks * sizeof(uint32_t), 16)) != hipSuccess ||
        hipMalloc((void**)&c->planes, c->npix * 12 * sizeof(float)) != hipSuccess) {
        c->release();
        return pt::fail(PT_ERR_NOMEM, "hipMalloc (adaptive sampling)");
    }
    const int rc = rebase(ctx, c, c->io_stream);
    if (rc) c->release();   // (the first bounce still reads the camera masks: adaptive_apply points it last)
    return rc;
}

int pt_adaptive_update(pt_ctx* ctx, int32_t demodulate, void* stream) {
    CtxHead* c = ctx_head(ctx);
    if (!c) return pt::fail(PT_ERR_ARG, "null context");
    if (!c->ad) return pt::fail(PT_ERR_ARG, "adaptive sampling is off (pt_adaptive_enable)");
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = wait_finalize(c, st)) return rc;
    if (demodulate && !c->planes_valid)
        if (int rc = fill_planes(ctx, c, st)) return rc;
    const float* alb = demodulate ? c->planes + 8 * c->npix : nullptr;
    if (int rc = pt_adaptive_obj_update(c->ad, c->image, (float)c->spp, alb, st)) return rc;
    return mark_ctx(c, st);
}

int pt_adaptive_select(pt_ctx* ctx, const pt_adaptive_params* p, int32_t* active_blocks, int32_t* blocks) {
    CtxHead* c = ctx_head(ctx);
    if (!c) return pt::fail(PT_ERR_ARG, "null context");
    if (!c->ad) return pt::fail(PT_ERR_ARG, "adaptive sampling is off (pt_adaptive_enable)");
    if (int rc = pt::adaptive_params_check(p)) return rc;
    if (int rc = adaptive_quiesce(ctx)) return rc;
    int32_t n = 0;
    if (int rc = pt_adaptive_obj_select(c->ad, p, c->io_stream, &n, blocks)) return rc;
    if (active_blocks) *active_blocks = n;
    return adaptive_apply(ctx);
}

int pt_adaptive_set_mask(pt_ctx* ctx, const uint8_t* host_mask, int32_t nblocks) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !host_mask) return pt::fail(PT_ERR_ARG, "null argument");
    if (!c->ad) return pt::fail(PT_ERR_ARG, "adaptive sampling is off (pt_adaptive_enable)");
    if ((size_t)nblocks != camera_masks(ctx).blocks || nblocks < 0)
        return pt::fail(PT_ERR_ARG, "the mask length differs from the number of blocks");
    if (int rc = adaptive_quiesce(ctx)) return rc;
    if (int rc = pt_adaptive_obj_set_mask(c->ad, host_mask, nblocks, c->io_stream)) return rc;
    return adaptive_apply(ctx);
}

int pt_adaptive_info(const pt_ctx* ctx, int32_t* on, int32_t* blocks, int32_t* active_blocks, int32_t* updates,
                     float* batch_samples) {
    const CtxHead* c = ctx_head(const_cast<pt_ctx*>(ctx));
    if (!c) return pt::fail(PT_ERR_ARG, "null context");
    if (on) *on = c->ad ? 1 : 0;
    if (blocks) *blocks = 0;
    if (active_blocks) *active_blocks = c->ad ? c->ad_active : 0;
    if (updates) *updates = 0;
    if (batch_samples) *batch_samples = 0.0f;
    return c->ad ? pt_adaptive_obj_info(c->ad, blocks, updates, batch_samples) : PT_OK;
}

int pt_adaptive_get(pt_ctx* ctx, float* h_m1, float* h_m2, float* h_prev_rgb, uint32_t* h_nb, uint32_t* h_act,
                    uint8_t* h_hot) {
    CtxHead* c = ctx_head(ctx);
    if (!c) return pt::fail(PT_ERR_ARG, "null context");
    if (!c->ad) return pt::fail(PT_ERR_ARG, "adaptive sampling is off (pt_adaptive_enable)");
    if (int rc = wait_ctx(c)) return rc;
    return pt_adaptive_obj_get(c->ad, h_m1, h_m2, h_prev_rgb, h_nb, h_act, h_hot);
}

// Resolve, the optional variance-guided filter over fresh first-hit planes (samples = 1) and the
// copies, all on the io stream.
int pt_adaptive_image(pt_ctx* ctx, const pt_denoise_var_params* prm, float* host_rgb, float* host_var) {
    CtxHead* c = ctx_head(ctx);
    if (!c || (!host_rgb && !host_var)) return pt::fail(PT_ERR_ARG, "null argument");
    if (!c->ad) return pt::fail(PT_ERR_ARG, "adaptive sampling is off (pt_adaptive_enable)");
    if (prm)
        if (int rc = pt::denoise_var_check(prm, 1.0f)) return rc;
    int32_t updates = 0;
    (void)pt_adaptive_obj_info(c->ad, nullptr, &updates, nullptr);
    if (updates < 1) return pt::fail(PT_ERR_ARG, "pt_adaptive_image needs an update (pt_adaptive_update)");
    const size_t npix = c->npix;
    float* d = nullptr;   // rgb | var | filtered rgb | filtered var
    if (hipMalloc((void**)&d, npix * 8 * sizeof(float)) != hipSuccess) return pt::fail(PT_ERR_NOMEM, "hipMalloc (adaptive image)");
    float *d_rgb = d, *d_var = d + 3 * npix, *d_frgb = d + 4 * npix, *d_fvar = d + 7 * npix;
    pt_denoiser* dn = nullptr;
    int rc = wait_finalize(c, c->io_stream);
    if (!rc) rc = pt_adaptive_obj_resolve(c->ad, c->image, d_rgb, d_var, c->io_stream);
    if (!rc && prm) {
        rc = pt_denoiser_create(c->W, (int32_t)(c->npix / c->W), &dn);
        if (!rc) rc = fill_planes(ctx, c, c->io_stream);
        if (!rc) rc = pt_denoiser_run_var(dn, d_rgb, 1.0f, d_var, c->planes, c->planes + 4 * npix, c->planes + 8 * npix, prm,
                                          d_frgb, d_fvar, c->io_stream);
    }
    return read_back(c, "pt_adaptive_image", rc, d, dn,
                     {{host_rgb, prm ? d_frgb : d_rgb, npix * 3}, {host_var, prm ? d_fvar : d_var, npix}});
}

// ---- temporal reprojection ----------------------------------------------------
// One frame of a pt_temporal from this context: the accumulator in place, and for a frame that is not
// of the stored view a fresh first-hit G-buffer written straight into the object's planes.
int pt_temporal_frame_ctx(pt_temporal* t, pt_ctx* ctx, float samples, void* stream) {
    CtxHead* c = ctx_head(ctx);
    if (!t || !c) return pt::fail(PT_ERR_ARG, "null argument");
    if (c->world > 1) return pt::fail(PT_ERR_ARG, "pt_temporal_frame_ctx needs the whole image (world == 1)");
    int32_t tw = 0, th = 0;
    if (int rc = pt::temporal_size(t, &tw, &th)) return rc;
    if (tw != c->W || (int64_t)tw * th != (int64_t)c->npix)
        return pt::fail(PT_ERR_ARG, "the temporal history and the context differ in size");
    const int kind = pt::temporal_case(t, &c->scene_cam, samples);
    if (kind < 0) return -kind;
    const hipStream_t st = (hipStream_t)stream;
    float *gA = nullptr, *gB = nullptr, *alb = nullptr;
    if (int rc = pt::temporal_staging(t, kind, &gA, &gB, &alb)) return rc;
    if (kind != PT_TEMPORAL_SAME_VIEW) {
        if (int rc = pt_gbuffer(ctx, gA, gB, alb, nullptr, st)) return rc;   // (waits for the finalize, marks the context)
    } else if (int rc = wait_finalize(c, st)) {
        return rc;
    }
    if (int rc = pt_temporal_frame(t, &c->scene_cam, c->image, samples, gA, gB, alb, st)) return rc;
    return mark_ctx(c, st);
}

// ---- preview frames as JPEG ---------------------------------------------------
// pt_preview_rgba's ordering and division by iter, the bytes going straight into the encoder's blocks
// kernel: no RGBA plane is written.
int pt_preview_jpeg(pt_ctx* ctx, int32_t iter, pt_jpeg_enc* e, uint8_t* d_out, int64_t cap, int64_t* d_size, void* stream) {
    return preview_file(ctx, iter, e, pt_jpeg_enc_accum, "JPEG", nullptr, d_out, cap, d_size, stream);
}

// ---- frames and final images as PNG -------------------------------------------
// The same ordering; the encoder's filter kernel converts the accumulator as its params.conv says.
int pt_preview_png(pt_ctx* ctx, int32_t iter, pt_png_enc* e, uint8_t* d_out, int64_t cap, int64_t* d_size, void* stream) {
    return preview_file(ctx, iter, e, pt_png_enc_accum, "PNG", "pt_preview_png needs the whole image (world == 1)", d_out, cap,
                        d_size, stream);
}

// ---- final images as Radiance HDR ---------------------------------------------
// The same ordering; the encoder's convert kernel divides the accumulator by iter.
int pt_preview_hdr(pt_ctx* ctx, int32_t iter, pt_hdr_enc* e, uint8_t* d_out, int64_t cap, int64_t* d_size, void* stream) {
    return preview_file(ctx, iter, e, pt_hdr_enc_accum, "HDR", "pt_preview_hdr needs the whole image (world == 1)", d_out, cap,
                        d_size, stream);
}

// ---- beauty and first-hit layers as OpenEXR -----------------------------------
// The same ordering.  The beauty planes are the accumulator's, divided by iter in the encoder's convert kernel; the
// other layers are read in place from pt_gbuffer's planes in the context's scratch.
int pt_preview_exr(pt_ctx* ctx, int32_t iter, int32_t layers, pt_exr_enc* e, uint8_t* d_out, int64_t cap, int64_t* d_size,
                   void* stream) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !e || !d_out || !d_size || iter <= 0) return pt::fail(PT_ERR_ARG, "bad argument");
    if (c->world > 1) return pt::fail(PT_ERR_ARG, "pt_preview_exr needs the whole image (world == 1)");
    int32_t ew = 0, eh = 0;
    pt::enc_size(pt::enc_head(e), &ew, &eh);
    if (ew != c->W || (int64_t)ew * eh != (int64_t)c->npix)
        return pt::fail(PT_ERR_ARG, "the EXR encoder and the context's tile differ in size");
    // the encoder's channels: pt_exr_ctx_channels(layers, half)'s, with `half` read off the first channel of each layer
    const pt_exr_channel* have = nullptr;
    int32_t nhave = 0, nwant = 0, half = 0;
    pt::exr_channels(e, &have, &nhave);
    pt_exr_channel want[16];
    if (int rc = pt_exr_ctx_channels(layers, 0, want, &nwant)) return rc;
    bool same = nhave == nwant;
    if (same) {
        int at = 0;
        for (int32_t bit = 1; bit <= PT_EXR_ID; bit <<= 1) {
            if (!(layers & bit)) continue;
            if (have[at].type == PT_EXR_HALF) half |= bit;
            at += bit == PT_EXR_DEPTH || bit == PT_EXR_ID ? 1 : (bit == PT_EXR_UV ? 2 : 3);
        }
        (void)pt_exr_ctx_channels(layers, half, want, &nwant);
        for (int k = 0; k < nwant; ++k) same = same && !std::strcmp(have[k].name, want[k].name) && have[k].type == want[k].type;
    }
    if (!same) return pt::fail(PT_ERR_ARG, "the EXR encoder's channels are not pt_exr_ctx_channels' for these layers");
    const hipStream_t st = (hipStream_t)stream;
    const size_t n = c->npix;
    if ((layers & ~PT_EXR_BEAUTY) && !c->exr_planes && hipMalloc((void**)&c->exr_planes, n * 14 * sizeof(float)) != hipSuccess) {
        c->exr_planes = nullptr;
        (void)hipGetLastError();
        return pt::fail(PT_ERR_NOMEM, "hipMalloc (EXR layers)");
    }
    float* s = c->exr_planes;
    if (layers & ~PT_EXR_BEAUTY) {
        if (int rc = pt_gbuffer(ctx, s, s + 4 * n, s + 8 * n, s + 12 * n, st)) return rc;   // (waits for the finalize, marks the context)
    } else if (int rc = wait_finalize(c, st)) {
        return rc;
    }
    pt_exr_plane pl[16];
    int at = 0;
    auto add = [&](const float* d, int count, int stride, float divisor) {
        for (int k = 0; k < count; ++k) pl[at++] = pt_exr_plane{d + k, stride, divisor};
    };
    if (layers & PT_EXR_BEAUTY) add(c->image, 3, 3, (float)iter);
    if (layers & PT_EXR_ALBEDO) add(s + 8 * n, 3, 4, 1.0f);
    if (layers & PT_EXR_NORMAL) add(s, 3, 4, 1.0f);
    if (layers & PT_EXR_POSITION) add(s + 4 * n, 3, 4, 1.0f);
    if (layers & PT_EXR_DEPTH) add(s + 4 * n + 3, 1, 4, 1.0f);
    if (layers & PT_EXR_UV) add(s + 12 * n, 2, 2, 1.0f);
    if (layers & PT_EXR_ID) add(s + 3, 1, 4, 1.0f);
    if (int rc = pt_exr_enc_planes(e, pl, d_out, cap, d_size, st)) return rc;
    return mark_ctx(c, st);
}

// ---- display bytes ------------------------------------------------------------
// The same ordering; in auto mode the metering runs first, on the same stream.
int pt_preview_display(pt_ctx* ctx, int32_t iter, pt_display* d, uint8_t* d_pix, int32_t pixel_stride, void* stream) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !d || !d_pix || iter <= 0) return pt::fail(PT_ERR_ARG, "bad argument");
    if (c->world > 1) return pt::fail(PT_ERR_ARG, "pt_preview_display needs the whole image (world == 1)");
    int32_t dw = 0, dh = 0, automatic = 0;
    if (int rc = pt::display_size(d, &dw, &dh, &automatic)) return rc;
    if (dw != c->W || (int64_t)dw * dh != (int64_t)c->npix)
        return pt::fail(PT_ERR_ARG, "the display transform and the context's tile differ in size");
    if (pixel_stride != 3 && pixel_stride != 4) return pt::fail(PT_ERR_ARG, "the pixel stride must be 3 or 4");
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = wait_finalize(c, st)) return rc;
    if (int rc = automatic ? pt_display_frame(d, c->image, (float)iter, d_pix, pixel_stride, st)
                           : pt_display_apply(d, c->image, (float)iter, d_pix, pixel_stride, st))
        return rc;
    return mark_ctx(c, st);
}

// ---- bloom --------------------------------------------------------------------
// The same ordering; the output is an accumulator of `iter` samples like the input.
int pt_preview_bloom(pt_ctx* ctx, int32_t iter, pt_bloom* b, float* d_out, void* stream) {
    CtxHead* c = ctx_head(ctx);
    if (!c || !b || !d_out || iter <= 0) return pt::fail(PT_ERR_ARG, "bad argument");
    if (c->world > 1) return pt::fail(PT_ERR_ARG, "pt_preview_bloom needs the whole image (world == 1)");
    int32_t bw = 0, bh = 0;
    if (int rc = pt::bloom_size(b, &bw, &bh)) return rc;
    if (bw != c->W || (int64_t)bw * bh != (int64_t)c->npix)
        return pt::fail(PT_ERR_ARG, "the bloom and the context's tile differ in size");
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = wait_finalize(c, st)) return rc;
    if (int rc = pt_bloom_apply(b, c->image, (float)iter, d_out, st)) return rc;
    return mark_ctx(c, st);
}

}  // extern "C"
