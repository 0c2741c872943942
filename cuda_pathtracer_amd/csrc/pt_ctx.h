// What the image-level entry points (pt_ctx_image.cpp) see of a render context: pt_ctx's base.  The
// launch arguments, path buffers, lanes and render-ahead stay private to pt_kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include "pt_internal.h"

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return pt::fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

#pragma GCC visibility push(hidden)   // (internal to the library: no exported symbol)
namespace pt {

struct CtxHead {
    // The tile's image, fixed after pt_create (copies of args.image and args.tile, set there once).
    float* image = nullptr;   // the accumulator, npix * 3
    size_t npix = 0;
    int W = 0, world = 1, spp = 1;
    pt_camera scene_cam{};    // the scene camera the context was created with (pt_temporal_frame_ctx)
    // Context-scoped synchronisation (no hipDeviceSynchronize, no synchronous copy on the legacy
    // default stream): ev_done is recorded after the last work this context enqueued (a pass ends
    // with it on the stream that finishes the pass: the caller's, or the finalize stream, which the
    // lanes join); the synchronous entry points wait for that event alone and move data on io_stream,
    // a non-blocking stream of their own.  So reading one context's image does not wait for another
    // context's passes, nor for unrelated work elsewhere on the GPU.
    hipStream_t io_stream = nullptr;
    hipEvent_t ev_done = nullptr;
    bool done_recorded = false;
    hipStream_t done_stream = nullptr;   // the stream ev_done was last recorded on
    hipEvent_t ev_fin[2] = {};           // the finalize of each colour half of a batched pass
    int last_fin = -1;
    // Variance tracking (pt_track_variance, world == 1): luminance moments of the accumulator's batch means.
    pt_moments* mom = nullptr;
    // Adaptive sampling (pt_adaptive_enable): the per-block state, and the effective masks
    // the first bounce reads while enabled (word b = act[b] ? camera mask b : 0).
    pt_adaptive* ad = nullptr;
    uint32_t* ad_cmask = nullptr;
    int32_t ad_active = 0;
    // First-hit planes gA | gB | alb (12 floats per pixel) of whichever of the two is on: their albedo demodulates
    // the moments.  Filled at the first demodulated update after the feature starts or the accumulator is rebased.
    float* planes = nullptr;
    bool planes_valid = false;
    void release();   // both features off, their state freed (pt_ctx_image.cpp)
    // pt_preview_exr's first-hit planes gA | gB | alb | uv (14 floats per pixel), from its first call with a layer
    // other than the beauty until the context is destroyed.
    float* exr_planes = nullptr;
    ~CtxHead();       // (pt_ctx_image.cpp)
};

// Synchronous copy on the context's own non-blocking stream (CtxHead::io_stream): unlike hipMemcpy,
// which runs on the legacy default stream, it waits for nothing but itself.
inline hipError_t io_copy(CtxHead* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (!c->io_stream) return hipMemcpy(dst, src, bytes, kind);   // (pt_create, before the stream exists)
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->io_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->io_stream);
    return e;
}

// Wait for everything this context has enqueued so far (CtxHead::ev_done).
inline int wait_ctx(CtxHead* c) {
    if (c->done_recorded) HIP_TRY(hipEventSynchronize(c->ev_done));
    return PT_OK;
}
inline int mark_ctx(CtxHead* c, hipStream_t s) {
    HIP_TRY(hipEventRecord(c->ev_done, s));
    c->done_recorded = true;
    c->done_stream = s;
    return PT_OK;
}
// Work about to be queued on st that shares the context's path buffers, control words or ahead
// buffers waits for everything the context queued before, when that went to another stream (on
// the same stream, stream order already holds).
inline int order_after_ctx(CtxHead* c, hipStream_t st) {
    if (c->done_recorded && c->done_stream != st) HIP_TRY(hipStreamWaitEvent(st, c->ev_done, 0));
    return PT_OK;
}
// Work on `st` that reads or writes the image first waits for this context's last enqueued work
// (the last deferred finalize of a batched pass, or an image call on another stream), and is then
// itself the work the synchronous entry points wait for (mark_ctx).
inline int wait_finalize(CtxHead* c, hipStream_t st) {
    if (c->done_recorded) HIP_TRY(hipStreamWaitEvent(st, c->ev_done, 0));
    else if (c->last_fin >= 0) HIP_TRY(hipStreamWaitEvent(st, c->ev_fin[c->last_fin], 0));
    return PT_OK;
}

// pt_kernels.hip, for pt_ctx_image.cpp:
CtxHead* ctx_head(pt_ctx* ctx);   // (null for null)
// Before an adaptive context's masks change: the first-bounce kernels of its queued passes read them, and a
// render-ahead iteration traced through the old masks must not be claimed (dropped, as after a flag change).
int adaptive_quiesce(pt_ctx* ctx);
const char* adaptive_refusal(const pt_ctx* ctx);   // null, or why block masks cannot gate this context's first bounce
struct CameraMasks { const uint32_t* dev; size_t blocks; };   // one word per 64 tile pixels
CameraMasks camera_masks(const pt_ctx* ctx);
// The first bounce reads `masks` (null: the camera masks again); the empty share of the host camera
// masks, gated by act where given, chooses its instantiation.
void point_cmask(pt_ctx* ctx, const uint32_t* masks, const uint32_t* act);
// pt_ctx_image.cpp, for build_cmask: an adaptive context whose camera masks or act changed, with none
// of its work queued: the effective masks, their empty share, and the first bounce reads them.
int adaptive_apply(pt_ctx* ctx);

}  // namespace pt
#pragma GCC visibility pop
