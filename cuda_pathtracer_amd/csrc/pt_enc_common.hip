// The shared part of the device encoders (pt_enc.h), gfx950: the prefix sum and the host side of an encoder object.
//
// Kernel shape: no inter-workgroup wait, no co-resident grid, no look-back; a prefix sum is the three-kernel
// reduce / one-workgroup scan / apply of k_hist_*, so an encode can run beside render passes on other streams.
#include "pt_enc.h"

namespace pt {
namespace {

__global__ __launch_bounds__(256) void k_scan_reduce(const int32_t* __restrict__ in, int n, int32_t* __restrict__ sums) {
    __shared__ int s_w[4];
    for (int tile = (int)blockIdx.x; tile * kScanTile < n; tile += (int)gridDim.x) {
        const int base = tile * kScanTile + (int)threadIdx.x * kScanPer;
        int v = 0, total;
#pragma unroll
        for (int k = 0; k < kScanPer; ++k) v += base + k < n ? in[base + k] : 0;
        (void)block_excl_scan(v, s_w, &total);
        if (threadIdx.x == 0) sums[tile] = total;
    }
}

// One workgroup: the tile sums scanned in place, their total to *total_out.  With `ntiles_dev` the number of
// tiles is read there (an earlier kernel on the stream stored it).
__global__ __launch_bounds__(256) void k_scan_sums(int32_t* __restrict__ sums, int ntiles, const int32_t* __restrict__ ntiles_dev,
                                                    int32_t* __restrict__ total_out) {
    __shared__ int s_w[4];
    if (ntiles_dev) ntiles = ntiles_dev[0];
    const int per = (ntiles + 255) / 256, j0 = (int)threadIdx.x * per;
    int v = 0, total;
    for (int j = j0; j < j0 + per && j < ntiles; ++j) v += sums[j];
    int run = block_excl_scan(v, s_w, &total);
    for (int j = j0; j < j0 + per && j < ntiles; ++j) {
        const int a = sums[j];
        sums[j] = run;
        run += a;
    }
    if (threadIdx.x == 0) *total_out = total;
}

__global__ __launch_bounds__(256) void k_scan_apply(int32_t* __restrict__ io, int n, const int32_t* __restrict__ sums) {
    __shared__ int s_w[4];
    for (int tile = (int)blockIdx.x; tile * kScanTile < n; tile += (int)gridDim.x) {
        const int base = tile * kScanTile + (int)threadIdx.x * kScanPer;
        int x[kScanPer], v = 0, total;
#pragma unroll
        for (int k = 0; k < kScanPer; ++k) {
            x[k] = base + k < n ? io[base + k] : 0;
            v += x[k];
        }
        int run = block_excl_scan(v, s_w, &total) + sums[tile];
#pragma unroll
        for (int k = 0; k < kScanPer; ++k) {
            if (base + k < n) io[base + k] = run;
            run += x[k];
        }
    }
}

#define ENC_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess)                                                           \
            return fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

}  // namespace

void scan_exclusive_i32(int32_t* io, int n, int32_t* sums, int32_t* total, hipStream_t st) {
    const int tiles = (n + kScanTile - 1) / kScanTile, grid = std::min(tiles, kMaxGrid);
    hipLaunchKernelGGL(k_scan_reduce, dim3(grid), dim3(256), 0, st, (const int32_t*)io, n, sums);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, st, sums, tiles, (const int32_t*)nullptr, total);
    hipLaunchKernelGGL(k_scan_apply, dim3(grid), dim3(256), 0, st, io, n, (const int32_t*)sums);
}

void scan_tile_sums_i32(int32_t* sums, const int32_t* ntiles, int32_t* total, hipStream_t st) {
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, st, sums, 0, ntiles, total);
}

EncHead::~EncHead() {
    if (ev_recorded) (void)hipEventSynchronize(ev);
    if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t v : stage_ev)
        if (v) (void)hipEventDestroy(v);
    if (dev) (void)hipFree(dev);
}

int enc_alloc(EncHead* e, std::initializer_list<size_t> bytes, uint8_t** part, const void* consts, const char* consts_name) {
    size_t total = 0;
    for (size_t b : bytes) total += align256(b);
    if (hipMalloc((void**)&e->dev, total) != hipSuccess ||
        (!e->ev && hipEventCreateWithFlags(&e->ev, hipEventDisableTiming) != hipSuccess)) {
        if (e->dev) (void)hipFree(e->dev);
        e->dev = nullptr;
        (void)hipGetLastError();
        return fail(PT_ERR_NOMEM, std::string("hipMalloc (") + e->name + " encoder scratch)");
    }
    size_t at = 0;
    for (size_t b : bytes) {
        *part++ = e->dev + at;
        at += align256(b);
    }
    const hipError_t he = hipMemcpy(e->dev, consts, *bytes.begin(), hipMemcpyHostToDevice);
    if (he != hipSuccess) {
        (void)hipFree(e->dev);
        e->dev = nullptr;
        return fail(PT_ERR_HIP, std::string("hipMemcpy (") + e->name + " " + consts_name + "): " + hipGetErrorString(he));
    }
    return PT_OK;
}

int enc_stage(EncHead* e, int k, hipStream_t st) {
    if (e->profile) ENC_TRY(hipEventRecord(e->stage_ev[k], st));
    return PT_OK;
}

int enc_done(EncHead* e, hipStream_t st) {
    ENC_TRY(hipGetLastError());
    if (int rc = enc_stage(e, e->stages, st)) return rc;
    ENC_TRY(hipEventRecord(e->ev, st));
    e->ev_recorded = true;
    return PT_OK;
}

int enc_profile(EncHead* e, int32_t on) {
    if (on)
        for (int k = 0; k <= e->stages; ++k)
            if (!e->stage_ev[k]) ENC_TRY(hipEventCreate(&e->stage_ev[k]));
    e->profile = on != 0;
    return PT_OK;
}

int enc_profile_read(EncHead* e, float* ms) {
    if (!e || !ms) return fail(PT_ERR_ARG, "null argument");
    if (!e->profile || !e->ev_recorded)
        return fail(PT_ERR_ARG, std::string("no profiled encode (pt_") + e->tag + "_enc_profile)");
    ENC_TRY(hipEventSynchronize(e->stage_ev[e->stages]));
    for (int k = 0; k < e->stages; ++k) ENC_TRY(hipEventElapsedTime(ms + k, e->stage_ev[k], e->stage_ev[k + 1]));
    return PT_OK;
}

int encode_check(const void* e, const void* src, const uint8_t* d_out, int64_t cap, const int64_t* d_size) {
    if (!e || !src || !d_out || !d_size) return fail(PT_ERR_ARG, "null argument");
    if (cap < 0) return fail(PT_ERR_ARG, "negative output capacity");
    return PT_OK;
}

void enc_size(const EncHead* e, int32_t* width, int32_t* height) {
    *width = e->W;
    *height = e->H;
}

}  // namespace pt
