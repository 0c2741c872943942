// What the device encoders (pt_jpeg_enc.hip, pt_png_enc.hip) share, defined in pt_enc_common.hip:
// the accumulator's byte conversions, the workgroup scan and the three-kernel prefix sum, and the host side of an
// encoder object: its scratch, completion event, stage profile and argument checks.  No global state: everything
// hangs off the object.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "pt_internal.h"

namespace pt {

constexpr int kScanPer = 4, kScanTile = 256 * kScanPer;   // values per lane and per workgroup of the scan kernels
constexpr int kMaxGrid = 1024;                            // grid-stride kernels: workgroups at most
constexpr int kEncStagesMax = 6;

// ---- device ---------------------------------------------------------------------------------------------
// Restatements (pt_kernels.hip and pt_image.cpp are not touched): k_preview's byte of an accumulator value
__device__ __forceinline__ int preview_byte(float v, float n) {
    int q = (int)((double)(v / n) * 255.0);
    return q < 0 ? 0 : (q > 255 ? 255 : q);
}
// and pt_tonemap's
__device__ __forceinline__ int save_byte(float v, float n) {
    v = v / n;
    v = v > 0.0f ? v : 0.0f;
    v = v < 1.0f ? v : 1.0f;
    return (int)(uint8_t)(v * 255.f);
}

// Exclusive scan of one value per lane over a workgroup of 256 (every lane calls it; s_w: 4 words of LDS);
// *total: the workgroup's sum.
__device__ __forceinline__ int block_excl_scan(int v, int* s_w, int* total) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    __syncthreads();   // (s_w may still be read by the previous call)
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int base = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int t = s_w[k];
        if (k < wave) base += t;
        sum += t;
    }
    *total = sum;
    return base + inc - v;
}

// ---- prefix sums ----------------------------------------------------------------------------------------
// Three launches on st, no inter-workgroup wait: io[0..n) becomes its exclusive scan, *total its sum.
// sums: n / kScanTile + 1 words of scratch.
void scan_exclusive_i32(int32_t* io, int n, int32_t* sums, int32_t* total, hipStream_t st);
// One launch: sums[0..*ntiles), tile sums that another kernel reduced (*ntiles is read on the device), become
// their exclusive scan and *total their sum.
void scan_tile_sums_i32(int32_t* sums, const int32_t* ntiles, int32_t* total, hipStream_t st);

// ---- host -----------------------------------------------------------------------------------------------
// What every encoder object begins with.  name, tag: "JPEG", "jpeg" (messages); stages: those of its profile.
struct EncHead {
    const char *name, *tag;
    const int stages;
    int32_t W = 0, H = 0;
    uint8_t* dev = nullptr;           // the device side, one allocation made at the first encode (enc_alloc)
    hipEvent_t ev = nullptr;          // after the last queued work (the destructor waits for it)
    bool ev_recorded = false;
    bool profile = false;             // enc_profile: events around the stages of the last encode
    hipEvent_t stage_ev[kEncStagesMax + 1] = {};
    EncHead(const char* name_, const char* tag_, int stages_) : name(name_), tag(tag_), stages(stages_) {}
    EncHead(const EncHead&) = delete;
    ~EncHead();                       // waits for the last encode, then frees the events and the scratch
};

// e->dev and the completion event: one allocation of the parts of `bytes`, each aligned to 256, their addresses
// to part[]; `consts` (as many bytes as the first part) is uploaded there, synchronously, once per object: a later
// encode on any stream reads it.  On any failure nothing is kept: the next encode allocates and uploads again.
int enc_alloc(EncHead* e, std::initializer_list<size_t> bytes, uint8_t** part, const void* consts, const char* consts_name);
int enc_stage(EncHead* e, int k, hipStream_t st);   // the mark before stage k (after the last: k = stages)
int enc_done(EncHead* e, hipStream_t st);           // behind an encode's launches: their error, the last mark, the event
int enc_profile(EncHead* e, int32_t on);
int enc_profile_read(EncHead* e, float* ms);
// The arguments of an encode; touches no device.
int encode_check(const void* e, const void* src, const uint8_t* d_out, int64_t cap, const int64_t* d_size);

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int grid_of(int64_t items, int per) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + per - 1) / per, kMaxGrid)); }

// pt_*_encode_host: one object made, used and destroyed around a device buffer "size word | pixels | file".
template <class Enc, class Prm>
int encode_host(int (*create)(int32_t, int32_t, const Prm*, Enc**), int64_t (*bound)(const Enc*),
                int (*pixels)(Enc*, const uint8_t*, int32_t, uint8_t*, int64_t, int64_t*, void*), int32_t width, int32_t height,
                const uint8_t* pix, int32_t pixel_stride, const Prm* p, uint8_t* out, int64_t cap, int64_t* size) {
    if (!pix || !out || !size) return fail(PT_ERR_ARG, "null argument");
    if (cap < 0) return fail(PT_ERR_ARG, "negative output capacity");
    if (pixel_stride != 3 && pixel_stride != 4) return fail(PT_ERR_ARG, "the pixel stride must be 3 or 4");
    Enc* e = nullptr;
    if (int rc = create(width, height, p, &e)) return rc;
    const std::string name = e->name, who = std::string("pt_") + e->tag + "_encode_host: ";
    const size_t in_bytes = (size_t)width * height * pixel_stride;
    const int64_t dcap = std::min(cap, bound(e));
    uint8_t* d = nullptr;
    const size_t o_pix = 256, o_out = o_pix + align256(in_bytes);
    if (hipMalloc((void**)&d, o_out + (size_t)dcap + 16) != hipSuccess) {
        (void)hipGetLastError();
        delete e;
        return fail(PT_ERR_NOMEM, "hipMalloc (" + name + " host encode)");
    }
    int64_t got = 0;
    hipError_t he = hipMemcpy(d + o_pix, pix, in_bytes, hipMemcpyHostToDevice);
    int rc = PT_OK;
    if (he == hipSuccess) rc = pixels(e, d + o_pix, pixel_stride, d + o_out, dcap, (int64_t*)d, nullptr);
    if (he == hipSuccess && !rc) he = hipMemcpy(&got, d, sizeof(got), hipMemcpyDeviceToHost);   // (waits for the encode)
    if (he == hipSuccess && !rc && got > 0) he = hipMemcpy(out, d + o_out, (size_t)got, hipMemcpyDeviceToHost);
    delete e;
    (void)hipFree(d);
    if (rc) return rc;
    if (he != hipSuccess) return fail(PT_ERR_HIP, who + hipGetErrorString(he));
    *size = got < 0 ? -got : got;
    if (got < 0) return fail(PT_ERR_ARG, "the " + name + " file needs " + std::to_string(-got) + " bytes");
    return PT_OK;
}

}  // namespace pt
