// Radiance HDR encoder on the device (pt_hdr_enc), gfx950: the file of pt_encode_hdr (pt_image.cpp),
// byte for byte, from the float accumulator in device memory.
//
// Pixels.  lin[k] = rgb[k] / samples (one correctly rounded float division: this unit is built with the flags of
// every other unit, no fast-math, no contraction); maxcomp by to_rgbe's `>` order; (double)maxcomp < 1e-32 gives
// four zero bytes; otherwise the bytes are the conversions of lin[k] * scale and e + 128 (see rgbe_of for e and
// scale).  A component's product lies in 0 .. 255.99 whenever it is not negative (it is at most the maximum's), and
// there the byte is the truncation.  A negative component beside a positive maximum is converted out of uint8_t's
// range, which C++ leaves undefined; the file is defined as what the host library's x86 code makes of it, so that
// device and host files stay equal on such input too: R and G go through a packed conversion with saturating
// narrowing (host_u8: 0 for every product in -32768 .. -0), B through a scalar truncation to int32 of which the low
// byte is kept (-3.7 -> -3 -> 253).  The contract covers finite inputs with |lin[k] * scale| < 2^31.  NaN,
// infinities and larger magnitudes are outside it: the host's truncation to int32 is itself out of range there.
// mirror_x: input column x lands at W - 1 - x.
//
// Rows.  W < 8 or W >= 32768: a row is its 4 W RGBE bytes, pixel-interleaved (k_hdr_rgbe<true> writes them behind
// the header and nothing else runs).  Otherwise a row is {2, 2, W >> 8, W & 255} and the coded R, G, B and E planes.
//
// The segment rule (what k_hdr_rle computes) and why it equals rle_channel's sequential loop.  Cut a plane row
// c[0..W) into maximal segments of equal bytes.  A segment of length >= 3 is a run, every other byte a literal; a
// stretch is a maximal interval of literal bytes.
//   (a) The loop's x is always a segment start.  It is at x = 0.  After a run is emitted x is the first byte that
//       differs from the run's, a segment start.  After a literal dump x = r, the first position >= the old x with
//       c[r] == c[r + 1] == c[r + 2] (or W): were r > x not a segment start, c[r - 1] == c[r] with r - 1 >= x (x is a
//       start, so r - 1 >= x) and r - 1 would be an earlier such position.
//   (b) Three equal bytes lie inside one segment, and a segment of length >= 3 has them at its start.  So the first
//       r >= x with three equal bytes is the start of the first run at or after x, [x, r) is a whole stretch (the
//       run before x, if any, ended at x; the bytes between are segments shorter than 3), and the inner
//       `while (c[r] == v)` takes that whole segment.  Without such an r the stretch reaches W.
//   (c) A stretch of n bytes is dumped from its start in pieces of 128: the literal at offset j contributes its own
//       byte, preceded by the count byte min(128, n - j) where j % 128 == 0.  A run of n bytes of value v is emitted
//       from its start in pieces of 127: the byte at offset j contributes {128 + min(127, n - j), v} where
//       j % 127 == 0 and nothing otherwise.  A byte's output position is the sum of the contributions before it.
// Bound: a plane row takes at most W + ceil(W / 128) bytes.  A run of n >= 3 costs 2 ceil(n / 127) <= n - 1 (n = 3:
// 2; n >= 4: 2 ceil(n / 127) <= 2 n / 127 + 2 <= n - 1).  A stretch of n costs n + ceil(n / 128) =
// n + 1 + floor((n - 1) / 128).  A row of m stretches n_1 .. n_m (s bytes together) and q runs has q >= m - 1, a run
// lying between two stretches, so it costs at most W - q + m + floor((s - m) / 128): W for m = 0, and for m >= 1 at
// most W + 1 + floor((W - 1) / 128) = W + ceil(W / 128).  Asserted over every row of tests/test_hdr_enc_cpu.py.
//
// Kernel shape: no inter-workgroup wait, no co-resident grid, no look-back, no atomics (one writer per byte); the
// prefix sum and the host side of the object are the shared unit's (pt_enc.h).
//   k_hdr_rgbe        the accumulator (streamed once, non-temporal loads) to four byte planes, a lane converting
//                     four consecutive output pixels and storing one word per plane
//   k_hdr_rle<false>  one wave per (row, plane), the four waves of a workgroup taking a row's four planes: the wave
//                     steps over the plane row 64 bytes at a time, a byte per lane, and sums the contributions
//   scan              pt::scan_exclusive_i32 over the 4 H lengths (the row marker's 4 bytes charged to plane 0)
//   k_hdr_rle<true>   the same stepping; the bytes go to the file, then the header and the size word
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "pt_enc.h"

using namespace pt;

namespace {

constexpr int kStages = 4;      // convert, count, scan, emit (pt_hdr_enc_profile)
constexpr int kHeadMax = 160;   // pt_encode_hdr's buffer

struct Geo {
    int W, H, pitch;            // pitch: bytes between the rows of a plane, a multiple of 4
    int mirror, head;           // head: the header's length
};

// to_rgbe's (uint8_t)(lin[k] * scale) as the host library computes it for R and G: a truncation to int32 (cvttps2dq)
// narrowed by two unsigned-saturating packs of signed 16-bit words (packuswb), each half of the int32 on its own.
// For 0 <= x <= 255 that is x; a negative x down to -32768 gives 0.  (B: cvttss2si and the low byte.)
__device__ __forceinline__ uint32_t host_u8(float v) {
    const int x = (int)v, lo = (int)(short)x, hi = x >> 16;
    const int b0 = min(max(lo, 0), 255), b1 = min(max(hi, 0), 255);   // the first pack: the bytes of the word b0 | b1 << 8
    return (uint32_t)(b1 >= 128 ? 0 : (b1 ? 255 : b0));                // the second: that word, signed, saturated
}

// to_rgbe (pt_image.cpp) of one pixel, r | g << 8 | b << 16 | e << 24.  maxcomp >= 1e-32 is a normal float (1e-32 is
// far above FLT_MIN), so frexp's exponent e is its biased exponent - 126, read from the bit pattern, and
// scale = mant * 256 / maxcomp = 2^(8 - e) exactly (mant * 256 is exact, and the quotient of maxcomp 2^-e 2^8 by
// maxcomp is a power of two in the normal range: 8 - e lies in -120 .. 113), built from its bit pattern as well.
__device__ __forceinline__ uint32_t rgbe_of(float r, float g, float b) {
    const float m = g > b ? g : b;
    const float maxcomp = r > m ? r : m;
    if ((double)maxcomp < 1e-32) return 0u;   // (false for NaN, as on the host)
    const int biased = (int)(__float_as_uint(maxcomp) >> 23) & 255;
    const float scale = __uint_as_float((uint32_t)(261 - biased) << 23);   // 2^(8 - e), e = biased - 126
    const uint32_t br = host_u8(r * scale), bg = host_u8(g * scale), bb = (uint32_t)(int)(b * scale) & 255u,
                   be = (uint32_t)(biased + 2) & 255u;   // e + 128
    return br | (bg << 8) | (bb << 16) | (be << 24);
}

__device__ __forceinline__ uint32_t pixel_rgbe(const float* __restrict__ rgb, float n, const Geo& g, int y, int X) {
    const float* p = rgb + 3 * ((size_t)y * g.W + (g.mirror ? g.W - 1 - X : X));
    const float r = __builtin_nontemporal_load(p), gg = __builtin_nontemporal_load(p + 1), b = __builtin_nontemporal_load(p + 2);
    return rgbe_of(r / n, gg / n, b / n);
}

// FLAT: the interleaved pixels straight behind the header in the file, with the header and the size word (`total`,
// known on the host); otherwise the planes (plane k at planes + k * pitch * H).
template <bool FLAT>
__global__ __launch_bounds__(256) void k_hdr_rgbe(const float* __restrict__ rgb, float n, Geo g, uint8_t* __restrict__ planes,
                                                   const uint8_t* __restrict__ head, uint8_t* __restrict__ out, long long cap,
                                                   long long total, long long* __restrict__ size) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    if (FLAT) {
        const long long npix = (long long)g.W * g.H;
        for (long long i = gid; i < npix; i += stride) {
            const int y = (int)(i / g.W), X = (int)(i - (long long)y * g.W);
            const uint32_t v = pixel_rgbe(rgb, n, g, y, X);
            const long long at = g.head + 4 * i;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (at + k < cap) out[at + k] = (uint8_t)(v >> (8 * k));
        }
        if (gid < g.head && gid < cap) out[gid] = head[gid];
        if (gid == 0) *size = total <= cap ? total : -total;
    } else {
        const int groups = g.pitch / 4;
        const size_t plane = (size_t)g.pitch * g.H;
        const long long items = (long long)groups * g.H;
        for (long long i = gid; i < items; i += stride) {
            const int y = (int)(i / groups), X0 = 4 * (int)(i - (long long)y * groups);
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (X0 + q >= g.W) break;
                const uint32_t v = pixel_rgbe(rgb, n, g, y, X0 + q);
#pragma unroll
                for (int k = 0; k < 4; ++k) w[k] |= ((v >> (8 * k)) & 255u) << (8 * q);
            }
            uint8_t* o = planes + (size_t)y * g.pitch + X0;
#pragma unroll
            for (int k = 0; k < 4; ++k) *reinterpret_cast<uint32_t*>(o + k * plane) = w[k];
        }
    }
}

// What a wave carries from one step of a plane row to the next (wave-uniform).
struct Carry {
    int seg_len = 0;     // bytes so far of the segment that is open at the step's first byte
    int seg_run = 0;     // that segment is a run (known at its start: the loads reach two bytes ahead)
    int stretch = 0;     // bytes so far of the open stretch (0 behind a run byte)
    int last = -1;       // the byte before the step (-1 before the row)
    int off = 0;         // the plane row's output bytes so far
};

// The bytes d = 1..3 positions ahead of a lane's: the step's (cur) or the next step's (nxt), -1 beyond the row.
__device__ __forceinline__ int ahead(int cur, int nxt, int lane, int d) {
    const int src = (lane + d) & 63, a = __shfl(cur, src, 64), b = __shfl(nxt, src, 64);
    return lane + d < 64 ? a : b;
}

// One wave per (row, plane), by the segment rule above.  A step takes 64 consecutive bytes, one per lane, and the
// next 64 are already loaded (they are the following step's, and the two bytes past the step that classify a
// segment starting at its last lanes).  Ballots give the segment starts (S: differs from the previous byte) and
// their class (T: three equal from here); a lane finds its segment's start as the highest start at or below it
// and its stretch's start behind the highest run byte below it (clz of the masked ballot), or in the carried state
// where the step has none.  Contributions are 0, 1 or 2, so the wave's exclusive prefix is two popcounts.  No lane
// walks bytes in a dependent loop.
// EMIT: a count byte depends on how long its stretch or run turns out to be, so the lane that completes a piece
// writes it: offset % 128 == 127 of a stretch, % 127 == 126 of a run, or the last byte of the stretch or segment.
// The piece's first byte lies a known distance back (every run byte but a piece's first contributes nothing, every
// literal exactly its own byte).  One writer per byte, every store guarded by cap.
// len: !EMIT the lengths out, EMIT their exclusive scan; tot: the sum (EMIT).
template <bool EMIT>
__global__ __launch_bounds__(256) void k_hdr_rle(const uint8_t* __restrict__ planes, Geo g, int32_t* __restrict__ len,
                                                  const int32_t* __restrict__ tot, const uint8_t* __restrict__ head,
                                                  uint8_t* __restrict__ out, long long cap, long long* __restrict__ size) {
    const int lane = (int)threadIdx.x & 63, k = (int)threadIdx.x >> 6, W = g.W;
    const unsigned long long lt = (1ull << lane) - 1ull, le = lt | (1ull << lane);
    auto put = [&](long long at, int byte) {
        if (at < cap) out[at] = (uint8_t)byte;
    };
    for (int y = (int)blockIdx.x; y < g.H; y += (int)gridDim.x) {
        const uint8_t* c = planes + ((size_t)k * g.H + y) * g.pitch;
        long long base_at = 0;
        if (EMIT) {
            base_at = (long long)g.head + len[4 * y + k];
            if (k == 0) {   // the row marker, charged to plane 0
                if (lane < 4) put(base_at + lane, lane < 2 ? 2 : (lane == 2 ? (W >> 8) & 255 : W & 255));
                base_at += 4;
            }
        }
        Carry st;
        int nxt = lane < W ? (int)c[lane] : -1;
        for (int base = 0; base < W; base += 64) {
            const int cur = nxt, i = base + lane;
            nxt = i + 64 < W ? (int)c[i + 64] : -1;
            const int nvalid = min(64, W - base);
            const bool valid = cur >= 0;
            int prev = __shfl(cur, (lane - 1) & 63, 64);
            if (lane == 0) prev = st.last;
            const int b1 = ahead(cur, nxt, lane, 1), b2 = ahead(cur, nxt, lane, 2);
            const int b3 = EMIT ? ahead(cur, nxt, lane, 3) : -1;   // (every lane takes part in a shuffle: none in a branch)
            const unsigned long long S = __ballot(valid && cur != prev), T = __ballot(valid && cur == b1 && cur == b2);
            // the lane's segment: its class and the lane's offset in it
            const unsigned long long sb = S & le;
            int run, j;
            if (sb) {
                const int ps = 63 - __clzll((long long)sb);
                run = (int)(T >> ps) & 1;
                j = lane - ps;
            } else {
                run = st.seg_run;
                j = st.seg_len + lane;
            }
            // the lane's stretch: its offset in it (literals only)
            const unsigned long long Lm = __ballot(valid && !run), zb = ~Lm & lt;
            const int sj = zb ? lane - (64 - __clzll((long long)zb)) : st.stretch + lane;
            int cnt = 0, jj = 0;
            if (valid) {
                jj = run ? j % 127 : sj % 128;
                cnt = run ? (jj == 0 ? 2 : 0) : (jj == 0 ? 2 : 1);
            }
            const unsigned long long B1 = __ballot(cnt == 1), B2 = __ballot(cnt == 2);
            if (EMIT && valid) {
                const long long pos = base_at + st.off + __popcll(B1 & lt) + 2 * __popcll(B2 & lt);
                if (run) {
                    if (jj == 126 || b1 != cur) {   // completes a run piece of jj + 1 bytes
                        const long long cp = jj == 0 ? pos : pos - 2;
                        put(cp, 128 + jj + 1);
                        put(cp + 1, cur);
                    }
                } else {
                    const long long own = pos + (jj == 0 ? 1 : 0);
                    put(own, cur);
                    // the stretch ends here: the row does, or the next byte starts a run
                    const bool ends = b1 < 0 || (b1 != cur && b1 == b2 && b1 == b3);
                    if (jj == 127 || ends) put(own - 1 - jj, jj + 1);
                }
            }
            // the state behind the step's last byte
            const int lastl = nvalid - 1;
            if (S) {
                const int ps = 63 - __clzll((long long)S);
                st.seg_len = nvalid - ps;
                st.seg_run = (int)(T >> ps) & 1;
            } else {
                st.seg_len += nvalid;
            }
            const unsigned long long vm = nvalid == 64 ? ~0ull : (1ull << nvalid) - 1ull, za = ~Lm & vm;
            st.stretch = za ? lastl - (63 - __clzll((long long)za)) : st.stretch + nvalid;
            st.last = __shfl(cur, lastl, 64);
            st.off += __popcll(B1) + 2 * __popcll(B2);
        }
        if (!EMIT && lane == 0) len[4 * y + k] = st.off + (k == 0 ? 4 : 0);
    }
    if (EMIT && blockIdx.x == 0) {
        for (int i = (int)threadIdx.x; i < g.head; i += 256) put(i, head[i]);
        if (threadIdx.x == 0) {
            const long long total = (long long)g.head + tot[0];
            *size = total <= cap ? total : -total;
        }
    }
}

}  // namespace

struct pt_hdr_enc : EncHead {
    pt_hdr_enc() : EncHead("HDR", "hdr", kStages) {}
    Geo geo{};
    bool flat = false;
    int64_t bound = 0;
    uint8_t head[kHeadMax] = {};
    // The device side: head | the four planes | the 4 H lengths (then offsets) | scan tile sums | the total.
    uint8_t *d_head = nullptr, *d_planes = nullptr;
    int32_t *d_len = nullptr, *d_sums = nullptr, *d_tot = nullptr;
};

const EncHead* pt::enc_head(const pt_hdr_enc* e) { return e; }

namespace {

int he_alloc(pt_hdr_enc* e) {
    if (e->dev) return PT_OK;
    const Geo& g = e->geo;
    const size_t n = e->flat ? 0 : 4 * (size_t)g.H;
    uint8_t* p[5];
    if (int rc = enc_alloc(e, {sizeof(e->head), e->flat ? 16 : 4 * (size_t)g.pitch * g.H, n * 4 + 16, (n / kScanTile + 1) * 4, 256},
                           p, e->head, "header"))
        return rc;
    e->d_head = p[0];
    e->d_planes = p[1];
    e->d_len = (int32_t*)p[2];
    e->d_sums = (int32_t*)p[3];
    e->d_tot = (int32_t*)p[4];
    return PT_OK;
}

int encode(pt_hdr_enc* e, const float* d_rgb, float samples, uint8_t* d_out, int64_t cap, int64_t* d_size, hipStream_t st) {
    if (int rc = he_alloc(e)) return rc;
    const Geo& g = e->geo;
    if (int rc = enc_stage(e, 0, st)) return rc;
    if (e->flat) {
        hipLaunchKernelGGL(k_hdr_rgbe<true>, dim3(grid_of((int64_t)g.W * g.H, 256)), dim3(256), 0, st, d_rgb, samples, g,
                           e->d_planes, (const uint8_t*)e->d_head, d_out, (long long)cap, (long long)e->bound, (long long*)d_size);
        for (int k = 1; k < kStages; ++k)
            if (int rc = enc_stage(e, k, st)) return rc;
        return enc_done(e, st);
    }
    hipLaunchKernelGGL(k_hdr_rgbe<false>, dim3(grid_of((int64_t)(g.pitch / 4) * g.H, 256)), dim3(256), 0, st, d_rgb, samples, g,
                       e->d_planes, (const uint8_t*)e->d_head, d_out, (long long)cap, 0LL, (long long*)d_size);
    if (int rc = enc_stage(e, 1, st)) return rc;
    const int rows = std::min(g.H, 1 << 20);
    hipLaunchKernelGGL(k_hdr_rle<false>, dim3(rows), dim3(256), 0, st, (const uint8_t*)e->d_planes, g, e->d_len,
                       (const int32_t*)e->d_tot, (const uint8_t*)e->d_head, d_out, (long long)cap, (long long*)d_size);
    if (int rc = enc_stage(e, 2, st)) return rc;
    scan_exclusive_i32(e->d_len, 4 * g.H, e->d_sums, e->d_tot, st);
    if (int rc = enc_stage(e, 3, st)) return rc;
    hipLaunchKernelGGL(k_hdr_rle<true>, dim3(rows), dim3(256), 0, st, (const uint8_t*)e->d_planes, g, e->d_len,
                       (const int32_t*)e->d_tot, (const uint8_t*)e->d_head, d_out, (long long)cap, (long long*)d_size);
    return enc_done(e, st);
}

int samples_check(float samples) {
    if (!std::isfinite(samples) || !(samples > 0.0f)) return pt::fail(PT_ERR_ARG, "samples must be finite and > 0");
    return PT_OK;
}

}  // namespace

extern "C" {

void pt_hdr_params_default(pt_hdr_params* p) {
    if (p) *p = pt_hdr_params{};
}

int pt_hdr_enc_create(int32_t width, int32_t height, const pt_hdr_params* p, pt_hdr_enc** out) {
    if (!out || !p) return pt::fail(PT_ERR_ARG, "null argument");
    for (int32_t r : p->reserved)
        if (r != 0) return pt::fail(PT_ERR_ARG, "pt_hdr_params.reserved must be zero");
    if (width < 1 || height < 1) return pt::fail(PT_ERR_ARG, "HDR width and height must be at least 1");
    char head[kHeadMax];
    const int n = std::snprintf(head, sizeof head,
                                "#?RADIANCE\n# Written by stb_image_write.h\nFORMAT=32-bit_rle_rgbe\n"
                                "EXPOSURE=          1.0000000000000\n\n-Y %d +X %d\n", height, width);
    const bool flat = width < 8 || width >= 32768;
    const int64_t W = width, H = height;
    const int64_t bound = n + (flat ? 4 * W * H : H * (4 + 4 * (W + (W + 127) / 128)));
    if (bound >= ((int64_t)1 << 31))   // the byte offsets are int32
        return pt::fail(PT_ERR_ARG, "HDR image too large: the byte offsets of its file must stay below 2^31");
    pt_hdr_enc* e = new pt_hdr_enc;   // (the device side comes with the first encode: he_alloc)
    e->W = width;
    e->H = height;
    e->flat = flat;
    e->bound = bound;
    e->geo = Geo{width, height, (width + 3) & ~3, p->mirror_x ? 1 : 0, n};
    std::copy(head, head + n, e->head);
    *out = e;
    return PT_OK;
}

int pt_hdr_enc_destroy(pt_hdr_enc* e) {
    delete e;   // (~EncHead waits for the last encode)
    return PT_OK;
}

int64_t pt_hdr_enc_bound(const pt_hdr_enc* e) { return e ? e->bound : 0; }

int pt_hdr_enc_accum(pt_hdr_enc* e, const float* d_rgb, float samples, uint8_t* d_out, int64_t cap, int64_t* d_size,
                     void* stream) {
    if (int rc = encode_check(e, d_rgb, d_out, cap, d_size)) return rc;
    if (int rc = samples_check(samples)) return rc;
    return encode(e, d_rgb, samples, d_out, cap, d_size, (hipStream_t)stream);
}

// pt::encode_host is written for byte pixels with a stride; this is its shape for a float array: one object made,
// used and destroyed around a device buffer "size word | accumulator | file".
int pt_hdr_encode_host(int32_t width, int32_t height, const float* rgb, float samples, const pt_hdr_params* p, uint8_t* out,
                       int64_t cap, int64_t* size) {
    if (!rgb || !out || !size) return pt::fail(PT_ERR_ARG, "null argument");
    if (cap < 0) return pt::fail(PT_ERR_ARG, "negative output capacity");
    if (int rc = samples_check(samples)) return rc;
    pt_hdr_enc* e = nullptr;
    if (int rc = pt_hdr_enc_create(width, height, p, &e)) return rc;
    const size_t in_bytes = (size_t)width * height * 3 * sizeof(float);
    const int64_t dcap = std::min(cap, e->bound);
    uint8_t* d = nullptr;
    const size_t o_rgb = 256, o_out = o_rgb + align256(in_bytes);
    if (hipMalloc((void**)&d, o_out + (size_t)dcap + 16) != hipSuccess) {
        (void)hipGetLastError();
        delete e;
        return pt::fail(PT_ERR_NOMEM, "hipMalloc (HDR host encode)");
    }
    int64_t got = 0;
    hipError_t he = hipMemcpy(d + o_rgb, rgb, in_bytes, hipMemcpyHostToDevice);
    int rc = PT_OK;
    if (he == hipSuccess) rc = pt_hdr_enc_accum(e, (const float*)(d + o_rgb), samples, d + o_out, dcap, (int64_t*)d, nullptr);
    if (he == hipSuccess && !rc) he = hipMemcpy(&got, d, sizeof(got), hipMemcpyDeviceToHost);   // (waits for the encode)
    if (he == hipSuccess && !rc && got > 0) he = hipMemcpy(out, d + o_out, (size_t)got, hipMemcpyDeviceToHost);
    delete e;
    (void)hipFree(d);
    if (rc) return rc;
    if (he != hipSuccess) return pt::fail(PT_ERR_HIP, std::string("pt_hdr_encode_host: ") + hipGetErrorString(he));
    *size = got < 0 ? -got : got;
    if (got < 0) return pt::fail(PT_ERR_ARG, "the HDR file needs " + std::to_string(-got) + " bytes");
    return PT_OK;
}

int pt_hdr_enc_profile(pt_hdr_enc* e, int32_t on) {
    if (!e) return pt::fail(PT_ERR_ARG, "null HDR encoder");
    return enc_profile(e, on);
}

int pt_hdr_enc_profile_read(pt_hdr_enc* e, float ms[4]) { return enc_profile_read(e, ms); }

}  // extern "C"
