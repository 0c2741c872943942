// OpenEXR encoder on the device (pt_exr_enc), gfx950: a single-part scanline OpenEXR 2.0 file of 1 to 16
// HALF, FLOAT or UINT channels read from float planes in device memory, uncompressed or with ZIPS / ZIP compression (one
// zlib stream per 1 / 16 scanlines, or the raw bytes where the stream is not shorter).  §18 is the definition of the file;
// tests/exr_ref.py restates it and the GPU tests compare byte for byte.  Every step is an integer operation but the one
// float division of a value by its plane's divisor (correctly rounded: no fast-math, no contraction).
//
// A stream's bytes p are coded by §15's run-length deflate (pt_deflate_dev.h), every stream on its own: lane chunks and
// deflate blocks are counted from the stream's first byte, and a run never reaches into another stream.
//
// Kernel shape: no inter-workgroup wait, no co-resident grid, no look-back.  The scratch holds one slot per EXR chunk
// (stream) in T, P and S, each a multiple of 16 bytes apart.
//   k_exr_convert     a lane takes 4 consecutive pixels of one channel row (one 16-byte load where the plane allows it),
//                     converts them, and stores the value bytes: NONE straight to the file, whose positions the host knows
//                     (with the chunk heads, the offset table, the header and the size word: nothing else runs); otherwise
//                     to the even and odd halves of the stream's t in T
//   k_exr_diff        p = t - left neighbour + 128, a lane per 16 bytes of a stream: T to P
//   k_exr_block       one wave per deflate block of every stream (deflate_block)
//   k_exr_scan        a workgroup per stream: the exclusive scan of its chunk bit lengths, its size z and the raw fallback
//   k_exr_zero        the words of every coded stream's slot in S up to its length (the zlib header in the first)
//   k_exr_emit        one wave per deflate block (deflate_emit); streams that fall back to raw bytes are skipped
//   k_exr_adler_*     per 4096 bytes of p; a workgroup per stream combines them behind the stream
//   scan              pt::scan_exclusive_i32 over the chunk sizes: the offset table
//   k_exr_out         every chunk behind the table, a lane per 4 bytes: the stream's, or the raw bytes put together again
//                     from T's halves; then the table, the header and the size word.  Byte stores: a chunk starts anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pt_deflate_dev.h"
#include "pt_enc.h"

using namespace pt;
using namespace pt::deflate;

namespace {

constexpr int kStages = 6;       // convert, block, scan, emit, checksums and sizes, out (pt_exr_enc_profile)
constexpr int kMaxChan = 16;
constexpr int kHeadMax = 1280;   // magic 8, chlist 21 + 16 * 49, the seven other attributes 225, the end
constexpr int kPer = 4;          // pixels of a channel row per lane of k_exr_convert

struct Chan {
    const float* d;              // the plane
    int32_t stride;              // floats between its pixels
    float div;
    int32_t type, bpv, coff;     // PT_EXR_*; bytes per value; the channel row's offset in a scanline's bytes
    int32_t pad;
};
struct Planes { Chan c[kMaxChan]; };

struct Geo {
    int W, H, nch, L;            // L: scanlines per chunk
    int LB;                      // bytes of a scanline
    int nchunks, nfull, nlast;   // n of every chunk but the last, and of the last
    int mirror, comp, block_bytes;
    int cps, bps, pps;           // lane chunks, deflate blocks and Adler pieces of a stream of nfull bytes
    int pitch, spitch;           // bytes between the streams' slots in T and P, and in S
    int head;                    // the header's length
};

__device__ __forceinline__ int stream_bytes(const Geo& g, int j) { return j == g.nchunks - 1 ? g.nlast : g.nfull; }

// §18's HALF: IEEE round to nearest even of a float's bits; subnormal halves, overflow to infinity, NaN to sign | 0x7e00.
__device__ __forceinline__ uint32_t half_bits(uint32_t f) {
    const uint32_t sign = (f >> 16) & 0x8000u, a = f & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7e00u;
    if (a >= 0x477ff000u) return sign | 0x7c00u;   // 65520, the midpoint of 65504 and 2^16, goes to the even side: infinity
    if (a >= 0x38800000u) {                        // a normal half: the exponent rebiased, 13 bits rounded away
        const uint32_t v = a - 0x38000000u;
        return sign | ((v + 0xfffu + ((v >> 13) & 1u)) >> 13);
    }
    if (a <= 0x33000000u) return sign;             // up to 2^-25, the midpoint of 0 and the smallest subnormal
    const int shift = 126 - (int)(a >> 23);        // 14 .. 24: the value in units of 2^-24
    const uint32_t mant = (a & 0x7fffffu) | 0x800000u, m = mant >> shift, rem = mant & ((1u << shift) - 1u),
                   halfway = 1u << (shift - 1);
    return sign | (m + ((rem > halfway || (rem == halfway && (m & 1u))) ? 1u : 0u));
}

// nb = 4 or 8 bytes (fewer at a row's end) of v to p, by words where p is aligned.
__device__ __forceinline__ void store_bytes(uint8_t* p, uint64_t v, int nb) {
    if ((nb & 3) == 0 && ((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)v;
        if (nb == 8) *reinterpret_cast<uint32_t*>(p + 4) = (uint32_t)(v >> 32);
    } else {
        for (int i = 0; i < nb; ++i) p[i] = (uint8_t)(v >> (8 * i));
    }
}

// NONE: the whole file.  Otherwise T.  Every store to out is guarded by cap.
template <bool NONE>
__global__ __launch_bounds__(256) void k_exr_convert(Planes pl, Geo g, uint8_t* __restrict__ T, const uint8_t* __restrict__ head,
                                                      uint8_t* __restrict__ out, long long cap, long long total,
                                                      long long* __restrict__ size) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    const int groups = (g.W + kPer - 1) / kPer;
    const long long items = (long long)g.H * g.nch * groups;
    for (long long i = gid; i < items; i += step) {
        const int grp = (int)(i % groups);
        const long long t = i / groups;
        const int k = (int)(t % g.nch), y = (int)(t / g.nch);
        const Chan ch = pl.c[k];
        const int x0 = grp * kPer, cnt = min(kPer, g.W - x0);
        uint32_t v[kPer] = {0u, 0u, 0u, 0u};
        const uint32_t* src = reinterpret_cast<const uint32_t*>(ch.d);
        const size_t row = (size_t)y * g.W;
        if (!g.mirror && cnt == kPer && ch.stride == 1 && (((uintptr_t)(src + row + x0)) & 15) == 0) {
            const uint4 q = *reinterpret_cast<const uint4*>(src + row + x0);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
            for (int q = 0; q < kPer; ++q)
                if (q < cnt) v[q] = src[(row + (g.mirror ? g.W - 1 - (x0 + q) : x0 + q)) * (size_t)ch.stride];
        }
        if (ch.type != PT_EXR_UINT) {
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                if (ch.div != 1.0f) v[q] = __float_as_uint(__uint_as_float(v[q]) / ch.div);
                if (ch.type == PT_EXR_HALF) v[q] = half_bits(v[q]);
            }
        }
        if (NONE) {   // L = 1: chunk y is the table's 8 nchunks bytes, y chunks of 8 + LB and its own head behind the header
            const long long at0 = (long long)g.head + 8LL * g.nchunks + (long long)y * (8 + g.LB);
            long long at = at0 + 8 + ch.coff + (long long)x0 * ch.bpv;
            for (int q = 0; q < cnt; ++q)
                for (int b = 0; b < ch.bpv; ++b, ++at)
                    if (at < cap) out[at] = (uint8_t)(v[q] >> (8 * b));
            if (k == 0 && grp == 0) {
                const uint32_t w[4] = {(uint32_t)y, (uint32_t)g.LB, (uint32_t)at0, (uint32_t)((unsigned long long)at0 >> 32)};
                for (int b = 0; b < 8; ++b) {
                    const long long hp = at0 + b, tp = (long long)g.head + 8LL * y + b;
                    if (hp < cap) out[hp] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
                    if (tp < cap) out[tp] = (uint8_t)(w[2 + (b >> 2)] >> (8 * (b & 3)));
                }
            }
        } else {
            const int j = y / g.L, half = stream_bytes(g, j) >> 1;
            const int e = ((y - j * g.L) * g.LB + ch.coff + x0 * ch.bpv) >> 1;   // (a value starts at an even byte)
            uint64_t ev = 0, od = 0;
            if (ch.bpv == 2) {
#pragma unroll
                for (int q = 0; q < kPer; ++q) {
                    ev |= (uint64_t)(v[q] & 255u) << (8 * q);
                    od |= (uint64_t)((v[q] >> 8) & 255u) << (8 * q);
                }
            } else {
#pragma unroll
                for (int q = 0; q < kPer; ++q) {
                    ev |= (uint64_t)((v[q] & 255u) | ((v[q] >> 8) & 0xff00u)) << (16 * q);
                    od |= (uint64_t)(((v[q] >> 8) & 255u) | ((v[q] >> 16) & 0xff00u)) << (16 * q);
                }
            }
            uint8_t* t0 = T + (size_t)j * g.pitch + e;
            const int nb = cnt * (ch.bpv >> 1);
            store_bytes(t0, ev, nb);
            store_bytes(t0 + half, od, nb);
        }
    }
    if (NONE) {
        if (gid < g.head && gid < cap) out[gid] = head[gid];
        if (gid == 0) *size = total <= cap ? total : -total;
    }
}

__global__ __launch_bounds__(256) void k_exr_diff(const uint8_t* __restrict__ T, Geo g, uint8_t* __restrict__ P) {
    const int per = g.pitch / 16;
    const long long items = (long long)g.nchunks * per;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const int j = (int)(i / per), i0 = 16 * (int)(i % per);
        if (i0 >= stream_bytes(g, j)) continue;
        const uint8_t* t = T + (size_t)j * g.pitch;
        const uint4 q = *reinterpret_cast<const uint4*>(t + i0);   // (the slots are padded to 16 bytes)
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        uint32_t prev = i0 ? t[i0 - 1] : 128u;                     // p[0] = t[0]
        uint32_t o[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            o[a] = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t cur = (w[a] >> (8 * b)) & 255u;
                o[a] |= ((cur - prev + 128u) & 255u) << (8 * b);
                prev = cur;
            }
        }
        *reinterpret_cast<uint4*>(P + (size_t)j * g.pitch + i0) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// Deflate block b of the grid is block b % bps of stream b / bps; the last stream may have fewer: false then.
__device__ __forceinline__ bool block_range(const Geo& g, int b, int& j, int& n, int& c0, int& c1, int& last) {
    j = b / g.bps;
    const int lb = b - j * g.bps;
    n = stream_bytes(g, j);
    const int nblk = (n + g.block_bytes - 1) / g.block_bytes, per = g.block_bytes / kChunk;
    c0 = lb * per;
    c1 = min(c0 + per, (n + kChunk - 1) / kChunk);
    last = j * g.bps + nblk - 1;   // the stream's last block, in the grid's numbering
    return lb < nblk;
}

__global__ __launch_bounds__(64) void k_exr_block(const uint8_t* __restrict__ P, Geo g, uint32_t* __restrict__ tabs,
                                                   uint32_t* __restrict__ hdrs, int32_t* __restrict__ len) {
    const int b = (int)blockIdx.x;
    int j, n, c0, c1, last;
    if (!block_range(g, b, j, n, c0, c1, last)) return;
    deflate_block(P + (size_t)j * g.pitch, n, c0, c1, b, last, tabs, hdrs, len + (size_t)j * g.cps);
}

// A stream's chunk bit lengths become their exclusive scan; bits[j]: their sum; dsize[j]: the chunk's data size, the stream's
// z = 2 + ceil(bits / 8) + 4 or, where z >= n, n (the raw bytes); csize[j] = 8 + dsize[j].
__global__ __launch_bounds__(256) void k_exr_scan(int32_t* __restrict__ len, Geo g, int32_t* __restrict__ bits,
                                                   int32_t* __restrict__ dsize, int32_t* __restrict__ csize) {
    __shared__ int s_w[4];
    for (int j = (int)blockIdx.x; j < g.nchunks; j += (int)gridDim.x) {
        const int n = stream_bytes(g, j), nc = (n + kChunk - 1) / kChunk;
        int32_t* io = len + (size_t)j * g.cps;
        int carry = 0;
        for (int base0 = 0; base0 < nc; base0 += kScanTile) {
            const int base = base0 + (int)threadIdx.x * kScanPer;
            int x[kScanPer], v = 0, total;
#pragma unroll
            for (int k = 0; k < kScanPer; ++k) {
                x[k] = base + k < nc ? io[base + k] : 0;
                v += x[k];
            }
            int run = block_excl_scan(v, s_w, &total) + carry;
#pragma unroll
            for (int k = 0; k < kScanPer; ++k) {
                if (base + k < nc) io[base + k] = run;
                run += x[k];
            }
            carry += total;
        }
        if (threadIdx.x == 0) {
            const int z = 6 + ((carry + 7) >> 3), d = z >= n ? n : z;
            bits[j] = carry;
            dsize[j] = d;
            csize[j] = 8 + d;
        }
    }
}

// (A stream of z < n bytes is coded; z >= n, so dsize == n, is raw.)
__device__ __forceinline__ bool coded(const Geo& g, const int32_t* dsize, int j) { return dsize[j] != stream_bytes(g, j); }
__device__ __forceinline__ int coded_bytes(const int32_t* bits, int j) { return 6 + ((bits[j] + 7) >> 3); }

__global__ __launch_bounds__(256) void k_exr_zero(uint32_t* __restrict__ S, Geo g, const int32_t* __restrict__ bits,
                                                   const int32_t* __restrict__ dsize) {
    const int per = g.spitch / 4;
    const long long items = (long long)g.nchunks * per;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const int j = (int)(i / per), w = (int)(i % per);
        if (!coded(g, dsize, j) || 4 * w >= coded_bytes(bits, j)) continue;
        S[i] = w == 0 ? 0x0178u : 0u;
    }
}

__global__ __launch_bounds__(64) void k_exr_emit(const uint8_t* __restrict__ P, Geo g, const uint32_t* __restrict__ tabs,
                                                  const uint32_t* __restrict__ hdrs, const int32_t* __restrict__ off,
                                                  const int32_t* __restrict__ dsize, uint32_t* __restrict__ S) {
    const int b = (int)blockIdx.x;
    int j, n, c0, c1, last;
    if (!block_range(g, b, j, n, c0, c1, last) || !coded(g, dsize, j)) return;
    deflate_emit(P + (size_t)j * g.pitch, n, c0, c1, b, tabs, hdrs, off + (size_t)j * g.cps, 16, S + (size_t)j * (g.spitch / 4));
}

// part[2 i], part[2 i + 1]: the sum of bytes and the s2 term mod 65521 of piece i % pps of stream i / pps.
__global__ __launch_bounds__(256) void k_exr_adler_part(const uint8_t* __restrict__ P, Geo g, const int32_t* __restrict__ dsize,
                                                         uint32_t* __restrict__ part) {
    __shared__ int s_w[4];
    const long long items = (long long)g.nchunks * g.pps;
    for (long long i = blockIdx.x; i < items; i += gridDim.x) {
        const int j = (int)(i / g.pps), piece = (int)(i % g.pps), n = stream_bytes(g, j);
        if (piece * kAdlerPiece >= n || !coded(g, dsize, j)) continue;   // (the same for every lane of the workgroup)
        int t_sum, t_term;
        adler_piece(P + (size_t)j * g.pitch, n, piece, s_w, &t_sum, &t_term);
        if (threadIdx.x == 0) {
            part[2 * i] = (uint32_t)t_sum;
            part[2 * i + 1] = (uint32_t)t_term % kAdlerMod;
        }
    }
}

// A workgroup per stream: the Adler-32 of p, big-endian behind the deflate stream in S.
__global__ __launch_bounds__(256) void k_exr_adler_fin(const uint32_t* __restrict__ part, Geo g, const int32_t* __restrict__ bits,
                                                        const int32_t* __restrict__ dsize, uint8_t* __restrict__ S) {
    __shared__ unsigned long long s_a[256], s_b[256];
    for (int j = (int)blockIdx.x; j < g.nchunks; j += (int)gridDim.x) {
        if (!coded(g, dsize, j)) continue;
        const int n = stream_bytes(g, j), pieces = (n + kAdlerPiece - 1) / kAdlerPiece;
        const uint32_t* mine = part + 2 * (size_t)j * g.pps;
        unsigned long long a = 0, b = 0;
        for (int p = (int)threadIdx.x; p < pieces; p += 256) {
            a += mine[2 * p];
            b += mine[2 * p + 1];
        }
        __syncthreads();   // (the previous stream's sums are read)
        s_a[threadIdx.x] = a;
        s_b[threadIdx.x] = b;
        __syncthreads();
        if (threadIdx.x == 0) {
            a = 1, b = (unsigned long long)n;
            for (int k = 0; k < 256; ++k) a += s_a[k], b += s_b[k];
            const uint32_t s1 = (uint32_t)(a % kAdlerMod), s2 = (uint32_t)(b % kAdlerMod);
            uint8_t* o = S + (size_t)j * g.spitch + coded_bytes(bits, j) - 4;
            o[0] = (uint8_t)(s2 >> 8), o[1] = (uint8_t)s2, o[2] = (uint8_t)(s1 >> 8), o[3] = (uint8_t)s1;
        }
    }
}

// off: the exclusive scan of csize, tot its sum.  Nothing at or beyond out + cap is written.
__global__ __launch_bounds__(256) void k_exr_out(const uint8_t* __restrict__ T, const uint32_t* __restrict__ S, Geo g,
                                                  const int32_t* __restrict__ dsize, const int32_t* __restrict__ off,
                                                  const int32_t* __restrict__ tot, const uint8_t* __restrict__ head,
                                                  uint8_t* __restrict__ out, long long cap, long long* __restrict__ size) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    const int per = (g.nfull + 3) / 4;
    const long long items = (long long)g.nchunks * per, data = (long long)g.head + 8LL * g.nchunks;
    auto put = [&](long long at, uint32_t byte) {
        if (at < cap) out[at] = (uint8_t)byte;
    };
    for (long long i = gid; i < items; i += step) {
        const int j = (int)(i / per), w = (int)(i % per), d = dsize[j];
        const long long at0 = data + off[j];
        if (w == 0) {   // the table's word and the chunk's head: y, the data size
            const uint32_t h[4] = {(uint32_t)at0, (uint32_t)((unsigned long long)at0 >> 32), (uint32_t)(j * g.L), (uint32_t)d};
            for (int b = 0; b < 8; ++b) {
                put((long long)g.head + 8LL * j + b, h[b >> 2] >> (8 * (b & 3)));
                put(at0 + b, h[2 + (b >> 2)] >> (8 * (b & 3)));
            }
        }
        if (4 * w >= d) continue;
        uint32_t v;
        const int n = stream_bytes(g, j);
        if (d != n) {
            v = S[(size_t)j * (g.spitch / 4) + w];
        } else {   // r[2 i] = t[i], r[2 i + 1] = t[n / 2 + i]
            const uint8_t* t = T + (size_t)j * g.pitch + 2 * w;
            const int half = n >> 1;
            v = (uint32_t)t[0] | ((uint32_t)t[half] << 8);
            if (4 * w + 2 < n) v |= ((uint32_t)t[1] << 16) | ((uint32_t)t[half + 1] << 24);
        }
        for (int b = 0; b < 4; ++b)
            if (4 * w + b < d) put(at0 + 8 + 4 * w + b, v >> (8 * b));
    }
    if (gid < g.head) put(gid, head[gid]);
    if (gid == 0) {
        const long long total = data + tot[0];
        *size = total <= cap ? total : -total;
    }
}

}  // namespace

struct pt_exr_enc : EncHead {
    pt_exr_enc() : EncHead("EXR", "exr", kStages) {}
    pt_exr_params prm{};
    Geo geo{};
    int nch = 0;
    pt_exr_channel given[kMaxChan] = {};   // the channels in creation order
    int order[kMaxChan] = {};              // order[k]: the creation index of the k-th channel of the sorted list
    int bpv[kMaxChan] = {}, coff[kMaxChan] = {};   // of the sorted list
    int64_t bound = 0;
    uint8_t head[kHeadMax] = {};
    // The device side: head | T | P | chunk bit lengths (then offsets) | block tables | block headers | S | Adler pieces |
    // bits | dsize | csize (then offsets) | scan tile sums | the total.
    uint8_t *d_head = nullptr, *d_T = nullptr, *d_P = nullptr;
    int32_t *d_len = nullptr, *d_bits = nullptr, *d_dsize = nullptr, *d_csize = nullptr, *d_sums = nullptr, *d_tot = nullptr;
    uint32_t *d_tabs = nullptr, *d_hdrs = nullptr, *d_S = nullptr, *d_adler = nullptr;
};

const EncHead* pt::enc_head(const pt_exr_enc* e) { return e; }

void pt::exr_channels(const pt_exr_enc* e, const pt_exr_channel** channels, int32_t* n) {
    *channels = e->given;
    *n = e->nch;
}

namespace {

struct HeadWriter {
    uint8_t* p;
    int n = 0;
    void bytes(const void* s, int len) {
        std::memcpy(p + n, s, (size_t)len);
        n += len;
    }
    void str(const char* s) { bytes(s, (int)std::strlen(s) + 1); }
    void u8(int v) { p[n++] = (uint8_t)v; }
    void i32(int32_t v) {
        for (int k = 0; k < 4; ++k) u8(((uint32_t)v >> (8 * k)) & 255);
    }
    void f32(float v) { i32(pt::__float_as_int_host(v)); }
    void attr(const char* name, const char* type, int size) {
        str(name);
        str(type);
        i32(size);
    }
};

int name_check(const char* name) {   // 1 to 31 bytes of [A-Za-z0-9_.] and the end inside the 32
    int len = 0;
    while (len < 32 && name[len]) {
        const char ch = name[len];
        if (!((ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z') || (ch >= '0' && ch <= '9') || ch == '_' || ch == '.'))
            return pt::fail(PT_ERR_ARG, "an EXR channel name may hold A-Z, a-z, 0-9, '_' and '.' only");
        ++len;
    }
    if (len == 0 || len == 32) return pt::fail(PT_ERR_ARG, "an EXR channel name has 1 to 31 bytes");
    return PT_OK;
}

int params_check(const pt_exr_params* p) {
    if (!p) return pt::fail(PT_ERR_ARG, "null EXR parameters");
    if (p->compression != PT_EXR_NONE && p->compression != PT_EXR_ZIPS && p->compression != PT_EXR_ZIP)
        return pt::fail(PT_ERR_ARG, "EXR compression must be PT_EXR_NONE, PT_EXR_ZIPS or PT_EXR_ZIP");
    if (p->block_bytes < kBlockMin || p->block_bytes > kBlockMax || p->block_bytes % kChunk != 0)
        return pt::fail(PT_ERR_ARG, "EXR block_bytes must be a multiple of " + std::to_string(kChunk) + " in 1024..1048576");
    for (int32_t r : p->reserved)
        if (r != 0) return pt::fail(PT_ERR_ARG, "pt_exr_params.reserved must be zero");
    return PT_OK;
}

int xe_alloc(pt_exr_enc* e) {
    if (e->dev) return PT_OK;
    const Geo& g = e->geo;
    const bool none = g.comp == PT_EXR_NONE;
    const size_t ns = none ? 0 : (size_t)g.nchunks, slots = ns * g.pitch, nb = ns * g.bps;
    uint8_t* p[13];
    if (int rc = enc_alloc(e, {sizeof(e->head), slots + 16, slots + 16, ns * g.cps * 4 + 16, nb * kTab * 4 + 16, nb * kHdrWords * 4 + 16,
                               ns * g.spitch + 16, ns * g.pps * 8 + 16, ns * 4 + 16, ns * 4 + 16, ns * 4 + 16,
                               (ns / kScanTile + 1) * 4, 256},
                           p, e->head, "header"))
        return rc;
    e->d_head = p[0];
    e->d_T = p[1];
    e->d_P = p[2];
    e->d_len = (int32_t*)p[3];
    e->d_tabs = (uint32_t*)p[4];
    e->d_hdrs = (uint32_t*)p[5];
    e->d_S = (uint32_t*)p[6];
    e->d_adler = (uint32_t*)p[7];
    e->d_bits = (int32_t*)p[8];
    e->d_dsize = (int32_t*)p[9];
    e->d_csize = (int32_t*)p[10];
    e->d_sums = (int32_t*)p[11];
    e->d_tot = (int32_t*)p[12];
    return PT_OK;
}

int encode(pt_exr_enc* e, const pt_exr_plane* planes, uint8_t* d_out, int64_t cap, int64_t* d_size, hipStream_t st) {
    if (int rc = xe_alloc(e)) return rc;
    const Geo& g = e->geo;
    Planes pl{};
    for (int k = 0; k < e->nch; ++k) {
        const pt_exr_plane& s = planes[e->order[k]];
        pl.c[k] = Chan{s.d, s.stride, s.divisor, e->given[e->order[k]].type, e->bpv[k], e->coff[k], 0};
    }
    const int64_t items = (int64_t)g.H * g.nch * ((g.W + kPer - 1) / kPer);
    if (int rc = enc_stage(e, 0, st)) return rc;
    if (g.comp == PT_EXR_NONE) {
        hipLaunchKernelGGL(k_exr_convert<true>, dim3(grid_of(std::max<int64_t>(items, g.head), 256)), dim3(256), 0, st, pl, g,
                           e->d_T, (const uint8_t*)e->d_head, d_out, (long long)cap, (long long)e->bound, (long long*)d_size);
        for (int k = 1; k < kStages; ++k)
            if (int rc = enc_stage(e, k, st)) return rc;
        return enc_done(e, st);
    }
    const int nblocks = g.nchunks * g.bps, slot_grid = grid_of((int64_t)g.nchunks * (g.pitch / 16), 256);
    hipLaunchKernelGGL(k_exr_convert<false>, dim3(grid_of(items, 256)), dim3(256), 0, st, pl, g, e->d_T, (const uint8_t*)e->d_head,
                       d_out, (long long)cap, 0LL, (long long*)d_size);
    hipLaunchKernelGGL(k_exr_diff, dim3(slot_grid), dim3(256), 0, st, (const uint8_t*)e->d_T, g, e->d_P);
    if (int rc = enc_stage(e, 1, st)) return rc;
    hipLaunchKernelGGL(k_exr_block, dim3(nblocks), dim3(64), 0, st, (const uint8_t*)e->d_P, g, e->d_tabs, e->d_hdrs, e->d_len);
    if (int rc = enc_stage(e, 2, st)) return rc;
    hipLaunchKernelGGL(k_exr_scan, dim3(std::min(g.nchunks, kMaxGrid)), dim3(256), 0, st, e->d_len, g, e->d_bits, e->d_dsize,
                       e->d_csize);
    if (int rc = enc_stage(e, 3, st)) return rc;
    hipLaunchKernelGGL(k_exr_zero, dim3(grid_of((int64_t)g.nchunks * (g.spitch / 4), 256)), dim3(256), 0, st, e->d_S, g,
                       (const int32_t*)e->d_bits, (const int32_t*)e->d_dsize);
    hipLaunchKernelGGL(k_exr_emit, dim3(nblocks), dim3(64), 0, st, (const uint8_t*)e->d_P, g, (const uint32_t*)e->d_tabs,
                       (const uint32_t*)e->d_hdrs, (const int32_t*)e->d_len, (const int32_t*)e->d_dsize, e->d_S);
    if (int rc = enc_stage(e, 4, st)) return rc;
    hipLaunchKernelGGL(k_exr_adler_part, dim3(grid_of((int64_t)g.nchunks * g.pps, 1)), dim3(256), 0, st, (const uint8_t*)e->d_P, g,
                       (const int32_t*)e->d_dsize, e->d_adler);
    hipLaunchKernelGGL(k_exr_adler_fin, dim3(std::min(g.nchunks, kMaxGrid)), dim3(256), 0, st, (const uint32_t*)e->d_adler, g,
                       (const int32_t*)e->d_bits, (const int32_t*)e->d_dsize, (uint8_t*)e->d_S);
    scan_exclusive_i32(e->d_csize, g.nchunks, e->d_sums, e->d_tot, st);
    if (int rc = enc_stage(e, 5, st)) return rc;
    hipLaunchKernelGGL(k_exr_out, dim3(grid_of(std::max<int64_t>((int64_t)g.nchunks * ((g.nfull + 3) / 4), g.head), 256)), dim3(256),
                       0, st, (const uint8_t*)e->d_T, (const uint32_t*)e->d_S, g, (const int32_t*)e->d_dsize,
                       (const int32_t*)e->d_csize, (const int32_t*)e->d_tot, (const uint8_t*)e->d_head, d_out, (long long)cap,
                       (long long*)d_size);
    return enc_done(e, st);
}

struct Layer { int32_t bit; int n; const char* names[3]; int32_t type; bool halfable; };
const Layer kLayers[7] = {
    {PT_EXR_BEAUTY, 3, {"R", "G", "B"}, PT_EXR_FLOAT, true},
    {PT_EXR_ALBEDO, 3, {"albedo.R", "albedo.G", "albedo.B"}, PT_EXR_FLOAT, true},
    {PT_EXR_NORMAL, 3, {"N.X", "N.Y", "N.Z"}, PT_EXR_FLOAT, true},
    {PT_EXR_POSITION, 3, {"P.X", "P.Y", "P.Z"}, PT_EXR_FLOAT, false},
    {PT_EXR_DEPTH, 1, {"Z", nullptr, nullptr}, PT_EXR_FLOAT, false},
    {PT_EXR_UV, 2, {"UV.U", "UV.V", nullptr}, PT_EXR_FLOAT, true},
    {PT_EXR_ID, 1, {"id", nullptr, nullptr}, PT_EXR_UINT, false},
};

}  // namespace

extern "C" {

void pt_exr_params_default(pt_exr_params* p) {
    if (!p) return;
    *p = pt_exr_params{};
    p->compression = PT_EXR_ZIP;
    p->block_bytes = 32768;
}

int pt_exr_enc_create(int32_t width, int32_t height, const pt_exr_channel* channels, int32_t nchannels, const pt_exr_params* p,
                      pt_exr_enc** out) {
    if (!out || !channels) return pt::fail(PT_ERR_ARG, "null argument");
    if (int rc = params_check(p)) return rc;
    if (nchannels < 1 || nchannels > kMaxChan) return pt::fail(PT_ERR_ARG, "an EXR file has 1 to 16 channels");
    if (width < 1 || height < 1) return pt::fail(PT_ERR_ARG, "EXR width and height must be at least 1");
    int order[kMaxChan];
    for (int k = 0; k < nchannels; ++k) {
        if (int rc = name_check(channels[k].name)) return rc;
        if (channels[k].type != PT_EXR_UINT && channels[k].type != PT_EXR_HALF && channels[k].type != PT_EXR_FLOAT)
            return pt::fail(PT_ERR_ARG, "an EXR channel type must be PT_EXR_UINT, PT_EXR_HALF or PT_EXR_FLOAT");
        order[k] = k;
    }
    auto before = [&](int a, int b) {   // by the bytes of the names
        return std::strcmp(channels[a].name, channels[b].name) < 0;
    };
    std::sort(order, order + nchannels, before);
    for (int k = 1; k < nchannels; ++k)
        if (!before(order[k - 1], order[k])) return pt::fail(PT_ERR_ARG, "EXR channel names must be distinct");
    // The sizes: the file's bound, which is the NONE file's size, must stay below 2^31 (the byte offsets
    // of the chunks are int32), and so must the bit offsets inside a stream: 16 + 9 n + 10 blocks.
    int64_t per_pixel = 0;
    for (int k = 0; k < nchannels; ++k) per_pixel += channels[k].type == PT_EXR_HALF ? 2 : 4;
    const int64_t W = width, H = height, LB = W * per_pixel, L = p->compression == PT_EXR_ZIP ? 16 : 1;
    const int64_t nchunks = (H + L - 1) / L, nfull = std::min(L, H) * LB, nlast = (H - (nchunks - 1) * L) * LB;
    pt_exr_enc* e = new pt_exr_enc;   // (the device side comes with the first encode: xe_alloc)
    HeadWriter hw{e->head};
    const uint8_t magic[8] = {0x76, 0x2f, 0x31, 0x01, 2, 0, 0, 0};
    hw.bytes(magic, 8);
    int chl = 1;
    for (int k = 0; k < nchannels; ++k) chl += (int)std::strlen(channels[k].name) + 1 + 16;
    hw.attr("channels", "chlist", chl);
    for (int k = 0; k < nchannels; ++k) {
        const pt_exr_channel& ch = channels[order[k]];
        hw.str(ch.name);
        hw.i32(ch.type);
        hw.i32(0);   // pLinear and three reserved bytes
        hw.i32(1);
        hw.i32(1);
    }
    hw.u8(0);
    hw.attr("compression", "compression", 1);
    hw.u8(p->compression);
    for (const char* name : {"dataWindow", "displayWindow"}) {
        hw.attr(name, "box2i", 16);
        hw.i32(0), hw.i32(0), hw.i32(width - 1), hw.i32(height - 1);
    }
    hw.attr("lineOrder", "lineOrder", 1);
    hw.u8(0);
    hw.attr("pixelAspectRatio", "float", 4);
    hw.f32(1.0f);
    hw.attr("screenWindowCenter", "v2f", 8);
    hw.f32(0.0f), hw.f32(0.0f);
    hw.attr("screenWindowWidth", "float", 4);
    hw.f32(1.0f);
    hw.u8(0);
    const int64_t bound = hw.n + 8 * nchunks + (8 * nchunks + H * LB);   // the NONE file: header, table, chunks
    const int64_t bps = (nfull + p->block_bytes - 1) / p->block_bytes;
    const char* why = nullptr;
    if (bound >= ((int64_t)1 << 31)) why = "EXR image too large: the byte offsets of its file must stay below 2^31";
    else if (p->compression != PT_EXR_NONE && 16 + 9 * nfull + 10 * bps + 64 >= ((int64_t)1 << 31))
        why = "EXR image too large: the bit offsets of a chunk's stream must stay below 2^31";
    if (why) {
        delete e;
        return pt::fail(PT_ERR_ARG, why);
    }
    e->W = width;
    e->H = height;
    e->prm = *p;
    e->nch = nchannels;
    e->bound = bound;
    int coff = 0;
    for (int k = 0; k < nchannels; ++k) {
        e->given[k] = channels[k];
        e->order[k] = order[k];
        e->bpv[k] = channels[order[k]].type == PT_EXR_HALF ? 2 : 4;
        e->coff[k] = coff;
        coff += width * e->bpv[k];
    }
    Geo& g = e->geo;
    g.W = width, g.H = height, g.nch = nchannels, g.L = (int)L, g.LB = (int)LB;
    g.nchunks = (int)nchunks, g.nfull = (int)nfull, g.nlast = (int)nlast;
    g.mirror = p->mirror_x ? 1 : 0, g.comp = p->compression, g.block_bytes = p->block_bytes;
    g.cps = (int)((nfull + kChunk - 1) / kChunk), g.bps = (int)bps, g.pps = (int)((nfull + kAdlerPiece - 1) / kAdlerPiece);
    g.pitch = (int)(((nfull + 15) & ~(int64_t)15) + 16);
    g.spitch = (int)(((6 + (9 * nfull + 10 * bps + 7) / 8 + 4 + 15) & ~(int64_t)15) + 16);
    g.head = hw.n;
    *out = e;
    return PT_OK;
}

int pt_exr_enc_destroy(pt_exr_enc* e) {
    delete e;   // (~EncHead waits for the last encode)
    return PT_OK;
}

int64_t pt_exr_enc_bound(const pt_exr_enc* e) { return e ? e->bound : 0; }

int64_t pt_exr_enc_header(const pt_exr_enc* e, uint8_t* buf, int64_t cap) {
    if (!e) return 0;
    if (buf && cap > 0) std::memcpy(buf, e->head, (size_t)std::min<int64_t>(cap, e->geo.head));
    return e->geo.head;
}

int pt_exr_enc_planes(pt_exr_enc* e, const pt_exr_plane* planes, uint8_t* d_out, int64_t cap, int64_t* d_size, void* stream) {
    if (int rc = encode_check(e, planes, d_out, cap, d_size)) return rc;
    for (int k = 0; k < e->nch; ++k) {
        if (!planes[k].d) return pt::fail(PT_ERR_ARG, "null EXR plane");
        if (planes[k].stride < 1) return pt::fail(PT_ERR_ARG, "an EXR plane's stride must be at least 1");
        if (!std::isfinite(planes[k].divisor) || !(planes[k].divisor > 0.0f))
            return pt::fail(PT_ERR_ARG, "an EXR plane's divisor must be finite and > 0");
    }
    return encode(e, planes, d_out, cap, d_size, (hipStream_t)stream);
}

// pt::encode_host is written for one array of byte pixels; this is its shape for float planes: one object made, used and
// destroyed around a device buffer "size word | planes | file".
int pt_exr_encode_host(int32_t width, int32_t height, const pt_exr_channel* channels, int32_t nchannels, const float* const* planes,
                       const int32_t* strides, const float* divisors, const pt_exr_params* p, uint8_t* out, int64_t cap,
                       int64_t* size) {
    if (!planes || !out || !size) return pt::fail(PT_ERR_ARG, "null argument");
    if (cap < 0) return pt::fail(PT_ERR_ARG, "negative output capacity");
    pt_exr_enc* e = nullptr;
    if (int rc = pt_exr_enc_create(width, height, channels, nchannels, p, &e)) return rc;
    const size_t npix = (size_t)width * height;
    pt_exr_plane pl[kMaxChan];
    size_t at[kMaxChan], o_out = 256;
    for (int k = 0; k < nchannels; ++k) {
        pl[k].stride = strides ? strides[k] : 1;
        pl[k].divisor = divisors ? divisors[k] : 1.0f;
        if (!planes[k] || pl[k].stride < 1) {
            delete e;
            return pt::fail(PT_ERR_ARG, "null EXR plane or a stride below 1");
        }
        at[k] = o_out;
        o_out += align256(npix * pl[k].stride * sizeof(float));
    }
    const int64_t dcap = std::min(cap, e->bound);
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, o_out + (size_t)dcap + 16) != hipSuccess) {
        (void)hipGetLastError();
        delete e;
        return pt::fail(PT_ERR_NOMEM, "hipMalloc (EXR host encode)");
    }
    int64_t got = 0;
    hipError_t he = hipSuccess;
    for (int k = 0; k < nchannels && he == hipSuccess; ++k) {
        he = hipMemcpy(d + at[k], planes[k], npix * pl[k].stride * sizeof(float), hipMemcpyHostToDevice);
        pl[k].d = (const float*)(d + at[k]);
    }
    int rc = PT_OK;
    if (he == hipSuccess) rc = pt_exr_enc_planes(e, pl, d + o_out, dcap, (int64_t*)d, nullptr);
    if (he == hipSuccess && !rc) he = hipMemcpy(&got, d, sizeof(got), hipMemcpyDeviceToHost);   // (waits for the encode)
    if (he == hipSuccess && !rc && got > 0) he = hipMemcpy(out, d + o_out, (size_t)got, hipMemcpyDeviceToHost);
    delete e;
    (void)hipFree(d);
    if (rc) return rc;
    if (he != hipSuccess) return pt::fail(PT_ERR_HIP, std::string("pt_exr_encode_host: ") + hipGetErrorString(he));
    *size = got < 0 ? -got : got;
    if (got < 0) return pt::fail(PT_ERR_ARG, "the EXR file needs " + std::to_string(-got) + " bytes");
    return PT_OK;
}

int pt_exr_enc_profile(pt_exr_enc* e, int32_t on) {
    if (!e) return pt::fail(PT_ERR_ARG, "null EXR encoder");
    return enc_profile(e, on);
}

int pt_exr_enc_profile_read(pt_exr_enc* e, float ms[6]) { return enc_profile_read(e, ms); }

int pt_exr_ctx_channels(int32_t layers, int32_t half, pt_exr_channel out[16], int32_t* n) {
    if (!out || !n) return pt::fail(PT_ERR_ARG, "null argument");
    if (layers <= 0 || layers > PT_EXR_ALL_LAYERS) return pt::fail(PT_ERR_ARG, "layers: a non-empty mask of PT_EXR_BEAUTY .. PT_EXR_ID");
    if (half < 0 || half > PT_EXR_ALL_LAYERS) return pt::fail(PT_ERR_ARG, "half: a mask of PT_EXR_BEAUTY .. PT_EXR_ID");
    int at = 0;
    for (const Layer& l : kLayers) {
        if (!(layers & l.bit)) continue;
        for (int k = 0; k < l.n; ++k, ++at) {
            out[at] = pt_exr_channel{};
            std::strcpy(out[at].name, l.names[k]);
            out[at].type = l.halfable && (half & l.bit) ? PT_EXR_HALF : l.type;
        }
    }
    *n = at;
    return PT_OK;
}

}  // extern "C"
