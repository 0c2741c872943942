// PNG encoder on the device (pt_png_enc), gfx950: 8-bit RGB, one IDAT holding one zlib stream.
// The filtered stream F (libpng's five row filters, fixed or chosen per row by the smallest sum of |signed
// residual|) is cut into lane chunks of kChunk bytes; a chunk is tokenised greedily into literals and matches
// of distance 1 (runs of the previous byte), and every block_bytes of F form one deflate block coded with the
// fixed or a dynamic Huffman code, whichever is shorter.  Every step is an integer operation, so the file is a
// function of the input bytes; tests/png_enc_ref.py restates the definition and the GPU tests compare byte for
// byte.
//
// Kernel shape: no inter-workgroup wait, no co-resident grid, no look-back; the prefix sum, and the host side that
// every encoder object has, are the shared unit's (pt_enc.h).
//   k_png_filter    rows dealt to workgroups: the five costs by workgroup reduction, the chosen row to F; the
//                   accumulator variants fuse the conversion and re-convert the previous row
//   k_png_block     one wave per deflate block: its chunks, staged in LDS 64 at a time by coalesced loads (a lane
//                   walking its chunk in global memory waits a memory latency per byte), tokenised into an LDS
//                   histogram, the code lengths
//                   (rank sort by the wave; two-queue Huffman, Kraft repair and canonical codes by one lane),
//                   the code-length code and the header, both bit costs, the block type, the block's table
//                   (length << 16 | reversed code) and header bits, then the bit length of every chunk
//   scan            exclusive scan of the chunk bit lengths, in place (pt::scan_exclusive_i32)
//   k_png_zero      the words of the payload up to its length ("IDAT" and the zlib header in the first two)
//   k_png_emit      one wave per deflate block, a lane per chunk: words inside the chunk's bit range are stored,
//                   the first and last are ORed in (atomicOr)
//   k_adler_*       per 4096 bytes of F: sum and weighted sum; one workgroup combines them behind the stream
//   k_png_crc       raw CRC-32 of 256-byte pieces aligned to the payload's end, each times x^(8 * 256 * k)
//   k_png_out       the payload behind the signature and IHDR in the caller's buffer, then the chunk length,
//                   the CRC, IEND and the size word
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include <zlib.h>

#include "pt_enc.h"

using namespace pt;

namespace {

#ifndef PT_PNG_CHUNK                   // (build.build_png_chunk_variant: the grid behind C; the definition's C is 512)
#define PT_PNG_CHUNK 512
#endif
constexpr int kChunk = PT_PNG_CHUNK;   // C: bytes of F per lane
constexpr int kRound = 32768 / kChunk; // chunks a wave stages in LDS and walks at a time, one per lane (32 KiB of F)
constexpr int kLdsStride = kChunk + 4; // a chunk's bytes in LDS: an odd number of words apart, so the lanes' byte reads
                                       // fall on different banks
static_assert(kChunk >= 512 && kChunk <= 1024 && 1024 % kChunk == 0, "C: at least 259 for matches of 258, a divisor of 1024");
constexpr int kBlockMin = 1024, kBlockMax = 1 << 20;
constexpr int kSyms = 286, kTab = 288; // a block's table: 286 symbols, [286] the distance code's bits, [287] the header's
constexpr int kHdrWords = 68;          // 3 + 14 + 19 * 3 + 287 * 7 = 2083 bits at most
constexpr int kFraming = 63;           // signature 8, IHDR 25, IDAT 12, zlib header 2, Adler-32 4, IEND 12
constexpr int kPayloadAt = 37;         // "IDAT" in the file: the stream buffer S starts with it
constexpr int kAdlerPiece = 4096;      // bytes of F per workgroup of k_adler_part (16 per lane)
constexpr int kCrcPiece = 256;         // bytes of the payload per lane of k_png_crc
constexpr uint32_t kAdlerMod = 65521u, kCrcPoly = 0xedb88320u;
constexpr int kStages = 6;             // filter, block, scan, emit, checksums, out (pt_png_enc_profile)

struct Geo {
    int W, H, row, N;                  // row = 1 + 3 W bytes, N = H row bytes of F
    int filter, mirror, block_bytes, nblocks, nchunks;
};

// ---- filtering ------------------------------------------------------------------------------------------
// Byte i of unfiltered row y (0 left of the row and above the image).  MODE 0: pixels, 1: accumulator as
// k_preview, 2: accumulator as pt_tonemap.
template <int MODE>
__device__ __forceinline__ int src_byte(const void* __restrict__ src, int stride, float n, const Geo& g, int y, int i) {
    if (y < 0 || i < 0) return 0;
    const int x = i / 3, k = i - 3 * x;
    const size_t p = (size_t)y * g.W + (g.mirror ? g.W - 1 - x : x);
    if (MODE == 0) return ((const uint8_t*)src)[p * stride + k];
    const float v = ((const float*)src)[3 * p + k];
    return MODE == 1 ? preview_byte(v, n) : save_byte(v, n);
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int residual(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (x - pred) & 255;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_png_filter(const void* __restrict__ src, int stride, float n, Geo g,
                                                     uint8_t* __restrict__ F) {
    __shared__ long long s_cost[4][5];   // (a lane's cost is below 2^27; a row's may pass 2^31 for W above 5.5 million)
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, bytes = g.row - 1;
    for (int y = (int)blockIdx.x; y < g.H; y += (int)gridDim.x) {
        int type = g.filter;
        if (type == PT_PNG_FILTER_ADAPTIVE) {
            int cost[5] = {0, 0, 0, 0, 0};
            for (int i = (int)threadIdx.x; i < bytes; i += 256) {
                const int x = src_byte<MODE>(src, stride, n, g, y, i), a = src_byte<MODE>(src, stride, n, g, y, i - 3),
                          b = src_byte<MODE>(src, stride, n, g, y - 1, i), c = src_byte<MODE>(src, stride, n, g, y - 1, i - 3);
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    const int r = residual(t, x, a, b, c);
                    cost[t] += r < 128 ? r : 256 - r;
                }
            }
            long long wsum[5];
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                long long v = cost[t];
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
                wsum[t] = v;
            }
            __syncthreads();   // (s_cost may still be read for the previous row)
            if (lane == 0) {
#pragma unroll
                for (int t = 0; t < 5; ++t) s_cost[wave][t] = wsum[t];
            }
            __syncthreads();
            long long best = 0x7fffffffffffffffLL;
            type = 0;
            for (int t = 0; t < 5; ++t) {   // ties go to the lowest type
                const long long v = s_cost[0][t] + s_cost[1][t] + s_cost[2][t] + s_cost[3][t];
                if (v < best) best = v, type = t;
            }
        }
        uint8_t* out = F + (size_t)y * g.row;
        if (threadIdx.x == 0) out[0] = (uint8_t)type;
        for (int i = (int)threadIdx.x; i < bytes; i += 256) {
            const int x = src_byte<MODE>(src, stride, n, g, y, i);
            int a = 0, b = 0, c = 0;
            if (type == 1 || type >= 3) a = src_byte<MODE>(src, stride, n, g, y, i - 3);
            if (type >= 2) b = src_byte<MODE>(src, stride, n, g, y - 1, i);
            if (type == 4) c = src_byte<MODE>(src, stride, n, g, y - 1, i - 3);
            out[1 + i] = (uint8_t)residual(type, x, a, b, c);
        }
    }
}

// ---- tokens -----------------------------------------------------------------------------------------------
// Length symbol 257 + j of a match of k bytes (RFC 1951 §3.2.5), its extra bits e and their value.
__device__ __forceinline__ int len_symbol(int k, int& e, int& ev) {
    e = ev = 0;
    if (k == 258) return 285;
    const int d = k - 3;
    if (d < 8) return 257 + d;
    e = 29 - __clz(d);   // floor(log2 d) - 2
    ev = d & ((1 << e) - 1);
    return 261 + 4 * e + ((d >> e) & 3);
}
__device__ __forceinline__ int sym_extra(int s) { return (s < 265 || s == 285) ? 0 : (s - 261) >> 2; }
__device__ __forceinline__ int fixed_len(int s) { return s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8)); }
__device__ __forceinline__ uint32_t fixed_code(int s) {
    return s < 144 ? 0x30u + s : (s < 256 ? 0x190u + (s - 144) : (s < 280 ? (uint32_t)(s - 256) : 0xc0u + (s - 280)));
}

// One round of a deflate block's chunks, kRound from chunk r0: the wave copies their bytes, up to byte `end` of F, into LDS
// with coalesced 16-byte loads (F is padded to 16 bytes); chunk r0 + l lies at byte l * kLdsStride of s_tile.
__device__ __forceinline__ void stage_round(const uint8_t* __restrict__ F, int r0, int end, uint32_t* s_tile) {
    const int base = r0 * kChunk;
    for (int o = (int)threadIdx.x * 16; o < kRound * kChunk && base + o < end; o += 64 * 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(F + base + o);
        uint32_t* d = s_tile + ((o / kChunk) * kLdsStride + (o % kChunk)) / 4;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
}
// The byte before chunk c = r0 + lane (-1 before the stream): the previous lane's last byte, or F's for lane 0.
__device__ __forceinline__ int chunk_prev(const uint8_t* __restrict__ F, const uint32_t* s_tile, int c, int lane) {
    if (c == 0) return -1;
    if (lane == 0) return F[c * kChunk - 1];
    return ((const uint8_t*)s_tile)[(lane - 1) * kLdsStride + kChunk - 1];
}

// A chunk of len bytes at F (in LDS), greedily: where the next k >= 3 bytes equal byte i - 1 a match (k <= 258 and the
// chunk's end), a literal otherwise.  prev: the byte before the chunk; it may lie before the chunk, not before the stream.
template <class Sink>
__device__ __forceinline__ void walk_chunk(const uint8_t* F, int end, int prev, Sink& sink) {
    int i = 0;
    while (i < end) {
        const int cur = F[i];
        if (cur == prev) {
            const int lim = min(258, end - i);
            int k = 1;
            while (k < lim && F[i + k] == prev) ++k;
            if (k >= 3) {
                sink.match(k);
                i += k;
                continue;   // (prev stays: the run's byte)
            }
        }
        sink.lit(cur);
        prev = cur;
        ++i;
    }
}

struct HistSink {
    int* freq;
    __device__ __forceinline__ void lit(int b) { atomicAdd(freq + b, 1); }
    __device__ __forceinline__ void match(int k) {
        int e, ev;
        atomicAdd(freq + len_symbol(k, e, ev), 1);
    }
};
struct CountSink {
    const uint32_t* tab;
    int dist_bits, bits = 0;
    __device__ __forceinline__ void lit(int b) { bits += (int)(tab[b] >> 16); }
    __device__ __forceinline__ void match(int k) {
        int e, ev;
        bits += (int)(tab[len_symbol(k, e, ev)] >> 16) + e + dist_bits;
    }
};

// Bits from bit `off` of the stream, LSB first: nb < 32 bits of the current word are taken, acc holds them.
struct BitWriter {
    uint32_t* buf;
    uint32_t w;
    uint64_t acc = 0;
    int nb;
    bool shared;   // the current word also holds another chunk's bits (or the zlib header's)
    __device__ __forceinline__ BitWriter(uint32_t* stream, int off) : buf(stream), w((uint32_t)off >> 5), nb(off & 31), shared((off & 31) != 0) {}
    __device__ __forceinline__ void put(uint32_t bits, int len) {   // len <= 16
        acc |= (uint64_t)bits << nb;
        nb += len;
        if (nb >= 32) {
            if (shared) atomicOr(buf + w, (uint32_t)acc);
            else buf[w] = (uint32_t)acc;
            shared = false;
            ++w;
            acc >>= 32;
            nb -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (nb > 0) atomicOr(buf + w, (uint32_t)acc);
    }
};
struct EmitSink {
    const uint32_t* tab;
    int dist_bits;
    BitWriter wr;
    __device__ __forceinline__ void sym(int s) { wr.put(tab[s] & 0xffffu, (int)(tab[s] >> 16)); }
    __device__ __forceinline__ void lit(int b) { sym(b); }
    __device__ __forceinline__ void match(int k) {
        int e, ev;
        sym(len_symbol(k, e, ev));
        wr.put((uint32_t)ev, e);
        wr.put(0u, dist_bits);   // distance 1: symbol 0, all zeros in both codings
    }
};

// ---- code lengths ---------------------------------------------------------------------------------------
// Every lane of the (one-wave) workgroup calls it.  freq[0..nsym): counts, at least two of them > 0; len[0..nsym):
// the code lengths, at most `limit`; cnt[1..limit]: the codes of each length.  sorted, wt, par: scratch.
//   1. the used symbols sorted by (freq, symbol): a rank sort by the wave
//   2. the two-queue Huffman construction over that order, a leaf before an internal node of the same weight
//   3. codes per length, depths beyond the limit counted at the limit
//   4. while the Kraft sum exceeds 1: one code leaves the limit and becomes the sibling of the longest shorter code
//   5. the lengths dealt out over the sorted order, the shortest to the most frequent
__device__ void build_lengths(const int* freq, int nsym, int limit, int* len, int* sorted, int* wt, int* par, int* cnt) {
    const int lane = (int)threadIdx.x;
    int used = 0;
    for (int s = lane; s < nsym; s += 64) {
        len[s] = 0;
        const int f = freq[s];
        if (f <= 0) continue;
        ++used;
        const int key = f * 512 + s;
        int r = 0;
        for (int t = 0; t < nsym; ++t) {
            const int ft = freq[t];
            r += (ft > 0 && ft * 512 + t < key) ? 1 : 0;
        }
        sorted[r] = s;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) used += __shfl_xor(used, d, 64);
    __syncthreads();
    if (lane == 0) {
        const int n = used;
        for (int v = 0; v < n; ++v) wt[v] = freq[sorted[v]];
        int i = 0, j = n;
        for (int nxt = n; nxt < 2 * n - 1; ++nxt) {
            const int a = (i < n && (j >= nxt || wt[i] <= wt[j])) ? i++ : j++;
            const int b = (i < n && (j >= nxt || wt[i] <= wt[j])) ? i++ : j++;
            wt[nxt] = wt[a] + wt[b];
            par[a] = par[b] = nxt;
        }
        for (int l = 0; l <= limit; ++l) cnt[l] = 0;
        wt[2 * n - 2] = 0;   // (from here wt holds depths)
        for (int v = 2 * n - 3; v >= 0; --v) {
            const int d = wt[par[v]] + 1;
            wt[v] = d;
            if (v < n) ++cnt[min(d, limit)];
        }
        int total = 0;
        for (int l = 1; l <= limit; ++l) total += cnt[l] << (limit - l);
        for (; total > 1 << limit; --total) {
            --cnt[limit];
            for (int l = limit - 1; l > 0; --l)
                if (cnt[l]) {
                    --cnt[l];
                    cnt[l + 1] += 2;
                    break;
                }
        }
        int at = n;
        for (int l = 1; l <= limit; ++l)
            for (int q = cnt[l]; q > 0; --q) len[sorted[--at]] = l;
    }
    __syncthreads();
}

// Canonical codes (RFC 1951 §3.2.2) by one lane: tab[s] = length << 16 | the code bit-reversed.
__device__ void canonical_codes(const int* len, int nsym, int limit, const int* cnt, uint32_t* next, uint32_t* tab) {
    uint32_t code = 0;
    for (int l = 1; l <= limit; ++l) {
        code = (code + (l > 1 ? (uint32_t)cnt[l - 1] : 0u)) << 1;
        next[l] = code;
    }
    for (int s = 0; s < nsym; ++s) {
        const int l = len[s];
        tab[s] = l ? ((uint32_t)l << 16) | (__brev(next[l]++) >> (32 - l)) : 0u;
    }
}

struct LdsBits {
    uint32_t* w;
    int pos = 0;
    __device__ __forceinline__ void put(uint32_t v, int len) {   // len <= 16
        const int at = pos >> 5, sh = pos & 31;
        w[at] |= v << sh;
        if (sh + len > 32) w[at + 1] |= v >> (32 - sh);
        pos += len;
    }
};

__device__ __constant__ uint8_t c_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// The chunks of deflate block b: [c0, c1), and the block's end in F.
__device__ __forceinline__ void block_range(const Geo& g, int b, int& c0, int& c1) {
    const int per = g.block_bytes / kChunk;
    c0 = b * per;
    c1 = min(c0 + per, g.nchunks);
}

__global__ __launch_bounds__(64) void k_png_block(const uint8_t* __restrict__ F, Geo g, uint32_t* __restrict__ tabs,
                                                   uint32_t* __restrict__ hdrs, int32_t* __restrict__ len_out) {
    __shared__ int s_freq[kTab], s_len[kTab], s_sorted[kTab], s_wt[2 * kTab], s_par[2 * kTab], s_cnt[16];
    __shared__ int s_clfreq[19], s_cllen[19];
    __shared__ uint32_t s_tab[kTab], s_cltab[19], s_hdr[kHdrWords];
    __shared__ uint32_t s_next[16];
    __shared__ int s_pick[3];   // [1]: header bits
    __shared__ uint32_t s_tile[kRound * kLdsStride / 4];
    const int lane = (int)threadIdx.x, b = (int)blockIdx.x;
    int c0, c1;
    block_range(g, b, c0, c1);
    const int end = min(c1 * kChunk, g.N);
    const uint8_t* mine = (const uint8_t*)s_tile + lane * kLdsStride;
    for (int s = lane; s < kTab; s += 64) s_freq[s] = 0;
    for (int s = lane; s < kHdrWords; s += 64) s_hdr[s] = 0u;
    if (lane < 19) s_clfreq[lane] = 0;
    __syncthreads();
    {
        HistSink hs{s_freq};
        for (int r0 = c0; r0 < c1; r0 += kRound) {
            __syncthreads();   // (the previous round's walks are done with s_tile)
            stage_round(F, r0, end, s_tile);
            __syncthreads();
            const int c = r0 + lane;
            if (lane < kRound && c < c1) walk_chunk(mine, min(kChunk, end - c * kChunk), chunk_prev(F, s_tile, c, lane), hs);
        }
    }
    __syncthreads();
    if (lane == 0) s_freq[256] = 1;
    __syncthreads();
    build_lengths(s_freq, kSyms, 15, s_len, s_sorted, s_wt, s_par, s_cnt);
    int nmatch = 0, nlit = 0;
    for (int s = lane; s < kSyms; s += 64) {
        if (s > 256) nmatch += s_freq[s];
        if (s_len[s]) nlit = s + 1;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        nmatch += __shfl_xor(nmatch, d, 64);
        nlit = max(nlit, __shfl_xor(nlit, d, 64));
    }
    nlit = max(nlit, 257);
    const int dist_len = nmatch > 0 ? 1 : 0;
    if (lane == 0) canonical_codes(s_len, kSyms, 15, s_cnt, s_next, s_tab);
    // the code-length code over the nlit lengths and the distance code's one length (no repeat symbols)
    for (int s = lane; s < nlit; s += 64) atomicAdd(s_clfreq + s_len[s], 1);
    if (lane == 0) atomicAdd(s_clfreq + dist_len, 1);
    __syncthreads();
    build_lengths(s_clfreq, 19, 7, s_cllen, s_sorted, s_wt, s_par, s_cnt);
    const bool final_block = b == g.nblocks - 1;
    if (lane == 0) {
        canonical_codes(s_cllen, 19, 7, s_cnt, s_next, s_cltab);
        int ncl = 4;
        for (int i = 4; i < 19; ++i)
            if (s_cllen[c_cl_order[i]]) ncl = i + 1;
        LdsBits hb{s_hdr};
        hb.put(final_block ? 1u : 0u, 1);
        hb.put(2u, 2);
        hb.put((uint32_t)(nlit - 257), 5);
        hb.put(0u, 5);
        hb.put((uint32_t)(ncl - 4), 4);
        for (int i = 0; i < ncl; ++i) hb.put((uint32_t)s_cllen[c_cl_order[i]], 3);
        for (int s = 0; s <= nlit; ++s) {
            const uint32_t t = s_cltab[s < nlit ? s_len[s] : dist_len];
            hb.put(t & 0xffffu, (int)(t >> 16));
        }
        s_pick[1] = hb.pos;
    }
    __syncthreads();
    int dyn = 0, fix = 0;
    for (int s = lane; s < kSyms; s += 64) {
        const int f = s_freq[s], e = sym_extra(s);
        dyn += f * (s_len[s] + e);
        fix += f * (fixed_len(s) + e);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        dyn += __shfl_xor(dyn, d, 64);
        fix += __shfl_xor(fix, d, 64);
    }
    dyn += s_pick[1] + nmatch;
    fix += 3 + 5 * nmatch;
    const bool dynamic = dyn < fix;   // ties go to fixed
    __syncthreads();
    if (!dynamic) {
        for (int s = lane; s < kSyms; s += 64) {
            const int l = fixed_len(s);
            s_tab[s] = ((uint32_t)l << 16) | (__brev(fixed_code(s)) >> (32 - l));
        }
        if (lane == 0) {
            s_hdr[0] = (final_block ? 1u : 0u) | (1u << 1);
            s_pick[1] = 3;
        }
    }
    __syncthreads();
    const int hdr_bits = s_pick[1], dist_bits = dynamic ? 1 : 5;
    if (lane == 0) {
        s_tab[286] = (uint32_t)dist_bits;
        s_tab[287] = (uint32_t)hdr_bits;
    }
    __syncthreads();
    for (int s = lane; s < kTab; s += 64) tabs[(size_t)b * kTab + s] = s_tab[s];
    for (int s = lane; s < (hdr_bits + 31) / 32; s += 64) hdrs[(size_t)b * kHdrWords + s] = s_hdr[s];
    for (int r0 = c0; r0 < c1; r0 += kRound) {
        if (c1 - c0 > kRound) {   // (a block of one round is still staged)
            __syncthreads();
            stage_round(F, r0, end, s_tile);
            __syncthreads();
        }
        const int c = r0 + lane;
        if (lane >= kRound || c >= c1) continue;
        CountSink cs{s_tab, dist_bits};
        walk_chunk(mine, min(kChunk, end - c * kChunk), chunk_prev(F, s_tile, c, lane), cs);
        len_out[c] = cs.bits + (c == c0 ? hdr_bits : 0) + (c == c1 - 1 ? (int)(s_tab[256] >> 16) : 0);
    }
}

// off: the exclusive scan of the chunk bit lengths; the deflate stream starts at bit 48 of S.
__global__ __launch_bounds__(64) void k_png_emit(const uint8_t* __restrict__ F, Geo g, const uint32_t* __restrict__ tabs,
                                                  const uint32_t* __restrict__ hdrs, const int32_t* __restrict__ off,
                                                  uint32_t* __restrict__ S) {
    __shared__ uint32_t s_tab[kTab];
    __shared__ uint32_t s_tile[kRound * kLdsStride / 4];
    const int lane = (int)threadIdx.x, b = (int)blockIdx.x;
    int c0, c1;
    block_range(g, b, c0, c1);
    const int end = min(c1 * kChunk, g.N);
    for (int s = lane; s < kTab; s += 64) s_tab[s] = tabs[(size_t)b * kTab + s];
    __syncthreads();
    const int dist_bits = (int)s_tab[286], hdr_bits = (int)s_tab[287];
    for (int r0 = c0; r0 < c1; r0 += kRound) {
        __syncthreads();
        stage_round(F, r0, end, s_tile);
        __syncthreads();
        const int c = r0 + lane;
        if (lane >= kRound || c >= c1) continue;
        EmitSink es{s_tab, dist_bits, BitWriter(S, 48 + off[c])};
        if (c == c0) {
            const uint32_t* h = hdrs + (size_t)b * kHdrWords;
            for (int pos = 0; pos < hdr_bits; pos += 16) {
                const int l = min(16, hdr_bits - pos);
                es.wr.put((h[pos >> 5] >> (pos & 31)) & ((1u << l) - 1u), l);
            }
        }
        walk_chunk((const uint8_t*)s_tile + lane * kLdsStride, min(kChunk, end - c * kChunk), chunk_prev(F, s_tile, c, lane), es);
        if (c == c1 - 1) es.sym(256);
        es.wr.finish();
    }
}

// S: "IDAT", the zlib header 78 01, the deflate stream of tot[0] bits, the Adler-32.
__device__ __forceinline__ int payload_bytes(const int32_t* tot) { return 10 + ((tot[0] + 7) >> 3); }

__global__ __launch_bounds__(256) void k_png_zero(uint32_t* __restrict__ S, const int32_t* __restrict__ tot) {
    const int words = (payload_bytes(tot) + 3) >> 2;
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < words; i += (int)gridDim.x * 256)
        S[i] = i == 0 ? 0x54414449u : (i == 1 ? 0x0178u : 0u);
}

// ---- Adler-32 -------------------------------------------------------------------------------------------
// s1 = 1 + sum d_i, s2 = N + sum (N - i) d_i (mod 65521).  A lane's 16 bytes [at, e): (N - e) sum + sum (e - i) d_i.
// part[2 p], part[2 p + 1]: piece p's sum of bytes (below 2^21) and its s2 term mod 65521.
__global__ __launch_bounds__(256) void k_adler_part(const uint8_t* __restrict__ F, int N, uint32_t* __restrict__ part) {
    __shared__ int s_w[4];
    for (int piece = (int)blockIdx.x; piece * kAdlerPiece < N; piece += (int)gridDim.x) {
        const int at = piece * kAdlerPiece + (int)threadIdx.x * 16, e = min(at + 16, N);
        uint32_t sum = 0, local = 0;
        if (at < N) {
            const uint4 v = *reinterpret_cast<const uint4*>(F + at);   // (F is padded to 16 bytes)
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t d = at + j < N ? (w[j >> 2] >> (8 * (j & 3))) & 0xffu : 0u;
                sum += d;
                local += (uint32_t)(e - at - j) * d;   // (d is 0 where the weight is not positive)
            }
        }
        const uint32_t term = (uint32_t)(((uint64_t)((uint32_t)(N - e) % kAdlerMod) * sum + local) % kAdlerMod);
        int t_sum, t_term;
        (void)block_excl_scan((int)sum, s_w, &t_sum);
        (void)block_excl_scan((int)term, s_w, &t_term);   // 256 terms below 65521
        if (threadIdx.x == 0) {
            part[2 * piece] = (uint32_t)t_sum;
            part[2 * piece + 1] = (uint32_t)t_term % kAdlerMod;
        }
    }
}

// One workgroup: the Adler-32 of F, big-endian behind the deflate stream in S.
__global__ __launch_bounds__(256) void k_adler_fin(const uint32_t* __restrict__ part, int N, const int32_t* __restrict__ tot,
                                                    uint8_t* __restrict__ S) {
    __shared__ unsigned long long s_a[256], s_b[256];
    const int pieces = (N + kAdlerPiece - 1) / kAdlerPiece;
    unsigned long long a = 0, b = 0;
    for (int p = (int)threadIdx.x; p < pieces; p += 256) {
        a += part[2 * p];
        b += part[2 * p + 1];
    }
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = 1, b = (unsigned long long)N;
        for (int k = 0; k < 256; ++k) a += s_a[k], b += s_b[k];
        const uint32_t s1 = (uint32_t)(a % kAdlerMod), s2 = (uint32_t)(b % kAdlerMod);
        uint8_t* o = S + payload_bytes(tot) - 4;
        o[0] = (uint8_t)(s2 >> 8), o[1] = (uint8_t)s2, o[2] = (uint8_t)(s1 >> 8), o[3] = (uint8_t)s1;
    }
}

// ---- CRC-32 ---------------------------------------------------------------------------------------------
// Polynomials over GF(2) modulo the CRC-32 polynomial, reflected: bit 31 is x^0.
__device__ __forceinline__ uint32_t mul_mod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// x^n by square and multiply
__device__ __forceinline__ uint32_t x_pow(uint32_t n) {
    uint32_t p = 0x80000000u, sq = 0x40000000u;   // x^0, x^1
    for (; n; n >>= 1) {
        if (n & 1u) p = mul_mod(sq, p);
        sq = mul_mod(sq, sq);
    }
    return p;
}

// The raw CRC (initial value 0, no final complement) of the payload's L bytes is the sum over 256-byte pieces,
// counted from the END (piece k ends at L - 256 k; only the last one is partial, and a raw CRC ignores the zero
// bytes that would fill it), of crc_k x^(8 * 256 * k).  part[workgroup]: the sum of its lanes' terms.
__global__ __launch_bounds__(256) void k_png_crc(const uint8_t* __restrict__ S, const int32_t* __restrict__ tot,
                                                  uint32_t* __restrict__ part) {
    __shared__ uint32_t s_tab[256], s_w[4];
    {
        uint32_t c = threadIdx.x;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        s_tab[threadIdx.x] = c;
    }
    __syncthreads();
    const int L = payload_bytes(tot), pieces = (L + kCrcPiece - 1) / kCrcPiece;
    uint32_t acc = 0;
    for (int k = (int)blockIdx.x * 256 + (int)threadIdx.x; k < pieces; k += (int)gridDim.x * 256) {
        const int end = L - k * kCrcPiece, start = max(0, end - kCrcPiece);
        uint32_t crc = 0;
        int i = start;   // bytes up to a word boundary, whole words (S is word-aligned), the bytes left
        for (; i < end && (i & 3); ++i) crc = s_tab[(crc ^ S[i]) & 0xffu] ^ (crc >> 8);
        for (; i + 4 <= end; i += 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(S + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) crc = s_tab[(crc ^ (w >> (8 * j))) & 0xffu] ^ (crc >> 8);
        }
        for (; i < end; ++i) crc = s_tab[(crc ^ S[i]) & 0xffu] ^ (crc >> 8);
        acc ^= mul_mod(crc, x_pow(8u * kCrcPiece * (uint32_t)k));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc ^= __shfl_xor(acc, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = s_w[0] ^ s_w[1] ^ s_w[2] ^ s_w[3];
}

// ---- the file -------------------------------------------------------------------------------------------
// head: the signature and IHDR (33 bytes).  Nothing at or beyond out + cap is written.
__global__ __launch_bounds__(256) void k_png_out(const uint8_t* __restrict__ S, const int32_t* __restrict__ tot,
                                                  const uint32_t* __restrict__ crc_part, int crc_parts,
                                                  const uint8_t* __restrict__ head, uint8_t* __restrict__ out, long long cap,
                                                  long long* __restrict__ size) {
    const int L = payload_bytes(tot);
    const int gid = (int)blockIdx.x * 256 + (int)threadIdx.x;
    for (int i = gid; 4 * i < L; i += (int)gridDim.x * 256) {   // a word of S (coalesced), its bytes to the odd offset 37
        const uint32_t w = reinterpret_cast<const uint32_t*>(S)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * i + j < L && kPayloadAt + 4 * i + j < cap) out[kPayloadAt + 4 * i + j] = (uint8_t)(w >> (8 * j));
    }
    if (gid != 0) return;
    auto put = [&](long long at, uint32_t byte) {
        if (at < cap) out[at] = (uint8_t)byte;
    };
    auto put_u32 = [&](long long at, uint32_t v) {
        for (int k = 0; k < 4; ++k) put(at + k, v >> (24 - 8 * k));
    };
    for (int i = 0; i < 33; ++i) put(i, head[i]);
    put_u32(33, (uint32_t)(L - 4));
    // the all-ones initial value: one term, ffffffff x^(8 L); and the final complement
    uint32_t crc = mul_mod(0xffffffffu, x_pow(8u * (uint32_t)L));
    for (int k = 0; k < crc_parts; ++k) crc ^= crc_part[k];
    put_u32(kPayloadAt + L, ~crc);
    put_u32((long long)kPayloadAt + L + 4, 0u);            // IEND: length 0, type, CRC
    put_u32((long long)kPayloadAt + L + 8, 0x49454e44u);
    put_u32((long long)kPayloadAt + L + 12, 0xae426082u);
    const long long end = (long long)L + 53;
    *size = end <= cap ? end : -end;
}

}  // namespace

struct pt_png_enc : EncHead {
    pt_png_enc() : EncHead("PNG", "png", kStages) {}
    pt_png_params prm{};
    Geo geo{};
    int64_t stream_max = 0;           // bytes of the deflate stream at most: (9 N + 10 blocks + 7) / 8
    uint8_t head[33] = {};            // signature and IHDR
    // The device side: head | F | chunk bit lengths (then offsets) | scan tile sums | block tables | block
    // headers | S | Adler pieces | CRC parts | total bits.
    uint8_t *d_head = nullptr, *d_F = nullptr;
    int32_t *d_len = nullptr, *d_sums = nullptr, *d_tot = nullptr;
    uint32_t *d_tabs = nullptr, *d_hdrs = nullptr, *d_S = nullptr, *d_adler = nullptr, *d_crc = nullptr;
};

const EncHead* pt::enc_head(const pt_png_enc* e) { return e; }

namespace {

int params_check(const pt_png_params* p) {
    if (!p) return pt::fail(PT_ERR_ARG, "null PNG parameters");
    if (p->filter < 0 || p->filter > PT_PNG_FILTER_ADAPTIVE) return pt::fail(PT_ERR_ARG, "PNG filter must be 0..4 or PT_PNG_FILTER_ADAPTIVE");
    if (p->block_bytes < kBlockMin || p->block_bytes > kBlockMax || p->block_bytes % kChunk != 0)
        return pt::fail(PT_ERR_ARG, "PNG block_bytes must be a multiple of " + std::to_string(kChunk) + " in 1024..1048576");
    if (p->conv != PT_PNG_CONV_PREVIEW && p->conv != PT_PNG_CONV_SAVE)
        return pt::fail(PT_ERR_ARG, "PNG conv must be PT_PNG_CONV_PREVIEW or PT_PNG_CONV_SAVE");
    for (int32_t r : p->reserved)
        if (r != 0) return pt::fail(PT_ERR_ARG, "pt_png_params.reserved must be zero");
    return PT_OK;
}

// The bit offsets are int32: 48 + 9 N + 10 blocks must stay below 2^31.
int size_check(int32_t W, int32_t H, int32_t block_bytes) {
    if (W < 1 || H < 1) return pt::fail(PT_ERR_ARG, "PNG width and height must be at least 1");
    const int64_t N = (int64_t)H * (1 + 3 * (int64_t)W), blocks = (N + block_bytes - 1) / block_bytes;
    if (9 * N + 10 * blocks + 48 + 64 >= ((int64_t)1 << 31))
        return pt::fail(PT_ERR_ARG, "PNG image too large: the bit offsets of its stream must stay below 2^31");
    return PT_OK;
}

int pe_alloc(pt_png_enc* e) {
    if (e->dev) return PT_OK;
    const Geo& g = e->geo;
    const size_t N = (size_t)g.N, nc = (size_t)g.nchunks, nb = (size_t)g.nblocks;
    uint8_t* p[10];
    if (int rc = enc_alloc(e, {sizeof(e->head), N + 16, nc * 4, (nc / kScanTile + 1) * 4, nb * kTab * 4, nb * kHdrWords * 4,
                               (size_t)e->stream_max + 32, (N / kAdlerPiece + 1) * 8, kMaxGrid * 4, 256},
                           p, e->head, "header"))
        return rc;
    e->d_head = p[0];
    e->d_F = p[1];
    e->d_len = (int32_t*)p[2];
    e->d_sums = (int32_t*)p[3];
    e->d_tabs = (uint32_t*)p[4];
    e->d_hdrs = (uint32_t*)p[5];
    e->d_S = (uint32_t*)p[6];
    e->d_adler = (uint32_t*)p[7];
    e->d_crc = (uint32_t*)p[8];
    e->d_tot = (int32_t*)p[9];
    return PT_OK;
}

// src: pixels (stride 3 or 4) or, with mode 1 / 2, the float accumulator of `samples` samples.
int encode(pt_png_enc* e, const void* src, int stride, int mode, float samples, uint8_t* d_out, int64_t cap, int64_t* d_size,
           hipStream_t st) {
    if (int rc = pe_alloc(e)) return rc;
    const Geo& g = e->geo;
    if (int rc = enc_stage(e, 0, st)) return rc;
    auto filter = mode == 0 ? k_png_filter<0> : (mode == 1 ? k_png_filter<1> : k_png_filter<2>);
    hipLaunchKernelGGL(filter, dim3(std::min(g.H, 65535)), dim3(256), 0, st, src, stride, samples, g, e->d_F);
    if (int rc = enc_stage(e, 1, st)) return rc;
    hipLaunchKernelGGL(k_png_block, dim3(g.nblocks), dim3(64), 0, st, (const uint8_t*)e->d_F, g, e->d_tabs, e->d_hdrs, e->d_len);
    if (int rc = enc_stage(e, 2, st)) return rc;
    scan_exclusive_i32(e->d_len, g.nchunks, e->d_sums, e->d_tot, st);
    if (int rc = enc_stage(e, 3, st)) return rc;
    hipLaunchKernelGGL(k_png_zero, dim3(grid_of(e->stream_max / 4 + 4, 256)), dim3(256), 0, st, e->d_S, (const int32_t*)e->d_tot);
    hipLaunchKernelGGL(k_png_emit, dim3(g.nblocks), dim3(64), 0, st, (const uint8_t*)e->d_F, g, (const uint32_t*)e->d_tabs,
                       (const uint32_t*)e->d_hdrs, (const int32_t*)e->d_len, e->d_S);
    if (int rc = enc_stage(e, 4, st)) return rc;
    hipLaunchKernelGGL(k_adler_part, dim3(grid_of(g.N, kAdlerPiece)), dim3(256), 0, st, (const uint8_t*)e->d_F, g.N, e->d_adler);
    hipLaunchKernelGGL(k_adler_fin, dim3(1), dim3(256), 0, st, (const uint32_t*)e->d_adler, g.N, (const int32_t*)e->d_tot,
                       (uint8_t*)e->d_S);
    const int crc_grid = grid_of(e->stream_max + 10, kCrcPiece * 256);
    hipLaunchKernelGGL(k_png_crc, dim3(crc_grid), dim3(256), 0, st, (const uint8_t*)e->d_S, (const int32_t*)e->d_tot, e->d_crc);
    if (int rc = enc_stage(e, 5, st)) return rc;
    hipLaunchKernelGGL(k_png_out, dim3(grid_of(e->stream_max + 10, 256 * 16)), dim3(256), 0, st, (const uint8_t*)e->d_S,
                       (const int32_t*)e->d_tot, (const uint32_t*)e->d_crc, crc_grid, (const uint8_t*)e->d_head, d_out,
                       (long long)cap, (long long*)d_size);
    return enc_done(e, st);
}

void put_be32(uint8_t* o, uint32_t v) { o[0] = (uint8_t)(v >> 24), o[1] = (uint8_t)(v >> 16), o[2] = (uint8_t)(v >> 8), o[3] = (uint8_t)v; }

}  // namespace

extern "C" {

void pt_png_params_default(pt_png_params* p) {
    if (!p) return;
    *p = pt_png_params{};
    p->filter = PT_PNG_FILTER_ADAPTIVE;
    p->block_bytes = 32768;
    p->conv = PT_PNG_CONV_PREVIEW;
}

int pt_png_enc_create(int32_t width, int32_t height, const pt_png_params* p, pt_png_enc** out) {
    if (!out) return pt::fail(PT_ERR_ARG, "null argument");
    if (int rc = params_check(p)) return rc;
    if (int rc = size_check(width, height, p->block_bytes)) return rc;
    pt_png_enc* e = new pt_png_enc;   // (the device side comes with the first encode: pe_alloc)
    e->W = width;
    e->H = height;
    e->prm = *p;
    Geo& g = e->geo;
    g.W = width, g.H = height, g.row = 1 + 3 * width, g.N = height * g.row;
    g.filter = p->filter, g.mirror = p->mirror_x ? 1 : 0, g.block_bytes = p->block_bytes;
    g.nblocks = (g.N + g.block_bytes - 1) / g.block_bytes;
    g.nchunks = (g.N + kChunk - 1) / kChunk;
    e->stream_max = (9 * (int64_t)g.N + 10 * (int64_t)g.nblocks + 7) / 8;
    const uint8_t sig[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    std::copy(sig, sig + 16, e->head);
    put_be32(e->head + 16, (uint32_t)width);
    put_be32(e->head + 20, (uint32_t)height);
    e->head[24] = 8, e->head[25] = 2;   // 8 bits, colour type RGB; compression, filter method, interlace: 0
    put_be32(e->head + 29, (uint32_t)crc32(0L, e->head + 12, 17));
    *out = e;
    return PT_OK;
}

int pt_png_enc_destroy(pt_png_enc* e) {
    delete e;   // (~EncHead waits for the last encode)
    return PT_OK;
}

int64_t pt_png_enc_bound(const pt_png_enc* e) { return e ? e->stream_max + kFraming : 0; }

int pt_png_enc_pixels(pt_png_enc* e, const uint8_t* d_pix, int32_t pixel_stride, uint8_t* d_out, int64_t cap, int64_t* d_size,
                      void* stream) {
    if (int rc = encode_check(e, d_pix, d_out, cap, d_size)) return rc;
    if (pixel_stride != 3 && pixel_stride != 4) return pt::fail(PT_ERR_ARG, "the pixel stride must be 3 or 4");
    return encode(e, d_pix, pixel_stride, 0, 1.0f, d_out, cap, d_size, (hipStream_t)stream);
}

int pt_png_enc_accum(pt_png_enc* e, const float* d_rgb, float samples, uint8_t* d_out, int64_t cap, int64_t* d_size,
                     void* stream) {
    if (int rc = encode_check(e, d_rgb, d_out, cap, d_size)) return rc;
    if (!std::isfinite(samples) || !(samples > 0.0f)) return pt::fail(PT_ERR_ARG, "samples must be finite and > 0");
    return encode(e, d_rgb, 0, e->prm.conv == PT_PNG_CONV_SAVE ? 2 : 1, samples, d_out, cap, d_size, (hipStream_t)stream);
}

int pt_png_encode_host(int32_t width, int32_t height, const uint8_t* pix, int32_t pixel_stride, const pt_png_params* p,
                       uint8_t* out, int64_t cap, int64_t* size) {
    return encode_host(pt_png_enc_create, pt_png_enc_bound, pt_png_enc_pixels, width, height, pix, pixel_stride, p, out, cap, size);
}

int pt_png_enc_profile(pt_png_enc* e, int32_t on) {
    if (!e) return pt::fail(PT_ERR_ARG, "null PNG encoder");
    return enc_profile(e, on);
}

int pt_png_enc_profile_read(pt_png_enc* e, float ms[6]) { return enc_profile_read(e, ms); }

}  // extern "C"
