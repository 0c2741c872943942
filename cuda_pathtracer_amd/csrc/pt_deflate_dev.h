// The run-length deflate coder of the device encoders (pt_png_enc.hip codes one stream of it, pt_exr_enc.hip
// one per OpenEXR chunk), gfx950, device code only: a stream of bytes F is cut into lane chunks of kChunk bytes; a chunk is
// tokenised greedily into literals and matches of distance 1 (runs of the previous byte), and a range of chunks forms one
// deflate block coded with the fixed or a dynamic Huffman code, whichever is shorter.  Every step is an integer operation.
//   deflate_block   one wave per deflate block: its chunks, staged in LDS 64 at a time by coalesced loads (a lane walking its
//                   chunk in global memory waits a memory latency per byte), tokenised into an LDS histogram, the code
//                   lengths (rank sort by the wave; two-queue Huffman, Kraft repair and canonical codes by one lane), the
//                   code-length code and the header, both bit costs, the block type, the block's table (length << 16 |
//                   reversed code) and header bits, then the bit length of every chunk
//   deflate_emit    one wave per deflate block, a lane per chunk: words inside the chunk's bit range are stored, the first
//                   and last are ORed in (atomicOr)
//   adler_piece     a workgroup's 4096 bytes of a stream: their sum and weighted sum
// The streams are padded to 16 bytes (the staging and the Adler pieces load 16 bytes wide).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_enc.h"

namespace pt {
namespace deflate {
namespace {   // (every unit that includes the header has its own copy, as of kernels of its own)

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
constexpr int kAdlerPiece = 4096;      // bytes of F per workgroup of an Adler-32 part kernel (16 per lane)
constexpr uint32_t kAdlerMod = 65521u;

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

// ---- a deflate block ------------------------------------------------------------------------------------
// One wave (a workgroup of 64): deflate block b, the chunks [c0, c1) of the stream F of N bytes, the stream's last block
// when b == last.  tabs, hdrs: block b's kTab and kHdrWords words are written; len_out[c]: the bits of chunk c of the
// stream (the header's with the block's first chunk, the end-of-block symbol's with its last).
__device__ __forceinline__ void deflate_block(const uint8_t* __restrict__ F, int N, int c0, int c1, int b, int last,
                                              uint32_t* __restrict__ tabs, uint32_t* __restrict__ hdrs,
                                              int32_t* __restrict__ len_out) {
    __shared__ int s_freq[kTab], s_len[kTab], s_sorted[kTab], s_wt[2 * kTab], s_par[2 * kTab], s_cnt[16];
    __shared__ int s_clfreq[19], s_cllen[19];
    __shared__ uint32_t s_tab[kTab], s_cltab[19], s_hdr[kHdrWords];
    __shared__ uint32_t s_next[16];
    __shared__ int s_pick[3];   // [1]: header bits
    __shared__ uint32_t s_tile[kRound * kLdsStride / 4];
    const int lane = (int)threadIdx.x;
    const int end = min(c1 * kChunk, N);
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
    const bool final_block = b == last;
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

// One wave: the bits of deflate block b, the chunks [c0, c1) of the stream, into S.  off[c]: the exclusive scan of the
// stream's chunk bit lengths; the deflate stream starts at bit `first` of S, whose words were zeroed.
__device__ __forceinline__ void deflate_emit(const uint8_t* __restrict__ F, int N, int c0, int c1, int b,
                                             const uint32_t* __restrict__ tabs, const uint32_t* __restrict__ hdrs,
                                             const int32_t* __restrict__ off, int first, uint32_t* __restrict__ S) {
    __shared__ uint32_t s_tab[kTab];
    __shared__ uint32_t s_tile[kRound * kLdsStride / 4];
    const int lane = (int)threadIdx.x;
    const int end = min(c1 * kChunk, N);
    for (int s = lane; s < kTab; s += 64) s_tab[s] = tabs[(size_t)b * kTab + s];
    __syncthreads();
    const int dist_bits = (int)s_tab[286], hdr_bits = (int)s_tab[287];
    for (int r0 = c0; r0 < c1; r0 += kRound) {
        __syncthreads();
        stage_round(F, r0, end, s_tile);
        __syncthreads();
        const int c = r0 + lane;
        if (lane >= kRound || c >= c1) continue;
        EmitSink es{s_tab, dist_bits, BitWriter(S, first + off[c])};
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

// ---- Adler-32 -------------------------------------------------------------------------------------------
// s1 = 1 + sum d_i, s2 = N + sum (N - i) d_i (mod 65521).  A lane's 16 bytes [at, e): (N - e) sum + sum (e - i) d_i.
// Every lane of a workgroup of 256 calls it for piece `piece` of F (N bytes, padded to 16): *p_sum the piece's sum of bytes
// (below 2^21), *p_term its s2 term, the sum of 256 terms below 65521 (the caller reduces it).  s_w: 4 words of LDS.
__device__ __forceinline__ void adler_piece(const uint8_t* __restrict__ F, int N, int piece, int* s_w, int* p_sum, int* p_term) {
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
    (void)block_excl_scan((int)sum, s_w, p_sum);
    (void)block_excl_scan((int)term, s_w, p_term);   // 256 terms below 65521
}

}  // namespace
}  // namespace deflate
}  // namespace pt
