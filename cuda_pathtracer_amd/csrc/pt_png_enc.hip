// PNG encoder on the device (pt_png_enc), gfx950: 8-bit RGB, one IDAT holding one zlib stream.
// The filtered stream F (libpng's five row filters, fixed or chosen per row by the smallest sum of |signed
// residual|) is cut into lane chunks of kChunk bytes; a chunk is tokenised greedily into literals and matches
// of distance 1 (runs of the previous byte), and every block_bytes of F form one deflate block coded with the
// fixed or a dynamic Huffman code, whichever is shorter.  Every step is an integer operation, so the file is a
// function of the input bytes; tests/png_enc_ref.py restates the definition and the GPU tests compare byte for
// byte.
//
// Kernel shape: no inter-workgroup wait, no co-resident grid, no look-back; the prefix sum, and the host side that
// every encoder object has, are the shared unit's (pt_enc.h); the deflate coder of a stream, which the OpenEXR encoder
// runs once per chunk, is pt_deflate_dev.h's (deflate_block, deflate_emit, adler_piece).
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

#include "pt_deflate_dev.h"
#include "pt_enc.h"

using namespace pt;
using namespace pt::deflate;

namespace {

constexpr int kFraming = 63;           // signature 8, IHDR 25, IDAT 12, zlib header 2, Adler-32 4, IEND 12
constexpr int kPayloadAt = 37;         // "IDAT" in the file: the stream buffer S starts with it
constexpr int kCrcPiece = 256;         // bytes of the payload per lane of k_png_crc
constexpr uint32_t kCrcPoly = 0xedb88320u;
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

// The chunks of deflate block b: [c0, c1), and the block's end in F.
__device__ __forceinline__ void block_range(const Geo& g, int b, int& c0, int& c1) {
    const int per = g.block_bytes / kChunk;
    c0 = b * per;
    c1 = min(c0 + per, g.nchunks);
}

__global__ __launch_bounds__(64) void k_png_block(const uint8_t* __restrict__ F, Geo g, uint32_t* __restrict__ tabs,
                                                   uint32_t* __restrict__ hdrs, int32_t* __restrict__ len_out) {
    const int b = (int)blockIdx.x;
    int c0, c1;
    block_range(g, b, c0, c1);
    deflate_block(F, g.N, c0, c1, b, g.nblocks - 1, tabs, hdrs, len_out);
}

// off: the exclusive scan of the chunk bit lengths; the deflate stream starts at bit 48 of S.
__global__ __launch_bounds__(64) void k_png_emit(const uint8_t* __restrict__ F, Geo g, const uint32_t* __restrict__ tabs,
                                                  const uint32_t* __restrict__ hdrs, const int32_t* __restrict__ off,
                                                  uint32_t* __restrict__ S) {
    const int b = (int)blockIdx.x;
    int c0, c1;
    block_range(g, b, c0, c1);
    deflate_emit(F, g.N, c0, c1, b, tabs, hdrs, off, 48, S);
}

// S: "IDAT", the zlib header 78 01, the deflate stream of tot[0] bits, the Adler-32.
__device__ __forceinline__ int payload_bytes(const int32_t* tot) { return 10 + ((tot[0] + 7) >> 3); }

__global__ __launch_bounds__(256) void k_png_zero(uint32_t* __restrict__ S, const int32_t* __restrict__ tot) {
    const int words = (payload_bytes(tot) + 3) >> 2;
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < words; i += (int)gridDim.x * 256)
        S[i] = i == 0 ? 0x54414449u : (i == 1 ? 0x0178u : 0u);
}

// ---- Adler-32 -------------------------------------------------------------------------------------------
// part[2 p], part[2 p + 1]: piece p's sum of bytes (below 2^21) and its s2 term mod 65521 (deflate::adler_piece).
__global__ __launch_bounds__(256) void k_adler_part(const uint8_t* __restrict__ F, int N, uint32_t* __restrict__ part) {
    __shared__ int s_w[4];
    for (int piece = (int)blockIdx.x; piece * kAdlerPiece < N; piece += (int)gridDim.x) {
        int t_sum, t_term;
        adler_piece(F, N, piece, s_w, &t_sum, &t_term);
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
