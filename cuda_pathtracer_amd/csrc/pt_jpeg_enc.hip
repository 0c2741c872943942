// Baseline JPEG encoder on the device (pt_jpeg_enc), gfx950: JFIF, YCbCr 4:4:4 or 4:2:0,
// the Annex K quantisation tables under the IJG quality rule, the four Annex K Huffman tables, one scan
// without restart markers.  Every operation is an exactly defined int32 operation, so the file's bytes are
// a function of the input bytes alone; tests/jpeg_enc_ref.py restates the definition in numpy integers and
// the GPU tests compare byte for byte.
//
// Kernel shape: no inter-workgroup wait, no co-resident grid, no look-back; the prefix sums, and the host side that
// every encoder object has, are the shared unit's (pt_enc.h).
//   k_jpeg_blocks   8 lanes per 8x8 block (lane = row, then lane = column), 32 blocks per workgroup: colour
//                   conversion (the accumulator variant fuses k_preview's bytes), edge replication, 4:2:0
//                   averaging (an MCU's Cb and Cr lanes split the row's pixels and swap halves), the row pass into LDS (transposed, block stride 72 words: conflict-free on
//                   both sides), the column pass, quantisation, and the zigzag through LDS so that a lane
//                   stores 16 contiguous bytes of the block's 128
//   k_jpeg_count    one lane per block: the bit length of its code
//   scan            exclusive scan of the bit lengths, in place (pt::scan_exclusive_i32)
//   k_jpeg_zero     the words of the unstuffed stream up to the total length
//   k_jpeg_emit     one lane per block: the code assembled in a 64-bit register; words wholly inside the
//                   block's bit range are stored, the first and last are ORed in (atomicOr)
//   k_stuff_*       0xFF bytes per 4096-byte chunk (16 bytes per lane), their scan (pt::scan_tile_sums_i32), and the stuffed bytes
//                   behind the header in the caller's buffer, then FF D9 and the size word
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "pt_enc.h"

using namespace pt;

namespace {

constexpr int kHeaderBytes = 623;
constexpr int kBlockBitsMax = 1664;   // 20 (DC) + 63 * 26 (AC)
constexpr int kTile = 32;             // 8x8 blocks per workgroup of k_jpeg_blocks
constexpr int kRowPad = 72;           // words per block of the row pass in LDS
constexpr int kStuffChunk = 4096;     // bytes per workgroup of the stuffing kernels (16 per lane)
constexpr int kStages = 5;            // blocks, count, scan, emit, stuff (pt_jpeg_enc_profile)

// T[u][x] = round(2^13 s(u) cos((2x + 1) u pi / 16)), s(0) = sqrt(1/8), s(u) = 1/2
constexpr int kT[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},
                          {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                          {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},
                          {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                          {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},
                          {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                          {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},
                          {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// zigzag position -> natural index (ITU T.81 figure A.6), and its inverse for the kernel
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
__device__ __constant__ uint8_t c_zig_of[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                                                3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                                10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                                21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// ITU T.81 Annex K.1 (natural order) and K.3 (BITS, HUFFVAL)
constexpr uint8_t kQLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                  99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// What the kernels read of an encoder: the scaled quantisation tables (natural order; luma, chroma), the
// Huffman codes as (length << 16 | code) indexed by symbol (DC then AC; luma, chroma) and the file header.
struct Tables {
    int32_t q[128];
    uint32_t huff[2 * 16 + 2 * 256];
    uint8_t header[640];
};
constexpr int kHuffWords = 2 * 16 + 2 * 256;

struct Geo {
    int W, H, sub, mirror, mcus_x, nblocks;
};

// ---- blocks ---------------------------------------------------------------------------------------------
// The bytes of source pixel (x, y).
template <bool ACC>
__device__ __forceinline__ void rgb_at(const void* __restrict__ src, int stride, float n, int W, int x, int y, int& r,
                                       int& g, int& b) {
    const size_t i = (size_t)y * W + x;
    if (ACC) {
        const float* a = (const float*)src + 3 * i;
        r = preview_byte(a[0], n);
        g = preview_byte(a[1], n);
        b = preview_byte(a[2], n);
    } else {
        const uint8_t* p = (const uint8_t*)src + i * stride;
        r = p[0];
        g = p[1];
        b = p[2];
    }
}

// The JFIF matrix in 16-bit fixed point.  The chroma rounding term is 2^15 - 1, with which every result lies
// in 0..255.
constexpr int kChromaOff = (128 << 16) + 32767;
__device__ __forceinline__ int cb_of(int r, int g, int b) { return (-11058 * r - 21710 * g + 32768 * b + kChromaOff) >> 16; }
__device__ __forceinline__ int cr_of(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + kChromaOff) >> 16; }

template <bool ACC>
__global__ __launch_bounds__(256) void k_jpeg_blocks(const void* __restrict__ src, int stride, float n, Geo g,
                                                      const int32_t* __restrict__ q, int16_t* __restrict__ coef) {
    __shared__ int32_t s_r[kTile * kRowPad];                 // [block][u][y]
    __shared__ __attribute__((aligned(16))) int16_t s_o[kTile * 64];
    const int lb = (int)threadIdx.x >> 3, r = (int)threadIdx.x & 7;
    const int b = (int)blockIdx.x * kTile + lb;
    const bool valid = b < g.nblocks;
    int comp = 0;
    if (valid) {
        int ox, oy, step = 1;   // the block's first pixel, and pixels per sample
        if (g.sub == PT_JPEG_444) {
            const int mcu = b / 3;
            comp = b - 3 * mcu;
            const int my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
            ox = 8 * mx;
            oy = 8 * my;
        } else {
            const int mcu = b / 6, k = b - 6 * mcu;
            const int my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
            ox = 16 * mx;
            oy = 16 * my;
            if (k < 4) {
                ox += 8 * (k & 1);
                oy += 8 * (k >> 1);
            } else {
                comp = k - 3;
                step = 2;
            }
        }
        int d[8];
        if (step == 1) {
            const int y = min(oy + r, g.H - 1);
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int xs = min(ox + x, g.W - 1);
                int pr, pg, pb;
                rgb_at<ACC>(src, stride, n, g.W, g.mirror ? g.W - 1 - xs : xs, y, pr, pg, pb);
                const int v = comp == 0 ? (19595 * pr + 38470 * pg + 7471 * pb + 32768) >> 16
                                        : (comp == 1 ? cb_of(pr, pg, pb) : cr_of(pr, pg, pb));
                d[x] = v - 128;
            }
        } else {
            // An MCU's Cb and Cr blocks are neighbours, b even and b + 1: lanes l and l ^ 8 of one wave hold the same
            // row of the same 16 x 16 pixels.  Each converts one half of the row (Cb lane: samples 0..3, Cr lane:
            // 4..7) to both components, keeps its own and hands the other lane the rest.
            const bool second = comp == 2;
            int mine[4], theirs[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = j + (second ? 4 : 0);
                int scb = 2, scr = 2;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int xs = min(ox + 2 * x + (k & 1), g.W - 1), y = min(oy + 2 * r + (k >> 1), g.H - 1);
                    int pr, pg, pb;
                    rgb_at<ACC>(src, stride, n, g.W, g.mirror ? g.W - 1 - xs : xs, y, pr, pg, pb);
                    scb += cb_of(pr, pg, pb);
                    scr += cr_of(pr, pg, pb);
                }
                const int vcb = (scb >> 2) - 128, vcr = (scr >> 2) - 128;
                mine[j] = second ? vcr : vcb;
                theirs[j] = second ? vcb : vcr;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int got = __shfl_xor(theirs[j], 8, 64);
                d[j] = second ? got : mine[j];
                d[j + 4] = second ? mine[j] : got;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int acc = 256;
#pragma unroll
            for (int x = 0; x < 8; ++x) acc += kT[u][x] * d[x];
            s_r[lb * kRowPad + u * 8 + r] = acc >> 9;
        }
    }
    __syncthreads();
    if (valid) {
        const int u = r;
        int row[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) row[y] = s_r[lb * kRowPad + u * 8 + y];
        const int32_t* qt = q + (comp ? 64 : 0);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            int f = 0;
#pragma unroll
            for (int y = 0; y < 8; ++y) f += kT[v][y] * row[y];
            const uint32_t qv = (uint32_t)qt[v * 8 + u];
            int m = (int)(((uint32_t)abs(f) + (qv << 16)) / (qv << 17));
            if (f < 0) m = -m;
            const int lo = (v | u) == 0 ? -1024 : -1023;
            m = m < lo ? lo : (m > 1023 ? 1023 : m);
            s_o[lb * 64 + c_zig_of[v * 8 + u]] = (int16_t)m;
        }
    }
    __syncthreads();
    if (valid)
        *reinterpret_cast<uint4*>(coef + (size_t)b * 64 + r * 8) = *reinterpret_cast<const uint4*>(s_o + lb * 64 + r * 8);
}

// ---- entropy coding -------------------------------------------------------------------------------------
// The previous block of the same component in scan order (-1: none) and the block's table (0 luma, 1 chroma).
__device__ __forceinline__ int prev_block(int b, int sub) {
    if (sub == PT_JPEG_444) return b - 3;
    const int k = b % 6;
    if (k >= 4) return b - 6;
    if (k > 0) return b - 1;
    return b >= 6 ? b - 3 : -1;
}
__device__ __forceinline__ int table_of(int b, int sub) { return sub == PT_JPEG_444 ? (b % 3 != 0) : (b % 6 >= 4); }

struct BitCounter {
    int bits = 0;
    __device__ __forceinline__ void put(uint32_t, int len) { bits += len; }
};

// The code of one block from bit `off` of the stream (bits big-endian within bytes, so a word is stored
// byte-swapped): nb < 32 bits of the current word are taken, acc holds them from its top.
struct BitWriter {
    uint32_t* buf;
    uint32_t w;
    uint64_t acc = 0;
    int nb;
    bool shared;   // the current word also holds another block's bits
    __device__ __forceinline__ BitWriter(uint32_t* stream, int off) : buf(stream), w((uint32_t)off >> 5), nb(off & 31), shared((off & 31) != 0) {}
    __device__ __forceinline__ void put(uint32_t bits, int len) {   // len <= 26
        acc |= (uint64_t)bits << (64 - nb - len);
        nb += len;
        if (nb >= 32) {
            const uint32_t word = __builtin_bswap32((uint32_t)(acc >> 32));
            if (shared) atomicOr(buf + w, word);
            else buf[w] = word;
            shared = false;
            ++w;
            acc <<= 32;
            nb -= 32;
        }
    }
    __device__ __forceinline__ void finish(bool last) {
        if (last) {   // the final byte padded with 1-bits
            const int pad = (8 - (nb & 7)) & 7;
            acc |= (((uint64_t)1 << pad) - 1) << (64 - nb - pad);
            nb += pad;
        }
        if (nb > 0) atomicOr(buf + w, __builtin_bswap32((uint32_t)(acc >> 32)));
    }
};

template <class Sink>
__device__ __forceinline__ void put_value(uint32_t entry, int v, int s, Sink& sink) {
    const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
    sink.put(((entry & 0xffffu) << s) | extra, (int)(entry >> 16) + s);
}

// c: the block's 64 zigzag coefficients; dc / ac: its tables in LDS
template <class Sink>
__device__ __forceinline__ void walk_block(const int16_t* __restrict__ c, int pred, const uint32_t* dc, const uint32_t* ac,
                                           Sink& sink) {
    int run = 0;
    for (int q = 0; q < 8; ++q) {
        const uint4 v4 = reinterpret_cast<const uint4*>(c)[q];
        const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int v = (int)(int16_t)(w[j >> 1] >> (16 * (j & 1)));
            if (j == 0 && q == 0) {
                const int d = v - pred, s = 32 - __clz(abs(d));
                put_value(dc[s], d, s, sink);
                continue;
            }
            if (v == 0) {
                ++run;
                continue;
            }
            for (; run >= 16; run -= 16) sink.put(ac[0xF0] & 0xffffu, (int)(ac[0xF0] >> 16));   // ZRL
            const int s = 32 - __clz(abs(v));
            put_value(ac[(run << 4) | s], v, s, sink);
            run = 0;
        }
    }
    if (run > 0) sink.put(ac[0] & 0xffffu, (int)(ac[0] >> 16));   // EOB
}

__device__ __forceinline__ void load_huff(const uint32_t* __restrict__ huff, uint32_t* s_huff) {
    for (int i = (int)threadIdx.x; i < kHuffWords; i += 256) s_huff[i] = huff[i];
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_jpeg_count(const int16_t* __restrict__ coef, const uint32_t* __restrict__ huff,
                                                     int32_t* __restrict__ len, int nblocks, int sub) {
    __shared__ uint32_t s_huff[kHuffWords];
    load_huff(huff, s_huff);
    const int b = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (b >= nblocks) return;
    const int p = prev_block(b, sub), t = table_of(b, sub);
    BitCounter cnt;
    walk_block(coef + (size_t)b * 64, p >= 0 ? (int)coef[(size_t)p * 64] : 0, s_huff + 16 * t, s_huff + 32 + 256 * t, cnt);
    len[b] = cnt.bits;
}

__global__ __launch_bounds__(256) void k_jpeg_emit(const int16_t* __restrict__ coef, const uint32_t* __restrict__ huff,
                                                    const int32_t* __restrict__ off, uint32_t* __restrict__ stream,
                                                    int nblocks, int sub) {
    __shared__ uint32_t s_huff[kHuffWords];
    load_huff(huff, s_huff);
    const int b = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (b >= nblocks) return;
    const int p = prev_block(b, sub), t = table_of(b, sub);
    BitWriter wr(stream, off[b]);
    walk_block(coef + (size_t)b * 64, p >= 0 ? (int)coef[(size_t)p * 64] : 0, s_huff + 16 * t, s_huff + 32 + 256 * t, wr);
    wr.finish(b == nblocks - 1);
}

__global__ __launch_bounds__(256) void k_jpeg_zero(uint32_t* __restrict__ stream, const int32_t* __restrict__ tot) {
    const int words = (tot[0] + 31) >> 5;
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < words; i += (int)gridDim.x * 256) stream[i] = 0u;
}

// ---- byte stuffing --------------------------------------------------------------------------------------
// The lane's 16 bytes of the unstuffed stream (those below nbytes) and how many of them are 0xFF.
__device__ __forceinline__ int stuff_load(const uint8_t* __restrict__ stream, int at, int nbytes, uint32_t (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (at >= nbytes) return 0;
    const uint4 v = *reinterpret_cast<const uint4*>(stream + at);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) cnt += (at + j < nbytes && ((w[j >> 2] >> (8 * (j & 3))) & 0xffu) == 0xffu) ? 1 : 0;
    return cnt;
}

// *nchunks: the chunks of the unstuffed stream, for the scan of their sums.
__global__ __launch_bounds__(256) void k_stuff_count(const uint8_t* __restrict__ stream, const int32_t* __restrict__ tot,
                                                      int32_t* __restrict__ sums, int32_t* __restrict__ nchunks) {
    __shared__ int s_w[4];
    const int nbytes = (tot[0] + 7) >> 3;
    if (blockIdx.x == 0 && threadIdx.x == 0) *nchunks = (nbytes + kStuffChunk - 1) / kStuffChunk;
    for (int tile = (int)blockIdx.x; tile * kStuffChunk < nbytes; tile += (int)gridDim.x) {
        uint32_t w[4];
        int total;
        const int cnt = stuff_load(stream, tile * kStuffChunk + (int)threadIdx.x * 16, nbytes, w);
        (void)block_excl_scan(cnt, s_w, &total);
        if (threadIdx.x == 0) sums[tile] = total;
    }
}

// tot[0]: the stream's bits; tot[1]: its 0xFF bytes (tot[2]: k_stuff_count's chunks).  Nothing at or beyond out + cap is written.
__global__ __launch_bounds__(256) void k_stuff_write(const uint8_t* __restrict__ stream, const int32_t* __restrict__ tot,
                                                      const int32_t* __restrict__ sums, const uint8_t* __restrict__ header,
                                                      uint8_t* __restrict__ out, long long cap, long long* __restrict__ size) {
    __shared__ int s_w[4];
    const int nbytes = (tot[0] + 7) >> 3;
    const int gid = (int)blockIdx.x * 256 + (int)threadIdx.x;
    for (int i = gid; i < kHeaderBytes; i += (int)gridDim.x * 256)
        if (i < cap) out[i] = header[i];
    for (int tile = (int)blockIdx.x; tile * kStuffChunk < nbytes; tile += (int)gridDim.x) {
        uint32_t w[4];
        int total;
        const int at = tile * kStuffChunk + (int)threadIdx.x * 16;
        const int cnt = stuff_load(stream, at, nbytes, w);
        long long dst = (long long)kHeaderBytes + at + sums[tile] + block_excl_scan(cnt, s_w, &total);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (at + j >= nbytes) break;
            const uint8_t byte = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
            if (dst < cap) out[dst] = byte;
            ++dst;
            if (byte == 0xffu) {
                if (dst < cap) out[dst] = 0u;
                ++dst;
            }
        }
    }
    if (gid == 0) {
        const long long end = (long long)kHeaderBytes + nbytes + tot[1];
        if (end < cap) out[end] = 0xffu;
        if (end + 1 < cap) out[end + 1] = 0xd9u;
        *size = end + 2 <= cap ? end + 2 : -(end + 2);
    }
}

// ---- host: tables and header ------------------------------------------------------------------------------
void quant_table(const uint8_t (&base)[64], int quality, int32_t* out) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) out[k] = std::min(std::max((base[k] * scale + 50) / 100, 1), 255);
}

// Canonical codes (T.81 Annex C) of one table: out[symbol] = length << 16 | code
void huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
}

void segment(std::vector<uint8_t>& out, uint8_t marker, const std::vector<uint8_t>& body) {
    const size_t n = body.size() + 2;
    out.insert(out.end(), {0xff, marker, (uint8_t)(n >> 8), (uint8_t)(n & 0xff)});
    out.insert(out.end(), body.begin(), body.end());
}

void fill_tables(Tables& t, int32_t W, int32_t H, const pt_jpeg_params& p) {
    t = Tables{};
    quant_table(kQLuma, p.quality, t.q);
    quant_table(kQChroma, p.quality, t.q + 64);
    uint8_t dcvals[12];
    for (int i = 0; i < 12; ++i) dcvals[i] = (uint8_t)i;
    for (int c = 0; c < 2; ++c) {
        huff_codes(kDcBits[c], dcvals, t.huff + 16 * c);
        huff_codes(kAcBits[c], kAcVals[c], t.huff + 32 + 256 * c);
    }
    std::vector<uint8_t> h = {0xff, 0xd8};
    segment(h, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int c = 0; c < 2; ++c) {
        std::vector<uint8_t> body = {(uint8_t)c};
        for (int k = 0; k < 64; ++k) body.push_back((uint8_t)t.q[64 * c + kZigzag[k]]);
        segment(h, 0xdb, body);
    }
    const uint8_t hv = p.subsampling == PT_JPEG_444 ? 0x11 : 0x22;
    segment(h, 0xc0, {8, (uint8_t)(H >> 8), (uint8_t)(H & 0xff), (uint8_t)(W >> 8), (uint8_t)(W & 0xff), 3, 1, hv, 0, 2, 0x11,
                      1, 3, 0x11, 1});
    for (int c = 0; c < 2; ++c)
        for (int ac = 0; ac < 2; ++ac) {
            const uint8_t* bits = ac ? kAcBits[c] : kDcBits[c];
            std::vector<uint8_t> body = {(uint8_t)((ac << 4) | c)};
            body.insert(body.end(), bits, bits + 16);
            if (ac) body.insert(body.end(), kAcVals[c], kAcVals[c] + 162);
            else body.insert(body.end(), dcvals, dcvals + 12);
            segment(h, 0xc4, body);
        }
    segment(h, 0xda, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    std::copy(h.begin(), h.end(), t.header);   // (kHeaderBytes of them: pt_jpeg_enc_create checks)
    t.header[639] = (uint8_t)(h.size() == (size_t)kHeaderBytes);
}

}  // namespace

struct pt_jpeg_enc : EncHead {
    pt_jpeg_enc() : EncHead("JPEG", "jpeg", kStages) {}
    pt_jpeg_params prm{};
    Geo geo{};
    int64_t worst = 0;                // bytes of the unstuffed stream at most: nblocks * 1664 / 8
    Tables tables{};
    // The device side: tables | coefficients | bit lengths, then offsets | unstuffed stream | the two scans' tile
    // sums | totals (bits, 0xFF bytes, stuffing chunks).
    Tables* d_tab = nullptr;
    int16_t* d_coef = nullptr;
    int32_t* d_len = nullptr;
    uint32_t* d_stream = nullptr;
    int32_t *d_sums1 = nullptr, *d_sums2 = nullptr, *d_tot = nullptr;
};

const EncHead* pt::enc_head(const pt_jpeg_enc* e) { return e; }

namespace {

int params_check(const pt_jpeg_params* p) {
    if (!p) return pt::fail(PT_ERR_ARG, "null JPEG parameters");
    if (p->quality < 1 || p->quality > 100) return pt::fail(PT_ERR_ARG, "JPEG quality must be in 1..100");
    if (p->subsampling != PT_JPEG_444 && p->subsampling != PT_JPEG_420)
        return pt::fail(PT_ERR_ARG, "JPEG subsampling must be PT_JPEG_444 or PT_JPEG_420");
    for (int32_t r : p->reserved)
        if (r != 0) return pt::fail(PT_ERR_ARG, "pt_jpeg_params.reserved must be zero");
    return PT_OK;
}

int64_t blocks_of(int64_t W, int64_t H, int32_t sub) {
    return sub == PT_JPEG_444 ? 3 * ((W + 7) / 8) * ((H + 7) / 8) : 6 * ((W + 15) / 16) * ((H + 15) / 16);
}

int size_check(int32_t W, int32_t H, int32_t sub) {
    if (W < 1 || H < 1 || W > 65535 || H > 65535) return pt::fail(PT_ERR_ARG, "JPEG width and height must be in 1..65535");
    if (blocks_of(W, H, sub) * kBlockBitsMax >= ((int64_t)1 << 31))
        return pt::fail(PT_ERR_ARG, "JPEG image too large: the bit offsets of its blocks must stay below 2^31");
    return PT_OK;
}

int je_alloc(pt_jpeg_enc* e) {
    if (e->dev) return PT_OK;
    const size_t nb = (size_t)e->geo.nblocks, worst = (size_t)e->worst;
    uint8_t* p[7];
    if (int rc = enc_alloc(e, {sizeof(Tables), nb * 128, nb * 4, worst + 16, (nb / kScanTile + 1) * 4, (worst / kStuffChunk + 1) * 4, 256},
                           p, &e->tables, "tables"))
        return rc;
    e->d_tab = (Tables*)p[0];
    e->d_coef = (int16_t*)p[1];
    e->d_len = (int32_t*)p[2];
    e->d_stream = (uint32_t*)p[3];
    e->d_sums1 = (int32_t*)p[4];
    e->d_sums2 = (int32_t*)p[5];
    e->d_tot = (int32_t*)p[6];
    return PT_OK;
}

// src: pixels (stride 3 or 4) or, with acc, the float accumulator of `samples` samples.
int encode(pt_jpeg_enc* e, const void* src, int stride, bool acc, float samples, uint8_t* d_out, int64_t cap,
           int64_t* d_size, hipStream_t st) {
    if (int rc = je_alloc(e)) return rc;
    const Geo& g = e->geo;
    const int nb = g.nblocks;
    if (int rc = enc_stage(e, 0, st)) return rc;
    auto blocks = acc ? k_jpeg_blocks<true> : k_jpeg_blocks<false>;
    hipLaunchKernelGGL(blocks, dim3((nb + kTile - 1) / kTile), dim3(256), 0, st, src, stride, samples, g,
                       (const int32_t*)e->d_tab->q, e->d_coef);
    if (int rc = enc_stage(e, 1, st)) return rc;
    const uint32_t* huff = e->d_tab->huff;
    hipLaunchKernelGGL(k_jpeg_count, dim3((nb + 255) / 256), dim3(256), 0, st, (const int16_t*)e->d_coef, huff, e->d_len, nb,
                       g.sub);
    if (int rc = enc_stage(e, 2, st)) return rc;
    scan_exclusive_i32(e->d_len, nb, e->d_sums1, e->d_tot, st);
    if (int rc = enc_stage(e, 3, st)) return rc;
    hipLaunchKernelGGL(k_jpeg_zero, dim3(grid_of(e->worst / 4 + 1, 256)), dim3(256), 0, st, e->d_stream,
                       (const int32_t*)e->d_tot);
    hipLaunchKernelGGL(k_jpeg_emit, dim3((nb + 255) / 256), dim3(256), 0, st, (const int16_t*)e->d_coef, huff,
                       (const int32_t*)e->d_len, e->d_stream, nb, g.sub);
    if (int rc = enc_stage(e, 4, st)) return rc;
    const int grid2 = grid_of(e->worst, kStuffChunk);
    const uint8_t* stream = (const uint8_t*)e->d_stream;
    hipLaunchKernelGGL(k_stuff_count, dim3(grid2), dim3(256), 0, st, stream, (const int32_t*)e->d_tot, e->d_sums2, e->d_tot + 2);
    scan_tile_sums_i32(e->d_sums2, e->d_tot + 2, e->d_tot + 1, st);
    hipLaunchKernelGGL(k_stuff_write, dim3(grid2), dim3(256), 0, st, stream, (const int32_t*)e->d_tot,
                       (const int32_t*)e->d_sums2, (const uint8_t*)e->d_tab->header, d_out, (long long)cap,
                       (long long*)d_size);
    return enc_done(e, st);
}

}  // namespace

extern "C" {

void pt_jpeg_params_default(pt_jpeg_params* p) {
    if (!p) return;
    *p = pt_jpeg_params{};
    p->quality = 90;
    p->subsampling = PT_JPEG_420;
}

int pt_jpeg_enc_create(int32_t width, int32_t height, const pt_jpeg_params* p, pt_jpeg_enc** out) {
    if (!out) return pt::fail(PT_ERR_ARG, "null argument");
    if (int rc = params_check(p)) return rc;
    if (int rc = size_check(width, height, p->subsampling)) return rc;
    pt_jpeg_enc* e = new pt_jpeg_enc;   // (the device side comes with the first encode: je_alloc)
    e->W = width;
    e->H = height;
    e->prm = *p;
    const int m = p->subsampling == PT_JPEG_444 ? 8 : 16;
    e->geo = Geo{width, height, p->subsampling, p->mirror_x ? 1 : 0, (width + m - 1) / m,
                 (int)blocks_of(width, height, p->subsampling)};
    e->worst = (int64_t)e->geo.nblocks * kBlockBitsMax / 8;
    fill_tables(e->tables, width, height, *p);
    if (!e->tables.header[639]) {
        delete e;
        return pt::fail(PT_ERR_ARG, "internal: JPEG header length");
    }
    *out = e;
    return PT_OK;
}

int pt_jpeg_enc_destroy(pt_jpeg_enc* e) {
    delete e;   // (~EncHead waits for the last encode)
    return PT_OK;
}

int64_t pt_jpeg_enc_bound(const pt_jpeg_enc* e) { return e ? kHeaderBytes + 2 * e->worst + 2 : 0; }

int64_t pt_jpeg_enc_header(const pt_jpeg_enc* e, uint8_t* out, int64_t cap) {
    if (!e) return 0;
    if (out && cap > 0) std::copy(e->tables.header, e->tables.header + std::min<int64_t>(cap, kHeaderBytes), out);
    return kHeaderBytes;
}

int pt_jpeg_enc_pixels(pt_jpeg_enc* e, const uint8_t* d_pix, int32_t pixel_stride, uint8_t* d_out, int64_t cap,
                       int64_t* d_size, void* stream) {
    if (int rc = encode_check(e, d_pix, d_out, cap, d_size)) return rc;
    if (pixel_stride != 3 && pixel_stride != 4) return pt::fail(PT_ERR_ARG, "the pixel stride must be 3 or 4");
    return encode(e, d_pix, pixel_stride, false, 1.0f, d_out, cap, d_size, (hipStream_t)stream);
}

int pt_jpeg_enc_accum(pt_jpeg_enc* e, const float* d_rgb, float samples, uint8_t* d_out, int64_t cap, int64_t* d_size,
                      void* stream) {
    if (int rc = encode_check(e, d_rgb, d_out, cap, d_size)) return rc;
    if (!std::isfinite(samples) || !(samples > 0.0f)) return pt::fail(PT_ERR_ARG, "samples must be finite and > 0");
    return encode(e, d_rgb, 0, true, samples, d_out, cap, d_size, (hipStream_t)stream);
}

int pt_jpeg_encode_host(int32_t width, int32_t height, const uint8_t* pix, int32_t pixel_stride, const pt_jpeg_params* p,
                        uint8_t* out, int64_t cap, int64_t* size) {
    return encode_host(pt_jpeg_enc_create, pt_jpeg_enc_bound, pt_jpeg_enc_pixels, width, height, pix, pixel_stride, p, out, cap, size);
}

int pt_jpeg_enc_profile(pt_jpeg_enc* e, int32_t on) {
    if (!e) return pt::fail(PT_ERR_ARG, "null JPEG encoder");
    return enc_profile(e, on);
}

int pt_jpeg_enc_profile_read(pt_jpeg_enc* e, float ms[5]) { return enc_profile_read(e, ms); }

}  // extern "C"
