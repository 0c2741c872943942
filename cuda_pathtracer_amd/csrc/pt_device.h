// Device-side math for the MI355X path tracer (gfx950, wave64).
//
// Evaluation contract: this file is compiled with -ffp-contract=off, so every
// a*b+c below is a separate correctly-rounded multiply and add unless fmaf() is written; the
// association follows glm 0.9.6.3 as used by the reference (dot = (xx'+yy')+zz',
// mat*vec = (m0 v0 + m1 v1) + (m2 v2 + m3 v3), normalize = v * (1/sqrt(dot))).  hipcc lowers
// sqrtf and '/' to correctly-rounded sequences on gfx950, so the kernels reproduce the CPU
// oracle bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_layout.h"

namespace ptd {

struct f3 { float x, y, z; };
__device__ __forceinline__ f3 F3(float x, float y, float z) { return f3{x, y, z}; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return F3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return F3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 operator-(f3 a) { return F3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ f3 hadamard(f3 a, f3 b) { return F3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return F3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ f3 operator*(float s, f3 a) { return F3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ f3 operator/(f3 a, float s) { return F3(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ float dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ f3 cross(f3 a, f3 b) {
    return F3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y);
}

// ---- correctly rounded sqrt and division, range-gated --------------------------------------
// hipcc expands sqrtf into v_sqrt + two neighbour corrections, wrapped in a scaling step for tiny
// inputs and a zero/inf fix-up (16 instructions), and '/' into v_div_scale x2, v_rcp, a Newton
// step, two residual corrections (v_div_fmas) and v_div_fixup (11 instructions + hazard nops).
// For operands in a safe range the wrapping steps are identities, so the cores below — the same
// operations in the same order — return the same bits; outside it (or for 0, NaN, inf, denormal
// intermediates) the library form runs instead (a divergent branch, skipped when no lane needs it).
//   sqrt:  x in [2^-96, FLT_MAX]: no scaling, not zero/inf.
//   n / d: |n|, |d| in [2^-40, 2^40]: exponent gap < 96, no denormal 1/d or quotient, no tiny n,
//          no zero (a zero numerator's sign would not survive the residual steps).
// pt_selftest_math checks cores == library ops on the device over random and edge operands.
__device__ __forceinline__ float sqrt_core(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u);
    const float sp = __uint_as_float(__float_as_uint(s) + 1u);
    const float r1 = fmaf(-sm, s, x);
    const float s1 = r1 <= 0.0f ? sm : s;
    const float r2 = fmaf(-sp, s, x);
    return r2 > 0.0f ? sp : s1;
}
__device__ __forceinline__ bool sqrt_ok(float x) { return x >= 0x1p-96f && x <= 3.402823466e+38f; }
__device__ __forceinline__ float recip_core(float d) {   // v_rcp + one Newton step (the divisor's part)
    const float r = __builtin_amdgcn_rcpf(d);
    return fmaf(fmaf(-d, r, 1.0f), r, r);
}
__device__ __forceinline__ float div_core(float n, float d, float r) {
    float q = n * r;
    float e = fmaf(-d, q, n);
    q = fmaf(e, r, q);
    e = fmaf(-d, q, n);
    return fmaf(e, r, q);
}
__device__ __forceinline__ bool div_ok(float v) {
    const float a = fabsf(v);
    return a >= 0x1p-40f && a <= 0x1p+40f;
}
__device__ __forceinline__ float sqrt_cr(float x) {
    float s = sqrt_core(x);
    if (__builtin_expect(!sqrt_ok(x), 0)) s = sqrtf(x);
    return s;
}
__device__ __forceinline__ float div_cr(float n, float d) {
    float q = div_core(n, d, recip_core(d));
    if (__builtin_expect(!(div_ok(n) && div_ok(d)), 0)) q = n / d;
    return q;
}
// n1 / d and n2 / d sharing the divisor's reciprocal step
__device__ __forceinline__ void div2_cr(float n1, float n2, float d, float& q1, float& q2) {
    const float r = recip_core(d);
    q1 = div_core(n1, d, r);
    q2 = div_core(n2, d, r);
    if (__builtin_expect(!(div_ok(n1) && div_ok(n2) && div_ok(d)), 0)) {
        q1 = n1 / d;
        q2 = n2 / d;
    }
}
// glm normalize: v * (1 / sqrt(dot(v, v))); dot in [2^-80, 2^80] keeps sqrt and 1/sqrt in range
__device__ __forceinline__ f3 normalize(f3 v) {
    const float x = dot(v, v);
    const float s = sqrt_core(x);
    float inv = div_core(1.0f, s, recip_core(s));
    if (__builtin_expect(!(x >= 0x1p-80f && x <= 0x1p+80f), 0)) inv = 1.0f / sqrtf(x);
    return v * inv;
}
__device__ __forceinline__ float length(f3 v) { return sqrt_cr(dot(v, v)); }
// normalize's core for x = dot(v, v): what normalize returns when x passes its range test
__device__ __forceinline__ f3 norm_core(f3 v, float x) {
    const float s = sqrt_core(x);
    return v * div_core(1.0f, s, recip_core(s));
}

// ---- renormalising a vector that is already of unit length ----------------------------------
// getPointOnRay normalizes a direction that a normalize, a reflection or a hemisphere sample has just
// produced: x = dot(v, v) is within a few ulp of 1.  For x in [1 - 2^-12, 1 + 2^-12] the factor
// 1 / sqrt(x) of norm_core, both roundings included, is a function of x's signed distance from 1.0f
// in ulps, k = bits(x) - bits(1.0f) (one ulp is 2^-23 above 1 and 2^-24 below; k in [-4096, 2048]):
//   k >= 0:  sqrt(1 + k 2^-23) = 1 + (k/2) 2^-23 - (k^2/8) 2^-46 + ...: below 1 + (k/2) 2^-23 by less
//            than 2^-4 ulp, so it rounds to s = 1 + m 2^-23 with m = floor(k/2) (an odd k lies just
//            under the midpoint).  1 / s = 1 - 2m 2^-24 + m^2 2^-46 - ...: above 1 - 2m 2^-24 by at
//            most 2^-2 ulp (of 2^-24), so it rounds to it:            bits = bits(1) - (k & ~1);
//   k < 0:   with j = -k, sqrt(1 - j 2^-24) = 1 - (j/2) 2^-24 - (j^2/8) 2^-48 - ...: rounds to
//            s = 1 - m 2^-24 with m = ceil(j/2) (an odd j lies just beyond the midpoint).
//            1 / s = 1 + (m/2) 2^-23 + (m^2/2) 2^-47 + ...: above 1 + (m/2) 2^-23 by at most 2^-3 ulp,
//            so it rounds to 1 + ceil(m/2) 2^-23 = 1 + ceil(j/4) 2^-23:  bits = bits(1) + ((j + 3) >> 2).
// The argument is a guide only.  The proof is exhaustive: tests/test_renorm_unit_cpu.py compares the
// host restatement of unit_rnorm (pt_renorm.cpp) with the correctly rounded 1.0f / sqrtf(x) for every
// one of the 6,145 floats of the range, and tests/test_renorm_unit_gpu.py compares renorm_unit_core
// with norm_core on the device for the same values.  sqrt_core and div_core are correctly rounded on
// the whole range (pt_selftest_math), so the three agree.
// (unit_ok_bits, unit_rnorm_bits: pt_layout.h, shared with the host's restatement.)
__device__ __forceinline__ bool unit_ok(float x) { return unit_ok_bits(__float_as_uint(x)); }
// 1 / sqrt(x) as norm_core rounds it, for unit_ok(x)
__device__ __forceinline__ float unit_rnorm(float x) { return __uint_as_float(unit_rnorm_bits(__float_as_uint(x))); }
// norm_core(v, x), bit for bit, for every x: the closed form in range, norm_core's own operations
// behind a branch (cold where v is a unit vector) for every other x, zero, infinite and NaN included.
__device__ __forceinline__ f3 renorm_unit_core(f3 v, float x) {
    float inv = unit_rnorm(x);
    if (__builtin_expect(!unit_ok(x), 0)) {
        const float s = sqrt_core(x);
        inv = div_core(1.0f, s, recip_core(s));
    }
    return v * inv;
}

// ---- one range gate for a whole exact test (pt_kernels.hip exact_geom) --------
// The per-operation forms above pay a compare, an exec-mask region and a branch for each sqrt,
// division and normalize.  A fast path runs the cores unconditionally and feeds every gated operand
// to one RangeGate instead: two running unsigned words (v_add / v_sub, v_min3 / v_max3: no SGPR,
// no exec change), compared once at the end of the test.  ok() holds exactly
// when every operand fed passed the range its per-operation form states above:
//   div_lo / div_hi (the smallest and the largest magnitude of a group of division operands):
//            |v| in [2^-40, 2^40]   <=> bits(|v|) in [kLo, kHi]  (a float's order is its bit pattern's
//            for non-negative values; zero and denormals lie below kLo, inf above kHi);
//   norm(x): x in [2^-80, 2^80]     <=> u = bits(x) in [kLo - D, kHi + D] with D = 40 << 23.  mn takes
//            u + D, mx takes u - D.  u + D wraps only for u >= 2^32 - D (sign bit set: out of range) and
//            is then < D < kLo: tripped; u - D wraps only for u < D (x < 2^-87: out of range) and is then
//            > kHi: tripped; without a wrap the two comparisons are u >= kLo - D and u <= kHi + D;
//   root(x): x in [2^-96, FLT_MAX]  <=> u in [31 << 23, 0x7f7fffff].  mn takes u + (56 << 23) (>= kLo iff
//            u >= 31 << 23; a wrap needs the sign bit and gives < kLo: tripped), mx takes the saturating
//            u - (0x7f7fffff - kHi) (<= kHi iff u <= 0x7f7fffff: -0, negative values, inf and NaN trip).
struct RangeGate {
    static constexpr uint32_t kLo = 0x2b800000u, kHi = 0x53800000u;   // bits of 2^-40 and 2^40
    uint32_t mn = kHi, mx = kLo;
    // Several division operands at once: lo = the smallest, hi = the largest of their magnitudes, taken
    // with fminf / fmaxf of fabsf (v_min3_f32 / v_max3_f32 with |x| source modifiers: no v_and).  Those
    // skip a NaN operand, so the caller shows that none of the operands is one, or trips the gate itself.
    __device__ __forceinline__ void div_lo(float lo) { mn = min(mn, __float_as_uint(lo)); }
    __device__ __forceinline__ void div_hi(float hi) { mx = max(mx, __float_as_uint(hi)); }
    __device__ __forceinline__ void norm(float x) {
        const uint32_t u = __float_as_uint(x);
        mn = min(mn, u + (40u << 23));
        mx = max(mx, u - (40u << 23));
    }
    __device__ __forceinline__ void root(float x) {
        const uint32_t u = __float_as_uint(x);
        mn = min(mn, u + (56u << 23));
        mx = max(mx, __builtin_elementwise_sub_sat(u, 0x7f7fffffu - kHi));
    }
    // unit(x): unit_ok(x) <=> w = bits(x) - bits(1 - 2^-12) <= kUnitSpan (unsigned: a smaller x wraps to a
    // large w).  mx takes the saturating w + (kHi - kUnitSpan): <= kHi iff w <= kUnitSpan, and no wrap.
    __device__ __forceinline__ void unit(float x) {
        const uint32_t w = __float_as_uint(x) - (kUnitBits - kUnitBelow);
        mx = max(mx, __builtin_elementwise_add_sat(w, kHi - kUnitSpan));
    }
    __device__ __forceinline__ bool ok() const { return mn >= kLo && mx <= kHi; }
};
__device__ __forceinline__ float gmin(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float gmax(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float at(f3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }

// Scene tables that every lane of a wave reads at the same address are accessed through the
// constant address space so hipcc emits scalar (s_load) reads into SGPRs instead of 64 copies.
#define PT_CONST_AS __attribute__((address_space(4)))
template <class T>
__device__ __forceinline__ const T PT_CONST_AS* as_const(const T* p) {
    return (const T PT_CONST_AS*)(p);
}
template <class M>
__device__ __forceinline__ f3 xform_point(const M& m, f3 v) {
    return F3((m.c[0][0] * v.x + m.c[1][0] * v.y) + (m.c[2][0] * v.z + m.c[3][0]),
              (m.c[0][1] * v.x + m.c[1][1] * v.y) + (m.c[2][1] * v.z + m.c[3][1]),
              (m.c[0][2] * v.x + m.c[1][2] * v.y) + (m.c[2][2] * v.z + m.c[3][2]));
}
template <class M>
__device__ __forceinline__ f3 xform_vector(const M& m, f3 v) {
    return F3((m.c[0][0] * v.x + m.c[1][0] * v.y) + (m.c[2][0] * v.z + m.z3[0]),
              (m.c[0][1] * v.x + m.c[1][1] * v.y) + (m.c[2][1] * v.z + m.z3[1]),
              (m.c[0][2] * v.x + m.c[1][2] * v.y) + (m.c[2][2] * v.z + m.z3[2]));
}

// ---- RNG: thrust::default_random_engine (minstd_rand) seeded like makeSeededRandomEngine ----
__device__ __forceinline__ uint32_t utilhash(uint32_t a) {   // intersections.h:13-22
    a = (a + 0x7ed55d16u) + (a << 12);
    a = (a ^ 0xc761c23cu) ^ (a >> 19);
    a = (a + 0x165667b1u) + (a << 5);
    a = (a + 0xd3a2646cu) ^ (a << 9);
    a = (a + 0xfd7046c5u) + (a << 3);
    a = (a ^ 0xb55a4f09u) ^ (a >> 16);
    return a;
}
struct Rng {
    uint32_t x;
    __device__ __forceinline__ Rng(int iter, int index, int depth) {
        const uint32_t key = 0x80000000u | ((uint32_t)depth << 22) | (uint32_t)iter;
        const uint32_t h = utilhash(key) ^ utilhash((uint32_t)index);
        const uint32_t s = h % 2147483647u;
        x = s == 0u ? 1u : s;
    }
    // x <- 48271 x mod (2^31 - 1) via the Mersenne fold (exact), u = float(x-1) / 2^31.
    __device__ __forceinline__ float u01() {
        const uint64_t p = (uint64_t)48271u * x;
        uint32_t r = (uint32_t)(p & 0x7fffffffu) + (uint32_t)(p >> 31);
        if (r >= 2147483647u) r -= 2147483647u;
        x = r;
        return (float)(x - 1u) * 4.656612873077392578125e-10f;   // / 2147483648.0f (exact)
    }
};

// ---- deterministic sin/cos (evaluation contract; mirrored by the oracle) --------------------
__device__ __forceinline__ void sincos_c(float x, float* s_out, float* c_out) {
    const float j = rintf(x * 0.636619772367581343f);
    float r = fmaf(-j, 1.5707962513e+00f, x);
    r = fmaf(-j, 7.5497894159e-08f, r);
    r = fmaf(-j, 5.3903029534e-15f, r);
    const float z = r * r;
    const float ps = fmaf(fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), z, -1.6666654611e-1f);
    const float s = fmaf(r * z, ps, r);
    const float pc = fmaf(fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
    const float c = fmaf(z * z, pc, fmaf(-0.5f, z, 1.0f));
    const int q = ((int)j) & 3;
    const float sa = (q & 1) ? c : s;
    const float ca = (q & 1) ? s : c;
    *s_out = (q & 2) ? -sa : sa;
    *c_out = ((q + 1) & 2) ? -ca : ca;
}

// getPointOnRay (intersections.h:29-32)
__device__ __forceinline__ f3 point_on_ray(f3 o, f3 d, float t) { return o + (t - .0001f) * normalize(d); }
// point_on_ray for a direction that is a unit vector in all ordinary use (shade's path: a camera ray, a
// reflection, a hemisphere sample): the same bits for every d, normalize's own code behind one cold branch.
__device__ __forceinline__ f3 point_on_ray_unit(f3 o, f3 d, float t) {
    const float x = dot(d, d);
    float inv = unit_rnorm(x);
    if (__builtin_expect(!unit_ok(x), 0)) {
        const float s = sqrt_core(x);
        inv = div_core(1.0f, s, recip_core(s));
        if (__builtin_expect(!(x >= 0x1p-80f && x <= 0x1p+80f), 0)) inv = 1.0f / sqrtf(x);
    }
    return o + (t - .0001f) * (d * inv);
}

}  // namespace ptd
