// Host view of the closed form the kernels use to renormalise a unit vector (pt_layout.h
// unit_rnorm_bits, pt_device.h renorm_unit_core): the same constexpr lines, compiled as plain C++, behind
// a C entry point, so that the form can be checked against a correctly rounded 1.0f / sqrtf(x) over its
// whole range without a device (tests/test_renorm_unit_cpu.py).
#include <cstring>

#include "pt_internal.h"

using namespace ptd;

// out[i] = the bits of 1 / sqrt(x) for x = the float with bits[i], in_range[i] = 1, where x lies in
// [1 - 2^-12, 1 + 2^-12]; elsewhere in_range[i] = 0 (the kernels run the general normalize) and out[i] = 0.
extern "C" int pt_unit_rnorm_host(const uint32_t* bits, int64_t n, uint32_t* out, uint8_t* in_range) {
    if (!bits || !out || !in_range || n < 0) return pt::fail(PT_ERR_ARG, "pt_unit_rnorm_host: null argument");
    for (int64_t i = 0; i < n; ++i) {
        const bool ok = unit_ok_bits(bits[i]);
        in_range[i] = ok ? 1 : 0;
        out[i] = ok ? unit_rnorm_bits(bits[i]) : 0u;
    }
    return PT_OK;
}
