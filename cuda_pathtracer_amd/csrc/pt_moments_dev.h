// Device pieces shared by the units that keep luminance moments of batch means (pt_denoise.hip's
// pt_moments, pt_adaptive.hip's pt_adaptive): DESIGN.md §10's albedo (de)modulation, §11's lum and
// the moments update of one pixel.  Same contract as those units: -ffp-contract=off, every operation
// one correctly rounded fp32 operation in the stated order.
#pragma once
#include "pt_device.h"

namespace ptd {

constexpr float kAlbMin = 0x1p-10f;               // albedo components below are not (de)modulated

__device__ __forceinline__ f3 dn_modulate(f3 c, v4f a, bool divide) {
    if (a[0] >= kAlbMin) c.x = divide ? div_cr(c.x, a[0]) : c.x * a[0];
    if (a[1] >= kAlbMin) c.y = divide ? div_cr(c.y, a[1]) : c.y * a[1];
    if (a[2] >= kAlbMin) c.z = divide ? div_cr(c.z, a[2]) : c.z * a[2];
    return c;
}

__device__ __forceinline__ float lum(f3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// pm = (prev.rgb, m1) of the pixel, m2 its second sum; (r, g, b) its accumulator after the batch
__device__ __forceinline__ void mom_pixel(float r, float g, float b, v4f& pm, float& m2, float bs, bool use_alb, v4f alb) {
    f3 d = F3(div_cr(r - pm[0], bs), div_cr(g - pm[1], bs), div_cr(b - pm[2], bs));
    if (use_alb) d = dn_modulate(d, alb, true);
    const float l = lum(d);
    pm = v4f{r, g, b, pm[3] + l};
    m2 = m2 + l * l;
}

}  // namespace ptd
