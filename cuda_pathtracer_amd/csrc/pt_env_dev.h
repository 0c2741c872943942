// The environment lookup L(d) of the MI355X path tracer: one octahedral radiance map,
// bilinearly interpolated in its padded texel grid (EnvDev, pt_layout.h).  Shared by the bounce kernels
// (pt_kernels.hip: a path that leaves the scene ends with colour x L(direction)) and by pt_env_eval
// (pt_env.hip), which the tests hold to a numpy restatement bit for bit: only + - * /, fabs, floor and
// compares, each correctly rounded and never contracted (-ffp-contract=off), in the order written here.
#pragma once
#include "pt_device.h"

namespace ptd {

// d need not be normalised (the projection divides by the 1-norm).  A direction whose 1-norm is zero, NaN
// or infinite returns 0: glm::refract's NaN ray (k < 0) misses everything and must keep contributing 0.
__device__ __forceinline__ f3 env_lookup(const EnvDev& E, f3 d) {
    // 1. rotate into the map's frame, each row (a x + b y) + c z
    const float rx = (E.rot[0] * d.x + E.rot[1] * d.y) + E.rot[2] * d.z;
    const float ry = (E.rot[3] * d.x + E.rot[4] * d.y) + E.rot[5] * d.z;
    const float rz = (E.rot[6] * d.x + E.rot[7] * d.y) + E.rot[8] * d.z;
    // 2, 3. the 1-norm and its guard
    const float s = (fabsf(rx) + fabsf(ry)) + fabsf(rz);
    if (!(s > 0.0f) || !(s < __builtin_inff())) return F3(0.0f, 0.0f, 0.0f);
    // 4. project onto the octahedron, 5. fold the lower half over the square's edges (sgn(0) = +1)
    float px = rx / s, pz = rz / s;
    if (ry < 0.0f) {
        const float qx = (1.0f - fabsf(pz)) * (px >= 0.0f ? 1.0f : -1.0f);
        const float qz = (1.0f - fabsf(px)) * (pz >= 0.0f ? 1.0f : -1.0f);
        px = qx;
        pz = qz;
    }
    // 6. padded texel coordinates: + 1 for the gutter, - 0.5 for the texel centre
    const float nf = (float)E.n;
    const float fx = (px * 0.5f + 0.5f) * nf + 0.5f;
    const float fz = (pz * 0.5f + 0.5f) * nf + 0.5f;
    int ix = (int)floorf(fx), iz = (int)floorf(fz);
    ix = ix < 0 ? 0 : (ix > E.n ? E.n : ix);   // ([0, n]: the four texels stay inside the (n + 2)^2 map)
    iz = iz < 0 ? 0 : (iz > E.n ? E.n : iz);
    const float wx = fx - (float)ix, wz = fz - (float)iz;
    // 7. four 16-byte loads, x then z, then the scale
    const v4f* row = E.map + (size_t)iz * (size_t)(E.n + 2) + (size_t)ix;
    const v4f a = row[0], b = row[1], c = row[E.n + 2], e = row[E.n + 3];
    const float t0 = a[0] + (b[0] - a[0]) * wx, u0 = c[0] + (e[0] - c[0]) * wx;
    const float t1 = a[1] + (b[1] - a[1]) * wx, u1 = c[1] + (e[1] - c[1]) * wx;
    const float t2 = a[2] + (b[2] - a[2]) * wx, u2 = c[2] + (e[2] - c[2]) * wx;
    return F3((t0 + (u0 - t0) * wz) * E.scale, (t1 + (u1 - t1) * wz) * E.scale, (t2 + (u2 - t2) * wz) * E.scale);
}

}  // namespace ptd
