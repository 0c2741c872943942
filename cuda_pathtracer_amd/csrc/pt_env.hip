// pt_env_eval, gfx950: the environment lookup of the bounce kernels (pt_env_dev.h env_lookup)
// over a list of directions, so that the tests can hold it to their numpy restatement bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pt_ctx.h"
#include "pt_env_dev.h"

using namespace ptd;

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_env_eval(const EnvDev E, const float* __restrict__ dirs, float* __restrict__ rgb,
                                                     int64_t n) {
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
        const f3 L = env_lookup(E, F3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
        rgb[3 * i] = L.x;
        rgb[3 * i + 1] = L.y;
        rgb[3 * i + 2] = L.z;
    }
}

struct DevBuf {   // a device allocation freed on every exit
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

}  // namespace

extern "C" {

int pt_env_eval(const pt_scene* s, int64_t n, const float* d_dirs, float* d_rgb, void* stream) {
    if (!s || n < 0 || (n > 0 && (!d_dirs || !d_rgb))) return pt::fail(PT_ERR_ARG, "bad pt_env_eval arguments");
    const pt::EnvHost& H = reinterpret_cast<const pt::Scene*>(s)->env;
    if (H.n <= 0) return pt::fail(PT_ERR_ARG, "the scene has no environment (pt_scene_set_environment)");
    if (n == 0) return PT_OK;
    const size_t texels = (size_t)(H.n + 2) * (size_t)(H.n + 2);
    if (H.rgba.size() != 4 * texels) return pt::fail(PT_ERR_ARG, "environment map of the wrong size");
    const hipStream_t st = (hipStream_t)stream;
    DevBuf map;
    HIP_TRY(hipMalloc(&map.p, texels * sizeof(v4f)));
    HIP_TRY(hipMemcpyAsync(map.p, H.rgba.data(), texels * sizeof(v4f), hipMemcpyHostToDevice, st));
    EnvDev E{};
    E.map = static_cast<const v4f*>(map.p);
    E.n = H.n;
    E.scale = H.params.scale;
    for (int k = 0; k < 9; ++k) E.rot[k] = H.rot[k];
    const int grid = (int)std::min<int64_t>((n + kBlock - 1) / kBlock, 8192);
    hipLaunchKernelGGL(k_env_eval, dim3(grid), dim3(kBlock), 0, st, E, d_dirs, d_rgb, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the map is this call's own: freed on return)
    return PT_OK;
}

int pt_env_eval_host(const pt_scene* s, int64_t n, const float* dirs, float* rgb) {
    if (!s || n < 0 || (n > 0 && (!dirs || !rgb))) return pt::fail(PT_ERR_ARG, "bad pt_env_eval_host arguments");
    if (reinterpret_cast<const pt::Scene*>(s)->env.n <= 0)
        return pt::fail(PT_ERR_ARG, "the scene has no environment (pt_scene_set_environment)");
    if (n == 0) return PT_OK;
    DevBuf in, out;
    const size_t bytes = (size_t)n * 3 * sizeof(float);
    HIP_TRY(hipMalloc(&in.p, bytes));
    HIP_TRY(hipMalloc(&out.p, bytes));
    HIP_TRY(hipMemcpy(in.p, dirs, bytes, hipMemcpyHostToDevice));
    if (int rc = pt_env_eval(s, n, static_cast<const float*>(in.p), static_cast<float*>(out.p), nullptr)) return rc;
    HIP_TRY(hipMemcpy(rgb, out.p, bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // extern "C"
