// nnr_regularise_api.cpp -- the extern "C" entry points of include/nnr_regularise.h (the ray-distortion regulariser): argument checking and
// marshalling into the kernels' argument struct (nnr_regularise_kernels.h).  A host unit of its own, as nnr_sparse_api.cpp is.  Every error
// return is decided before any device work -- no pointer is dereferenced here -- and the calls are asynchronous on the caller's stream.
// No state: the last HIP error is nnr_api.cpp's (launched).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/nnr_regularise.h"
#include "nnr_regularise_kernels.h"

using namespace nnr;

namespace {

bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }      // n a power of two

// what both entry points check alike; NNR_OK where the launch may go ahead
int check_common(const nnr_cfg* cfg, const float* raw, int32_t raw_stride, const float* z, float s_near, float s_inv) {
    if (!cfg || !raw || !z) return NNR_E_BADCFG;
    if (cfg->n_rays < 1 || cfg->n_samples < 1 || raw_stride < 1) return NNR_E_BADCFG;
    if (!std::isfinite(s_near) || !std::isfinite(s_inv) || !(s_inv > 0.f)) return NNR_E_BADCFG;
    return NNR_OK;
}

RayDistortionArgs common_args(const nnr_cfg* cfg, const float* raw, int32_t raw_stride, const float* z, float s_near, float s_inv) {
    RayDistortionArgs a{};
    a.raw = raw; a.raw_stride = raw_stride; a.z = z; a.s_near = s_near; a.s_inv = s_inv;
    a.R = cfg->n_rays; a.N = cfg->n_samples;
    a.flags = cfg->flags & (NNR_F_RELU_SIGMA | NNR_F_DIST_ALPHA);
    return a;
}

}  // namespace

extern "C" {

int nnr_ray_distortion_fwd(const nnr_cfg* cfg, const float* raw, int32_t raw_stride, const float* z, float s_near, float s_inv,
                           float* loss, void* stream) {
    if (const int rc = check_common(cfg, raw, raw_stride, z, s_near, s_inv)) return rc;
    if (!loss) return NNR_E_BADCFG;
    if (cfg->n_samples > kMaxSamplesRayDistortion) return NNR_E_UNSUPPORTED;
    for (const void* p : {(const void*)raw, (const void*)z, (const void*)loss})
        if (!aligned(p, 4)) return NNR_E_ALIGN;
    RayDistortionArgs a = common_args(cfg, raw, raw_stride, z, s_near, s_inv);
    a.loss = loss;
    return launched(launch_ray_distortion_fwd(a, (hipStream_t)stream));
}

int nnr_ray_distortion_bwd(const nnr_cfg* cfg, const float* raw, int32_t raw_stride, const float* z, float s_near, float s_inv,
                           const float* g, float* d_raw, int32_t d_raw_stride, int32_t accumulate, void* stream) {
    if (const int rc = check_common(cfg, raw, raw_stride, z, s_near, s_inv)) return rc;
    if (!g || !d_raw || d_raw_stride < 1) return NNR_E_BADCFG;
    if (cfg->n_samples > kMaxSamplesRayDistortion) return NNR_E_UNSUPPORTED;
    for (const void* p : {(const void*)raw, (const void*)z, (const void*)g, (const void*)d_raw})
        if (!aligned(p, 4)) return NNR_E_ALIGN;
    RayDistortionArgs a = common_args(cfg, raw, raw_stride, z, s_near, s_inv);
    a.g = g; a.d_raw = d_raw; a.d_raw_stride = d_raw_stride; a.accumulate = accumulate != 0;
    return launched(launch_ray_distortion_bwd(a, (hipStream_t)stream));
}

}  // extern "C"
