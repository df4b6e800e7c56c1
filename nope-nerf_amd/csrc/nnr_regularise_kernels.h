// nnr_regularise_kernels.h -- the argument block and launchers of the ray-distortion regulariser (include/nnr_regularise.h; DESIGN.md
// section 13): ray_distortion_fwd_kernel / ray_distortion_bwd_kernel (nnr_ray_distortion.hip) and what their host unit
// (nnr_regularise_api.cpp) needs of nnr_api.cpp.  Included by those two units alone: touching it rebuilds nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nnr {

constexpr int kMaxSamplesRayDistortion = 1024;      // nnr_composite_bwd's limit; 16 blocks of 64 samples, one carry per lane (the kernels)

struct RayDistortionArgs {
    const float* raw;        // sample j of ray r: raw[(r N + j) raw_stride]
    const float* z;          // (R,N)
    const float* g;          // (R): backward only
    float* loss;             // (R): forward only
    float* d_raw;            // d_raw[(r N + j) d_raw_stride]: backward only
    int raw_stride, d_raw_stride;
    int accumulate;
    float s_near, s_inv;
    int R, N;
    uint32_t flags;          // NNR_F_RELU_SIGMA / NNR_F_DIST_ALPHA
};

hipError_t launch_ray_distortion_fwd(const RayDistortionArgs& a, hipStream_t st);      // nnr_ray_distortion.hip
hipError_t launch_ray_distortion_bwd(const RayDistortionArgs& a, hipStream_t st);

// nnr_api.cpp: what a launcher returned -> the entry point's return code (NNR_E_HIP, the HIP error kept for nnr_last_hip_error)
int launched(hipError_t e);

}  // namespace nnr
