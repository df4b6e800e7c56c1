// nnr_fusion_kernels.h -- the argument blocks and launchers of the depth-fusion side of the geometry export (include/nnr_fusion.h; DESIGN.md
// section 11.2): depth_f16_kernel (nnr_depth_f16.hip) and tsdf_integrate_kernel (nnr_tsdf.hip), and what their host unit (nnr_fusion_api.cpp)
// needs of nnr_api.cpp.  Included by those three units alone: touching it rebuilds nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nnr {

// the rendered depth of a ray from the density alone (nnr_depth_f16.hip): the proposal kernel's passes, a compositing epilogue
struct DepthArgs {
    const float *pts_o, *pts_d;   // (R,3)
    const float *z_lo, *z_hi;     // (C)
    const float* jitter;          // (R,C) or null
    const float* packed;          // Layout<D, 3> (NNR_F_SPLIT3 | NNR_F_SPLIT2)
    float* out;                   // (R,2): (depth, acc)
    float *opt_raw, *opt_z;       // (R,C), (R,C) or null
    int R, C;
    uint32_t flags;               // NNR_F_RELU_SIGMA / NNR_F_DIST_ALPHA
};

// the same render with the quantile depth beside (nnr_depth_f16.hip under NNR_DEPTH_MEDIAN=1; include/nnr_depth_median.h)
struct DepthMedianArgs : DepthArgs {      // out: (R,3): (depth, acc, q)
    float level;                  // q: the depth at which the transmittance falls below this; 0 < level < 1
};

// the integration of depth maps into a truncated signed distance volume held in 8 x 8 x 8 bricks (nnr_tsdf.hip)
struct TsdfArgs {
    const int32_t* bricks;        // (B,3): (bx, by, bz)
    const float* cams;            // (n_cams,12): rows 0..2 of K . world_mat . scale_mat, row-major
    const float* depth;           // (n_cams,H,W) z-depth
    float *sum, *weight;          // (B,8,8,8) each, read and written
    float origin[3], step[3];
    float trunc, z_min;
    float cw, ch;                 // (W - 1) / 2, (H - 1) / 2, rounded on the host
    float col_max, row_max;       // (float)(W - 1), (float)(H - 1): exact, W and H are at most 2^24
    int n_cams, H, W;
    uint32_t V;                   // 512 B voxels
};
constexpr int kTsdfMaxExtent = 1 << 24;      // W, H: every pixel index is an exact fp32

hipError_t launch_render_depth(int D, const DepthArgs& a, hipStream_t st);      // nnr_depth_f16.hip
hipError_t launch_render_depth_median(int D, const DepthMedianArgs& a, hipStream_t st);      // nnr_depth_f16.hip under NNR_DEPTH_MEDIAN=1
hipError_t launch_tsdf_integrate(const TsdfArgs& a, hipStream_t st);            // nnr_tsdf.hip

// nnr_api.cpp: what a launcher returned -> the entry point's return code (NNR_E_HIP, the HIP error kept for nnr_last_hip_error)
int launched(hipError_t e);

}  // namespace nnr
