// nnr_depth_sparse_kernels.h -- the argument block and launcher of the sparse depth render (include/nnr_depth_sparse.h; DESIGN.md section
// 11.3): depth_sparse_f16_kernel (nnr_propose_f16.hip under NNR_PROPOSE_SPARSE=1 NNR_PROPOSE_DEPTH=1) and what its host entry (in
// nnr_sparse_api.cpp) needs of nnr_api.cpp.  Self-contained: no layout, no other kernel's block.  Included by those two units alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nnr {

// the depth render (DepthArgs, nnr_fusion_kernels.h) behind the compaction prologue and with the stop of the sparse render: the fields of
// both, by their names there
struct DepthSparseArgs {
    const float *pts_o, *pts_d;   // (R,3)
    const float *z_lo, *z_hi;     // (C)
    const float* jitter;          // (R,C) or null
    const uint32_t* bits;         // (n_z, n_y, w_x) words; bit i_x & 31 of word (i_z n_y + i_y) w_x + (i_x >> 5): the cell may hold matter
    const float* packed;          // Layout<D, 3> (NNR_F_SPLIT3 | NNR_F_SPLIT2)
    float* out;                   // (R,2): depth, acc
    float* opt_raw;               // (R,C) or null: the raw density of every EVALUATED sample; untouched elsewhere
    int32_t* opt_count;           // (R) or null: the ray's live samples
    int32_t* opt_cell;            // (R,C) or null: the cell of every sample, -1 outside the grid
    int32_t* opt_passes;          // (R) or null: the passes the ray's workgroup ran
    float lo[3], inv_step[3];
    int n[3];                     // (n_x, n_y, n_z) cells
    int wx;                       // ceil(n_x / 32)
    int R, C;
    float t_min;                  // a wave is done once its transmittance carry is below this; 0: never by transmittance
    uint32_t flags;               // NNR_F_RELU_SIGMA / NNR_F_DIST_ALPHA
};

// the same render with the quantile depth beside (nnr_propose_f16.hip under NNR_PROPOSE_DEPTH=2; include/nnr_depth_median.h)
struct DepthSparseMedianArgs : DepthSparseArgs {      // out: (R,3): depth, acc, q
    float level;                  // q: the depth at which the transmittance falls below this; 0 < level < 1, t_min <= level
};

hipError_t launch_render_depth_sparse(int D, const DepthSparseArgs& a, hipStream_t st);      // nnr_propose_f16.hip under NNR_PROPOSE_DEPTH=1
hipError_t launch_render_depth_sparse_median(int D, const DepthSparseMedianArgs& a, hipStream_t st);      // the same under NNR_PROPOSE_DEPTH=2

// nnr_api.cpp: what a launcher returned -> the entry point's return code (NNR_E_HIP, the HIP error kept for nnr_last_hip_error)
int launched(hipError_t e);

}  // namespace nnr
