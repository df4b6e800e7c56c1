// nnr_sparse_kernels.h -- the argument block and launcher of the sparse inference render (include/nnr_sparse.h):
// sparse_f16_kernel (nnr_sparse_f16.hip) and what its host unit (nnr_sparse_api.cpp) needs of nnr_api.cpp.  Included by those two units
// alone: touching it rebuilds nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nnr {

// a render that evaluates only the samples an occupancy bitfield does not call empty (nnr_sparse_f16.hip)
struct SparseArgs {
    const float *pts_o, *pts_d, *view_d;   // (R,3)
    const float *z_lo, *z_hi;              // (C)
    const float* jitter;                   // (R,C) or null
    const uint32_t* bits;                  // (n_z, n_y, w_x) words; bit i_x & 31 of word (i_z n_y + i_y) w_x + (i_x >> 5): the cell may hold matter
    const float* packed;                   // Layout<D, 3> (NNR_F_SPLIT3 | NNR_F_SPLIT2)
    float* out;                            // (R,5): r, g, b, sum w z, sum w
    int32_t* opt_count;                    // (R) or null
    int32_t* opt_cell;                     // (R,C) or null
    float* opt_out4;                       // (R,C,4) or null
    float lo[3], inv_step[3];
    int n[3];                              // (n_x, n_y, n_z) cells
    int wx;                                // ceil(n_x / 32)
    int R, C;
    uint32_t flags;                        // NNR_F_RELU_SIGMA / NNR_F_DIST_ALPHA / NNR_F_WHITE_BG
};

hipError_t launch_render_sparse(int D, const SparseArgs& a, hipStream_t st);      // nnr_sparse_f16.hip

// the stopping render (include/nnr_sparse_stop.h): SparseArgs and what the stop needs behind it, a block of its own
// so that sparse_f16_kernel's kernel arguments stay what they are
struct SparseStopArgs : SparseArgs {
    float t_min;                           // a wave is done once its transmittance carry is < t_min (fp32); 0 stops nothing
    int32_t* opt_passes;                   // (R) or null: the passes the ray's workgroup ran
};

hipError_t launch_render_sparse_stop(int D, const SparseStopArgs& a, hipStream_t st);      // nnr_sparse_f16.hip under NNR_SPARSE_STOP=1

// nnr_api.cpp: what a launcher returned -> the entry point's return code (NNR_E_HIP, the HIP error kept for nnr_last_hip_error)
int launched(hipError_t e);

}  // namespace nnr
