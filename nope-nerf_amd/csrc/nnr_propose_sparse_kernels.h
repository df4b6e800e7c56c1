// nnr_propose_sparse_kernels.h -- the argument block and launcher of the sparse proposal (include/nnr_propose_sparse.h; DESIGN.md section
// 12.2): propose_sparse_f16_kernel (nnr_propose_f16.hip under NNR_PROPOSE_SPARSE=1) and what its host entry (in nnr_sparse_api.cpp) needs of
// nnr_api.cpp.  Self-contained: no layout, no other kernel's block.  Included by those two units alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nnr {

// the fused proposal (ProposeArgs, nnr_kernels.h) behind the compaction prologue of the sparse render: the fields of both, by their names there
struct ProposeSparseArgs {
    const float *pts_o, *pts_d;   // (R,3)
    const float *z_lo, *z_hi;     // (C)
    const float* jitter;          // (R,C) or null
    const float* xi;              // (R,F) or null
    const uint32_t* bits;         // (n_z, n_y, w_x) words; bit i_x & 31 of word (i_z n_y + i_y) w_x + (i_x >> 5): the cell may hold matter
    const float* packed;          // Layout<D, 3> (NNR_F_SPLIT3 | NNR_F_SPLIT2)
    float* z_all;                 // (R,C+F)
    float *opt_alpha, *opt_z, *opt_fine;   // (R,C), (R,C), (R,F) or null
    int32_t* opt_count;           // (R) or null: the ray's live samples
    int32_t* opt_cell;            // (R,C) or null: the cell of every sample, -1 outside the grid
    int32_t* opt_passes;          // (R) or null: the passes the ray's workgroup ran
    float lo[3], inv_step[3];
    int n[3];                     // (n_x, n_y, n_z) cells
    int wx;                       // ceil(n_x / 32)
    int R, C, F;
    uint32_t flags;               // NNR_F_RELU_SIGMA / NNR_F_DIST_ALPHA
};

hipError_t launch_propose_sparse(int D, const ProposeSparseArgs& a, hipStream_t st);      // nnr_propose_f16.hip under NNR_PROPOSE_SPARSE=1

// nnr_api.cpp: what a launcher returned -> the entry point's return code (NNR_E_HIP, the HIP error kept for nnr_last_hip_error)
int launched(hipError_t e);

}  // namespace nnr
