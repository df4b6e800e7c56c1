// nnr_cell_rule.h -- the cell rule of include/nnr_sparse.h, once: shared by the sparse inference render (nnr_sparse_f16.hip) and the
// compaction front end of the sparse frozen-field render (nnr_frozen_sparse.hip), both through nnr_sparse_cell.h, and by the sparse proposal
// (nnr_propose_f16.hip under NNR_PROPOSE_SPARSE=1), which includes this file itself.  `A`: an argument block with the grid's lo[3],
// inv_step[3], n[3] and wx (SparseArgs, FrozenSparseArgs, ProposeSparseArgs).
#pragma once
#include <hip/hip_runtime.h>

namespace nnr {

// the cell of a point: (i_z n_y + i_y) n_x + i_x, or -1 outside the grid; `word`, `bit`: its place in the bitfield
template <class A>
__device__ __forceinline__ int sparse_cell(const A& a, float px, float py, float pz, int& word, int& bit) {
    const float fx = __fmul_rn(__fsub_rn(px, a.lo[0]), a.inv_step[0]);
    const float fy = __fmul_rn(__fsub_rn(py, a.lo[1]), a.inv_step[1]);
    const float fz = __fmul_rn(__fsub_rn(pz, a.lo[2]), a.inv_step[2]);
    const bool inside = fx >= 0.f && fx < (float)a.n[0] && fy >= 0.f && fy < (float)a.n[1] && fz >= 0.f && fz < (float)a.n[2];
    word = 0;
    bit = 0;
    if (!inside) return -1;
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    const int row = iz * a.n[1] + iy;
    word = row * a.wx + (ix >> 5);
    bit = ix & 31;
    return row * a.n[0] + ix;
}

}  // namespace nnr
