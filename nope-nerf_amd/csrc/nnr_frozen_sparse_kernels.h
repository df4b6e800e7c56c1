// nnr_frozen_sparse_kernels.h -- the argument blocks and launchers of the sparse frozen-field render (include/nnr_frozen_sparse.h, DESIGN.md
// section 15): the compaction front end (nnr_frozen_sparse.hip) and the LIST-DRIVEN builds of the two frozen MLP kernels
// (nnr_mlp_fwd_f16.hip with NNR_FWD_TRAIN=3, nnr_mlp_dgrad_f16.hip with NNR_DGRAD_LIST=1).  The two kernels take the training kernels'
// argument blocks (nnr_kernels.h) with the live list behind them; the blocks of every other build stay what they are.
// A header of its own, as nnr_frozen_kernels.h is: nnr_kernels.h stays what every other unit was compiled against.
#pragma once
#include "nnr_frozen_kernels.h"

namespace nnr {

// slot s of the compacted order is the sample live[min(s, *n_live - 1)] (flat index ray * N + j, ascending); both on the device
struct MlpFwdListArgs : MlpFwdArgs {
    const int32_t* live;
    const int32_t* n_live;
};
struct MlpDgradListArgs : MlpDgradArgs {
    const int32_t* live;
    const int32_t* n_live;
};

// the list of an argument block, null for the blocks without one: the kernels' source names them in `if constexpr (LIST)` branches that every
// build parses
__host__ __device__ inline const int32_t* list_live(const MlpFwdListArgs& a) { return a.live; }
__host__ __device__ inline const int32_t* list_live(const MlpDgradListArgs& a) { return a.live; }
__host__ __device__ inline const int32_t* list_live(const MlpFwdArgs&) { return nullptr; }
__host__ __device__ inline const int32_t* list_live(const MlpDgradArgs&) { return nullptr; }
__host__ __device__ inline const int32_t* list_n_live(const MlpFwdListArgs& a) { return a.n_live; }
__host__ __device__ inline const int32_t* list_n_live(const MlpDgradListArgs& a) { return a.n_live; }
__host__ __device__ inline const int32_t* list_n_live(const MlpFwdArgs&) { return nullptr; }
__host__ __device__ inline const int32_t* list_n_live(const MlpDgradArgs&) { return nullptr; }

// the compaction front end: which samples are live, the substitutes of those that are not, the list
struct FrozenSparseArgs {
    const float *pts_o, *pts_d;            // (R,3)
    const float *z_lo, *z_hi;              // (N)
    const float* jitter;                   // (R,N) or null
    const uint32_t* bits;                  // the bitfield of include/nnr_sparse.h
    float* ws_out4;                        // (S_pad,4): culled rows get (0, 0, 0, E)
    float* ws_z;                           // (S_pad): every sample's z
    float* ws_dpts;                        // (S_pad,4): culled rows get zeros
    float* ws_dview;                       // (S_pad,4): culled rows get zeros
    uint32_t* ray_mask;                    // (R, kFrozenSparseMaskWords): bit j & 31 of word j >> 5: sample j of the ray is live
    int32_t* ray_count;                    // (R): the ray's live samples
    int32_t* ray_off;                      // (R): the ray's first place in `live`
    int32_t* live;                         // (S_pad)
    int32_t* n_live;                       // (1)
    int32_t* opt_count;                    // (R) or null: a copy of ray_count for the caller
    int32_t* opt_live;                     // (R N) or null: a copy of the list's n_live entries for the caller
    int32_t* opt_n_live;                   // (1) or null: a copy of n_live
    float lo[3], inv_step[3];
    int n[3];                              // (n_x, n_y, n_z) cells
    int wx;                                // ceil(n_x / 32)
    int R, N;
    uint32_t flags;                        // NNR_F_DIST_ALPHA: the last sample of every ray is live
};
constexpr int kFrozenSparseMaskWords = 32;      // N <= 1024

hipError_t launch_frozen_sparse_compact(const FrozenSparseArgs& a, hipStream_t st);      // nnr_frozen_sparse.hip: three launches

template <int D> hipError_t launch_mlp_fwd_frozen_list_variant(const MlpFwdListArgs& a, hipStream_t st);       // one translation unit each (csrc/build.py)
template <int D> hipError_t launch_mlp_dgrad_frozen_list_variant(const MlpDgradListArgs& a, hipStream_t st);

}  // namespace nnr
