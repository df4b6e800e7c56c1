// nnr_frozen_kernels.h -- the launchers of the frozen-field render (include/nnr_frozen.h): the two-term forward and
// input-gradient kernels built WITHOUT their activation and gradient stashes (nnr_mlp_fwd_f16.hip with NNR_FWD_TRAIN=2, nnr_mlp_dgrad_f16.hip
// with NNR_DGRAD_STASH=0).  They take the training kernels' argument blocks (nnr_kernels.h); the planes the frozen workspace does not have --
// ws_xh, ws_xg, ws_dh, ws_dg, plane_max -- are null there, and no instruction of these builds stores through them.
// A header of its own, as nnr_fusion_kernels.h is: nnr_kernels.h stays what every other unit was compiled against.
#pragma once
#include "nnr_kernels.h"

namespace nnr {

template <int D> hipError_t launch_mlp_fwd_frozen_variant(const MlpFwdArgs& a, hipStream_t st);       // one translation unit each (csrc/build.py)
template <int D> hipError_t launch_mlp_dgrad_frozen_variant(const MlpDgradArgs& a, hipStream_t st);

// passes per ray in ray mode, 0 = the flat decomposition (nnr_api.cpp: the training kernels' rule, the same samples per chunk here)
int chunks_per_ray(const nnr_cfg* c);

// the one launch-result path of the library (nnr_api.cpp): a HIP result -> the entry point's return code, kept for nnr_last_hip_error
int launched(hipError_t e);

}  // namespace nnr
