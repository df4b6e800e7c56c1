// nnr_grid_check.h -- the checks of an occupancy grid's three host arrays (include/nnr_sparse.h), shared by the host units whose entry points
// take one: nnr_sparse_api.cpp and nnr_frozen_api.cpp.  Host only, no state.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/nnr.h"

namespace nnr {

// NNR_E_BADCFG: a dim below 1, a non-finite lo or inv_step, an inv_step that is not positive.  NNR_E_UNSUPPORTED: more than 2^31 - 1 rows
// (n_z n_y), words or cells -- the kernels index them in int32.  NNR_OK: *wx = ceil(n_x / 32).  The three arrays are not null (the callers
// check that with their other pointers).  A caller that has refusals of its own between the two kinds tests the code for NNR_E_BADCFG
// first and for NNR_OK later: nnr_sparse_api.cpp.
inline int check_grid(const float lo[3], const float inv_step[3], const int32_t dims[3], int64_t* wx) {
    for (int c = 0; c < 3; ++c) {
        if (dims[c] < 1) return NNR_E_BADCFG;
        if (!std::isfinite(lo[c]) || !std::isfinite(inv_step[c]) || !(inv_step[c] > 0.f)) return NNR_E_BADCFG;
    }
    *wx = ((int64_t)dims[0] + 31) / 32;
    const int64_t rows = (int64_t)dims[2] * dims[1];      // < 2^62
    if (rows > INT32_MAX || rows * *wx > INT32_MAX || rows * dims[0] > INT32_MAX) return NNR_E_UNSUPPORTED;
    return NNR_OK;
}

}  // namespace nnr
