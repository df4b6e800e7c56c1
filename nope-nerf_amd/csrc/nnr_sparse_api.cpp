// nnr_sparse_api.cpp -- the extern "C" entry points of include/nnr_sparse.h (the sparse inference render) and include/nnr_sparse_stop.h (the same
// render, stopped per workgroup once its rays are opaque): argument checking, shared, and marshalling into the kernels' argument structs
// (nnr_sparse_kernels.h); of include/nnr_propose_sparse.h (the sparse proposal; nnr_propose_sparse_kernels.h) and of
// include/nnr_depth_sparse.h (the sparse depth render; nnr_depth_sparse_kernels.h) and the sparse entry of include/nnr_depth_median.h (that
// render with the quantile depth beside).  A host unit of its own, as nnr_fusion_api.cpp is.  Every error return is
// decided before any device work -- no pointer is dereferenced here except the host arrays of the grid -- and the call is asynchronous on
// the caller's stream.  No state: the last HIP error is nnr_api.cpp's (launched).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nnr_depth_median.h"
#include "../../include/nnr_depth_sparse.h"
#include "../../include/nnr_propose_sparse.h"
#include "../../include/nnr_sparse_stop.h"
#include "nnr_depth_sparse_kernels.h"
#include "nnr_grid_check.h"
#include "nnr_propose_sparse_kernels.h"
#include "nnr_sparse_kernels.h"

using namespace nnr;

namespace {

bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }      // n a power of two; null passes

// What both entries check and marshal: NNR_OK and `a` filled, or the refusal.  t_min: the stopping entry's (0 for the plain one); opt_passes: its
// extra output (null for the plain one).  The order is the precedence: bad value > unsupported > misaligned.
int check_and_fill(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo, const float* z_hi,
                   const float* jitter, const float grid_lo[3], const float grid_inv_step[3], const int32_t grid_dims[3], const uint32_t* bits,
                   const float* packed, float t_min, float* out, int32_t* opt_count, int32_t* opt_cell, float* opt_out4, int32_t* opt_passes,
                   SparseArgs& a) {
    if (!cfg || cfg->n_rays < 1 || cfg->n_samples < 1) return NNR_E_BADCFG;
    if (!pts_o || !pts_d || !view_d || !z_lo || !z_hi || !grid_lo || !grid_inv_step || !grid_dims || !bits || !packed || !out)
        return NNR_E_BADCFG;      // (jitter and the opt_* may be null)
    if (!(t_min >= 0.f && t_min < 1.f)) return NNR_E_BADCFG;      // (a NaN fails both comparisons)
    int64_t wx;
    const int grid_rc = check_grid(grid_lo, grid_inv_step, grid_dims, &wx);
    if (grid_rc == NNR_E_BADCFG) return grid_rc;      // (a bad grid is refused before an unsupported cfg, an unsupported grid behind it)
    if (cfg->n_samples > 256 || (cfg->hidden != 128 && cfg->hidden != 256)) return NNR_E_UNSUPPORTED;
    if ((cfg->flags & (NNR_F_BF16 | NNR_F_SPLIT3 | NNR_F_SPLIT2)) != (NNR_F_SPLIT3 | NNR_F_SPLIT2) || (cfg->flags & NNR_F_TRAIN)) return NNR_E_UNSUPPORTED;
    if (grid_rc != NNR_OK) return grid_rc;
    if (!aligned(packed, 16)) return NNR_E_ALIGN;
    for (const void* p : {(const void*)pts_o, (const void*)pts_d, (const void*)view_d, (const void*)z_lo, (const void*)z_hi, (const void*)jitter,
                          (const void*)bits, (const void*)out, (const void*)opt_count, (const void*)opt_cell, (const void*)opt_out4,
                          (const void*)opt_passes})
        if (!aligned(p, 4)) return NNR_E_ALIGN;
    a.pts_o = pts_o; a.pts_d = pts_d; a.view_d = view_d; a.z_lo = z_lo; a.z_hi = z_hi; a.jitter = jitter; a.bits = bits; a.packed = packed;
    a.out = out; a.opt_count = opt_count; a.opt_cell = opt_cell; a.opt_out4 = opt_out4;
    for (int c = 0; c < 3; ++c) { a.lo[c] = grid_lo[c]; a.inv_step[c] = grid_inv_step[c]; a.n[c] = grid_dims[c]; }
    a.wx = (int)wx;
    a.R = cfg->n_rays; a.C = cfg->n_samples;
    a.flags = cfg->flags & (NNR_F_RELU_SIGMA | NNR_F_DIST_ALPHA | NNR_F_WHITE_BG);
    return NNR_OK;
}

}  // namespace

extern "C" {

int nnr_render_sparse(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo, const float* z_hi,
                      const float* jitter, const float grid_lo[3], const float grid_inv_step[3], const int32_t grid_dims[3],
                      const uint32_t* bits, const float* packed, float* out, int32_t* opt_count, int32_t* opt_cell, float* opt_out4,
                      void* stream) {
    SparseArgs a{};
    const int rc = check_and_fill(cfg, pts_o, pts_d, view_d, z_lo, z_hi, jitter, grid_lo, grid_inv_step, grid_dims, bits, packed, 0.f, out, opt_count,
                                  opt_cell, opt_out4, nullptr, a);
    if (rc != NNR_OK) return rc;
    return launched(launch_render_sparse(cfg->hidden, a, (hipStream_t)stream));
}

int nnr_render_sparse_stop(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo, const float* z_hi,
                           const float* jitter, const float grid_lo[3], const float grid_inv_step[3], const int32_t grid_dims[3],
                           const uint32_t* bits, const float* packed, float t_min, float* out, int32_t* opt_count, int32_t* opt_cell,
                           float* opt_out4, int32_t* opt_passes, void* stream) {
    SparseStopArgs a{};
    const int rc = check_and_fill(cfg, pts_o, pts_d, view_d, z_lo, z_hi, jitter, grid_lo, grid_inv_step, grid_dims, bits, packed, t_min, out, opt_count,
                                  opt_cell, opt_out4, opt_passes, a);
    if (rc != NNR_OK) return rc;
    a.t_min = t_min;
    a.opt_passes = opt_passes;
    return launched(launch_render_sparse_stop(cfg->hidden, a, (hipStream_t)stream));      // always the stopping kernel, also for t_min = 0
}

// the sparse proposal (include/nnr_propose_sparse.h): nnr_propose's checks and this unit's grid checks, in this unit's precedence
int nnr_propose_sparse(const nnr_cfg* cfg, int32_t n_fine, const float* pts_o, const float* pts_d, const float* z_lo, const float* z_hi,
                       const float* jitter, const float* xi, const float grid_lo[3], const float grid_inv_step[3],
                       const int32_t grid_dims[3], const uint32_t* bits, const float* packed, float* z_all, float* opt_alpha, float* opt_z,
                       float* opt_fine, int32_t* opt_count, int32_t* opt_cell, int32_t* opt_passes, void* stream) {
    if (!cfg || cfg->n_rays < 1 || cfg->n_samples < 3 || n_fine < 1) return NNR_E_BADCFG;
    if (!pts_o || !pts_d || !z_lo || !z_hi || !grid_lo || !grid_inv_step || !grid_dims || !bits || !packed || !z_all)
        return NNR_E_BADCFG;      // (jitter, xi and the opt_* may be null)
    int64_t wx;
    const int grid_rc = check_grid(grid_lo, grid_inv_step, grid_dims, &wx);
    if (grid_rc == NNR_E_BADCFG) return grid_rc;
    if (cfg->n_samples > 256 || (int64_t)cfg->n_samples + n_fine > 1024 || (cfg->hidden != 128 && cfg->hidden != 256)) return NNR_E_UNSUPPORTED;
    if ((cfg->flags & (NNR_F_BF16 | NNR_F_SPLIT3 | NNR_F_SPLIT2)) != (NNR_F_SPLIT3 | NNR_F_SPLIT2) || (cfg->flags & NNR_F_TRAIN)) return NNR_E_UNSUPPORTED;
    if (grid_rc != NNR_OK) return grid_rc;
    if (!aligned(packed, 16) || !aligned(z_all, 16)) return NNR_E_ALIGN;
    for (const void* p : {(const void*)pts_o, (const void*)pts_d, (const void*)z_lo, (const void*)z_hi, (const void*)jitter, (const void*)xi,
                          (const void*)bits, (const void*)opt_alpha, (const void*)opt_z, (const void*)opt_fine, (const void*)opt_count,
                          (const void*)opt_cell, (const void*)opt_passes})
        if (!aligned(p, 4)) return NNR_E_ALIGN;
    ProposeSparseArgs a{};
    a.pts_o = pts_o; a.pts_d = pts_d; a.z_lo = z_lo; a.z_hi = z_hi; a.jitter = jitter; a.xi = xi; a.bits = bits; a.packed = packed;
    a.z_all = z_all; a.opt_alpha = opt_alpha; a.opt_z = opt_z; a.opt_fine = opt_fine;
    a.opt_count = opt_count; a.opt_cell = opt_cell; a.opt_passes = opt_passes;
    for (int c = 0; c < 3; ++c) { a.lo[c] = grid_lo[c]; a.inv_step[c] = grid_inv_step[c]; a.n[c] = grid_dims[c]; }
    a.wx = (int)wx;
    a.R = cfg->n_rays; a.C = cfg->n_samples; a.F = n_fine;
    a.flags = cfg->flags & (NNR_F_RELU_SIGMA | NNR_F_DIST_ALPHA);
    return launched(launch_propose_sparse(cfg->hidden, a, (hipStream_t)stream));
}

// the sparse depth render (include/nnr_depth_sparse.h): nnr_render_depth's checks, the stopping render's for the grid and t_min, in this
// unit's precedence
int nnr_render_depth_sparse(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* z_lo, const float* z_hi,
                            const float* jitter, const float grid_lo[3], const float grid_inv_step[3], const int32_t grid_dims[3],
                            const uint32_t* bits, float t_min, const float* packed, float* out, float* opt_raw, int32_t* opt_count,
                            int32_t* opt_cell, int32_t* opt_passes, void* stream) {
    if (!cfg || cfg->n_rays < 1 || cfg->n_samples < 1) return NNR_E_BADCFG;
    if (!pts_o || !pts_d || !z_lo || !z_hi || !grid_lo || !grid_inv_step || !grid_dims || !bits || !packed || !out)
        return NNR_E_BADCFG;      // (jitter and the opt_* may be null)
    if (!(t_min >= 0.f && t_min < 1.f)) return NNR_E_BADCFG;      // (a NaN fails both comparisons)
    int64_t wx;
    const int grid_rc = check_grid(grid_lo, grid_inv_step, grid_dims, &wx);
    if (grid_rc == NNR_E_BADCFG) return grid_rc;
    if (cfg->n_samples > 256 || (cfg->hidden != 128 && cfg->hidden != 256)) return NNR_E_UNSUPPORTED;
    if ((cfg->flags & (NNR_F_BF16 | NNR_F_SPLIT3 | NNR_F_SPLIT2)) != (NNR_F_SPLIT3 | NNR_F_SPLIT2) || (cfg->flags & NNR_F_TRAIN)) return NNR_E_UNSUPPORTED;
    if (grid_rc != NNR_OK) return grid_rc;
    if (!aligned(packed, 16)) return NNR_E_ALIGN;
    for (const void* p : {(const void*)pts_o, (const void*)pts_d, (const void*)z_lo, (const void*)z_hi, (const void*)jitter, (const void*)bits,
                          (const void*)out, (const void*)opt_raw, (const void*)opt_count, (const void*)opt_cell, (const void*)opt_passes})
        if (!aligned(p, 4)) return NNR_E_ALIGN;
    DepthSparseArgs a{};
    a.pts_o = pts_o; a.pts_d = pts_d; a.z_lo = z_lo; a.z_hi = z_hi; a.jitter = jitter; a.bits = bits; a.packed = packed;
    a.out = out; a.opt_raw = opt_raw; a.opt_count = opt_count; a.opt_cell = opt_cell; a.opt_passes = opt_passes;
    for (int c = 0; c < 3; ++c) { a.lo[c] = grid_lo[c]; a.inv_step[c] = grid_inv_step[c]; a.n[c] = grid_dims[c]; }
    a.wx = (int)wx;
    a.R = cfg->n_rays; a.C = cfg->n_samples;
    a.t_min = t_min;
    a.flags = cfg->flags & (NNR_F_RELU_SIGMA | NNR_F_DIST_ALPHA);
    return launched(launch_render_depth_sparse(cfg->hidden, a, (hipStream_t)stream));
}

// the sparse depth render with the quantile depth (include/nnr_depth_median.h): nnr_render_depth_sparse's checks in their order; `level`
// and t_min > level (the quantile would not be the unstopped one) are refused with the other bad values
int nnr_render_depth_median_sparse(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* z_lo, const float* z_hi,
                                   const float* jitter, const float grid_lo[3], const float grid_inv_step[3], const int32_t grid_dims[3],
                                   const uint32_t* bits, float t_min, float level, const float* packed, float* out, float* opt_raw,
                                   int32_t* opt_count, int32_t* opt_cell, int32_t* opt_passes, void* stream) {
    if (!cfg || cfg->n_rays < 1 || cfg->n_samples < 1) return NNR_E_BADCFG;
    if (!pts_o || !pts_d || !z_lo || !z_hi || !grid_lo || !grid_inv_step || !grid_dims || !bits || !packed || !out)
        return NNR_E_BADCFG;      // (jitter and the opt_* may be null)
    if (!(t_min >= 0.f && t_min < 1.f)) return NNR_E_BADCFG;      // (a NaN fails both comparisons)
    if (!(level > 0.f && level < 1.f) || t_min > level) return NNR_E_BADCFG;
    int64_t wx;
    const int grid_rc = check_grid(grid_lo, grid_inv_step, grid_dims, &wx);
    if (grid_rc == NNR_E_BADCFG) return grid_rc;
    if (cfg->n_samples > 256 || (cfg->hidden != 128 && cfg->hidden != 256)) return NNR_E_UNSUPPORTED;
    if ((cfg->flags & (NNR_F_BF16 | NNR_F_SPLIT3 | NNR_F_SPLIT2)) != (NNR_F_SPLIT3 | NNR_F_SPLIT2) || (cfg->flags & NNR_F_TRAIN)) return NNR_E_UNSUPPORTED;
    if (grid_rc != NNR_OK) return grid_rc;
    if (!aligned(packed, 16)) return NNR_E_ALIGN;
    for (const void* p : {(const void*)pts_o, (const void*)pts_d, (const void*)z_lo, (const void*)z_hi, (const void*)jitter, (const void*)bits,
                          (const void*)out, (const void*)opt_raw, (const void*)opt_count, (const void*)opt_cell, (const void*)opt_passes})
        if (!aligned(p, 4)) return NNR_E_ALIGN;
    DepthSparseMedianArgs a{};
    a.pts_o = pts_o; a.pts_d = pts_d; a.z_lo = z_lo; a.z_hi = z_hi; a.jitter = jitter; a.bits = bits; a.packed = packed;
    a.out = out; a.opt_raw = opt_raw; a.opt_count = opt_count; a.opt_cell = opt_cell; a.opt_passes = opt_passes;
    for (int c = 0; c < 3; ++c) { a.lo[c] = grid_lo[c]; a.inv_step[c] = grid_inv_step[c]; a.n[c] = grid_dims[c]; }
    a.wx = (int)wx;
    a.R = cfg->n_rays; a.C = cfg->n_samples;
    a.t_min = t_min;
    a.flags = cfg->flags & (NNR_F_RELU_SIGMA | NNR_F_DIST_ALPHA);
    a.level = level;
    return launched(launch_render_depth_sparse_median(cfg->hidden, a, (hipStream_t)stream));
}

}  // extern "C"
