/*
 * nnr_depth_median.h -- the quantile (median) depth of a ray beside its expected depth: the dense depth render of
 * nnr_fusion.h and the sparse depth render of nnr_depth_sparse.h, each with a third output column.  What the depth fusion of the TSDF
 * export integrates under depth_mode 'median': a depth that always lies on a surface the ray really crosses, and that stopping the ray
 * does not move.  The same C ABI as nnr.h (plain device pointers and sizes, asynchronous on `stream`, no global state, the error codes
 * and nnr_cfg of nnr.h); declared here so that the lists of functions of the other headers stay what they are.  nnr/lib.py lists the two
 * in DEPTH_MEDIAN_EXPORTS.  They change no signature, struct or blob layout: the version stays nnr.h's.
 *
 * The definition, for both.  The row of evaluated samples of a ray, their alphas alpha_i and depths z_i are exactly the parent entry's
 * (every sample for the dense render; the evaluated list entries E_r for the sparse one).  Over the evaluated samples in order
 *   T_0 = 1,  T_{i+1} = T_i (1 - alpha_i + 1e-6)
 * in fp32, the products the parent kernel forms for its weights, in its order (dense: the lane's run from the wave scan's prefix; sparse:
 * the carry of the earlier passes times the pass's scan).  m = the first evaluated sample with T_{m+1} < level (fp32 <; a NaN never
 * crosses); z_next = the depth of sample m + 1 of the ORIGINAL row, culled or not -- the neighbour alpha_m's delta uses --, z_m behind the
 * last sample of the row.  Then
 *   q = z_m + (z_next - z_m) * ((T_m - level) / (T_m - T_{m+1}))
 * every operation rounded to fp32 in this order, none fused, one IEEE division: the inverse of the piecewise-constant weight histogram's
 * CDF at 1 - level, the model nnr_resample draws from.  level = 0.5: the median.
 *   no crossing, T finite          q = +inf
 *   no crossing, T NaN             q = NaN
 *   dense, a ray that is (NaN, NaN) in the parent: all three columns NaN
 *   sparse, a ray that crossed before its first NaN alpha keeps its q; columns 0 and 1 are NaN as in the parent
 * Exact under the stop: once T < level nothing behind can change m or q, so the sparse entry gives the same q, bit for bit, at every
 * t_min <= level as at t_min = 0 -- which is why it refuses t_min > level.
 */
#ifndef NNR_DEPTH_MEDIAN_H
#define NNR_DEPTH_MEDIAN_H

#include "nnr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The dense depth render (nnr_fusion.h) with q beside, in ONE launch (nnr_depth_f16.hip compiled with NNR_DEPTH_MEDIAN=1).  Arguments,
 * checks and return codes are that entry's, in its precedence, and
 *   level         0 < level < 1 and finite, otherwise NNR_E_BADCFG (with the sizes and the null pointers, before NNR_E_UNSUPPORTED)
 *   out           (n_rays, 3) fp32: (depth, acc, q) per ray; columns 0 and 1 are that entry's bit for bit.
 * No host synchronisation, no atomics: bit-reproducible. */
int nnr_render_depth_median(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* z_lo, const float* z_hi,
                            const float* jitter, float level, const float* packed, float* out, float* opt_raw, float* opt_z, void* stream);

/* The sparse depth render (nnr_depth_sparse.h) with q beside, in ONE launch (nnr_propose_f16.hip compiled with NNR_PROPOSE_SPARSE=1
 * NNR_PROPOSE_DEPTH=2).  Arguments, checks and return codes are that entry's, in its precedence, and
 *   level         0 < level < 1 and finite, otherwise NNR_E_BADCFG
 *   t_min         0 <= t_min <= level, otherwise NNR_E_BADCFG: stopped above the level, q would not be the unstopped one
 *   out           (n_rays, 3) fp32: depth, acc, q; columns 0 and 1, opt_raw, opt_count, opt_cell and opt_passes are that entry's bit for
 *                 bit at the same t_min.  A ray without a live sample gets (0, 0, +inf).
 * The stop rule, and with it opt_passes, does not look at level.  No host synchronisation, no atomics: bit-reproducible. */
int nnr_render_depth_median_sparse(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* z_lo, const float* z_hi,
                                   const float* jitter, const float grid_lo[3], const float grid_inv_step[3], const int32_t grid_dims[3],
                                   const uint32_t* bits, float t_min, float level, const float* packed, float* out,
                                   float* opt_raw, int32_t* opt_count, int32_t* opt_cell, int32_t* opt_passes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNR_DEPTH_MEDIAN_H */
