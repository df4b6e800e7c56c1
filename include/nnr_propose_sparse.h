/*
 * nnr_propose_sparse.h -- the sparse proposal stage of hierarchical sampling: nnr_propose (nnr.h) that does not
 * evaluate the coarse samples an occupancy bitfield calls empty.  The same C ABI as nnr.h (plain device pointers and sizes, asynchronous on
 * `stream`, no global state, the error codes and nnr_cfg of nnr.h); declared here so that the lists of functions of nnr.h and nnr_sparse.h
 * stay what they are.  nnr/lib.py lists it in PROPOSE_SPARSE_EXPORTS.  It changes no signature, struct or blob layout: the version stays
 * nnr.h's.
 */
#ifndef NNR_PROPOSE_SPARSE_H
#define NNR_PROPOSE_SPARSE_H

#include "nnr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nnr_propose in ONE launch (nnr_propose_f16.hip compiled with NNR_PROPOSE_SPARSE=1), evaluating the density only on LIVE coarse samples.
 * Every argument it shares with nnr_propose means what it means there: the sampling (z_j, p_j), a sample's raw density and its alpha, the
 * row code of nnr_resample.  The grid arguments and the cell rule are those of nnr_sparse.h's render: f_c = (p_c - grid_lo[c]) *
 * grid_inv_step[c], every operation rounded to fp32 and none fused; inside iff 0 <= f_c < (float) n_c on all three axes (a NaN fails:
 * outside); i_c = (int) f_c; cell (i_x, i_y, i_z) is bit i_x & 31 of word (i_z n_y + i_y) w_x + (i_x >> 5), w_x = ceil(n_x / 32).  A sample
 * is LIVE iff it is outside the grid or its bit is set; otherwise it is CULLED.
 * The definition: with alpha_j the alpha nnr_propose gives sample j (the delta to the next sample of the ORIGINAL row, culled or not; 1e10
 * behind the last), alpha'_j = alpha_j where j is live and exactly 0 where j is culled -- whatever the flags, also for the closing sample
 * under NNR_F_DIST_ALPHA -- the output row is, bit for bit, what nnr_resample gives for (alpha', z).  Hence:
 *   with every bit set the outputs are nnr_propose's bit for bit;
 *   a ray whose samples are all culled gets the row nnr_resample makes from zeros, which is finite: the floor of its definition spreads
 *   the fine samples uniformly over the bins;
 *   a culled sample is NOT EVALUATED and so can never make its ray NaN (no out-of-range activation, no NaN density): the one intended
 *   difference from nnr_propose.  A live sample can, exactly as there; a sample whose point is not finite is outside the grid, hence live.
 * Notation: workgroup g holds the rays 4g .. 4g + 3, one per wave; a wave past the last ray repeats ray n_rays - 1.
 *   grid_lo, grid_inv_step, grid_dims      HOST arrays of three
 *   bits          (n_z, n_y, w_x) uint32 on the device
 *   z_all, opt_alpha, opt_z, opt_fine      nnr_propose's; opt_alpha holds alpha' (0 for a culled sample), opt_z every sample's depth
 *   opt_count     (n_rays) int32 or NULL: the ray's live samples n_r.
 *   opt_cell      (n_rays, n_samples) int32 or NULL: (i_z n_y + i_y) n_x + i_x of EVERY sample, -1 outside the grid.
 *   opt_passes    (n_rays) int32 or NULL: the passes of 32 samples the ray's workgroup ran, max over its rays of ceil(n_r / 32); 0 where
 *                 none of them has a live sample (such a workgroup reads no weight).
 * Return codes, all decided before any device work (the outputs are untouched): the union of nnr_propose's and the grid checks of
 * nnr_sparse.h.  NNR_E_BADCFG for a null cfg or pointer (other than jitter, xi and the opt_*), n_rays < 1, n_samples < 3, n_fine < 1, a dim
 * below 1, a grid_lo or grid_inv_step that is not finite or an inverse step that is not positive; then NNR_E_UNSUPPORTED for n_samples >
 * 256, n_samples + n_fine > 1024, a hidden width other than 128 / 256, NNR_F_TRAIN or NNR_F_BF16, missing split flags, more than 2^31 - 1
 * words or cells; then NNR_E_ALIGN for `packed` or `z_all` not 16-byte or another pointer not 4-byte aligned.  No host synchronisation, no
 * atomics: bit-reproducible. */
int nnr_propose_sparse(const nnr_cfg* cfg, int32_t n_fine, const float* pts_o, const float* pts_d, const float* z_lo, const float* z_hi,
                       const float* jitter, const float* xi, const float grid_lo[3], const float grid_inv_step[3],
                       const int32_t grid_dims[3], const uint32_t* bits, const float* packed, float* z_all, float* opt_alpha, float* opt_z,
                       float* opt_fine, int32_t* opt_count, int32_t* opt_cell, int32_t* opt_passes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNR_PROPOSE_SPARSE_H */
