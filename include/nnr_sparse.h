/*
 * nnr_sparse.h -- the sparse inference render of libnnr.so: a forward-only render that does not evaluate the samples an
 * occupancy bitfield calls empty.  The same C ABI as nnr.h (plain device pointers and sizes, asynchronous on `stream`, no global state, the
 * error codes and nnr_cfg of nnr.h); declared here, as nnr_geometry.h and nnr_fusion.h declare their own, so that nnr.h's list of functions
 * stays what it is.  nnr/lib.py lists it in SPARSE_EXPORTS.  It changes no signature, struct or blob layout: the version stays nnr.h's.
 */
#ifndef NNR_SPARSE_H
#define NNR_SPARSE_H

#include "nnr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Render n_rays rays in ONE launch (nnr_sparse_f16.hip), evaluating the MLP only on LIVE samples.
 * Sampling is nnr_render_fwd's: sample j of ray r sits at z = z_lo[j] + (z_hi[j] - z_lo[j]) jitter[r][j] (z_lo[j] where jitter is NULL),
 * p = pts_o[r] + pts_d[r] z: nnr_render_fwd's depths and points, bit for bit.
 * The grid: n_c = grid_dims[c] cells on axis c (x, y, z), cell i_c spans [grid_lo[c] + i_c / grid_inv_step[c], + 1 / grid_inv_step[c]).
 * Cell lookup, every operation rounded to fp32 and none fused:
 *   f_c = (p_c - grid_lo[c]) * grid_inv_step[c];  the sample is INSIDE iff 0 <= f_c < (float) n_c on all three axes (a NaN fails: outside);
 *   i_c = (int) f_c.
 * The bitfield: uint32 words, cell (i_x, i_y, i_z) is bit i_x & 31 of word (i_z n_y + i_y) w_x + (i_x >> 5), w_x = ceil(n_x / 32);
 * n_z n_y w_x words.  A set bit: the cell may hold matter.  A clear bit: the cell is known to be empty.
 * A sample is LIVE iff it is outside the grid or its bit is set: a sample the grid knows nothing about is always evaluated.
 * A live sample's (r, g, b, raw) is, bit for bit, what nnr_mlp_fwd writes for (p, view_d[r]) under NNR_F_SPLIT3 | NNR_F_SPLIT2, incl. the
 * NaN of a sample where an activation left fp16's range; a sample whose point is not finite (outside the grid, hence live) is NaN, as in
 * nnr_render_depth.  Compositing, in fp32 and a fixed order, over the live samples j_0 < j_1 < ...:
 *   alpha_j = the compositor's alpha of (raw_j, z_{j+1} - z_j) under NNR_F_DIST_ALPHA / NNR_F_RELU_SIGMA, z_{j+1} the NEXT SAMPLE OF THE
 *             ORIGINAL LIST, culled or not (the last delta is 1e10): a live sample's alpha is its alpha in the dense render;
 *   T_k = prod_{i<k} (1 - alpha_{j_i} + 1e-6),  w_k = alpha_{j_k} T_k: a culled sample is absent from the product;
 *   rgb = sum w_k rgb_k (+ 1 - sum w_k under NNR_F_WHITE_BG),  sum w_k z_k,  sum w_k.
 * With every bit set and n_rays a multiple of 4, n_samples of 32, (r, g, b, sum w z) are nnr_render_fwd's fused inference outputs bit for bit.
 *   pts_o, pts_d, view_d  (n_rays, 3)      z_lo, z_hi  (n_samples)      jitter  (n_rays, n_samples) or NULL
 *   grid_lo, grid_inv_step, grid_dims      HOST arrays of three
 *   bits          (n_z, n_y, w_x) uint32 on the device
 *   packed        the NNR_F_SPLIT3 | NNR_F_SPLIT2 buffer of nnr_pack_weights
 *   out           (n_rays, 5) fp32: r, g, b, sum w z, sum w.  A ray is NaN iff one of its live samples is; no other ray is affected.  A ray
 *                 without a live sample gets the background: (0, 0, 0, 0, 0), or (1, 1, 1, 0, 0) under NNR_F_WHITE_BG.
 *   opt_count     (n_rays) int32 or NULL: the ray's live samples.
 *   opt_cell      (n_rays, n_samples) int32 or NULL: (i_z n_y + i_y) n_x + i_x of EVERY sample, -1 outside the grid.
 *   opt_out4      (n_rays, n_samples, 4) fp32 or NULL: (r, g, b, raw) of the LIVE samples; the rows of culled samples are not written.
 *   cfg           n_rays >= 1 (any: not only multiples of 4), 1 <= n_samples <= 256, hidden 128 / 256, flags NNR_F_SPLIT3 | NNR_F_SPLIT2
 *                 required; NNR_F_DIST_ALPHA, NNR_F_RELU_SIGMA and NNR_F_WHITE_BG are honoured.
 * NNR_E_BADCFG for a null pointer (other than jitter and the opt_*), a size below 1, a dim below 1, a grid_lo or grid_inv_step that is not
 * finite or an inverse step that is not positive; NNR_E_UNSUPPORTED for n_samples > 256, another hidden width, NNR_F_TRAIN or NNR_F_BF16,
 * missing split flags, more than 2^31 - 1 words or more than 2^31 - 1 cells; NNR_E_ALIGN for `packed` not 16-byte or another pointer not
 * 4-byte aligned; all decided before any device work.  No host synchronisation, no atomics: bit-reproducible. */
int nnr_render_sparse(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo, const float* z_hi,
                      const float* jitter, const float grid_lo[3], const float grid_inv_step[3], const int32_t grid_dims[3],
                      const uint32_t* bits, const float* packed, float* out, int32_t* opt_count, int32_t* opt_cell, float* opt_out4,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNR_SPARSE_H */
