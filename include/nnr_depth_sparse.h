/*
 * nnr_depth_sparse.h -- the sparse depth render: nnr_render_depth (nnr_fusion.h) that does not evaluate the samples
 * an occupancy bitfield calls empty and stops a workgroup once its rays are opaque.  What the depth fusion of the TSDF export renders when
 * the field is frozen and a grid is at hand.  The same C ABI as nnr.h (plain device pointers and sizes, asynchronous on `stream`, no global
 * state, the error codes and nnr_cfg of nnr.h); declared here so that the lists of functions of nnr.h, nnr_fusion.h, nnr_sparse.h and
 * nnr_sparse_stop.h stay what they are.  nnr/lib.py lists it in DEPTH_SPARSE_EXPORTS.  It changes no signature, struct or blob layout:
 * the version stays nnr.h's.
 */
#ifndef NNR_DEPTH_SPARSE_H
#define NNR_DEPTH_SPARSE_H

#include "nnr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (depth, acc) of every ray in ONE launch (nnr_propose_f16.hip compiled with NNR_PROPOSE_SPARSE=1 NNR_PROPOSE_DEPTH=1): no colour branch,
 * no view direction, 8 bytes out per ray and nothing per sample.
 * In one sentence: give the same cfg, rays, tables, jitter, grid, t_min and packed to the stopping render of nnr_sparse_stop.h, with any
 * finite view_d and either value of NNR_F_WHITE_BG; then out[r] = (out_stop[r][3], out_stop[r][4]) bit for bit, and opt_count, opt_cell
 * and opt_passes are equal to that call's.
 * The definition, on its own.  Notation: workgroup g holds the rays 4g .. 4g + 3, one per wave; a wave past the last ray repeats ray
 * n_rays - 1 and stores nothing.
 *   sampling     z_j = z_lo[j] + (z_hi[j] - z_lo[j]) jitter[r][j] (z_lo[j] without jitter), p_j = pts_o[r] + pts_d[r] z_j, each operation
 *                rounded to fp32: nnr_render_depth's.
 *   live         f_c = (p_c - grid_lo[c]) * grid_inv_step[c], every operation rounded to fp32 and none fused; inside iff 0 <= f_c <
 *                (float) n_c on all three axes (a NaN fails: outside); i_c = (int) f_c; cell (i_x, i_y, i_z) is bit i_x & 31 of word
 *                (i_z n_y + i_y) w_x + (i_x >> 5), w_x = ceil(n_x / 32).  Sample j is LIVE iff it is outside the grid or its bit is set;
 *                otherwise it is CULLED.  n_r: the live samples of ray r.
 *   list         the live j of a ray in increasing order, l_0 < l_1 < ... < l_{n_r - 1}.
 *   passes       pass p evaluates the list entries 32 p .. 32 p + 31 of each of the workgroup's four rays.  After pass p ray r is DONE iff
 *                32 (p + 1) >= n_r or its transmittance carry T_r(p) < t_min (fp32 <; a NaN carry is never done by transmittance);
 *                P_g = the number of passes workgroup g runs = 0 where none of its rays has a live sample (such a workgroup reads no
 *                weight), otherwise 1 + the first p after which all four rays are done (at most max over its rays of ceil(n_r / 32)).
 *   evaluated    the first min(n_r, 32 P_g) entries of ray r's list: E_r.  A ray that is done by transmittance is composited further for
 *                as long as its workgroup runs.
 *   alpha        for j in E_r: the raw density is nnr_render_depth's bit for bit, incl. the NaN of a sample whose activations left fp16's
 *                range or whose point is not finite; alpha_j = the compositor's alpha (nnr.h: NNR_F_DIST_ALPHA, NNR_F_RELU_SIGMA) of that
 *                density and the delta z_{j+1} - z_j to the next sample of the ORIGINAL row, culled or not; 1e10 behind the last sample.
 *                As in the stopping render's columns 3 and 4, a NaN density is a NaN alpha except under NNR_F_RELU_SIGMA, where
 *                max(raw, 0) drops it and the sample weighs nothing.
 *   product      T_j = prod over the EVALUATED i < j of ray r of (1 - alpha_i + 1e-6): culled and unevaluated samples are absent.
 *                w_j = alpha_j T_j; depth = sum over E_r of w_j z_j, acc = sum over E_r of w_j; T_r(p) = the product over the entries of
 *                passes 0 .. p.  fp32, per pass a wave product scan in list order, the sums lane-wise across the passes and one
 *                butterfly at the end: the order of the stopping render.
 * Hence:
 *   with every bit set and t_min = 0 every raw density is nnr_render_depth's bit for bit, and (depth, acc) is that kernel's within the
 *   output bar of DESIGN.md section 2 -- not bit for bit: that kernel composites by lane runs, this one by passes;
 *   a culled or unevaluated sample is NOT EVALUATED and so can never make its ray NaN; a live evaluated one with a NaN alpha does, and
 *   only its own ray (a sample whose point is not finite is outside the grid, hence live);
 *   a ray without a live sample gets (0, 0);
 *   against t_min = 0 on the same grid |acc' - acc| <= T_stop (1 + C 1e-6 (1 + 1e-6)^C), T_stop < t_min the carry it stopped with, and
 *   |depth' - depth| at most that times the row's largest depth; stopping only ever LOWERS acc up to rounding.
 *   grid_lo, grid_inv_step, grid_dims      HOST arrays of three
 *   bits          (n_z, n_y, w_x) uint32 on the device
 *   t_min         0 <= t_min < 1; 0: no ray is ever done by transmittance, the full lists run
 *   out           (n_rays, 2): depth, acc
 *   opt_raw       (n_rays, n_samples) or NULL: the raw density of every EVALUATED sample; untouched elsewhere
 *   opt_count     (n_rays) int32 or NULL: n_r
 *   opt_cell      (n_rays, n_samples) int32 or NULL: (i_z n_y + i_y) n_x + i_x of EVERY sample, -1 outside the grid
 *   opt_passes    (n_rays) int32 or NULL: P_g of the ray's workgroup
 * Return codes, all decided before any device work (the outputs are untouched), in this precedence: NNR_E_BADCFG for a null cfg or pointer
 * (other than jitter and the opt_*), n_rays < 1, n_samples < 1, a dim below 1, a grid_lo or grid_inv_step that is not finite, an inverse
 * step that is not positive, a t_min outside 0 <= t_min < 1 or not finite; then NNR_E_UNSUPPORTED for n_samples > 256, a hidden width other
 * than 128 / 256, NNR_F_TRAIN or NNR_F_BF16, missing split flags, more than 2^31 - 1 words or cells; then NNR_E_ALIGN for `packed` not
 * 16-byte or another pointer not 4-byte aligned.  No host synchronisation, no atomics: bit-reproducible. */
int nnr_render_depth_sparse(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* z_lo, const float* z_hi,
                            const float* jitter, const float grid_lo[3], const float grid_inv_step[3], const int32_t grid_dims[3],
                            const uint32_t* bits, float t_min, const float* packed, float* out,
                            float* opt_raw, int32_t* opt_count, int32_t* opt_cell, int32_t* opt_passes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNR_DEPTH_SPARSE_H */
