/*
 * nnr_frozen_sparse.h -- the sparse frozen-field render of libnnr.so: the frozen-field render of nnr_frozen.h (ray
 * gradients against a field that does not move) that does not evaluate the samples an occupancy bitfield calls empty, forward or
 * backward.  The same C ABI as nnr.h (plain device pointers and sizes, asynchronous on `stream`, no global state, the error codes and
 * nnr_cfg of nnr.h); declared here, as nnr_frozen.h and nnr_sparse.h declare their own, so that nnr.h's list of functions stays what it
 * is.  nnr/lib.py lists these in FROZEN_SPARSE_EXPORTS.  No signature, struct or blob layout of nnr.h changes: the version stays nnr.h's.
 *
 * DEFINITION.  Inputs: those of nnr_frozen_fwd plus the grid of nnr_sparse.h (grid_lo, grid_inv_step, grid_dims, bits): the same cell
 * rule -- f_c = (p_c - grid_lo[c]) * grid_inv_step[c], every operation rounded to fp32 and none fused, INSIDE iff 0 <= f_c < (float) n_c on
 * all three axes, i_c = (int) f_c -- the same bit layout, the same LIVE rule: a sample is LIVE iff it lies outside the grid or its bit is
 * set; a point that is not finite is outside, hence live.  One addition: under NNR_F_DIST_ALPHA the LAST sample of every ray is always
 * live (its alpha is 1 whatever its density: the grid knows nothing about it).
 * The live list: `live` holds the flat indices ray * n_samples + j of the live samples in ascending order, n_live entries, built on the
 * device; the host never reads n_live (no synchronisation).  Fixed-order scans, no atomics: the list is deterministic.
 * Per sample:
 *   - a LIVE sample's row of P_OUT4 and its z, P_DPTS and P_DVIEW rows are written at the DENSE index ray * n_samples + j and equal, bit
 *     for bit, what nnr_frozen_fwd / nnr_frozen_bwd write for that sample -- but for a sample whose point is NOT FINITE (outside, hence
 *     live): its P_OUT4 row is NaN here, as in nnr_render_sparse, so its ray and that ray's gradients are NaN and no other ray is affected
 *     (nnr_frozen_fwd leaves such a sample to ReLU, which swallows the NaN: a finite row of no meaning);
 *   - a CULLED sample's P_OUT4 row is (0, 0, 0, E) with E = -inf (the bit pattern 0xff800000): for that raw density the compositor's
 *     alpha is exactly 0 and its derivative exactly 0, with softplus (log1p(exp(-inf)) = 0, sigmoid(-inf) = 0) as with NNR_F_RELU_SIGMA,
 *     with and without NNR_F_DIST_ALPHA (every delta between two finite depths is finite, and the last one is 1e10);
 *   - a culled sample's z is its z; its P_DPTS and P_DVIEW rows are zero.
 * The result is BY DEFINITION the unchanged compositor forward, compositor backward and per-ray reduction on those dense planes: the dense
 * frozen render of a field whose culled samples hold no matter.  A culled sample's transmittance factor is therefore (1 - 0) + 1e-6 as
 * rounded in fp32 (1.00000095...), where the sparse INFERENCE render of nnr_sparse.h leaves the sample out of the product (a factor of
 * exactly 1): over n culled samples the two differ by at most n 1e-6 relative.  opt_alpha of a culled sample is 0.
 * The rows of P_DOUT4 that belong to culled samples are the compositor's and are read by nothing.
 *
 * cfg: as for nnr_frozen_fwd (flags NNR_F_TRAIN | NNR_F_SPLIT3 | NNR_F_SPLIT2 required; NNR_F_DIST_ALPHA, NNR_F_RELU_SIGMA and
 * NNR_F_WHITE_BG honoured; hidden 128 / 256; n_samples <= 1024).  The two MLP kernels always run the flat decomposition here.
 * Errors, all decided before any device work: those of nnr_frozen.h (NNR_E_BADCFG for a null cfg, sizes below 1 or a null pointer other
 * than jitter and the opt_*; NNR_E_UNSUPPORTED for NNR_F_BF16, a missing flag of the three, another width or more samples; NNR_E_ALIGN for
 * `packed` or `ws` not 16-byte aligned) and the grid's of nnr_sparse.h (NNR_E_BADCFG for a null grid pointer, a dim below 1, a grid_lo or
 * grid_inv_step that is not finite or an inverse step that is not positive; NNR_E_UNSUPPORTED for more than 2^31 - 1 words or cells;
 * NNR_E_ALIGN for `bits` or an opt_* pointer not 4-byte aligned), plus NNR_E_UNSUPPORTED for more than 2^31 - 1 padded samples (the list
 * holds int32 indices).
 */
#ifndef NNR_FROZEN_SPARSE_H
#define NNR_FROZEN_SPARSE_H

#include "nnr_frozen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* plane ids of nnr_frozen_sparse_ws_plane beside those of nnr_ws_plane: the int32 planes behind the frozen workspace */
#define NNR_FS_LIVE 100      /* (S_pad) the live list; entries [n_live, S_pad) are not written */
#define NNR_FS_RAY_OFF 101   /* (n_rays) a ray's first place in the list */
#define NNR_FS_N_LIVE 102    /* (1) */
#define NNR_FS_RAY_COUNT 103 /* (n_rays) a ray's live samples */
#define NNR_FS_RAY_MASK 104  /* (n_rays, 32) bit j & 31 of word j >> 5: sample j of the ray is live */

/* The workspace, in 4-byte words (0 for a cfg the entry points refuse): the frozen workspace of nnr_frozen_workspace_floats(cfg), its planes
 * in their order, followed by live (S_pad int32), the ray offsets (n_rays), n_live (1), the ray counts (n_rays) and the ray bitmasks
 * (32 n_rays). */
size_t nnr_frozen_sparse_workspace_floats(const nnr_cfg* cfg);

/* Offset (4-byte words) of a plane: nnr_frozen_ws_plane's for its ids, the NNR_FS_* ids above (pitch 1, the mask 32); -1 otherwise. */
int64_t nnr_frozen_sparse_ws_plane(const nnr_cfg* cfg, int plane, int32_t* pitch_out);

/* The forward: compaction (three small launches: flags and substitutes, scan, fill), the list-driven frozen forward kernel, the compositor.
 *   pts_o .. packed, rgb .. opt_z     as for nnr_frozen_fwd
 *   grid_lo, grid_inv_step, grid_dims  HOST arrays of three;  bits (n_z, n_y, w_x) uint32 on the device: as for nnr_render_sparse
 *   opt_count    (n_rays) int32 or NULL: the ray's live samples
 *   opt_live     (n_rays n_samples) int32 or NULL and opt_n_live (1) int32 or NULL: copies of the list (its first n_live entries are
 *                written, nothing behind them) and of its length, written by the compaction's own kernels
 *   ws           nnr_frozen_sparse_workspace_floats(cfg) words, 16-byte aligned; need not be initialised */
int nnr_frozen_sparse_fwd(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo,
                          const float* z_hi, const float* jitter, const float grid_lo[3], const float grid_inv_step[3],
                          const int32_t grid_dims[3], const uint32_t* bits, const float* packed, float* rgb, float* dist, float* opt_alpha,
                          float* opt_z, int32_t* opt_count, int32_t* opt_live, int32_t* opt_n_live, float* ws, void* stream);

/* The backward: the compositor's backward, the list-driven frozen input-gradient kernel, the per-ray reduction.  `ws` is the workspace
 * nnr_frozen_sparse_fwd of the same cfg and inputs left; the arguments are nnr_frozen_bwd's. */
int nnr_frozen_sparse_bwd(const nnr_cfg* cfg, const float* packed, const float* d_rgb, const float* d_dist, float* d_pts_o, float* d_pts_d,
                          float* d_view, float* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNR_FROZEN_SPARSE_H */
