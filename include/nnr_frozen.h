/*
 * nnr_frozen.h -- the frozen-field render of libnnr.so: nnr_render_fwd / nnr_render_bwd for a step in which only the
 * RAYS are differentiated (test-time pose refinement against a trained field).  The outputs and the ray gradients are those of the
 * training path bit for bit; there are no weight gradients, and nothing is kept for one: no hidden-activation plane, no gradient plane, no
 * plane maxima.  The same C ABI as nnr.h (plain device pointers and sizes, asynchronous on `stream`, no global state, the error codes
 * and nnr_cfg of nnr.h); declared here, as nnr_sparse.h and nnr_fusion.h declare their own, so that nnr.h's list of functions stays what it
 * is.  nnr/lib.py lists these in FROZEN_EXPORTS.  No signature, struct or blob layout of nnr.h changes: the version stays nnr.h's.
 *
 * cfg: as for the training path, flags NNR_F_TRAIN | NNR_F_SPLIT3 | NNR_F_SPLIT2 required (the two-term fp16 products, the only mode with
 * frozen kernels); NNR_F_DIST_ALPHA, NNR_F_RELU_SIGMA and NNR_F_WHITE_BG are honoured; hidden 128 / 256; n_samples <= 1024.  Ray mode and
 * flat mode are chosen as nnr_render_fwd chooses them.  NNR_E_BADCFG for a null cfg or sizes below 1; NNR_E_UNSUPPORTED for NNR_F_BF16, a
 * missing flag of the three, another width or more samples.
 */
#ifndef NNR_FROZEN_H
#define NNR_FROZEN_H

#include "nnr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The frozen workspace, in floats (0 for a cfg the entry points refuse).  It holds exactly the planes
 *   P_OUT4 (4)  P_Z (1)  P_DOUT4 (4)  P_DPTS (4)  P_DVIEW (4)  P_XE (64)  P_XF (32)  P_MASK (18 hidden / 64)
 * in this order, each S_pad rows of the width in brackets (floats per sample; S_pad = n_rays n_samples rounded up to a multiple of 128):
 * 185 floats per padded sample at hidden 256, 149 at 128.  Nothing follows the last plane. */
size_t nnr_frozen_workspace_floats(const nnr_cfg* cfg);

/* Offset (floats) of plane `plane` (the ids of nnr_ws_plane) in the frozen workspace and, through pitch_out (may be NULL), its floats per
 * sample.  -1 for every plane the frozen workspace does not have (P_XH1..8, P_XG, P_DH1..8, P_DG, ...) and for a refused cfg.
 * The planes have the training workspace's layouts (P_XE, P_XF tile-major, P_MASK [chunk][layer][lane][words]). */
int64_t nnr_frozen_ws_plane(const nnr_cfg* cfg, int plane, int32_t* pitch_out);

/* nnr_render_fwd of a training cfg without the stashes: the frozen forward kernel (gate words, both encodings, z and the per-sample outputs
 * into `ws`; a sample whose activations leave fp16's range is NaN, as on the training path), then the compositor.
 *   pts_o, pts_d, view_d (n_rays, 3)   z_lo, z_hi (n_samples)   jitter (n_rays, n_samples) or NULL
 *   packed      the NNR_F_SPLIT3 | NNR_F_SPLIT2 buffer of nnr_pack_weights
 *   rgb (n_rays, 3), dist (n_rays); opt_alpha, opt_z (n_rays, n_samples) or NULL
 *   ws          nnr_frozen_workspace_floats(cfg) floats, 16-byte aligned; need not be initialised
 * NNR_E_BADCFG for a null pointer (other than jitter and the opt_*), NNR_E_ALIGN for `packed` or `ws` not 16-byte aligned. */
int nnr_frozen_fwd(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo, const float* z_hi,
                   const float* jitter, const float* packed, float* rgb, float* dist, float* opt_alpha, float* opt_z, float* ws, void* stream);

/* nnr_render_bwd without the weight gradient: the compositor's backward, the frozen input-gradient kernel, the per-ray reduction.
 * `ws` is the workspace nnr_frozen_fwd of the same cfg and inputs left.  No plan, no gradient tensors, no memset.
 *   d_rgb (n_rays, 3), d_dist (n_rays)      upstream gradients
 *   d_pts_o, d_pts_d, d_view (n_rays, 3)    overwritten */
int nnr_frozen_bwd(const nnr_cfg* cfg, const float* packed, const float* d_rgb, const float* d_dist, float* d_pts_o, float* d_pts_d,
                   float* d_view, float* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNR_FROZEN_H */
