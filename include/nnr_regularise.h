/*
 * nnr_regularise.h -- regularisers on the compositing weights of libnnr.so: the ray distortion of mip-NeRF 360, forward
 * and backward.  The same C ABI as nnr.h (plain device pointers and sizes, asynchronous on `stream`, no global state, the error codes and
 * nnr_cfg of nnr.h); declared here, as nnr_geometry.h, nnr_fusion.h and nnr_sparse.h declare their own, so that nnr.h's list of functions
 * stays what it is.  nnr/lib.py lists them in REGULARISE_EXPORTS.  They change no signature, struct or blob layout: the version stays nnr.h's.
 */
#ifndef NNR_REGULARISE_H
#define NNR_REGULARISE_H

#include "nnr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The ray distortion of n_rays rays of N = n_samples samples each (nnr_ray_distortion.hip).  Sample j of ray r is raw[(r N + j) raw_stride]
 * (sigma_raw, the density before its activation) at depth z[r N + j]; z is non-decreasing along a ray.  Strides count floats: stride 4 with
 * the pointer at column 3 addresses plane 0 (and, for d_raw, plane 2) of a training workspace, stride 1 a plain (n_rays, N) tensor.
 * All arithmetic runs in float64 on the fp32 inputs, as nnr_composite_bwd's does, and is rounded to fp32 once at each store.
 *   alpha_j, T_j = prod_{i<j} (1 - alpha_i + 1e-6f), w_j = alpha_j T_j: the compositor's, under NNR_F_DIST_ALPHA / NNR_F_RELU_SIGMA: delta_j is
 *     the FP32 difference z_{j+1} - z_j, the last delta 1e10f; under NNR_F_DIST_ALPHA the last alpha is 1, with no gradient through it.
 *   s_j = (z_j - s_near) * s_inv: the normalised depth (the renderer passes the coarse range: near and 1 / (far - near), or 0 and 1 under ndc).
 *   m_j = (s_j + s_{j+1}) / 2, d_j = s_{j+1} - s_j for j < N - 1;  m_{N-1} = s_{N-1}, d_{N-1} = 0 (the compositor's closing 1e10 is a
 *     convention, not a length).
 *   L = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
 *     = 2 sum_k w_k (m_k W_<k - M_<k) + (1/3) sum_k w_k^2 d_k,   W_<k, M_<k the exclusive prefix sums of w and w m.
 *   a_k = dL/dw_k = 2 [m_k (W_<k - W_>k) - M_<k + M_>k] + (2/3) w_k d_k,   W_>k, M_>k the exclusive suffix sums;
 *   dL/dalpha_j = T_j a_j - B_j / (1 - alpha_j + 1e-6f),  B_j = sum_{m>j} w_m a_m (a true reverse sum);  dL/draw_j = dL/dalpha_j dalpha_j/draw_j.
 * z carries no gradient.  N = 1 gives exactly 0, loss and gradient.  A NaN in a ray makes that ray's loss and all its gradients NaN and
 * touches no other ray.
 *   fwd:  loss (n_rays) = L of every ray.
 *   bwd:  g (n_rays) the upstream gradient of `loss`; d_raw[(r N + j) d_raw_stride] receives v = g_r dL_r/draw_j: overwritten with (float) v
 *         where accumulate == 0, else (float) ((double) d_raw + v).  Nothing else of d_raw is read or written.
 * From cfg only n_rays, n_samples and the flags NNR_F_DIST_ALPHA / NNR_F_RELU_SIGMA are read: every other flag and `hidden` are ignored, the
 * functions serve every product mode.
 * NNR_E_BADCFG for a null pointer, n_rays, n_samples or a stride below 1, an s_near or s_inv that is not finite or an s_inv <= 0;
 * NNR_E_UNSUPPORTED for n_samples > 1024 (nnr_composite_bwd's limit); NNR_E_ALIGN for a pointer not 4-byte aligned; all decided before any
 * device work.  One launch each, one wave per ray, every sum in a fixed order, no atomics, no host synchronisation: bit-reproducible. */
int nnr_ray_distortion_fwd(const nnr_cfg* cfg, const float* raw, int32_t raw_stride, const float* z, float s_near, float s_inv,
                           float* loss, void* stream);
int nnr_ray_distortion_bwd(const nnr_cfg* cfg, const float* raw, int32_t raw_stride, const float* z, float s_near, float s_inv,
                           const float* g, float* d_raw, int32_t d_raw_stride, int32_t accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNR_REGULARISE_H */
