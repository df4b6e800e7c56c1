/*
 * nnr_fusion.h -- the depth-fusion entry points of libnnr.so: the rendered depth of rays from the density alone, and
 * the integration of depth maps into a truncated signed distance volume held in 8 x 8 x 8 bricks.  The same C ABI as nnr.h (plain device
 * pointers and sizes, asynchronous on `stream`, no global state, the error codes and nnr_cfg of nnr.h); declared here, as nnr_geometry.h
 * declares its own, so that nnr.h's list of functions stays what it is.  nnr/lib.py lists them in FUSION_EXPORTS.  They change no
 * signature, struct or blob layout: the version stays nnr.h's.
 */
#ifndef NNR_FUSION_H
#define NNR_FUSION_H

#include "nnr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rendered depth of n_rays rays in ONE launch (nnr_depth_f16.hip), from the density alone: no colour branch, no view direction, and
 * nothing per sample through HBM.  Sampling is nnr_render_fwd's: sample j of ray r sits at z = z_lo[j] + (z_hi[j] - z_lo[j]) jitter[r][j]
 * (z_lo[j] where jitter is NULL), p = pts_o[r] + pts_d[r] z: nnr_render_fwd's depths and points, bit for bit (each of the two is one fused
 * multiply-add of the difference z_hi[j] - z_lo[j], respectively of z).  The raw density at p is, bit for bit, the
 * sigma_raw nnr_mlp_fwd writes for that point under the same flags.  Then, in fp32 and in a fixed order,
 *   alpha_j = the compositor's alpha of (raw_j, z_{j+1} - z_j) under NNR_F_DIST_ALPHA / NNR_F_RELU_SIGMA (the last delta is 1e10),
 *   T_j = prod_{i<j} (1 - alpha_i + 1e-6),  w_j = alpha_j T_j,  depth = sum w_j z_j,  acc = sum w_j.
 *   pts_o, pts_d  (n_rays, 3)          z_lo, z_hi  (n_samples)          jitter  (n_rays, n_samples) or NULL
 *   packed        the NNR_F_SPLIT3 | NNR_F_SPLIT2 buffer of nnr_pack_weights
 *   out           (n_rays, 2) fp32: (depth, acc) per ray.  (NaN, NaN) for a ray with a sample whose point is not finite, whose raw density
 *                 is NaN or where an activation left fp16's range; no other ray is affected.
 *   opt_raw, opt_z   (n_rays, n_samples) or NULL: the raw densities and depths of the samples, for tests.
 *   cfg           n_rays >= 1, 1 <= n_samples <= 256, hidden 128 / 256, flags NNR_F_SPLIT3 | NNR_F_SPLIT2 required; NNR_F_DIST_ALPHA and
 *                 NNR_F_RELU_SIGMA are honoured, NNR_F_WHITE_BG is ignored, NNR_F_TRAIN or NNR_F_BF16 -> NNR_E_UNSUPPORTED.
 * NNR_E_BADCFG for a null pointer (other than jitter, opt_raw, opt_z) or a size below 1; NNR_E_UNSUPPORTED for n_samples > 256, another hidden
 * width or the flags above; NNR_E_ALIGN for `packed` not 16-byte or another pointer not 4-byte aligned; all decided before any device work.
 * No host synchronisation, no atomics: bit-reproducible. */
int nnr_render_depth(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* z_lo, const float* z_hi, const float* jitter,
                     const float* packed, float* out, float* opt_raw, float* opt_z, void* stream);

/* Integrate n_cams depth maps into the truncated signed distance accumulators of a list of 8 x 8 x 8 bricks in ONE launch (nnr_tsdf.hip).
 * The grid and the bricks are nnr_density_bricks' (nnr_geometry.h): origin, step HOST arrays of three; brick (bx, by, bz) holds the grid
 * points i_c = 8 b_c + l_c, l_c = 0..7, at p_c = origin_c + step_c * (float) i_c, product and sum rounded to fp32 one after the other; bricks
 * may repeat, come in any order and reach past the grid: a coordinate feeds arithmetic only.
 *   bricks   (n_bricks, 3) int32 on the device
 *   cams     (n_cams, 12) fp32 on the device: rows 0..2 of the 4 x 4 matrix that takes a world point to the camera's (x w, y w, w), row-major;
 *            x, y in [-1, 1] across the image, w the z-depth
 *   depth    (n_cams, height, width) fp32 on the device: z-depth per pixel; NaN, zero and negative mean unobserved, +inf free space
 *   sum, weight   (n_bricks, 8, 8, 8) fp32 on the device, [b][lz][ly][lx], read at the start and written at the end
 * Per voxel, for the cameras in index order, every operation rounded to fp32 and none fused:
 *   q_r = ((P_r0 px + P_r1 py) + P_r2 pz) + P_r3;  skip unless q_z > z_min;  u = q_x / q_z, v = q_y / q_z;
 *   col = (u + 1) * (float)((width - 1) / 2), row = (v + 1) * (float)((height - 1) / 2);  ci = rint(col), ri = rint(row), ties to even;
 *   skip unless 0 <= ci <= width - 1 and 0 <= ri <= height - 1;  d = depth[c][ri][ci];  skip unless d > 0;  sd = q_z - d;
 *   skip unless sd <= trunc;  sum += max(sd / trunc, -1),  weight += 1.
 * sum / weight is positive behind the surfaces the cameras saw and negative in front of them.  Cameras may be passed in chunks over several
 * calls: the result is the one-call result bit for bit.
 * NNR_E_BADCFG for a null pointer, a size below 1, an origin, step, trunc or z_min that is not finite, trunc <= 0 or z_min < 0;
 * NNR_E_UNSUPPORTED for 512 n_bricks > 2^31 - 1, n_cams height width > 2^31 - 1, or height or width > 2^24; NNR_E_ALIGN for a pointer not
 * 4-byte aligned; all decided before any device work.  No host synchronisation, no atomics: bit-reproducible. */
int nnr_tsdf_integrate(const float origin[3], const float step[3], const int32_t* bricks, int32_t n_bricks, const float* cams, int32_t n_cams,
                       const float* depth, int32_t height, int32_t width, float trunc, float z_min, float* sum, float* weight, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNR_FUSION_H */
