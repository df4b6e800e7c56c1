/*
 * nnr_geometry.h -- the geometry-export entry points of libnnr.so that came after include/nnr.h's own set was closed: the same C ABI (plain
 * device pointers and sizes, asynchronous on `stream`, no global state, the error codes and nnr_cfg of nnr.h), declared here so that nnr.h's
 * list of functions -- which nnr/lib.py's EXPORTS mirrors one to one -- stays what it is.  New geometry-side entry points go into this
 * header and into nnr/lib.py's GEOMETRY_EXPORTS; they change no signature, struct or blob layout, so NNR_ABI_VERSION (nnr.h) stays.
 */
#ifndef NNR_GEOMETRY_H
#define NNR_GEOMETRY_H

#include "nnr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The raw density of the field in a list of 8 x 8 x 8 BRICKS of a regular grid in ONE launch (nnr_bricks_f16.hip; model/geometry.py refines a
 * coarse mesh with it: extract_mesh_refined): the density where a surface is, at a resolution whose whole volume nobody could afford.
 * The grid is that of the density-grid entry point of nnr.h: origin, step are HOST arrays of three, grid point (ix, iy, iz) is
 * p_c = origin_c + step_c * (float) i_c, the product and the sum rounded to fp32 one after the other.
 *   bricks   (n_bricks, 3) int32 on the device, (bx, by, bz) per brick, non-negative.  Brick (bx, by, bz) holds the grid points
 *            i_c = 8 b_c + l_c, l_c = 0..7.  Bricks may repeat and come in any order.  The grid has no dims here: a brick that reaches past
 *            the caller's last grid point is evaluated all the same (those voxels are the field at the points the formula gives), and a
 *            coordinate feeds arithmetic only, never an address -- a wrong one gives a meaningless value, no access out of bounds.
 *   out      (n_bricks, 8, 8, 8) fp32 on the device: out[b][lz][ly][lx], x fastest, 512 n_bricks floats and no padding.  Every voxel is, bit
 *            for bit, what the density-grid entry point writes for the same grid point (the sigma_raw nnr_mlp_fwd writes for that point);
 *            NaN where an activation left fp16's range (NNR_F_SPLIT2).
 *   cfg      n_rays = 512 n_bricks, n_samples = 1, hidden 128 / 256, flags NNR_F_SPLIT3 | NNR_F_SPLIT2 (required: the kernel evaluates in the
 *            two-term fp16 arithmetic, `packed` is that mode's buffer); NNR_F_TRAIN or NNR_F_BF16 -> NNR_E_UNSUPPORTED (NNR_F_DIST_ALPHA /
 *            NNR_F_RELU_SIGMA / NNR_F_WHITE_BG are ignored: the output is the density before its activation).
 * NNR_E_BADCFG for a null pointer, n_bricks < 1, an origin or step that is not finite, n_rays != 512 n_bricks or n_samples != 1;
 * NNR_E_UNSUPPORTED for 512 n_bricks > 2^31 - 1, another hidden width or the flags above; NNR_E_ALIGN for `packed` not 16-byte or `bricks` /
 * `out` not 4-byte aligned; all decided before any device work.  One launch, no host synchronisation, no atomics: bit-reproducible. */
int nnr_density_bricks(const nnr_cfg* cfg, const float origin[3], const float step[3], const int32_t* bricks, int32_t n_bricks,
                       const float* packed, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNR_GEOMETRY_H */
