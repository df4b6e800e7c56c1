/*
 * nnr_sparse_stop.h -- the sparse inference render with early ray termination: nnr_render_sparse (nnr_sparse.h)
 * whose workgroups stop walking their rays' live lists once all four rays are opaque.  The same C ABI as nnr.h; declared here so that
 * nnr_sparse.h's list of functions stays what it is.  nnr/lib.py lists it in SPARSE_STOP_EXPORTS.  It changes no signature, struct or blob
 * layout: the version stays nnr.h's.
 */
#ifndef NNR_SPARSE_STOP_H
#define NNR_SPARSE_STOP_H

#include "nnr_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nnr_render_sparse, in ONE launch (nnr_sparse_f16.hip compiled with NNR_SPARSE_STOP=1), stopped per workgroup.  Every argument it shares
 * with nnr_render_sparse means what it means there: the sampling, the grid, the cell rule, the live list, a live sample's (r, g, b, raw), its
 * alpha and the compositing expressions and their order are that function's.
 * Notation: kChunk = 32.  Ray r has the live list j_0 < j_1 < ... < j_{n_r - 1} (nnr_render_sparse's list, unchanged).  Workgroup g holds the
 * rays 4g .. 4g + 3, one per wave; a wave past the last ray repeats ray n_rays - 1.  n_pass_g = max_r ceil(n_r / 32), the passes
 * nnr_render_sparse runs.  T_r(p), the fp32 transmittance carry of ray r after pass p, is the product of (1 - alpha + 1e-6) over its first
 * min(n_r, 32 (p + 1)) live samples, in the kernel's order.
 * The rule:
 *   wave r is DONE AFTER PASS p iff 32 (p + 1) >= n_r or T_r(p) < t_min (an fp32 <; a NaN carry is never done by transmittance: it ends by
 *   exhaustion of its list);
 *   workgroup g runs P_g passes, the smallest p + 1 such that all four waves are done after pass p: P_g <= n_pass_g, and P_g = 0 where
 *   n_pass_g = 0.  No lag: the decision taken after pass p governs pass p + 1;
 *   every ray of g composites its first min(n_r, 32 P_g) live samples, with nnr_render_sparse's expressions and order.  A wave that is done
 *   by transmittance keeps compositing for as long as its workgroup runs (the waves walk the weight stream together);
 *   the outputs come from these EVALUATED samples alone: out[0..4], the white background 1 - sum w, and under NNR_F_DIST_ALPHA the closing
 *   alpha (the last sample of the original list closes the ray only if it was evaluated).  A ray is NaN iff one of its evaluated samples is.
 *   t_min = 0 stops nothing: the outputs are nnr_render_sparse's bit for bit.
 * What stopping costs a ray is bounded by the transmittance it stopped with: the dropped weights sum to at most
 * T_stop (1 + C 1e-6 (1 + 1e-6)^C), C = n_samples; so |d rgb_c| and |d sum w| are at most that (also under NNR_F_WHITE_BG) and |d sum w z| at
 * most that times the largest z; T_stop < t_min for a ray that was done by transmittance, and a ray whose workgroup stopped while it was
 * only exhausted loses nothing.
 *   t_min         0 <= t_min < 1
 *   opt_passes    (n_rays) int32 or NULL: P_g of the ray's workgroup.
 *   opt_out4      as in nnr_render_sparse, but only the rows of EVALUATED samples are written.
 *   opt_count, opt_cell   nnr_render_sparse's, unchanged (the whole live list, stopped or not).
 * Return codes: nnr_render_sparse's, with its precedence, for everything that function refuses; NNR_E_BADCFG also for a t_min that is NaN,
 * negative or >= 1; NNR_E_ALIGN also for an opt_passes that is not 4-byte aligned; all decided before any device work.  This entry always
 * launches the stopping kernel, also for t_min = 0.  No host synchronisation, no atomics: bit-reproducible. */
int nnr_render_sparse_stop(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo, const float* z_hi,
                           const float* jitter, const float grid_lo[3], const float grid_inv_step[3], const int32_t grid_dims[3],
                           const uint32_t* bits, const float* packed, float t_min, float* out, int32_t* opt_count, int32_t* opt_cell,
                           float* opt_out4, int32_t* opt_passes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNR_SPARSE_STOP_H */
