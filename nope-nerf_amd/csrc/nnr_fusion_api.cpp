// nnr_fusion_api.cpp -- the extern "C" entry points of include/nnr_fusion.h (the depth-fusion side of the geometry export) and the dense entry
// of include/nnr_depth_median.h (the same depth render with the quantile depth beside): argument checking
// and marshalling into the two kernels' argument structs (nnr_fusion_kernels.h).  A host unit of its own: nnr_api.cpp keeps nnr.h's and
// nnr_geometry.h's sets.  Every error return is decided before any device work -- no pointer is dereferenced here except the host arrays
// `origin` and `step` -- and every call is asynchronous on the caller's stream.  No state: the last HIP error is nnr_api.cpp's (launched).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/nnr_depth_median.h"
#include "../../include/nnr_fusion.h"
#include "nnr_fusion_kernels.h"

using namespace nnr;

namespace {

bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }      // n a power of two; null passes

}  // namespace

extern "C" {

int nnr_render_depth(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* z_lo, const float* z_hi, const float* jitter,
                     const float* packed, float* out, float* opt_raw, float* opt_z, void* stream) {
    if (!cfg || cfg->n_rays < 1 || cfg->n_samples < 1) return NNR_E_BADCFG;
    if (!pts_o || !pts_d || !z_lo || !z_hi || !packed || !out) return NNR_E_BADCFG;      // (jitter and the opt_* may be null)
    if (cfg->n_samples > 256 || (cfg->hidden != 128 && cfg->hidden != 256)) return NNR_E_UNSUPPORTED;
    if ((cfg->flags & (NNR_F_BF16 | NNR_F_SPLIT3 | NNR_F_SPLIT2)) != (NNR_F_SPLIT3 | NNR_F_SPLIT2) || (cfg->flags & NNR_F_TRAIN)) return NNR_E_UNSUPPORTED;
    if (!aligned(packed, 16)) return NNR_E_ALIGN;
    for (const void* p : {(const void*)pts_o, (const void*)pts_d, (const void*)z_lo, (const void*)z_hi, (const void*)jitter, (const void*)out,
                          (const void*)opt_raw, (const void*)opt_z})
        if (!aligned(p, 4)) return NNR_E_ALIGN;
    DepthArgs a{};
    a.pts_o = pts_o; a.pts_d = pts_d; a.z_lo = z_lo; a.z_hi = z_hi; a.jitter = jitter; a.packed = packed;
    a.out = out; a.opt_raw = opt_raw; a.opt_z = opt_z;
    a.R = cfg->n_rays; a.C = cfg->n_samples;
    a.flags = cfg->flags & (NNR_F_RELU_SIGMA | NNR_F_DIST_ALPHA);
    return launched(launch_render_depth(cfg->hidden, a, (hipStream_t)stream));
}

// nnr_render_depth's checks in their order; `level` is a value: it is refused with the sizes and the null pointers
int nnr_render_depth_median(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* z_lo, const float* z_hi, const float* jitter,
                            float level, const float* packed, float* out, float* opt_raw, float* opt_z, void* stream) {
    if (!cfg || cfg->n_rays < 1 || cfg->n_samples < 1) return NNR_E_BADCFG;
    if (!pts_o || !pts_d || !z_lo || !z_hi || !packed || !out) return NNR_E_BADCFG;      // (jitter and the opt_* may be null)
    if (!(level > 0.f && level < 1.f)) return NNR_E_BADCFG;      // (a NaN fails both comparisons)
    if (cfg->n_samples > 256 || (cfg->hidden != 128 && cfg->hidden != 256)) return NNR_E_UNSUPPORTED;
    if ((cfg->flags & (NNR_F_BF16 | NNR_F_SPLIT3 | NNR_F_SPLIT2)) != (NNR_F_SPLIT3 | NNR_F_SPLIT2) || (cfg->flags & NNR_F_TRAIN)) return NNR_E_UNSUPPORTED;
    if (!aligned(packed, 16)) return NNR_E_ALIGN;
    for (const void* p : {(const void*)pts_o, (const void*)pts_d, (const void*)z_lo, (const void*)z_hi, (const void*)jitter, (const void*)out,
                          (const void*)opt_raw, (const void*)opt_z})
        if (!aligned(p, 4)) return NNR_E_ALIGN;
    DepthMedianArgs a{};
    a.pts_o = pts_o; a.pts_d = pts_d; a.z_lo = z_lo; a.z_hi = z_hi; a.jitter = jitter; a.packed = packed;
    a.out = out; a.opt_raw = opt_raw; a.opt_z = opt_z;
    a.R = cfg->n_rays; a.C = cfg->n_samples;
    a.flags = cfg->flags & (NNR_F_RELU_SIGMA | NNR_F_DIST_ALPHA);
    a.level = level;
    return launched(launch_render_depth_median(cfg->hidden, a, (hipStream_t)stream));
}

int nnr_tsdf_integrate(const float origin[3], const float step[3], const int32_t* bricks, int32_t n_bricks, const float* cams, int32_t n_cams,
                       const float* depth, int32_t height, int32_t width, float trunc, float z_min, float* sum, float* weight, void* stream) {
    if (!origin || !step || !bricks || !cams || !depth || !sum || !weight) return NNR_E_BADCFG;
    if (n_bricks < 1 || n_cams < 1 || height < 1 || width < 1) return NNR_E_BADCFG;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(origin[c]) || !std::isfinite(step[c])) return NNR_E_BADCFG;
    if (!std::isfinite(trunc) || !(trunc > 0.f) || !std::isfinite(z_min) || !(z_min >= 0.f)) return NNR_E_BADCFG;
    if (512 * (int64_t)n_bricks > INT32_MAX) return NNR_E_UNSUPPORTED;
    if (height > kTsdfMaxExtent || width > kTsdfMaxExtent) return NNR_E_UNSUPPORTED;      // (the kernel compares pixel indices as fp32)
    if ((int64_t)n_cams * height > INT32_MAX || (int64_t)n_cams * height * width > INT32_MAX) return NNR_E_UNSUPPORTED;
    for (const void* p : {(const void*)bricks, (const void*)cams, (const void*)depth, (const void*)sum, (const void*)weight})
        if (!aligned(p, 4)) return NNR_E_ALIGN;
    TsdfArgs a{};
    a.bricks = bricks; a.cams = cams; a.depth = depth; a.sum = sum; a.weight = weight;
    for (int c = 0; c < 3; ++c) { a.origin[c] = origin[c]; a.step[c] = step[c]; }
    a.trunc = trunc; a.z_min = z_min;
    a.cw = (float)((double)(width - 1) / 2.0); a.ch = (float)((double)(height - 1) / 2.0);
    a.col_max = (float)(width - 1); a.row_max = (float)(height - 1);
    a.n_cams = n_cams; a.H = height; a.W = width;
    a.V = 512u * (uint32_t)n_bricks;
    return launched(launch_tsdf_integrate(a, (hipStream_t)stream));
}

}  // extern "C"
