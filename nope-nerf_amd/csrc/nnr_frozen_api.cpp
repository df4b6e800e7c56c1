// nnr_frozen_api.cpp -- the extern "C" entry points of include/nnr_frozen.h (the frozen-field render): the frozen workspace's layout,
// argument checking, marshalling into the training kernels' argument blocks and the sequencing of the launches.  Its own file, as
// nnr_sparse_api.cpp is, but compiled as the tail of nnr_api.cpp's unit (which includes it): it is the one family that needs the host
// planner's cfg helpers (nnr_wgrad_plan.h: ws_layout), and those stay the business of nnr_api.cpp and nnr_wgrad_plan.cpp alone.  Hence the
// helpers' own namespace below.  Every error return is decided before any device work, every call is asynchronous on the caller's stream.
// No state: the last HIP error is nnr_api.cpp's (launched).
// The argument blocks are value-initialised and only the planes of the frozen workspace are filled in: ws_xh, ws_xg, ws_dh, ws_dg and
// plane_max stay NULL.  The two kernels launched here are built without any store through them (nnr_frozen_kernels.h).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nnr_frozen.h"
#include "nnr_frozen_kernels.h"
#include "nnr_wgrad_plan.h"

using namespace nnr;

namespace frozen_detail {

bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }      // n a power of two; null passes

int check_cfg(const nnr_cfg* c) {
    if (!c || c->n_rays <= 0 || c->n_samples <= 0) return NNR_E_BADCFG;
    if (c->hidden != 128 && c->hidden != 256) return NNR_E_UNSUPPORTED;
    if (c->n_samples > 1024) return NNR_E_UNSUPPORTED;      // (the compositor's bound for a training cfg: nnr_api.cpp)
    constexpr uint32_t need = NNR_F_TRAIN | NNR_F_SPLIT3 | NNR_F_SPLIT2;
    if ((c->flags & NNR_F_BF16) || (c->flags & need) != need) return NNR_E_UNSUPPORTED;
    return NNR_OK;
}

// The planes of the frozen workspace in their order, floats per sample each: what the input-gradient kernel reads from the forward (gate
// words, both encodings), what the compositor and the per-ray reduction exchange with the two kernels, nothing else.
struct FrozenWs {
    int64_t S, S_pad;
    int D;
    explicit FrozenWs(const nnr_cfg* c) {
        const WsLayout w = ws_layout(c);      // (the sample counts alone: the padding rule is the training workspace's)
        S = w.S; S_pad = w.S_pad; D = c->hidden;
    }
    // offset of plane p, -1 if absent; p == -1: the total
    int64_t plane(int p, int* pitch) const {
        const int ids[8] = {P_OUT4, P_Z, P_DOUT4, P_DPTS, P_DVIEW, P_XE, P_XF, P_MASK};
        const int widths[8] = {4, 1, 4, 4, 4, kPosPad, kDirPad, 9 * 2 * (D / 64)};
        int64_t o = 0;
        for (int i = 0; i < 8; ++i) {
            if (ids[i] == p) { *pitch = widths[i]; return o; }
            o += S_pad * (int64_t)widths[i];
        }
        *pitch = 0;
        return p == -1 ? o : -1;
    }
    int64_t at(int p) const { int pitch; return plane(p, &pitch); }
};

CompositeArgs composite_args(const nnr_cfg* cfg, const FrozenWs& w, float* ws) {
    CompositeArgs a{};
    a.ws_out4 = ws + w.at(P_OUT4);
    a.ws_z = ws + w.at(P_Z);
    a.R = cfg->n_rays; a.N = cfg->n_samples; a.flags = cfg->flags;
    return a;
}

}  // namespace frozen_detail

extern "C" {

size_t nnr_frozen_workspace_floats(const nnr_cfg* cfg) {
    return frozen_detail::check_cfg(cfg) == NNR_OK ? (size_t)frozen_detail::FrozenWs(cfg).at(-1) : 0;
}

int64_t nnr_frozen_ws_plane(const nnr_cfg* cfg, int pl, int32_t* pitch_out) {
    if (frozen_detail::check_cfg(cfg) != NNR_OK) return -1;
    int pitch = 0;
    const int64_t o = frozen_detail::FrozenWs(cfg).plane(pl, &pitch);
    if (pitch_out) *pitch_out = pitch;
    return pl < 0 ? -1 : o;
}

int nnr_frozen_fwd(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo, const float* z_hi,
                   const float* jitter, const float* packed, float* rgb, float* dist, float* opt_alpha, float* opt_z, float* ws, void* stream) {
    int rc = frozen_detail::check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!pts_o || !pts_d || !view_d || !z_lo || !z_hi || !packed || !rgb || !dist || !ws) return NNR_E_BADCFG;      // (jitter and the opt_* may be null)
    if (!frozen_detail::aligned(packed, 16) || !frozen_detail::aligned(ws, 16)) return NNR_E_ALIGN;
    const frozen_detail::FrozenWs w(cfg);
    MlpFwdArgs a{};
    a.pts_o = pts_o; a.pts_d = pts_d; a.view_d = view_d; a.z_lo = z_lo; a.z_hi = z_hi; a.jitter = jitter;
    a.packed = packed;
    a.ws_out4 = ws + w.at(P_OUT4);
    a.ws_z = ws + w.at(P_Z);
    a.ws_xe = ws + w.at(P_XE);
    a.ws_xf = ws + w.at(P_XF);
    a.ws_mask = reinterpret_cast<uint32_t*>(ws + w.at(P_MASK));
    a.S = w.S; a.S_pad = w.S_pad; a.N = cfg->n_samples;
    a.chunks_per_ray = chunks_per_ray(cfg);
    a.flags = cfg->flags;
    const hipStream_t st = (hipStream_t)stream;
    const hipError_t e = cfg->hidden == 256 ? launch_mlp_fwd_frozen_variant<256>(a, st) : launch_mlp_fwd_frozen_variant<128>(a, st);
    if (e != hipSuccess) return launched(e);
    CompositeArgs c = frozen_detail::composite_args(cfg, w, ws);
    c.rgb = rgb; c.dist = dist; c.opt_alpha = opt_alpha; c.opt_z = opt_z;
    return launched(launch_composite_fwd(c, st));
}

int nnr_frozen_bwd(const nnr_cfg* cfg, const float* packed, const float* d_rgb, const float* d_dist, float* d_pts_o, float* d_pts_d,
                   float* d_view, float* ws, void* stream) {
    int rc = frozen_detail::check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!packed || !d_rgb || !d_dist || !d_pts_o || !d_pts_d || !d_view || !ws) return NNR_E_BADCFG;
    if (!frozen_detail::aligned(packed, 16) || !frozen_detail::aligned(ws, 16)) return NNR_E_ALIGN;
    const frozen_detail::FrozenWs w(cfg);
    const hipStream_t st = (hipStream_t)stream;
    CompositeArgs c = frozen_detail::composite_args(cfg, w, ws);
    c.ws_dout4 = ws + w.at(P_DOUT4);
    c.d_rgb = d_rgb; c.d_dist = d_dist;
    hipError_t e = launch_composite_bwd(c, st);
    if (e != hipSuccess) return launched(e);
    MlpDgradArgs a{};
    a.packed = packed;
    a.ws_dout4 = ws + w.at(P_DOUT4);
    a.ws_xe = ws + w.at(P_XE);
    a.ws_xf = ws + w.at(P_XF);
    a.ws_mask = reinterpret_cast<const uint32_t*>(ws + w.at(P_MASK));
    a.ws_dpts = ws + w.at(P_DPTS);
    a.ws_dview = ws + w.at(P_DVIEW);
    a.S = w.S; a.S_pad = w.S_pad;
    a.chunks_per_ray = chunks_per_ray(cfg);
    e = cfg->hidden == 256 ? launch_mlp_dgrad_frozen_variant<256>(a, st) : launch_mlp_dgrad_frozen_variant<128>(a, st);
    if (e != hipSuccess) return launched(e);
    RayReduceArgs r{};
    r.ws_dpts = ws + w.at(P_DPTS);
    r.ws_dview = ws + w.at(P_DVIEW);
    r.ws_z = ws + w.at(P_Z);
    r.d_pts_o = d_pts_o; r.d_pts_d = d_pts_d; r.d_view = d_view;
    r.R = cfg->n_rays; r.N = cfg->n_samples;
    return launched(launch_ray_reduce(r, st));
}

}  // extern "C"
