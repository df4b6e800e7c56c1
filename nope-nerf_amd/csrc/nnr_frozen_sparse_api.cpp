// nnr_frozen_sparse_api.cpp -- the extern "C" entry points of include/nnr_frozen_sparse.h (the sparse frozen-field render): the workspace's
// layout, argument checking, marshalling and the sequencing of the launches.  Its own file, as nnr_frozen_api.cpp is, and like it compiled as
// the tail of nnr_api.cpp's unit (which includes it); the family's kernels of its own, the compaction front end nnr_frozen_sparse.hip, are
// compiled with it (included below): csrc/build.py's list of source files stays what it is.  Hence the helpers' own namespace.  The frozen
// planes are where nnr_frozen_ws_plane says (nnr_frozen_api.cpp, asked through the C ABI: one layout, stated once); the int32 planes of the
// compaction follow them.  Every error return is decided before any device work, every call is asynchronous on the caller's stream.  No
// state: the last HIP error is nnr_api.cpp's (launched).
// The two MLP kernels always run the flat decomposition (chunks_per_ray = 0) on the dense grid of S_pad / 128 workgroups; the three shared
// launchers (compositor forward and backward, per-ray reduction) are the dense path's, on the dense planes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/nnr_frozen_sparse.h"
#include "nnr_frozen_sparse_kernels.h"
#include "nnr_layout.h"

#include "nnr_frozen_sparse.hip"      // the compaction kernels and launch_frozen_sparse_compact: this family's device code, in this unit

using namespace nnr;

namespace frozen_sparse_detail {

bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }      // n a power of two; null passes

struct SparseWs {
    int64_t S = 0, S_pad = 0, R = 0;
    int64_t frozen = 0;      // words of the frozen workspace in front
    bool ok = false;
    explicit SparseWs(const nnr_cfg* c) {
        frozen = (int64_t)nnr_frozen_workspace_floats(c);      // 0: a cfg nnr_frozen.h refuses
        if (frozen == 0) return;
        R = c->n_rays;
        S = R * c->n_samples;
        S_pad = (S + kBlockSamples - 1) / kBlockSamples * kBlockSamples;
        ok = S_pad <= INT32_MAX;
    }
    int64_t extra(int id, int* pitch) const {      // the NNR_FS_* planes; id == -1: the total
        const int ids[5] = {NNR_FS_LIVE, NNR_FS_RAY_OFF, NNR_FS_N_LIVE, NNR_FS_RAY_COUNT, NNR_FS_RAY_MASK};
        const int64_t sizes[5] = {S_pad, R, 1, R, R * kFrozenSparseMaskWords};
        const int pitches[5] = {1, 1, 1, 1, kFrozenSparseMaskWords};
        int64_t o = frozen;
        for (int i = 0; i < 5; ++i) {
            if (ids[i] == id) { *pitch = pitches[i]; return o; }
            o += sizes[i];
        }
        *pitch = 0;
        return id == -1 ? o : -1;
    }
    int64_t at(int id) const { int p; return extra(id, &p); }
};

int check_cfg(const nnr_cfg* c) {      // nnr_frozen.h's refusals, in its order
    if (!c || c->n_rays <= 0 || c->n_samples <= 0) return NNR_E_BADCFG;
    if (c->hidden != 128 && c->hidden != 256) return NNR_E_UNSUPPORTED;
    if (c->n_samples > 1024) return NNR_E_UNSUPPORTED;
    constexpr uint32_t need = NNR_F_TRAIN | NNR_F_SPLIT3 | NNR_F_SPLIT2;
    if ((c->flags & NNR_F_BF16) || (c->flags & need) != need) return NNR_E_UNSUPPORTED;
    if (!SparseWs(c).ok) return NNR_E_UNSUPPORTED;      // (the list's indices are int32)
    return NNR_OK;
}

float* frozen_plane(const nnr_cfg* cfg, float* ws, int p) { return ws + nnr_frozen_ws_plane(cfg, p, nullptr); }

}  // namespace frozen_sparse_detail

extern "C" {

size_t nnr_frozen_sparse_workspace_floats(const nnr_cfg* cfg) {
    return frozen_sparse_detail::check_cfg(cfg) == NNR_OK ? (size_t)frozen_sparse_detail::SparseWs(cfg).at(-1) : 0;
}

int64_t nnr_frozen_sparse_ws_plane(const nnr_cfg* cfg, int pl, int32_t* pitch_out) {
    if (frozen_sparse_detail::check_cfg(cfg) != NNR_OK) return -1;
    if (pl >= NNR_FS_LIVE) {
        int pitch = 0;
        const int64_t o = frozen_sparse_detail::SparseWs(cfg).extra(pl, &pitch);
        if (pitch_out) *pitch_out = pitch;
        return o;
    }
    return nnr_frozen_ws_plane(cfg, pl, pitch_out);
}

int nnr_frozen_sparse_fwd(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo,
                          const float* z_hi, const float* jitter, const float grid_lo[3], const float grid_inv_step[3],
                          const int32_t grid_dims[3], const uint32_t* bits, const float* packed, float* rgb, float* dist, float* opt_alpha,
                          float* opt_z, int32_t* opt_count, int32_t* opt_live, int32_t* opt_n_live, float* ws, void* stream) {
    int rc = frozen_sparse_detail::check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!pts_o || !pts_d || !view_d || !z_lo || !z_hi || !packed || !rgb || !dist || !ws) return NNR_E_BADCFG;      // (jitter and the opt_* may be null)
    if (!grid_lo || !grid_inv_step || !grid_dims || !bits) return NNR_E_BADCFG;
    for (int c = 0; c < 3; ++c) {
        if (grid_dims[c] < 1) return NNR_E_BADCFG;
        if (!std::isfinite(grid_lo[c]) || !std::isfinite(grid_inv_step[c]) || !(grid_inv_step[c] > 0.f)) return NNR_E_BADCFG;
    }
    const int64_t wx = ((int64_t)grid_dims[0] + 31) / 32;
    const int64_t rows = (int64_t)grid_dims[2] * grid_dims[1];      // < 2^62
    if (rows > INT32_MAX || rows * wx > INT32_MAX || rows * grid_dims[0] > INT32_MAX) return NNR_E_UNSUPPORTED;
    if (!frozen_sparse_detail::aligned(packed, 16) || !frozen_sparse_detail::aligned(ws, 16)) return NNR_E_ALIGN;
    for (const void* p : {(const void*)bits, (const void*)opt_count, (const void*)opt_live, (const void*)opt_n_live})
        if (!frozen_sparse_detail::aligned(p, 4)) return NNR_E_ALIGN;
    const frozen_sparse_detail::SparseWs w(cfg);
    int32_t* const iws = reinterpret_cast<int32_t*>(ws);
    const hipStream_t st = (hipStream_t)stream;

    FrozenSparseArgs f{};
    f.pts_o = pts_o; f.pts_d = pts_d; f.z_lo = z_lo; f.z_hi = z_hi; f.jitter = jitter; f.bits = bits;
    f.ws_out4 = frozen_sparse_detail::frozen_plane(cfg, ws, P_OUT4);
    f.ws_z = frozen_sparse_detail::frozen_plane(cfg, ws, P_Z);
    f.ws_dpts = frozen_sparse_detail::frozen_plane(cfg, ws, P_DPTS);
    f.ws_dview = frozen_sparse_detail::frozen_plane(cfg, ws, P_DVIEW);
    f.ray_mask = reinterpret_cast<uint32_t*>(iws + w.at(NNR_FS_RAY_MASK));
    f.ray_count = iws + w.at(NNR_FS_RAY_COUNT);
    f.ray_off = iws + w.at(NNR_FS_RAY_OFF);
    f.live = iws + w.at(NNR_FS_LIVE);
    f.n_live = iws + w.at(NNR_FS_N_LIVE);
    f.opt_count = opt_count; f.opt_live = opt_live; f.opt_n_live = opt_n_live;
    for (int c = 0; c < 3; ++c) { f.lo[c] = grid_lo[c]; f.inv_step[c] = grid_inv_step[c]; f.n[c] = grid_dims[c]; }
    f.wx = (int)wx;
    f.R = cfg->n_rays; f.N = cfg->n_samples;
    f.flags = cfg->flags;
    hipError_t e = launch_frozen_sparse_compact(f, st);
    if (e != hipSuccess) return launched(e);

    MlpFwdListArgs a{};
    a.pts_o = pts_o; a.pts_d = pts_d; a.view_d = view_d; a.z_lo = z_lo; a.z_hi = z_hi; a.jitter = jitter;
    a.packed = packed;
    a.ws_out4 = f.ws_out4;
    a.ws_z = f.ws_z;
    a.ws_xe = frozen_sparse_detail::frozen_plane(cfg, ws, P_XE);
    a.ws_xf = frozen_sparse_detail::frozen_plane(cfg, ws, P_XF);
    a.ws_mask = reinterpret_cast<uint32_t*>(frozen_sparse_detail::frozen_plane(cfg, ws, P_MASK));
    a.S = w.S; a.S_pad = w.S_pad; a.N = cfg->n_samples;
    a.chunks_per_ray = 0;
    a.flags = cfg->flags;
    a.live = f.live; a.n_live = f.n_live;
    e = cfg->hidden == 256 ? launch_mlp_fwd_frozen_list_variant<256>(a, st) : launch_mlp_fwd_frozen_list_variant<128>(a, st);
    if (e != hipSuccess) return launched(e);
    CompositeArgs c{};
    c.ws_out4 = f.ws_out4;
    c.ws_z = f.ws_z;
    c.R = cfg->n_rays; c.N = cfg->n_samples; c.flags = cfg->flags;
    c.rgb = rgb; c.dist = dist; c.opt_alpha = opt_alpha; c.opt_z = opt_z;
    return launched(launch_composite_fwd(c, st));
}

int nnr_frozen_sparse_bwd(const nnr_cfg* cfg, const float* packed, const float* d_rgb, const float* d_dist, float* d_pts_o, float* d_pts_d,
                          float* d_view, float* ws, void* stream) {
    int rc = frozen_sparse_detail::check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!packed || !d_rgb || !d_dist || !d_pts_o || !d_pts_d || !d_view || !ws) return NNR_E_BADCFG;
    if (!frozen_sparse_detail::aligned(packed, 16) || !frozen_sparse_detail::aligned(ws, 16)) return NNR_E_ALIGN;
    const frozen_sparse_detail::SparseWs w(cfg);
    int32_t* const iws = reinterpret_cast<int32_t*>(ws);
    const hipStream_t st = (hipStream_t)stream;
    CompositeArgs c{};
    c.ws_out4 = frozen_sparse_detail::frozen_plane(cfg, ws, P_OUT4);
    c.ws_z = frozen_sparse_detail::frozen_plane(cfg, ws, P_Z);
    c.ws_dout4 = frozen_sparse_detail::frozen_plane(cfg, ws, P_DOUT4);
    c.R = cfg->n_rays; c.N = cfg->n_samples; c.flags = cfg->flags;
    c.d_rgb = d_rgb; c.d_dist = d_dist;
    hipError_t e = launch_composite_bwd(c, st);
    if (e != hipSuccess) return launched(e);
    MlpDgradListArgs a{};
    a.packed = packed;
    a.ws_dout4 = c.ws_dout4;
    a.ws_xe = frozen_sparse_detail::frozen_plane(cfg, ws, P_XE);
    a.ws_xf = frozen_sparse_detail::frozen_plane(cfg, ws, P_XF);
    a.ws_mask = reinterpret_cast<const uint32_t*>(frozen_sparse_detail::frozen_plane(cfg, ws, P_MASK));
    a.ws_dpts = frozen_sparse_detail::frozen_plane(cfg, ws, P_DPTS);
    a.ws_dview = frozen_sparse_detail::frozen_plane(cfg, ws, P_DVIEW);
    a.S = w.S; a.S_pad = w.S_pad;
    a.chunks_per_ray = 0;
    a.live = iws + w.at(NNR_FS_LIVE); a.n_live = iws + w.at(NNR_FS_N_LIVE);
    e = cfg->hidden == 256 ? launch_mlp_dgrad_frozen_list_variant<256>(a, st) : launch_mlp_dgrad_frozen_list_variant<128>(a, st);
    if (e != hipSuccess) return launched(e);
    RayReduceArgs r{};
    r.ws_dpts = a.ws_dpts;
    r.ws_dview = a.ws_dview;
    r.ws_z = c.ws_z;
    r.d_pts_o = d_pts_o; r.d_pts_d = d_pts_d; r.d_view = d_view;
    r.R = cfg->n_rays; r.N = cfg->n_samples;
    return launched(launch_ray_reduce(r, st));
}

}  // extern "C"
