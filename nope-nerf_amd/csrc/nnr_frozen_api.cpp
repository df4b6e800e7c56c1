// nnr_frozen_api.cpp -- the extern "C" entry points of include/nnr_frozen.h (the frozen-field render) and include/nnr_frozen_sparse.h (its
// sparse variant): the one layout of their workspaces, argument checking, marshalling into the training kernels' argument blocks and the
// sequencing of the launches.  A host unit of its own, as nnr_sparse_api.cpp is.  The two families are one forward tail and one backward: the
// sparse entry points run the compaction (nnr_frozen_sparse.hip) in front and hand the two MLP kernels its list, the dense ones hand them
// none.  Every error return is decided before any device work -- no pointer is dereferenced here except the host arrays of the grid -- and
// every call is asynchronous on the caller's stream.  No state: the last HIP error is nnr_api.cpp's (launched).
// The argument blocks are value-initialised and only the planes of the frozen workspace are filled in: ws_xh, ws_xg, ws_dh, ws_dg and
// plane_max stay NULL.  The kernels launched here are built without any store through them (nnr_frozen_kernels.h).
// With a list the two MLP kernels always run the flat decomposition (chunks_per_ray = 0) on the dense grid of S_pad / 128 workgroups; the
// compositor's forward and backward and the per-ray reduction run on the dense planes either way.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nnr_frozen_sparse.h"
#include "nnr_frozen_sparse_kernels.h"
#include "nnr_grid_check.h"
#include "nnr_layout.h"

using namespace nnr;

namespace {

bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }      // n a power of two; null passes

// The planes of the workspace in their order.  The eight frozen planes, floats per sample each: what the input-gradient kernel reads from
// the forward (gate words, both encodings), what the compositor and the per-ray reduction exchange with the two kernels, nothing else.
// Behind them, in the sparse workspace alone, the five int32 planes of the compaction.
struct Ws {
    static constexpr int kFrozen = 8, kSparse = 13;      // planes of the dense and of the sparse workspace
    int64_t S, S_pad, R;
    int D;
    explicit Ws(const nnr_cfg* c)
        : S((int64_t)c->n_rays * c->n_samples), S_pad((S + kBlockSamples - 1) / kBlockSamples * kBlockSamples), R(c->n_rays), D(c->hidden) {}
    // offset (4-byte words) of plane p among the first n, -1 if absent; p == -1: their total
    int64_t plane(int p, int* pitch, int n) const {
        const int ids[kSparse] = {P_OUT4, P_Z, P_DOUT4, P_DPTS, P_DVIEW, P_XE, P_XF, P_MASK,
                                  NNR_FS_LIVE, NNR_FS_RAY_OFF, NNR_FS_N_LIVE, NNR_FS_RAY_COUNT, NNR_FS_RAY_MASK};
        const int pitches[kSparse] = {4, 1, 4, 4, 4, kPosPad, kDirPad, 9 * 2 * (D / 64), 1, 1, 1, 1, kFrozenSparseMaskWords};
        const int64_t rows[kSparse] = {S_pad, S_pad, S_pad, S_pad, S_pad, S_pad, S_pad, S_pad, S_pad, R, 1, R, R};
        int64_t o = 0;
        for (int i = 0; i < n; ++i) {
            if (ids[i] == p) { *pitch = pitches[i]; return o; }
            o += rows[i] * pitches[i];
        }
        *pitch = 0;
        return p == -1 ? o : -1;
    }
    int64_t at(int p) const { int pitch; return plane(p, &pitch, kSparse); }      // (a plane's offset is the same in both workspaces)
};

// sparse: the live list's indices are int32, an extra refusal behind the shared ones
int check_cfg(const nnr_cfg* c, bool sparse) {
    if (!c || c->n_rays <= 0 || c->n_samples <= 0) return NNR_E_BADCFG;
    if (c->hidden != 128 && c->hidden != 256) return NNR_E_UNSUPPORTED;
    if (c->n_samples > 1024) return NNR_E_UNSUPPORTED;      // (the compositor's bound for a training cfg: nnr_api.cpp)
    constexpr uint32_t need = NNR_F_TRAIN | NNR_F_SPLIT3 | NNR_F_SPLIT2;
    if ((c->flags & NNR_F_BF16) || (c->flags & need) != need) return NNR_E_UNSUPPORTED;
    if (sparse && Ws(c).S_pad > INT32_MAX) return NNR_E_UNSUPPORTED;
    return NNR_OK;
}

size_t workspace_floats(const nnr_cfg* cfg, bool sparse) {
    int pitch;
    return check_cfg(cfg, sparse) == NNR_OK ? (size_t)Ws(cfg).plane(-1, &pitch, sparse ? Ws::kSparse : Ws::kFrozen) : 0;
}

int64_t ws_plane(const nnr_cfg* cfg, int pl, int32_t* pitch_out, bool sparse) {
    if (check_cfg(cfg, sparse) != NNR_OK) return -1;
    int pitch = 0;
    const int64_t o = Ws(cfg).plane(pl, &pitch, sparse ? Ws::kSparse : Ws::kFrozen);
    if (pitch_out) *pitch_out = pitch;
    return pl < 0 ? -1 : o;
}

// what the forward entry points check alike; jitter and the opt_* may be null
int check_fwd(const nnr_cfg* cfg, bool sparse, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo, const float* z_hi,
              const float* packed, const float* rgb, const float* dist, const float* ws) {
    const int rc = check_cfg(cfg, sparse);
    if (rc != NNR_OK) return rc;
    return (!pts_o || !pts_d || !view_d || !z_lo || !z_hi || !packed || !rgb || !dist || !ws) ? NNR_E_BADCFG : NNR_OK;
}

// the forward behind the checks (and behind the compaction, where there is a list): the MLP kernel, then the compositor
int fwd(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo, const float* z_hi, const float* jitter,
        const float* packed, float* rgb, float* dist, float* opt_alpha, float* opt_z, float* ws, const int32_t* live, const int32_t* n_live,
        hipStream_t st) {
    const Ws w(cfg);
    MlpFwdListArgs a{};
    a.pts_o = pts_o; a.pts_d = pts_d; a.view_d = view_d; a.z_lo = z_lo; a.z_hi = z_hi; a.jitter = jitter;
    a.packed = packed;
    a.ws_out4 = ws + w.at(P_OUT4);
    a.ws_z = ws + w.at(P_Z);
    a.ws_xe = ws + w.at(P_XE);
    a.ws_xf = ws + w.at(P_XF);
    a.ws_mask = reinterpret_cast<uint32_t*>(ws + w.at(P_MASK));
    a.S = w.S; a.S_pad = w.S_pad; a.N = cfg->n_samples;
    a.chunks_per_ray = live ? 0 : chunks_per_ray(cfg);
    a.flags = cfg->flags;
    a.live = live; a.n_live = n_live;
    const bool wide = cfg->hidden == 256;
    const hipError_t e = live ? (wide ? launch_mlp_fwd_frozen_list_variant<256>(a, st) : launch_mlp_fwd_frozen_list_variant<128>(a, st))
                              : (wide ? launch_mlp_fwd_frozen_variant<256>(a, st) : launch_mlp_fwd_frozen_variant<128>(a, st));
    if (e != hipSuccess) return launched(e);
    CompositeArgs c{};
    c.ws_out4 = a.ws_out4;
    c.ws_z = a.ws_z;
    c.R = cfg->n_rays; c.N = cfg->n_samples; c.flags = cfg->flags;
    c.rgb = rgb; c.dist = dist; c.opt_alpha = opt_alpha; c.opt_z = opt_z;
    return launched(launch_composite_fwd(c, st));
}

// the whole backward, checks included: compositor backward, input gradient (walking the list of the sparse workspace, or every sample), per-ray
// reduction
int bwd(const nnr_cfg* cfg, bool sparse, const float* packed, const float* d_rgb, const float* d_dist, float* d_pts_o, float* d_pts_d,
        float* d_view, float* ws, hipStream_t st) {
    const int rc = check_cfg(cfg, sparse);
    if (rc != NNR_OK) return rc;
    if (!packed || !d_rgb || !d_dist || !d_pts_o || !d_pts_d || !d_view || !ws) return NNR_E_BADCFG;
    if (!aligned(packed, 16) || !aligned(ws, 16)) return NNR_E_ALIGN;
    const Ws w(cfg);
    CompositeArgs c{};
    c.ws_out4 = ws + w.at(P_OUT4);
    c.ws_z = ws + w.at(P_Z);
    c.ws_dout4 = ws + w.at(P_DOUT4);
    c.R = cfg->n_rays; c.N = cfg->n_samples; c.flags = cfg->flags;
    c.d_rgb = d_rgb; c.d_dist = d_dist;
    hipError_t e = launch_composite_bwd(c, st);
    if (e != hipSuccess) return launched(e);
    MlpDgradListArgs a{};
    a.packed = packed;
    a.ws_dout4 = c.ws_dout4;
    a.ws_xe = ws + w.at(P_XE);
    a.ws_xf = ws + w.at(P_XF);
    a.ws_mask = reinterpret_cast<const uint32_t*>(ws + w.at(P_MASK));
    a.ws_dpts = ws + w.at(P_DPTS);
    a.ws_dview = ws + w.at(P_DVIEW);
    a.S = w.S; a.S_pad = w.S_pad;
    a.chunks_per_ray = sparse ? 0 : chunks_per_ray(cfg);
    const bool wide = cfg->hidden == 256;
    if (sparse) {
        const int32_t* const iws = reinterpret_cast<const int32_t*>(ws);
        a.live = iws + w.at(NNR_FS_LIVE); a.n_live = iws + w.at(NNR_FS_N_LIVE);
        e = wide ? launch_mlp_dgrad_frozen_list_variant<256>(a, st) : launch_mlp_dgrad_frozen_list_variant<128>(a, st);
    } else {
        e = wide ? launch_mlp_dgrad_frozen_variant<256>(a, st) : launch_mlp_dgrad_frozen_variant<128>(a, st);
    }
    if (e != hipSuccess) return launched(e);
    RayReduceArgs r{};
    r.ws_dpts = a.ws_dpts;
    r.ws_dview = a.ws_dview;
    r.ws_z = c.ws_z;
    r.d_pts_o = d_pts_o; r.d_pts_d = d_pts_d; r.d_view = d_view;
    r.R = cfg->n_rays; r.N = cfg->n_samples;
    return launched(launch_ray_reduce(r, st));
}

}  // namespace

extern "C" {

size_t nnr_frozen_workspace_floats(const nnr_cfg* cfg) { return workspace_floats(cfg, false); }
size_t nnr_frozen_sparse_workspace_floats(const nnr_cfg* cfg) { return workspace_floats(cfg, true); }

int64_t nnr_frozen_ws_plane(const nnr_cfg* cfg, int pl, int32_t* pitch_out) { return ws_plane(cfg, pl, pitch_out, false); }
int64_t nnr_frozen_sparse_ws_plane(const nnr_cfg* cfg, int pl, int32_t* pitch_out) { return ws_plane(cfg, pl, pitch_out, true); }

int nnr_frozen_fwd(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo, const float* z_hi,
                   const float* jitter, const float* packed, float* rgb, float* dist, float* opt_alpha, float* opt_z, float* ws, void* stream) {
    const int rc = check_fwd(cfg, false, pts_o, pts_d, view_d, z_lo, z_hi, packed, rgb, dist, ws);
    if (rc != NNR_OK) return rc;
    if (!aligned(packed, 16) || !aligned(ws, 16)) return NNR_E_ALIGN;
    return fwd(cfg, pts_o, pts_d, view_d, z_lo, z_hi, jitter, packed, rgb, dist, opt_alpha, opt_z, ws, nullptr, nullptr, (hipStream_t)stream);
}

int nnr_frozen_sparse_fwd(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo,
                          const float* z_hi, const float* jitter, const float grid_lo[3], const float grid_inv_step[3],
                          const int32_t grid_dims[3], const uint32_t* bits, const float* packed, float* rgb, float* dist, float* opt_alpha,
                          float* opt_z, int32_t* opt_count, int32_t* opt_live, int32_t* opt_n_live, float* ws, void* stream) {
    int rc = check_fwd(cfg, true, pts_o, pts_d, view_d, z_lo, z_hi, packed, rgb, dist, ws);
    if (rc != NNR_OK) return rc;
    if (!grid_lo || !grid_inv_step || !grid_dims || !bits) return NNR_E_BADCFG;
    int64_t wx;
    rc = check_grid(grid_lo, grid_inv_step, grid_dims, &wx);
    if (rc != NNR_OK) return rc;
    if (!aligned(packed, 16) || !aligned(ws, 16)) return NNR_E_ALIGN;
    for (const void* p : {(const void*)bits, (const void*)opt_count, (const void*)opt_live, (const void*)opt_n_live})
        if (!aligned(p, 4)) return NNR_E_ALIGN;
    const Ws w(cfg);
    int32_t* const iws = reinterpret_cast<int32_t*>(ws);
    const hipStream_t st = (hipStream_t)stream;

    FrozenSparseArgs f{};
    f.pts_o = pts_o; f.pts_d = pts_d; f.z_lo = z_lo; f.z_hi = z_hi; f.jitter = jitter; f.bits = bits;
    f.ws_out4 = ws + w.at(P_OUT4);
    f.ws_z = ws + w.at(P_Z);
    f.ws_dpts = ws + w.at(P_DPTS);
    f.ws_dview = ws + w.at(P_DVIEW);
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
    const hipError_t e = launch_frozen_sparse_compact(f, st);
    if (e != hipSuccess) return launched(e);
    return fwd(cfg, pts_o, pts_d, view_d, z_lo, z_hi, jitter, packed, rgb, dist, opt_alpha, opt_z, ws, f.live, f.n_live, st);
}

int nnr_frozen_bwd(const nnr_cfg* cfg, const float* packed, const float* d_rgb, const float* d_dist, float* d_pts_o, float* d_pts_d,
                   float* d_view, float* ws, void* stream) {
    return bwd(cfg, false, packed, d_rgb, d_dist, d_pts_o, d_pts_d, d_view, ws, (hipStream_t)stream);
}

int nnr_frozen_sparse_bwd(const nnr_cfg* cfg, const float* packed, const float* d_rgb, const float* d_dist, float* d_pts_o, float* d_pts_d,
                          float* d_view, float* ws, void* stream) {
    return bwd(cfg, true, packed, d_rgb, d_dist, d_pts_o, d_pts_d, d_view, ws, (hipStream_t)stream);
}

}  // extern "C"
