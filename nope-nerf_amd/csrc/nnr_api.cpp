// nnr_api.cpp -- the extern "C" surface of libnnr.so (include/nnr.h): argument checking, marshalling into the kernels' argument structs and
// kernel sequencing.  The weight-gradient planners and the workspace regions behind the planes live in nnr_wgrad_plan.h.  Every call is
// asynchronous on the caller's stream.  State: the process-constant plan knobs and the per-thread memo of the plan counts (nnr_wgrad_plan.h),
// the per-thread last HIP error, and the profiling state below.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/nnr.h"
#include "../../include/nnr_geometry.h"
#include "nnr_device.h"
#include "nnr_frozen_kernels.h"
#include "nnr_kernels.h"
#include "nnr_layout.h"
#include "nnr_wgrad_plan.h"

using namespace nnr;

static_assert(nnr::kPlaneMaxWsFloats == nnr::kPlaneMaxFloats, "the host planner's copy of the plane-maximum table's size (nnr_wgrad_plan.h) must equal nnr_kernels.h");

namespace {

thread_local int g_last_hip = 0;

bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }      // n a power of two; null passes

int check_cfg(const nnr_cfg* c) {
    if (!c || c->n_rays <= 0 || c->n_samples <= 0) return NNR_E_BADCFG;
    if (c->hidden != 128 && c->hidden != 256) return NNR_E_UNSUPPORTED;
    if ((c->flags & NNR_F_TRAIN) && c->n_samples > 1024) return NNR_E_UNSUPPORTED;
    return NNR_OK;
}

// what the density-only kernels (march, proposal, grid, bricks) share: width 128 / 256, two-term mode (which excludes NNR_F_BF16), not training
int check_density_cfg(const nnr_cfg* c) {
    return ((c->hidden != 128 && c->hidden != 256) || (c->flags & NNR_F_TRAIN) || !is_split2(c)) ? NNR_E_UNSUPPORTED : NNR_OK;
}

int64_t plane(const WsLayout& w, int id) {
    int pitch;
    return w.plane(id, &pitch);
}

size_t packed_floats(int D, int mode) {
    if (mode == 3) return D == 256 ? (size_t)Layout<256, 3>::packed_floats : (size_t)Layout<128, 3>::packed_floats;
    if (mode == 2) return D == 256 ? (size_t)Layout<256, 2>::packed_floats : (size_t)Layout<128, 2>::packed_floats;
    if (mode == 1) return D == 256 ? (size_t)Layout<256, 1>::packed_floats : (size_t)Layout<128, 1>::packed_floats;
    return D == 256 ? (size_t)Layout<256>::packed_floats : (size_t)Layout<128>::packed_floats;
}

// the 12 gradient tensors of a weight-gradient launch ([12], the merged matrix's scratch, is the caller's); false: one is null
template <class Args>
bool fill_grads(const nnr_param_grads* g, Args& a) {
    for (int i = 0; i < 12; ++i) {
        if (!g->weight[i] || !g->bias[i]) return false;
        a.gw[i] = g->weight[i];
        a.gb[i] = g->bias[i];
    }
    return true;
}

// what the compositor's forward and backward share
CompositeArgs composite_args(const nnr_cfg* cfg, float* ws) {
    const WsLayout w = ws_layout(cfg);
    CompositeArgs a{};
    a.ws_out4 = ws + plane(w, P_OUT4);
    a.ws_z = ws + plane(w, P_Z);
    a.R = cfg->n_rays; a.N = cfg->n_samples; a.flags = cfg->flags;
    return a;
}

}  // namespace

// the one launch-result path: what a launcher (or any HIP call) returned -> the entry point's return code.  Not file-local: the host unit of
// include/nnr_fusion.h (nnr_fusion_api.cpp) reports through it too, so that nnr_last_hip_error speaks for every entry point.
namespace nnr {
int launched(hipError_t e) {
    if (e == hipSuccess) return NNR_OK;
    g_last_hip = (int)e;
    return NNR_E_HIP;
}

// Ray mode of the two MLP kernels (nnr_mlp_fwd.hip): a wave walks the N / 32 chunks of ONE ray, a workgroup four rays.  Needs whole
// chunks per ray and whole workgroups; everything else runs the flat decomposition (same sample numbering, same planes).
// The bf16 kernels (nnr_mlp_fwd_bf16.hip) work on PAIRS of chunks: their unit is 64 samples.  Not file-local: the frozen-field entry
// points (nnr_frozen_api.cpp) decompose their launches by the same rule.
int chunks_per_ray(const nnr_cfg* c) {
    static const bool off = std::getenv("NNR_FLAT_GRID") != nullptr;    // experiments: force the flat decomposition
    const int unit = is_bf16(c) ? kBf16Tiles * kChunk : kChunk;         // samples a wave takes per pass
    const int waves = is_bf16(c) ? kBf16Waves : kWavesPerBlock;         // = rays per workgroup in ray mode
    return (!off && c->n_samples % unit == 0 && c->n_rays % waves == 0) ? c->n_samples / unit : 0;
}
}  // namespace nnr

// ---- in-step kernel timing -------------------------------------------------------------------------------------------------
// bench.py switches this on for its timed steps: every launch of a main MLP kernel is bracketed by two HIP events recorded on the
// launch stream, so the durations are those of the kernels INSIDE the training step (between the step's other kernels, at the clocks
// and cache state of the step), not of a kernel run back to back with itself.  One process, one stream at a time: plain globals.
namespace {
struct ProfState {
    bool on = false;
    int cap = 0;
    int n[nnr::PROF_KINDS] = {0, 0, 0, 0};
    std::vector<hipEvent_t> ev[nnr::PROF_KINDS][2];
} g_prof;
}  // namespace
namespace nnr {
void prof_before(int kind, hipStream_t st) {
    if (g_prof.on && g_prof.n[kind] < g_prof.cap) (void)hipEventRecord(g_prof.ev[kind][0][g_prof.n[kind]], st);
}
void prof_after(int kind, hipStream_t st) {
    if (g_prof.on && g_prof.n[kind] < g_prof.cap) (void)hipEventRecord(g_prof.ev[kind][1][g_prof.n[kind]++], st);
}
}  // namespace nnr


static_assert(nnr::kFlagDistAlpha == NNR_F_DIST_ALPHA && nnr::kFlagWhiteBg == NNR_F_WHITE_BG && nnr::kFlagReluSigma == NNR_F_RELU_SIGMA,
              "the device-side copies of the rendering switches (nnr_device.h) must equal include/nnr.h");

extern "C" {

int nnr_abi_version(void) { return NNR_ABI_VERSION; }

const char* nnr_strerror(int code) {
    switch (code) {
        case NNR_OK: return "ok";
        case NNR_E_BADCFG: return "bad configuration or null pointer";
        case NNR_E_UNSUPPORTED: return "unsupported configuration (hidden must be 128 or 256; N <= 1024 when training)";
        case NNR_E_ALIGN: return "pointer not 16-byte aligned";
        case NNR_E_HIP: return "HIP runtime error";
        default: return "unknown error";
    }
}

int nnr_last_hip_error(void) { return g_last_hip; }

int nnr_prof_begin(int32_t max_launches) {
    if (g_prof.on || max_launches <= 0 || max_launches > 4096) return NNR_E_BADCFG;
    for (int k = 0; k < nnr::PROF_KINDS; ++k) {
        g_prof.n[k] = 0;
        for (int s = 0; s < 2; ++s) {
            g_prof.ev[k][s].resize(max_launches);
            for (auto& e : g_prof.ev[k][s])
                if (hipEventCreate(&e) != hipSuccess) return NNR_E_HIP;
        }
    }
    g_prof.cap = max_launches;
    g_prof.on = true;
    return NNR_OK;
}

int nnr_prof_end(float* mean_ms4, int32_t* launches4) {
    if (!g_prof.on || !mean_ms4 || !launches4) return NNR_E_BADCFG;
    g_prof.on = false;
    int rc = NNR_OK;
    for (int k = 0; k < nnr::PROF_KINDS; ++k) {
        double sum = 0.0;
        for (int i = 0; i < g_prof.n[k]; ++i) {
            float ms = 0.f;
            if (hipEventSynchronize(g_prof.ev[k][1][i]) != hipSuccess || hipEventElapsedTime(&ms, g_prof.ev[k][0][i], g_prof.ev[k][1][i]) != hipSuccess)
                rc = NNR_E_HIP;
            sum += ms;
        }
        launches4[k] = g_prof.n[k];
        mean_ms4[k] = g_prof.n[k] ? (float)(sum / g_prof.n[k]) : 0.f;
        for (int s = 0; s < 2; ++s) {
            for (auto& e : g_prof.ev[k][s]) (void)hipEventDestroy(e);
            g_prof.ev[k][s].clear();
        }
    }
    return rc;
}

size_t nnr_packed_floats(const nnr_cfg* cfg) {
    if (check_cfg(cfg) != NNR_OK) return 0;
    return packed_floats(cfg->hidden, weight_mode(cfg));
}

size_t nnr_workspace_floats(const nnr_cfg* cfg) {
    return check_cfg(cfg) == NNR_OK ? (size_t)TrainWs(cfg).total : 0;
}

int64_t nnr_ws_plane(const nnr_cfg* cfg, int pl, int32_t* pitch_out) {
    if (check_cfg(cfg) != NNR_OK) return -1;
    int pitch = 0;
    const int64_t o = ws_layout(cfg).plane(pl, &pitch);
    if (pitch_out) *pitch_out = pitch;
    return pl < 0 ? -1 : o;
}

int nnr_ws_plane_layout(const nnr_cfg* cfg, int pl) {
    if (check_cfg(cfg) != NNR_OK) return -1;
    const WsLayout w = ws_layout(cfg);
    int pitch = 0;
    if (pl < 0 || w.plane(pl, &pitch) < 0) return -1;
    if (w.tiled(pl)) return 2;
    if (w.bf16 && ((pl >= P_XH1 && pl < P_XH1 + 8) || pl == P_XG || pl == P_XE16 || pl == P_XF16 || (pl >= P_DH1 && pl < P_DH1 + 8) || pl == P_DG)) return 1;
    return 0;
}

size_t nnr_plan_bytes(const nnr_cfg* cfg) {
    if (check_cfg(cfg) != NNR_OK) return 0;
    return is_bf16(cfg) ? plan_bytes(build_plan_bf16(cfg, process_knobs())) : plan_bytes(build_plan(cfg, process_knobs()));
}

int nnr_plan_counts(const nnr_cfg* cfg, int32_t* n_jobs, int32_t* n_waves) {
    int rc = check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    const PlanCounts n = plan_counts(cfg);
    if (n_jobs) *n_jobs = n.n_jobs;
    if (n_waves) *n_waves = is_bf16(cfg) ? 4 * n.n_waves_or_blocks : n.n_waves_or_blocks;   // bf16 mode: workgroup jobs, four waves per workgroup
    return NNR_OK;
}

int nnr_plan_build(const nnr_cfg* cfg, void* plan_host) {      // the blob: write_plan, nnr_wgrad_plan.h
    int rc = check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!plan_host) return NNR_E_BADCFG;
    if (is_bf16(cfg)) write_plan(build_plan_bf16(cfg, process_knobs()), plan_host);
    else write_plan(build_plan(cfg, process_knobs()), plan_host);
    return NNR_OK;
}

int nnr_pack_weights(const nnr_cfg* cfg, const nnr_params* p, float* packed, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!p || !packed) return NNR_E_BADCFG;
    if (!aligned(packed, 16)) return NNR_E_ALIGN;
    PackArgs a;
    for (int i = 0; i < 12; ++i) {
        if (!p->weight[i] || !p->bias[i]) return NNR_E_BADCFG;
        a.w[i] = p->weight[i];
        a.b[i] = p->bias[i];
    }
    a.packed = packed;
    return launched(launch_pack(cfg->hidden, a, weight_mode(cfg), (hipStream_t)stream));
}

// the forward MLP launch; fuse_rgb / fuse_dist != null: inference with the compositing in the kernel's epilogue (ray mode only)
static int mlp_fwd_impl(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo,
                        const float* z_hi, const float* jitter, const float* packed, float* ws, float* fuse_rgb, float* fuse_dist,
                        void* stream) {
    int rc = check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!pts_o || !pts_d || !view_d || !z_lo || !z_hi || !packed || !ws) return NNR_E_BADCFG;
    if (!aligned(packed, 16) || !aligned(ws, 16)) return NNR_E_ALIGN;
    const WsLayout w = ws_layout(cfg);
    MlpFwdArgs a{};
    a.pts_o = pts_o; a.pts_d = pts_d; a.view_d = view_d; a.z_lo = z_lo; a.z_hi = z_hi; a.jitter = jitter;
    a.packed = packed;
    a.ws_out4 = ws + plane(w, P_OUT4);
    a.ws_z = ws + plane(w, P_Z);
    if (w.train) {
        a.ws_xe = ws + plane(w, P_XE);
        a.ws_xh = ws + plane(w, P_XH1);
        a.ws_xf = ws + plane(w, P_XF);
        a.ws_xg = ws + plane(w, P_XG);
        if (w.bf16) {
            a.ws_xe16 = ws + plane(w, P_XE16);
            a.ws_xf16 = ws + plane(w, P_XF16);
            a.ws_pts = ws + plane(w, P_DPTS);      // the input-gradient kernel reads position / view direction here before it
            a.ws_view = ws + plane(w, P_DVIEW);    // writes their gradients to the same rows
        }
        a.ws_mask = reinterpret_cast<uint32_t*>(ws + plane(w, P_MASK));
        if (is_split2(cfg)) {      // the maxima start at zero in every training forward (the input-gradient kernel of the same step adds its planes)
            a.plane_max = ws + TrainWs(cfg).plane_max;
            hipError_t em = hipMemsetAsync(a.plane_max, 0, kPlaneMaxFloats * sizeof(float), (hipStream_t)stream);
            if (em != hipSuccess) return launched(em);
        }
    }
    a.S = w.S; a.S_pad = w.S_pad; a.N = cfg->n_samples;
    a.chunks_per_ray = chunks_per_ray(cfg);
    a.fuse_rgb = fuse_rgb; a.fuse_dist = fuse_dist; a.flags = cfg->flags;
    return launched(is_bf16(cfg) ? launch_mlp_fwd_bf16(cfg->hidden, a, w.train, (hipStream_t)stream)
                                : launch_mlp_fwd(cfg->hidden, a, w.train, (hipStream_t)stream, weight_mode(cfg)));
}

int nnr_mlp_fwd(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo,
                const float* z_hi, const float* jitter, const float* packed, float* ws, void* stream) {
    return mlp_fwd_impl(cfg, pts_o, pts_d, view_d, z_lo, z_hi, jitter, packed, ws, nullptr, nullptr, stream);
}

int nnr_composite_fwd(const nnr_cfg* cfg, float* rgb, float* dist, float* opt_alpha, float* opt_z, float* ws, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!rgb || !dist || !ws) return NNR_E_BADCFG;
    CompositeArgs a = composite_args(cfg, ws);
    a.rgb = rgb; a.dist = dist; a.opt_alpha = opt_alpha; a.opt_z = opt_z;
    return launched(launch_composite_fwd(a, (hipStream_t)stream));
}

int nnr_render_fwd(const nnr_cfg* cfg, const float* pts_o, const float* pts_d, const float* view_d, const float* z_lo,
                   const float* z_hi, const float* jitter, const float* packed, float* rgb, float* dist, float* opt_alpha,
                   float* opt_z, float* ws, void* stream) {
    // Inference without the per-sample outputs, whole chunks per ray: the forward kernel composites in its epilogue and writes 16
    // bytes per ray -- no per-sample (rgb, sigma, z) round trip through HBM, no second launch.
    static const bool no_fuse = std::getenv("NNR_NO_FUSED_COMPOSITE") != nullptr;     // experiments / A-B tests
    if (cfg && !(cfg->flags & NNR_F_TRAIN) && !opt_alpha && !opt_z && rgb && dist && !no_fuse && chunks_per_ray(cfg) > 0)
        return mlp_fwd_impl(cfg, pts_o, pts_d, view_d, z_lo, z_hi, jitter, packed, ws, rgb, dist, stream);
    int rc = nnr_mlp_fwd(cfg, pts_o, pts_d, view_d, z_lo, z_hi, jitter, packed, ws, stream);
    if (rc != NNR_OK) return rc;
    return nnr_composite_fwd(cfg, rgb, dist, opt_alpha, opt_z, ws, stream);
}

// the phong renderer's depth search: one march launch, n_secant secant launches, one launch that writes d (nnr_march_f16.hip)
int nnr_ray_march(const nnr_cfg* cfg, const float* ray_o, const float* ray_d, float radius, const float* t_table, int32_t n_secant,
                  const float* packed, float* state, float* d_out, void* stream) {
    if (!cfg || cfg->n_rays <= 0 || n_secant < 0) return NNR_E_BADCFG;
    if (check_density_cfg(cfg) != NNR_OK || cfg->n_samples < 2 || cfg->n_samples > 1024 || (cfg->flags & NNR_F_WHITE_BG)) return NNR_E_UNSUPPORTED;
    if (!ray_o || !ray_d || !t_table || !packed || !state || !d_out) return NNR_E_BADCFG;
    if (!aligned(packed, 16) || !aligned(state, 16)) return NNR_E_ALIGN;
    MarchArgs a{};
    a.ray_o = ray_o; a.ray_d = ray_d; a.t = t_table; a.packed = packed; a.state = state;
    a.radius = radius; a.R = cfg->n_rays; a.n_steps = cfg->n_samples;
    a.flags = cfg->flags & (NNR_F_RELU_SIGMA | NNR_F_DIST_ALPHA);
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e = launch_march(cfg->hidden, a, st);
    a.flat = 1;
    for (int i = 0; i < n_secant && e == hipSuccess; ++i) e = launch_march(cfg->hidden, a, st);
    if (e == hipSuccess) e = launch_march_finish(state, d_out, cfg->n_rays, st);
    return launched(e);
}

// hierarchical sampling: coarse alphas and depths -> the sorted union of the coarse depths and n_fine inverse-CDF samples (nnr_resample.hip)
int nnr_resample(int32_t n_rays, int32_t n_coarse, int32_t n_fine, const float* alpha, const float* z, const float* xi, float* z_all,
                 float* fine, void* stream) {
    if (n_rays <= 0 || n_coarse < 3 || n_fine < 1) return NNR_E_BADCFG;
    if ((int64_t)n_coarse + n_fine > 1024) return NNR_E_UNSUPPORTED;
    if (!alpha || !z || !z_all) return NNR_E_BADCFG;      // (xi and fine may be null)
    if (!aligned(alpha, 16) || !aligned(z, 16) || !aligned(xi, 16) || !aligned(z_all, 16) || !aligned(fine, 16)) return NNR_E_ALIGN;
    return launched(launch_resample(n_rays, n_coarse, n_fine, alpha, z, xi, z_all, fine, (hipStream_t)stream));
}

// the proposal stage of hierarchical sampling in one launch: coarse densities + the resampling row code (nnr_propose_f16.hip)
int nnr_propose(const nnr_cfg* cfg, int32_t n_fine, const float* pts_o, const float* pts_d, const float* z_lo, const float* z_hi,
                const float* jitter, const float* xi, const float* packed, float* z_all, float* opt_alpha, float* opt_z, float* opt_fine,
                void* stream) {
    if (!cfg || cfg->n_rays <= 0 || cfg->n_samples < 3 || n_fine < 1) return NNR_E_BADCFG;
    if (check_density_cfg(cfg) != NNR_OK || cfg->n_samples > kProposeMaxC || (int64_t)cfg->n_samples + n_fine > 1024) return NNR_E_UNSUPPORTED;
    if (!pts_o || !pts_d || !z_lo || !z_hi || !packed || !z_all) return NNR_E_BADCFG;      // (jitter, xi and the opt_* may be null)
    if (!aligned(packed, 16) || !aligned(z_all, 16)) return NNR_E_ALIGN;
    for (const void* p : {(const void*)pts_o, (const void*)pts_d, (const void*)z_lo, (const void*)z_hi, (const void*)jitter, (const void*)xi,
                          (const void*)opt_alpha, (const void*)opt_z, (const void*)opt_fine})
        if (!aligned(p, 4)) return NNR_E_ALIGN;
    ProposeArgs a{};
    a.pts_o = pts_o; a.pts_d = pts_d; a.z_lo = z_lo; a.z_hi = z_hi; a.jitter = jitter; a.xi = xi; a.packed = packed;
    a.z_all = z_all; a.opt_alpha = opt_alpha; a.opt_z = opt_z; a.opt_fine = opt_fine;
    a.R = cfg->n_rays; a.C = cfg->n_samples; a.F = n_fine;
    a.flags = cfg->flags & (NNR_F_RELU_SIGMA | NNR_F_DIST_ALPHA);
    return launched(launch_propose(cfg->hidden, a, (hipStream_t)stream));
}

// the raw density on a regular grid in one launch (nnr_grid_f16.hip); origin, step and dims are HOST arrays, everything is decided before any device work
int nnr_density_grid(const nnr_cfg* cfg, const float origin[3], const float step[3], const int32_t dims[3], const float* packed, float* out,
                     void* stream) {
    if (!cfg || !origin || !step || !dims || !packed || !out) return NNR_E_BADCFG;
    if (check_density_cfg(cfg) != NNR_OK) return NNR_E_UNSUPPORTED;
    for (int c = 0; c < 3; ++c)
        if (dims[c] < 1 || !std::isfinite(origin[c]) || !std::isfinite(step[c])) return NNR_E_BADCFG;
    int64_t V = 1;
    for (int c = 0; c < 3; ++c) {
        V *= dims[c];      // (three factors below 2^31 each could pass 2^63: checked per factor)
        if (V > INT32_MAX) return NNR_E_UNSUPPORTED;
    }
    if (cfg->n_rays != V || cfg->n_samples != 1) return NNR_E_BADCFG;
    if (!aligned(packed, 16) || !aligned(out, 4)) return NNR_E_ALIGN;
    GridArgs a{};
    a.packed = packed; a.out = out;
    for (int c = 0; c < 3; ++c) { a.origin[c] = origin[c]; a.step[c] = step[c]; }
    a.nx = (uint32_t)dims[0]; a.ny = (uint32_t)dims[1]; a.V = (uint32_t)V;
    return launched(launch_density_grid(cfg->hidden, a, (hipStream_t)stream));
}

// the raw density in a list of 8 x 8 x 8 bricks of a regular grid in one launch (nnr_bricks_f16.hip; include/nnr_geometry.h); origin and step are
// HOST arrays, `bricks` is on the device and is never read here: everything is decided before any device work
int nnr_density_bricks(const nnr_cfg* cfg, const float origin[3], const float step[3], const int32_t* bricks, int32_t n_bricks,
                       const float* packed, float* out, void* stream) {
    if (!cfg || !origin || !step || !bricks || !packed || !out || n_bricks < 1) return NNR_E_BADCFG;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(origin[c]) || !std::isfinite(step[c])) return NNR_E_BADCFG;
    const int64_t V = 512 * (int64_t)n_bricks;
    if (check_density_cfg(cfg) != NNR_OK || V > INT32_MAX) return NNR_E_UNSUPPORTED;
    if (cfg->n_rays != V || cfg->n_samples != 1) return NNR_E_BADCFG;
    if (!aligned(packed, 16) || !aligned(bricks, 4) || !aligned(out, 4)) return NNR_E_ALIGN;
    BricksArgs a{};
    a.packed = packed; a.bricks = bricks; a.out = out;
    for (int c = 0; c < 3; ++c) { a.origin[c] = origin[c]; a.step[c] = step[c]; }
    return launched(launch_density_bricks(cfg->hidden, a, n_bricks, (hipStream_t)stream));
}

int nnr_composite_bwd(const nnr_cfg* cfg, const float* d_rgb, const float* d_dist, float* ws, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!(cfg->flags & NNR_F_TRAIN) || !d_rgb || !d_dist || !ws) return NNR_E_BADCFG;
    CompositeArgs a = composite_args(cfg, ws);
    a.ws_dout4 = ws + plane(ws_layout(cfg), P_DOUT4);
    a.d_rgb = d_rgb; a.d_dist = d_dist;
    return launched(launch_composite_bwd(a, (hipStream_t)stream));
}

int nnr_mlp_dgrad(const nnr_cfg* cfg, const float* packed, float* ws, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!(cfg->flags & NNR_F_TRAIN) || !packed || !ws) return NNR_E_BADCFG;
    if (!aligned(packed, 16) || !aligned(ws, 16)) return NNR_E_ALIGN;
    const WsLayout w = ws_layout(cfg);
    MlpDgradArgs a{};
    a.packed = packed;
    a.ws_dout4 = ws + plane(w, P_DOUT4);
    a.ws_xe = ws + plane(w, P_XE);
    a.ws_xf = ws + plane(w, P_XF);
    a.ws_mask = reinterpret_cast<const uint32_t*>(ws + plane(w, P_MASK));
    a.ws_dh = ws + plane(w, P_DH1);
    a.ws_dg = ws + plane(w, P_DG);
    a.ws_dpts = ws + plane(w, P_DPTS);
    a.ws_dview = ws + plane(w, P_DVIEW);
    a.plane_max = is_split2(cfg) ? ws + TrainWs(cfg).plane_max : nullptr;
    a.S = w.S; a.S_pad = w.S_pad;
    a.chunks_per_ray = chunks_per_ray(cfg);
    return launched(is_bf16(cfg) ? launch_mlp_dgrad_bf16(cfg->hidden, a, (hipStream_t)stream)
                                : launch_mlp_dgrad(cfg->hidden, a, (hipStream_t)stream, weight_mode(cfg)));
}

int nnr_mlp_wgrad(const nnr_cfg* cfg, const float* packed, const nnr_param_grads* g, const void* plan, float* ws, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!(cfg->flags & NNR_F_TRAIN) || !packed || !g || !plan || !ws) return NNR_E_BADCFG;
    const WsLayout w = ws_layout(cfg);
    const TrainWs behind(cfg);
    const PlanCounts n = plan_counts(cfg);      // the counts that locate the tables in `plan` (memoised: no plan is built on a training loop's launch path)
    if (w.bf16) {
        WgradBArgs b{};
        if (!fill_grads(g, b)) return NNR_E_BADCFG;
        b.n_jobs = n.n_jobs; b.n_blocks = n.n_waves_or_blocks; b.n_outs = n.n_heads_or_outs;
        b.jobs = static_cast<const WgradJobB*>(plan);
        b.block_first = reinterpret_cast<const int32_t*>(b.jobs + b.n_jobs);
        b.outs = reinterpret_cast<const WgradOutB*>(b.block_first + b.n_blocks + 1);
        b.ws = ws;
        b.slots = ws + behind.slots;
        b.gw[kMergedLayer] = ws + behind.merged_w;
        b.gb[kMergedLayer] = ws + behind.merged_b;
        b.packed = packed;
        b.D = cfg->hidden;
        return launched(launch_wgrad_bf16(b, (hipStream_t)stream));
    }
    WgradArgs a{};
    if (!fill_grads(g, a)) return NNR_E_BADCFG;
    a.jobs = static_cast<const WgradJob*>(plan);
    a.ws = ws;
    for (int p = 0; p < 48; ++p) {
        int pitch = 0;
        a.plane_off[p] = w.plane(p, &pitch);
        a.plane_pitch[p] = pitch;
        a.plane_tile[p] = w.tiled(p) ? 1 : 0;
    }
    a.n_jobs = n.n_jobs; a.n_waves = n.n_waves_or_blocks; a.n_heads = n.n_heads_or_outs;
    a.wave_first = reinterpret_cast<const int32_t*>(a.jobs + a.n_jobs);
    a.heads = a.wave_first + a.n_waves + 2;      // behind the wave table and the count
    a.slots = ws + behind.slots;
    a.gw[kMergedLayer] = ws + behind.merged_w;
    a.gb[kMergedLayer] = ws + behind.merged_b;
    a.packed = packed;
    a.D = cfg->hidden;
    a.plane_max = behind.plane_max >= 0 ? ws + behind.plane_max : nullptr;
    a.bf16 = weight_mode(cfg);   // 0, 2 or 3 here (>= 2: the 4 x 4 tiles with six bf16 terms): locates the merge area of the packed buffer for the un-merge step
    {
        const int D = cfg->hidden;
        const int rows[13] = {D, D, D, D, D, D, D, D, 1, D, D / 2, 3, D / 2};   // outputs of the 12 nn.Linear + the merged colour-hidden matrix
        for (int l = 0; l < 13; ++l) a.bias_rows[l] = rows[l];
    }
    return launched(launch_wgrad(a, (hipStream_t)stream));
}

int nnr_ray_reduce(const nnr_cfg* cfg, float* d_pts_o, float* d_pts_d, float* d_view, float* ws, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != NNR_OK) return rc;
    if (!(cfg->flags & NNR_F_TRAIN) || !d_pts_o || !d_pts_d || !d_view || !ws) return NNR_E_BADCFG;
    const WsLayout w = ws_layout(cfg);
    RayReduceArgs a{};
    a.ws_dpts = ws + plane(w, P_DPTS);
    a.ws_dview = ws + plane(w, P_DVIEW);
    a.ws_z = ws + plane(w, P_Z);
    a.d_pts_o = d_pts_o; a.d_pts_d = d_pts_d; a.d_view = d_view;
    a.R = cfg->n_rays; a.N = cfg->n_samples;
    return launched(launch_ray_reduce(a, (hipStream_t)stream));
}

int nnr_render_bwd(const nnr_cfg* cfg, const float* packed, const float* d_rgb, const float* d_dist,
                   const nnr_param_grads* grads, float* d_pts_o, float* d_pts_d, float* d_view, const void* plan, float* ws,
                   void* stream) {
    int rc = nnr_composite_bwd(cfg, d_rgb, d_dist, ws, stream);
    if (rc != NNR_OK) return rc;
    rc = nnr_mlp_dgrad(cfg, packed, ws, stream);
    if (rc != NNR_OK) return rc;
    rc = nnr_mlp_wgrad(cfg, packed, grads, plan, ws, stream);
    if (rc != NNR_OK) return rc;
    return nnr_ray_reduce(cfg, d_pts_o, d_pts_d, d_view, ws, stream);
}

int nnr_se3_exp_fwd(const float* r_all, const float* t_all, int32_t idx, float* c2w, void* stream) {
    if (!r_all || !t_all || !c2w || idx < 0) return NNR_E_BADCFG;
    return launched(launch_se3_exp_fwd(r_all, t_all, idx, c2w, (hipStream_t)stream));
}
int nnr_se3_exp_bwd(const float* r_all, int32_t idx, int32_t n_cams, const float* d_c2w, float* d_r_all, float* d_t_all,
                    void* stream) {
    if (!r_all || !d_c2w || !d_r_all || !d_t_all || idx < 0 || idx >= n_cams) return NNR_E_BADCFG;
    return launched(launch_se3_exp_bwd(r_all, idx, n_cams, d_c2w, d_r_all, d_t_all, (hipStream_t)stream));
}
int nnr_inv4_fwd(const float* a, float* y, int32_t batch, void* stream) {
    if (!a || !y || batch <= 0) return NNR_E_BADCFG;
    return launched(launch_inv4(a, y, batch, (hipStream_t)stream));
}
int nnr_inv4_bwd(const float* y, const float* d_y, float* d_a, int32_t batch, void* stream) {
    if (!y || !d_y || !d_a || batch <= 0) return NNR_E_BADCFG;
    return launched(launch_inv4_bwd(y, d_y, d_a, batch, (hipStream_t)stream));
}
int nnr_ray_setup_fwd(const float* pixels, const float* depth, const float* K, const float* W, const float* S, int32_t n_rays,
                      int32_t normalise, int32_t use_dir, float* pts_o, float* dir, float* view, float* ray_norm, float* d_gt,
                      uint8_t* mask, void* stream) {
    if (!pixels || !K || !W || !S || !pts_o || !dir || !view || !ray_norm || !d_gt || !mask || n_rays <= 0) return NNR_E_BADCFG;
    RaySetupArgs a{};
    a.pixels = pixels; a.depth = depth; a.K = K; a.W = W; a.S = S;
    a.pts_o = pts_o; a.dir = dir; a.view = view; a.ray_norm = ray_norm; a.d_gt = d_gt; a.mask = mask;
    a.R = n_rays; a.normalise = normalise; a.use_dir = use_dir;
    return launched(launch_ray_setup_fwd(a, (hipStream_t)stream));
}
int nnr_ray_setup_bwd(const float* pixels, const float* depth, const float* K, const float* W, const float* S, int32_t n_rays,
                      int32_t normalise, int32_t use_dir, const float* g_pts_o, const float* g_dir, const float* g_view,
                      const float* g_ray_norm, const float* g_d_gt, float* d_depth, float* dK, float* dW, float* dS,
                      float* scratch, void* stream) {
    if (!pixels || !K || !W || !S || !dK || !dW || !dS || !scratch || n_rays <= 0) return NNR_E_BADCFG;
    RaySetupArgs a{};
    a.pixels = pixels; a.depth = depth; a.K = K; a.W = W; a.S = S;
    a.g_o = g_pts_o; a.g_dir = g_dir; a.g_view = g_view; a.g_norm = g_ray_norm; a.g_dgt = g_d_gt;
    a.g_depth = d_depth; a.acc = scratch; a.gK = dK; a.gW = dW; a.gS = dS;
    a.R = n_rays; a.normalise = normalise; a.use_dir = use_dir;
    return launched(launch_ray_setup_bwd(a, (hipStream_t)stream));
}
int nnr_adam_step(const nnr_adam_table* t, void* stream) {
    if (!t || t->n_tensors < 0 || t->n_tensors > NNR_ADAM_MAX_TENSORS) return NNR_E_BADCFG;
    if (t->block_first[0] != 0 || (t->flavour != NNR_ADAM_FUSED && t->flavour != NNR_ADAM_SINGLE)) return NNR_E_BADCFG;
    for (int i = 0; i < t->n_tensors; ++i) {
        if (!t->param[i] || !t->grad[i] || !t->exp_avg[i] || !t->exp_avg_sq[i] || !t->step_in[i] || !t->step_out[i] || t->numel[i] <= 0 ||
            t->step_in[i] == t->step_out[i])
            return NNR_E_BADCFG;
        if (t->flavour == NNR_ADAM_SINGLE && !(t->bc2_sqrt[i] > 0.0)) return NNR_E_BADCFG;
        if (t->block_first[i + 1] - t->block_first[i] != (int32_t)((t->numel[i] + 1023) / 1024)) return NNR_E_BADCFG;
    }
    return launched(launch_adam_multi(*t, (hipStream_t)stream));
}
// what the step front end's forward and backward share: the step's geometry and the eight input tables; false: a bad cfg or a null table
static bool step_fill(const nnr_step_cfg* c, const float* r_all, const float* t_all, const float* scales, const float* shifts, const float* K,
                      const float* S, const int64_t* ray_idx, const float* depth_img, nnr::StepRaysArgs& a) {
    if (!c || c->n_rays <= 0 || c->h < 2 || c->w < 2 || c->hd <= 0 || c->wd <= 0 || c->n_cams <= 0 || c->cam < 0 || c->cam >= c->n_cams)
        return false;
    a.R = c->n_rays; a.h = c->h; a.w = c->w; a.hd = c->hd; a.wd = c->wd; a.cam = c->cam; a.n_cams = c->n_cams;
    a.normalise = (c->flags & NNR_STEP_NORMALISE) != 0; a.use_dir = (c->flags & NNR_STEP_USE_DIR) != 0;
    a.shift_first = (c->flags & NNR_STEP_SHIFT_FIRST) != 0; a.fix_last_scale = (c->flags & NNR_STEP_FIX_LAST_SCALE) != 0;
    if (c->ref >= c->n_cams || c->ref == c->cam) return false;
    a.ref = c->ref < 0 ? -1 : c->ref;
    a.detach_ref = (c->flags & NNR_STEP_DETACH_REF) != 0;
    a.r_all = r_all; a.t_all = t_all; a.scales = scales; a.shifts = shifts; a.K = K; a.S = S; a.ray_idx = ray_idx; a.depth_img = depth_img;
    return r_all && t_all && scales && shifts && K && S && ray_idx && depth_img;
}
int nnr_step_rays_fwd(const nnr_step_cfg* cfg, const float* r_all, const float* t_all, const float* scales, const float* shifts,
                      const float* K, const float* S, const int64_t* ray_idx, const float* depth_img, const float* img, float* pts_o,
                      float* dir, float* view, float* ray_norm, float* d_gt, uint8_t* mask, float* rgb_gt, float* pixels, float* mats,
                      void* stream) {
    nnr::StepRaysArgs a{};
    if (!step_fill(cfg, r_all, t_all, scales, shifts, K, S, ray_idx, depth_img, a)) return NNR_E_BADCFG;
    if (!pts_o || !dir || !view || !ray_norm || !d_gt || !mask || !pixels || !mats || (img && !rgb_gt)) return NNR_E_BADCFG;
    a.img = img; a.pts_o = pts_o; a.dir = dir; a.view = view; a.ray_norm = ray_norm; a.d_gt = d_gt;
    a.mask = mask; a.rgb_gt = rgb_gt; a.pixels = pixels; a.mats = mats;
    return launched(launch_step_rays_fwd(a, (hipStream_t)stream));
}
int nnr_step_rays_bwd(const nnr_step_cfg* cfg, const float* r_all, const float* t_all, const float* scales, const float* shifts,
                      const float* K, const float* S, const int64_t* ray_idx, const float* depth_img, const float* g_pts_o,
                      const float* g_dir, const float* g_view, const float* g_ray_norm, const float* g_d_gt, const float* g_mats,
                      float* d_r, float* d_t, float* d_scales, float* d_shifts, float* scratch, void* stream) {
    nnr::StepRaysArgs a{};
    if (!step_fill(cfg, r_all, t_all, scales, shifts, K, S, ray_idx, depth_img, a)) return NNR_E_BADCFG;
    if (!d_r || !d_t || !d_scales || !d_shifts || !scratch) return NNR_E_BADCFG;
    a.g_mats = g_mats;
    a.bwd_scratch = scratch;
    a.g_o = g_pts_o; a.g_dir = g_dir; a.g_view = g_view; a.g_norm = g_ray_norm; a.g_dgt = g_d_gt;
    a.d_r = d_r; a.d_t = d_t; a.d_scales = d_scales; a.d_shifts = d_shifts;
    return launched(launch_step_rays_bwd(a, (hipStream_t)stream));
}
int nnr_depth_gather_affine_fwd(const float* depth_img, const int64_t* ray_idx, const float* scale, const float* shift, int32_t shift_first,
                                float* out, int32_t n_rays, int32_t h, int32_t w, int32_t hd, int32_t wd, void* stream) {
    if (!depth_img || !ray_idx || !scale || !shift || !out || n_rays <= 0 || h <= 0 || w <= 0 || hd <= 0 || wd <= 0) return NNR_E_BADCFG;
    return launched(launch_depth_gather_affine_fwd(depth_img, ray_idx, scale, shift, shift_first, out, n_rays, h, w, hd, wd, (hipStream_t)stream));
}
int nnr_depth_gather_affine_bwd(const float* g_out, const float* depth_img, const int64_t* ray_idx, const float* scale, const float* shift,
                                int32_t shift_first, float* g_scale_shift, int32_t n_rays, int32_t h, int32_t w, int32_t hd, int32_t wd,
                                void* stream) {
    if (!g_out || !depth_img || !ray_idx || !scale || !shift || !g_scale_shift || n_rays <= 0 || h <= 0 || w <= 0 || hd <= 0 || wd <= 0)
        return NNR_E_BADCFG;
    return launched(launch_depth_gather_affine_bwd(g_out, depth_img, ray_idx, scale, shift, shift_first, g_scale_shift, n_rays, h, w, hd, wd,
                                              (hipStream_t)stream));
}

int nnr_ndc_rays_fwd(const float* rays_o, const float* rays_d, const float* camera_mat, float near_plane, float* o_ndc, float* d_ndc,
                     int32_t n_rays, void* stream) {
    if (!rays_o || !rays_d || !camera_mat || !o_ndc || !d_ndc || n_rays <= 0) return NNR_E_BADCFG;
    return launched(launch_ndc_rays_fwd(rays_o, rays_d, camera_mat, near_plane, o_ndc, d_ndc, n_rays, (hipStream_t)stream));
}
int nnr_ndc_rays_bwd(const float* rays_o, const float* rays_d, const float* camera_mat, float near_plane, const float* g_o_ndc,
                     const float* g_d_ndc, float* g_rays_o, float* g_rays_d, int32_t n_rays, void* stream) {
    if (!rays_o || !rays_d || !camera_mat || !g_o_ndc || !g_d_ndc || !g_rays_o || !g_rays_d || n_rays <= 0) return NNR_E_BADCFG;
    return launched(launch_ndc_rays_bwd(rays_o, rays_d, camera_mat, near_plane, g_o_ndc, g_d_ndc, g_rays_o, g_rays_d, n_rays, (hipStream_t)stream));
}

int nnr_depth_gather_fwd(const float* depth_img, const int64_t* ray_idx, float* out, int32_t n_rays, int32_t h, int32_t w,
                         int32_t hd, int32_t wd, void* stream) {
    if (!depth_img || !ray_idx || !out || n_rays <= 0 || h <= 0 || w <= 0 || hd <= 0 || wd <= 0) return NNR_E_BADCFG;
    return launched(launch_depth_gather_fwd(depth_img, ray_idx, out, n_rays, h, w, hd, wd, (hipStream_t)stream));
}
int nnr_depth_gather_bwd(const float* g_out, const int64_t* ray_idx, float* g_img, int32_t n_rays, int32_t h, int32_t w,
                         int32_t hd, int32_t wd, void* stream) {
    if (!g_out || !ray_idx || !g_img || n_rays <= 0 || h <= 0 || w <= 0 || hd <= 0 || wd <= 0) return NNR_E_BADCFG;
    return launched(launch_depth_gather_bwd(g_out, ray_idx, g_img, n_rays, h, w, hd, wd, (hipStream_t)stream));
}
int nnr_render_loss(const float* rgb, const float* rgb_gt, const float* dist, const float* d_gt, const uint8_t* mask,
                    int32_t n_rays, float r_total, float m_total, float w_rgb, float w_depth, int32_t rgb_l2, int32_t ndc,
                    int32_t detach_gt, const float* m_total_dev, float* out5, float* g_rgb, float* g_dist, float* g_d_gt,
                    void* stream) {
    if (!rgb || !rgb_gt || !dist || !d_gt || !mask || !out5 || !g_rgb || !g_dist || !g_d_gt || n_rays <= 0 || r_total <= 0.f)
        return NNR_E_BADCFG;
    LossArgs a{};
    a.rgb = rgb; a.rgb_gt = rgb_gt; a.dist = dist; a.d_gt = d_gt; a.mask = mask; a.out = out5;
    a.g_rgb = g_rgb; a.g_dist = g_dist; a.g_dgt = g_d_gt; a.R = n_rays; a.r_total = r_total; a.m_total = m_total;
    a.w_rgb = w_rgb; a.w_depth = w_depth; a.rgb_l2 = rgb_l2; a.ndc = ndc; a.detach_gt = detach_gt;
    a.m_total_dev = m_total_dev;
    return launched(launch_render_loss(a, (hipStream_t)stream));
}

int nnr_pixels_from_index(const int64_t* ray_idx, float* pixels, int32_t n_rays, int32_t h, int32_t w, void* stream) {
    if (!ray_idx || !pixels || n_rays <= 0 || h < 2 || w < 2) return NNR_E_BADCFG;
    return launched(launch_pixels_from_index(ray_idx, pixels, n_rays, h, w, (hipStream_t)stream));
}

int nnr_pc_nearest(const float* src, const float* dst, int32_t n_src, int32_t n_dst, int64_t* idx, float* dist, void* scratch,
                   void* stream) {
    if (!src || !dst || !idx || !dist || !scratch || n_src <= 0 || n_dst <= 0) return NNR_E_BADCFG;
    if (!aligned(scratch, 8)) return NNR_E_ALIGN;
    return launched(launch_pc_nearest(src, dst, n_src, n_dst, idx, dist, static_cast<unsigned long long*>(scratch), (hipStream_t)stream));
}

int nnr_pc_error_bwd(const float* src, const float* dst, const int64_t* idx, const float* dist, const float* g_loss, int32_t n_src,
                     int32_t n_dst, float* g_src, float* g_dst, void* stream) {
    if (!src || !dst || !idx || !dist || !g_loss || n_src <= 0 || n_dst <= 0 || (!g_src && !g_dst)) return NNR_E_BADCFG;
    return launched(launch_pc_error_bwd(src, dst, idx, dist, g_loss, n_src, n_dst, g_src, g_dst, (hipStream_t)stream));
}

size_t nnr_randperm_scratch_bytes(int32_t r) {
    const unsigned int cap = r > 0 ? nnr::randperm_capacity(r) : 0;
    return cap ? 8 + 20 * (size_t)cap : 0;   // header, u32 ranks, u64 candidates, u64 candidates in order
}

int nnr_randperm_prefix(const int64_t* keys, int64_t n, int32_t bits, int32_t r, uint64_t seed, uint64_t offset, int64_t* out,
                        void* scratch, void* stream) {
    int idx_bits = 1;
    while ((1ll << idx_bits) < n) ++idx_bits;
    if (!keys || !out || !scratch || n <= 0 || r <= 0 || r > n || bits < 1 || bits > 64) return NNR_E_BADCFG;
    if (bits + idx_bits > 64 || nnr::randperm_capacity(r) == 0 || n < 8 * (int64_t)r) return NNR_E_UNSUPPORTED;
    if (!aligned(scratch, 8)) return NNR_E_ALIGN;
    return launched(launch_randperm_prefix(keys, n, bits, r, seed, offset, out, static_cast<unsigned int*>(scratch), (hipStream_t)stream));
}

int nnr_uniform_rows(uint64_t seed, uint64_t offset, uint64_t threads, uint64_t first, uint64_t n, float* out, void* stream) {
    if (!out || threads == 0 || (threads & 255) != 0) return NNR_E_BADCFG;
    return launched(launch_uniform_rows(seed, offset, threads, first, n, out, (hipStream_t)stream));
}

namespace {
// workspace of the per-image losses, in floats; 8-byte items first so that they stay aligned
size_t aux_fill(const nnr_aux_cfg* c, float* ws, nnr::AuxArgs& a) {   // returns the workspace size in floats, 0 = bad cfg
    if (!c || c->hd <= 0 || c->wd <= 0 || c->hr < 2 || c->wr < 2 || c->hr > c->hd || c->wr > c->wd) return 0;
    const int64_t S = (int64_t)c->hr * c->wr;
    if (c->shard_lo < 0 || c->shard_hi < c->shard_lo || c->shard_hi > S) return 0;
    a.hd = c->hd; a.wd = c->wd; a.hr = c->hr; a.wr = c->wr; a.S = (int)S;
    a.s_lo = c->shard_lo;
    a.s_hi = (c->shard_lo == 0 && c->shard_hi == 0) ? (int)S : c->shard_hi;   // 0, 0 = every point (one GPU)
    a.nl = c->nearest_limit;
    a.flags = c->flags;
    a.w_pc = c->w_pc; a.w_rgbs = c->w_rgbs;
    if ((c->flags & NNR_AUX_MATS_GRAD) && (!(c->flags & NNR_AUX_AFFINE) || (c->flags & NNR_AUX_GRAD_K))) return 0;
    float* p = ws;
    auto take = [&](int64_t n) { float* r = p; p += n; return r; };
    a.keys = reinterpret_cast<unsigned long long*>(take(4 * S));
    a.idx_xy = reinterpret_cast<int64_t*>(take(2 * S));
    a.idx_yx = reinterpret_cast<int64_t*>(take(2 * S));
    a.gXq = reinterpret_cast<long long*>(take(6 * S));
    a.gYq = reinterpret_cast<long long*>(take(6 * S));
    a.X = take(3 * S); a.Y = take(3 * S);
    a.gxy = take(2 * S);
    if (c->flags & NNR_AUX_SSIM) {
        a.rgb1 = take(3 * S); a.rgb2 = take(3 * S);
        a.drgb = take(6 * S);
    }
    a.dist_xy = take(S); a.dist_yx = take(S);
    a.pflags = reinterpret_cast<uint32_t*>(take(S));
    a.acc = take(8);
    const int64_t nb = (S + 255) / 256;
    a.part_fwd = take(4 * nb);
    a.part_bwd = take(44 * nb);
    return (size_t)(p - ws);
}
}  // namespace

size_t nnr_aux_workspace_floats(const nnr_aux_cfg* cfg) {
    nnr::AuxArgs a{};
    static float origin;   // only differences of pointers derived from it are used
    return aux_fill(cfg, &origin, a);
}

// what the per-image losses' forward and backward share: the workspace carving, the inputs and the rules that tie them to cfg->flags.
// need_imgs: NNR_AUX_RGBS needs both images (the forward).  Every refusal but the last is NNR_E_BADCFG: the callers test their own pointers first.
static int aux_inputs(const nnr_aux_cfg* cfg, const float* d1_img, const float* d2_img, const float* img1r, const float* img2r, const float* K,
                      const float* Kinv, const float* rel, const float* scale2, const float* aff, bool need_imgs, float* ws, nnr::AuxArgs& a) {
    if (!ws || !aux_fill(cfg, ws, a)) return NNR_E_BADCFG;
    if (!d1_img || !d2_img || !K || !Kinv || !rel) return NNR_E_BADCFG;
    if (((cfg->flags & NNR_AUX_AFFINE) != 0) != (aff != nullptr)) return NNR_E_BADCFG;
    if (need_imgs && (cfg->flags & NNR_AUX_RGBS) && (!img1r || !img2r)) return NNR_E_BADCFG;
    if ((cfg->flags & NNR_AUX_SCALE_PCS) && !scale2) return NNR_E_BADCFG;
    a.aff = aff; a.shift_first = (cfg->flags & NNR_AUX_SHIFT_FIRST) != 0;
    a.d1_img = d1_img; a.d2_img = d2_img; a.img1r = img1r; a.img2r = img2r; a.K = K; a.Kinv = Kinv; a.rel = rel; a.scale2 = scale2;
    return aligned(ws, 8) ? NNR_OK : NNR_E_ALIGN;
}

int nnr_aux_terms_fwd(const nnr_aux_cfg* cfg, const float* d1_img, const float* d2_img, const float* img1r, const float* img2r,
                      const float* K, const float* Kinv, const float* rel, const float* scale2, const float* aff, float* out, float* ws,
                      void* stream) {
    nnr::AuxArgs a{};
    if (!out) return NNR_E_BADCFG;
    int rc = aux_inputs(cfg, d1_img, d2_img, img1r, img2r, K, Kinv, rel, scale2, aff, true, ws, a);
    if (rc != NNR_OK) return rc;
    a.out = out;
    return launched(launch_aux_fwd(a, (hipStream_t)stream));
}

int nnr_aux_terms_bwd(const nnr_aux_cfg* cfg, const float* d1_img, const float* d2_img, const float* img1r, const float* img2r,
                      const float* K, const float* Kinv, const float* rel, const float* scale2, const float* aff, const float* g_out,
                      float* g_d1_img, float* g_d2_img, float* g_rel_scale, float* ws, void* stream) {
    nnr::AuxArgs a{};
    if (!g_out || !g_rel_scale) return NNR_E_BADCFG;
    int rc = aux_inputs(cfg, d1_img, d2_img, img1r, img2r, K, Kinv, rel, scale2, aff, false, ws, a);
    if (rc != NNR_OK) return rc;
    a.g_out = g_out; a.g_d1_img = g_d1_img; a.g_d2_img = g_d2_img;
    return launched(launch_aux_bwd(a, g_rel_scale, (hipStream_t)stream));
}

}  // extern "C"
