// nnr_mlp_fwd_f16.hip -- the fused NeRF MLP forward of nnr_mlp_fwd.hip with every fp32 product taken as three fp16 MFMA terms of two-term
// operands (NNR_F_SPLIT2, Layout<D, 3>; the arithmetic: nnr_split2.h).  Restates, per sample: model/rendering.py:184-195 (z, points, view dir)
// and model/official_nerf.py:60-96 (the MLP).  Same decomposition (one wave = 32 samples, ray mode / flat mode, weights through the DMA-fed
// LDS ring, every D-wide layer as two half-output passes with the epilogue of one pass hidden in the MFMA stream of the next), same planes,
// same outputs as the six-term kernel.  The kernel is its prologue (sampling, the two encodings and their stashes), the trunk on packed fp16 terms
// (nnr_trunk_f16.h, which says what differs from the six-term kernel; the occupancy march, nnr_march_f16.hip, shares it), the colour branch
// (nnr_colour_f16.inc, shared with the sparse render nnr_sparse_f16.hip) and the output.  The density head is summed inside the units of hidden 8 (the fp32 values exist only there).
// Roofline: the matrix pipe in fp16 (2.5 PFLOP/s dense): 3 x 528 000 MACs per sample executed.
// A third build beside inference and training (csrc/build.py: NNR_FWD_TRAIN=2), the FROZEN-FIELD forward mlp_fwd_frozen_f16_kernel: the
// training forward for a step that wants the ray gradients only.  It leaves what the input-gradient kernel reads -- the gate words, the two
// encoding planes, z and the outputs -- keeps the range guard, and neither stores the hidden and colour-hidden activations nor keeps the
// plane maxima: both exist for the weight gradient alone.  Its argument block carries null pointers for those planes (nnr_frozen_api.cpp);
// every store through them is compiled out (NNR_STASH_ACT, nnr_trunk_f16.h), none is guarded at run time.
// A fourth build (NNR_FWD_TRAIN=3), the LIST-DRIVEN frozen forward mlp_fwd_frozen_list_f16_kernel of the sparse frozen-field render
// (include/nnr_frozen_sparse.h): flat mode only, slot s of the COMPACTED order takes the sample live[min(s, n_live - 1)]
// of a device-built list.  P_XE, P_XF and P_MASK stay indexed by the compact chunk (private to this kernel and its input gradient); P_OUT4 is
// written at the sample's dense index; z is the compaction kernel's.  A slot past n_live stores nothing to P_OUT4; a workgroup whose first
// slot is past n_live returns before the weight stream starts.  A sample whose point is not finite comes out NaN (the other builds leave it
// to ReLU, which makes it finite): its ray is NaN, as in the sparse inference render.
#if defined(NNR_FWD_TRAIN) && NNR_FWD_TRAIN == 3
#define NNR_STASH_ACT false
#define NNR_FWD_KERNEL mlp_fwd_frozen_list_f16_kernel
#define NNR_FWD_ARGS MlpFwdListArgs
#define NNR_FWD_LIST 1
#elif defined(NNR_FWD_TRAIN) && NNR_FWD_TRAIN == 2
#define NNR_STASH_ACT false
#define NNR_FWD_KERNEL mlp_fwd_frozen_f16_kernel
#define NNR_FWD_ARGS MlpFwdArgs
#define NNR_FWD_LIST 0
#else
#define NNR_FWD_KERNEL mlp_fwd_f16_kernel
#define NNR_FWD_ARGS MlpFwdArgs
#define NNR_FWD_LIST 0
#endif
#include "nnr_trunk_f16.h"
#include "nnr_frozen_kernels.h"
#include "nnr_frozen_sparse_kernels.h"

namespace nnr {

static_assert(kTileActPlanes, "the activation planes of a three-term / two-term training workspace are tile-major");

template <int D, bool TRAIN>
__global__ __launch_bounds__(256, 1) void NNR_FWD_KERNEL(NNR_FWD_ARGS a) {
    constexpr bool STASH = NNR_STASH_ACT;      // the kernel stores the activation planes and keeps their maxima
    constexpr bool LIST = NNR_FWD_LIST;       // the samples come from a live list (the sparse frozen-field render)
    using L = Layout<D, 3>;
    using Pipe = Split2PipeT<false>;
    constexpr int kRingF4 = kNBuf * Pipe::F4;
    constexpr int DT = L::DT, HT = L::HT;
    const int lane0 = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;

    constexpr int kPark = kWavesPerBlock * 12 * 64;   // per wave 12 16-byte slots per lane: the packed terms of posenc (8) + direnc (4)
    __shared__ __attribute__((aligned(16))) f32x4 smem[kRingF4 + kPark + (L::table_floats + 3) / 4];
    float* const ltab = reinterpret_cast<float*>(smem + kRingF4 + kPark);
    for (int i = threadIdx.x; i < L::table_floats; i += 256) ltab[i] = a.packed[L::bias_base + i];
    __shared__ uint32_t wg_max[9];      // training: the workgroup's largest stashed value per activation plane P_XH1..8 (as integers: the values are >= 0); [8]: the position encoding's
    if (STASH && threadIdx.x < 9) wg_max[threadIdx.x] = 0;
    __syncthreads();   // before any DMA is in flight: the only full barrier in front of the passes
    int n_live = 0;
    if constexpr (LIST) {
        n_live = __builtin_amdgcn_readfirstlane(*list_n_live(a));
        if ((int)blockIdx.x * kBlockSamples >= n_live) return;      // workgroup-uniform, and no DMA is in flight yet
    }
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    Pipe pipe{reinterpret_cast<const f32x4*>(a.packed) + wave_u * (Pipe::PW * 64), smem, wave_u, lane0, L::fwd_panels};
    const int n_pass = LIST ? 1 : a.chunks_per_ray > 0 ? a.chunks_per_ray : 1;
    pipe.more = n_pass > 1;
    pipe.start();
    float cT = 1.f, cr = 0.f, cg = 0.f, cb = 0.f, cz = 0.f, cw = 0.f;      // fused compositing (inference, ray mode), carried across the chunks
#pragma unroll 1
    for (int pass = 0; pass < n_pass; ++pass) {
    int lane = lane0;      // opaque per pass: keeps lane-constant addresses from being hoisted out of the pass loop and spilled (nnr_mlp_fwd.hip)
    asm volatile("" : "+v"(lane));
    pipe.lane = lane;
    const int half = lane >> 5;
    f32x4* const park = smem + kRingF4 + wave * (12 * 64) + lane;
    // wave-uniform: every plane address below is (scalar block base of this chunk) + 16 bytes per lane
    const int col = lane & 31;
    const int64_t chunk_id = a.chunks_per_ray > 0 ? ((int64_t)blockIdx.x * kWavesPerBlock + wave_u) * n_pass + pass
                                                   : (int64_t)blockIdx.x * kWavesPerBlock + wave_u;
#if NNR_FWD_LIST      // (the preprocessor, not `if constexpr`: the other builds keep their text, and with it their listings, to the letter)
    const int slot = (int)chunk_id * kChunk + col;                                 // this lane's slot of the compacted order
    const bool in_list = slot < n_live;                                            // a slot past the list recomputes the list's last sample and stores nothing
    const int64_t s = list_live(a)[in_list ? slot : n_live - 1];                   // this lane's sample: its dense index
    const int64_t sc = s;
    const int ray = (int)sc / a.N;
    const int j = (int)sc - ray * a.N;
#define NNR_FWD_STORES in_list
#else
    const int64_t s = chunk_id * kChunk + col;                                     // this lane's sample
    const int64_t sc = s < a.S ? s : a.S - 1;                                      // clamp: padded samples recompute the last one
    const int ray = (int)(sc / a.N);
    const int j = (int)(sc - (int64_t)ray * a.N);
#define NNR_FWD_STORES s < a.S
#endif
    const int lane_off = 16 * lane;

    // ---- sampling (model/rendering.py:184-195).  Unfused mul/add to round exactly like the reference. ----
    float zlo = a.z_lo[j], zhi = a.z_hi[j];
    float z = zlo;
    if (a.jitter) z = __fadd_rn(zlo, __fmul_rn(__fsub_rn(zhi, zlo), a.jitter[sc]));
    const float* ro = a.pts_o + 3 * (int64_t)ray;
    const float* rd = a.pts_d + 3 * (int64_t)ray;
    const float* rv = a.view_d + 3 * (int64_t)ray;
    const float px = __fadd_rn(ro[0], __fmul_rn(rd[0], z));
    const float py = __fadd_rn(ro[1], __fmul_rn(rd[1], z));
    const float pz = __fadd_rn(ro[2], __fmul_rn(rd[2], z));
    const float vx = rv[0], vy = rv[1], vz = rv[2];
    const bool fuse = !TRAIN && a.fuse_rgb != nullptr;
#if NNR_FWD_LIST      // a sample whose point is not finite (outside every grid, hence live) is made NaN at the output, as in the sparse inference
                      // render and the depth kernel: ReLU would turn its NaN activations into zeros and the sample out finite
    const float kInfP = __uint_as_float(0x7f800000u);
    const bool finite_p = fabsf(px) < kInfP && fabsf(py) < kInfP && fabsf(pz) < kInfP;
#endif
#if !NNR_FWD_LIST      // (LIST: the compaction kernel wrote z of every sample, by the same expressions)
    if (half == 0 && s < a.S && !fuse) a.ws_z[s] = z;
#endif
    constexpr int HR = 16 * HT;              // registers of half a layer's outputs
    constexpr int NP = HR / 2;               // register pairs per half (the unit of hidden epilogue work)
    constexpr int HW = (HR + 31) / 32;       // mask words per half

    // ---- encodings, straight into fragment layout; split once, parked in LDS until their layers ----
    uint32_t eh[16], em[16];      // gamma_10(p): 63 -> 64 values = 16 pairs
    {
        float e[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) e[r] = enc_register(r, half, kPosReal, px, py, pz);
        if constexpr (TRAIN) {
            const char* const xe = reinterpret_cast<const char*>(a.ws_xe + chunk_id * (int64_t)((kPosPad / 8) * 256));
#pragma unroll
            for (int q = 0; q < 8; ++q) tile_store(xe, lane_off, q, f32x4{e[4 * q], e[4 * q + 1], e[4 * q + 2], e[4 * q + 3]});
        }
        if constexpr (STASH) {
            // the plane's largest magnitude (the weight gradient's two-term job against this plane scales by it: nnr_wgrad.hip wgrad_job_enc2): the
            // identity block's coordinates, or 1 (the sines and cosines)
            const float me = wave_max_f32(fmaxf(1.f, fmaxf(fabsf(px), fmaxf(fabsf(py), fabsf(pz)))));
            if (lane == 0) atomicMax(&wg_max[8], __float_as_uint(me));
        }
        split2_all(eh, em, [&](int r) { return e[r]; });
        float dirv[16];  // gamma_4(v): 27 -> 32
#pragma unroll
        for (int r = 0; r < 16; ++r) dirv[r] = enc_register(r, half, kDirReal, vx, vy, vz);
        if constexpr (TRAIN) {
            const char* const xf = reinterpret_cast<const char*>(a.ws_xf + chunk_id * (int64_t)((kDirPad / 8) * 256));
#pragma unroll
            for (int q = 0; q < 4; ++q) tile_store(xf, lane_off, q, f32x4{dirv[4 * q], dirv[4 * q + 1], dirv[4 * q + 2], dirv[4 * q + 3]});
        }
        uint32_t dh[8], dm[8];
        split2_all(dh, dm, [&](int r) { return dirv[r]; });
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            park[(8 + q) * 64] = __builtin_bit_cast(f32x4, u32x4{dh[4 * q], dh[4 * q + 1], dh[4 * q + 2], dh[4 * q + 3]});
            park[(10 + q) * 64] = __builtin_bit_cast(f32x4, u32x4{dm[4 * q], dm[4 * q + 1], dm[4 * q + 2], dm[4 * q + 3]});
        }
    }
    const float* bias = ltab - L::bias_base;   // index with L::bias_off(layer), L::wsig_off, L::wrgb_off, L::scale_off

    TrunkStash st{lane_off, nullptr, wg_max};
    if (TRAIN) st.mask_base = a.ws_mask + ((chunk_id * L::n_mask_layers) * 64 + lane) * L::mask_words;

    uint32_t ph[8 * DT], pm[8 * DT];      // the packed terms of the current layer input (pairs [0, NP): half A, [NP, 2 NP): half B), rewritten in place
    f32x16 accA[HT], accB[HT];           // halves A ([0,D/2)) and B ([D/2,D)) of the layer being computed
    float mx = 0.f;                      // running maximum of the activations the units make (training: of the current plane, reset per plane)
    float mxa = 0.f;                     // training: ... of all planes of this pass so far
    float sg0 = 0.f, sg1 = 0.f;          // density head: this lane's share of w_sigma . h8
    auto xh = [&](int hidden_idx /*0..7*/) -> const char* {      // block (this chunk, octet 0) of hidden layer hidden_idx + 1's activation plane
        if constexpr (!STASH) return nullptr;
        else return reinterpret_cast<const char*>(a.ws_xh + (int64_t)hidden_idx * a.S_pad * D + chunk_id * (int64_t)((D / 8) * 256));
    };

    auto p0 = [&](int part) { return L::fwd_panel0(part); };

    {
#include "nnr_trunk_f16.inc"
    }

    auto xg = [&]() -> const char* {      // block (this chunk, octet 0) of the colour-hidden activation plane
        if constexpr (!STASH) return nullptr;
        else return reinterpret_cast<const char*>(a.ws_xg + chunk_id * (int64_t)((D / 16) * 256));
    };
#include "nnr_colour_f16.inc"
    {
        const float* b = bias + L::bias_off(11);
        f32x4 o;
        o[0] = sigmoid_ref(rgbv[0] + b[0]);
        o[1] = sigmoid_ref(rgbv[1] + b[1]);
        o[2] = sigmoid_ref(rgbv[2] + b[2]);
        o[3] = sigma_raw;
        {   // a sample that saw an activation outside fp16's range (either of its two lanes) is made NaN here: the loss is NaN, the caller's
            // check fires (model/losses.py:204-205), an inference frame shows it
#if NNR_FWD_LIST
            const bool over = left_f16_range(TRAIN ? fmaxf(mxa, mx) : mx) || !finite_p;
#else
            const bool over = left_f16_range(TRAIN ? fmaxf(mxa, mx) : mx);
#endif
            const float qnan = __uint_as_float(0x7fc00000u);
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = over ? qnan : o[c];
        }
        if (!fuse) {
            if (half == 0 && NNR_FWD_STORES) *reinterpret_cast<f32x4*>(a.ws_out4 + 4 * s) = o;
        } else if constexpr (!TRAIN) {
            // model/rendering.py:119-132,145-147 for the 32 samples of this chunk, as in nnr_mlp_fwd.hip (= composite_fwd_kernel 64 at a time)
            const int jn = j + 1;
            float zn = 0.f;
            if (jn < a.N) {
                const float lo1 = a.z_lo[jn], hi1 = a.z_hi[jn];
                zn = a.jitter ? __fadd_rn(lo1, __fmul_rn(__fsub_rn(hi1, lo1), a.jitter[sc + 1])) : lo1;
            }
            float unused;
            const float alpha = half == 0 ? sample_alpha(o[3], jn < a.N ? zn - z : 1e10f, jn == a.N, a.flags, unused) : 0.f;
            const float incl = wave_scan_mul(half == 0 ? (1.f - alpha) + kEpsT : 1.f, lane);
            float excl = __shfl_up(incl, 1, 64);
            if (lane == 0) excl = 1.f;
            const float w = alpha * cT * excl;
            cT *= __shfl(incl, 31, 64);
            cr += w * o[0]; cg += w * o[1]; cb += w * o[2]; cz += w * z; cw += w;
            if (pass + 1 == n_pass) {
                const float sr = wave_sum(cr), sgn = wave_sum(cg), sb = wave_sum(cb), sz = wave_sum(cz), sw = wave_sum(cw);
                if (lane == 0) {
                    const float bg = (a.flags & kFlagWhiteBg) ? 1.f - sw : 0.f;
                    float* out = a.fuse_rgb + 3 * (int64_t)ray;
                    out[0] = sr + bg; out[1] = sgn + bg; out[2] = sb + bg;
                    a.fuse_dist[ray] = sz;
                }
            }
        }
    }
#undef NNR_FINISH
#undef NNR_FWD_STORES
    pipe.next_pass(pass + 2 < n_pass);
    }   // pass
    if constexpr (STASH) {      // the workgroup's maxima to the launch's table (NNR_F_SPLIT2: the weight-gradient kernel's scales)
        __syncthreads();
        if (a.plane_max != nullptr && threadIdx.x < 8) atomicMax(reinterpret_cast<uint32_t*>(a.plane_max) + threadIdx.x, wg_max[threadIdx.x]);
        if (a.plane_max != nullptr && threadIdx.x == 8) atomicMax(reinterpret_cast<uint32_t*>(a.plane_max) + 17, wg_max[8]);      // (kPlaneMaxEnc, nnr_wgrad.hip)
    }
}

// One (D, TRAIN) instantiation per translation unit (csrc/build.py: -DNNR_FWD_D=.. -DNNR_FWD_TRAIN=..), as for nnr_mlp_fwd.hip
#if defined(NNR_FWD_D) && NNR_FWD_TRAIN == 3
template <>
hipError_t launch_mlp_fwd_frozen_list_variant<NNR_FWD_D>(const MlpFwdListArgs& a, hipStream_t st) {
    dim3 grid((unsigned)(a.S_pad / kBlockSamples)), block(256);      // the dense grid: the host does not know n_live
    hipLaunchKernelGGL((mlp_fwd_frozen_list_f16_kernel<NNR_FWD_D, true>), grid, block, 0, st, a);
    return hipGetLastError();
}
#elif defined(NNR_FWD_D) && NNR_FWD_TRAIN == 2
template <>
hipError_t launch_mlp_fwd_frozen_variant<NNR_FWD_D>(const MlpFwdArgs& a, hipStream_t st) {
    dim3 grid = mlp_fwd_grid(a), block(256);
    hipLaunchKernelGGL((mlp_fwd_frozen_f16_kernel<NNR_FWD_D, true>), grid, block, 0, st, a);
    return hipGetLastError();
}
#elif defined(NNR_FWD_D)
template <>
hipError_t launch_mlp_fwd_variant<NNR_FWD_D, (NNR_FWD_TRAIN != 0), 3>(const MlpFwdArgs& a, hipStream_t st) {
    dim3 grid = mlp_fwd_grid(a), block(256);
    constexpr bool train = NNR_FWD_TRAIN != 0;
    prof_before(train ? PROF_FWD_TRAIN : PROF_FWD_INFER, st);
    hipLaunchKernelGGL((mlp_fwd_f16_kernel<NNR_FWD_D, train>), grid, block, 0, st, a);
    prof_after(train ? PROF_FWD_TRAIN : PROF_FWD_INFER, st);
    return hipGetLastError();
}
#endif

}  // namespace nnr
