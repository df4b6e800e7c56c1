// nnr_propose_f16.hip -- the proposal stage of hierarchical sampling in one launch (rendering.proposal: 'density'; include/nnr.h: nnr_propose;
// DESIGN.md section 10): ray in, the sorted row of C coarse and F fine depths out, nothing per sample through HBM.  Two stages:
//   * the passes are the density-only pass shared with march_f16_kernel and grid_f16_kernel (nnr_density_setup_f16.inc: LDS and the weight
//     stream, with this kernel's staging rows between park and tables; nnr_density_pass_f16.inc: position encoding, the eight trunk layers and
//     the density head in the two-term fp16 arithmetic), walked as the march's ray mode: one wave walks one ray's C coarse samples in passes
//     of 32 (the workgroup four rays).  The depths are the forward kernel's (nnr_mlp_fwd_f16.hip: z = z_lo + (z_hi - z_lo) jitter,
//     p = o + d z, rounded op by op).  Lanes of half 0 leave the
//     sample's raw density and depth in the wave's LDS staging row.  Every pass runs for every wave (the four waves share the weight stream
//     and its barriers): a wave past the last ray repeats the last ray and stores nothing; samples j >= C of the last pass are clamped loads
//     and are not staged.
//   * behind the last pass the alphas are made from the staged row with the compositor's own function (sample_alpha, nnr_device.h: under
//     NNR_F_DIST_ALPHA it needs z_{j+1}, which is in LDS by then), and nnr_resample's row code (nnr_resample_row.h) runs on them.
// LDS: the weight ring (3 panels, 96 KB), the park area (32 KB), the tables, and the staging: 2 x 256 floats per wave (8 KB).  The ring and
// the park are dead behind the last pass; behind one workgroup barrier the rows of the resampling stage (mm, cdf, fs, out: at most
// 2 x 256 + 768 + 1024 floats = 9 KB per wave) take the ring's place.
// A sample is NaN (alpha, and with it the ray's whole row) where an activation left fp16's range (left_f16_range), where its point is not
// finite (ReLU would turn the NaN products into zeros, as it does behind an overflow) or where the raw density is NaN (fmaxf(raw, 0) of
// NNR_F_RELU_SIGMA would drop it).  No atomics, every sum in a fixed order: bit-reproducible.
#include "nnr_trunk_f16.h"
#include "nnr_resample_row.h"

namespace nnr {

template <int D>
__global__ __launch_bounds__(256, 1) void propose_f16_kernel(ProposeArgs a) {
    constexpr int kDensityExtraF4 = kWavesPerBlock * 2 * kProposeMaxC / 4;      // per wave the raw densities and the depths of its ray
#include "nnr_density_setup_f16.inc"
    static_assert(kWavesPerBlock * (2 * kProposeMaxC + 2 * kResampleMaxN) <= kRingF4 * 4, "the rows of the resampling stage fit in the weight ring");
    const int C = a.C, F = a.F;
    const int n_pass = (C + kChunk - 1) / kChunk;
    pipe.more = n_pass > 1;
    pipe.start();

    const int wave_ray = blockIdx.x * kWavesPerBlock + wave_u;
    const bool live = wave_ray < a.R;
    const int ray = live ? wave_ray : a.R - 1;
    float* const s_raw = reinterpret_cast<float*>(smem + kRingF4 + kPark) + wave * (2 * kProposeMaxC);
    float* const s_z = s_raw + kProposeMaxC;

#pragma unroll 1
    for (int pass = 0; pass < n_pass; ++pass) {
    int lane = lane0;      // opaque per pass (nnr_mlp_fwd_f16.hip)
    asm volatile("" : "+v"(lane));
    pipe.lane = lane;
    const int half = lane >> 5;
    const int col = lane & 31;
    f32x4* const park = smem + kRingF4 + wave * (8 * 64) + lane;

    // ---- sampling, as the forward kernel's: unfused mul/add ----
    const int j = pass * kChunk + col;
    const int jc = j < C ? j : C - 1;
    const float zlo = a.z_lo[jc], zhi = a.z_hi[jc];
    float z = zlo;
    if (a.jitter) z = __fadd_rn(zlo, __fmul_rn(__fsub_rn(zhi, zlo), a.jitter[(int64_t)ray * C + jc]));
    const float* ro = a.pts_o + 3 * (int64_t)ray;
    const float* rd = a.pts_d + 3 * (int64_t)ray;
    const float px = __fadd_rn(ro[0], __fmul_rn(rd[0], z));
    const float py = __fadd_rn(ro[1], __fmul_rn(rd[1], z));
    const float pz = __fadd_rn(ro[2], __fmul_rn(rd[2], z));

#include "nnr_density_pass_f16.inc"
    const bool finite_p = fabsf(px) < __uint_as_float(0x7f800000u) && fabsf(py) < __uint_as_float(0x7f800000u) && fabsf(pz) < __uint_as_float(0x7f800000u);
    if (left_f16_range(mx) || !finite_p) raw = __uint_as_float(0x7fc00000u);
    if (half == 0 && j < C) {
        s_raw[j] = raw;
        s_z[j] = z;
    }
    pipe.next_pass(pass + 2 < n_pass);
    }   // pass

    // ---- the rows take the ring's place: every wave is done with the last panel (and this wave's staged row is visible to all its lanes) ----
    __syncthreads();
    const int Cp = (C + 3) & ~3, Fp = (F + 3) & ~3, Np = (C + F + 3) & ~3;
    float* const mm = reinterpret_cast<float*>(smem) + (size_t)wave * (2 * Cp + Fp + Np);
    float* const cdf = mm + Cp;
    float* const fs = cdf + Cp;
    float* const out = fs + Fp;
    bool bad = false;
    for (int i = lane0; i < C; i += 64) {
        const float raw = s_raw[i], zz = s_z[i];
        float unused;
        float al = sample_alpha(raw, i + 1 < C ? s_z[i + 1] - zz : 1e10f, i == C - 1, a.flags, unused);
        if (raw != raw) al = __uint_as_float(0x7fc00000u);
        bad = bad || (al != al) || (zz != zz);
        out[i] = al;
        if (live) {
            if (a.opt_alpha) a.opt_alpha[(int64_t)ray * C + i] = al;
            if (a.opt_z) a.opt_z[(int64_t)ray * C + i] = zz;
        }
    }
    bad = __any(bad) != 0;
    __syncthreads();
    resample_row(s_z, mm, cdf, fs, out, C, F, a.xi ? a.xi + (int64_t)ray * F : nullptr, a.z_all + (int64_t)ray * (C + F),
                 a.opt_fine ? a.opt_fine + (int64_t)ray * F : nullptr, lane0, live, bad);
}

hipError_t launch_propose(int D, const ProposeArgs& a, hipStream_t st) {
    if (a.R <= 0 || a.C < 3 || a.C > kProposeMaxC || a.F < 1 || a.C + a.F > kResampleMaxN) return hipErrorInvalidValue;
    dim3 grid((a.R + kWavesPerBlock - 1) / kWavesPerBlock), block(256);
    if (D == 256) hipLaunchKernelGGL(propose_f16_kernel<256>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(propose_f16_kernel<128>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace nnr
