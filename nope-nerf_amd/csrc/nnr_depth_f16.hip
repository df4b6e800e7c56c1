// nnr_depth_f16.hip -- the rendered depth of a ray from the density alone, in one launch (include/nnr_fusion.h: nnr_render_depth; DESIGN.md
// section 11.2): ray in, (depth, acc) out, 8 bytes per ray and nothing per sample through HBM.  What the depth fusion of the geometry export
// needs of a render (model/geometry.py: render_depth_maps): no colour branch, no view direction, no rgb.  Two stages:
//   * the passes are propose_f16_kernel's (nnr_propose_f16.hip), on the density-only pass shared with the march, proposal, grid and bricks
//     kernels (nnr_density_setup_f16.inc, nnr_density_pass_f16.inc): one wave walks one ray's C samples in passes of 32, the workgroup four
//     rays; the depths and points are the forward kernel's (z = z_lo + (z_hi - z_lo) jitter, p = o + d z: the same expressions, which hipcc
//     compiles to one fused multiply-add each in both kernels -- the two agree bit for bit); lanes of half 0 leave the
//     sample's raw density and depth in the wave's LDS staging row (sized with kProposeMaxC).  Every pass runs for every wave: a wave past
//     the last ray repeats the last ray and stores nothing; samples j >= C of the last pass are clamped loads and are not staged.
//   * behind the last pass and one workgroup barrier each wave composites its own row, the compositor's arithmetic (nnr_composite.hip) on
//     contiguous runs: lane l owns samples [l per, l per + per), per = ceil(C / 64) <= 4.  alpha_i = sample_alpha (last delta 1e10, as the
//     proposal kernel calls it), left in place of the staged raw density; T_i = prod_{j<i} (1 - alpha_j + 1e-6): the lane's own product, a wave
//     product scan (wave_scan_mul), the lane's run again; w_i = alpha_i T_i; depth = sum w_i z_i, acc = sum w_i: the lane's run in order,
//     then the xor butterfly (wave_sum).  Every product and sum in a fixed order: bit-reproducible.  No atomics, no scratch.
// A sample is NaN where an activation left fp16's range (left_f16_range), where its point is not finite or where the raw density is NaN, as
// in the proposal kernel; a ray with a NaN alpha or z gets (NaN, NaN), and no other ray of its workgroup is touched.
// LDS: the weight ring (3 panels, 96 KB), the park area (32 KB), the tables, and the staging: 2 x 256 floats per wave (8 KB).
// The compositing row is this file's own text: nnr_resample_row.h belongs to the resample and proposal units.
//
// NNR_DEPTH_MEDIAN=1 compiles this text a second time as depth_median_f16_kernel (include/nnr_depth_median.h: nnr_render_depth_median;
// DESIGN.md section 11.4), a unit of its own: (depth, acc, q) per ray, q the depth at which the transmittance falls below a.level.  Without
// the define nothing here changes.  The passes and the first two columns are untouched; in the second loop of the epilogue a lane has the
// transmittance in front of and behind each sample of its run (the products the weights are made of): the first sample i of the run with
// T_{i+1} < level (a NaN never crosses) gives the lane's q = z_i + (z_next - z_i) ((T_i - level) / (T_i - T_{i+1})), z_next the depth of
// sample i + 1 (z_i behind the last), every operation rounded to fp32, one IEEE division.  Runs are contiguous and increase with the lane:
// one ballot, the lowest lane that crossed, its q broadcast.  No crossing: +inf, NaN where the row's product is NaN; a `bad` ray: NaN.
#include "nnr_trunk_f16.h"
#include "nnr_fusion_kernels.h"

#ifndef NNR_DEPTH_MEDIAN
#define NNR_DEPTH_MEDIAN 0
#endif

namespace nnr {

#if NNR_DEPTH_MEDIAN
#define NNR_DEPTH_KERNEL depth_median_f16_kernel
typedef DepthMedianArgs DepthKernelArgs;
#else
#define NNR_DEPTH_KERNEL depth_f16_kernel
typedef DepthArgs DepthKernelArgs;
#endif

template <int D>
__global__ __launch_bounds__(256, 1) void NNR_DEPTH_KERNEL(DepthKernelArgs a) {
    constexpr int kDensityExtraF4 = kWavesPerBlock * 2 * kProposeMaxC / 4;      // per wave the raw densities and the depths of its ray
#include "nnr_density_setup_f16.inc"
    const int C = a.C;
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

    // ---- sampling: the forward kernel's expressions, to the letter ----
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

    // ---- this wave's staged row is visible to all its lanes ----
    __syncthreads();
    const int per = (C + 63) >> 6;
    const int i0 = min(lane0 * per, C), i1 = min(i0 + per, C);
    float prod = 1.f;
    bool bad = false;
    for (int i = i0; i < i1; ++i) {
        const float raw = s_raw[i], zz = s_z[i];
        float unused;
        float al = sample_alpha(raw, i + 1 < C ? s_z[i + 1] - zz : 1e10f, i == C - 1, a.flags, unused);
        if (raw != raw) al = __uint_as_float(0x7fc00000u);
        bad = bad || (al != al) || (zz != zz);
        if (live) {
            if (a.opt_raw) a.opt_raw[(int64_t)ray * C + i] = raw;
            if (a.opt_z) a.opt_z[(int64_t)ray * C + i] = zz;
        }
        s_raw[i] = al;      // the lane's own run: read again below by this lane alone
        prod *= (1.f - al) + kEpsT;
    }
    bad = __any(bad) != 0;
    const float incl = wave_scan_mul(prod, lane0);
    float T = __shfl_up(incl, 1, 64);
    if (lane0 == 0) T = 1.f;
    float sd = 0.f, sw = 0.f;
#if NNR_DEPTH_MEDIAN
    bool crossed = false;      // this lane's run holds a crossing; q: of the first one
    float q = 0.f;
#endif
    for (int i = i0; i < i1; ++i) {
        const float al = s_raw[i];
        const float w = al * T;
        sd += w * s_z[i];
        sw += w;
#if NNR_DEPTH_MEDIAN
        const float T0 = T;
#endif
        T *= (1.f - al) + kEpsT;
#if NNR_DEPTH_MEDIAN
        if (!crossed && T < a.level) {      // (a NaN never crosses)
#pragma clang fp contract(off)      // (this block: every operation of q is rounded on its own)
            const float zm = s_z[i], zn = i + 1 < C ? s_z[i + 1] : zm;
            q = zm + (zn - zm) * ((T0 - a.level) / (T0 - T));
            crossed = true;
        }
#endif
    }
    sd = wave_sum(sd);
    sw = wave_sum(sw);
#if NNR_DEPTH_MEDIAN
    {   // the first crossing of the row is the lowest lane's that has one; without one the row's product (lane 63 ends with it) decides
        const uint64_t who = __ballot(crossed);
        const float Tc = __shfl(T, 63, 64);
        const float qc = __shfl(q, who ? __ffsll((unsigned long long)who) - 1 : 0, 64);
        q = who ? qc : (Tc == Tc ? __uint_as_float(0x7f800000u) : __uint_as_float(0x7fc00000u));
    }
    if (live && lane0 == 0) {
        const float qnan = __uint_as_float(0x7fc00000u);
        a.out[3 * (int64_t)ray] = bad ? qnan : sd;
        a.out[3 * (int64_t)ray + 1] = bad ? qnan : sw;
        a.out[3 * (int64_t)ray + 2] = bad ? qnan : q;
    }
#else
    if (live && lane0 == 0) {
        const float qnan = __uint_as_float(0x7fc00000u);
        a.out[2 * (int64_t)ray] = bad ? qnan : sd;
        a.out[2 * (int64_t)ray + 1] = bad ? qnan : sw;
    }
#endif
}

#if NNR_DEPTH_MEDIAN
hipError_t launch_render_depth_median(int D, const DepthMedianArgs& a, hipStream_t st) {
#else
hipError_t launch_render_depth(int D, const DepthArgs& a, hipStream_t st) {
#endif
    if (a.R <= 0 || a.C < 1 || a.C > kProposeMaxC) return hipErrorInvalidValue;
    dim3 grid(((uint32_t)a.R + kWavesPerBlock - 1) / kWavesPerBlock), block(256);
    if (D == 256) hipLaunchKernelGGL(NNR_DEPTH_KERNEL<256>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(NNR_DEPTH_KERNEL<128>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace nnr
