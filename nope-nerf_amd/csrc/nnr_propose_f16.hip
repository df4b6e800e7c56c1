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
//
// NNR_PROPOSE_SPARSE=1 compiles this text a second time as propose_sparse_f16_kernel (include/nnr_propose_sparse.h: nnr_propose_sparse;
// DESIGN.md section 12.2), a unit of its own: the same passes and the same row code behind the compaction prologue of sparse_f16_kernel
// (nnr_sparse_f16.hip).  Without the define nothing here changes.
//   * prologue, in front of the setup (whose workgroup barrier, the one in front of the weight stream, then covers the tables AND the four
//     lists: there is no second one): lane l takes the samples j = l + 64 k, makes z_j and p_j with the expressions of the passes, looks the
//     cell up (sparse_cell, nnr_cell_rule.h: fp32, a NaN is outside) and reads the cell's bit with a plain vector load.  A sample is live
//     iff it is outside the grid or its bit is set.  Ballot and popcount compact the live j in increasing order into the wave's LDS list,
//     the count beside it.  The lane keeps z_j (staged for EVERY j < C once the setup has carved LDS up: the neighbours' deltas, the CDF
//     edges and the merged row need a culled sample's depth too) and a bit per round: whether its sample is live.
//   * n_pass = the largest ceil(n_live / 32) of the four waves, workgroup-uniform, before pipe.start().  A workgroup without a live sample
//     starts no DMA and runs no pass.
//   * passes: lane `col` takes j = list[32 pass + col]; a slot past n_live takes a clamped index, is computed like any other and is not
//     staged.
//   * behind the last pass a live sample's alpha is the dense kernel's (the delta to the next sample of the ORIGINAL row, the NaN rules
//     above); a culled sample's is 0.0f BY SELECT on the lane's liveness bit, whatever the flags (also the closing sample of
//     NNR_F_DIST_ALPHA): its staged density is never read, liveness is never encoded in a density.  resample_row runs on the full row.
// A culled sample is not evaluated and so cannot make its ray NaN: the one intended difference from the dense kernel.
// LDS: the dense kernel's + 4 x 256 bytes of lists + 4 counts.
//
// NNR_PROPOSE_SPARSE=1 with NNR_PROPOSE_DEPTH=1 compiles this text a third time as depth_sparse_f16_kernel (include/nnr_depth_sparse.h:
// nnr_render_depth_sparse), a unit of its own: the rendered depth of a ray, (depth, acc), from the live samples alone,
// stopped per workgroup once its rays are opaque -- to sparse_stop_f16_kernel (nnr_sparse_f16.hip under NNR_SPARSE_STOP=1) what depth_f16_kernel
// is to the inference forward: no colour branch, no view direction, 8 bytes out per ray.  Without the second define nothing here changes;
// the second without the first is an error.
//   * prologue and pass count: the sparse proposal's, without the per-lane depths and liveness bits (no row is staged: the staging rows
//     keep their place in the LDS map and are not touched).
//   * passes: the sparse proposal's (the same list, the same sampling, the same NaN rule); a live evaluated sample's raw density is the dense
//     depth kernel's bit for bit.
//   * the resampling stage is absent.  Behind each pass stands the sparse render's per-pass compositing (nnr_sparse_f16.hip, the block behind
//     opt_out4) with `raw` in place of o[3] and the carries cT, cz, cw alone: the delta to the next sample of the ORIGINAL row (recomputed
//     from z_lo / z_hi / jitter), sample_alpha on half 0, wave_scan_mul of the counted factors, a dead slot's factor 1 and weight 0 by
//     select.  Those lines are restated here -- this file's own text, as nnr_depth_f16.hip's compositing row is its own: nnr_sparse_f16.hip
//     shares no header with this unit -- and must stay that block's arithmetic: (depth, acc) are columns 3 and 4 of
//     nnr_render_sparse_stop bit for bit (tests/test_gpu_depth_sparse.py).
//   * the stop is sparse_stop_f16_kernel's to the letter: done = 32 (pass + 1) >= n_live || cT < t_min (a NaN carry is never done by
//     transmittance), s_done[pass & 1][wave], lgkmcnt(0), one raw s_barrier, every wave reads the four flags and leaves together;
//     vmcnt(0) on every way out of the loop.  t_min = 0: the comparison is never true, the full lists run.
//   * out[2 r] = wave_sum(cz), out[2 r + 1] = wave_sum(cw) from lane 0 of a wave that has a ray.
// LDS: the sparse proposal's map + 2 x 4 flags.
//
// NNR_PROPOSE_DEPTH=2 (with NNR_PROPOSE_SPARSE=1) compiles the depth build once more as depth_sparse_median_f16_kernel
// (include/nnr_depth_median.h: nnr_render_depth_median_sparse): (depth, acc, q), q the depth at which the ray's
// transmittance falls below a.level.  Everything under `#if NNR_PROPOSE_DEPTH` holds for both values; the lines of this build alone stand
// under `== 2`: a wave-uniform `found` and the carry q.  Per pass a counted lane has T in front of its sample, cT excl, and behind it,
// cT incl (cT: the carry of the earlier passes); the first counted lane with cT incl < level while `found` is still false gives
// q = z + (z_next - z) ((cT excl - level) / (cT excl - cT incl)), z_next the neighbour alpha's delta uses (z behind the last sample of
// the row), every operation rounded on its own (fp contract off), one IEEE division; list order is lane order: ballot, then readlane.  That
// block sits in front of the carry's update and outside the stop's barrier region; the stop rule, the flags, the barrier and the opt_*
// are the depth build's.  Once cT < level a crossing has been found, so t_min <= level (the host entry refuses more) stops no ray in
// front of its crossing: q is the t_min = 0 one bit for bit.  No crossing: +inf, NaN where the carry is NaN.  LDS: the depth build's.
#include "nnr_trunk_f16.h"
#include "nnr_resample_row.h"
#include "nnr_cell_rule.h"
#include "nnr_propose_sparse_kernels.h"
#include "nnr_depth_sparse_kernels.h"

#ifndef NNR_PROPOSE_SPARSE
#define NNR_PROPOSE_SPARSE 0
#endif
#ifndef NNR_PROPOSE_DEPTH
#define NNR_PROPOSE_DEPTH 0
#endif
#if NNR_PROPOSE_DEPTH && !NNR_PROPOSE_SPARSE
#error "NNR_PROPOSE_DEPTH=1 is a build of the sparse proposal's text: it needs NNR_PROPOSE_SPARSE=1"
#endif

namespace nnr {

#if NNR_PROPOSE_DEPTH == 2
#define NNR_PROPOSE_KERNEL depth_sparse_median_f16_kernel
typedef DepthSparseMedianArgs ProposeKernelArgs;
#elif NNR_PROPOSE_DEPTH
#define NNR_PROPOSE_KERNEL depth_sparse_f16_kernel
typedef DepthSparseArgs ProposeKernelArgs;
#elif NNR_PROPOSE_SPARSE
#define NNR_PROPOSE_KERNEL propose_sparse_f16_kernel
typedef ProposeSparseArgs ProposeKernelArgs;
#else
#define NNR_PROPOSE_KERNEL propose_f16_kernel
typedef ProposeArgs ProposeKernelArgs;
#endif

template <int D>
__global__ __launch_bounds__(256, 1) void NNR_PROPOSE_KERNEL(ProposeKernelArgs a) {
    constexpr int kDensityExtraF4 = kWavesPerBlock * 2 * kProposeMaxC / 4;      // per wave the raw densities and the depths of its ray
#if NNR_PROPOSE_SPARSE
    // ---- prologue: which samples are live (sparse_f16_kernel's, with the depths kept) ----
    constexpr int kRounds = kProposeMaxC / 64;
    __shared__ uint8_t s_list[kWavesPerBlock][kProposeMaxC];      // per wave: the live samples' indices, increasing
    __shared__ int s_cnt[kWavesPerBlock];                         // per wave: how many
    int n_live = 0;
#if NNR_PROPOSE_DEPTH
    __shared__ int s_done[2][kWavesPerBlock];                     // per pass parity and wave: done after that pass (sparse_stop_f16_kernel's)
#else
    uint32_t live_bits = 0;      // bit k: this lane's sample lane + 64 k is live
    float zk[kRounds];           // the depth of this lane's sample lane + 64 k
#endif
    {
        const int pl = threadIdx.x & 63, pw = threadIdx.x >> 6;
        const int p_ray_u = blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(pw);
        const bool p_has = p_ray_u < a.R;
        const int p_ray = p_has ? p_ray_u : a.R - 1;
        const float* const ro = a.pts_o + 3 * (int64_t)p_ray;
        const float* const rd = a.pts_d + 3 * (int64_t)p_ray;
        const int64_t row0 = (int64_t)p_ray * a.C;
#pragma unroll
        for (int k = 0; k < kRounds; ++k) {
#if !NNR_PROPOSE_DEPTH
            zk[k] = 0.f;
#endif
            if (64 * k < a.C) {
                const int j = pl + 64 * k;
                const bool valid = j < a.C;
                const int jc = valid ? j : a.C - 1;
                const float zlo = a.z_lo[jc], zhi = a.z_hi[jc];
                float z = zlo;
                if (a.jitter) z = __fadd_rn(zlo, __fmul_rn(__fsub_rn(zhi, zlo), a.jitter[row0 + jc]));
                const float px = __fadd_rn(ro[0], __fmul_rn(rd[0], z));
                const float py = __fadd_rn(ro[1], __fmul_rn(rd[1], z));
                const float pz = __fadd_rn(ro[2], __fmul_rn(rd[2], z));
                int word, bit;
                const int cell = sparse_cell(a, px, py, pz, word, bit);
                bool lv = valid;
                if (cell >= 0) lv = valid && ((a.bits[word] >> bit) & 1u) != 0;
                const uint64_t m = __ballot(lv);
                const int pos = n_live + __popcll(m & ((1ull << pl) - 1ull));
                if (lv) s_list[pw][pos] = (uint8_t)j;
                if (valid && p_has && a.opt_cell) a.opt_cell[row0 + j] = cell;
                n_live += __popcll(m);
#if !NNR_PROPOSE_DEPTH
                live_bits |= lv ? 1u << k : 0u;
                zk[k] = z;
#endif
            }
        }
        n_live = __builtin_amdgcn_readfirstlane(n_live);
        if (pl == 0) {
            s_cnt[pw] = n_live;
            if (p_has && a.opt_count) a.opt_count[p_ray] = n_live;
        }
    }
#endif
#include "nnr_density_setup_f16.inc"
    static_assert(kWavesPerBlock * (2 * kProposeMaxC + 2 * kResampleMaxN) <= kRingF4 * 4, "the rows of the resampling stage fit in the weight ring");
#if NNR_PROPOSE_DEPTH
    const int C = a.C;
#else
    const int C = a.C, F = a.F;
#endif
#if NNR_PROPOSE_SPARSE
    int n_pass = 0;      // (behind the setup's barrier: the four counts are visible)
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) n_pass = max(n_pass, (s_cnt[w] + kChunk - 1) / kChunk);
    n_pass = __builtin_amdgcn_readfirstlane(n_pass);
    pipe.more = n_pass > 1;
    if (n_pass > 0) pipe.start();      // (no pass: no DMA is ever in flight)
#else
    const int n_pass = (C + kChunk - 1) / kChunk;
    pipe.more = n_pass > 1;
    pipe.start();
#endif

    const int wave_ray = blockIdx.x * kWavesPerBlock + wave_u;
    const bool live = wave_ray < a.R;
    const int ray = live ? wave_ray : a.R - 1;
#if NNR_PROPOSE_DEPTH
    float cT = 1.f, cz = 0.f, cw = 0.f;      // the compositing carries, across the passes
    int n_ran = 0;                           // P_g: the passes this workgroup ran
#if NNR_PROPOSE_DEPTH == 2
    bool found = false;                      // the ray's transmittance has fallen below a.level: the same value in every lane
    float q = 0.f;                           // the depth at which it did
#endif
#else
    float* const s_raw = reinterpret_cast<float*>(smem + kRingF4 + kPark) + wave * (2 * kProposeMaxC);
    float* const s_z = s_raw + kProposeMaxC;
#endif
#if NNR_PROPOSE_SPARSE && !NNR_PROPOSE_DEPTH
#pragma unroll
    for (int k = 0; k < kRounds; ++k)      // every depth of the row, culled or not (read behind the barrier that follows the passes)
        if (lane0 + 64 * k < C) s_z[lane0 + 64 * k] = zk[k];
#endif

#pragma unroll 1
    for (int pass = 0; pass < n_pass; ++pass) {
    int lane = lane0;      // opaque per pass (nnr_mlp_fwd_f16.hip)
    asm volatile("" : "+v"(lane));
    pipe.lane = lane;
    const int half = lane >> 5;
    const int col = lane & 31;
    f32x4* const park = smem + kRingF4 + wave * (8 * 64) + lane;

    // ---- sampling, as the forward kernel's: unfused mul/add ----
#if NNR_PROPOSE_SPARSE
    const int slot = pass * kChunk + col;
    const bool dead = slot >= n_live;      // a slot past the list: computed on a clamped index, not staged
    int jl = 0;
    if (n_live > 0) jl = s_list[wave][dead ? n_live - 1 : slot];
    const int j = jl < C ? jl : C - 1;
    const int jc = j;
#else
    const int j = pass * kChunk + col;
    const int jc = j < C ? j : C - 1;
#endif
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
#if NNR_PROPOSE_DEPTH
    {   // the sparse render's per-pass compositing (nnr_sparse_f16.hip), restated: raw for o[3], the carries cT, cz, cw alone
        const bool counted = half == 0 && !dead;
        const int64_t sc = (int64_t)ray * C + j;
        if (counted && live && a.opt_raw) a.opt_raw[sc] = raw;
        const int jn = j + 1;
        float zn = 0.f;
        if (jn < C) {
            const float lo1 = a.z_lo[jn], hi1 = a.z_hi[jn];
            zn = a.jitter ? __fadd_rn(lo1, __fmul_rn(__fsub_rn(hi1, lo1), a.jitter[sc + 1])) : lo1;
        }
        float unused;
        const float alpha = half == 0 ? sample_alpha(raw, jn < C ? zn - z : 1e10f, jn == C, a.flags, unused) : 0.f;
        const float incl = wave_scan_mul(counted ? (1.f - alpha) + kEpsT : 1.f, lane);      // by select: a dead slot's alpha may be NaN
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.f;
        const float w = counted ? alpha * cT * excl : 0.f;
#if NNR_PROPOSE_DEPTH == 2
        {   // the first counted lane behind which the transmittance is below the level: list order is lane order, ballot then readlane
#pragma clang fp contract(off)      // (this block: every operation of q is rounded on its own)
            const float T0 = cT * excl, T1 = cT * incl;
            const uint64_t who = __ballot(counted && T1 < a.level);      // (a NaN never crosses)
            if (!found && who) {      // wave-uniform
                const float ql = z + ((jn < C ? zn : z) - z) * ((T0 - a.level) / (T0 - T1));
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)who) - 1);
                q = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ql), src));
                found = true;
            }
        }
#endif
        cT *= __shfl(incl, 31, 64);
        if (counted) { cz += w * z; cw += w; }
    }
    pipe.next_pass(pass + 2 < n_pass);
    {   // the stop (sparse_stop_f16_kernel's): flags by pass parity, one barrier, the same four flags in every wave
        n_ran = pass + 1;
        const bool done = kChunk * (pass + 1) >= n_live || cT < a.t_min;      // (cT: the same value in every lane; NaN < t_min is false)
        if (lane0 == 0) s_done[pass & 1][wave] = done ? 1 : 0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the flag is written; the next pass's DMA stays in flight
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        int all = 1;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) all &= s_done[pass & 1][w];
        if (__builtin_amdgcn_readfirstlane(all)) break;
    }
    }   // pass
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // no DMA piece of this wave is in flight past here, stopped early or not
    if (live && lane0 == 0 && a.opt_passes) a.opt_passes[ray] = n_ran;
    {
        const float sz = wave_sum(cz), sw = wave_sum(cw);
#if NNR_PROPOSE_DEPTH == 2
        if (live && lane0 == 0) {      // no crossing: +inf, NaN where the carry is
            a.out[3 * (int64_t)ray] = sz;
            a.out[3 * (int64_t)ray + 1] = sw;
            a.out[3 * (int64_t)ray + 2] = found ? q : (cT == cT ? __uint_as_float(0x7f800000u) : __uint_as_float(0x7fc00000u));
        }
#else
        if (live && lane0 == 0) {
            a.out[2 * (int64_t)ray] = sz;
            a.out[2 * (int64_t)ray + 1] = sw;
        }
#endif
    }
}
#else      // ---- the proposal's staging and resampling stage ----
#if NNR_PROPOSE_SPARSE
    if (half == 0 && !dead) s_raw[j] = raw;      // (its depth is staged already)
#else
    if (half == 0 && j < C) {
        s_raw[j] = raw;
        s_z[j] = z;
    }
#endif
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
#if NNR_PROPOSE_SPARSE
    if (live && lane0 == 0 && a.opt_passes) a.opt_passes[ray] = n_pass;
#endif
    for (int i = lane0; i < C; i += 64) {
#if NNR_PROPOSE_SPARSE
        const bool lv = ((live_bits >> (i >> 6)) & 1u) != 0;      // sample i = lane0 + 64 k is this lane's sample of round k
        const float raw = lv ? s_raw[i] : 0.f, zz = s_z[i];       // (a culled sample's density was never staged)
#else
        const float raw = s_raw[i], zz = s_z[i];
#endif
        float unused;
        float al = sample_alpha(raw, i + 1 < C ? s_z[i + 1] - zz : 1e10f, i == C - 1, a.flags, unused);
        if (raw != raw) al = __uint_as_float(0x7fc00000u);
#if NNR_PROPOSE_SPARSE
        al = lv ? al : 0.0f;      // by select: whatever the flags made of a density of 0
#endif
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
#endif      // NNR_PROPOSE_DEPTH

#if NNR_PROPOSE_DEPTH
#if NNR_PROPOSE_DEPTH == 2
hipError_t launch_render_depth_sparse_median(int D, const DepthSparseMedianArgs& a, hipStream_t st) {
#else
hipError_t launch_render_depth_sparse(int D, const DepthSparseArgs& a, hipStream_t st) {
#endif
    if (a.R <= 0 || a.C < 1 || a.C > kProposeMaxC) return hipErrorInvalidValue;
#elif NNR_PROPOSE_SPARSE
hipError_t launch_propose_sparse(int D, const ProposeSparseArgs& a, hipStream_t st) {
#else
hipError_t launch_propose(int D, const ProposeArgs& a, hipStream_t st) {
#endif
#if !NNR_PROPOSE_DEPTH
    if (a.R <= 0 || a.C < 3 || a.C > kProposeMaxC || a.F < 1 || a.C + a.F > kResampleMaxN) return hipErrorInvalidValue;
#endif
    dim3 grid((a.R + kWavesPerBlock - 1) / kWavesPerBlock), block(256);
    if (D == 256) hipLaunchKernelGGL(NNR_PROPOSE_KERNEL<256>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(NNR_PROPOSE_KERNEL<128>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace nnr
