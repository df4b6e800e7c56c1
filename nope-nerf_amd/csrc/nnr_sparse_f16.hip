// nnr_sparse_f16.hip -- the sparse inference render (include/nnr_sparse.h: nnr_render_sparse): the inference forward's
// ray mode (nnr_mlp_fwd_f16.hip: one wave walks one ray in passes of 32 samples, the workgroup four rays, compositing in the epilogue) behind
// a compaction prologue that drops the samples an occupancy bitfield calls empty.  Two-term fp16 products only (Layout<D, 3>).
//   * prologue, before any pass: lane l takes the samples j = l + 64 k (C <= kProposeMaxC: at most four rounds), makes z_j and p_j with the
//     forward kernel's expressions, looks its cell up -- f_c = (p_c - lo_c) * inv_step_c, each operation rounded to fp32; inside iff
//     0 <= f_c < n_c on all three axes (a NaN fails: outside); i_c = (int) f_c -- and reads the cell's bit with a plain vector load.  A
//     sample is live iff it is outside the grid or its bit is set: the grid only ever says "known empty".  Ballot and popcount compact the
//     live j in increasing order into the wave's LDS list (uint8 entries, 256 bytes per wave, a count per wave beside them).  One
//     workgroup barrier (the one in front of the weight stream, shared with the table load); then n_pass = the largest ceil(n_live / 32) of
//     the four waves, workgroup-uniform, before the stream's first prefetch.  A workgroup without a live sample runs NO pass and starts no
//     DMA: its rays get the background.
//   * passes: lane `col` of both halves takes j = list[32 pass + col]; a slot past n_live is dead, takes a clamped index and is computed
//     like any other (the waves of a workgroup walk the weight stream together).  Trunk: nnr_trunk_f16.inc, TRAIN = false.  The colour
//     branch and the rgb head are the inference forward's text, nnr_colour_f16.inc.  A live sample's (r, g, b, raw) is the forward's bit
//     for bit, incl. the NaN of a sample that saw an activation outside fp16's range; a sample whose point is not finite is NaN (it is outside the
//     grid, hence live: its ray comes out NaN).
//   * compositing: the forward's fused epilogue on the compacted list.  alpha_j = sample_alpha(raw_j, z_{j+1} - z_j) with z_{j+1} the next
//     sample of the ORIGINAL list (the last delta 1e10): a live sample's alpha is its alpha in the dense render.  A culled sample is absent
//     from the product; a dead slot's factor is 1 and its weight 0 BY SELECT (its recomputed value may be NaN).  The carries run across the
//     passes; the sums are taken once behind the last pass, in the forward's order.  No atomics, every sum in a fixed order.
// A wave past the last ray repeats the last ray and stores nothing.
// LDS: the forward's (ring 3 panels, park 12 slots per lane, tables) + 4 x 256 bytes of lists + 4 counts.
//
// NNR_SPARSE_STOP=1 compiles this text a second time as sparse_stop_f16_kernel (include/nnr_sparse_stop.h: nnr_render_sparse_stop; DESIGN.md
// section 12.1), a unit of its own: the same prologue, passes and compositing, and behind the compositing of every pass a workgroup-uniform
// decision whether another pass is run.  A wave is DONE after pass p iff its list is exhausted (32 (p + 1) >= n_live) or its transmittance
// carry cT < t_min (fp32 <: a NaN carry is never done by transmittance).  Lane 0 of each wave writes that flag into s_done[p & 1][wave], one
// raw s_barrier follows (behind lgkmcnt(0) only: the first two panels of the next pass are in flight, and __syncthreads would drain them),
// every wave reads the four flags and the loop ends where all four are set.  The flags alternate between two rows by pass parity, so that a
// wave's write after pass p + 1 cannot land in the row a slower wave still reads for pass p.  A wave that is done by transmittance keeps
// compositing for as long as its workgroup runs: the waves walk the weight stream together.  A workgroup that stops before its list ends has
// the next pass's first two panels in flight (pipe.more was true during the pass): every wave waits for its own DMA pieces (vmcnt(0)) on the
// way out of the loop, on every path, since LDS goes back with the workgroup.  + 2 x 4 flags of LDS.  Without the define nothing here changes.
#include "nnr_trunk_f16.h"
#include "nnr_sparse_cell.h"
#include "nnr_sparse_kernels.h"

#ifndef NNR_SPARSE_STOP
#define NNR_SPARSE_STOP 0
#endif

namespace nnr {

#if NNR_SPARSE_STOP
#define NNR_SPARSE_KERNEL sparse_stop_f16_kernel
typedef SparseStopArgs SparseKernelArgs;
#else
#define NNR_SPARSE_KERNEL sparse_f16_kernel
typedef SparseArgs SparseKernelArgs;
#endif

template <int D>
__global__ __launch_bounds__(256, 1) void NNR_SPARSE_KERNEL(SparseKernelArgs a) {
    constexpr bool TRAIN = false;
    using L = Layout<D, 3>;
    using Pipe = Split2PipeT<false>;
    constexpr int kRingF4 = kNBuf * Pipe::F4;
    constexpr int DT = L::DT, HT = L::HT;
    const int lane0 = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int C = a.C;

    constexpr int kPark = kWavesPerBlock * 12 * 64;   // per wave 12 16-byte slots per lane: the packed terms of posenc (8) + direnc (4)
    __shared__ __attribute__((aligned(16))) f32x4 smem[kRingF4 + kPark + (L::table_floats + 3) / 4];
    __shared__ uint8_t s_list[kWavesPerBlock][kProposeMaxC];      // per wave: the live samples' indices, increasing
    __shared__ int s_cnt[kWavesPerBlock];                         // per wave: how many
#if NNR_SPARSE_STOP
    __shared__ int s_done[2][kWavesPerBlock];                     // per pass parity and wave: done after that pass
#endif
    float* const ltab = reinterpret_cast<float*>(smem + kRingF4 + kPark);
    for (int i = threadIdx.x; i < L::table_floats; i += 256) ltab[i] = a.packed[L::bias_base + i];

    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int wave_ray = blockIdx.x * kWavesPerBlock + wave_u;
    const bool has_ray = wave_ray < a.R;
    const int ray = has_ray ? wave_ray : a.R - 1;
    const float* const ro = a.pts_o + 3 * (int64_t)ray;
    const float* const rd = a.pts_d + 3 * (int64_t)ray;
    const float* const rv = a.view_d + 3 * (int64_t)ray;
    const int64_t row0 = (int64_t)ray * C;

    // ---- prologue: which samples are live ----
    int n_live = 0;
    for (int k = 0; 64 * k < C; ++k) {
        const int j = lane0 + 64 * k;
        const bool valid = j < C;
        const int jc = valid ? j : C - 1;
        const float zlo = a.z_lo[jc], zhi = a.z_hi[jc];
        float z = zlo;
        if (a.jitter) z = __fadd_rn(zlo, __fmul_rn(__fsub_rn(zhi, zlo), a.jitter[row0 + jc]));
        const float px = __fadd_rn(ro[0], __fmul_rn(rd[0], z));
        const float py = __fadd_rn(ro[1], __fmul_rn(rd[1], z));
        const float pz = __fadd_rn(ro[2], __fmul_rn(rd[2], z));
        int word, bit;
        const int cell = sparse_cell(a, px, py, pz, word, bit);
        bool live = valid;
        if (cell >= 0) live = valid && ((a.bits[word] >> bit) & 1u) != 0;
        const uint64_t m = __ballot(live);
        const int pos = n_live + __popcll(m & ((1ull << lane0) - 1ull));
        if (live) s_list[wave][pos] = (uint8_t)j;
        if (valid && has_ray && a.opt_cell) a.opt_cell[row0 + j] = cell;
        n_live += __popcll(m);
    }
    n_live = __builtin_amdgcn_readfirstlane(n_live);
    if (lane0 == 0) {
        s_cnt[wave] = n_live;
        if (has_ray && a.opt_count) a.opt_count[ray] = n_live;
    }
    __syncthreads();   // the tables and the four lists; before any DMA is in flight: the only full barrier in front of the passes
    int n_pass = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) n_pass = max(n_pass, (s_cnt[w] + kChunk - 1) / kChunk);
    n_pass = __builtin_amdgcn_readfirstlane(n_pass);

    Pipe pipe{reinterpret_cast<const f32x4*>(a.packed) + wave_u * (Pipe::PW * 64), smem, wave_u, lane0, L::fwd_panels};
    pipe.more = n_pass > 1;
    if (n_pass > 0) pipe.start();      // (no pass: no DMA is ever in flight)
    float cT = 1.f, cr = 0.f, cg = 0.f, cb = 0.f, cz = 0.f, cw = 0.f;      // the compositing carries, across the passes
#if NNR_SPARSE_STOP
    int n_ran = 0;      // P_g: the passes this workgroup ran
#endif
#pragma unroll 1
    for (int pass = 0; pass < n_pass; ++pass) {
    int lane = lane0;      // opaque per pass (nnr_mlp_fwd_f16.hip)
    asm volatile("" : "+v"(lane));
    pipe.lane = lane;
    const int half = lane >> 5;
    f32x4* const park = smem + kRingF4 + wave * (12 * 64) + lane;
    const int col = lane & 31;
    const int slot = pass * kChunk + col;
    const bool dead = slot >= n_live;      // a slot past the list: computed on a clamped index, absent from the product
    int j = 0;
    if (n_live > 0) j = s_list[wave][dead ? n_live - 1 : slot];
    j = j < C ? j : C - 1;
    const int64_t sc = row0 + j;
    const int lane_off = 16 * lane;

    // ---- sampling: the forward kernel's expressions, to the letter ----
    float zlo = a.z_lo[j], zhi = a.z_hi[j];
    float z = zlo;
    if (a.jitter) z = __fadd_rn(zlo, __fmul_rn(__fsub_rn(zhi, zlo), a.jitter[sc]));
    const float px = __fadd_rn(ro[0], __fmul_rn(rd[0], z));
    const float py = __fadd_rn(ro[1], __fmul_rn(rd[1], z));
    const float pz = __fadd_rn(ro[2], __fmul_rn(rd[2], z));
    const float vx = rv[0], vy = rv[1], vz = rv[2];
    constexpr int HR = 16 * HT;              // registers of half a layer's outputs
    constexpr int NP = HR / 2;               // register pairs per half
    constexpr int HW = (HR + 31) / 32;       // mask words per half

    // ---- encodings, straight into fragment layout; split once, parked in LDS until their layers ----
    uint32_t eh[16], em[16];      // gamma_10(p): 63 -> 64 values = 16 pairs
    {
        float e[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) e[r] = enc_register(r, half, kPosReal, px, py, pz);
        split2_all(eh, em, [&](int r) { return e[r]; });
        float dirv[16];  // gamma_4(v): 27 -> 32
#pragma unroll
        for (int r = 0; r < 16; ++r) dirv[r] = enc_register(r, half, kDirReal, vx, vy, vz);
        uint32_t dh[8], dm[8];
        split2_all(dh, dm, [&](int r) { return dirv[r]; });
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            park[(8 + q) * 64] = __builtin_bit_cast(f32x4, u32x4{dh[4 * q], dh[4 * q + 1], dh[4 * q + 2], dh[4 * q + 3]});
            park[(10 + q) * 64] = __builtin_bit_cast(f32x4, u32x4{dm[4 * q], dm[4 * q + 1], dm[4 * q + 2], dm[4 * q + 3]});
        }
    }
    const float* bias = ltab - L::bias_base;   // index with L::bias_off(layer), L::wsig_off, L::wrgb_off, L::scale_off

    const TrunkStash st{lane_off, nullptr, nullptr};
    uint32_t ph[8 * DT], pm[8 * DT];      // the packed terms of the current layer input, rewritten in place
    f32x16 accA[HT], accB[HT];           // halves A and B of the layer being computed
    float mx = 0.f, mxa = 0.f;           // running maximum of the activations (the fp16 range check)
    float sg0 = 0.f, sg1 = 0.f;          // density head: this lane's share of w_sigma . h8
    auto xh = [](int) -> const char* { return nullptr; };
    auto p0 = [&](int part) { return L::fwd_panel0(part); };

    {
#include "nnr_trunk_f16.inc"
    }

    auto xg = []() -> const char* { return nullptr; };
#include "nnr_colour_f16.inc"
    {
        const float* b = bias + L::bias_off(11);
        f32x4 o;
        o[0] = sigmoid_ref(rgbv[0] + b[0]);
        o[1] = sigmoid_ref(rgbv[1] + b[1]);
        o[2] = sigmoid_ref(rgbv[2] + b[2]);
        o[3] = sigma_raw;
        {   // a sample that saw an activation outside fp16's range (either of its two lanes) is made NaN here; so is one whose point is not
            // finite, as in the depth and proposal kernels (ReLU would turn its NaN activations into zeros and the sample out finite)
            const float kInf = __uint_as_float(0x7f800000u);
            const bool finite_p = fabsf(px) < kInf && fabsf(py) < kInf && fabsf(pz) < kInf;
            const bool over = left_f16_range(mx) || !finite_p;
            const float qnan = __uint_as_float(0x7fc00000u);
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = over ? qnan : o[c];
        }
        const bool counted = half == 0 && !dead;
        if (counted && has_ray && a.opt_out4) *reinterpret_cast<f32x4*>(a.opt_out4 + 4 * sc) = o;
        // the forward's fused epilogue on the compacted list: the next depth is the ORIGINAL list's, by index
        const int jn = j + 1;
        float zn = 0.f;
        if (jn < C) {
            const float lo1 = a.z_lo[jn], hi1 = a.z_hi[jn];
            zn = a.jitter ? __fadd_rn(lo1, __fmul_rn(__fsub_rn(hi1, lo1), a.jitter[sc + 1])) : lo1;
        }
        float unused;
        const float alpha = half == 0 ? sample_alpha(o[3], jn < C ? zn - z : 1e10f, jn == C, a.flags, unused) : 0.f;
        const float incl = wave_scan_mul(counted ? (1.f - alpha) + kEpsT : 1.f, lane);      // by select: a dead slot's alpha may be NaN
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.f;
        const float w = counted ? alpha * cT * excl : 0.f;
        cT *= __shfl(incl, 31, 64);
        if (counted) { cr += w * o[0]; cg += w * o[1]; cb += w * o[2]; cz += w * z; cw += w; }
    }
#undef NNR_FINISH
    pipe.next_pass(pass + 2 < n_pass);
#if NNR_SPARSE_STOP
    {   // the stop: flags by pass parity, one barrier, the same four flags in every wave -> the loop ends workgroup-uniformly
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
#endif
    }   // pass
#if NNR_SPARSE_STOP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // no DMA piece of this wave is in flight past here, stopped early or not
    if (has_ray && lane0 == 0 && a.opt_passes) a.opt_passes[ray] = n_ran;
#endif
    {
        const float sr = wave_sum(cr), sgn = wave_sum(cg), sb = wave_sum(cb), sz = wave_sum(cz), sw = wave_sum(cw);
        if (has_ray && lane0 == 0) {
            const float bg = (a.flags & kFlagWhiteBg) ? 1.f - sw : 0.f;
            float* out = a.out + 5 * (int64_t)ray;
            out[0] = sr + bg; out[1] = sgn + bg; out[2] = sb + bg;
            out[3] = sz;
            out[4] = sw;
        }
    }
}

#if NNR_SPARSE_STOP
hipError_t launch_render_sparse_stop(int D, const SparseStopArgs& a, hipStream_t st) {
#else
hipError_t launch_render_sparse(int D, const SparseArgs& a, hipStream_t st) {
#endif
    if (a.R <= 0 || a.C < 1 || a.C > kProposeMaxC) return hipErrorInvalidValue;
    dim3 grid(((uint32_t)a.R + kWavesPerBlock - 1) / kWavesPerBlock), block(256);
    if (D == 256) hipLaunchKernelGGL(NNR_SPARSE_KERNEL<256>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(NNR_SPARSE_KERNEL<128>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace nnr
