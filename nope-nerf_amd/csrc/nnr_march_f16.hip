// nnr_march_f16.hip -- the occupancy march of the phong geometry renderer (reference model/rendering.py:277-418): position encoding, the eight
// trunk layers and the density head of OfficialStaticNerf (official_nerf.py:60-83, only_occupancy=True), nothing of the colour branch, in the
// two-term fp16 arithmetic of nnr_mlp_fwd_f16.hip (NNR_F_SPLIT3 | NNR_F_SPLIT2, Layout<D, 3>, three fp16 MFMA terms per product, fp32 accumulation,
// weights through the DMA-fed LDS ring).  It shares that kernel's trunk (nnr_trunk_f16.h, TRAIN = false) and has nothing of its direction
// encoding and colour GEMMs; the weight stream stops in front of the colour panels (n_panels = fwd_panel0(F_RGBH_F)), so a workgroup's
// passes wrap around the trunk's panels only.  The LDS carve-up and the stream (nnr_density_setup_f16.inc) and the pass from the point to the
// raw density (nnr_density_pass_f16.inc) are text shared with propose_f16_kernel and grid_f16_kernel; this file holds the march's own points
// and what it does with the density.
//
// Two modes, one kernel:
//   * ray mode (MarchArgs::flat == 0): one wave walks one ray's n_steps proposals d_j = d_far * t_j in passes of 32 samples (the workgroup four
//     rays).  d_far = the far root of |o + d dir| = radius (0 without a root, clamped at 0: get_sphere_intersection, :439-459) is computed here,
//     t_j comes from the host's torch.linspace table.  val_j = occ(p_j) - 0.5 and the first j with val_j * val_{j+1} < 0 are found in registers
//     (a wave ballot per pass, the previous pass's last value carried in), so nothing per sample reaches HBM: the wave writes one 16-byte
//     state (d_lo, d_hi, f_lo, f_hi) per ray.  Every pass runs (the four waves of a workgroup share the weight stream and its barriers), so
//     the search sees every sample: a NaN anywhere on the ray makes it a miss, as torch.min's propagation does in the reference (:357-359).
//   * flat mode (flat == 1): one secant step (:404-417) for 32 rays per wave: the estimate from the state, occ there, the bracket update.
//     Rays that are not hits are evaluated too (no compaction, no host sync) and keep their state.
// State encoding: hit = (d_lo, d_hi, f_lo < 0, f_hi); miss = (+inf, +inf, 0, 0); first proposal occupied (val_0 >= 0) = (0, 0, 0, 0).  A hit's
// f_lo stays negative through every step (it is only ever replaced by an f_mid < 0), so `f_lo < 0` is the hit test; march_finish_kernel turns
// the state into the reference's d (secant estimate / inf / 0).
#include "nnr_trunk_f16.h"

namespace nnr {

// the reference's occupancy (official_nerf.py:76-83) minus tau = 0.5; torch.relu keeps a NaN, so does this
__device__ __forceinline__ float march_val(float raw, uint32_t flags) {
    float occ = (flags & kFlagReluSigma) ? (raw < 0.f ? 0.f : raw) : softplus_ref(raw);
    if (!(flags & kFlagDistAlpha)) occ = __fsub_rn(1.f, expf(-occ));
    return __fsub_rn(occ, 0.5f);
}

// d_pred = -f_low * (d_high - d_low) / (f_high - f_low) + d_low, rounded op by op as torch does (:403, :417)
__device__ __forceinline__ float secant_pred(f32x4 st) {
    return __fadd_rn(__fdiv_rn(__fmul_rn(-st[2], __fsub_rn(st[1], st[0])), __fsub_rn(st[3], st[2])), st[0]);
}

template <int D>
__global__ __launch_bounds__(256, 1) void march_f16_kernel(MarchArgs a) {
    constexpr int kDensityExtraF4 = 0;      // nothing of its own in LDS
#include "nnr_density_setup_f16.inc"
    const int n_pass = a.flat ? 1 : (a.n_steps + kChunk - 1) / kChunk;
    pipe.more = n_pass > 1;
    pipe.start();

    // ray mode: this wave's ray and its far sphere root (wave-uniform)
    const int wave_ray = blockIdx.x * kWavesPerBlock + wave_u;
    const int mray = wave_ray < a.R ? wave_ray : a.R - 1;
    float d_far = 0.f;
    if (!a.flat) {
        const float ox = a.ray_o[3 * mray], oy = a.ray_o[3 * mray + 1], oz = a.ray_o[3 * mray + 2];
        const float dx = a.ray_d[3 * mray], dy = a.ray_d[3 * mray + 1], dz = a.ray_d[3 * mray + 2];
        const float dot = dx * ox + dy * oy + dz * oz;
        const float on = sqrtf(ox * ox + oy * oy + oz * oz);
        const float under = dot * dot - (on * on - a.radius * a.radius);
        d_far = under > 0.f ? fmaxf(sqrtf(under) - dot, 0.f) : 0.f;
    }
    // the search, carried across the passes (wave-uniform)
    float carry_v = 0.f, carry_d = 0.f, v0 = 0.f;
    f32x4 hit = {0.f, 0.f, 0.f, 0.f};
    bool found = false, any_nan = false;

#pragma unroll 1
    for (int pass = 0; pass < n_pass; ++pass) {
    int lane = lane0;      // opaque per pass (nnr_mlp_fwd_f16.hip)
    asm volatile("" : "+v"(lane));
    pipe.lane = lane;
    const int half = lane >> 5;
    const int col = lane & 31;
    f32x4* const park = smem + kRingF4 + wave * (8 * 64) + lane;

    int ray, j = 0;
    float d;
    f32x4 st = {0.f, 0.f, 0.f, 0.f};
    if (a.flat) {
        ray = wave_ray * kChunk + col;
        if (ray > a.R - 1) ray = a.R - 1;
        st = *reinterpret_cast<const f32x4*>(a.state + 4 * (int64_t)ray);
        d = st[2] < 0.f ? secant_pred(st) : 0.f;
    } else {
        ray = mray;
        j = pass * kChunk + col;
        d = __fmul_rn(d_far, a.t[j < a.n_steps ? j : a.n_steps - 1]);      // 0 * (1 - t) + d_far * t
    }
    const float* ro = a.ray_o + 3 * (int64_t)ray;
    const float* rd = a.ray_d + 3 * (int64_t)ray;
    const float px = __fadd_rn(ro[0], __fmul_rn(rd[0], d));
    const float py = __fadd_rn(ro[1], __fmul_rn(rd[1], d));
    const float pz = __fadd_rn(ro[2], __fmul_rn(rd[2], d));

#include "nnr_density_pass_f16.inc"
    if (left_f16_range(mx)) raw = __uint_as_float(0x7fc00000u);
    const float val = march_val(raw, a.flags);

    if (a.flat) {      // one secant step (:404-417) on the rays that are hits
        if (half == 0 && wave_ray * kChunk + col < a.R && st[2] < 0.f) {
            if (val < 0.f) { st[0] = d; st[2] = val; }
            else { st[1] = d; st[3] = val; }
            *reinterpret_cast<f32x4*>(a.state + 4 * (int64_t)ray) = st;
        }
    } else {           // the first sign change (:341-359): pair (j - 1, j) sits in the lane of sample j
        const bool valid = j < a.n_steps;
        const int src = col > 0 ? lane - 1 : lane;
        float vl = __shfl(val, src, 64), dl = __shfl(d, src, 64);
        if (col == 0) { vl = carry_v; dl = carry_d; }
        const bool cross = valid && j >= 1 && __fmul_rn(vl, val) < 0.f;
        const uint64_t b = __ballot(half == 0 && cross);
        if (__ballot(half == 0 && valid && val != val)) any_nan = true;
        if (pass == 0) v0 = __shfl(val, 0, 64);
        if (!found && b) {
            const int k = __builtin_ctzll(b);
            hit = f32x4{__shfl(dl, k, 64), __shfl(d, k, 64), __shfl(vl, k, 64), __shfl(val, k, 64)};
            found = true;
        }
        carry_v = __shfl(val, kChunk - 1, 64);
        carry_d = __shfl(d, kChunk - 1, 64);
    }
    pipe.next_pass(pass + 2 < n_pass);
    }   // pass
    if (!a.flat && lane0 == 0 && wave_ray < a.R) {
        const float inf = __uint_as_float(0x7f800000u);
        f32x4 out;
        if (!(v0 < 0.f)) out = f32x4{0.f, 0.f, 0.f, 0.f};                                    // mask_0_not_occupied == 0 -> d = 0
        else if (any_nan || !found || !(hit[2] < 0.f)) out = f32x4{inf, inf, 0.f, 0.f};      // no (neg -> pos) first sign change -> inf
        else out = hit;
        *reinterpret_cast<f32x4*>(a.state + 4 * (int64_t)wave_ray) = out;
    }
}

__global__ __launch_bounds__(256) void march_finish_kernel(const float* __restrict__ state, float* __restrict__ d_out, int R) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const f32x4 st = *reinterpret_cast<const f32x4*>(state + 4 * (int64_t)i);
    d_out[i] = st[2] < 0.f ? secant_pred(st) : st[0];
}

hipError_t launch_march(int D, const MarchArgs& a, hipStream_t st) {
    const unsigned waves = a.flat ? (unsigned)((a.R + kChunk - 1) / kChunk) : (unsigned)a.R;
    dim3 grid((waves + kWavesPerBlock - 1) / kWavesPerBlock), block(256);
    if (D == 256) hipLaunchKernelGGL(march_f16_kernel<256>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(march_f16_kernel<128>, grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_march_finish(const float* state, float* d_out, int R, hipStream_t st) {
    hipLaunchKernelGGL(march_finish_kernel, dim3((R + 255) / 256), dim3(256), 0, st, state, d_out, R);
    return hipGetLastError();
}

}  // namespace nnr
