// nnr_ray_distortion.hip -- the ray distortion of mip-NeRF 360 on the compositing weights, forward and backward (include/nnr_regularise.h;
// DESIGN.md section 13).  One wavefront per ray, four rays per workgroup, like the compositor (nnr_composite.hip); every per-sample value in
// DOUBLE on the fp32 inputs, as composite_bwd_kernel's, rounded once at the store.  All sums are 64-lane shuffle scans with carries across
// blocks of 64 samples, in a fixed order: a product scan for T, add scans for W_< and M_<, reverse add scans for W_>, M_> and B.
// Neither kernel uses LDS.  The backward needs T, W_< and M_< of every sample in its reverse pass: its forward pass keeps only the three
// carries at the START of every block -- block b's in lane b, N <= 1024 = 16 blocks -- and the reverse pass scans each block again from them,
// the same operations in the same order, hence the same bits (the alphas are evaluated twice, as composite_bwd_kernel evaluates them).
#include "nnr_device.h"
#include "nnr_regularise_kernels.h"
#include "../../include/nnr_regularise.h"

namespace nnr {

namespace {

__device__ __forceinline__ double rd_scan_mul(double v, int lane) {      // inclusive, lane i: product of lanes <= i
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double t = __shfl_up(v, d, 64);
        if (lane >= d) v *= t;
    }
    return v;
}
__device__ __forceinline__ double rd_scan_add(double v, int lane) {      // inclusive, lane i: sum of lanes <= i
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ double rd_rscan_add(double v, int lane) {      // inclusive, lane i: sum of lanes >= i
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double t = __shfl_down(v, d, 64);
        if (lane + d < 64) v += t;
    }
    return v;
}
__device__ __forceinline__ double rd_excl(double incl, int lane, double first) {      // the inclusive scan's value one lane down
    const double t = __shfl_up(incl, 1, 64);
    return lane == 0 ? first : t;
}

// density / alpha of one sample in double -- composite_bwd_kernel's sample_alpha_d (nnr_composite.hip), restated: returns alpha;
// d_alpha_d_raw receives d alpha / d sigma_raw.  One difference: a NaN raw stays a NaN under NNR_F_RELU_SIGMA too (there the comparison
// alone would turn it into sigma = 0), so that a ray with a NaN is NaN under every flag combination.
__device__ __forceinline__ double rd_sample_alpha(double raw, double delta, bool last, uint32_t flags, double& d_alpha_d_raw) {
    double sigma, dsig;
    if (flags & kFlagReluSigma) {
        sigma = raw > 0.0 ? raw : (raw == raw ? 0.0 : raw);
        dsig = raw > 0.0 ? 1.0 : 0.0;
    } else {      // F.softplus, beta = 1, threshold 20
        sigma = raw > 20.0 ? raw : log1p(exp(raw));
        dsig = raw > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-raw));
    }
    double alpha;
    if (flags & kFlagDistAlpha) {
        const double e = exp(-sigma * delta);
        alpha = last ? 1.0 : 1.0 - e;                  // the last alpha is 1: no gradient through it
        d_alpha_d_raw = last ? 0.0 : delta * e * dsig;
    } else {
        const double e = exp(-sigma);
        alpha = 1.0 - e;
        d_alpha_d_raw = e * dsig;
    }
    return alpha;
}

// one sample of a block: its alpha, the centre m and the length d of its interval in normalised depth; a lane past the ray's end is neutral
struct RdSample {
    double alpha, dadr, m, d;
    bool ok;
};
__device__ __forceinline__ RdSample rd_load(const RayDistortionArgs& a, int64_t base, int j) {
    RdSample s{0.0, 0.0, 0.0, 0.0, j < a.N};
    if (s.ok) {
        const float raw = a.raw[(base + j) * a.raw_stride];
        const float z = a.z[base + j];
        const bool last = j == a.N - 1;
        const float zn = last ? z : a.z[base + j + 1];
        const float delta = last ? 1e10f : zn - z;      // (the fp32 difference the compositor used)
        s.alpha = rd_sample_alpha(raw, delta, last, a.flags, s.dadr);
        const double s0 = ((double)z - (double)a.s_near) * (double)a.s_inv;
        const double s1 = ((double)zn - (double)a.s_near) * (double)a.s_inv;
        s.m = last ? s0 : 0.5 * (s0 + s1);
        s.d = last ? 0.0 : s1 - s0;
    }
    return s;
}

// the three forward scans of one block from the carries at its start: T, W_< and M_< of the lane's sample and w = alpha T; moves the carries on
struct RdPrefix {
    double T, w, Wlt, Mlt;
};
__device__ __forceinline__ RdPrefix rd_prefix(const RdSample& s, int lane, double& cT, double& cW, double& cM) {
    const double eps = (double)kEpsT;
    const double v = s.ok ? (1.0 - s.alpha) + eps : 1.0;
    const double iT = rd_scan_mul(v, lane);
    RdPrefix p;
    p.T = cT * rd_excl(iT, lane, 1.0);
    p.w = s.ok ? s.alpha * p.T : 0.0;
    const double wm = s.ok ? p.w * s.m : 0.0;
    const double iW = rd_scan_add(p.w, lane);
    const double iM = rd_scan_add(wm, lane);
    p.Wlt = cW + rd_excl(iW, lane, 0.0);
    p.Mlt = cM + rd_excl(iM, lane, 0.0);
    cT *= __shfl(iT, 63, 64);
    cW += __shfl(iW, 63, 64);
    cM += __shfl(iM, 63, 64);
    return p;
}

}  // namespace

__global__ __launch_bounds__(256) void ray_distortion_fwd_kernel(RayDistortionArgs a) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= a.R) return;      // (the whole wave: before any shuffle)
    const int64_t base = (int64_t)ray * a.N;
    double cT = 1.0, cW = 0.0, cM = 0.0, acc = 0.0;
    for (int j0 = 0; j0 < a.N; j0 += 64) {
        const RdSample s = rd_load(a, base, j0 + lane);
        const RdPrefix p = rd_prefix(s, lane, cT, cW, cM);
        if (s.ok) acc += 2.0 * p.w * (s.m * p.Wlt - p.Mlt) + p.w * p.w * s.d / 3.0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane == 0) a.loss[ray] = (float)acc;
}

__global__ __launch_bounds__(256) void ray_distortion_bwd_kernel(RayDistortionArgs a) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= a.R) return;      // (the whole wave: before any shuffle)
    const int64_t base = (int64_t)ray * a.N;
    const double g = a.g[ray];
    const double eps = (double)kEpsT;
    const int nblk = (a.N + 63) / 64;      // <= 16
    // pass 1: the carries at the start of every block, block b's kept by lane b
    double cT = 1.0, cW = 0.0, cM = 0.0, kT = 1.0, kW = 0.0, kM = 0.0;
    for (int b = 0; b < nblk; ++b) {
        if (lane == b) { kT = cT; kW = cW; kM = cM; }
        const RdSample s = rd_load(a, base, b * 64 + lane);
        (void)rd_prefix(s, lane, cT, cW, cM);
    }
    // pass 2: blocks in reverse; the suffix sums of w, w m and w a are true reverse sums (never total - prefix: B is divided by 1 - alpha + eps)
    double tW = 0.0, tM = 0.0, tB = 0.0;      // the sums over all samples after the current block
    for (int b = nblk - 1; b >= 0; --b) {
        const int j = b * 64 + lane;
        const RdSample s = rd_load(a, base, j);
        double bT = __shfl(kT, b, 64), bW = __shfl(kW, b, 64), bM = __shfl(kM, b, 64);
        const RdPrefix p = rd_prefix(s, lane, bT, bW, bM);
        const double wm = s.ok ? p.w * s.m : 0.0;
        const double rW = rd_rscan_add(p.w, lane), rM = rd_rscan_add(wm, lane);
        const double Wgt = (rW - p.w) + tW, Mgt = (rM - wm) + tM;
        const double ak = s.ok ? 2.0 * (s.m * (p.Wlt - Wgt) - p.Mlt + Mgt) + (2.0 / 3.0) * p.w * s.d : 0.0;
        const double wa = s.ok ? p.w * ak : 0.0;
        const double rB = rd_rscan_add(wa, lane);
        const double B = (rB - wa) + tB;
        tW += __shfl(rW, 0, 64);
        tM += __shfl(rM, 0, 64);
        tB += __shfl(rB, 0, 64);
        if (s.ok) {
            const double dalpha = p.T * ak - B / ((1.0 - s.alpha) + eps);
            const double v = g * (dalpha * s.dadr);
            float* out = a.d_raw + (base + j) * a.d_raw_stride;
            *out = a.accumulate ? (float)((double)*out + v) : (float)v;
        }
    }
}

hipError_t launch_ray_distortion_fwd(const RayDistortionArgs& a, hipStream_t st) {
    if (a.N > kMaxSamplesRayDistortion) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ray_distortion_fwd_kernel, dim3((a.R + 3) / 4), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_ray_distortion_bwd(const RayDistortionArgs& a, hipStream_t st) {
    if (a.N > kMaxSamplesRayDistortion) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ray_distortion_bwd_kernel, dim3((a.R + 3) / 4), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace nnr
