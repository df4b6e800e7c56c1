// nnr_resample.hip -- hierarchical sampling: from the alphas and depths of a coarse render, F more depths per ray drawn from the
// piecewise-constant density the compositor's weights define (NeRF's sample_pdf with stratified u), merged with the C coarse depths
// into one sorted row of C + F.  The definition is in include/nnr.h (nnr_resample) and DESIGN.md section 10; the reference has no
// counterpart.
//
// One wavefront per ray, four rays per workgroup (two where the rays are long: launch_resample); every array of a ray lives in that wave's own LDS region:
//   zc  [C]     the coarse depths
//   mm  [C-1]   bin edges m_i = (z_i + z_{i+1}) / 2
//   cdf [C-1]   cdf_0 = 0, cdf_{k+1} = cdf_k + p_k / sum p
//   fs  [F]     the fine samples
//   out [C+F]   first the alphas (staged by coalesced loads), then in place the bin masses p_k at [k + 1], last the merged row
// Stages (a workgroup barrier between them; every wave runs every stage, a wave past the last ray repeats that ray and stores nothing):
//   1. coalesced loads of alpha and z into LDS;
//   2. each lane owns a contiguous run of ceil(C / 64) samples: the run's product of (1 - a + 1e-6), the lanes' offsets by a
//      64-lane product scan, then T_i, w_i = a_i T_i and p_{i-1} = w_i + 1e-5 walking the run once more -- the compositor's weights
//      (nnr_composite.hip) up to the order of the product;
//   3. the CDF the same way over runs of bins; the lanes' offsets are the sequential sum of the 64 run totals (every lane adds the same
//      broadcast values in the same order: one fixed order, no tree).  Where a lane owns more than one bin, the last value of its run,
//      ((off + p_a) + p_b), and the next lane's offset, off + (p_a + p_b), can differ by an ulp; the CDF is non-decreasing all the same,
//      because every bin adds at least the 1e-5 floor to a sum of about 1, far more than an fp32 rounding there, before the division
//      by the total -- which the searches below rely on;
//   4. the inverse CDF of u_j = (j + xi_j) / F by binary search, s_j clamped to its bin [m_below, m_above] (a no-op in exact
//      arithmetic; in fp32 m_below + t (m_above - m_below) can round one ulp past the edge and break the order of the fine samples);
//   5. merge by rank: coarse i goes to i + #{fine < z_i}, fine j to j + #{coarse <= s_j} (coarse first on ties): two more searches;
//   6. the merged row out of LDS in coalesced 16-byte stores (4-byte ones where C + F is not a multiple of 4).
// Every search runs exactly kSearchTrips = ceil(log2 1024) steps with clamped indices: a NaN can neither loop nor index outside the
// region.  A ray with a NaN in alpha or z gets an all-NaN row.  No atomics; every sum and product in a fixed order: bit-reproducible.
#include "nnr_device.h"
#include "nnr_kernels.h"
#include "nnr_resample_row.h"
#include "../../include/nnr.h"

namespace nnr {

struct ResampleArgs {
    const float *alpha, *z, *xi;   // (R,C), (R,C), (R,F) or null
    float *z_all, *fine;           // (R,C+F), (R,F) or null
    int R, C, F;
    int stride;                    // floats of LDS per wave
};

__global__ __launch_bounds__(256) void resample_kernel(ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int ray_raw = blockIdx.x * (blockDim.x >> 6) + wv;
    const bool live = ray_raw < a.R;
    const int ray = live ? ray_raw : a.R - 1;
    const int C = a.C, F = a.F, N = C + F;
    const int Cp = (C + 3) & ~3, Fp = (F + 3) & ~3;
    float* zc = lds + (size_t)wv * a.stride;
    float* mm = zc + Cp;
    float* cdf = mm + Cp;
    float* fs = cdf + Cp;
    float* out = fs + Fp;
    const float* g_alpha = a.alpha + (int64_t)ray * C;
    const float* g_z = a.z + (int64_t)ray * C;

    // 1. coalesced loads
    bool bad = false;
    for (int i = lane; i < C; i += 64) {
        const float al = g_alpha[i], zz = g_z[i];
        bad = bad || (al != al) || (zz != zz);
        out[i] = al;
        zc[i] = zz;
    }
    bad = __any(bad) != 0;
    __syncthreads();

    // 2. to 6.: the row code shared with the fused proposal kernel (nnr_resample_row.h)
    resample_row(zc, mm, cdf, fs, out, C, F, a.xi ? a.xi + (int64_t)ray * F : nullptr, a.z_all + (int64_t)ray * N,
                 a.fine ? a.fine + (int64_t)ray * F : nullptr, lane, live, bad);
}

hipError_t launch_resample(int R, int C, int F, const float* alpha, const float* z, const float* xi, float* z_all, float* fine, hipStream_t st) {
    if (R <= 0 || C < 3 || F < 1 || C + F > kResampleMaxN) return hipErrorInvalidValue;
    ResampleArgs a{};
    a.alpha = alpha; a.z = z; a.xi = xi; a.z_all = z_all; a.fine = fine;
    a.R = R; a.C = C; a.F = F;
    const int Cp = (C + 3) & ~3, Fp = (F + 3) & ~3, Np = (C + F + 3) & ~3;
    a.stride = 3 * Cp + Fp + Np;      // <= 3 * 1024 + 4 + 1024 floats = 16.4 KB per wave
    // four rays per workgroup while that stays within 48 KB of LDS (8 KB at 64 + 128), two above it (at most 32.8 KB)
    const int waves = (size_t)a.stride * 4 * sizeof(float) <= 48 * 1024 ? 4 : 2;
    const size_t lds_bytes = (size_t)a.stride * waves * sizeof(float);
    hipLaunchKernelGGL(resample_kernel, dim3((R + waves - 1) / waves), dim3(64 * waves), lds_bytes, st, a);
    return hipGetLastError();
}

}  // namespace nnr
