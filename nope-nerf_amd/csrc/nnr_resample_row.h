// nnr_resample_row.h -- the row code of hierarchical sampling (stages 2 to 6 of nnr_resample.hip's header: transmittance and bin masses, CDF,
// inverse CDF, merge by rank, stores), ONCE, for the two kernels that run it on a ray's alphas and depths in LDS: resample_kernel
// (nnr_resample.hip: the row loaded from HBM) and propose_f16_kernel (nnr_propose_f16.hip: the row made by the density passes of the same
// launch).  One wavefront per ray; the same arithmetic in the same order in both, so the two give the same bits on the same row.
#pragma once
#include "nnr_device.h"

namespace nnr {

constexpr int kResampleMaxN = 1024;     // C + F: the training limit on samples per ray
constexpr int kSearchTrips = 10;        // ceil(log2 kResampleMaxN): an interval of at most 1023 elements closes in 10 halvings
constexpr float kPdfFloor = 1e-5f;      // added to every bin's weight; also the guard on the CDF difference

// how many leading elements of the non-decreasing arr[0, n) are <= x (LE) or < x (!LE); 1 <= n < kResampleMaxN
template <bool LE>
__device__ __forceinline__ int count_leading(const float* arr, int n, float x) {
    int lo = 0, hi = n;
#pragma unroll
    for (int t = 0; t < kSearchTrips; ++t) {
        const int mid = min((lo + hi) >> 1, n - 1);
        const float v = arr[mid];
        const bool go = LE ? (v <= x) : (v < x);      // false for a NaN on either side
        const bool open = lo < hi;
        lo = (open && go) ? mid + 1 : lo;
        hi = (open && !go) ? mid : hi;
    }
    return lo;
}

// On entry (behind a workgroup barrier of the caller's): zc[0, C) the ray's depths, out[0, C) its alphas, both in this wave's own LDS
// region, as are mm, cdf (C floats each), fs (F) and out (C + F, 16-byte aligned).  g_xi: the ray's (F) offsets or null (= 0.5); g_out: its
// (C + F) row of z_all, g_fine: its (F) fine samples or null.  live: this wave has a ray of its own (a wave past the last ray repeats that
// ray and stores nothing); bad: a NaN in the ray's alpha or z -- the row is stored as NaN.
// The barriers between the stages are WORKGROUP barriers (they order only a wave's own LDS traffic, but every wave of the workgroup must
// reach them): every wave of the workgroup calls this function, with the same C and F.
__device__ __forceinline__ void resample_row(float* zc, float* mm, float* cdf, float* fs, float* out, int C, int F, const float* g_xi,
                                             float* g_out, float* g_fine, int lane, bool live, bool bad) {
    const int N = C + F;
    // 2. transmittance and bin masses over contiguous runs of samples
    {
        const int per = (C + 63) >> 6;
        const int i0 = min(lane * per, C), i1 = min(i0 + per, C);
        float prod = 1.f;
        for (int i = i0; i < i1; ++i) prod *= (1.f - out[i]) + kEpsT;
        const float incl = wave_scan_mul(prod, lane);
        float T = __shfl_up(incl, 1, 64);
        if (lane == 0) T = 1.f;
        for (int i = i0; i < i1; ++i) {
            const float al = out[i];
            if (i < C - 1) mm[i] = 0.5f * (zc[i] + zc[i + 1]);
            out[i] = al * T + kPdfFloor;      // p_{i-1}; [0] and [C-1] are not bins and are never read again
            T *= (1.f - al) + kEpsT;
        }
    }
    __syncthreads();

    // 3. CDF over contiguous runs of bins k in [0, C-2): p_k sits at out[k + 1]
    {
        const int nb = C - 2;
        const int per = (nb + 63) >> 6;
        const int k0 = min(lane * per, nb), k1 = min(k0 + per, nb);
        float sum = 0.f;
        for (int k = k0; k < k1; ++k) sum += out[k + 1];
        float off = 0.f, total = 0.f;
#pragma unroll
        for (int t = 0; t < 64; ++t) {
            const float v = __shfl(sum, t, 64);
            if (t < lane) off += v;
            total += v;
        }
        float acc = off;
        for (int k = k0; k < k1; ++k) {
            acc += out[k + 1];
            cdf[k + 1] = acc / total;
        }
        if (lane == 0) cdf[0] = 0.f;
    }
    __syncthreads();

    // 4. inverse CDF at the stratified u
    {
        const float n_fine = (float)F;
        for (int j = lane; j < F; j += 64) {
            const float xi = g_xi ? g_xi[j] : 0.5f;
            const float u = ((float)j + xi) / n_fine;
            const int i = count_leading<true>(cdf, C - 1, u);
            const int below = max(i - 1, 0), above = min(i, C - 2);
            const float cb = cdf[below], mb = mm[below], ma = mm[above];
            float den = cdf[above] - cb;
            if (den < kPdfFloor) den = 1.f;
            float s = mb + (u - cb) / den * (ma - mb);
            s = fminf(fmaxf(s, mb), ma);      // (fmaxf / fminf return the other operand for a NaN: s stays inside the bin)
            fs[j] = s;
        }
    }
    __syncthreads();

    // 5. merge by rank (reads zc, fs; writes out, whose bin masses are dead)
    for (int i = lane; i < C; i += 64) {
        const float v = zc[i];
        out[i + count_leading<false>(fs, F, v)] = v;
    }
    for (int j = lane; j < F; j += 64) {
        const float v = fs[j];
        out[j + count_leading<true>(zc, C, v)] = v;
    }
    __syncthreads();

    // 6. stores
    if (!live) return;
    const float qnan = __builtin_nanf("");
    if ((N & 3) == 0) {
        for (int i = 4 * lane; i < N; i += 256) {
            f32x4 v = *reinterpret_cast<const f32x4*>(out + i);
            if (bad) v = f32x4{qnan, qnan, qnan, qnan};
            *reinterpret_cast<f32x4*>(g_out + i) = v;
        }
    } else {
        for (int i = lane; i < N; i += 64) g_out[i] = bad ? qnan : out[i];
    }
    if (g_fine) {
        for (int j = lane; j < F; j += 64) g_fine[j] = bad ? qnan : fs[j];
    }
}

}  // namespace nnr
