// nnr_frozen_sparse.hip -- the compaction front end of the sparse frozen-field render (include/nnr_frozen_sparse.h):
// which samples an occupancy bitfield leaves LIVE, the substitutes of those it culls, and the list of the live ones in ascending flat order
// ray * N + j -- ACROSS the rays, which the list-driven frozen kernels (nnr_mlp_fwd_f16.hip NNR_FWD_TRAIN=3, nnr_mlp_dgrad_f16.hip
// NNR_DGRAD_LIST=1) then walk in chunks of 32.  Three small launches, no atomics, every scan in a fixed order: the list is deterministic.
//   * flags: one wave per ray, lane l takes the samples j = l + 64 k.  z_j and p_j by the forward kernel's own unfused expressions, the cell
//     by the one rule of nnr_sparse_cell.h, the bit by a plain vector load.  LIVE iff outside the grid (a non-finite point is) or the bit is
//     set, or -- under NNR_F_DIST_ALPHA -- j is the ray's last sample, whose alpha is 1 whatever its density.  z goes to P_Z for EVERY sample;
//     a culled sample gets its P_OUT4 row (0, 0, 0, E), E = -inf (softplus, ReLU, with and without dist_alpha: alpha 0 and derivative 0,
//     exactly), and zero P_DPTS / P_DVIEW rows, which no later kernel touches.  The ballots are kept as the ray's bitmask (N <= 1024: 32
//     words), their popcounts as the ray's count.
//   * scan: ONE workgroup, thread t adds the counts of a contiguous run of rays, the 1024 partial sums are scanned in LDS, the run is walked
//     again: the ray's exclusive offset, and n_live behind the last.  Integer sums: any order gives the same numbers.
//   * fill: one wave per ray again, lane l of round k holds bit l of the mask's words 2 k, 2 k + 1: live[offset + popcount of the bits
//     below] = ray * N + j.
// Plain vector loads and stores only.  A unit of its own (csrc/build.py); its one launcher is called from nnr_frozen_api.cpp.
#include "nnr_device.h"
#include "nnr_frozen_sparse_kernels.h"
#include "nnr_sparse_cell.h"

namespace nnr {

constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(256) void frozen_sparse_flag_kernel(FrozenSparseArgs a) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (ray >= a.R) return;      // (per wave; no barrier below)
    const int N = a.N;
    const float* const ro = a.pts_o + 3 * (int64_t)ray;
    const float* const rd = a.pts_d + 3 * (int64_t)ray;
    const int64_t row0 = (int64_t)ray * N;
    uint32_t* const mask = a.ray_mask + (int64_t)ray * kFrozenSparseMaskWords;
    const float kE = __uint_as_float(0xff800000u);      // -inf
    int n_live = 0;
    for (int k = 0; 64 * k < N; ++k) {
        const int j = lane + 64 * k;
        const bool valid = j < N;
        const int jc = valid ? j : N - 1;
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
        if ((a.flags & kFlagDistAlpha) && j == N - 1) live = true;
        const uint64_t m = __ballot(live);
        if (valid) {
            const int64_t s = row0 + j;
            a.ws_z[s] = z;
            if (!live) {
                *reinterpret_cast<f32x4*>(a.ws_out4 + 4 * s) = f32x4{0.f, 0.f, 0.f, kE};
                *reinterpret_cast<f32x4*>(a.ws_dpts + 4 * s) = f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(a.ws_dview + 4 * s) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        if (lane == 0) {
            mask[2 * k] = (uint32_t)m;
            mask[2 * k + 1] = (uint32_t)(m >> 32);
        }
        n_live += __popcll(m);
    }
    if (lane == 0) {
        a.ray_count[ray] = n_live;
        if (a.opt_count) a.opt_count[ray] = n_live;
    }
}

__global__ __launch_bounds__(kScanThreads) void frozen_sparse_scan_kernel(FrozenSparseArgs a) {
    __shared__ int part[kScanThreads];
    const int t = threadIdx.x;
    const int per = (a.R + kScanThreads - 1) / kScanThreads;      // rays per thread, a contiguous run
    const int r0 = min(t * per, a.R), r1 = min(r0 + per, a.R);
    int sum = 0;
    for (int r = r0; r < r1; ++r) sum += a.ray_count[r];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {      // inclusive scan of the partial sums
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int off = part[t] - sum;
    for (int r = r0; r < r1; ++r) {
        a.ray_off[r] = off;
        off += a.ray_count[r];
    }
    if (t == kScanThreads - 1) {
        a.n_live[0] = part[t];
        if (a.opt_n_live) a.opt_n_live[0] = part[t];
    }
}

__global__ __launch_bounds__(256) void frozen_sparse_fill_kernel(FrozenSparseArgs a) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (ray >= a.R) return;
    const int N = a.N;
    const uint32_t* const mask = a.ray_mask + (int64_t)ray * kFrozenSparseMaskWords;
    const int row0 = ray * N;      // (S <= 2^31 - 1: nnr_frozen_api.cpp)
    int pos = a.ray_off[ray];
    for (int k = 0; 64 * k < N; ++k) {
        const uint64_t m = (uint64_t)mask[2 * k] | ((uint64_t)mask[2 * k + 1] << 32);
        if ((m >> lane) & 1ull) {
            const int at = pos + __popcll(m & ((1ull << lane) - 1ull));
            a.live[at] = row0 + lane + 64 * k;
            if (a.opt_live) a.opt_live[at] = row0 + lane + 64 * k;
        }
        pos += __popcll(m);
    }
}

hipError_t launch_frozen_sparse_compact(const FrozenSparseArgs& a, hipStream_t st) {
    if (a.R <= 0 || a.N < 1 || a.N > 32 * kFrozenSparseMaskWords) return hipErrorInvalidValue;
    dim3 grid(((uint32_t)a.R + kWavesPerBlock - 1) / kWavesPerBlock), block(256);
    hipLaunchKernelGGL(frozen_sparse_flag_kernel, grid, block, 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(frozen_sparse_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(frozen_sparse_fill_kernel, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace nnr
