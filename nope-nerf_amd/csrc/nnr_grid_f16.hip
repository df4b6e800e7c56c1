// nnr_grid_f16.hip -- the raw density of OfficialStaticNerf on a regular grid in one launch (include/nnr.h: nnr_density_grid; DESIGN.md
// section 11): the input of the mesh extraction (model/geometry.py).  Four waves of 32 points per pass; the pass is the density-only pass
// shared with march_f16_kernel and propose_f16_kernel (nnr_density_setup_f16.inc: LDS and the weight stream, which stops in front of the
// colour panels; nnr_density_pass_f16.inc: position encoding, the eight trunk layers and the density head in the two-term fp16 arithmetic,
// nothing of the colour branch and no view direction).  This file holds the voxel's point and the store.
//   * points: nothing per point is read from HBM.  Voxel v (linear, x fastest) = (ix, iy, iz), coordinate c of its point
//     p_c = origin_c + step_c * i_c, the product and the sum rounded separately (grid_coord: no contraction): fp32 code on the host that
//     multiplies and then adds gets the same bits.
//   * output: one fp32 per voxel, the raw density (before softplus / relu), (nz, ny, nx) row-major: the lanes of half 0 of a wave write 32
//     consecutive floats.
//   * passes: a workgroup walks `passes` consecutive 128-voxel blocks (the stream wraps: only the first pass waits for weights, and the table
//     load is paid once), the last workgroup what is left of them.  Every wave runs every pass of its workgroup (the four waves share the
//     weight stream and its barriers); a voxel past the volume's end is evaluated at the last voxel's point and stores nothing.
// A voxel is NaN where an activation left fp16's range (left_f16_range).  No atomics, no scratch, every sum in a fixed order:
// bit-reproducible.  LDS: the weight ring (3 panels, 96 KB), the park area (32 KB), the tables.
#include "nnr_trunk_f16.h"

namespace nnr {

// origin + step * i, the product rounded before the sum.  Plain operators under `fp contract(off)`, not __fadd_rn(., __fmul_rn(.)): this
// toolchain's headers define those two as the plain operators, and behind the inlining -ffp-contract=fast joins them into one v_fma_f32.
__device__ __forceinline__ float grid_coord(float origin, float step, uint32_t i) {
#pragma clang fp contract(off)
    const float prod = step * (float)i;
    return origin + prod;
}

template <int D>
__global__ __launch_bounds__(256, 1) void grid_f16_kernel(GridArgs a) {
    constexpr int kDensityExtraF4 = 0;      // nothing of its own in LDS
#include "nnr_density_setup_f16.inc"
    // this workgroup's 128-voxel blocks: [block0, block0 + n_pass) (the launcher's grid leaves every workgroup at least one)
    const uint32_t block0 = blockIdx.x * (uint32_t)a.passes;
    const uint32_t left = a.n_blocks - block0;
    const int n_pass = left < (uint32_t)a.passes ? (int)left : a.passes;
    pipe.more = n_pass > 1;
    pipe.start();

#pragma unroll 1
    for (int pass = 0; pass < n_pass; ++pass) {
    int lane = lane0;      // opaque per pass (nnr_mlp_fwd_f16.hip)
    asm volatile("" : "+v"(lane));
    pipe.lane = lane;
    const int half = lane >> 5;
    const int col = lane & 31;
    f32x4* const park = smem + kRingF4 + wave * (8 * 64) + lane;

    // ---- the voxel and its point: V <= 2^31 - 1, so the padded index stays below 2^31 + 128 ----
    const uint32_t v = ((block0 + (uint32_t)pass) * kWavesPerBlock + (uint32_t)wave_u) * kChunk + (uint32_t)col;
    const uint32_t vc = v < a.V ? v : a.V - 1u;
    const uint32_t row = vc / a.nx;
    const uint32_t ix = vc - row * a.nx;
    const uint32_t iz = row / a.ny;
    const uint32_t iy = row - iz * a.ny;
    const float px = grid_coord(a.origin[0], a.step[0], ix);
    const float py = grid_coord(a.origin[1], a.step[1], iy);
    const float pz = grid_coord(a.origin[2], a.step[2], iz);

#include "nnr_density_pass_f16.inc"
    if (left_f16_range(mx)) raw = __uint_as_float(0x7fc00000u);
    if (half == 0 && v < a.V) a.out[v] = raw;
    pipe.next_pass(pass + 2 < n_pass);
    }   // pass
}

// Passes per workgroup: the 128-voxel blocks are dealt out so that the launch has about kGridGroups workgroups -- four for each of the
// 256 CUs of an MI355X, so that every CU gets a few and the tail of the launch is short -- but at most kGridMaxPasses passes each (beyond
// that the table load and the start of the weight stream, one pass's worth of time, are below 4 % of a workgroup's work), and at least one:
// a volume of fewer than 2 * kGridGroups blocks launches one workgroup per block.
constexpr uint32_t kGridGroups = 1024, kGridMaxPasses = 32;

hipError_t launch_density_grid(int D, GridArgs a, hipStream_t st) {
    if (a.V == 0 || a.V > 0x7fffffffu || a.nx == 0 || a.ny == 0) return hipErrorInvalidValue;
    a.n_blocks = (a.V + (kWavesPerBlock * kChunk - 1)) / (kWavesPerBlock * kChunk);
    uint32_t passes = a.n_blocks / kGridGroups;
    passes = passes < 1 ? 1 : passes > kGridMaxPasses ? kGridMaxPasses : passes;
    a.passes = (int)passes;
    dim3 grid((a.n_blocks + passes - 1) / passes), block(256);
    if (D == 256) hipLaunchKernelGGL(grid_f16_kernel<256>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(grid_f16_kernel<128>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace nnr
