// nnr_bricks_f16.hip -- the raw density of OfficialStaticNerf in a list of 8 x 8 x 8 bricks of a regular grid in one launch
// (include/nnr_geometry.h: nnr_density_bricks): the input of the refined mesh extraction (model/geometry.py:
// extract_mesh_refined), whose cost follows the surface and not the volume.  Built as grid_f16_kernel (nnr_grid_f16.hip): four waves of 32
// points per pass, the density-only pass shared with the march, proposal and grid kernels (nnr_density_setup_f16.inc, nnr_density_pass_f16.inc).
// This file holds the brick voxel's point and the store.
//   * bricks: (B, 3) int32 on the device, (bx, by, bz).  Brick b holds the fine grid points i_c = 8 b_c + l_c, l_c in 0..7: 512 voxels = four
//     128-voxel blocks.  Block k of the launch is quarter q = k & 3 of brick k >> 2; in it wave w, lane column col is the brick's voxel
//     l = 128 q + 32 w + col = (lx, ly, lz) = (l & 7, (l >> 3) & 7, l >> 6): shifts only.  The three coordinates are read per lane in front of
//     the pass (as the march's flat mode reads its state) and feed arithmetic only, never an address: a coordinate outside the grid -- the
//     bricks that reach past the grid's last point among them -- gives the value at that point, a meaningless one a meaningless value, no access
//     out of bounds.  Bricks may repeat and come in any order.
//   * points: p_c = origin_c + step_c * i_c, product and sum rounded separately, as the grid kernel forms them (grid_coord, repeated here with
//     its `fp contract(off)`): a brick voxel is, bit for bit, the dense grid's value at the same global index.
//   * output: one fp32 per voxel, (B, 8, 8, 8) = out[b][lz][ly][lx], which is out[128 k + 32 w + col]: the lanes of half 0 of a wave write 32
//     consecutive floats.  V = 512 B exactly: no padding, no voxel past the end.
//   * passes: a workgroup walks `passes` consecutive blocks under the grid kernel's rule, the last workgroup what is left of them.
// A voxel is NaN where an activation left fp16's range (left_f16_range).  No atomics, no scratch, every sum in a fixed order:
// bit-reproducible.  LDS: the weight ring (3 panels, 96 KB), the park area (32 KB), the tables.
#include "nnr_trunk_f16.h"

namespace nnr {

// origin + step * i, the product rounded before the sum: grid_f16_kernel's function (nnr_grid_f16.hip, where the reason for this form is
// written down), repeated so that that unit's text stays as it is.  The two must stay the same: tests/test_gpu_bricks.py compares bits.
__device__ __forceinline__ float brick_coord(float origin, float step, uint32_t i) {
#pragma clang fp contract(off)
    const float prod = step * (float)i;
    return origin + prod;
}

template <int D>
__global__ __launch_bounds__(256, 1) void bricks_f16_kernel(BricksArgs a) {
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

    // ---- the brick, the voxel in it and its point: block < n_blocks = 4 B, so the brick is one of the list and v < 512 B <= 2^31 - 1 ----
    const uint32_t block = block0 + (uint32_t)pass;
    const int32_t* const bc = a.bricks + 3 * (int64_t)(block >> 2);
    const uint32_t l = (block & 3u) * (kWavesPerBlock * kChunk) + (uint32_t)wave_u * kChunk + (uint32_t)col;
    const float px = brick_coord(a.origin[0], a.step[0], 8u * (uint32_t)bc[0] + (l & 7u));
    const float py = brick_coord(a.origin[1], a.step[1], 8u * (uint32_t)bc[1] + ((l >> 3) & 7u));
    const float pz = brick_coord(a.origin[2], a.step[2], 8u * (uint32_t)bc[2] + (l >> 6));

#include "nnr_density_pass_f16.inc"
    if (left_f16_range(mx)) raw = __uint_as_float(0x7fc00000u);
    if (half == 0) a.out[(block * kWavesPerBlock + (uint32_t)wave_u) * kChunk + (uint32_t)col] = raw;
    pipe.next_pass(pass + 2 < n_pass);
    }   // pass
}

// the grid kernel's rule (nnr_grid_f16.hip: kGridGroups, kGridMaxPasses): about 1024 workgroups, at most 32 and at least one pass each
constexpr uint32_t kBrickGroups = 1024, kBrickMaxPasses = 32;

hipError_t launch_density_bricks(int D, BricksArgs a, int n_bricks, hipStream_t st) {
    if (n_bricks < 1 || (int64_t)n_bricks * 512 > 0x7fffffff) return hipErrorInvalidValue;
    a.n_blocks = 4u * (uint32_t)n_bricks;
    uint32_t passes = a.n_blocks / kBrickGroups;
    passes = passes < 1 ? 1 : passes > kBrickMaxPasses ? kBrickMaxPasses : passes;
    a.passes = (int)passes;
    dim3 grid((a.n_blocks + passes - 1) / passes), block(256);
    if (D == 256) hipLaunchKernelGGL(bricks_f16_kernel<256>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(bricks_f16_kernel<128>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace nnr
