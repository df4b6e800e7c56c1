// nnr_tsdf.hip -- depth maps of known cameras integrated into a truncated signed distance volume held in 8 x 8 x 8 bricks, in one launch
// (include/nnr_fusion.h: nnr_tsdf_integrate; Curless-Levoy / KinectFusion with weight 1 per observation): the volume
// whose zero set model/geometry.py: extract_mesh_tsdf meshes.  One thread per voxel, the cameras in index order in every thread: no atomics,
// every sum in a fixed order, bit-reproducible; tests/fusion_ref.py restates it in torch fp32 operation for operation.
//   * bricks: (B, 3) int32, as the brick kernel takes them (nnr_bricks_f16.hip).  Workgroup k holds half h = k & 1 of brick k >> 1: its 256
//     threads are the voxels l = 256 h + t = (lx, ly, lz) = (l & 7, (l >> 3) & 7, l >> 6), and voxel v = 256 k + t of the (B, 8, 8, 8)
//     accumulators.  The brick's coordinates are workgroup-uniform and feed arithmetic only, never an address: a brick outside the grid gives
//     the values at the points the formula gives, no access out of bounds.  Bricks may repeat and come in any order.
//   * point: p_c = origin_c + step_c * (float)(8 b_c + l_c), product and sum rounded separately (brick_coord's form).
//   * per camera c = 0, 1, ...: q_r = ((P_r0 px + P_r1 py) + P_r2 pz) + P_r3, r = 0, 1, 2, every operation rounded to fp32 (the whole kernel is
//     under `fp contract(off)`: no fused multiply-add anywhere); skip unless q_z > z_min; u = q_x / q_z, v = q_y / q_z (IEEE division);
//     col = (u + 1) cw, row = (v + 1) ch; ci = rintf(col), ri = rintf(row) (ties to even); skip unless 0 <= ci <= W - 1 and 0 <= ri <= H - 1,
//     decided on the floats -- a NaN fails -- before any conversion to an integer and before the address is formed; d = depth[c][ri][ci]: the
//     one data-dependent address of the kernel; skip unless d > 0 (NaN, zero and negative are unobserved; +inf passes: free space);
//     sd = q_z - d; skip unless sd <= trunc; sum += fmaxf(sd / trunc, -1), weight += 1.
//     The twelve floats of a camera are read through a wave-uniform index: scalar loads, once per wave and camera.
//   * both accumulators are loaded at the start and stored at the end: cameras may arrive in chunks over several launches, and the result is
//     the one-launch result bit for bit.
// No frustum cull: it was not shown to pay.  No LDS, no scratch.
#include "nnr_fusion_kernels.h"

namespace nnr {

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(TsdfArgs a) {
#pragma clang fp contract(off)
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;      // < V = 512 B <= 2^31 - 1: the grid is V / 256 workgroups exactly
    const int32_t* const bc = a.bricks + 3 * (int64_t)(blockIdx.x >> 1);
    const uint32_t l = (blockIdx.x & 1u) * 256u + threadIdx.x;
    const float sx = a.step[0] * (float)(8u * (uint32_t)bc[0] + (l & 7u));
    const float sy = a.step[1] * (float)(8u * (uint32_t)bc[1] + ((l >> 3) & 7u));
    const float sz = a.step[2] * (float)(8u * (uint32_t)bc[2] + (l >> 6));
    const float px = a.origin[0] + sx, py = a.origin[1] + sy, pz = a.origin[2] + sz;

    float sum = a.sum[v], weight = a.weight[v];
    const size_t image = (size_t)a.H * (size_t)a.W;
    for (int c = 0; c < a.n_cams; ++c) {
        const float* const P = a.cams + 12 * (size_t)c;
        const float t0 = P[0] * px, t1 = P[1] * py, t2 = P[2] * pz;
        const float t4 = P[4] * px, t5 = P[5] * py, t6 = P[6] * pz;
        const float t8 = P[8] * px, t9 = P[9] * py, t10 = P[10] * pz;
        const float qx = ((t0 + t1) + t2) + P[3];
        const float qy = ((t4 + t5) + t6) + P[7];
        const float qz = ((t8 + t9) + t10) + P[11];
        if (!(qz > a.z_min)) continue;
        const float u = __fdiv_rn(qx, qz), w = __fdiv_rn(qy, qz);
        const float u1 = u + 1.f, w1 = w + 1.f;
        const float col = u1 * a.cw, row = w1 * a.ch;
        const float cf = rintf(col), rf = rintf(row);
        if (!(cf >= 0.f && cf <= a.col_max && rf >= 0.f && rf <= a.row_max)) continue;
        const float d = a.depth[(size_t)c * image + (size_t)(uint32_t)rf * (size_t)a.W + (size_t)(uint32_t)cf];
        if (!(d > 0.f)) continue;
        const float sd = qz - d;
        if (!(sd <= a.trunc)) continue;
        sum = sum + fmaxf(__fdiv_rn(sd, a.trunc), -1.f);
        weight = weight + 1.f;
    }
    a.sum[v] = sum;
    a.weight[v] = weight;
}

hipError_t launch_tsdf_integrate(const TsdfArgs& a, hipStream_t st) {
    if (a.V < 512u || (a.V & 511u) || a.V > 0x7fffffffu || a.n_cams < 1 || a.H < 1 || a.W < 1 || a.H > kTsdfMaxExtent || a.W > kTsdfMaxExtent)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(a.V / 256u), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace nnr
