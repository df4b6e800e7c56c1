// nnr_mlp_fwd_common.h -- what the forward kernels with fp32 results (nnr_mlp_fwd.hip: fp32-MFMA and six-term modes; nnr_mlp_fwd_f16.hip and
// nnr_march_f16.hip through nnr_trunk_f16.h: two-term mode) share word for word around their GEMM parts and whose move into a forceinlined function
// leaves their listings as they are (tools/isa_listing.py): the accumulators' start at the bias, the mask words, the launch grid.
// (Tried and NOT shared for that reason, hipcc 7.2: the rgb head -- operands of four commutative adds swap; the fused compositing as a carry
// struct or over references -- the inference kernel's register allocation changes throughout.  The colour branch with the rgb head is shared by
// the two-term forward and the sparse render as included text, nnr_colour_f16.inc, which keeps the listings: profiles/colour_refactor/.)
#pragma once
#include "nnr_device.h"
#include "nnr_kernels.h"

namespace nnr {

// accumulators start at the bias (`b`: the layer half's bias row in the LDS tables; the pack kernel stored s_w bias where there is a weight
// scale), so an epilogue is only ReLU (+ gates) or a move
template <int HT>
__device__ __forceinline__ void init_acc(f32x16 (&acc)[HT], const float* bias, int bias_offset, int half) {
    const float* b = bias + bias_offset + 4 * half;
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 bb = *reinterpret_cast<const f32x4*>(b + 32 * t + 8 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t][4 * q + i] = bb[i];
        }
}

template <int HW>
__device__ __forceinline__ void clear_mask(uint32_t (&mw)[HW]) {
#pragma unroll
    for (int w = 0; w < HW; ++w) mw[w] = 0;
}
// the mask words of half `hb` of layer `layer_idx`: [chunk][layer][lane][words], half A owns the low words (mask_base: this chunk's, this lane's)
template <class L, int HW>
__device__ __forceinline__ void store_mask(uint32_t* mask_base, const uint32_t (&mw)[HW], int layer_idx, int hb) {
    uint32_t* m = mask_base + (int64_t)layer_idx * 64 * L::mask_words + hb * HW;
#pragma unroll
    for (int w = 0; w < HW; ++w) m[w] = mw[w];
}

// ray mode: one workgroup per 4 rays, chunks_per_ray passes each; flat mode: one workgroup per 128 samples
inline dim3 mlp_fwd_grid(const MlpFwdArgs& a) {
    return dim3((unsigned)(a.chunks_per_ray > 0 ? a.S_pad / kBlockSamples / a.chunks_per_ray : a.S_pad / kBlockSamples));
}

}  // namespace nnr
