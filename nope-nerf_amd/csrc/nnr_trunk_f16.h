// nnr_trunk_f16.h, nnr_trunk_f16.inc -- the trunk of OfficialStaticNerf (model/official_nerf.py:60-66: hidden 1 to 8, the skip connection into hidden 5) in
// the two-term fp16 arithmetic of nnr_split2.h, ONCE, for the four kernels that evaluate it: mlp_fwd_f16_kernel (nnr_mlp_fwd_f16.hip: inference
// and training, the colour branch behind it) and the three density-only kernels, TRAIN = false and nothing of the colour branch: march_f16_kernel
// (nnr_march_f16.hip), propose_f16_kernel (nnr_propose_f16.hip) and grid_f16_kernel (nnr_grid_f16.hip), which include the trunk through their
// one shared pass (nnr_density_pass_f16.inc, behind nnr_density_setup_f16.inc).
//   * between the layers a lane holds the PACKED TERMS of the activations (pair p -> ph[p], pm[p]: 32 bits per value, as many registers as the
//     fp32 values took), made once by the epilogue unit that finishes the pair; a GEMM row is 3 MT MFMAs + 3 MT fragment refills and nothing else;
//   * an epilogue unit = read the accumulator pair, undo the weight scale (one packed multiply by 1 / s_w: the accumulator started at s_w bias),
//     ReLU, [training: two gate bits, every second unit one whole-block non-temporal store of the four fp32 values to the activation plane],
//     [hidden 8: two FMAs of the density head], split;
//   * every D-wide layer runs as two half-output passes, the epilogue of one pass hidden in the MFMA stream of the next.
// Where the weight stream ends is the caller's pipe (n_panels: L::fwd_panels, or L::fwd_panel0(F_RGBH_F) without the colour branch).
// This header: what the trunk's text and its four consumers use.  nnr_trunk_f16.inc: the trunk itself, a block of statements that the forward
// kernel and the density-only pass include inside the pass loop.  Text, not a function template: as a forceinlined template over the register arrays (by reference) everything inlined and
// the resources stayed, but hipcc 7.2 reduced the panel arithmetic of the `#pragma unroll 1` layer loops differently and the forward kernels'
// listings changed (tools/isa_listing.py); included as text they are the listings of the kernel that held this text itself.
#pragma once
#include "nnr_mlp_fwd_common.h"
#include "nnr_split2.h"

#include <type_traits>

// NNR_STASH_ACT: "this kernel stores activations" -- the hidden and colour-hidden planes (xh(i), xg()) and the plane maxima the weight
// gradient scales by.  TRAIN unless the including unit says otherwise before this header: the frozen-field forward (nnr_mlp_fwd_f16.hip,
// NNR_FWD_TRAIN=2) is a training forward -- gate words, encodings, the NaN guard's per-plane maxima -- that stores none of them.
#ifndef NNR_STASH_ACT
#define NNR_STASH_ACT TRAIN
#endif

namespace nnr {

// One epilogue unit: pair u of a half (registers 2 u, 2 u + 1 of ACC) -> pair OFFP + u of the packed input of the next layer.
// INV: 1 / s_w of the layer; PLANE: block (this chunk, octet 0) of the layer's activation plane (training), BLK0: the half's first octet;
// SIG: hidden 8 -- add the pair's share of the density head (its row sits in the head tables in register order).
// A macro: its arguments name accumulator and mask arrays by token.  Names it takes from the scope it is used in: TRAIN, L, DT, bias, half, lane_off,
// ph, pm (the packed terms), keep (the first pair of an octet between its unit and the next one's store), mx, sg0, sg1.  Used by nnr_trunk_f16.inc and
// by the one part behind the trunk that finishes hidden 8 under the colour GEMM (nnr_mlp_fwd_f16.hip).  NNR_STASH_ACT (above) removes the stores alone.
#define NNR_FINISH(ACC, OFFP, MW, INV, PLANE, BLK0, SIG)                                                           \
    [&](int u) __attribute__((always_inline)) {                                                                  \
        const int r = 2 * u;                                                                                     \
        float x0, x1;                                                                                            \
        if constexpr (TRAIN) {      /* (x > 0) == (relu(x) != 0): two gate bits appended to the half's mask word (nnr_split2.h) */ \
            unit_fwd_train(ACC[r >> 4][r & 15], ACC[(r + 1) >> 4][(r + 1) & 15], INV, MW[r >> 5], x0, x1, ph[(OFFP) + u], pm[(OFFP) + u], mx); \
            if constexpr (NNR_STASH_ACT) {                                                                       \
                if (u & 1) tile_store(PLANE, lane_off, (BLK0) + (u >> 1), f32x4{keep[0], keep[1], x0, x1});      \
                else keep = f32x2{x0, x1};                                                                       \
            }                                                                                                    \
        } else {                                                                                                 \
            unit_fwd_infer(ACC[r >> 4][r & 15], ACC[(r + 1) >> 4][(r + 1) & 15], INV, x0, x1, ph[(OFFP) + u], pm[(OFFP) + u], mx); \
        }                                                                                                        \
        if constexpr (SIG) {                                                                                     \
            const f32x2 w2 = *reinterpret_cast<const f32x2*>(bias + L::wsig_off + half * (16 * DT) + 2 * (OFFP) + r); \
            sg0 = fmaf(w2[0], x0, sg0);                                                                          \
            sg1 = fmaf(w2[1], x1, sg1);                                                                          \
        }                                                                                                        \
    }

// 1 / s_w of a weight tensor's scale slot, wave-uniform (nnr_layout.h: scale_slot; the accumulators start at s_w bias)
template <class L>
__device__ __forceinline__ float inv_scale(const float* bias, int slot) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(bias[L::scale_off + 16 + slot])));
}

// The one bound of this arithmetic (include/nnr.h, NNR_F_SPLIT2): a hidden activation that rounds to inf in fp16 (>= 65520).  Its terms are
// inf / -inf, the next layer's products NaN -- and ReLU (v_max_f32 returns the operand that is a number) turns those into ZEROS: left
// alone the sample would come out finite and wrong.  `seen`: the largest activation this lane made for the sample; true if either of the
// sample's two lanes saw such an activation -- the caller then makes the sample NaN.
__device__ __forceinline__ bool left_f16_range(float seen) { return !(fmaxf(seen, __shfl_xor(seen, 32, 64)) < 65520.f); }

// what the training forward leaves behind per pass beside the activation planes (all unused, and free, with TRAIN = false)
struct TrunkStash {
    int lane_off = 0;                   // 16 bytes per lane: the lane's place in a 1 KiB block of a tile-major plane
    uint32_t* mask_base = nullptr;      // [chunk][layer][lane][words]; half A owns the low words; register r of a half at bit 31 - (r & 31) of word r >> 5 (gate_append2: NOT the bit order of the other modes' planes)
    uint32_t* wg_max = nullptr;         // the workgroup's largest stashed value per activation plane P_XH1..8 (as integers: the values are >= 0)
};

// A plane is complete (half A in the pass B of its layer, half B in the pass A of the next): its maximum to the workgroup's table
// (STASH: the kernel stores the plane; without it only the sample's own running maximum moves on, for the range guard)
template <bool TRAIN, bool STASH = TRAIN>
__device__ __forceinline__ void flush_max(const TrunkStash& st, int plane, int lane, float& mx, float& mxa) {
    if constexpr (TRAIN) {
        if constexpr (STASH) {
            const float m = wave_max_f32(mx);
            if (lane == 0) atomicMax(&st.wg_max[plane], __float_as_uint(m));
        }
        mxa = fmaxf(mxa, mx);
        mx = 0.f;
    }
}

}  // namespace nnr
