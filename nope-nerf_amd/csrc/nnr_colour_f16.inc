// nnr_colour_f16.inc -- the colour branch behind the two-term trunk, as statements: #include "nnr_colour_f16.inc" once, behind the block of
// nnr_trunk_f16.inc, in the pass loop of a kernel that goes on to colour (the forward nnr_mlp_fwd_f16.hip, the sparse render nnr_sparse_f16.hip).
// Text and not a function for the trunk's reason (nnr_mlp_fwd_common.h, profiles/colour_refactor/).  Names it takes from that scope:
//   D, TRAIN, L = Layout<D, 3>, DT, HT, NP, HR, HW   the kernel's template arguments, tile counts and per-half register, pair and mask-word counts
//   pipe, p0(part)                           the weight stream and a part's first panel in it
//   bias, lane, lane_off, half               the LDS tables (L::bias_off(layer), L::wrgb_off, L::scale_off), the lane, 16 * lane, lane >> 5
//   park                                     slots 8..11 of this lane (stride 64): the packed terms of gamma_4(v), high pairs in 8, 9, low in 10, 11
//   ph, pm [8 DT], accA, accB [HT]           in: as the trunk leaves them (half A of hidden 8 in pairs [0, NP), accB its half B to be finished)
//   sg0, sg1, mx, mxa                        in: as the trunk leaves them; out: mx (training: and mxa) cover hidden 8 whole
//   st (TrunkStash), xh(i), xg()             training: the stash, the trunk's plane hook, block (this chunk, octet 0) of the colour-hidden plane;
//                                            a kernel without training stores returns nullptr from both
// It defines, for the kernel's output block: sigma_raw (the density head with its bias) and rgbv[3] (the rgb head before bias and sigmoid).
// NNR_FINISH (nnr_trunk_f16.h) stays defined behind it: the kernel #undefs it.
    // colour hidden: g = relu(W' h8 + Wg[:, D:] gamma_4(v) + b'), W' = Wg[:, :D] Wf (the feature layer folded in by the pack kernel, nnr_layout.h);
    // both parts share scale slot 8.  Its side work finishes hidden 8 (half B) incl. the density head's other half.
    uint32_t mwA[HW], mwB[HW];
    init_acc(accA, bias, L::bias_off(10), half);
    clear_mask(mwB);
    {
        f32x2 keep = {0.f, 0.f};      // (NNR_FINISH takes this name from here, as it takes TRAIN, L, DT, bias, half, lane_off, ph, pm, mx, sg0, sg1)
        const float inv = inv_scale<L>(bias, 7);
        const char* const pl = xh(7);
        // (stash stores: every second unit one octet; gemm_part2's PRE: those the trunk's last pass certainly issued while it consumed its last panel)
        gemm_part2<DT, HT, NP, 1, 0, NNR_STASH_ACT ? 2 : 0, NNR_STASH_ACT ? mode_gp(HT, 3) : 0>(accA, ph, pm, pipe, p0(F_RGBH_F),
                                                                             NNR_FINISH(accB, NP, mwB, inv, pl, HR / 4, true));
    }
    if constexpr (TRAIN) store_mask<L>(st.mask_base, mwB, 7, 1);
    flush_max<TRAIN, NNR_STASH_ACT>(st, 7, lane, mx, mxa);
    const float sg = sg0 + sg1;
    const float sigma_raw = sg + __shfl_xor(sg, 32, 64) + bias[L::bias_off(8)];
    {
        uint32_t dh[8], dm[8];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const u32x4 vh = __builtin_bit_cast(u32x4, park[(8 + q) * 64]), vm = __builtin_bit_cast(u32x4, park[(10 + q) * 64]);
#pragma unroll
            for (int i = 0; i < 4; ++i) { dh[4 * q + i] = vh[i]; dm[4 * q + i] = vm[i]; }
        }
        gemm_part2<1, HT>(accA, dh, dm, pipe, p0(F_RGBH_D));
    }
    float g[HR];      // the colour-hidden activations stay fp32: the rgb head is a per-lane dot product
    clear_mask(mwA);
    {
        const float inv = inv_scale<L>(bias, 8);
#pragma unroll
        for (int r = 0; r < HR; r += 2) {
            g[r] = relu1(accA[r >> 4][r & 15] * inv);
            g[r + 1] = relu1(accA[(r + 1) >> 4][(r + 1) & 15] * inv);
            if constexpr (TRAIN) gate_append2(mwA[r >> 5], g[r], g[r + 1]);
        }
    }
    if constexpr (TRAIN) store_mask<L>(st.mask_base, mwA, 8, 0);
    if constexpr (NNR_STASH_ACT) {      // registers 4 q .. 4 q + 3 = features 8 q + 4 half + {0..3}: octet q of the plane, one whole block per store
        const char* const pg = xg();
#pragma unroll
        for (int q = 0; q < HR / 4; ++q) tile_store(pg, lane_off, q, f32x4{g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]});
    }
    // rgb head: 3 per-lane dot products over the lane's half of g, halves combined by one shuffle, then sigmoid
    float rgbv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* wc = bias + L::wrgb_off + (2 * c + half) * HR;
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
        for (int q = 0; q < HR / 4; ++q) {
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(wc + 4 * q);
            acc0 = fmaf(w4[0], g[4 * q], acc0);
            acc1 = fmaf(w4[1], g[4 * q + 1], acc1);
            acc0 = fmaf(w4[2], g[4 * q + 2], acc0);
            acc1 = fmaf(w4[3], g[4 * q + 3], acc1);
        }
        const float part = acc0 + acc1;
        rgbv[c] = part + __shfl_xor(part, 32, 64);
    }
