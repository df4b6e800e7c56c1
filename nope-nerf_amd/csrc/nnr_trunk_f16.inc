// nnr_trunk_f16.inc -- hidden 1 to 8 on packed fp16 terms (nnr_trunk_f16.h), as a block of statements: `{` #include "nnr_trunk_f16.inc" `}` inside
// the pass loop of a kernel, behind its opaque lane id.  Names it takes from that scope:
//   D, TRAIN, L = Layout<D, 3>, DT, HT      the kernel's template arguments and tile counts (NNR_STASH_ACT, nnr_trunk_f16.h: TRAIN unless the unit defines it)
//   pipe, p0(part)                           the weight stream and a part's first panel in it (L::fwd_panel0)
//   bias, lane, half                         the LDS tables (index with L::bias_off(layer), L::wsig_off, L::scale_off), the lane
//   park                                     8 free 16-byte LDS slots of this lane (stride 64)
//   eh, em [16]                              in: the packed terms of gamma_10(p); the same behind it
//   ph, pm [8 DT], accA, accB [HT]           out: pairs [0, NP) hold half A of hidden 8, accB its half B still to be finished (1 / s_w:
//                                            inv_scale<L>(bias, 7); plane xh(7), mask layer 7 half 1 and flush_max of plane 7 are the finisher's)
//   sg0, sg1, mx, mxa                        in: 0; out: half A's share of the density head, the running maximum of the activations (training: of
//                                            plane 8's half A in mx, of the planes before in mxa)
//   st (TrunkStash), xh(i)                   training: the stash, block (this chunk, octet 0) of hidden layer i + 1's activation plane
    constexpr int HR = 16 * HT;              // registers of half a layer's outputs
    constexpr int NP = HR / 2;               // register pairs per half (the unit of hidden epilogue work)
    constexpr int HW = (HR + 31) / 32;       // mask words per half
    constexpr int PP = mode_panels(DT, HT, 3);  // panels of one D x D/2 pass
    // stash stores a dense pass certainly issues while it consumes its last panel (gemm_part2's PRE of the part behind it): an "ahead" pass one per row but the last, a "behind" pass one per row
    constexpr int kPreA = NNR_STASH_ACT ? mode_gp(HT, 3) - 1 : 0, kPreB = NNR_STASH_ACT ? mode_gp(HT, 3) : 0;
    constexpr int SE = NNR_STASH_ACT ? 2 : 0;      // every second unit stores an octet
    const int lane_off = st.lane_off;
    uint32_t mwA[HW], mwB[HW];
    f32x2 keep = {0.f, 0.f};      // the first pair of an octet between its unit and the next one's store
    auto store_gates = [&](const uint32_t(&mw)[HW], int layer_idx, int hb) __attribute__((always_inline)) {
        if constexpr (TRAIN) store_mask<L>(st.mask_base, mw, layer_idx, hb);
    };

    // ---- hidden 1: 63 -> D, input = posenc.  Pass A, then pass B with A's epilogue hidden under it. ----
    init_acc(accA, bias, L::bias_off(0), half);
    gemm_part2<2, HT>(accA, eh, em, pipe, p0(F_L1A));
    init_acc(accB, bias, L::bias_off(0) + L::Dh, half);
    clear_mask(mwA);
    {
        const float inv = inv_scale<L>(bias, 0);
        const char* const pl = xh(0);
        gemm_part2<2, HT, NP, 0, NP / 4, SE, 0>(accB, eh, em, pipe, p0(F_L1B), NNR_FINISH(accA, 0, mwA, inv, pl, 0, false));
    }
    store_gates(mwA, 0, 0);
    // posenc is needed again only by the skip layer: its terms wait in LDS
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        park[q * 64] = __builtin_bit_cast(f32x4, u32x4{eh[4 * q], eh[4 * q + 1], eh[4 * q + 2], eh[4 * q + 3]});
        park[(4 + q) * 64] = __builtin_bit_cast(f32x4, u32x4{em[4 * q], em[4 * q + 1], em[4 * q + 2], em[4 * q + 3]});
    }
    // Invariant from here on: pairs [0, NP) hold half A of the newest layer, accB holds its half B still to be finished.

    // one D -> D ReLU layer (state_dict index `li`, previous layer index li - 1), packed at panel pa; SIG: this layer is hidden 8
    // (pre: the part before this one stashed -- not so behind the skip layer's encoding part)
    auto dense_layer = [&](int li, int pa, auto sig_tag, bool pre) __attribute__((always_inline)) {
        constexpr bool SIG = decltype(sig_tag)::value;
        init_acc(accA, bias, L::bias_off(li), half);
        clear_mask(mwB);
        {   // pass A: its first half of rows only reads pairs [0, NP); the previous layer's half B is finished meanwhile
            const float inv = inv_scale<L>(bias, li - 1);
            const char* const pl = xh(li - 1);
            gemm_part2<DT, HT, NP, 1, 0, SE, kPreB>(accA, ph, pm, pipe, pa, NNR_FINISH(accB, NP, mwB, inv, pl, HR / 4, false), pre);
        }
        store_gates(mwB, li - 1, 1);
        flush_max<TRAIN, NNR_STASH_ACT>(st, li - 1, lane, mx, mxa);
        init_acc(accB, bias, L::bias_off(li) + L::Dh, half);
        clear_mask(mwA);
        {   // pass B: half A of the new layer replaces pairs [0, NP) in place, one row behind the reads
            const float inv = inv_scale<L>(bias, li);
            const char* const pl = xh(li);
            gemm_part2<DT, HT, NP, 2, 0, SE, kPreA>(accB, ph, pm, pipe, pa + PP, NNR_FINISH(accA, 0, mwA, inv, pl, 0, SIG));
        }
        store_gates(mwA, li, 0);
    };
    // hidden 2..4
#pragma unroll 1
    for (int l = 0; l < 3; ++l) dense_layer(1 + l, p0(F_L2A) + 2 * PP * l, std::false_type{}, true);
    // hidden 5: [h4 ; e] -> D   (skip connection, input order [h, posenc]: model/official_nerf.py:63)
    init_acc(accA, bias, L::bias_off(4), half);
    clear_mask(mwB);
    {
        const float inv = inv_scale<L>(bias, 3);
        const char* const pl = xh(3);
        gemm_part2<DT, HT, NP, 1, 0, SE, kPreB>(accA, ph, pm, pipe, p0(F_L5HA), NNR_FINISH(accB, NP, mwB, inv, pl, HR / 4, false));
    }
    store_gates(mwB, 3, 1);
    flush_max<TRAIN, NNR_STASH_ACT>(st, 3, lane, mx, mxa);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u32x4 vh = __builtin_bit_cast(u32x4, park[q * 64]), vm = __builtin_bit_cast(u32x4, park[(4 + q) * 64]);
#pragma unroll
        for (int i = 0; i < 4; ++i) { eh[4 * q + i] = vh[i]; em[4 * q + i] = vm[i]; }
    }
    gemm_part2<2, HT>(accA, eh, em, pipe, p0(F_L5EA));
    init_acc(accB, bias, L::bias_off(4) + L::Dh, half);
    clear_mask(mwA);
    {
        const float inv = inv_scale<L>(bias, 4);
        const char* const pl = xh(4);
        gemm_part2<DT, HT, NP, 2, 0, SE, 0>(accB, ph, pm, pipe, p0(F_L5HB), NNR_FINISH(accA, 0, mwA, inv, pl, 0, false));
    }
    gemm_part2<2, HT>(accB, eh, em, pipe, p0(F_L5EB));
    store_gates(mwA, 4, 0);
    // hidden 6, 7, 8
#pragma unroll 1
    for (int l = 0; l < 2; ++l) dense_layer(5 + l, p0(F_L6A) + 2 * PP * l, std::false_type{}, l > 0);
    dense_layer(7, p0(F_L6A) + 2 * PP * 2, std::true_type{}, true);
