// nnr_density_pass_f16.inc -- one density-only pass on packed fp16 terms, as a block of statements inside the pass loop of a kernel, behind its
// opaque lane id and its point: position encoding, the eight trunk layers (nnr_trunk_f16.inc, TRAIN = false -- the one place that includes it
// outside the forward kernel), the density head.  Nothing of the colour branch and no view direction.  Included by march_f16_kernel,
// propose_f16_kernel and grid_f16_kernel behind nnr_density_setup_f16.inc.  Names it takes from the including scope:
//   D, L = Layout<D, 3>, DT, HT              the kernel's template argument, the layout and the tile counts
//   px, py, pz                               the sample's point (lanes l and l + 32 hold the same sample)
//   lane, half                               the pass's opaque lane id, lane >> 5
//   park                                     8 free 16-byte LDS slots of this lane (stride 64)
//   pipe, ltab                               the weight stream and the LDS tables of the setup
// Names it leaves behind:
//   raw                                      float, not const: the raw density (before softplus / relu), the same in both lanes of a sample
//   mx                                       the maximum of the activations: left_f16_range(mx) is the including kernel's to ask, and what a sample
//                                            out of range becomes is its own
//   HR, NP, eh, em, bias, ph, pm, accA, accB, mxa, sg0, sg1, sg      its working names, dead behind it
    constexpr int HR = 16 * HT;
    constexpr int NP = HR / 2;

    uint32_t eh[16], em[16];      // gamma_10(p): 63 -> 64 values = 16 pairs
    {
        float e[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) e[r] = enc_register(r, half, kPosReal, px, py, pz);
        split2_all(eh, em, [&](int r) { return e[r]; });
    }
    const float* bias = ltab - L::bias_base;

    uint32_t ph[8 * DT], pm[8 * DT];
    f32x16 accA[HT], accB[HT];
    float mx = 0.f, mxa = 0.f;           // running maximum of the activations (the fp16 range check)
    float sg0 = 0.f, sg1 = 0.f;          // density head: this lane's share of w_sigma . h8
    {   // the trunk, nothing of the training side.  The braces stay: `st` here shadows a kernel's own (the march's state)
        constexpr bool TRAIN = false;
        const TrunkStash st{};
        auto xh = [](int) -> const char* { return nullptr; };
        auto p0 = [&](int part) { return L::fwd_panel0(part); };
#include "nnr_trunk_f16.inc"
    }
    {   // hidden 8, half B: no colour GEMM to hide it under -- finished here in plain code (the units' inline asm reads accumulators with no
        // hazard cover of its own; here the compiler sees the MFMA results it reads), the same products as unit_fwd_infer and the head's other half
        const float inv = inv_scale<L>(bias, 7);
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int r = 2 * u;
            const float x0 = relu1(accB[r >> 4][r & 15] * inv), x1 = relu1(accB[(r + 1) >> 4][(r + 1) & 15] * inv);
            mx = fmaxf(mx, fmaxf(x0, x1));
            const f32x2 w2 = *reinterpret_cast<const f32x2*>(bias + L::wsig_off + half * (16 * DT) + 2 * NP + r);
            sg0 = fmaf(w2[0], x0, sg0);
            sg1 = fmaf(w2[1], x1, sg1);
        }
    }
    const float sg = sg0 + sg1;
    float raw = sg + __shfl_xor(sg, 32, 64) + bias[L::bias_off(8)];
