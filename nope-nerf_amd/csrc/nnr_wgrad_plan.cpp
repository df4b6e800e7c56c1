// nnr_wgrad_plan.cpp -- the weight-gradient planners, the plan blob and the workspace regions behind the planes (nnr_wgrad_plan.h).
// Host arithmetic only: the C++ standard library, include/nnr.h and nnr_layout.h.
#include "nnr_wgrad_plan.h"

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>

namespace nnr {

WsLayout ws_layout(const nnr_cfg* c) {
    WsLayout w;
    w.S = (int64_t)c->n_rays * c->n_samples;
    w.S_pad = (w.S + kBlockSamples - 1) / kBlockSamples * kBlockSamples;
    w.D = c->hidden;
    w.train = (c->flags & NNR_F_TRAIN) != 0;
    w.bf16 = w.train && (c->flags & NNR_F_BF16) != 0;
    w.tile32 = w.train && (c->flags & (NNR_F_BF16 | NNR_F_SPLIT3)) == NNR_F_SPLIT3;   // the three-term training mode's gradient planes (nnr_layout.h)
    return w;
}

PlanKnobs PlanKnobs::from_env() {
    PlanKnobs k;
    auto num = [](const char* name, int lowest, int unset) {
        const char* e = std::getenv(name);
        return e ? std::max(lowest, std::atoi(e)) : unset;
    };
    auto set = [](const char* name) { return std::getenv(name) != nullptr; };
    k.split_w = num("NNR_WGRAD_SPLIT_WEIGHT", 50, k.split_w);
    k.split2_w = num("NNR_WGRAD_SPLIT2_WEIGHT", 50, k.split2_w);
    k.enc2_w = num("NNR_WGRAD_ENC2_WEIGHT", 0, k.enc2_w);
    k.max_blocks = num("NNR_WGRAD_MAX_BLOCKS", INT32_MIN, k.max_blocks);
    k.f16_off = set("NNR_WGRAD_BF16_TERMS");
    k.fp32 = set("NNR_WGRAD_FP32");
    k.bundles = set("NNR_WGRAD_BUNDLES");
    k.no_coop = set("NNR_WGRAD_NO_COOP");
    k.no_merge = set("NNR_WGRAD_NO_MERGE");
    return k;
}

const PlanKnobs& process_knobs() {
    static const PlanKnobs k = PlanKnobs::from_env();
    return k;
}

// ---- weight-gradient plan -------------------------------------------------------------------------------------------
std::vector<Unit> wgrad_units(int D) {
    std::vector<Unit> u;
    const int nb = D / 128;  // 128-wide blocks per D
    int group = 0;
    auto add = [&](int layer, int MI, int NI, int dpl, int dcol, int dvalid, int xpl, int xcol, int xvalid, int row0, int wcol0,
                   int rows_real, int cols_real, int ldw, int bias) {
        Unit x{};
        x.j = WgradJob{layer, MI, NI, dpl, dcol, dvalid, xpl, xcol, xvalid, row0, wcol0, rows_real, cols_real, ldw, 0, 0, bias, 0, -1, 0};
        x.group = group;
        u.push_back(x);
    };
    // D x D layers: hidden 2,3,4,6,7,8 (params 1,2,3,5,6,7) and the h-part of hidden 5 (param 4), feature (param 9)
    auto dxd = [&](int layer, int dpl, int xpl, int ldw, int cols_real) {
        for (int a = 0; a < nb; ++a)
            for (int b = 0; b < nb; ++b)
                add(layer, 4, 4, dpl, 128 * a, D - 128 * a, xpl, 128 * b, D - 128 * b, 128 * a, 128 * b, D, cols_real, ldw,
                    nb == 2 ? 2 + b : 1);   // the two tiles of a row block share d(bias): even / odd sample pairs
        ++group;
    };
    // posenc-input parts: hidden 1 (param 0) and the e-part of hidden 5 (param 4, columns D..D+62)
    auto dxe = [&](int layer, int dpl, int wcol0, int ldw, int cols_real, int bias) {
        for (int a = 0; a < nb; ++a)
            add(layer, 4, 2, dpl, 128 * a, D - 128 * a, P_XE, 0, kPosPad, 128 * a, wcol0, D, cols_real, ldw, bias);
        ++group;
    };
    dxe(0, P_DH1 + 0, 0, kPosReal, kPosReal, 1);
    dxd(1, P_DH1 + 1, P_XH1 + 0, D, D);
    dxd(2, P_DH1 + 2, P_XH1 + 1, D, D);
    dxd(3, P_DH1 + 3, P_XH1 + 2, D, D);
    dxd(4, P_DH1 + 4, P_XH1 + 3, D + kPosReal, D + kPosReal);
    dxe(4, P_DH1 + 4, D, D + kPosReal, D + kPosReal, 0);
    dxd(5, P_DH1 + 5, P_XH1 + 4, D, D);
    dxd(6, P_DH1 + 6, P_XH1 + 5, D, D);
    dxd(7, P_DH1 + 7, P_XH1 + 6, D, D);
    // density head (param 8): 1 x D, gradient operand = column 3 of the per-sample output gradients
    for (int b = 0; b < nb; ++b) add(8, 1, 4, P_DOUT4, 3, 1, P_XH1 + 7, 128 * b, D - 128 * b, 0, 128 * b, 1, D, D, b == 0);
    ++group;
    // colour hidden: the merged matrix W' = Wg[:, :D] Wf (D/2 x D, pseudo-parameter kMergedLayer) against hidden 8, and the
    // direction-encoding columns of param 10 (D/2 x 27 at column D).  dWf, dWg[:, :D], dbf follow from dW', db' in the
    // un-merge step after the reduction (nnr_wgrad.hip).
    const int mi_g = D == 256 ? 4 : 2;
    for (int b = 0; b < nb; ++b)
        add(kMergedLayer, mi_g, 4, P_DG, 0, D / 2, P_XH1 + 7, 128 * b, D - 128 * b, 0, 128 * b, D / 2, D, D, b == 0);
    add(10, mi_g, 1, P_DG, 0, D / 2, P_XF, 0, kDirPad, 0, D, D / 2, D + kDirReal, D + kDirReal, 0);
    ++group;
    // rgb (param 11): 3 x D/2, gradient operand = columns 0..2 of the per-sample output gradients
    add(11, 1, D == 256 ? 4 : 2, P_DOUT4, 0, 3, P_XG, 0, D / 2, 0, 0, 3, D / 2, D / 2, 1);
    ++group;
    return u;
}

// Balanced static schedule.  Work is measured in cost-granules (MI*NI MFMAs-per-sample-pair x 16 samples).  The D x D
// layers (4 tiles of 4x4 that share their two operand column halves) are scheduled per WORKGROUP: the 8 layers form one
// tape of (layer, granule) positions that is cut into equal spans, a span crossing a layer boundary becoming two segments
// whose four tiles go to the four waves -- same sample range in one CU, so the operand re-reads hit L1/L2.  Everything else
// (posenc parts, density, colour, rgb: 14 % of the work) is scheduled per WAVE on a second tape weighted by tile cost.
// Each job flushes to its own slot; the splits of a tile are chained (next_split) for the reduction kernel.
Plan build_plan(const nnr_cfg* c, const PlanKnobs& k) {
    const WsLayout w = ws_layout(c);
    const std::vector<Unit> units = wgrad_units(c->hidden);
    const int64_t granules = w.S_pad / kGranule;
    std::vector<std::vector<int>> groups;   // class A: groups of four 4x4 tiles
    std::vector<int> small;                  // class B: unit indices
    for (size_t i = 0; i < units.size();) {
        size_t e = i;
        while (e < units.size() && units[e].group == units[i].group) ++e;
        bool dxd = (e - i) == 4;
        for (size_t t = i; t < e; ++t) dxd = dxd && units[t].j.MI == 4 && units[t].j.NI == 4;
        if (dxd) groups.push_back({(int)i, (int)i + 1, (int)i + 2, (int)i + 3});
        else
            for (size_t t = i; t < e; ++t) small.push_back((int)t);
        i = e;
    }
    // Measured cycles per cost-granule relative to a 4x4 tile (tools/timeline.py, MI355X): narrow tiles issue the same
    // loads for fewer MFMAs.  Weights in 1/1000.
    // The term-split modes weigh their 4 x 4 tiles and position-encoding tiles by the knobs (PlanKnobs: split_w, split2_w, enc2_w, with their sweeps).
    const int split_w = k.split_w, split2_w = k.split2_w, enc2_w = k.enc2_w;
    const bool split = is_split3(c) && !k.fp32;
    const bool f16_groups = split && is_split2(c) && !k.f16_off && c->hidden == 256;      // (class-A groups exist at D = 256 only)
    const bool enc2 = f16_groups && enc2_w > 0;
    auto is_enc2 = [enc2](const WgradJob& j) { return enc2 && j.MI == 4 && j.NI == 2 && j.x_plane == P_XE; };
    auto weight = [=](const WgradJob& j) -> int64_t {
        const int mn = j.MI * j.NI;
        if (is_enc2(j)) return (int64_t)mn * enc2_w;      // (d(bias) rides in the split: no surcharge)
        // (the merged layer's two 4 x 4 tiles are class B: private six-term split in either mode; a class-A tile is recognised by its layer: hidden 2..8)
        const bool group_tile = mn == 16 && j.layer >= 1 && j.layer <= 7;
        int w = mn == 16 ? (split ? (f16_groups && group_tile ? split2_w : split_w) : 1000) : mn == 8 ? 1035 : mn == 4 ? 1145 : 1250;
        if (j.bias == 1) w += mn == 16 ? 20 : mn == 8 ? 42 : 20;
        return (int64_t)mn * w;
    };
    int64_t cost_a = 0, cost_b = 0;
    for (auto& g : groups) cost_a += 4 * weight(units[g[0]].j);   // bias halves: all four tiles of a group weigh the same
    for (int u : small) cost_b += weight(units[u].j);
    // Class B at D = 256 in BUNDLES (round 6, OFF unless NNR_WGRAD_BUNDLES is set -- a measured negative): the four waves of a workgroup take
    // narrow tiles that read the same planes over the SAME sample range at the same time, so a plane comes from HBM once and the other
    // readers find it in the CU's L1 / the XCD's L2.  On the per-wave tape below the tiles of one plane run on different workgroups -- other
    // XCDs, other L2s -- and the planes they share are fetched once per tile: 4.26 GB per launch against 3.4 GB of distinct planes.
    //   bundle 0: hidden-1 tiles a, b | skip layer's encoding tiles a, b             (share the position encoding)
    //   bundle 1: merged colour tiles a, b | density a + rgb | density b + direction   (share hidden 8, d colour-hidden, the 4-wide gradients)
    // A bundle costs its heaviest wave (7.0 / 7.0 / 9.2 / 9.2 in bundle 1: 12 % of those workgroups' time idle).  Measured, 1024 x 192
    // (profiles/r06/q_wgrad_bundles_ab.txt): fetched bytes 4.26 -> 4.04 GB, kernel 0.893 -> 0.915 ms.  The kernel is not waiting on those
    // bytes; the perfectly balanced tape wins.
    std::vector<std::array<std::vector<int>, 4>> bundles;
    if (c->hidden == 256 && k.bundles && !groups.empty()) {
        auto find = [&](int layer, int row0, int wcol0) {
            for (int u : small)
                if (units[u].j.layer == layer && units[u].j.row0 == row0 && units[u].j.wcol0 == wcol0) return u;
            return -1;
        };
        const int D = c->hidden;
        bundles.push_back({{{find(0, 0, 0)}, {find(0, 128, 0)}, {find(4, 0, D)}, {find(4, 128, D)}}});
        bundles.push_back({{{find(kMergedLayer, 0, 0)}, {find(kMergedLayer, 0, 128)}, {find(8, 0, 0), find(11, 0, 0)}, {find(8, 0, 128), find(10, 0, D)}}});
        size_t n = 0;
        bool ok = true;
        for (auto& b : bundles)
            for (auto& wv : b)
                for (int u : wv) { ok = ok && u >= 0; ++n; }
        if (!ok || n != small.size()) bundles.clear();      // (a unit list this table does not know: the per-wave tape)
    }
    std::vector<int64_t> bundle_cost;
    if (!bundles.empty()) {
        cost_b = 0;
        for (auto& b : bundles) {
            int64_t mx = 0;
            for (auto& wv : b) {
                int64_t s = 0;
                for (int u : wv) s += weight(units[u].j);
                mx = std::max(mx, s);
            }
            bundle_cost.push_back(mx);
            cost_b += 4 * mx;      // in wave-equivalents, like cost_a
        }
    }
    const int max_blocks = std::max(2, k.max_blocks);
    // Workgroups: one per kMinGranulesPerBlock granules of a D x D-at-256 group's worth of work (four 4x4 tiles), counted over
    // BOTH classes -- at D = 128 every unit is class B (a D x D layer is a single tile there), and sizing the launch by the
    // class-A groups alone left that whole configuration on one workgroup.
    const int64_t group_cost = 4 * 16 * 1000;
    const int64_t group_equiv = std::max<int64_t>(1, (cost_a + cost_b + group_cost / 2) / group_cost);
    const int n_blocks = (int)std::max<int64_t>(2, std::min<int64_t>(max_blocks, granules * group_equiv / kMinGranulesPerBlock));
    int nb_b = (int)((cost_b * n_blocks + (cost_a + cost_b) / 2) / (cost_a + cost_b));
    nb_b = groups.empty() ? n_blocks : std::max(1, std::min(n_blocks - 1, nb_b));
    const int nb_a = n_blocks - nb_b;

    std::vector<std::vector<WgradJob>> per_wave((size_t)n_blocks * 4);
    auto emit = [&](int wave, int unit, int64_t g0, int64_t g1) {
        if (g1 <= g0) return;
        WgradJob j = units[unit].j;
        j.k0 = (int32_t)(g0 * kGranule);
        j.k1 = (int32_t)(g1 * kGranule);
        j.split = unit;   // temporarily: the tile id, replaced by the split index below
        per_wave[wave].push_back(j);
    };
    // class A
    const int64_t tape_a = granules * (int64_t)groups.size();
    for (int b = 0; b < nb_a; ++b) {
        const int64_t a0 = tape_a * b / nb_a, a1 = tape_a * (b + 1) / nb_a;
        for (int64_t g = a0 / granules; g <= (a1 - 1) / granules && a1 > a0; ++g) {
            const int64_t lo = std::max(a0, g * granules) - g * granules, hi = std::min(a1, (g + 1) * granules) - g * granules;
            for (int t = 0; t < 4; ++t) emit(4 * b + t, groups[g][t], lo, hi);
        }
    }
    // Three-term mode: the four tiles of a class-A segment sit in one workgroup over ONE sample range -- the kernel runs them as a workgroup
    // job in which every operand value is split once (wgrad_group_split, nnr_wgrad.hip: barriers inside, so all four waves must be there)
    if (split && !k.no_coop)
        for (int wv = 0; wv < 4 * nb_a; ++wv)
            for (auto& j : per_wave[wv]) j.reserved = 1;
    // class B in bundles: bundle i occupies [off_i, off_i + cost_i * granules) of a tape that is cut per WORKGROUP
    if (!bundles.empty()) {
        int64_t tape = 0;
        for (int64_t cb : bundle_cost) tape += cb * granules;
        int64_t off = 0;
        for (size_t i = 0; i < bundles.size(); ++i) {
            const int64_t cb = bundle_cost[i], end = off + cb * granules;
            auto to_granule = [&](int64_t x) { return std::min(granules, std::max<int64_t>(0, (x - off + cb / 2) / cb)); };
            for (int b = 0; b < nb_b; ++b) {
                const int64_t c0 = tape * b / nb_b, c1 = tape * (b + 1) / nb_b;
                if (c1 <= off || c0 >= end) continue;
                const int64_t g0 = c0 <= off ? 0 : to_granule(c0), g1 = c1 >= end ? granules : to_granule(c1);
                for (int t = 0; t < 4; ++t)
                    for (int u : bundles[i][t]) emit(4 * (nb_a + b) + t, u, g0, g1);
            }
            off = end;
        }
    }
    // class B per wave (D = 128, or the bundles switched off): tile u occupies [off_u, off_u + cost_u * granules) of the tape; a cut inside a tile
    // is rounded to a granule
    const int nw_b = nb_b * 4;
    const int64_t tape_b = cost_b * granules;
    std::vector<int64_t> cuts((size_t)nw_b + 1);
    for (int v = 0; v <= nw_b; ++v) cuts[v] = tape_b * v / nw_b;
    int64_t off = 0;
    for (int u : bundles.empty() ? small : std::vector<int>{}) {
        const int64_t cu = weight(units[u].j), end = off + cu * granules;
        auto to_granule = [&](int64_t x) { return std::min(granules, std::max<int64_t>(0, (x - off + cu / 2) / cu)); };
        for (int v = 0; v < nw_b; ++v) {
            if (cuts[v + 1] <= off || cuts[v] >= end) continue;
            const int64_t g0 = cuts[v] <= off ? 0 : to_granule(cuts[v]);
            const int64_t g1 = cuts[v + 1] >= end ? granules : to_granule(cuts[v + 1]);
            emit(4 * nb_a + v, u, g0, g1);
        }
        off = end;
    }
    for (auto& v : per_wave)
        for (auto& j : v)
            if (is_enc2(j)) j.reserved = 2;
    // flatten by wave, then chain the splits of every tile in sample order
    Plan p;
    p.wave_first.push_back(0);
    for (auto& v : per_wave) {
        for (auto& j : v) p.jobs.push_back(j);
        p.wave_first.push_back((int32_t)p.jobs.size());
    }
    std::vector<std::vector<int>> by_tile(units.size());
    for (size_t i = 0; i < p.jobs.size(); ++i) by_tile[p.jobs[i].split].push_back((int)i);
    for (auto& v : by_tile) {
        std::sort(v.begin(), v.end(), [&](int x, int y) { return p.jobs[x].k0 < p.jobs[y].k0; });
        for (size_t s = 0; s < v.size(); ++s) {
            p.jobs[v[s]].split = (int32_t)s;
            p.jobs[v[s]].next_split = s + 1 < v.size() ? v[s + 1] : -1;
        }
        if (!v.empty()) p.heads.push_back(v[0]);
    }
    return p;
}

size_t plan_bytes(const Plan& p) { return p.jobs.size() * sizeof(WgradJob) + (p.wave_first.size() + 1 + p.heads.size() + 4) * sizeof(int32_t); }

namespace {
template <class T>
char* put(char* out, const T* v, size_t n) {
    if (n) std::memcpy(out, v, n * sizeof(T));
    return out + n * sizeof(T);
}
}  // namespace

void write_plan(const Plan& p, void* out) {
    const int32_t n_heads = (int32_t)p.heads.size();
    const int32_t trailer[4] = {kPlanMagic, (int32_t)p.jobs.size(), (int32_t)p.wave_first.size() - 1, n_heads};
    char* o = put(static_cast<char*>(out), p.jobs.data(), p.jobs.size());
    o = put(o, p.wave_first.data(), p.wave_first.size());
    o = put(o, &n_heads, 1);
    o = put(o, p.heads.data(), p.heads.size());
    put(o, trailer, 4);
}

// ---- weight-gradient plan of the bf16 training mode (nnr_wgrad_bf16.hip) ------------------------------------------------------
// Units = the products dW = Dlt^T X of the 12 layers (the feature layer merged into the colour-hidden one, the density head riding
// on the merged unit's extra gradient group; at D = 256 the skip layer and the colour-hidden layer take their two input planes --
// hidden | encoding -- in one unit, at D = 128 as two units), each with its tiling over the four waves of a workgroup.  The kernel is bound by streaming the operands once, so a unit's cost per 32-sample chunk is the KiB it
// stages; the units form one tape of (unit, chunk) positions that is cut into equal spans, one per workgroup (a span that
// crosses a unit boundary becomes two jobs).  Outputs = where the rectangles of a unit's product go.
void bf16_units(int D, bool no_merge, std::vector<BUnit>& units, std::vector<WgradOutB>& outs) {
    const int G = D / 16, Gh = D / 32;            // groups of a D-wide / D/2-wide plane
    const bool big = D == 256;
    const bool merge = big && !no_merge;
    auto out = [&](int unit, int layer, int d_row, int n_rows, int w_row, int x_col, int n_cols, int w_col, int ldw, int bias) {
        const BUnit& u = units[unit];
        outs.push_back(WgradOutB{unit, layer, d_row, n_rows, w_row, x_col, n_cols, w_col, ldw, bias, -1, u.MT, u.NT, u.WR, u.WC, 0});
    };
    auto dxd = [&](int layer, int dpl, int xpl, int ldw) {          // D x D: 256 -> four waves of 4 x 4 tiles, 128 -> of 2 x 2
        units.push_back(BUnit{dpl, 0, G, xpl, 0, G, big ? 4 : 2, big ? 4 : 2, 2, 2, 1});
        out((int)units.size() - 1, layer, 0, D, 0, 0, D, 0, ldw, 1);
    };
    auto dxe = [&](int layer, int dpl, int w_col, int ldw, int bias) {   // D x 63 against the bf16 copy of the position encoding
        units.push_back(BUnit{dpl, 0, G, P_XE16, 0, kPosPad / 16, big ? 2 : 1, 2, 4, 1, bias});
        out((int)units.size() - 1, layer, 0, D, 0, 0, kPosReal, w_col, ldw, bias);
    };
    dxe(0, P_DH1 + 0, 0, kPosReal, 1);
    dxd(1, P_DH1 + 1, P_XH1 + 0, D);
    dxd(2, P_DH1 + 2, P_XH1 + 1, D);
    dxd(3, P_DH1 + 3, P_XH1 + 2, D);
    if (merge) {      // skip layer, input = hidden 4 | position encoding: 8 x 10 tiles as four waves of 4 x 5, the gradient read once
        units.push_back(BUnit{P_DH1 + 4, 0, G, P_XH1 + 3, 0, G, 4, 5, 2, 2, 1, P_XE16, kPosPad / 16});
        out((int)units.size() - 1, 4, 0, D, 0, 0, D, 0, D + kPosReal, 1);
        out((int)units.size() - 1, 4, 0, D, 0, D, kPosReal, D, D + kPosReal, 0);
    } else {
        dxd(4, P_DH1 + 4, P_XH1 + 3, D + kPosReal);
        dxe(4, P_DH1 + 4, D, D + kPosReal, 0);
    }
    dxd(5, P_DH1 + 5, P_XH1 + 4, D);
    dxd(6, P_DH1 + 6, P_XH1 + 5, D);
    dxd(7, P_DH1 + 7, P_XH1 + 6, D);
    // merged colour-hidden matrix W' (D/2 x D) and the density row: gradient operand = P_DG groups 0..Gh (the last group holds
    // d rgb_pre[0..2], d sigma_raw), activation operand = hidden 8; the direction-encoding columns of the colour-hidden layer are
    // the same gradient against the encoding
    if (merge) {      // 5 x 9 tiles: three waves of 5 x 3 (the fourth only moves data)
        units.push_back(BUnit{P_DG, 0, Gh + 1, P_XH1 + 7, 0, G, 5, 3, 1, 3, 1, P_XF16, kDirPad / 16});
        out((int)units.size() - 1, kMergedLayer, 0, D / 2, 0, 0, D, 0, D, 1);
        out((int)units.size() - 1, 8, D / 2 + 3, 1, 0, 0, D, 0, D, 1);
        out((int)units.size() - 1, 10, 0, D / 2, 0, D, kDirReal, D, D + kDirReal, 0);
    } else {
        units.push_back(BUnit{P_DG, 0, Gh + 1, P_XH1 + 7, 0, G, big ? 5 : 3, big ? 2 : 1, 1, 4, 1});
        out((int)units.size() - 1, kMergedLayer, 0, D / 2, 0, 0, D, 0, D, 1);
        out((int)units.size() - 1, 8, D / 2 + 3, 1, 0, 0, D, 0, D, 1);
        units.push_back(BUnit{P_DG, 0, Gh, P_XF16, 0, kDirPad / 16, 1, 1, big ? 4 : 2, 1, 0});
        out((int)units.size() - 1, 10, 0, D / 2, 0, 0, kDirReal, D, D + kDirReal, 0);
    }
    // rgb head: the 3 output-gradient rows against the colour-hidden activations
    units.push_back(BUnit{P_DG, Gh, 1, P_XG, 0, Gh, 1, 1, 1, big ? 4 : 2, 1});
    out((int)units.size() - 1, 11, 0, 3, 0, 0, D / 2, 0, D / 2, 1);
}

BPlan build_plan_bf16(const nnr_cfg* c, const PlanKnobs& k) {
    const WsLayout w = ws_layout(c);
    BPlan p;
    std::vector<BUnit> units;
    bf16_units(c->hidden, k.no_merge, units, p.outs);
    const int64_t chunks = w.S_pad / 32;
    std::vector<int64_t> cost(units.size()), start(units.size() + 1, 0);
    for (size_t u = 0; u < units.size(); ++u) {
        cost[u] = units[u].d_groups + units[u].x_groups + units[u].x2_groups;
        start[u + 1] = start[u] + cost[u] * chunks;
    }
    const int64_t tape = start[units.size()];
    const int max_blocks = std::max(1, k.max_blocks);
    const int n_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(max_blocks, tape / kMinTapePerBlock));
    // cut u-th unit at chunk boundaries: position x on the tape inside unit u -> chunk round((x - start[u]) / cost[u])
    auto cut_chunk = [&](size_t u, int64_t x) {
        if (x <= start[u]) return (int64_t)0;
        if (x >= start[u + 1]) return chunks;
        return std::min(chunks, (x - start[u] + cost[u] / 2) / cost[u]);
    };
    p.block_first.push_back(0);
    for (int b = 0; b < n_blocks; ++b) {
        const int64_t lo = tape * b / n_blocks, hi = tape * (b + 1) / n_blocks;
        for (size_t u = 0; u < units.size(); ++u) {
            if (hi <= start[u] || lo >= start[u + 1]) continue;
            const int64_t c0 = cut_chunk(u, lo), c1 = cut_chunk(u, hi);
            if (c1 <= c0) continue;
            const BUnit& un = units[u];
            int dp = 0, xp = 0;
            int x2p = 0;
            const int64_t d_off = w.plane(un.d_plane, &dp), x_off = w.plane(un.x_plane, &xp);   // floats; pitch = floats per sample
            const int64_t x2_off = un.x2_groups ? w.plane(un.x2_plane, &x2p) : 0;
            p.jobs.push_back(WgradJobB{4 * d_off + 1024ll * un.d_g0, 4 * x_off + 1024ll * un.x_g0, 4 * 32 * dp, 4 * 32 * xp, un.d_groups,
                                       un.x_groups, (int32_t)u, un.MT, un.NT, un.WR, un.WC, (int32_t)c0, (int32_t)c1, un.bias, 0, -1,
                                       4 * x2_off, 4 * 32 * x2p, un.x2_groups});
        }
        p.block_first.push_back((int32_t)p.jobs.size());
    }
    // chain the jobs of every unit in sample order (they are generated in that order)
    std::vector<int> last(units.size(), -1), count(units.size(), 0), first(units.size(), -1);
    for (size_t j = 0; j < p.jobs.size(); ++j) {
        const int u = p.jobs[j].unit;
        p.jobs[j].split = count[u]++;
        if (last[u] >= 0) p.jobs[last[u]].next_split = (int32_t)j;
        else first[u] = (int)j;
        last[u] = (int)j;
    }
    for (auto& o : p.outs) o.first_job = first[o.unit];
    return p;
}

size_t plan_bytes(const BPlan& p) {
    return p.jobs.size() * sizeof(WgradJobB) + p.block_first.size() * sizeof(int32_t) + p.outs.size() * sizeof(WgradOutB);
}
void write_plan(const BPlan& p, void* out) {
    char* o = put(static_cast<char*>(out), p.jobs.data(), p.jobs.size());
    o = put(o, p.block_first.data(), p.block_first.size());
    put(o, p.outs.data(), p.outs.size());
}

PlanCounts plan_counts(const nnr_cfg* c) {
    struct Memo {
        int hidden = 0;
        int64_t S_pad = -1;
        uint32_t mode = 0;
        PlanCounts n{};
    };
    thread_local Memo m;
    const int64_t S_pad = ws_layout(c).S_pad;
    const uint32_t mode = c->flags & (NNR_F_TRAIN | NNR_F_BF16 | NNR_F_SPLIT3 | NNR_F_SPLIT2);
    if (m.hidden == c->hidden && m.S_pad == S_pad && m.mode == mode) return m.n;
    PlanCounts n;
    if (is_bf16(c)) {
        const BPlan p = build_plan_bf16(c, process_knobs());
        n = {(int)p.jobs.size(), (int)p.block_first.size() - 1, (int)p.outs.size()};
    } else {
        const Plan p = build_plan(c, process_knobs());
        n = {(int)p.jobs.size(), (int)p.wave_first.size() - 1, (int)p.heads.size()};
    }
    m.hidden = c->hidden; m.S_pad = S_pad; m.mode = mode; m.n = n;
    return n;
}

TrainWs::TrainWs(const nnr_cfg* c) {
    const WsLayout w = ws_layout(c);
    slots = merged_w = merged_b = total = w.total();
    plane_max = -1;
    if (!w.train) return;
    const int64_t D = c->hidden;
    merged_w = slots + plan_counts(c).n_jobs * (int64_t)(w.bf16 ? 4 * kSlotBFloats : kSlotFloats);
    merged_b = merged_w + D / 2 * D;
    total = merged_b + D / 2;
    if (is_split2(c)) {
        plane_max = total;
        total += kPlaneMaxWsFloats;
    }
}

}  // namespace nnr
