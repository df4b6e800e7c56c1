// plan_check.cpp -- a stand-alone program over the host planners (nope-nerf_amd/csrc/nnr_wgrad_plan.h), meant to be built together with
// nnr_wgrad_plan.cpp under -fsanitize=address,undefined (tests/test_plan_host_cpu.py).  No GPU, no HIP.  For every cfg of the grid and every
// knob setting it builds the plan, serialises it into a heap buffer of exactly plan_bytes (an overrun is a sanitizer report), states the
// plan's coverage, chaining and balance, and checks plan_counts' memo and the workspace regions behind the planes.  Exit status 0 = all held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "nnr_wgrad_plan.h"

using namespace nnr;

static int g_failed = 0;
static char g_ctx[160] = "";
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) std::printf("FAILED %s:%d [%s]: %s\n", __FILE__, __LINE__, g_ctx, #cond); \
        }                                                                                  \
    } while (0)

static const int kShapes[][2] = {{1, 1}, {4, 32}, {5, 33}, {5, 130}, {2, 128}, {3, 128}, {32, 64}, {256, 64}, {4, 1024}, {1024, 192}, {4096, 128}};
static const uint32_t kModes[] = {0, NNR_F_SPLIT3, NNR_F_SPLIT3 | NNR_F_SPLIT2, NNR_F_BF16};

// rows x cols of the 12 weight tensors and [12] the merged colour matrix W'
static void shapes_of(int D, int (&s)[13][2]) {
    const int t[13][2] = {{D, 63}, {D, D}, {D, D}, {D, D}, {D, D + 63}, {D, D}, {D, D}, {D, D}, {1, D}, {D, D}, {D / 2, D + 27}, {3, D / 2}, {D / 2, D}};
    std::memcpy(s, t, sizeof(t));
}

// Every (layer, row, col) is produced by jobs whose sample ranges partition [0, S_pad); bias rows are reduced exactly once per range; the splits of
// a tile are chained in sample order from its head.  (The statements of tests/test_layout_cpu.py::test_wgrad_plan_covers_every_weight_once.)
static void check_plan(const nnr_cfg& c, const PlanKnobs& k, const Plan& p) {
    const int D = c.hidden;
    const int64_t S_pad = ws_layout(&c).S_pad;
    int sh[13][2];
    shapes_of(D, sh);
    std::vector<std::vector<int64_t>> cover(13), bias(13);
    for (int l = 0; l < 13; ++l) {
        cover[l].assign((size_t)sh[l][0] * sh[l][1], 0);
        bias[l].assign(sh[l][0], 0);
    }
    // the splits of a tile differ in their sample range alone: add the ranges up per tile first, then cover the tile's elements once
    std::map<std::tuple<int, int, int, int, int, int, int, int, int, int>, int64_t> tiles;
    for (const WgradJob& j : p.jobs) {
        CHECK(j.k0 % 16 == 0 && j.k1 % 16 == 0 && 0 <= j.k0 && j.k0 < j.k1 && j.k1 <= S_pad);
        CHECK(j.layer >= 0 && j.layer < 13);
        if (j.layer < 0 || j.layer >= 13) continue;
        CHECK(j.ldw == sh[j.layer][1] && j.rows_real == sh[j.layer][0]);
        tiles[std::make_tuple(j.layer, j.MI, j.NI, j.d_valid, j.x_valid, j.row0, j.wcol0, j.rows_real, j.cols_real, j.bias)] += j.k1 - j.k0;
    }
    for (const auto& t : tiles) {
        WgradJob j{};
        std::tie(j.layer, j.MI, j.NI, j.d_valid, j.x_valid, j.row0, j.wcol0, j.rows_real, j.cols_real, j.bias) = t.first;
        j.k1 = (int32_t)t.second;      // (k0 = 0: the tile's samples in all)
        std::vector<int> rows, cols;
        for (int e = 0; e < 32 * j.MI; ++e)
            if (e < j.d_valid && j.row0 + e < j.rows_real) rows.push_back(j.row0 + e);
        for (int e = 0; e < 32 * j.NI; ++e)
            if (e < j.x_valid && j.wcol0 + e < j.cols_real) cols.push_back(j.wcol0 + e);
        for (int r : rows) {
            for (int q : cols) cover[j.layer][(size_t)r * sh[j.layer][1] + q] += j.k1 - j.k0;
            if (j.bias) bias[j.layer][r] += (int64_t)(j.k1 - j.k0) * (j.bias == 1 ? 2 : 1);
        }
    }
    for (int l = 0; l < 13; ++l)
        for (int r = 0; r < sh[l][0]; ++r) {
            for (int q = 0; q < sh[l][1]; ++q) {
                const bool none = l == 9 || (l == 10 && q < D);      // the feature layer and Wg[:, :D] come from the un-merge step
                CHECK(cover[l][(size_t)r * sh[l][1] + q] == (none ? 0 : S_pad));
            }
            CHECK(bias[l][r] == ((l == 9 || l == 10) ? 0 : 2 * S_pad));
        }
    const int n_waves = (int)p.wave_first.size() - 1;
    CHECK(n_waves % 4 == 0 && n_waves / 4 <= std::max(2, k.max_blocks) && p.wave_first.front() == 0 && p.wave_first.back() == (int32_t)p.jobs.size());
    CHECK(std::is_sorted(p.wave_first.begin(), p.wave_first.end()));
    size_t heads = 0;
    for (size_t i = 0; i < p.jobs.size(); ++i) {
        const WgradJob& j = p.jobs[i];
        if (j.split != 0) continue;
        ++heads;
        CHECK(std::count(p.heads.begin(), p.heads.end(), (int32_t)i) == 1);
        int64_t at = 0;
        int n = 0;
        for (int cur = (int)i; cur >= 0; cur = p.jobs[cur].next_split, ++n) {
            CHECK(cur < (int)p.jobs.size() && n <= (int)p.jobs.size());
            if (cur >= (int)p.jobs.size() || n > (int)p.jobs.size()) break;
            const WgradJob& o = p.jobs[cur];
            CHECK(o.layer == j.layer && o.row0 == j.row0 && o.wcol0 == j.wcol0 && o.split == n && o.k0 == at);
            at = o.k1;
        }
        CHECK(at == S_pad);
    }
    CHECK(heads == p.heads.size());
    // balance at the benchmark size, default weights (test_layout_cpu.py): no workgroup -- done when its slowest wave is -- more than 3 % above the mean
    if (D == 256 && c.n_rays == 1024 && c.n_samples == 192 && k.max_blocks == kMaxBlocks && is_split3(&c)) {
        const bool two = is_split2(&c);
        auto enc = [&](const WgradJob& j) { return two && j.MI == 4 && j.NI == 2 && j.x_plane == P_XE; };
        auto cost = [&](const WgradJob& j) {
            const int mn = j.MI * j.NI;
            const double w = mn == 16 ? ((two && j.layer >= 1 && j.layer <= 7) ? 0.34 : 0.44) : enc(j) ? 0.625 : mn == 8 ? 1.035 : mn == 4 ? 1.145 : 1.25;
            return w * mn * (j.k1 - j.k0);
        };
        std::vector<double> load;
        double sum = 0;
        for (int b = 0; b < n_waves / 4; ++b) {
            double mx = 0;
            for (int wv = 4 * b; wv < 4 * b + 4; ++wv) {
                double s = 0;
                for (int i = p.wave_first[wv]; i < p.wave_first[wv + 1]; ++i) s += cost(p.jobs[i]);
                mx = std::max(mx, s);
            }
            load.push_back(mx);
            sum += mx;
        }
        for (const WgradJob& j : p.jobs) CHECK((j.reserved == 2) == enc(j));
        CHECK(n_waves == 1024 && *std::max_element(load.begin(), load.end()) <= 1.03 * sum / load.size());
    }
}

// bf16 plan: the jobs of a unit partition the chunks and are chained in order from the head its outputs name; every weight is the destination of
// exactly one rectangle.  (The statements of tests/test_layout_cpu.py::test_bf16_wgrad_plan_covers_every_weight_once that need no library.)
static void check_plan(const nnr_cfg& c, const PlanKnobs& k, const BPlan& p) {
    const int D = c.hidden;
    const int64_t chunks = ws_layout(&c).S_pad / 32;
    int sh[13][2];
    shapes_of(D, sh);
    const int n_blocks = (int)p.block_first.size() - 1;
    CHECK(n_blocks >= 1 && n_blocks <= std::max(1, k.max_blocks) && p.block_first.front() == 0 && p.block_first.back() == (int32_t)p.jobs.size());
    CHECK(std::is_sorted(p.block_first.begin(), p.block_first.end()));
    std::map<int, std::vector<int>> units;
    for (size_t i = 0; i < p.jobs.size(); ++i) {
        const WgradJobB& j = p.jobs[i];
        units[j.unit].push_back((int)i);
        CHECK(0 <= j.c0 && j.c0 < j.c1 && j.c1 <= chunks && j.WR * j.WC >= 1 && j.WR * j.WC <= 4 && j.MT * j.NT <= kSlotBMaxTiles);
        CHECK(j.d_groups + j.x_groups + j.x2_groups <= 36 && (j.x2_groups == 0 || j.x_groups % 2 == 0));
    }
    for (auto& u : units) {      // generated in sample order
        int64_t at = 0;
        for (size_t s = 0; s < u.second.size(); ++s) {
            const WgradJobB& j = p.jobs[u.second[s]];
            CHECK(j.c0 == at && j.split == (int)s && j.next_split == (s + 1 < u.second.size() ? u.second[s + 1] : -1));
            at = j.c1;
        }
        CHECK(at == chunks);
    }
    std::vector<std::vector<int>> cover(13), bias(13);
    for (int l = 0; l < 13; ++l) {
        cover[l].assign((size_t)sh[l][0] * sh[l][1], 0);
        bias[l].assign(sh[l][0], 0);
    }
    for (const WgradOutB& o : p.outs) {
        CHECK(o.layer >= 0 && o.layer < 13 && units.count(o.unit) == 1);
        if (o.layer < 0 || o.layer >= 13 || !units.count(o.unit)) continue;
        CHECK(o.first_job == units[o.unit][0] && o.ldw == sh[o.layer][1]);
        CHECK(o.d_row + o.n_rows <= 32 * o.MT * o.WR && o.x_col + o.n_cols <= 32 * o.NT * o.WC);
        CHECK(o.w_row + o.n_rows <= sh[o.layer][0] && o.w_col + o.n_cols <= sh[o.layer][1]);
        if (o.w_row + o.n_rows > sh[o.layer][0] || o.w_col + o.n_cols > sh[o.layer][1]) continue;
        for (int r = o.w_row; r < o.w_row + o.n_rows; ++r) {
            for (int q = o.w_col; q < o.w_col + o.n_cols; ++q) ++cover[o.layer][(size_t)r * sh[o.layer][1] + q];
            if (o.bias) ++bias[o.layer][r];
        }
    }
    for (int l = 0; l < 13; ++l)
        for (int r = 0; r < sh[l][0]; ++r) {
            for (int q = 0; q < sh[l][1]; ++q) CHECK(cover[l][(size_t)r * sh[l][1] + q] == ((l == 9 || (l == 10 && q < D)) ? 0 : 1));
            CHECK(bias[l][r] == ((l == 9 || l == 10) ? 0 : 1));
        }
}

// serialise into exactly plan_bytes on the heap and read the tables back where the kernels' launchers look for them
template <class P>
static std::unique_ptr<char[]> serialise(const P& p, size_t* n) {
    *n = plan_bytes(p);
    std::unique_ptr<char[]> blob(new char[*n]);
    write_plan(p, blob.get());
    return blob;
}

static PlanCounts counts_of(const Plan& p) { return {(int)p.jobs.size(), (int)p.wave_first.size() - 1, (int)p.heads.size()}; }
static PlanCounts counts_of(const BPlan& p) { return {(int)p.jobs.size(), (int)p.block_first.size() - 1, (int)p.outs.size()}; }
static bool same(const PlanCounts& a, const PlanCounts& b) {
    return a.n_jobs == b.n_jobs && a.n_waves_or_blocks == b.n_waves_or_blocks && a.n_heads_or_outs == b.n_heads_or_outs;
}
static PlanCounts built_counts(const nnr_cfg& c) {
    return is_bf16(&c) ? counts_of(build_plan_bf16(&c, process_knobs())) : counts_of(build_plan(&c, process_knobs()));
}

// the regions behind the planes: in order, disjoint, 16-byte aligned, the plane maxima last and in the two-term training mode only
static void check_ws(const nnr_cfg& c) {
    const WsLayout w = ws_layout(&c);
    const TrainWs t(&c);
    const int64_t D = c.hidden;
    if (!w.train) {
        CHECK(t.total == w.total() && t.slots == t.total && t.plane_max == -1);
        return;
    }
    const int64_t slot = is_bf16(&c) ? 4 * (int64_t)kSlotBFloats : (int64_t)kSlotFloats;
    const int64_t n_jobs = built_counts(c).n_jobs;
    const bool two = is_split2(&c);
    CHECK(t.slots == w.total() && t.merged_w == t.slots + n_jobs * slot && t.merged_b == t.merged_w + D / 2 * D);
    CHECK(t.slots < t.merged_w && t.merged_w < t.merged_b && t.merged_b + D / 2 <= t.total);
    CHECK(t.slots % 4 == 0 && t.merged_w % 4 == 0 && t.merged_b % 4 == 0 && t.total % 4 == 0);
    CHECK(t.total == w.total() + n_jobs * slot + D / 2 * D + D / 2 + (two ? 32 : 0));      // nnr_workspace_floats as include/nnr.h describes it
    if (two) CHECK(t.plane_max == t.total - 32 && t.plane_max == t.merged_b + D / 2 && t.plane_max % 4 == 0);
    else CHECK(t.plane_max == -1 && t.total == t.merged_b + D / 2);
}

int main() {
    std::vector<nnr_cfg> grid;
    for (int D : {128, 256})
        for (uint32_t mode : kModes)
            for (auto& s : kShapes) grid.push_back(nnr_cfg{s[0], s[1], D, mode | NNR_F_TRAIN});
    size_t plans = 0;
    for (bool bundles : {false, true})
        for (int max_blocks : {2, 256}) {
            PlanKnobs k;      // the defaults, not the environment
            k.bundles = bundles;
            k.max_blocks = max_blocks;
            for (const nnr_cfg& c : grid) {
                std::snprintf(g_ctx, sizeof(g_ctx), "D=%d flags=0x%x R=%d N=%d bundles=%d max_blocks=%d", c.hidden, c.flags, c.n_rays, c.n_samples, (int)bundles, max_blocks);
                size_t n = 0;
                if (is_bf16(&c)) {
                    const BPlan p = build_plan_bf16(&c, k);
                    check_plan(c, k, p);
                    const auto blob = serialise(p, &n);
                    CHECK(n == p.jobs.size() * sizeof(WgradJobB) + p.block_first.size() * 4 + p.outs.size() * sizeof(WgradOutB));
                    CHECK(p.outs.empty() || !std::memcmp(blob.get() + n - sizeof(WgradOutB), &p.outs.back(), sizeof(WgradOutB)));
                } else {
                    const Plan p = build_plan(&c, k);
                    check_plan(c, k, p);
                    const auto blob = serialise(p, &n);
                    int32_t trailer[4];
                    std::memcpy(trailer, blob.get() + n - sizeof(trailer), sizeof(trailer));
                    CHECK(trailer[0] == kPlanMagic && trailer[1] == (int32_t)p.jobs.size() && trailer[2] == (int32_t)p.wave_first.size() - 1 &&
                          trailer[3] == (int32_t)p.heads.size());
                    int32_t n_heads;      // behind the wave table: where nnr_mlp_wgrad's `heads = wave_first + n_waves + 2` starts, minus one
                    std::memcpy(&n_heads, blob.get() + p.jobs.size() * sizeof(WgradJob) + p.wave_first.size() * 4, 4);
                    CHECK(n_heads == trailer[3]);
                }
                ++plans;
            }
        }
    // plan_counts and its memo (the process's knobs): alternate two cfgs -- a miss, a miss, then the same pair again, and one cfg twice in a row (a hit)
    for (size_t i = 0; i < grid.size(); ++i) {
        const nnr_cfg &a = grid[i], &b = grid[(i + 7) % grid.size()];
        std::snprintf(g_ctx, sizeof(g_ctx), "plan_counts / TrainWs %zu: D=%d flags=0x%x R=%d N=%d", i, a.hidden, a.flags, a.n_rays, a.n_samples);
        const PlanCounts ca = built_counts(a), cb = built_counts(b);
        for (int round = 0; round < 2; ++round) {
            CHECK(same(plan_counts(&a), ca));
            CHECK(same(plan_counts(&a), ca));
            CHECK(same(plan_counts(&b), cb));
        }
        nnr_cfg other = a;      // same plan, another cfg: the rendering switches are not part of the key, the mode bits are
        other.flags |= NNR_F_WHITE_BG | NNR_F_RELU_SIGMA;
        CHECK(same(plan_counts(&other), ca));
        check_ws(a);
        nnr_cfg infer = a;
        infer.flags &= ~(uint32_t)NNR_F_TRAIN;
        check_ws(infer);
        check_ws(a);
    }
    std::printf("plan_check: %zu plans, %zu cfgs, %d failed\n", plans, grid.size(), g_failed);
    return g_failed ? 1 : 0;
}
