// nnr_wgrad_plan.h -- the host side of the weight gradient: the two planners (fp32 / term-split modes: Plan; bf16 mode: BPlan), the
// blob they are serialised into, and the training workspace's regions behind the planes.  Pure host arithmetic: this unit includes no HIP
// header, so a stand-alone program can build, print and check a plan on a CPU (tests/host/plan_check.cpp).
// State: the process-constant knobs (process_knobs) and plan_counts' one-entry memo per thread; everything else is a function of its arguments.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/nnr.h"
#include "nnr_layout.h"

namespace nnr {

// ---- what a cfg selects ---------------------------------------------------------------------------------------------------------
WsLayout ws_layout(const nnr_cfg* c);
inline bool is_bf16(const nnr_cfg* c) { return (c->flags & NNR_F_BF16) != 0; }
inline bool is_split3(const nnr_cfg* c) { return (c->flags & (NNR_F_BF16 | NNR_F_SPLIT3)) == NNR_F_SPLIT3; }
inline bool is_split2(const nnr_cfg* c) { return is_split3(c) && (c->flags & NNR_F_SPLIT2) != 0; }      // forward / input gradient with two-term fp16 operands (nnr_split2.h)
inline int weight_mode(const nnr_cfg* c) { return is_bf16(c) ? 1 : (is_split2(c) ? 3 : (is_split3(c) ? 2 : 0)); }   // Layout<D, MODE>

constexpr int kMaxBlocks = 256;   // one 4-wave workgroup per CU: the kernel needs the whole register file, and every
                                  // workgroup must be resident at once (a 257th would run as a second round)
constexpr int kGranule = 16;      // samples per loop iteration of the wgrad kernel (two stages of kU = 4 sample pairs)
constexpr int kMinGranulesPerBlock = 16;  // small problems use fewer workgroups: a job costs a 64 KB slot + its flush (~2 us),
                                          // a granule of a 4x4 tile ~3.4 us of MFMA, so 16 granules keep the flush under 4 %
constexpr int64_t kMinTapePerBlock = 16 * 32;   // KiB (bf16 plan): at least ~16 full stages per workgroup, or the ring never fills

// ---- the knobs that shape a plan: environment variables for experiments, read ONCE per process (process_knobs) -- a plan built under one
// setting never meets a launch that assumes another.  from_env() is the only getenv of this unit; the planners take the knobs as an argument.
struct PlanKnobs {
    // NNR_WGRAD_SPLIT_WEIGHT (>= 50).  Three-term mode (nnr_wgrad.hip, wgrad_job_split): the 4 x 4 tiles run on the bf16 matrix pipe, the narrow ones
    // still on fp32 MFMAs -- per MFMA-equivalent a 4 x 4 tile costs split_w / 1000 of what it costs in fp32.  (round 4, shared split, row-major
    // activations: 1.18 / 1.16 / 1.14 / 1.11 / 1.12 ms at 360 / 400 / 440 / 480 / 520; both operands tile-major: 1.12 / 1.11 / 1.10 / 1.11 at 380 /
    // 420 / 440 / 460, 1.14 at 480 on another box where 440 gave 1.11 -- profiles/r04/r*_wgrad_weight_sweep_tile_x.txt)
    int split_w = 440;
    // NNR_WGRAD_SPLIT2_WEIGHT (>= 50).  Two-term mode: the workgroup jobs take three fp16 MFMAs per product instead of six bf16 ones (wgrad_group_split2):
    // cheaper again, relative to a narrow fp32 tile.  (profiles/r06/h_wgrad_f16_plan_weight_sweep.txt, in sequence with the other kernels: 0.974 /
    // 0.941 / 0.926 / 0.918 / 0.947 ms at 280 / 300 / 320 / 340 / 360)
    int split2_w = 340;
    // NNR_WGRAD_ENC2_WEIGHT (>= 0).  Two-term mode: the 128 x 64 tiles against the position encoding as private two-term jobs (wgrad_job_enc2) -- their
    // weight relative to a narrow fp32 tile; 0: leave them on fp32 MFMAs.  (profiles/r06/t2_wgrad_enc2_weight_sweep.txt, kernel in sequence: 0.930 ms
    // without the jobs; 0.915 / 0.879 / 0.884 / 0.894 / 0.897 at 550 / 600 / 650 / 700 / 750 -- a cliff below the job's true cost, a gentle slope above)
    int enc2_w = 625;
    bool f16_off = false;     // NNR_WGRAD_BF16_TERMS (= nnr_wgrad.hip's): the six-term workgroup jobs in the two-term mode
    bool fp32 = false;        // NNR_WGRAD_FP32 (= nnr_wgrad.hip's): fp32 MFMAs in the weight gradient of the term-split modes
    bool bundles = false;     // NNR_WGRAD_BUNDLES: class B at D = 256 per workgroup (build_plan: a measured negative, hence off)
    int max_blocks = kMaxBlocks;   // NNR_WGRAD_MAX_BLOCKS, as given: tuning knob for experiments; build_plan uses at least 2, build_plan_bf16 at least 1
    bool no_coop = false;     // NNR_WGRAD_NO_COOP: the class-A segments as four private jobs instead of one workgroup job
    bool no_merge = false;    // NNR_WGRAD_NO_MERGE: profiling knob of the bf16 plan -- the two-plane units as separate passes
    static PlanKnobs from_env();
};
const PlanKnobs& process_knobs();

// ---- fp32 / three-term / two-term modes: wave jobs (nnr_wgrad.hip) ---------------------------------------------------------------
struct Unit {  // a wave tile before the split over samples
    WgradJob j;
    int group;  // units of one group share operands: same-k jobs are placed in one workgroup
};
std::vector<Unit> wgrad_units(int D);

struct Plan {
    std::vector<WgradJob> jobs;        // grouped by wave: wave w runs jobs [wave_first[w], wave_first[w+1])
    std::vector<int32_t> wave_first;   // n_waves + 1 entries, n_waves a multiple of 4
    std::vector<int32_t> heads;        // job index of split 0 of every tile: the reduction kernel launches 16 workgroups per HEAD, not per job
};
Plan build_plan(const nnr_cfg* c, const PlanKnobs& k);

// ---- bf16 mode: workgroup jobs (nnr_wgrad_bf16.hip) ------------------------------------------------------------------------------
struct BUnit {
    int d_plane, d_g0, d_groups, x_plane, x_g0, x_groups, MT, NT, WR, WC, bias;
    int x2_plane = -1, x2_groups = 0;     // a second activation plane behind the first (x_groups even): one pass over the gradient
};
struct BPlan {
    std::vector<WgradJobB> jobs;
    std::vector<int32_t> block_first;   // n_blocks + 1
    std::vector<WgradOutB> outs;
};
void bf16_units(int D, bool no_merge, std::vector<BUnit>& units, std::vector<WgradOutB>& outs);
BPlan build_plan_bf16(const nnr_cfg* c, const PlanKnobs& k);

// ---- the blob nnr_plan_build hands out (part of the ABI: the kernels index it) ---------------------------------------------------
// Plan:  WgradJob[n_jobs], int32 wave_first[n_waves + 1], int32 n_heads, int32 heads[n_heads], then the trailer the weight-gradient kernel checks
//        before it trusts the blob (a blob of another ABI, shape or plan setting makes it trap instead of indexing the job table with garbage):
//        int32 {kPlanMagic, n_jobs, n_waves, n_heads}
// BPlan: WgradJobB[n_jobs], int32 block_first[n_blocks + 1], WgradOutB[n_outs]
constexpr int32_t kPlanMagic = 0x4e4e5235;      // 'NNR5' (= nnr_wgrad.hip's)
size_t plan_bytes(const Plan& p);
size_t plan_bytes(const BPlan& p);
void write_plan(const Plan& p, void* out);      // exactly plan_bytes(p) bytes
void write_plan(const BPlan& p, void* out);

// ---- what the entry points need of a plan: its counts.  One-entry memo per thread, keyed on all the plan depends on (hidden, S_pad, the mode
// bits TRAIN | BF16 | SPLIT3 | SPLIT2; the knobs are process constants): a training loop repeats one cfg, so its launches build no plan.
struct PlanCounts {
    int n_jobs, n_waves_or_blocks, n_heads_or_outs;      // Plan: jobs, waves, heads; BPlan (NNR_F_BF16): jobs, workgroups, outputs
};
PlanCounts plan_counts(const nnr_cfg* c);

// ---- the workspace behind the planes (float offsets; WsLayout::total() floats of planes come first) -------------------------------
// training: one partial slot per weight-gradient job (bf16 mode: four wave slots per workgroup job), then dW' (D/2 x D) and db' (D/2) of the
// merged colour matrix; two-term mode: the planes' maxima behind everything else (include/nnr.h).  Inference: the planes alone.
constexpr int kPlaneMaxWsFloats = 32;      // (= nnr_kernels.h's kPlaneMaxFloats: nnr_api.cpp asserts it)
struct TrainWs {
    int64_t slots, merged_w, merged_b;
    int64_t plane_max;      // -1: none (every mode but two-term training)
    int64_t total;
    explicit TrainWs(const nnr_cfg* c);
};

}  // namespace nnr
