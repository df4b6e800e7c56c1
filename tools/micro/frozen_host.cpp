// frozen_host.cpp -- the host helpers of csrc/nnr_frozen_api.cpp (the workspace layout, check_cfg, the entry points' refusals) and of
// csrc/nnr_grid_check.h in a stand-alone program, for a run under the host sanitizers; no GPU, no launch.  From the repository's root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Inope-nerf_amd/csrc -Iinclude -x hip -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tools/micro/frozen_host.cpp -o tools/micro/frozen_host && tools/micro/frozen_host
// It walks the cfg cases of oracle/frozen_refusals.py and more (every flag combination, sizes around the int32 bound), and for every cfg
// checks the two workspaces' planes against the list written out here: back to back, the sparse workspace the frozen one with five int32
// planes behind it.  The unit is included as text, its launchers are stubs that abort: every call below is refused before it gets to one.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "nnr_frozen_sparse_kernels.h"

namespace nnr {      // (the specialisations stand in front of the unit that calls them)
static hipError_t reached(const char* what) { std::fprintf(stderr, "frozen_host: %s was reached\n", what); std::abort(); }
template <> hipError_t launch_mlp_fwd_frozen_variant<128>(const MlpFwdArgs&, hipStream_t) { return reached("a launcher"); }
template <> hipError_t launch_mlp_fwd_frozen_variant<256>(const MlpFwdArgs&, hipStream_t) { return reached("a launcher"); }
template <> hipError_t launch_mlp_dgrad_frozen_variant<128>(const MlpDgradArgs&, hipStream_t) { return reached("a launcher"); }
template <> hipError_t launch_mlp_dgrad_frozen_variant<256>(const MlpDgradArgs&, hipStream_t) { return reached("a launcher"); }
template <> hipError_t launch_mlp_fwd_frozen_list_variant<128>(const MlpFwdListArgs&, hipStream_t) { return reached("a launcher"); }
template <> hipError_t launch_mlp_fwd_frozen_list_variant<256>(const MlpFwdListArgs&, hipStream_t) { return reached("a launcher"); }
template <> hipError_t launch_mlp_dgrad_frozen_list_variant<128>(const MlpDgradListArgs&, hipStream_t) { return reached("a launcher"); }
template <> hipError_t launch_mlp_dgrad_frozen_list_variant<256>(const MlpDgradListArgs&, hipStream_t) { return reached("a launcher"); }
hipError_t launch_frozen_sparse_compact(const FrozenSparseArgs&, hipStream_t) { return reached("a launcher"); }
hipError_t launch_composite_fwd(const CompositeArgs&, hipStream_t) { return reached("a launcher"); }
hipError_t launch_composite_bwd(const CompositeArgs&, hipStream_t) { return reached("a launcher"); }
hipError_t launch_ray_reduce(const RayReduceArgs&, hipStream_t) { return reached("a launcher"); }
int chunks_per_ray(const nnr_cfg*) { return (int)reached("chunks_per_ray"); }
int launched(hipError_t) { return (int)reached("launched"); }
}  // namespace nnr

#include "nnr_frozen_api.cpp"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "frozen_host: %s:%d: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

static long g_cfgs = 0, g_calls = 0;

static void walk_cfg(const nnr_cfg& c) {
    ++g_cfgs;
    const bool sizes = c.n_rays > 0 && c.n_samples > 0;
    const uint32_t need = NNR_F_TRAIN | NNR_F_SPLIT3 | NNR_F_SPLIT2;
    const bool kernels = (c.hidden == 128 || c.hidden == 256) && c.n_samples <= 1024 && !(c.flags & NNR_F_BF16) && (c.flags & need) == need;
    const int64_t S = (int64_t)c.n_rays * c.n_samples, S_pad = (S + 127) / 128 * 128;
    const int want[2] = {!sizes ? NNR_E_BADCFG : !kernels ? NNR_E_UNSUPPORTED : NNR_OK,
                         !sizes ? NNR_E_BADCFG : (!kernels || S_pad > INT32_MAX) ? NNR_E_UNSUPPORTED : NNR_OK};
    const int ids[13] = {0, 1, 2, 3, 4, 10, 19, 25, NNR_FS_LIVE, NNR_FS_RAY_OFF, NNR_FS_N_LIVE, NNR_FS_RAY_COUNT, NNR_FS_RAY_MASK};
    const int64_t words[13] = {4 * S_pad, S_pad, 4 * S_pad, 4 * S_pad, 4 * S_pad, 64 * S_pad, 32 * S_pad, 18 * (c.hidden / 64) * S_pad,
                               S_pad, c.n_rays, 1, c.n_rays, 32 * (int64_t)c.n_rays};
    const int pitches[13] = {4, 1, 4, 4, 4, 64, 32, 18 * (c.hidden / 64), 1, 1, 1, 1, 32};
    float* const fake = reinterpret_cast<float*>(0x10000);
    float* const odd = reinterpret_cast<float*>(0x10002);
    for (int sparse = 0; sparse < 2; ++sparse) {
        REQUIRE(check_cfg(&c, sparse) == want[sparse]);
        const int n = sparse ? 13 : 8;
        const size_t floats = sparse ? nnr_frozen_sparse_workspace_floats(&c) : nnr_frozen_workspace_floats(&c);
        int64_t off = 0;
        for (int i = 0; i < 13; ++i) {
            int32_t pitch = -7;
            const int64_t got = sparse ? nnr_frozen_sparse_ws_plane(&c, ids[i], &pitch) : nnr_frozen_ws_plane(&c, ids[i], &pitch);
            if (want[sparse] != NNR_OK) REQUIRE(got == -1 && pitch == -7);
            else if (i < n) REQUIRE(got == off && pitch == pitches[i]);
            else REQUIRE(got == -1 && pitch == 0);
            if (i < n) off += words[i];
        }
        REQUIRE(floats == (want[sparse] == NNR_OK ? (size_t)off : 0));
        for (int pl : {-2, -1, 5, 11, 20, 31, 40, 99, 105, 1000}) {
            int32_t pitch = -7;
            REQUIRE((sparse ? nnr_frozen_sparse_ws_plane(&c, pl, &pitch) : nnr_frozen_ws_plane(&c, pl, &pitch)) == -1);
            REQUIRE(pitch == (want[sparse] == NNR_OK ? 0 : -7));
        }
        // the entry points: a misaligned workspace is the last thing they refuse
        const int rc = sparse ? nnr_frozen_sparse_bwd(&c, fake, fake, fake, fake, fake, fake, odd, nullptr)
                              : nnr_frozen_bwd(&c, fake, fake, fake, fake, fake, fake, odd, nullptr);
        REQUIRE(rc == (want[sparse] == NNR_OK ? NNR_E_ALIGN : want[sparse]));
        const int rf = sparse ? NNR_OK : nnr_frozen_fwd(&c, fake, fake, fake, fake, fake, nullptr, fake, fake, fake, nullptr, nullptr, odd, nullptr);
        REQUIRE(sparse || rf == rc);
        g_calls += 2;
    }
}

static int grid_code(float lo, float inv, int nx, int ny, int nz, const nnr_cfg& c) {
    const float lo3[3] = {-1.f, lo, -1.f}, inv3[3] = {8.f, 8.f, inv};
    const int32_t dims[3] = {nx, ny, nz};
    int64_t wx = -1;
    const int rc = nnr::check_grid(lo3, inv3, dims, &wx);
    REQUIRE(rc != NNR_OK || wx == ((int64_t)nx + 31) / 32);
    float* const fake = reinterpret_cast<float*>(0x10000);
    const uint32_t* const bits = reinterpret_cast<const uint32_t*>(0x20000);
    int32_t* const odd = reinterpret_cast<int32_t*>(0x30001);      // opt_n_live off by one: the entry point's very last refusal
    const int full = nnr_frozen_sparse_fwd(&c, fake, fake, fake, fake, fake, nullptr, lo3, inv3, dims, bits, fake, fake, fake, nullptr, nullptr,
                                           nullptr, nullptr, odd, fake, nullptr);
    REQUIRE(full == (rc == NNR_OK ? NNR_E_ALIGN : rc));
    ++g_calls;
    return rc;
}

int main() {
    for (int hidden : {0, 64, 128, 192, 256, 512})
        for (int n_samples : {-1, 0, 1, 33, 130, 256, 257, 1024, 1025})
            for (int n_rays : {-1, 0, 1, 5, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, (1 << 23) + 1, INT32_MAX})
                for (uint32_t flags = 0; flags < 128; ++flags) walk_cfg(nnr_cfg{n_rays, n_samples, hidden, flags});
    REQUIRE(check_cfg(nullptr, false) == NNR_E_BADCFG && check_cfg(nullptr, true) == NNR_E_BADCFG);
    REQUIRE(nnr_frozen_workspace_floats(nullptr) == 0 && nnr_frozen_sparse_ws_plane(nullptr, 0, nullptr) == -1);

    const nnr_cfg good{5, 130, 128, NNR_F_TRAIN | NNR_F_SPLIT3 | NNR_F_SPLIT2};
    const float nan = std::nanf(""), inf = INFINITY;
    REQUIRE(grid_code(-1.f, 8.f, 16, 16, 16, good) == NNR_OK);
    for (float lo : {nan, inf, -inf}) REQUIRE(grid_code(lo, 8.f, 16, 16, 16, good) == NNR_E_BADCFG);
    for (float inv : {0.f, -2.f, nan, inf}) REQUIRE(grid_code(-1.f, inv, 16, 16, 16, good) == NNR_E_BADCFG);
    for (int d : {0, -1, INT32_MIN}) {
        REQUIRE(grid_code(-1.f, 8.f, d, 16, 16, good) == NNR_E_BADCFG && grid_code(-1.f, 8.f, 16, d, 16, good) == NNR_E_BADCFG);
        REQUIRE(grid_code(-1.f, 8.f, 16, 16, d, good) == NNR_E_BADCFG);
    }
    REQUIRE(grid_code(-1.f, 8.f, 32, 1 << 16, 1 << 16, good) == NNR_E_UNSUPPORTED);       // rows
    REQUIRE(grid_code(-1.f, 8.f, 1, 1 << 16, 1 << 15, good) == NNR_E_UNSUPPORTED);
    REQUIRE(grid_code(-1.f, 8.f, 1 << 26, 1 << 10, 1, good) == NNR_E_UNSUPPORTED);        // words
    REQUIRE(grid_code(-1.f, 8.f, 1 << 16, 1 << 16, 2, good) == NNR_E_UNSUPPORTED);        // cells
    REQUIRE(grid_code(-1.f, 8.f, 1 << 30, 2, 1, good) == NNR_E_UNSUPPORTED);
    REQUIRE(grid_code(-1.f, 8.f, INT32_MAX, INT32_MAX, INT32_MAX, good) == NNR_E_UNSUPPORTED);      // (rows < 2^62: no overflow on the way)
    REQUIRE(grid_code(-1.f, 8.f, INT32_MAX, 1, 1, good) == NNR_OK && grid_code(-1.f, 8.f, 1, INT32_MAX, 1, good) == NNR_OK);
    REQUIRE(grid_code(nan, 8.f, 1 << 16, 1 << 16, 2, good) == NNR_E_BADCFG);              // a bad grid before an unsupported one
    std::printf("frozen_host: %ld cfgs, %ld entry-point calls, all as expected\n", g_cfgs, g_calls);
    return 0;
}
