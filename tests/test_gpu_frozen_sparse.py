"""GPU (-m gpu): the sparse frozen-field render (include/nnr_frozen_sparse.h) against the dense frozen-field render it
thins out.  Through the C ABI with own buffers (the workspace starts as NaN, sentinels behind it), on tests/test_gpu_frozen.py's inputs and
seeds.  Statements: with every bit set, and wherever every culled sample's alpha is exactly 0 in the dense render (ReLU density), all seven
results are the dense ones BIT FOR BIT; under softplus the results are the float64 restatement's (tests/frozen_sparse_ref.py) at
tests/test_gpu_sparse.py's bar, and what the compositor hands the list-driven input gradient is as close to float64 as the dense one's."""
import contextlib
import ctypes as C
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nope-nerf_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

import frozen_sparse_ref as FS      # noqa: E402
import sparse_ref as SR             # noqa: E402
from test_gpu_frozen import OUT_KEYS, SENTINELS, _inputs, _params, counted      # noqa: E402,F401  (its inputs, seeds and call counter)

pytestmark = pytest.mark.gpu
BAR = 1e-4      # tests/test_gpu_sparse.py's: 1e-4 max(1, |ref|)
P_OUT4, P_DOUT4 = 0, 2
F64 = torch.float64


class Grid:
    """what render_sparse and the frozen operator take: lo, inv_step, dims = (n_x, n_y, n_z), bits"""

    def __init__(self, lo, hi, n, occ):
        self.lo, self.inv_step, self.dims = (float(lo),) * 3, (n / (float(hi) - float(lo)),) * 3, (n, n, n)
        self.bits = SR.pack_bits(occ).cuda()


def _grid64(occ=None, fill=True):
    """the issue's grid: 64^3 cells over [-11, 11]^3 (every sample of _inputs lies inside: |o| small, |d| = 1, z <= 10)"""
    return Grid(-11., 11., 64, occ if occ is not None else torch.full((64, 64, 64), bool(fill)))


def _plane(lib, fn, cfg, ws, plane, rows):
    pitch = C.c_int32(0)
    off = fn(C.byref(cfg), plane, C.byref(pitch))
    assert off >= 0
    return ws[off:off + rows * pitch.value].view(rows, pitch.value).clone()


def _run(D, R, N, dist_alpha, relu_sigma, inp, w, b, grid=None):
    """The dense frozen path (grid None: nnr_frozen_fwd + nnr_frozen_bwd) or the sparse one on `grid`, own buffers, the workspace NaN with
    SENTINELS words behind its end that must survive -> the seven results, P_OUT4 and P_DOUT4 as (R,N,4), and count / live / n_live."""
    from nnr import lib as L
    lib = L.load()
    dev = torch.device("cuda")
    cfg = L.make_cfg(R, N, D, dist_alpha=dist_alpha, relu_sigma=relu_sigma, train=True)
    assert cfg.flags & L.NNR_F_SPLIT2
    st = L.stream()
    packed = torch.empty(lib.nnr_packed_floats(C.byref(cfg)), device=dev)
    L.check(lib.nnr_pack_weights(C.byref(cfg), C.byref(L.params_struct(w, b)), L.ptr(packed), st), "pack")
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(rgb=torch.empty(R, 3, **f32), dist=torch.empty(R, **f32), alpha=torch.empty(R, N, **f32), z=torch.empty(R, N, **f32),
               d_pts_o=torch.empty(R, 3, **f32), d_pts_d=torch.empty(R, 3, **f32), d_view=torch.empty(R, 3, **f32))
    fwd_in = [L.ptr(inp[k]) for k in ("pts_o", "pts_d", "view_d", "z_lo", "z_hi", "jitter")]
    sizer, planer = (lib.nnr_frozen_workspace_floats, lib.nnr_frozen_ws_plane) if grid is None else \
        (lib.nnr_frozen_sparse_workspace_floats, lib.nnr_frozen_sparse_ws_plane)
    n = sizer(C.byref(cfg))
    assert n > 0
    buf = torch.full((n + SENTINELS,), float("nan"), **f32)
    mark = torch.arange(SENTINELS, **f32) + 0.5
    buf[n:] = mark
    ws = buf[:n]
    outs = [L.ptr(out[k]) for k in ("rgb", "dist", "alpha", "z")]
    bwd = [L.ptr(packed), L.ptr(inp["d_rgb"]), L.ptr(inp["d_dist"]), L.ptr(out["d_pts_o"]), L.ptr(out["d_pts_d"]), L.ptr(out["d_view"]), L.ptr(ws), st]
    if grid is None:
        L.check(lib.nnr_frozen_fwd(C.byref(cfg), *fwd_in, L.ptr(packed), *outs, L.ptr(ws), st), "nnr_frozen_fwd")
        L.check(lib.nnr_frozen_bwd(C.byref(cfg), *bwd), "nnr_frozen_bwd")
    else:
        out["count"] = torch.full((R,), -7, dtype=torch.int32, device=dev)
        out["live"] = torch.full((R * N,), -1, dtype=torch.int32, device=dev)
        out["n_live"] = torch.full((1,), -7, dtype=torch.int32, device=dev)
        lo3, is3, d3 = (C.c_float * 3)(*grid.lo), (C.c_float * 3)(*grid.inv_step), (C.c_int32 * 3)(*grid.dims)
        L.check(lib.nnr_frozen_sparse_fwd(C.byref(cfg), *fwd_in, lo3, is3, d3, L.ptr(grid.bits), L.ptr(packed), *outs, L.ptr(out["count"]),
                                          L.ptr(out["live"]), L.ptr(out["n_live"]), L.ptr(ws), st), "nnr_frozen_sparse_fwd")
        L.check(lib.nnr_frozen_sparse_bwd(C.byref(cfg), *bwd), "nnr_frozen_sparse_bwd")
    torch.cuda.synchronize()
    assert torch.equal(buf[n:], mark), "the path wrote behind its workspace"
    out["out4"] = _plane(lib, planer, cfg, ws, P_OUT4, R * N).view(R, N, 4)
    out["dout4"] = _plane(lib, planer, cfg, ws, P_DOUT4, R * N).view(R, N, 4)
    if grid is not None:
        k = int(out["n_live"])
        assert 0 <= k <= R * N and bool((out["live"][k:] == -1).all())      # nothing behind the list's end was copied as an index ... of ours
        out["live"] = out["live"][:k].cpu().long()
    return out


def _same(got, want, keys=OUT_KEYS):
    for k in keys:
        assert torch.equal(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))


def _cells(D, R, N, inp, w, b, grid):
    """every sample's cell, from the sparse inference render's own lookup"""
    from nnr import ops
    res = ops.render_sparse(inp["pts_o"], inp["pts_d"], inp["view_d"], inp["z_lo"], inp["z_hi"], inp["jitter"], grid, w, b, hidden=D,
                            dist_alpha=False, white_bg=False, relu_sigma=False, debug=True)
    return res[4].cpu().long()


def _grid_of(cell, keep):
    """64^3 bits: exactly the cells that hold a sample with keep (R,N) set"""
    assert bool((cell >= 0).all())      # (the grid holds every sample)
    occ = torch.zeros(64 * 64 * 64, dtype=torch.bool)
    occ[cell[keep]] = True
    return _grid64(occ.view(64, 64, 64))


def _expected_list(grid, cell, dist_alpha):
    live = FS.live_rule(SR.live_ref(grid.bits, cell, grid.dims), dist_alpha)
    return live, torch.nonzero(live.reshape(-1)).reshape(-1)


def _culling_is_real(live):
    share = 1. - float(live.float().mean())
    assert 0.2 <= share <= 0.8, share
    assert bool(live.any(1).all()) and bool((~live).any(1).all())      # every ray has both kinds of sample
    return share


# ------------------------------------------------------------------------------------------------------------ 1: every bit set
# (rays, samples, dist_alpha, jitter): flat with padded chunks; two shapes the dense path runs in ray mode (this path runs flat); flat
ALL_SET = [(5, 130, False, True), (8, 64, False, False), (4, 64, True, False), (3, 33, False, False)]


@pytest.mark.parametrize("case", ALL_SET, ids=["flat_5x130", "ray_8x64", "ray_4x64_dist_alpha", "flat_3x33"])
@pytest.mark.parametrize("D", [128, 256])
def test_with_every_bit_set_the_render_is_the_dense_frozen_render_bit_for_bit(D, case):
    R, N, dist_alpha, jitter = case
    inp = _inputs(R, N, jitter, seed=100 * D + R)
    w, b = _params(D, seed=D + N)
    dense = _run(D, R, N, dist_alpha, False, inp, w, b)
    got = _run(D, R, N, dist_alpha, False, inp, w, b, _grid64())
    for k in OUT_KEYS:
        assert torch.isfinite(dense[k]).all(), k
    _same(got, dense)
    assert torch.equal(got["live"], torch.arange(R * N)) and torch.equal(got["count"].cpu(), torch.full((R,), N, dtype=torch.int32))
    assert torch.equal(got["out4"], dense["out4"]) and torch.equal(got["dout4"], dense["dout4"])
    assert float(dense["d_pts_d"].abs().max()) > 0.0      # (the comparison is not of zeros)


# ------------------------------------------------------------------------------------------------------------ 2: exact equality under culling
@functools.lru_cache(maxsize=None)
def _relu_scene(D, R, N, dist_alpha, jitter):
    """ReLU density, the density bias lowered by the median raw of the dense render: about half of the samples have raw <= 0, alpha exactly 0.
    The grid: exactly the cells that hold a sample with raw > 0 (or NaN).  -> inputs, parameters, the dense run, the grid, every cell."""
    from nnr import lib as L
    inp = _inputs(R, N, jitter, seed=100 * D + R)
    w, b = _params(D, seed=D + N)
    first = _run(D, R, N, dist_alpha, True, inp, w, b)
    i = L.LAYER_NAMES.index("fc_density")
    b = list(b)
    b[i] = (b[i] - first["out4"][..., 3].flatten().nanmedian()).contiguous()
    dense = _run(D, R, N, dist_alpha, True, inp, w, b)
    raw = dense["out4"][..., 3].cpu()
    cell = _cells(D, R, N, inp, w, b, _grid64())
    return inp, w, b, dense, _grid_of(cell, (raw > 0) | torch.isnan(raw)), cell


@pytest.mark.parametrize("R,N,jitter", [(5, 130, True), (8, 64, False)], ids=["5x130_jitter", "8x64"])
@pytest.mark.parametrize("dist_alpha", [False, True], ids=["", "dist_alpha"])
@pytest.mark.parametrize("D", [128, 256])
def test_culling_samples_without_matter_changes_no_bit(D, dist_alpha, R, N, jitter, capsys):
    inp, w, b, dense, grid, cell = _relu_scene(D, R, N, dist_alpha, jitter)
    got = _run(D, R, N, dist_alpha, True, inp, w, b, grid)
    live, want_list = _expected_list(grid, cell, dist_alpha)
    share = _culling_is_real(live)
    with capsys.disabled():
        print("\n  [frozen sparse, exact] D=%d %dx%d dist_alpha=%d: %.1f %% culled, n_live %d" % (D, R, N, dist_alpha, 100 * share, len(want_list)))
    assert torch.equal(got["live"], want_list) and torch.equal(got["count"].cpu().long(), live.sum(1))
    assert torch.equal(got["alpha"].cpu()[~live], torch.zeros(int((~live).sum())))      # alpha == 0 exactly on the culled samples
    assert torch.equal(dense["alpha"].cpu()[~live], torch.zeros(int((~live).sum())))    # (and the dense render agrees: the premise)
    for k in OUT_KEYS:
        assert torch.isfinite(dense[k]).all(), k
    _same(got, dense)
    assert torch.equal(got["out4"].cpu()[live], dense["out4"].cpu()[live])
    e = got["out4"].cpu()[~live]
    assert bool((e[:, :3] == 0).all()) and bool((e[:, 3] == float("-inf")).all())       # the substitute (0, 0, 0, E)
    assert float(dense["d_pts_d"].abs().max()) > 0.0 and float(dense["d_view"].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------ 3: softplus
@functools.lru_cache(maxsize=None)
def _softplus_scene(D, R, N, jitter):
    inp = _inputs(R, N, jitter, seed=100 * D + R)
    w, b = _params(D, seed=D + N)
    dense = _run(D, R, N, False, False, inp, w, b)
    raw = dense["out4"][..., 3].cpu()
    cell = _cells(D, R, N, inp, w, b, _grid64())
    return inp, w, b, dense, _grid_of(cell, (raw > raw.flatten().nanmedian()) | torch.isnan(raw)), cell


def _rel_l2(a, ref):
    return float((a.to(F64) - ref).norm() / ref.norm())


@pytest.mark.parametrize("R,N,jitter", [(5, 130, True), (8, 64, False)], ids=["5x130_jitter", "8x64"])
@pytest.mark.parametrize("D", [128, 256])
def test_softplus_render_meets_the_float64_restatement(D, R, N, jitter, capsys):
    """Measured on the MI355X (relative L2 over the live rows of P_DOUT4 against float64 autograd; sparse | dense): see DESIGN.md section 15."""
    inp, w, b, dense, grid, cell = _softplus_scene(D, R, N, jitter)
    got = _run(D, R, N, False, False, inp, w, b, grid)
    live, want_list = _expected_list(grid, cell, False)
    _culling_is_real(live)
    assert torch.equal(got["live"], want_list)
    for k in OUT_KEYS + ("out4",):
        assert torch.isfinite(got[k].cpu()[live] if k == "out4" else got[k]).all(), k      # E leaks no NaN
    assert torch.isfinite(got["dout4"].cpu()[live]).all()
    ref = FS.render(dense["out4"], dense["z"], live)
    for k in ("rgb", "dist"):
        err = (got[k].cpu().to(F64) - ref[k]).abs()
        assert bool((err <= BAR * ref[k].abs().clamp(min=1.)).all()), (k, float(err.max()))
    assert torch.equal(got["out4"].cpu()[live], dense["out4"].cpu()[live])
    assert torch.equal(got["alpha"].cpu()[live], dense["alpha"].cpu()[live]) and bool((got["alpha"].cpu()[~live] == 0).all())
    all_live = torch.ones_like(live)
    want_sparse = FS.dout4(dense["out4"], dense["z"], live, inp["d_rgb"], inp["d_dist"])
    want_dense = FS.dout4(dense["out4"], dense["z"], all_live, inp["d_rgb"], inp["d_dist"])
    d_sparse = _rel_l2(got["dout4"].cpu()[live], want_sparse[live])
    d_dense = _rel_l2(dense["dout4"].cpu()[live], want_dense[live])
    with capsys.disabled():
        print("\n  [frozen sparse, softplus] D=%d %dx%d: P_DOUT4 live rows against float64, relative L2: sparse %.3e, dense %.3e" % (D, R, N, d_sparse, d_dense))
    assert d_sparse <= 2. * d_dense, (d_sparse, d_dense)      # the same kernel and arithmetic, only terms removed
    for k in ("d_pts_o", "d_pts_d", "d_view"):
        assert float(got[k].abs().max()) > 0.


# ------------------------------------------------------------------------------------------------------------ 4: edge cases
@pytest.mark.parametrize("D", [128, 256])
def test_a_grid_that_culls_everything_gives_the_background_and_zero_gradients(D):
    R, N = 5, 130
    inp = _inputs(R, N, True, seed=100 * D + R)
    w, b = _params(D, seed=D + N)
    got = _run(D, R, N, False, False, inp, w, b, _grid64(fill=False))      # (returns: no hang; asserts the sentinels itself)
    assert int(got["n_live"]) == 0 and len(got["live"]) == 0 and not got["count"].any()
    for k in ("rgb", "dist", "alpha", "d_pts_o", "d_pts_d", "d_view"):
        assert torch.equal(got[k], torch.zeros_like(got[k])), k
    dense = _run(D, R, N, False, False, inp, w, b)
    assert torch.equal(got["z"], dense["z"])


@pytest.mark.parametrize("D", [128, 256])
def test_a_nan_origin_makes_its_ray_nan_and_leaves_the_others_alone(D):
    R, N = 7, 33
    inp = dict(_inputs(R, N, False, seed=100 * D + R))
    inp["pts_o"] = inp["pts_o"].clone()
    inp["pts_o"][3, 1] = float("nan")
    w, b = _params(D, seed=D + N)
    dense = _run(D, R, N, False, False, inp, w, b)
    got = _run(D, R, N, False, False, inp, w, b, _grid64(fill=False))      # all clear: the NaN ray is outside, hence live; the others are culled
    assert bool(torch.isnan(got["rgb"][3]).all()) and torch.equal(got["count"].cpu(), torch.tensor([0, 0, 0, N, 0, 0, 0], dtype=torch.int32))
    others = [r for r in range(R) if r != 3]
    assert bool((got["rgb"][others] == 0).all()) and bool((got["d_pts_o"][others] == 0).all())
    got = _run(D, R, N, False, False, inp, w, b, _grid64())                # all set: the dense run, the NaN ray included
    assert bool(torch.isnan(got["rgb"][3]).all())
    for k in OUT_KEYS:
        assert torch.equal(got[k][others], dense[k][others]), k


@pytest.mark.parametrize("D", [128, 256])
def test_one_ray_and_a_grid_that_holds_no_sample(D):
    for R, N in ((1, 33), (3, 33)):
        inp = _inputs(R, N, False, seed=100 * D + R)
        w, b = _params(D, seed=D + N)
        dense = _run(D, R, N, False, False, inp, w, b)
        far = Grid(100., 101., 4, torch.zeros(4, 4, 4, dtype=torch.bool))      # all clear, and nowhere near a sample: every sample is live
        for grid in ((_grid64(), far) if R == 1 else (far,)):
            got = _run(D, R, N, False, False, inp, w, b, grid)
            _same(got, dense)
            assert torch.equal(got["live"], torch.arange(R * N))


# ------------------------------------------------------------------------------------------------------------ 5: the operator
def _operator(D, R, N, *, grid, frozen=True, bf16=False, context=False, relu_sigma=True, seed=5):
    import nnr
    inp = _inputs(R, N, True, seed=seed)
    w, b = _params(D, seed=seed + 1)
    for t in w + b:
        t.requires_grad_(True)
    rays = [inp[k].clone().requires_grad_(True) for k in ("pts_o", "pts_d", "view_d")]
    kw = dict(hidden=D, dist_alpha=False, white_bg=False, relu_sigma=relu_sigma, bf16=bf16)
    if context:
        with nnr.frozen_field(occupancy=grid):
            rgb, dist, alpha, z = nnr.render_rays(*rays, inp["z_lo"], inp["z_hi"], inp["jitter"], w, b, **kw)
    else:
        rgb, dist, alpha, z = nnr.render_rays(*rays, inp["z_lo"], inp["z_hi"], inp["jitter"], w, b, frozen=frozen, occupancy=grid, **kw)
    ((rgb * inp["d_rgb"]).sum() + (dist * inp["d_dist"]).sum()).backward()
    torch.cuda.synchronize()
    return inp, w, b, dict(rgb=rgb.detach(), dist=dist.detach(), alpha=alpha, z=z, d_pts_o=rays[0].grad, d_pts_d=rays[1].grad, d_view=rays[2].grad,
                           wgrads=[t.grad for t in w + b])


@pytest.mark.parametrize("D", [128, 256])
def test_operator_with_a_grid_gives_the_abis_results_and_no_weight_gradient(D, counted):
    from nnr import ops
    R, N = 5, 130
    g = torch.Generator().manual_seed(3)
    grid = _grid64(torch.rand(64, 64, 64, generator=g) < 0.5)
    inp, w, b, keyword = _operator(D, R, N, grid=grid)
    assert counted.calls.get("nnr_frozen_sparse_fwd") == 1 and counted.calls.get("nnr_frozen_sparse_bwd") == 1, counted.calls
    for name in ("nnr_frozen_fwd", "nnr_mlp_wgrad", "nnr_render_fwd", "nnr_render_bwd", "nnr_workspace_floats", "nnr_plan_build"):
        assert name not in counted.calls, (name, counted.calls)
    _, _, _, context = _operator(D, R, N, grid=grid, frozen=None, context=True)
    abi = _run(D, R, N, False, True, inp, [t.detach() for t in w], [t.detach() for t in b], grid)
    assert 0 < int(abi["n_live"]) < R * N
    for got in (keyword, context):
        assert all(t is None for t in got["wgrads"])      # the parameters' .grad is None
        _same(got, abi)
    plain = ops.render_frozen_sparse(inp["pts_o"], inp["pts_d"], inp["view_d"], inp["z_lo"], inp["z_hi"], inp["jitter"], grid,
                                     [t.detach() for t in w], [t.detach() for t in b], hidden=D, dist_alpha=False, white_bg=False, relu_sigma=True,
                                     d_rgb=inp["d_rgb"], d_dist=inp["d_dist"], debug=True)
    torch.cuda.synchronize()
    _same(plain, abi)
    assert torch.equal(plain["count"], abi["count"]) and int(plain["n_live"]) == int(abi["n_live"])
    assert torch.equal(plain["live"][:int(plain["n_live"])].cpu().long(), abi["live"])


def test_dense_and_sparse_nodes_in_alternation_keep_their_entry_points_and_workspaces_apart():
    """One operator serves both kinds: dense, sparse, dense again on one leaf set of rays, a backward behind each.  Hidden 128, 5 rays of 33
    samples: the rays straddle the 32-sample chunks and the last workgroup is padded.  Rounds one and three are the same bits (the sparse node
    in between left nothing behind), the sparse round is render_frozen_sparse's bit for bit, and every buffer a node handed back lies in the
    pool of its own kind, at that kind's size."""
    import nnr
    from nnr import lib as L
    from nnr import ops
    D, R, N = 128, 5, 33
    inp = _inputs(R, N, True, seed=21)
    dev = inp["pts_o"].device
    w, b = _params(D, seed=22)
    g = torch.Generator().manual_seed(23)
    grid = _grid64(torch.rand(64, 64, 64, generator=g) < 0.5)
    kw = dict(hidden=D, dist_alpha=False, white_bg=False, relu_sigma=True)
    cfg = L.make_cfg(R, N, D, dist_alpha=False, white_bg=False, relu_sigma=True, train=True)
    lib = L.load()
    sizes = {"frozen": lib.nnr_frozen_workspace_floats(C.byref(cfg)), "frozen_sparse": lib.nnr_frozen_sparse_workspace_floats(C.byref(cfg))}
    assert 0 < sizes["frozen"] < sizes["frozen_sparse"]
    for kind in sizes:
        ops._ws_pool_of(cfg, dev, kind).clear()
    rays = [inp[k].clone().requires_grad_(True) for k in ("pts_o", "pts_d", "view_d")]
    rounds, pools = [], []
    for occupancy in (None, grid, None):
        for t in rays:
            t.grad = None
        rgb, dist, alpha, z = nnr.render_rays(*rays, inp["z_lo"], inp["z_hi"], inp["jitter"], w, b, frozen=True, occupancy=occupancy, **kw)
        torch.autograd.backward([rgb, dist], [inp["d_rgb"], inp["d_dist"]])
        torch.cuda.synchronize()
        rounds.append(dict(rgb=rgb.detach(), dist=dist.detach(), alpha=alpha, z=z, d_pts_o=rays[0].grad, d_pts_d=rays[1].grad, d_view=rays[2].grad))
        pools.append({kind: [(t.numel(), t.data_ptr()) for t in ops._ws_pool_of(cfg, dev, kind)] for kind in sizes})
    for n, held in enumerate(pools):      # what lies in each pool behind round n: one buffer of the kind's own size once a node of the kind has run
        assert [s for s, _ in held["frozen"]] == [sizes["frozen"]], (n, held)
        assert [s for s, _ in held["frozen_sparse"]] == ([sizes["frozen_sparse"]] if n >= 1 else []), (n, held)
    assert pools[2]["frozen"] == pools[0]["frozen"]      # round three took round one's buffer and gave it back where it was
    _same(rounds[2], rounds[0])
    plain = ops.render_frozen_sparse(inp["pts_o"], inp["pts_d"], inp["view_d"], inp["z_lo"], inp["z_hi"], inp["jitter"], grid, w, b,
                                     d_rgb=inp["d_rgb"], d_dist=inp["d_dist"], debug=True, **kw)
    torch.cuda.synchronize()
    _same(rounds[1], plain)
    assert 0 < int(plain["n_live"]) < R * N      # (the grid did cull: the sparse round is not the dense one under another name)
    assert [t.numel() for t in ops._ws_pool_of(cfg, dev, "frozen_sparse")] == [sizes["frozen_sparse"]]


def test_operator_with_a_grid_and_bf16_falls_back_and_says_so_once(counted, caplog):
    from nnr import ops
    ops._frozen_said.clear()
    grid = _grid64()
    with caplog.at_level(logging.INFO, logger="nnr"):
        _, _, _, got = _operator(256, 8, 64, grid=grid, bf16=True, relu_sigma=False)
        _operator(256, 8, 64, grid=grid, bf16=True, relu_sigma=False)
    assert "nnr_frozen_sparse_fwd" not in counted.calls and "nnr_frozen_fwd" not in counted.calls and "nnr_mlp_wgrad" not in counted.calls
    assert counted.calls.get("nnr_render_fwd") == 2
    assert all(t is None for t in got["wgrads"]) and all(torch.isfinite(got[k]).all() for k in ("d_pts_o", "d_pts_d", "d_view"))
    said = [r.getMessage() for r in caplog.records if "frozen" in r.getMessage()]
    assert len(said) == 1 and "bf16" in said[0] and "grid is ignored" in said[0]      # one line, however many calls


def test_operator_refuses_a_grid_without_a_frozen_call():
    import nnr
    inp = _inputs(4, 32, False, seed=3)
    w, b = _params(128, seed=4)
    with pytest.raises(ValueError, match="occupancy"):
        nnr.render_rays(inp["pts_o"].requires_grad_(True), inp["pts_d"], inp["view_d"], inp["z_lo"], inp["z_hi"], None, w, b, hidden=128,
                        dist_alpha=False, white_bg=False, relu_sigma=False, occupancy=_grid64())


def _refine(scene_dir, occupancy, steps=20, lr=1e-3):
    import dataloading as dl
    import model as mdl
    import train_scene
    from model import geometry
    torch.manual_seed(11)
    np.random.seed(11)
    dev = torch.device("cuda")
    cfg = train_scene.scene_cfg(scene_dir, "toy", n_rays=96, n_samples=24, hidden=128, sample_rate=10 ** 6)
    loader, fields = dl.get_dataloader(cfg, mode="train", shuffle=False)
    trainer, _, _ = train_scene.build(cfg, dev, fields["img"].N_imgs)
    # the grid's settings: an untrained field has no empty space, so alpha_min is put at the alpha of the field's MEDIAN raw density over the
    # grid's own points -- about half of the points lie below the level, and without dilation a good part of the cells is culled.  An input
    # of this test, chosen so that the sparse path has something to skip; no bound depends on it.
    vol = geometry.density_volume(trainer.model.renderer, [-4.] * 3, [4.] * 3, (33,) * 3)
    sigma = float(torch.nn.functional.softplus(vol.flatten().nanmedian().double()))
    trainer.model.renderer.cfg["occupancy"] = {"resolution": 32, "alpha_min": 1. - float(np.exp(-sigma)), "dilate": 0}
    pose = mdl.LearnPose(fields["img"].N_imgs, True, True, cfg, init_c2w=None).to(dev)
    opt = torch.optim.Adam(pose.parameters(), lr=lr)
    steps_taken = [0]
    opt.register_step_post_hook(lambda *_: steps_taken.__setitem__(0, steps_taken[0] + 1))
    tp = mdl.Trainer_pose(trainer.model, {"n_points": 96, "type": "nope_nerf", **({"occupancy": True} if occupancy else {})}, device=dev,
                          optimizer_pose=opt, pose_param_net=pose)
    builds, real = [0], geometry.occupancy_grid

    def counting(*a, **k):
        builds[0] += 1
        return real(*a, **k)
    geometry.occupancy_grid = counting
    try:
        done = 0
        while done < steps:
            for batch in loader:
                tp.train_step(batch)
                done += 1
                if done == steps:
                    break
        torch.cuda.synchronize()
    finally:
        geometry.occupancy_grid = real
    return pose.r.detach().clone(), pose.t.detach().clone(), builds[0], steps_taken[0], tp


def test_twenty_refinement_steps_build_the_grid_once_and_stay_within_the_cullings_reach(tmp_path, counted, capsys):
    """The bound: Adam moves a parameter by at most lr (1 - beta1) / sqrt(1 - beta2) = 3.17 lr per step whatever the gradients are; two runs
    of 20 steps from the same start are therefore never further apart than 2 x 20 x 3.17 lr per parameter.  That is all that can be SAID
    about two runs whose renders differ by the culled samples' matter; the distance reached is printed.  The exact check is
    test_culling_samples_without_matter_changes_no_bit."""
    import scene_writer
    scene_writer.write_scene(str(tmp_path), scene="toy", frames=4, size=(30, 40), seed=0)
    lr = 1e-3
    r1, t1, builds, steps, tp = _refine(str(tmp_path), True, lr=lr)
    assert builds == 1 and tp.occupancy_builds == 1 and steps == 20 and tp.occupancy_grid is not None      # built once, across twenty optimiser steps
    assert counted.calls.get("nnr_frozen_sparse_fwd") == 20 and counted.calls.get("nnr_frozen_sparse_bwd") == 20, counted.calls
    assert "nnr_frozen_fwd" not in counted.calls and "nnr_mlp_wgrad" not in counted.calls
    counted.calls.clear()
    r0, t0, builds0, _, tp0 = _refine(str(tmp_path), False, lr=lr)
    assert builds0 == 0 and tp0.occupancy_grid is None and counted.calls.get("nnr_frozen_fwd") == 20 and "nnr_frozen_sparse_fwd" not in counted.calls
    assert torch.isfinite(r1).all() and torch.isfinite(t1).all() and float(r1.abs().max()) > 0.0      # the poses moved
    dist = max(float((r1 - r0).abs().max()), float((t1 - t0).abs().max()))
    with capsys.disabled():
        print("\n  [frozen sparse, Trainer_pose] 20 steps: occupied share %.3f, largest pose-parameter distance to the dense run %.3e"
              % (float(tp.occupancy_grid.occupied), dist))
    assert 0.05 < float(tp.occupancy_grid.occupied) < 0.95      # (the grid did cull: the run above is not the dense one under another name)
    assert dist <= 2 * 20 * lr * (1 - 0.9) / (1 - 0.999) ** 0.5
