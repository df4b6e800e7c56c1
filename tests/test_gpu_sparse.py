"""GPU (-m gpu): the sparse inference render (nnr_sparse_f16.hip through nnr_render_sparse / nnr.ops.render_sparse).
  * cells: opt_cell against the float64 restatement of tests/sparse_ref.py (excused only within 1e-3 cells of a border: fp32's error there is
    below 1e-4 cells for |p| <= 8), live == outside | bit exactly, opt_count its row sum;
  * samples: the live rows of opt_out4 bit for bit nnr.ops.mlp_points(., split2=True) at host-built points, the culled rows untouched;
  * compositing: `out` against the float64 compositing of the kernel's own live samples at the project's output bar
    |x - ref| <= 1e-4 max(1, |ref|); all bits set: nnr.render_rays' fused inference outputs, bit for bit where the forward
    kernel takes the shape (R % 4 == 0, C % 32 == 0); against the dense render on the fitted scene within the bound of the culled alphas;
  * determinism, guard bands, the NaN rule, and the renderer's rendering.occupancy key.
Shapes as for the depth kernel: one ray and one sample; fewer rays than a workgroup's four; C = 32 and 33; several workgroups with a short
last one; the limit C = 256 (four compaction rounds per lane).  Grids: all set, all clear, random bits, and an all-clear half space with rays
wholly inside and wholly outside interleaved, so that one workgroup holds waves without a live sample beside full ones."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fusion_ref as FR      # noqa: E402
import sparse_ref as SR      # noqa: E402
from test_gpu_depth import _net, _rays, _bits, _worst      # noqa: E402  (the depth kernel's networks and rays: the issue's fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
SENTINEL = 0x7fc0beef             # a NaN with a payload no kernel writes
SHAPES = [(1, 1), (5, 3), (6, 32), (7, 33), (130, 64), (1023, 256)]
EXACT_SHAPES = [(8, 32), (128, 64), (1024, 256)]
BAR = 1e-4
GRIDS = ["set", "clear", "random", "halfspace", "clear_everywhere"]


class Grid:
    def __init__(self, lo, inv_step, dims, occ):
        self.lo, self.inv_step, self.dims = tuple(lo), tuple(inv_step), tuple(dims)
        self.bits = SR.pack_bits(occ).to(DEV)


@functools.lru_cache(maxsize=None)
def _grid(kind):
    """16^3 cells over [-2, 2]^3 (the random rays leave it: samples outside stay live); halfspace: x < 0 of [-8, 8]^3, all clear;
    clear_everywhere: 3 x 2 x 1 clear cells over [-16, 16]^3, every sample inside"""
    g = torch.Generator().manual_seed(77)
    if kind == "halfspace":
        return Grid((-8., -8., -8.), (2., 2., 2.), (16, 32, 32), torch.zeros(32, 32, 16, dtype=torch.bool))
    if kind == "clear_everywhere":
        return Grid((-16., -16., -16.), (3. / 32., 2. / 32., 1. / 32.), (3, 2, 1), torch.zeros(1, 2, 3, dtype=torch.bool))
    occ = {"set": torch.ones(16, 16, 16, dtype=torch.bool), "clear": torch.zeros(16, 16, 16, dtype=torch.bool),
           "random": torch.rand(16, 16, 16, generator=g) < 0.5}[kind]
    return Grid((-2., -2., -2.), (4., 4., 4.), (16, 16, 16), occ)


@functools.lru_cache(maxsize=None)
def _scene(n_rays, n, kind, grid_kind):
    """(o, d, view, lo, hi, jit).  halfspace: even rays start at x = -1 and head towards -x, odd rays at x = +1 towards +x"""
    o, d, lo, hi, jit = _rays(n_rays, n, kind)
    if grid_kind == "halfspace":
        side = torch.where(torch.arange(n_rays, device=DEV) % 2 == 0, -1., 1.)
        o, d = o.clone(), d.clone()
        o[:, 0] = side
        d[:, 0] = d[:, 0].abs() * side
    return o, d, (-d).contiguous(), lo, hi, jit


@functools.lru_cache(maxsize=None)
def _samples(hidden, n_rays, n, kind, grid_kind):
    """the references every check of one (network, rays) shares: the depths (nnr.ops.render_depth's, bit for bit the forward's), the
    host-built points, and mlp_points(split2=True) of every sample -> (z (R,C), pts (R,C,3) cpu float32, rgb (R,C,3), raw (R,C))"""
    from nnr import ops
    net = _net(hidden, kind)
    o, d, view, lo, hi, jit = _scene(n_rays, n, kind, grid_kind)
    _, _, zv = ops.render_depth(o, d, lo, hi, jit, net.weights(), net.biases(), hidden=hidden, dist_alpha=False, relu_sigma=False, debug=True)
    pts = FR.fma32(d.cpu().numpy()[:, None, :], zv.cpu().numpy()[:, :, None], o.cpu().numpy()[:, None, :])
    flat = torch.from_numpy(pts.reshape(-1, 3)).to(DEV)
    views = view[:, None, :].expand(n_rays, n, 3).reshape(-1, 3).contiguous()
    rgb, raw = ops.mlp_points(flat, views, net.weights(), net.biases(), hidden=hidden, split2=True)
    return zv, torch.from_numpy(pts), rgb.view(n_rays, n, 3).clone(), raw.view(n_rays, n).clone()


def _guarded(n_words):
    buf = torch.full((n_words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, C.c_void_p(buf.data_ptr() + 4 * GUARD)


def _split(buf, n_words):
    return buf[GUARD:GUARD + n_words], torch.cat([buf[:GUARD], buf[GUARD + n_words:]])


def _sparse_guarded(net, hidden, scene, grid, dist_alpha=False, relu=False, white=False, debug=True, flags=None, n_samples=None):
    """nnr_render_sparse through the C ABI into the middle of sentinel-filled buffers -> (rc, out (R,5), count, cell, out4 as int32 words,
    all guard bands in one tensor)"""
    from nnr import lib as L
    from nnr import ops
    o, d, view, lo, hi, jit = scene
    R, n = o.shape[0], lo.shape[0]
    f = L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2 | (L.NNR_F_DIST_ALPHA if dist_alpha else 0) | (L.NNR_F_RELU_SIGMA if relu else 0) | \
        (L.NNR_F_WHITE_BG if white else 0)
    cfg = L.Cfg(R, n if n_samples is None else n_samples, hidden, f if flags is None else flags)
    packed = ops._packed_for(ops.split2_cfg(R, n, hidden), net.weights(), net.biases())
    sizes = dict(out=5 * R, count=R, cell=R * n, out4=4 * R * n)
    bufs = {k: _guarded(v) for k, v in sizes.items()}
    p = {k: (bufs[k][1] if (debug or k == "out") else None) for k in sizes}
    lo3, is3, d3 = (C.c_float * 3)(*grid.lo), (C.c_float * 3)(*grid.inv_step), (C.c_int32 * 3)(*grid.dims)
    rc = L.load().nnr_render_sparse(C.byref(cfg), L.ptr(o), L.ptr(d), L.ptr(view), L.ptr(lo), L.ptr(hi), L.ptr(jit), lo3, is3, d3,
                                    L.ptr(grid.bits), L.ptr(packed), p["out"], p["count"], p["cell"], p["out4"], L.stream())
    torch.cuda.synchronize()
    parts = {k: _split(bufs[k][0], v) for k, v in sizes.items()}
    guard = torch.cat([parts[k][1] for k in sizes])
    return (rc, parts["out"][0].view(torch.float32).view(R, 5), parts["count"][0], parts["cell"][0].view(R, n),
            parts["out4"][0].view(R, n, 4), guard)


def _check(hidden, kind, shape, grid_kind, dist_alpha, relu, white, capsys):
    import nnr
    from nnr import ops
    R, n = shape
    net, grid = _net(hidden, kind), _grid(grid_kind)
    scene = _scene(R, n, kind, grid_kind)
    o, d, view, lo, hi, jit = scene
    zv, pts, want_rgb, want_raw = _samples(hidden, R, n, kind, grid_kind)
    rc, out, count, cell, out4, guard = _sparse_guarded(net, hidden, scene, grid, dist_alpha, relu, white)
    assert rc == 0
    assert bool((guard == SENTINEL).all()), "the kernel wrote outside its outputs"
    assert not bool((_bits(out) == SENTINEL).any()), "a ray was not written"
    assert not bool((cell == SENTINEL).any()) and not bool((count == SENTINEL).any())

    # 1. cells
    ref_cell, near = SR.cell_ref(pts, grid.lo, grid.inv_step, grid.dims)
    cell_c = cell.cpu().to(torch.int64)
    wrong = cell_c != ref_cell
    assert not bool((wrong & ~near).any()), "a cell differs from the float64 restatement away from every border"
    excused = int(wrong.sum())
    assert excused <= 0.02 * R * n, "%d of %d cells excused" % (excused, R * n)
    written = (out4 != SENTINEL).any(-1).cpu()
    live = SR.live_ref(grid.bits, cell_c, grid.dims)
    assert torch.equal(written, live), "live != outside | bit"
    assert torch.equal(count.cpu().to(torch.int64), live.sum(1))
    if grid_kind == "set":
        assert bool(live.all())
    if grid_kind == "clear_everywhere":
        assert not bool(live.any())
    if grid_kind == "halfspace" and R > 1:
        assert not bool(live[0::2].any()) and bool(live[1::2].all())

    # 2. samples: live rows bit for bit, culled rows untouched
    got4 = out4.view(torch.float32)
    want4 = torch.cat([want_rgb, want_raw[..., None]], -1)
    lv = live.to(DEV)
    assert torch.equal(_bits(got4[lv]), _bits(want4[lv])), "%d live samples differ from mlp_points" % int(
        (_bits(got4[lv]) != _bits(want4[lv])).any(-1).sum())
    assert bool((out4[~lv] == SENTINEL).all())

    # 3. compositing of the kernel's own live samples, float64
    alpha = FR.alpha_ref(want_raw, zv, dist_alpha, relu)
    ref = SR.composite_masked(alpha, want_rgb, zv, live, white)
    w64 = _worst(out, ref)
    assert torch.isfinite(out).all()
    if not bool(live.any()):
        bg = 1. if white else 0.
        assert torch.equal(out.cpu(), torch.tensor([bg, bg, bg, 0., 0.]).expand(R, 5))
    # 4. all set: the dense render
    wf = float('nan')
    if grid_kind == "set":
        with torch.no_grad():
            rgb_f, dist_f, _, _ = nnr.render_rays(o, d, view, lo, hi, jit, net.weights(), net.biases(), hidden=hidden, white_bg=white,
                                                  dist_alpha=dist_alpha, relu_sigma=relu, samples=False)
        fwd = torch.cat([rgb_f, dist_f[:, None]], 1)
        wf = _worst(out[:, :4], fwd)
        if R % 4 == 0 and n % 32 == 0:
            assert torch.equal(_bits(out[:, :4]), _bits(fwd)), "all bits set: not the forward's fused outputs bit for bit"
    with capsys.disabled():
        print("\nsparse D=%d %s %s R=%d C=%d%s%s%s: live %.1f %%, %d cells excused; worst |x - ref| / max(1, |ref|): %.3e against float64, "
              "%.3e against render_rays" % (hidden, kind, grid_kind, R, n, " dist_alpha" if dist_alpha else "", " relu" if relu else "",
                                           " white" if white else "", 100. * float(live.double().mean()), excused, w64, wf))
    assert w64 <= BAR
    assert not wf > BAR

    # 6. ops.render_sparse is that entry point; two runs agree bit for bit
    rgb2, dist2, acc2, count2, cell2, _ = ops.render_sparse(o, d, view, lo, hi, jit, grid, net.weights(), net.biases(), hidden=hidden,
                                                            dist_alpha=dist_alpha, white_bg=white, relu_sigma=relu, debug=True)
    again = torch.cat([rgb2, dist2[:, None], acc2[:, None]], 1)
    assert torch.equal(_bits(again), _bits(out)) and torch.equal(count2, count) and torch.equal(cell2, cell)
    return out, live, alpha


def _switches(i):
    """(dist_alpha, relu, white) of case i: every switch on and off for every grid over the six shapes"""
    return bool(i & 1), bool(i & 2), bool((i >> 2) & 1) ^ bool(i & 1)


@pytest.mark.parametrize("grid_kind", GRIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R%dxC%d" % s)
@pytest.mark.parametrize("hidden", [128, 256])
def test_sparse_kernel_on_random_networks(hidden, shape, grid_kind, capsys):
    i = SHAPES.index(shape) + GRIDS.index(grid_kind)
    _check(hidden, 'random', shape, grid_kind, *_switches(i), capsys)


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "R%dxC%d" % s)
@pytest.mark.parametrize("switches", [(False, False, False), (True, False, True), (False, True, False)], ids=["plain", "dist_alpha_white", "relu"])
@pytest.mark.parametrize("hidden", [128, 256])
def test_all_bits_set_is_the_forward_kernel_bit_for_bit(hidden, switches, shape, capsys):
    _check(hidden, 'random', shape, "set", *switches, capsys)


@pytest.mark.parametrize("hidden", [128, 256])
def test_against_the_dense_render_on_the_fitted_scene(hidden, capsys):
    """the fitted network, its rays at (130, 64), a grid from density_volume on [-2, 2]^3 at 32 cells, level -3.0 raw, dilate 1"""
    import nnr
    import model as mdl
    from model import geometry as G
    from test_host_logic import make_cfg
    R, n = 130, 64
    net = _net(hidden, 'fitted')
    o, d, view, lo, hi, jit = _scene(R, n, 'fitted', 'fitted')
    renderer = mdl.Renderer(net, make_cfg(hidden)['rendering'], device=DEV)
    grid = G.occupancy_grid(renderer, [-2.] * 3, [2.] * 3, 32, -3.0, dilate=1)
    assert grid.dims == (32, 32, 32) and tuple(grid.bits.shape) == (32, 32, 1)
    from nnr import ops
    rgb, dist, acc, count, cell, out4 = ops.render_sparse(o, d, view, lo, hi, jit, grid, net.weights(), net.biases(), hidden=hidden,
                                                          dist_alpha=False, white_bg=False, relu_sigma=False, debug=True)
    with torch.no_grad():
        rgb_d, dist_d, alpha_d, z_d = nnr.render_rays(o, d, view, lo, hi, jit, net.weights(), net.biases(), hidden=hidden, white_bg=False,
                                                      dist_alpha=False, relu_sigma=False, samples=True)
    alpha_d, z_d = alpha_d.view(R, n), z_d.view(R, n)
    live = ~torch.isnan(out4).any(-1).cpu()
    assert torch.equal(count.cpu().to(torch.int64), live.sum(1))
    culled = 1. - float(live.double().mean())
    mixed = int(((live.sum(1) > 0) & (live.sum(1) < n)).sum())
    bound = SR.culling_bound(alpha_d, live)
    acc_d = FR.composite_ref(alpha_d, z_d)[:, 1]
    err_rgb = (rgb.double().cpu() - rgb_d.double().cpu()).abs().max(1)[0]
    err_acc = (acc.double().cpu() - acc_d).abs()
    err_dist = (dist.double().cpu() - dist_d.double().cpu()).abs()
    zmax = z_d.double().cpu().max(1)[0]
    with capsys.disabled():
        print("\nsparse against dense D=%d: %.1f %% culled, %d of %d rays partly culled; worst error / bound: rgb %.3e / %.3e, acc %.3e / %.3e, "
              "sum w z %.3e / %.3e" % (hidden, 100. * culled, mixed, R, float(err_rgb.max()), float(bound[err_rgb.argmax()]),
                                       float(err_acc.max()), float(bound[err_acc.argmax()]), float(err_dist.max()),
                                       float((bound * zmax)[err_dist.argmax()])))
    assert culled >= 0.10 and mixed >= 100, "the fixture culls too little to test anything"
    assert bool((err_rgb <= bound + BAR).all()) and bool((err_acc <= bound + BAR).all())
    assert bool((err_dist <= bound * zmax + BAR * dist_d.double().cpu().abs().clamp(min=1.)).all())


@pytest.mark.parametrize("grid_kind", ["set", "random"])
@pytest.mark.parametrize("hidden", [128, 256])
def test_a_nan_origin_makes_its_ray_nan_and_leaves_its_workgroup_untouched(hidden, grid_kind):
    net, grid = _net(hidden, 'random'), _grid(grid_kind)
    scene = _scene(7, 33, 'random', grid_kind)
    _, clean, count0, _, _, _ = _sparse_guarded(net, hidden, scene, grid)
    o = scene[0].clone()
    o[5, 0] = float('nan')                                          # rays 4..6 share the second workgroup
    rc, out, count, cell, out4, guard = _sparse_guarded(net, hidden, (o,) + scene[1:], grid)
    assert rc == 0 and bool((guard == SENTINEL).all())
    assert bool(torch.isnan(out[5]).all()) and bool((cell[5] == -1).all()) and int(count[5]) == 33      # a NaN point is outside: live
    keep = [0, 1, 2, 3, 4, 6]
    assert torch.equal(_bits(out[keep]), _bits(clean[keep])) and torch.equal(count[keep], count0[keep])


def test_refused_configurations_leave_the_outputs_untouched():
    from nnr import lib as L
    net, grid = _net(128, 'random'), _grid("random")
    scene = _scene(6, 32, 'random', "random")
    s2 = L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    calls = [dict(n_samples=257)] + [dict(flags=f) for f in (s2 | L.NNR_F_TRAIN, s2 | L.NNR_F_BF16, L.NNR_F_SPLIT3, 0)]
    for kw in calls:
        rc, out, count, cell, out4, guard = _sparse_guarded(net, 128, scene, grid, **kw)
        assert rc == -2, kw
        for t in (_bits(out), count, cell, out4, guard):
            assert bool((t == SENTINEL).all()), kw


# ------------------------------------------------------------------------------------------------------------ the renderer's key
def _render_inputs(n_rays):
    g = torch.Generator().manual_seed(5)
    pixels = (torch.rand(1, n_rays, 2, generator=g) * 2. - 1.).to(DEV)
    depth = torch.ones(1, n_rays, 1, device=DEV)
    cam = torch.diag(torch.tensor([1.2, -1.2, -1., 1.]))[None].to(DEV)
    world = torch.eye(4)
    world[2, 3] = -3.0
    return pixels, depth, cam, world[None].to(DEV), torch.eye(4)[None].to(DEV)


@pytest.mark.parametrize("hidden", [128, 256])
def test_the_renderer_without_the_key_is_the_parent_and_with_it_reuses_its_grid(hidden, caplog):
    import nnr
    import model as mdl
    from nnr import camera
    from test_host_logic import make_cfg
    net = _net(hidden, 'fitted')
    base = make_cfg(hidden, num_points=48, depth_range=[0.5, 6.0], radius=2.0)['rendering']
    inputs = _render_inputs(64)
    plain = mdl.Renderer(net, dict(base), device=DEV)
    with torch.no_grad():
        a = plain.nope_nerf(*inputs, add_noise=False, eval_=True)
        # the parent's path, restated: ray_setup, the z tables, render_rays with the samples left out
        origin, ray, view, ray_norm, d_gt, mask = camera.ray_setup(*inputs, True, True)
        z_lo, z_hi = plain._z_tables(48, 0.5, 6.0, False, DEV)
        rgb, dist, _, _ = nnr.render_rays(origin, ray, view, z_lo, z_hi, None, net.weights(), net.biases(), hidden=hidden, dist_alpha=False,
                                          white_bg=False, relu_sigma=False, bf16=False, samples=False)
    assert torch.equal(_bits(a['rgb'][0]), _bits(rgb)) and torch.equal(_bits(a['dist_dense']), _bits(dist / ray_norm))
    assert not hasattr(plain, 'occupancy_builds')

    sparse = mdl.Renderer(net, dict(base, occupancy={'resolution': 24, 'alpha_min': 0.04, 'dilate': 1}), device=DEV)
    with torch.no_grad():
        b = sparse.nope_nerf(*inputs, add_noise=False, eval_=True)
        grid = sparse.__dict__['_occupancy_hit'][2]
        c = sparse.nope_nerf(*inputs, add_noise=False, eval_=True)
        assert sparse.occupancy_builds == 1 and sparse.__dict__['_occupancy_hit'][2] is grid, "the grid was not reused"
    assert grid.dims == (24, 24, 24) and grid.lo == (-2., -2., -2.)
    assert torch.equal(_bits(b['rgb']), _bits(c['rgb'])) and torch.isfinite(b['rgb']).all()
    assert 0. < float(grid.occupied) < 1.
    # (alpha_min 0.04 without dist_alpha is raw = -3.18: the fitted scene's empty space sits at about -4.4, its shapes far above)
    from nnr import ops
    with torch.no_grad():
        rgb_s, dist_s, _ = ops.render_sparse(origin, ray, view, z_lo, z_hi, None, grid, net.weights(), net.biases(), hidden=hidden,
                                             dist_alpha=False, white_bg=False, relu_sigma=False)
    assert torch.equal(_bits(b['rgb'][0]), _bits(rgb_s)) and torch.equal(_bits(b['dist_dense']), _bits(dist_s / ray_norm))
    assert not torch.equal(_bits(b['rgb']), _bits(a['rgb'])), "nothing was culled: the sparse path was not exercised"
    assert tuple(b['alpha'].shape[-2:]) == (64, 48)            # the lazily fetched samples still come from the dense pass
    # an optimiser step invalidates the packed weights, and with them the grid
    opt = torch.optim.SGD(net.parameters(), lr=0.)
    opt.step()
    with torch.no_grad():
        sparse.nope_nerf(*inputs, add_noise=False, eval_=True)
    assert sparse.occupancy_builds == 2 and sparse.__dict__['_occupancy_hit'][2] is not grid
    # with gradients enabled the dense path runs, and says so once
    import logging
    with caplog.at_level(logging.INFO, logger="model.rendering"):
        e = sparse.nope_nerf(*inputs, add_noise=False, eval_=True)
        sparse.nope_nerf(*inputs, add_noise=False, eval_=True)
    assert sparse.occupancy_builds == 2 and e['rgb'].requires_grad
    assert sum("rendering.occupancy: dense render" in r.getMessage() for r in caplog.records) == 1
    with pytest.raises(ValueError, match="alpha_min"):
        with torch.no_grad():
            mdl.Renderer(net, dict(base, occupancy={'resolution': 24}), device=DEV).nope_nerf(*inputs, add_noise=False, eval_=True)
