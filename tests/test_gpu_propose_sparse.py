"""GPU (-m gpu): the sparse proposal stage of hierarchical sampling (nnr_propose_f16.hip under NNR_PROPOSE_SPARSE=1 through
nnr.ops.propose_sparse; rendering.occupancy.proposal).  Every comparison is bitwise, on the int32 view: the cells
and counts against tests/sparse_ref.py, the alphas against the dense proposal's masked by liveness, the rows against nnr_resample fed with
the kernel's own alphas and depths, an all-set grid against nnr_propose; NaN containment both ways (a live NaN poisons its ray, a culled
one does not); the Renderer and Trainer_pose with the key against the hand-made compositions and against the key absent."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nope-nerf_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import propose_sparse_ref as PS      # noqa: E402
import sparse_ref as SR              # noqa: E402
import test_gpu_propose as tp        # noqa: E402 -- _net, _rays, _tables, _inputs and the dense proposal
import test_gpu_resample as tres     # noqa: E402 -- the end-to-end helpers

pytestmark = pytest.mark.gpu
DEV = "cuda"
_bits = tp._bits
R_E2E = tres.R_E2E


# ---------------------------------------------------------------------------------------------------------------- grids
def _centres(lo, hi):
    c = lo + (torch.arange(16, dtype=torch.float64) + 0.5) * ((hi - lo) / 16.)
    return torch.meshgrid(c, c, c, indexing="ij")      # (z, y, x)


@functools.lru_cache(maxsize=None)
def _grid(pattern, lo=-8.0, hi=8.0):
    """16^3 cells over [lo, hi]^3 (steps and origin are powers of two: the fp32 cell rule rounds nowhere but in p - lo).  'all' / 'none':
    every / no bit set; 'ball': the cells whose centre lies within 1.0 of the origin; 'random': p = 0.3, seeded."""
    from model import geometry as G
    if pattern == 'all':
        occ = torch.ones(16, 16, 16, dtype=torch.bool)
    elif pattern == 'none':
        occ = torch.zeros(16, 16, 16, dtype=torch.bool)
    elif pattern == 'ball':
        cz, cy, cx = _centres(lo, hi)
        occ = (cx * cx + cy * cy + cz * cz).sqrt() <= 1.0
    else:
        occ = torch.rand(16, 16, 16, generator=torch.Generator().manual_seed(29)) < 0.3
    return G.OccupancyGrid((lo,) * 3, (16. / (hi - lo),) * 3, (16, 16, 16), SR.pack_bits(occ).to(DEV))


def _sparse(net, hidden, inp, F, grid, dist_alpha=False, relu_sigma=False):
    from nnr import ops
    o, d, z_lo, z_hi, jit, xi = inp
    return ops.propose_sparse(o, d, z_lo, z_hi, jit, xi, F, grid, net.weights(), net.biases(), hidden=hidden, dist_alpha=dist_alpha,
                              relu_sigma=relu_sigma, debug=True)


# (hidden, net, C, F, R, mode, jitter, xi, pattern): every shape at both widths, every R, mode and pattern at least twice
CASES = [(128, 'fitted', 64, 128, 67, 'softplus', True, True, 'ball'), (256, 'fitted', 64, 128, 67, 'softplus', True, True, 'random'),
         (128, 'random', 64, 128, 5, 'dist_alpha', True, True, 'random'), (256, 'random', 64, 128, 1, 'relu', False, False, 'ball'),
         (128, 'random', 33, 7, 5, 'softplus', True, False, 'ball'), (256, 'fitted', 33, 7, 67, 'dist_alpha', False, True, 'random'),
         (128, 'fitted', 3, 1, 1, 'softplus', False, False, 'none'), (256, 'random', 3, 1, 5, 'dist_alpha', True, True, 'random'),
         (128, 'fitted', 100, 60, 67, 'relu', True, True, 'random'), (256, 'random', 100, 60, 5, 'softplus', False, True, 'ball'),
         (128, 'random', 100, 60, 1, 'dist_alpha', True, False, 'all'),
         (128, 'fitted', 256, 768, 5, 'dist_alpha', True, True, 'ball'), (256, 'fitted', 256, 768, 67, 'softplus', True, True, 'random'),
         (256, 'random', 256, 768, 1, 'relu', False, False, 'none'),
         (256, 'fitted', 64, 128, 5, 'softplus', True, True, 'all'), (128, 'random', 64, 128, 67, 'dist_alpha', True, True, 'none')]
ALL_SET = [(128, 'fitted', 64, 128, 67, 'softplus', True, True), (256, 'random', 33, 7, 5, 'dist_alpha', True, False),
           (128, 'random', 3, 1, 1, 'relu', False, False), (256, 'fitted', 100, 60, 67, 'relu', True, True),
           (128, 'fitted', 256, 768, 5, 'dist_alpha', True, True), (256, 'fitted', 256, 768, 1, 'softplus', False, True)]


@functools.lru_cache(maxsize=None)
def _case(hidden, kind, Cn, F, R, mode, jitter, xi, pattern):
    """inputs, the sparse kernel's debug outputs, the dense proposal's, computed once and left unchanged"""
    net = tp._net(hidden, kind)
    inp = tp._inputs(R, Cn, F, jitter, xi)
    got = _sparse(net, hidden, inp, F, _grid(pattern), **tp._mode_kw(mode))
    dense = tp._propose(net, hidden, inp, F, **tp._mode_kw(mode))
    return inp, got, dense


def _liveness(inp, z_c, cell, grid):
    """The kernel's cells against the float64 restatement on p = o + d z_c (fp32, unfused): equal wherever no coordinate lies within 1e-3
    cells of a border, and at most 2 % excused.  -> live (R,C) bool on the CPU, from the kernel's cells."""
    pts = PS.points(inp[0], inp[1], z_c)
    ref_cell, near = SR.cell_ref(pts, grid.lo, grid.inv_step, grid.dims)
    cell_c = cell.cpu().to(torch.int64)
    wrong = cell_c != ref_cell
    assert not bool((wrong & ~near).any()), "a cell differs from the float64 restatement away from every border"
    assert int(wrong.sum()) <= 0.02 * cell_c.numel()
    return SR.live_ref(grid.bits, cell_c, grid.dims)


# ---------------------------------------------------------------------------------------------------------------- 1. every bit set
@pytest.mark.parametrize("hidden,kind,Cn,F,R,mode,jitter,xi", ALL_SET)
def test_with_every_bit_set_the_outputs_are_nnr_proposes(hidden, kind, Cn, F, R, mode, jitter, xi):
    net = tp._net(hidden, kind)
    inp = tp._inputs(R, Cn, F, jitter, xi)
    z_all, alpha_c, z_c, fine, count, cell, passes = _sparse(net, hidden, inp, F, _grid('all'), **tp._mode_kw(mode))
    want = tp._propose(net, hidden, inp, F, **tp._mode_kw(mode))
    for got, ref in zip((z_all, alpha_c, z_c, fine), want):
        assert got.shape == ref.shape and torch.equal(_bits(got), _bits(ref))
    assert bool((cell >= 0).all()) and count.tolist() == [Cn] * R and passes.tolist() == [(Cn + 31) // 32] * R


# ---------------------------------------------------------------------------------------------------------------- 2-3. cells, alphas, rows
@pytest.mark.parametrize("hidden,kind,Cn,F,R,mode,jitter,xi,pattern", CASES)
def test_cells_counts_and_passes_are_the_references(hidden, kind, Cn, F, R, mode, jitter, xi, pattern):
    inp, (z_all, alpha_c, z_c, fine, count, cell, passes), _ = _case(hidden, kind, Cn, F, R, mode, jitter, xi, pattern)
    assert count.dtype == cell.dtype == passes.dtype == torch.int32 and cell.shape == (R, Cn) and count.shape == passes.shape == (R,)
    live = _liveness(inp, z_c, cell, _grid(pattern))
    assert torch.equal(count.cpu().to(torch.int64), live.sum(1))
    assert torch.equal(passes.cpu().to(torch.int64), PS.passes_ref(count, R))


@pytest.mark.parametrize("hidden,kind,Cn,F,R,mode,jitter,xi,pattern", CASES)
def test_alphas_are_the_dense_ones_where_live_and_zero_where_culled(hidden, kind, Cn, F, R, mode, jitter, xi, pattern):
    from nnr import ops
    inp, (z_all, alpha_c, z_c, fine, count, cell, passes), dense = _case(hidden, kind, Cn, F, R, mode, jitter, xi, pattern)
    live = _liveness(inp, z_c, cell, _grid(pattern)).to(DEV)
    assert torch.equal(_bits(alpha_c), _bits(torch.where(live, dense[1], torch.zeros_like(dense[1]))))
    assert torch.equal(_bits(z_c), _bits(dense[2]))
    want_all, want_fine = ops.resample(alpha_c, z_c, inp[5], F, return_fine=True)
    assert torch.equal(_bits(z_all), _bits(want_all)) and torch.equal(_bits(fine), _bits(want_fine))
    assert bool(torch.isfinite(z_all).all()) and bool((z_all[:, 1:] >= z_all[:, :-1]).all())


# ---------------------------------------------------------------------------------------------------------------- 4. the inputs do test it
def test_the_cases_cull_skip_passes_and_lose_matter():
    fewer, lost = 0, 0
    for case in CASES:
        hidden, kind, Cn, F, R, mode, jitter, xi, pattern = case
        inp, (z_all, alpha_c, z_c, fine, count, cell, passes), dense = _case(*case)
        if pattern in ('ball', 'random'):
            fewer += int((passes < (Cn + 31) // 32).sum())
            culled = ~_liveness(inp, z_c, cell, _grid(pattern)).to(DEV)
            inner = culled.clone()
            if mode == 'dist_alpha':
                inner[:, -1] = False      # (the closing alpha is 1 by definition, not by matter)
            lost += int((inner & (dense[1] > 0.05)).sum())
        elif pattern == 'none':
            assert count.tolist() == [0] * R and passes.tolist() == [0] * R
    assert fewer > 0, "no workgroup of the ball and random cases ran fewer passes than the dense kernel"
    assert lost > 0, "no culled sample of the ball and random cases has a dense alpha above 0.05"


@pytest.mark.parametrize("hidden,mode", [(128, 'softplus'), (256, 'dist_alpha')])
def test_a_small_empty_grid_leaves_the_samples_outside_it_live(hidden, mode):
    from nnr import ops
    net = tp._net(hidden, 'fitted')
    inp = tp._inputs(5, 64, 128, True, True)
    grid = _grid('none', -1.0, 1.0)
    z_all, alpha_c, z_c, fine, count, cell, passes = _sparse(net, hidden, inp, 128, grid, **tp._mode_kw(mode))
    dense = tp._propose(net, hidden, inp, 128, **tp._mode_kw(mode))
    live = _liveness(inp, z_c, cell, grid)
    assert int(count.max()) > 0 and bool((count < 64).any()) and torch.equal(count.cpu().to(torch.int64), live.sum(1))
    assert torch.equal(live, cell.cpu() < 0)      # no bit is set: live is outside
    assert torch.equal(passes.cpu().to(torch.int64), PS.passes_ref(count, 5))
    assert torch.equal(_bits(alpha_c), _bits(torch.where(live.to(DEV), dense[1], torch.zeros_like(dense[1]))))
    want_all, want_fine = ops.resample(alpha_c, z_c, inp[5], 128, return_fine=True)
    assert torch.equal(_bits(z_all), _bits(want_all)) and torch.equal(_bits(fine), _bits(want_fine))


# ---------------------------------------------------------------------------------------------------------------- 5-6. NaN
@pytest.mark.parametrize("hidden,Cn,F", [(128, 64, 128), (256, 33, 7)])
def test_nan_origin_poisons_exactly_its_ray(hidden, Cn, F):
    """Ray 5 of 7 under a grid without a set bit that holds every sample: the NaN point is outside the grid, hence live -- all C samples of
    the ray; its row, alphas and fine samples are NaN.  Every other ray (all culled: the uniform row) is bitwise what it is without it."""
    net = tp._net(hidden, 'random')
    inp = tp._inputs(7, Cn, F, True, True)
    grid = _grid('none')
    clean = _sparse(net, hidden, inp, F, grid)
    o2 = inp[0].clone()
    o2[5, 1] = float('nan')
    z_all, alpha_c, z_c, fine, count, cell, passes = _sparse(net, hidden, (o2,) + inp[1:], F, grid)
    bad = torch.zeros(7, dtype=torch.bool, device=DEV)
    bad[5] = True
    assert bool(torch.isnan(z_all[bad]).all()) and bool(torch.isnan(fine[bad]).all()) and bool(torch.isnan(alpha_c[bad]).all())
    assert count.tolist() == [0, 0, 0, 0, 0, Cn, 0] and cell[5].tolist() == [-1] * Cn
    assert passes.tolist() == [0] * 4 + [(Cn + 31) // 32] * 3 and clean[6].tolist() == [0] * 7
    assert torch.equal(z_c, clean[2])
    for got, want in zip((z_all, alpha_c, fine), (clean[0], clean[1], clean[3])):
        assert torch.equal(_bits(got[~bad]), _bits(want[~bad])) and bool(torch.isfinite(got[~bad]).all())


@pytest.mark.parametrize("hidden", [128, 256])
def test_an_activation_outside_fp16_range_counts_only_where_the_sample_is_live(hidden):
    """Ray 2 of 6 starts 3e4 away; with the 'hot' network its activations leave fp16's range.  Outside the grid the ray is live and its row
    NaN, as in the dense kernel.  With the grid moved so that the ray's samples lie in cleared cells they are not evaluated: the row is
    finite.  The other rays -- outside the moved grid, inside the first: live under 'all' -- are unchanged in both."""
    from model import geometry as G
    Cn, F = 64, 128
    inp = tp._inputs(6, Cn, F, True, True, seed=3)
    o2 = inp[0].clone()
    o2[2] = torch.tensor([3e4, -2e4, 1e4], device=DEV)
    far = (o2,) + inp[1:]
    hot = tp._net(hidden, 'hot')
    dense_clean = tp._propose(hot, hidden, inp, F)
    bad = torch.zeros(6, dtype=torch.bool, device=DEV)
    bad[2] = True
    here = _sparse(hot, hidden, far, F, _grid('all'))      # the far ray is outside [-8, 8]^3
    assert here[4].tolist() == [Cn] * 6 and bool((here[5][2] == -1).all())
    assert bool(torch.isnan(here[0][bad]).all()) and bool(torch.isnan(here[3][bad]).all()) and bool(torch.isnan(here[1][bad]).any())
    c = [3e4, -2e4, 1e4]
    moved = G.OccupancyGrid(tuple(v - 16. for v in c), (0.5,) * 3, (16, 16, 16), torch.zeros(16, 16, 1, dtype=torch.int32, device=DEV))
    there = _sparse(hot, hidden, far, F, moved)            # 32 units around the far origin, no bit set: |d z| <= 4 stays inside
    assert there[4].tolist() == [Cn, Cn, 0, Cn, Cn, Cn] and bool((there[5][2] >= 0).all())
    assert all(bool(torch.isfinite(t[bad]).all()) for t in there[:4]) and bool((there[1][bad] == 0).all())
    for res in (here, there):
        for got, want in zip((res[0], res[1], res[3]), (dense_clean[0], dense_clean[1], dense_clean[3])):
            assert torch.equal(_bits(got[~bad]), _bits(want[~bad])) and bool(torch.isfinite(got[~bad]).all())


# ---------------------------------------------------------------------------------------------------------------- 7. determinism
def test_two_runs_are_bitwise_equal_and_the_debug_outputs_do_not_change_the_row():
    from nnr import ops
    inp, first, _ = _case(128, 'fitted', 100, 60, 67, 'relu', True, True, 'random')
    net = tp._net(128, 'fitted')
    second = _sparse(net, 128, inp, 60, _grid('random'), relu_sigma=True)
    for a, b in zip(first, second):
        assert torch.equal(_bits(a), _bits(b))
    o, d, z_lo, z_hi, jit, xi = inp
    plain = ops.propose_sparse(o, d, z_lo, z_hi, jit, xi, 60, _grid('random'), net.weights(), net.biases(), hidden=128, dist_alpha=False,
                               relu_sigma=True)
    assert torch.is_tensor(plain) and not plain.requires_grad and torch.equal(_bits(plain), _bits(first[0]))


# ---------------------------------------------------------------------------------------------------------------- 8. the Renderer
def _occ_settings(renderer, option):
    """rendering.occupancy for an untrained field, which has no empty space: alpha_min at the alpha of the MEDIAN raw density over the
    grid's own points, no dilation -- about half the cells are culled.  An input of the test; no comparison depends on it."""
    from model import geometry
    lo, hi = (-4., 4.) if option == 'uniform' else (-1.5, 1.5)
    vol = geometry.density_volume(renderer, [lo] * 3, [hi] * 3, (17,) * 3)
    sigma = float(torch.nn.functional.softplus(vol.flatten().nanmedian().double()))
    delta = 1. if option == 'uniform' else 1. / 63.      # (ndc runs under dist_alpha: the level is taken at the coarse spacing)
    return {"resolution": 16, "alpha_min": 1. - float(np.exp(-sigma * delta)), "dilate": 0, "bounds": [lo, hi]}


def _thin(renderer):
    """The untrained field is opaque within a few samples of the camera (alpha about 0.5 a sample): what the grid culls further down the
    ray then weighs nothing, and no proposal could show it.  The density head's bias is lowered by 3 (alpha about 0.05 a sample: the
    weights spread over the whole ray).  An input of the tests, applied to every renderer they compare."""
    with torch.no_grad():
        renderer.model.fc_density.bias.sub_(3.0)
    return renderer


def _occ_renderer(option, key):
    """the renderer of tests/test_gpu_resample.py (D = 128, num_fine 128, 'density') with rendering.occupancy; key: True / False / None (absent)"""
    renderer, cfg = tres._renderer(128, option, "fp32", num_fine=128, proposal='density')
    _thin(renderer)
    occ = _occ_settings(renderer, option)
    if key is not None:
        occ["proposal"] = key
    renderer.cfg["occupancy"] = occ
    return renderer, cfg


def _eval_render(renderer, inputs, add_noise, seed=99):
    pixels, depth, K, Wm, S, _, _ = inputs
    torch.cuda.manual_seed(seed)
    with torch.no_grad():
        out = renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=add_noise)
    return (out['rgb'].reshape(-1, 3).clone(), out['dist_dense'].clone()), torch.cuda.get_rng_state()


def _by_hand(renderer, cfg, inputs, add_noise, grid, sparse_proposal, seed=99):
    """The sparse hierarchical frame spelled out with the public operators: ops.propose_sparse (or ops.propose) and ops.render_sparse."""
    from nnr import camera, ops
    pixels, depth, K, Wm, S, _, _ = inputs
    rc, net = cfg['rendering'], renderer.model
    C0, n_fine = rc['num_points'] - rc['outside_steps'], 128
    torch.cuda.manual_seed(seed)
    with torch.no_grad():
        origin, ray, view, _, _, _ = camera.ray_setup(pixels, depth, K, Wm, S, bool(rc['normalise_ray']), bool(rc['use_ray_dir']))
        jitter = None
        if rc['sample_option'] == 'ndc':
            pts_o, pts_d = camera.ndc_rays(origin, ray, K, 1.0)
            z_lo, z_hi = renderer._z_tables(C0, 0., 1., False, pixels.device)
        else:
            pts_o, pts_d = origin, ray
            z_lo, z_hi = renderer._z_tables(C0, rc['depth_range'][0], rc['depth_range'][1], bool(add_noise), pixels.device)
            if add_noise:
                jitter = torch.rand(1, R_E2E, C0, device=DEV)
        xi = torch.rand(R_E2E, n_fine, device=DEV) if jitter is not None else None
        kw = dict(hidden=net.hidden_dim, dist_alpha=bool(rc['dist_alpha']), relu_sigma=False)
        if sparse_proposal:
            z_all = ops.propose_sparse(pts_o, pts_d, z_lo, z_hi, jitter, xi, n_fine, grid, net.weights(), net.biases(), **kw)
        else:
            z_all = ops.propose(pts_o, pts_d, z_lo, z_hi, jitter, xi, n_fine, net.weights(), net.biases(), **kw)
        n_all = C0 + n_fine
        rgb, dist, _ = ops.render_sparse(pts_o, pts_d, view, torch.zeros(n_all, device=DEV), torch.ones(n_all, device=DEV), z_all, grid,
                                         net.weights(), net.biases(), white_bg=False, **kw)
    return (rgb.clone(), dist.clone()), torch.cuda.get_rng_state()


def _equal(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("option,add_noise", [("uniform", True), ("ndc", False)])
def test_renderer_with_the_key_is_the_hand_made_composition(option, add_noise):
    inputs = tres._scene_inputs()
    on, cfg = _occ_renderer(option, True)
    got_on, state_on = _eval_render(on, inputs, add_noise)
    grid = on.__dict__['_occupancy_hit'][2]
    assert 0.05 < float(grid.occupied) < 0.95 and on.occupancy_builds == 1
    want_on, state_hand = _by_hand(on, cfg, inputs, add_noise, grid, True)
    assert _equal(got_on, want_on) and all(bool(torch.isfinite(t).all()) for t in got_on)
    again, _ = _eval_render(on, inputs, add_noise)
    assert _equal(again, got_on) and on.occupancy_builds == 1      # the key is no part of the grid's cache key: no second build
    # key absent (and false): today's bits -- the dense proposal in front of the sparse render
    absent, cfg_a = _occ_renderer(option, None)
    got_absent, state_absent = _eval_render(absent, inputs, add_noise)
    grid_a = absent.__dict__['_occupancy_hit'][2]
    assert torch.equal(grid_a.bits, grid.bits)
    want_absent, _ = _by_hand(absent, cfg_a, inputs, add_noise, grid_a, False)
    assert _equal(got_absent, want_absent)
    off, _ = _occ_renderer(option, False)
    got_off, state_off = _eval_render(off, inputs, add_noise)
    assert _equal(got_off, got_absent)
    assert not _equal(got_on, got_absent), "the sparse proposal changed no bit of the frame: the grid culled nothing that matters"
    # an all-set grid: the key changes no bit
    for r in (on, absent):
        r.__dict__['_occupancy_hit'][2].bits.fill_(-1)
    full_on, state_full_on = _eval_render(on, inputs, add_noise)
    full_absent, state_full_absent = _eval_render(absent, inputs, add_noise)
    assert _equal(full_on, full_absent)
    for s in (state_hand, state_absent, state_off, state_full_on, state_full_absent):
        assert torch.equal(s, state_on)


def test_render_proposal_with_the_key_raises_on_the_gpu_too():
    renderer, _ = tres._renderer(128, "uniform", "fp32", num_fine=128, proposal='render')
    renderer.cfg["occupancy"] = {"resolution": 16, "alpha_min": 0.01, "proposal": True}
    pixels, depth, K, Wm, S, _, _ = tres._scene_inputs()
    with pytest.raises(ValueError, match="rendering.occupancy.proposal.*rendering.proposal"):
        renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=False)


def test_a_refused_grid_runs_the_dense_proposal(monkeypatch):
    """Gradients enabled and no frozen field: the grid is refused, the dense proposal runs, the training render is today's."""
    from nnr import ops
    calls = []
    real = ops.propose
    monkeypatch.setattr(ops, "propose", lambda *a, **k: calls.append("dense") or real(*a, **k))
    monkeypatch.setattr(ops, "propose_sparse", lambda *a, **k: calls.append("sparse"))
    inputs = tres._scene_inputs()
    on, _ = _occ_renderer("uniform", True)
    got, state = tp._render(on, inputs, True)
    assert calls == ["dense"]
    plain, _ = tres._renderer(128, "uniform", "fp32", num_fine=128, proposal='density')
    _thin(plain)
    want, state_plain = tp._render(plain, inputs, True)
    tp._same(got, want)
    assert torch.equal(state, state_plain)


# ---------------------------------------------------------------------------------------------------------------- 9. pose refinement
def _pose_trainer(scene_dir, key):
    import dataloading as dl
    import model as mdl
    import train_scene
    from model import geometry
    torch.manual_seed(11)
    np.random.seed(11)
    dev = torch.device("cuda")
    cfg = train_scene.scene_cfg(scene_dir, "toy", n_rays=96, n_samples=24, hidden=128, sample_rate=10 ** 6, num_fine=32, proposal='density')
    loader, fields = dl.get_dataloader(cfg, mode="train", shuffle=False)
    trainer, _, _ = train_scene.build(cfg, dev, fields["img"].N_imgs)
    vol = geometry.density_volume(trainer.model.renderer, [-4.] * 3, [4.] * 3, (33,) * 3)      # (tests/test_gpu_frozen_sparse.py::_refine)
    sigma = float(torch.nn.functional.softplus(vol.flatten().nanmedian().double()))
    occ = {"resolution": 32, "alpha_min": 1. - float(np.exp(-sigma)), "dilate": 0}
    if key is not None:
        occ["proposal"] = key
    trainer.model.renderer.cfg["occupancy"] = occ
    pose = mdl.LearnPose(fields["img"].N_imgs, True, True, cfg, init_c2w=None).to(dev)
    opt = torch.optim.Adam(pose.parameters(), lr=1e-3)
    tpose = mdl.Trainer_pose(trainer.model, {"n_points": 96, "type": "nope_nerf", "occupancy": True}, device=dev, optimizer_pose=opt,
                             pose_param_net=pose)
    return tpose, pose, next(iter(loader))


def _pose_step(tpose, pose, batch, all_set=False):
    """one compute_loss + backward from a fixed seed (the pixel draw) -> loss, the pose gradients; the grid is built by the first call"""
    if all_set and tpose.occupancy_builds == 0:
        tpose.occupancy_grid = tpose.model.renderer.frozen_occupancy_grid(torch.device("cuda"))
        tpose.occupancy_grid.bits.fill_(-1)
        tpose.occupancy_builds = 1
    pose.zero_grad()
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    loss = tpose.compute_loss(batch)['loss']
    loss.backward()
    return loss.detach().clone(), [p.grad.detach().clone() for p in pose.parameters()]


def test_pose_refinement_proposes_through_the_frozen_grid(tmp_path, monkeypatch):
    import scene_writer
    from nnr import ops
    scene_writer.write_scene(str(tmp_path), scene="toy", frames=4, size=(30, 40), seed=0)
    calls = []
    real_sparse, real_dense = ops.propose_sparse, ops.propose

    def sparse(*a, **k):
        calls.append(("sparse", a[7]))
        return real_sparse(*a, **k)
    monkeypatch.setattr(ops, "propose_sparse", sparse)
    monkeypatch.setattr(ops, "propose", lambda *a, **k: calls.append(("dense", None)) or real_dense(*a, **k))
    # an all-set grid: loss and pose gradient are bitwise those with the key off
    res = {}
    for key in (True, None):
        tpose, pose, batch = _pose_trainer(str(tmp_path), key)
        res[key] = _pose_step(tpose, pose, batch, all_set=True)
        assert [c[0] for c in calls] == (["sparse"] if key else ["dense"]) and (not key or calls[0][1] is tpose.occupancy_grid)
        calls.clear()
    assert torch.equal(_bits(res[True][0]), _bits(res[None][0]))
    for g, w in zip(res[True][1], res[None][1]):
        assert torch.equal(_bits(g), _bits(w))
    assert any(float(g.abs().max()) > 0 for g in res[True][1])
    # the field's own grid: the step is the hand-made composition -- the key-off step whose dense proposal is replaced by the sparse one on
    # the trainer's grid -- and its gradients are finite and not zero
    tpose, pose, batch = _pose_trainer(str(tmp_path), True)
    loss_on, grads_on = _pose_step(tpose, pose, batch)
    grid = tpose.occupancy_grid
    assert [c[0] for c in calls] == ["sparse"] and calls[0][1] is grid and 0.05 < float(grid.occupied) < 0.95
    calls.clear()
    hand, pose_h, batch_h = _pose_trainer(str(tmp_path), None)
    monkeypatch.setattr(ops, "propose", lambda *a, **k: real_sparse(*a[:7], hand.occupancy_grid, *a[7:], **k))
    loss_hand, grads_hand = _pose_step(hand, pose_h, batch_h)
    assert torch.equal(hand.occupancy_grid.bits, grid.bits)
    assert torch.equal(_bits(loss_on), _bits(loss_hand))
    for g, w in zip(grads_on, grads_hand):
        assert torch.equal(_bits(g), _bits(w)) and bool(torch.isfinite(g).all())
    assert any(float(g.abs().max()) > 0 for g in grads_on)


# ---------------------------------------------------------------------------------------------------------------- 10. no host sync
def _armed(step):
    step()                                                # lazy initialisations (tables, packed weights, the grid) happen once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(4, device='cuda').nonzero()       # the mode is armed: a synchronising call raises
        return step()
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_a_render_with_the_key_makes_no_device_to_host_sync():
    renderer, _ = _occ_renderer("uniform", True)
    pixels, depth, K, Wm, S, _, _ = tres._scene_inputs()

    def step():
        with torch.no_grad():
            return renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=True)
    out = _armed(step)
    assert bool(torch.isfinite(out['rgb']).all()) and renderer.occupancy_builds == 1


def test_a_refinement_step_with_the_key_makes_no_device_to_host_sync(tmp_path):
    import scene_writer
    scene_writer.write_scene(str(tmp_path), scene="toy", frames=4, size=(30, 40), seed=0)
    tpose, pose, batch = _pose_trainer(str(tmp_path), True)
    # The step's inputs are uploaded once, in front of the armed window: Trainer_pose.process_data_dict copies pageable host tensors (the
    # camera, the view index, an all-ones depth frame it makes itself), and this mode counts such an upload as synchronising.  The view
    # index stays on the host, where the loader leaves it (LearnPose reads it as a Python int).  Everything else of train_step runs armed:
    # the pose lookup, the pixel draw, the render with its sparse proposal, the loss, backward, the optimiser.
    prepared = tpose.process_data_dict(batch)
    prepared = tuple(prepared[:4]) + (prepared[4].cpu(),)
    tpose.process_data_dict = lambda data: prepared
    losses = _armed(lambda: tpose.train_step(batch))
    assert bool(torch.isfinite(losses['loss'])) and tpose.occupancy_builds == 1
