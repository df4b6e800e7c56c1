"""GPU (-m gpu): the fused proposal stage of hierarchical sampling (nnr_propose_f16.hip through nnr.ops.propose; rendering.proposal:
'density').  The kernel's depths against the forward kernel's, its resampling against nnr_resample fed with the kernel's own alphas and
depths, its alphas against the existing coarse pass (all bitwise: same inputs, same fixed-order arithmetic); the Renderer with the key
against the hand-made composition and against 'render'; NaN containment, determinism, no device-to-host synchronisation, the generator's
bookkeeping alone and under data parallelism, a short training run."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nope-nerf_amd", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

import test_gpu_resample as tres      # noqa: E402 -- the end-to-end helpers of the 'render' mode's tests

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _net(hidden, kind):
    """'fitted': the networks of tests/golden/phong_d*.npz (a sphere and a box: structure in the density).  'random': a fresh network with the
    density head's row scaled up, so that alpha spreads over (0, 1) instead of sitting at 1 - exp(-softplus(~0)).  'hot': 'random' with the
    first layer times 64 -- activations 64 times larger all the way down: still far inside fp16's range for points of the scene, outside it
    for a point 3e4 away (the identity block of the position encoding)."""
    import model as mdl
    from test_host_logic import make_cfg
    net = mdl.OfficialStaticNerf(make_cfg(hidden))
    if kind == 'fitted':
        import test_gpu_phong as tp
        net.load_state_dict(tp._state_dict(tp._gold(hidden)))
    else:
        torch.manual_seed(17 + hidden)
        net = mdl.OfficialStaticNerf(make_cfg(hidden))
        with torch.no_grad():
            net.fc_density.weight.mul_(40.0)
            if kind == 'hot':
                net.layers0[0].weight.mul_(64.0)
    return net.to(DEV)


def _rays(R, seed):
    """Cameras 2.5 from the origin looking at points of the unit ball: the rays cross the fitted scene between z = 1 and z = 4."""
    g = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 2.5
    t = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * torch.rand(R, 1, generator=g) ** (1 / 3)
    d = torch.nn.functional.normalize(t - o, dim=-1)
    return o.to(DEV), d.to(DEV)


def _tables(Cn, stratified, near=1.0, far=4.0):
    z = torch.linspace(near, far, Cn)
    if stratified:
        mid = .5 * (z[1:] + z[:-1])
        return torch.cat([z[:1], mid]).to(DEV), torch.cat([mid, z[-1:]]).to(DEV)
    return z.to(DEV), z.clone().to(DEV)


def _inputs(R, Cn, F, jitter, xi, seed=0):
    o, d = _rays(R, 100 + R + seed)
    g = torch.Generator().manual_seed(R * 7 + Cn + seed)
    jit = torch.rand(R, Cn, generator=g).to(DEV) if jitter else None
    x = torch.rand(R, F, generator=g).to(DEV) if xi else None
    z_lo, z_hi = _tables(Cn, jitter)
    return o, d, z_lo, z_hi, jit, x


def _propose(net, hidden, inp, F, dist_alpha=False, relu_sigma=False):
    from nnr import ops
    o, d, z_lo, z_hi, jit, xi = inp
    return ops.propose(o, d, z_lo, z_hi, jit, xi, F, net.weights(), net.biases(), hidden=hidden, dist_alpha=dist_alpha, relu_sigma=relu_sigma,
                       debug=True)


def _coarse(net, hidden, inp, dist_alpha=False, relu_sigma=False):
    """alpha, z of the existing coarse pass: render_rays under no_grad, products split2 (the default)."""
    import nnr
    from nnr import lib as L
    assert L.fp32_products() == "split2"
    o, d, z_lo, z_hi, jit, _ = inp
    with torch.no_grad():
        return nnr.render_rays(o, d, -d, z_lo, z_hi, jit, net.weights(), net.biases(), hidden=hidden, dist_alpha=dist_alpha, white_bg=False,
                               relu_sigma=relu_sigma, samples=True)[2:]


def _bits(t):
    return t.contiguous().view(torch.int32)


# (hidden, net, C, F, R, mode, jitter, xi): every shape of the list at both widths; every R, mode and input combination at least twice
SHAPES = [(64, 128), (33, 7), (3, 1), (100, 60), (256, 768)]
CASES = [(128, 'fitted', 64, 128, 67, 'softplus', True, True), (256, 'fitted', 64, 128, 67, 'softplus', True, True),
         (128, 'random', 64, 128, 5, 'dist_alpha', True, True), (256, 'random', 64, 128, 1, 'relu', False, False),
         (128, 'random', 33, 7, 5, 'softplus', True, False), (256, 'fitted', 33, 7, 67, 'dist_alpha', False, True),
         (128, 'fitted', 3, 1, 1, 'softplus', False, False), (256, 'random', 3, 1, 5, 'dist_alpha', True, True),
         (128, 'random', 3, 1, 67, 'relu', True, True),
         (128, 'fitted', 100, 60, 67, 'relu', True, True), (256, 'random', 100, 60, 5, 'softplus', False, True),
         (128, 'random', 100, 60, 1, 'dist_alpha', True, False),
         (128, 'fitted', 256, 768, 5, 'dist_alpha', True, True), (256, 'fitted', 256, 768, 67, 'softplus', True, True),
         (256, 'random', 256, 768, 1, 'relu', False, False)]


def _mode_kw(mode):
    return dict(dist_alpha=mode == 'dist_alpha', relu_sigma=mode == 'relu')


@functools.lru_cache(maxsize=None)
def _case(hidden, kind, Cn, F, R, mode, jitter, xi):
    net = _net(hidden, kind)
    inp = _inputs(R, Cn, F, jitter, xi)
    got = _propose(net, hidden, inp, F, **_mode_kw(mode))
    ref = _coarse(net, hidden, inp, **_mode_kw(mode))
    return inp, got, ref


# ---------------------------------------------------------------------------------------------------------------- 1-3. the kernel
@pytest.mark.parametrize("hidden,kind,Cn,F,R,mode,jitter,xi", CASES)
def test_depths_are_the_forward_kernels(hidden, kind, Cn, F, R, mode, jitter, xi):
    _, (z_all, alpha_c, z_c, fine), (_, z_ref) = _case(hidden, kind, Cn, F, R, mode, jitter, xi)
    assert z_c.shape == (R, Cn) and z_all.shape == (R, Cn + F) and fine.shape == (R, F)
    assert torch.equal(_bits(z_c), _bits(z_ref))


@pytest.mark.parametrize("hidden,kind,Cn,F,R,mode,jitter,xi", CASES)
def test_rows_are_nnr_resamples_on_the_kernels_own_alphas(hidden, kind, Cn, F, R, mode, jitter, xi):
    """Same inputs, same fixed-order arithmetic (csrc/nnr_resample_row.h in both kernels): no tolerance.  Sortedness, coarse-first ties and
    the clamp are nnr_resample's (tests/test_gpu_resample.py)."""
    from nnr import ops
    inp, (z_all, alpha_c, z_c, fine), _ = _case(hidden, kind, Cn, F, R, mode, jitter, xi)
    want_all, want_fine = ops.resample(alpha_c, z_c, inp[5], F, return_fine=True)
    assert bool(torch.isfinite(z_all).all())
    assert torch.equal(_bits(z_all), _bits(want_all)) and torch.equal(_bits(fine), _bits(want_fine))
    assert bool((z_all[:, 1:] >= z_all[:, :-1]).all())


@pytest.mark.parametrize("hidden,kind,Cn,F,R,mode,jitter,xi", CASES)
def test_alphas_are_the_coarse_passes(hidden, kind, Cn, F, R, mode, jitter, xi):
    """Both kernels run nnr_trunk_f16.inc, the same head products and the compositor's sample_alpha: bitwise.  The networks have structure:
    the alphas of a case are not all alike (a flat CDF would hide a wrong density)."""
    _, (_, alpha_c, _, _), (a_ref, _) = _case(hidden, kind, Cn, F, R, mode, jitter, xi)
    diff = float((alpha_c.double() - a_ref.double()).abs().max())
    print("D=%d %s C=%d F=%d R=%d %s: max |alpha - coarse pass| %.3e; alpha in [%.3g, %.3g], mean %.3g"
          % (hidden, kind, Cn, F, R, mode, diff, float(a_ref.min()), float(a_ref.max()), float(a_ref.mean())))
    assert torch.equal(_bits(alpha_c), _bits(a_ref))
    if R * Cn >= 300:      # (a handful of samples of one ray may all lie in empty space)
        inner = a_ref[:, :-1] if mode == 'dist_alpha' else a_ref      # (dist_alpha: the last alpha is 1 by definition)
        assert float(inner.max()) - float(inner.min()) > 0.05


# ---------------------------------------------------------------------------------------------------------------- 4-5. the Renderer
R_E2E = tres.R_E2E


def _by_hand_density(renderer, cfg, pixels, depth, K, Wm, S, add_noise, n_fine):
    """tests/test_gpu_resample.py::_by_hand with the coarse render + ops.resample pair replaced by ops.propose."""
    import nnr
    from nnr import camera, ops
    rc, net = cfg['rendering'], renderer.model
    C0 = rc['num_points'] - rc['outside_steps']
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
    kw = dict(hidden=net.hidden_dim, dist_alpha=bool(rc['dist_alpha']), white_bg=False, relu_sigma=False, bf16=rc['mfma_dtype'] == 'bf16')
    xi = torch.rand(R_E2E, n_fine, device=DEV) if jitter is not None else None
    z_all = ops.propose(pts_o, pts_d, z_lo, z_hi, jitter, xi, n_fine, net.weights(), net.biases(), hidden=kw['hidden'],
                        dist_alpha=kw['dist_alpha'], relu_sigma=False)
    assert not z_all.requires_grad
    n_all = C0 + n_fine
    return nnr.render_rays(pts_o, pts_d, view, torch.zeros(n_all, device=DEV), torch.ones(n_all, device=DEV), z_all, net.weights(), net.biases(), **kw)


def _render(renderer, inputs, add_noise, seed=99):
    pixels, depth, K, Wm, S, w_rgb, w_dist = inputs
    Wm.grad = None
    torch.cuda.manual_seed(seed)
    out = renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=add_noise)
    res = tres._collect(renderer, out['rgb'], out['dist_dense'], out['alpha'], out['z_vals'], depth, Wm, w_rgb, w_dist)
    return res, torch.cuda.get_rng_state()


def _same(got, want):
    for part_got, part_want in zip(got, want):
        assert len(part_got) == len(part_want)
        for i, (g, w) in enumerate(zip(part_got, part_want)):
            assert torch.equal(g, w), i


@pytest.mark.parametrize("mfma", ["fp32", "bf16"])
@pytest.mark.parametrize("option,add_noise", [("uniform", True), ("uniform", False), ("ndc", False)])
def test_density_renderer_equals_the_hand_made_composition(option, add_noise, mfma):
    renderer, cfg = tres._renderer(128, option, mfma, num_fine=128, proposal='density')
    inputs = tres._scene_inputs()
    pixels, depth, K, Wm, S, w_rgb, w_dist = inputs
    got, _ = _render(renderer, inputs, add_noise)
    Wm.grad = None
    torch.cuda.manual_seed(99)
    rgb, dist, alpha, zv = _by_hand_density(renderer, cfg, pixels, depth, K, Wm, S, add_noise, 128)
    want = tres._collect(renderer, rgb, dist, alpha, zv, depth, Wm, w_rgb, w_dist)
    _same(got, want)
    assert got[0][3].shape == (R_E2E, 192) and bool((got[0][3][:, 1:] >= got[0][3][:, :-1]).all())
    assert bool(torch.isfinite(got[0][0]).all()) and all(bool(torch.isfinite(g).all()) for g in got[1])
    assert any(float(g.abs().max()) > 0 for g in got[1][:-1]) and float(got[1][-1].abs().max()) > 0      # gradients do arrive


@pytest.mark.parametrize("hidden", [128, 256])
@pytest.mark.parametrize("option,add_noise", [("uniform", True), ("ndc", False)])
def test_density_and_render_agree_bitwise_in_split2_products(hidden, option, add_noise):
    """The alphas are the coarse pass's bit for bit (above), so with the default products the two modes are one render."""
    inputs = tres._scene_inputs()
    res = []
    for proposal in ('render', 'density'):
        renderer, _ = tres._renderer(hidden, option, "fp32", num_fine=128, proposal=proposal)
        res.append(_render(renderer, inputs, add_noise))
    _same(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("option,add_noise,mfma", [("uniform", True, "fp32"), ("ndc", False, "bf16")])
def test_key_absent_is_render(option, add_noise, mfma):
    inputs = tres._scene_inputs()
    res = []
    for extra in ({}, {'proposal': 'render'}):
        renderer, cfg = tres._renderer(128, option, mfma, num_fine=128, **extra)
        assert ('proposal' in cfg['rendering']) == bool(extra)
        res.append(_render(renderer, inputs, add_noise))
    _same(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("option,add_noise", [("uniform", True), ("ndc", False)])
def test_proposal_is_ignored_without_num_fine(option, add_noise):
    """num_fine 0 or absent: the key -- 'density', or a value that would be refused with num_fine > 0 -- changes no bit of the render, of a
    gradient or of the generator's state."""
    inputs = tres._scene_inputs()
    res = []
    for extra in ({}, {'proposal': 'density'}, {'num_fine': 0, 'proposal': 'density'}, {'num_fine': 0, 'proposal': 'bogus'}):
        renderer, _ = tres._renderer(128, option, "fp32", **extra)
        res.append(_render(renderer, inputs, add_noise))
        assert res[-1][0][0][3].shape == (R_E2E, 64)
    for other in res[1:]:
        _same(res[0][0], other[0])
        assert torch.equal(res[0][1], other[1])


def test_unknown_proposal_is_refused_on_the_gpu_too():
    renderer, _ = tres._renderer(128, "uniform", "fp32", num_fine=128, proposal='bogus')
    pixels, depth, K, Wm, S, _, _ = tres._scene_inputs()
    with pytest.raises(ValueError, match="proposal"):
        renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=False)


# ---------------------------------------------------------------------------------------------------------------- 6-7. NaN, determinism
@pytest.mark.parametrize("hidden,Cn,F", [(128, 64, 128), (256, 33, 7)])
def test_nan_origin_poisons_exactly_its_ray(hidden, Cn, F):
    """Ray 5 of 7 (the second workgroup: rays 4, 5, 6 and a wave without a ray): its row, alphas and fine samples are NaN, its depths are
    not (they do not depend on the origin); every other ray is bitwise what it is without the NaN."""
    net = _net(hidden, 'random')
    inp = _inputs(7, Cn, F, True, True)
    clean = _propose(net, hidden, inp, F)
    o2 = inp[0].clone()
    o2[5, 1] = float('nan')
    z_all, alpha_c, z_c, fine = _propose(net, hidden, (o2,) + inp[1:], F)
    bad = torch.zeros(7, dtype=torch.bool, device=DEV)
    bad[5] = True
    assert bool(torch.isnan(z_all[bad]).all()) and bool(torch.isnan(fine[bad]).all()) and bool(torch.isnan(alpha_c[bad]).all())
    assert torch.equal(z_c, clean[2])
    for got, want in zip((z_all, alpha_c, fine), (clean[0], clean[1], clean[3])):
        assert torch.equal(_bits(got[~bad]), _bits(want[~bad])) and bool(torch.isfinite(got[~bad]).all())


@pytest.mark.parametrize("hidden", [128, 256])
def test_activation_outside_fp16_range_poisons_exactly_its_ray(hidden):
    """An input-value case: ray 2 of 6 starts 3e4 from the scene.  With the first layer times 64 its activations pass 65520, the kernel makes
    its samples NaN (nnr_trunk_f16.h: left_f16_range) and the row with them; the other rays are bitwise what they are with ray 2 at home.
    With the unscaled network the same far ray stays in range and finite: it is the range bound that fires, not the distance."""
    Cn, F = 64, 128
    inp = _inputs(6, Cn, F, True, True, seed=3)
    o2 = inp[0].clone()
    o2[2] = torch.tensor([3e4, -2e4, 1e4], device=DEV)
    far = (o2,) + inp[1:]
    hot, mild = _net(hidden, 'hot'), _net(hidden, 'random')
    clean = _propose(hot, hidden, inp, F)
    z_all, alpha_c, z_c, fine = _propose(hot, hidden, far, F)
    bad = torch.zeros(6, dtype=torch.bool, device=DEV)
    bad[2] = True
    assert bool(torch.isfinite(clean[0]).all())
    assert bool(torch.isnan(z_all[bad]).all()) and bool(torch.isnan(fine[bad]).all()) and bool(torch.isnan(alpha_c[bad]).any())
    for got, want in zip((z_all, alpha_c, fine), (clean[0], clean[1], clean[3])):
        assert torch.equal(_bits(got[~bad]), _bits(want[~bad]))
    assert all(bool(torch.isfinite(t).all()) for t in _propose(mild, hidden, far, F))


def test_two_runs_are_bitwise_equal():
    net = _net(256, 'fitted')
    inp = _inputs(67, 100, 60, True, True)
    first = _propose(net, 256, inp, 60, dist_alpha=True)
    second = _propose(net, 256, inp, 60, dist_alpha=True)
    for a, b in zip(first, second):
        assert torch.equal(_bits(a), _bits(b))


def test_debug_outputs_do_not_change_the_row():
    from nnr import ops
    net = _net(128, 'fitted')
    o, d, z_lo, z_hi, jit, xi = _inputs(67, 64, 128, True, True)
    kw = dict(hidden=128, dist_alpha=False, relu_sigma=False)
    plain = ops.propose(o, d, z_lo, z_hi, jit, xi, 128, net.weights(), net.biases(), **kw)
    assert torch.is_tensor(plain) and not plain.requires_grad
    assert torch.equal(_bits(plain), _bits(_case(128, 'fitted', 64, 128, 67, 'softplus', True, True)[1][0]))


# ---------------------------------------------------------------------------------------------------------------- 8. no host sync
def test_density_step_makes_no_device_to_host_sync():
    renderer, cfg = tres._renderer(128, "uniform", "fp32", num_fine=128, proposal='density')
    pixels, depth, K, Wm, S, w_rgb, w_dist = tres._scene_inputs()

    def step():
        out = renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=True)
        ((out['rgb'].reshape(-1, 3) * w_rgb).sum() + (out['dist_dense'] * w_dist).sum()).backward()
        return out
    step()                                                # lazy initialisations (tables, plan upload, packed weights) happen once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(4, device='cuda').nonzero()       # the mode is armed: a synchronising call raises
        out = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert out['z_vals'].shape == (R_E2E, 192) and bool(torch.isfinite(out['rgb']).all())


# ---------------------------------------------------------------------------------------------------------------- 9. generator
def test_generator_ends_where_render_leaves_it():
    pixels, depth, K, Wm, S, _, _ = tres._scene_inputs()
    states = {}
    for proposal in ('render', 'density'):
        renderer, _ = tres._renderer(128, "uniform", "fp32", num_fine=128, proposal=proposal)
        renderer.train()
        torch.cuda.manual_seed(42)
        start = torch.cuda.get_rng_state()
        renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=True)
        states[proposal] = torch.cuda.get_rng_state()
        assert not torch.equal(states[proposal], start)
    assert torch.equal(states['render'], states['density'])


# ---------------------------------------------------------------------------------------------------------------- 10. data parallel
def _dp_step(case, n_rays, monkeypatch, n_fine, proposal, rank=0, world=1):
    """tests/test_gpu_resample.py::_dp_step with the proposal key set."""
    import test_gpu_dp as dp
    from nnr import parallel
    monkeypatch.setattr(parallel, "rank", lambda: rank)
    monkeypatch.setattr(parallel, "world_size", lambda: world)
    monkeypatch.setattr(parallel.dist, "all_reduce", lambda t, op=None: t)        # keep this rank's share
    tr, mods, data = dp._trainer(case, n_rays)
    tr.model.renderer.cfg['num_fine'] = n_fine
    tr.model.renderer.cfg['proposal'] = proposal
    torch.manual_seed(321)
    torch.cuda.manual_seed(321)
    ld = tr.train_step(data, it=0, epoch=0, scheduling_start=10000, render_path=None)
    grads = [p.grad.detach().clone() for m in mods for p in m.parameters()]
    return {k: float(ld[k]) for k in ('loss', 'loss_rgb', 'loss_depth', 'l2_mean')}, grads, torch.cuda.get_rng_state()


def test_virtual_ranks_sum_to_single_process_with_density(monkeypatch):
    """The pattern and the bars of test_virtual_ranks_sum_to_single_process_with_num_fine, rendering.proposal = 'density'."""
    import golden_util as gu
    name, n_rays, world = "uniform_distalpha_masked_d128", 96, 2
    case = gu.load_case(name)
    ref_l, ref_g, ref_state = _dp_step(case, n_rays, monkeypatch, 32, 'density')
    parts = [_dp_step(case, n_rays, monkeypatch, 32, 'density', r, world) for r in range(world)]
    for k, v in ref_l.items():
        total = sum(p[0][k] for p in parts)
        assert abs(total - v) <= 1e-5 * max(1.0, abs(v)), (k, total, v)
    for i, r in enumerate(ref_g):
        scale = max(1.0, float(r.abs().max()))
        assert float((sum(p[1][i] for p in parts) - r).abs().max()) / scale <= 2e-5
    for p in parts:
        assert torch.equal(p[2], ref_state)
    off_l, _, off_state = _dp_step(case, n_rays, monkeypatch, 0, 'density')
    assert not torch.equal(off_state, ref_state) and off_l['loss'] != ref_l['loss']      # the feature was on in the runs above


# ---------------------------------------------------------------------------------------------------------------- 11. training run
def test_short_scene_training_with_density(tmp_path):
    import scene_writer
    import train_scene
    scene_writer.write_scene(str(tmp_path), scene="toy", frames=6, size=(48, 64), seed=3)
    res = train_scene.run(str(tmp_path), "toy", epochs=4, log_every=1, n_rays=256, n_samples=64, hidden=128, sample_rate=10 ** 6,
                          num_fine=128, proposal='density')
    assert res["steps"] == 4 * 6 and res["fine_samples_per_ray"] == 128 and res["proposal"] == 'density'
    assert all(c["psnr"] is not None and torch.isfinite(torch.tensor(c["psnr"])) for c in res["curve"][1:]), res["curve"]
    assert all(bool(torch.isfinite(torch.tensor([c["ate"], c["rpe_rot_deg"]])).all()) for c in res["curve"][1:])
