"""GPU (-m gpu): hierarchical sampling -- the resampling kernel (nnr_resample.hip through nnr.ops.resample) against the fp64 CPU restatement
tests/resample_ref.py and its structural guarantees; the Renderer with rendering.num_fine against the hand-made composition coarse
render -> resample -> render; no device-to-host synchronisation; the random-number generator's bookkeeping, alone and under data
parallelism; a short tools/train_scene.py --num-fine run."""
import os
import sys

import pytest
import torch

import resample_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nope-nerf_amd", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(64, 128), (128, 64), (32, 992), (3, 1)]
RAYS = [1, 1023, 4096]


def _inputs(R, Cn, F, with_xi=True):
    a, z = rr.make_inputs(R, Cn, seed=Cn * 1000 + F)
    xi = torch.rand(R, F, generator=torch.Generator().manual_seed(R + 7)) if with_xi else None
    return a, z, xi


def _run(a, z, xi, F):
    from nnr import ops
    z_all, fine = ops.resample(a.to(DEV), z.to(DEV), xi.to(DEV) if xi is not None else None, F, return_fine=True)
    return z_all.cpu(), fine.cpu()


# ---------------------------------------------------------------------------------------------------------------- 1. against fp64
@pytest.mark.parametrize("R", RAYS)
@pytest.mark.parametrize("Cn,F", SHAPES)
def test_kernel_inverts_the_fp64_cdf(Cn, F, R):
    """Judged in CDF space (positions are ill-conditioned where a bin holds only the 1e-5 floor): the fp64 piecewise-linear CDF at every
    fine sample the kernel returns equals its u_j within 3e-5 -- three times what the fp32 CPU restatement measures against fp64, for the
    kernel's different summation order; the definition's `den` guard alone allows 1e-5.  No sample is excluded.  In z only the median
    distance to the fp64 restatement is held (1e-6)."""
    a, z, xi = _inputs(R, Cn, F)
    z_all, fine = _run(a, z, xi, F)
    u = rr.u_of(xi, R, F)
    dist = rr.cdf_distance(a, z, fine, u)
    _, s64 = rr.resample_ref(a, z, xi, F, torch.float64)
    _, s32 = rr.resample_ref(a, z, xi, F, torch.float32)
    med = float((fine.double() - s64).abs().median())
    print("C=%d F=%d R=%d: CDF distance kernel %.3e (fp32 restatement %.3e), z median %.3e max %.3e"
          % (Cn, F, R, float(dist.max()), float(rr.cdf_distance(a, z, s32, u).max()), med, float((fine.double() - s64).abs().max())))
    assert float(dist.max()) <= 3e-5
    assert med <= 1e-6


def test_kernel_without_xi_uses_bin_centres():
    a, z, _ = _inputs(257, 64, 128)
    _, fine = _run(a, z, None, 128)
    u = rr.u_of(None, 257, 128)
    assert float(rr.cdf_distance(a, z, fine, u).max()) <= 3e-5
    _, same = _run(a, z, torch.full((257, 128), 0.5), 128)
    assert torch.equal(fine, same)


# ---------------------------------------------------------------------------------------------------------------- 2. structure
@pytest.mark.parametrize("R", RAYS)
@pytest.mark.parametrize("Cn,F", SHAPES + [(61, 70), (1000, 24)])
def test_rows_are_sorted_unions_with_coarse_first(Cn, F, R):
    a, z, xi = _inputs(R, Cn, F)
    z_all, fine = _run(a, z, xi, F)
    assert z_all.shape == (R, Cn + F) and fine.shape == (R, F)
    assert bool((z_all[:, 1:] >= z_all[:, :-1]).all())
    assert bool((fine[:, 1:] >= fine[:, :-1]).all())
    union = torch.sort(torch.cat([z, fine], dim=1), dim=1).values
    assert torch.equal(union.view(torch.int32), z_all.view(torch.int32))                   # the multiset, bitwise
    # ties: coarse i sits at i + #{fine < z_i}, fine j at j + #{coarse <= s_j}
    pos_c = torch.arange(Cn).unsqueeze(0) + torch.searchsorted(fine.contiguous(), z.contiguous(), right=False)
    pos_f = torch.arange(F).unsqueeze(0) + torch.searchsorted(z.contiguous(), fine.contiguous(), right=True)
    assert torch.equal(z_all.gather(1, pos_c), z) and torch.equal(z_all.gather(1, pos_f), fine)
    both = torch.cat([pos_c, pos_f], dim=1).sort(dim=1).values
    assert torch.equal(both, torch.arange(Cn + F).unsqueeze(0).expand(R, -1))              # a permutation: nothing lost, nothing twice


def test_exact_ties_between_fine_samples_and_coarse_depths():
    """Four tied coarse depths make three equal edges, m = that depth, and two zero-width bins that hold real mass: every fine sample whose u
    falls into them IS the coarse depth, bit for bit.  The row must still be the sorted union, every element at its own index + its rank in
    the other list with the coarse depths counted first (equal values: the order shows in the positions adding up to a permutation)."""
    Cn, F, R = 18, 32, 5
    a = torch.full((R, Cn), 0.2)
    z = torch.arange(Cn, dtype=torch.float32).repeat(R, 1)
    z[:, 5:9] = 5.0
    xi = torch.rand(R, F, generator=torch.Generator().manual_seed(2))
    z_all, fine = _run(a, z, xi, F)
    hits = (fine == 5.0).sum(dim=1)
    assert int(hits.min()) >= 2, hits                                                      # the construction does produce ties
    assert bool((z_all[:, 1:] >= z_all[:, :-1]).all())
    assert torch.equal(torch.sort(torch.cat([z, fine], dim=1), dim=1).values, z_all)
    pos_c = torch.arange(Cn).unsqueeze(0) + (fine.unsqueeze(1) < z.unsqueeze(2)).sum(dim=2)
    pos_f = torch.arange(F).unsqueeze(0) + (z.unsqueeze(1) <= fine.unsqueeze(2)).sum(dim=2)
    assert torch.equal(torch.cat([pos_c, pos_f], dim=1).sort(dim=1).values, torch.arange(Cn + F).unsqueeze(0).expand(R, -1))
    assert int((z_all == 5.0).sum(dim=1).min()) >= 6 and torch.equal(z_all.gather(1, pos_c), z) and torch.equal(z_all.gather(1, pos_f), fine)


@pytest.mark.parametrize("Cn,F", [(64, 128), (3, 1), (61, 70)])
def test_nan_poisons_exactly_its_ray(Cn, F):
    R = 37
    a, z, xi = _inputs(R, Cn, F)
    clean_all, clean_fine = _run(a, z, xi, F)
    a2, z2 = a.clone(), z.clone()
    a2[5, Cn // 2] = float('nan')
    z2[20, 0] = float('nan')
    z_all, fine = _run(a2, z2, xi, F)
    bad = torch.zeros(R, dtype=torch.bool)
    bad[5] = bad[20] = True
    assert bool(torch.isnan(z_all[bad]).all()) and bool(torch.isnan(fine[bad]).all())
    assert torch.equal(z_all[~bad], clean_all[~bad]) and torch.equal(fine[~bad], clean_fine[~bad])


def test_two_runs_are_bitwise_equal():
    a, z, xi = _inputs(4096, 64, 128)
    first = _run(a, z, xi, 128)
    second = _run(a, z, xi, 128)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


# ---------------------------------------------------------------------------------------------------------------- 3. end to end
R_E2E = 256


def _renderer(hidden, option, mfma, **extra):
    import model as mdl
    from test_host_logic import make_cfg
    rend = dict(num_points=64, sample_option=option, mfma_dtype=mfma, **extra)
    if option == 'ndc':
        rend.update(depth_range=[0.0, 1.0], dist_alpha=True)
    cfg = make_cfg(hidden, **rend)
    torch.manual_seed(11)
    net = mdl.OfficialStaticNerf(cfg)
    return mdl.Renderer(net, cfg['rendering'], device=torch.device(DEV)), cfg


def _scene_inputs():
    g = torch.Generator().manual_seed(3)
    pixels = (torch.rand(1, R_E2E, 2, generator=g) * 2 - 1).to(DEV)
    depth = (1.0 + torch.rand(1, R_E2E, 1, generator=g)).to(DEV)      # (feeds d_gt only, which the feature does not touch: the distortion's gradient is held by the trainer test below)
    K = torch.tensor([[[2.0, 0, 0, 0], [0, -2.0, 0, 0], [0, 0, -1.0, 0], [0, 0, 0, 1.0]]], device=DEV)
    Wm = torch.eye(4, device=DEV).unsqueeze(0)
    Wm[0, :3, 3] = torch.tensor([0.05, -0.02, 0.03])
    Wm = Wm.requires_grad_(True)                                                           # stands for the learnable pose
    S = torch.eye(4, device=DEV).unsqueeze(0)
    w_rgb = torch.randn(R_E2E, 3, generator=g).to(DEV) / R_E2E
    w_dist = torch.randn(R_E2E, generator=g).to(DEV) / R_E2E
    return pixels, depth, K, Wm, S, w_rgb, w_dist


def _collect(renderer, out_rgb, out_dist, alpha, z_vals, depth, Wm, w_rgb, w_dist):
    net = renderer.model
    for p in net.parameters():
        p.grad = None
    ((out_rgb.reshape(-1, 3) * w_rgb).sum() + (out_dist * w_dist).sum()).backward()
    grads = [p.grad.detach().clone() for p in net.parameters()] + [Wm.grad.detach().clone()]
    return [out_rgb.detach().reshape(-1, 3).clone(), out_dist.detach().clone(), alpha.detach().clone(), z_vals.detach().clone()], grads


def _by_hand(renderer, cfg, pixels, depth, K, Wm, S, add_noise, n_fine):
    """The render as rendering.py writes it, spelled out with the public operators: ray set-up, (NDC warp,) the z tables and the
    jitter draw of today's sampling; with n_fine: coarse render under no_grad -> ops.resample -> render with jitter = z_all."""
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
    if n_fine:
        xi = torch.rand(R_E2E, n_fine, device=DEV) if jitter is not None else None
        with torch.no_grad():
            _, _, a_c, z_c = nnr.render_rays(pts_o, pts_d, view, z_lo, z_hi, jitter, net.weights(), net.biases(), samples=True, **kw)
        z_all = ops.resample(a_c, z_c, xi, n_fine)
        assert not z_all.requires_grad
        n_all = C0 + n_fine
        z_lo, z_hi, jitter = torch.zeros(n_all, device=DEV), torch.ones(n_all, device=DEV), z_all
    return nnr.render_rays(pts_o, pts_d, view, z_lo, z_hi, jitter, net.weights(), net.biases(), **kw)


@pytest.mark.parametrize("mfma", ["fp32", "bf16"])
@pytest.mark.parametrize("option,add_noise", [("uniform", True), ("uniform", False), ("ndc", False)])
@pytest.mark.parametrize("hidden", [128, 256])
def test_renderer_equals_the_hand_made_composition(hidden, option, add_noise, mfma):
    renderer, cfg = _renderer(hidden, option, mfma, num_fine=128)
    pixels, depth, K, Wm, S, w_rgb, w_dist = _scene_inputs()
    torch.cuda.manual_seed(99)
    out = renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=add_noise)
    assert out['z_vals'].shape == (R_E2E, 192) and out['alpha'].shape == (R_E2E, 192)
    got = _collect(renderer, out['rgb'], out['dist_dense'], out['alpha'], out['z_vals'], depth, Wm, w_rgb, w_dist)
    Wm.grad = None
    torch.cuda.manual_seed(99)
    rgb, dist, alpha, zv = _by_hand(renderer, cfg, pixels, depth, K, Wm, S, add_noise, 128)
    want = _collect(renderer, rgb, dist, alpha, zv, depth, Wm, w_rgb, w_dist)
    for part_got, part_want in zip(got, want):
        assert len(part_got) == len(part_want)
        for i, (g, w) in enumerate(zip(part_got, part_want)):
            assert torch.equal(g, w), i
    assert bool(torch.isfinite(got[0][0]).all()) and all(bool(torch.isfinite(g).all()) for g in got[1])
    assert bool((got[0][3][:, 1:] >= got[0][3][:, :-1]).all())
    assert any(float(g.abs().max()) > 0 for g in got[1][:-1]) and float(got[1][-1].abs().max()) > 0      # gradients do arrive


def test_evaluation_render_returns_fine_pass_samples_lazily():
    renderer, cfg = _renderer(128, "uniform", "fp32", num_fine=128)
    pixels, depth, K, Wm, S, _, _ = _scene_inputs()
    with torch.no_grad():
        out = renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=False, eval_=True)
        rgb, dist, alpha, zv = _by_hand(renderer, cfg, pixels, depth, K, Wm, S, False, 128)
    assert 'alpha' not in dict.keys(out)
    assert out['z_vals'].shape == (R_E2E, 192) and torch.equal(out['z_vals'], zv) and torch.equal(out['alpha'], alpha)
    assert float((out['rgb'].reshape(-1, 3) - rgb).abs().max()) <= 1e-5      # (the forward-only render composites in the MLP kernel's epilogue)


@pytest.mark.parametrize("option,add_noise", [("uniform", True), ("ndc", False)])
@pytest.mark.parametrize("mfma", ["fp32", "bf16"])
def test_num_fine_off_changes_nothing(option, add_noise, mfma):
    """Key absent and num_fine: 0 -- outputs and gradients bitwise those of the one render_rays call as written before the feature."""
    pixels, depth, K, Wm, S, w_rgb, w_dist = _scene_inputs()
    results = []
    for extra in ({}, {'num_fine': 0}, None):
        renderer, cfg = _renderer(128, option, mfma, **(extra or {}))
        Wm.grad = None
        torch.cuda.manual_seed(5)
        if extra is None:
            rgb, dist, alpha, zv = _by_hand(renderer, cfg, pixels, depth, K, Wm, S, add_noise, 0)
        else:
            assert ('num_fine' in cfg['rendering']) == bool(extra)
            out = renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=add_noise)
            rgb, dist, alpha, zv = out['rgb'], out['dist_dense'], out['alpha'], out['z_vals']
        assert zv.shape == (R_E2E, 64)
        results.append(list(_collect(renderer, rgb, dist, alpha, zv, depth, Wm, w_rgb, w_dist)) + [torch.cuda.get_rng_state()])
    for other in results[1:]:
        for part_a, part_b in zip(results[0][:2], other[:2]):
            for g, w in zip(part_a, part_b):
                assert torch.equal(g, w)
        assert torch.equal(results[0][2], other[2])


# ---------------------------------------------------------------------------------------------------------------- 4. no host sync
def test_num_fine_step_makes_no_device_to_host_sync():
    renderer, cfg = _renderer(128, "uniform", "fp32", num_fine=128)
    pixels, depth, K, Wm, S, w_rgb, w_dist = _scene_inputs()

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


# ---------------------------------------------------------------------------------------------------------------- 5. generator
def test_generator_advances_by_the_jitter_and_the_fine_draw():
    pixels, depth, K, Wm, S, _, _ = _scene_inputs()
    renderer, _ = _renderer(128, "uniform", "fp32", num_fine=128)
    plain, _ = _renderer(128, "uniform", "fp32")
    torch.cuda.manual_seed(42)
    torch.rand(1, R_E2E, 64, device=DEV)
    after_jitter = torch.cuda.get_rng_state()
    torch.rand(R_E2E, 128, device=DEV)
    after_both = torch.cuda.get_rng_state()
    assert not torch.equal(after_jitter, after_both)
    with torch.no_grad():
        torch.cuda.manual_seed(42)
        renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=True)
        assert torch.equal(torch.cuda.get_rng_state(), after_both)
        torch.cuda.manual_seed(42)
        plain.nope_nerf(pixels, depth, K, Wm, S, add_noise=True)
        assert torch.equal(torch.cuda.get_rng_state(), after_jitter)
        torch.cuda.manual_seed(42)
        start = torch.cuda.get_rng_state()
        renderer.nope_nerf(pixels, depth, K, Wm, S, add_noise=False)      # no draw at all, as today
        assert torch.equal(torch.cuda.get_rng_state(), start)
    ndc, _ = _renderer(128, "ndc", "fp32", num_fine=128)
    torch.cuda.manual_seed(42)
    with torch.no_grad():
        ndc.nope_nerf(pixels, depth, K, Wm, S, add_noise=True)           # NDC never jitters: xi = 0.5
    assert torch.equal(torch.cuda.get_rng_state(), start)


def _dp_step(case, n_rays, monkeypatch, n_fine, rank=0, world=1):
    import test_gpu_dp as dp
    from nnr import parallel
    monkeypatch.setattr(parallel, "rank", lambda: rank)
    monkeypatch.setattr(parallel, "world_size", lambda: world)
    monkeypatch.setattr(parallel.dist, "all_reduce", lambda t, op=None: t)        # keep this rank's share
    tr, mods, data = dp._trainer(case, n_rays)
    tr.model.renderer.cfg['num_fine'] = n_fine
    torch.manual_seed(321)
    torch.cuda.manual_seed(321)
    ld = tr.train_step(data, it=0, epoch=0, scheduling_start=10000, render_path=None)
    grads = [p.grad.detach().clone() for m in mods for p in m.parameters()]
    return {k: float(ld[k]) for k in ('loss', 'loss_rgb', 'loss_depth', 'l2_mean')}, grads, torch.cuda.get_rng_state()


@pytest.mark.parametrize("name,n_rays,world", [("tanks_d128", 61, 2), ("uniform_distalpha_masked_d128", 96, 2)])
def test_virtual_ranks_sum_to_single_process_with_num_fine(name, n_rays, world, monkeypatch):
    """The pattern and the tolerances of tests/test_gpu_dp.py with rendering.num_fine = 32: every rank draws its rows of the step's xi
    tensor after its rows of the jitter, and leaves the generator where the single-process step leaves it."""
    import golden_util as gu
    case = gu.load_case(name)
    ref_l, ref_g, ref_state = _dp_step(case, n_rays, monkeypatch, 32)
    parts = [_dp_step(case, n_rays, monkeypatch, 32, r, world) for r in range(world)]
    for k, v in ref_l.items():
        total = sum(p[0][k] for p in parts)
        assert abs(total - v) <= 1e-5 * max(1.0, abs(v)), (k, total, v)
    for i, r in enumerate(ref_g):
        scale = max(1.0, float(r.abs().max()))
        assert float((sum(p[1][i] for p in parts) - r).abs().max()) / scale <= 2e-5
    for p in parts:
        assert torch.equal(p[2], ref_state)
    off_l, _, off_state = _dp_step(case, n_rays, monkeypatch, 0)
    assert not torch.equal(off_state, ref_state) and off_l['loss'] != ref_l['loss']      # the feature was on in the runs above


# ---------------------------------------------------------------------------------------------------------------- 6. training run
def test_short_scene_training_with_num_fine(tmp_path):
    import scene_writer
    import train_scene
    scene_writer.write_scene(str(tmp_path), scene="toy", frames=6, size=(48, 64), seed=3)
    res = train_scene.run(str(tmp_path), "toy", epochs=4, log_every=1, n_rays=256, n_samples=64, hidden=128, sample_rate=10 ** 6,
                          num_fine=128)
    assert res["steps"] == 4 * 6 and res["fine_samples_per_ray"] == 128
    assert all(c["psnr"] is not None and torch.isfinite(torch.tensor(c["psnr"])) for c in res["curve"][1:]), res["curve"]
    assert all(bool(torch.isfinite(torch.tensor([c["ate"], c["rpe_rot_deg"]])).all()) for c in res["curve"][1:])
