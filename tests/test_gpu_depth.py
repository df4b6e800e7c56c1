"""GPU (-m gpu): the fused depth kernel (nnr_depth_f16.hip through nnr_render_depth / nnr.ops.render_depth).
  * its samples: the raw densities against nnr.ops.mlp_points(., split2=True) on host-built points and the depths against the forward's
    and the host's, all bit for bit (the kernel runs the pass and the sampling expressions of the other density-only kernels);
  * its compositing: (depth, acc) against a float64 compositing of the kernel's own samples (tests/fusion_ref.py) and against
    nnr.render_rays' forward-only depth, at the project's output bar |x - ref| <= 1e-4 max(1, |ref|);
  * determinism, the guard bands around the (R,2) output, the NaN rule and the refused configurations.
Shapes: one ray and one sample; fewer rays than a workgroup's four; C = 32 and 33 (one pass, one pass and one sample); several workgroups
with a short last one; and the limit C = 256 with lanes that own four samples each.  Random networks everywhere; the fitted networks of
tests/golden/phong_d{128,256}.npz supply rays that end on a surface."""
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

import fusion_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(ROOT, "tests", "golden")
LAYERS = ("layers0.0", "layers0.2", "layers0.4", "layers0.6", "layers1.0", "layers1.2", "layers1.4", "layers1.6", "fc_density",
          "fc_feature", "rgb_layers.0", "fc_rgb")
GUARD = 256
SENTINEL = 0x7fc0beef             # a NaN with a payload no kernel writes
E_UNSUPPORTED = -2
SHAPES = [(1, 1), (5, 3), (6, 32), (7, 33), (130, 64), (1023, 256)]
BAR = 1e-4


def _model_cfg(hidden):
    return {'model': {'hidden_dim': hidden, 'pos_enc_levels': 10, 'dir_enc_levels': 4, 'occ_activation': 'softplus'},
            'rendering': {'white_background': False, 'dist_alpha': False}}


@functools.lru_cache(maxsize=None)
def _net(hidden, kind):
    import model as mdl
    torch.manual_seed(41 + hidden)
    net = mdl.OfficialStaticNerf(_model_cfg(hidden))
    if kind == 'fitted':      # the network fitted to a sphere and a box that the phong goldens were rendered from
        gold = np.load(os.path.join(GOLDEN, "phong_d%d.npz" % hidden))
        sd = {}
        for n in LAYERS:
            q, e = torch.from_numpy(gold[n + ".q"].astype(np.float32)), torch.from_numpy(gold[n + ".e"].astype(np.float32))
            sd[n + ".weight"] = q * torch.exp2(e)[:, None]
            sd[n + ".bias"] = torch.from_numpy(gold[n + ".bias"])
        net.load_state_dict(sd)
    return net.to(DEV)


@functools.lru_cache(maxsize=None)
def _rays(n_rays, n_samples, kind):
    """origins, unit directions towards the scene, stratified z tables and a jitter; fitted: from a shell of radius 3.5 towards the shape"""
    g = torch.Generator().manual_seed(1000 * n_rays + n_samples)
    if kind == 'fitted':
        o = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=1) * 3.5
        target = (torch.rand(n_rays, 3, generator=g) - 0.5) * 2.0
        near, far = 0.1, 7.0
    else:
        o = (torch.rand(n_rays, 3, generator=g) - 0.5)
        target = o + torch.randn(n_rays, 3, generator=g)
        near, far = 0.05, 3.0
    d = torch.nn.functional.normalize(target - o, dim=1)
    z = torch.linspace(near, far, n_samples)
    if n_samples > 1:
        mid = .5 * (z[1:] + z[:-1])
        lo, hi = torch.cat([z[:1], mid]), torch.cat([mid, z[-1:]])
    else:
        lo = hi = z
    jit = torch.rand(n_rays, n_samples, generator=g)
    return tuple(t.contiguous().to(DEV) for t in (o, d, lo, hi, jit))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _flags(dist_alpha, relu):
    return dict(dist_alpha=bool(dist_alpha), relu_sigma=bool(relu))


def _depth_guarded(net, hidden, rays, dist_alpha, relu, debug=True, flags=None, n_samples=None):
    """nnr_render_depth through the C ABI into the middle of a sentinel-filled buffer -> (rc, out (R,2), guard bands, raw, z)"""
    from nnr import lib as L
    from nnr import ops
    o, d, lo, hi, jit = rays
    n_rays, n = o.shape[0], (lo.shape[0] if n_samples is None else n_samples)
    cfg = ops.split2_cfg(n_rays, n, hidden, **_flags(dist_alpha, relu))
    packed = ops._packed_for(ops.split2_cfg(n_rays, lo.shape[0], hidden), net.weights(), net.biases())
    if flags is not None:
        cfg.flags = flags
    buf = torch.full((2 * n_rays + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    raw = torch.full((n_rays, lo.shape[0]), float('nan'), device=DEV) if debug else None
    zv = torch.full((n_rays, lo.shape[0]), float('nan'), device=DEV) if debug else None
    rc = L.load().nnr_render_depth(C.byref(cfg), L.ptr(o), L.ptr(d), L.ptr(lo), L.ptr(hi), L.ptr(jit), L.ptr(packed),
                                   C.c_void_p(buf.data_ptr() + 4 * GUARD), L.ptr(raw), L.ptr(zv), L.stream())
    torch.cuda.synchronize()
    return rc, buf[GUARD:GUARD + 2 * n_rays].view(torch.float32).view(n_rays, 2), torch.cat([buf[:GUARD], buf[GUARD + 2 * n_rays:]]), raw, zv


def _worst(got, ref):
    """the largest |x - ref| / max(1, |ref|) of a float32 result against a float64 reference"""
    ref = ref.double().cpu()
    return float(((got.double().cpu() - ref).abs() / ref.abs().clamp(min=1.)).max())


def _check(hidden, kind, dist_alpha, relu, shape, capsys):
    import nnr
    from nnr import ops
    n_rays, n = shape
    net = _net(hidden, kind)
    rays = _rays(n_rays, n, kind)
    o, d, lo, hi, jit = rays
    rc, out, guard, raw, zv = _depth_guarded(net, hidden, rays, dist_alpha, relu)
    assert rc == 0
    assert bool((guard == SENTINEL).all()), "the kernel wrote outside its output"
    assert not bool((_bits(out) == SENTINEL).any()), "a ray was not written"
    assert torch.isfinite(out).all() and torch.isfinite(raw).all()

    # the samples: depths and points built on the host.  hipcc contracts z = z_lo + (z_hi - z_lo) jitter and p = o + d z into one fused
    # multiply-add each, in this kernel as in the forward kernel (the same expressions): the host restates them with an exact fma
    lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
    z_host = R.fma32((hi_h - lo_h)[None, :], jit.cpu().numpy(), lo_h[None, :])
    assert np.array_equal(zv.cpu().numpy().view(np.int32), z_host.view(np.int32))
    pts = R.fma32(d.cpu().numpy()[:, None, :], z_host[:, :, None], o.cpu().numpy()[:, None, :]).reshape(-1, 3)
    pts = torch.from_numpy(pts).to(DEV)
    want_raw = ops.mlp_points(pts, torch.zeros_like(pts), net.weights(), net.biases(), hidden=hidden, split2=True)[1].view(n_rays, n)
    assert torch.equal(_bits(raw), _bits(want_raw)), "%d of %d raw densities differ from mlp_points" % (
        int((_bits(raw) != _bits(want_raw)).sum()), raw.numel())

    # the forward with the default products: its z bit for bit, its depth and accumulated weight at the bar
    with torch.no_grad():
        _, dist, alpha_f, z_f = nnr.render_rays(o, d, -d, lo, hi, jit, net.weights(), net.biases(), hidden=hidden, white_bg=False,
                                                samples=True, **_flags(dist_alpha, relu))
    assert torch.equal(_bits(zv), _bits(z_f.view(n_rays, n)))
    ref = R.composite_ref(R.alpha_ref(raw, zv, dist_alpha, relu), zv)
    fwd = torch.stack([dist.double().cpu(), R.composite_ref(alpha_f, z_f.view(n_rays, n))[:, 1]], 1)
    w64, wf = _worst(out, ref), _worst(out, fwd)
    with capsys.disabled():
        print("\ndepth D=%d %s %s%s R=%d C=%d: worst |x - ref| / max(1, |ref|): %.3e against float64 compositing, %.3e against render_rays; "
              "acc in [%.3f, %.3f]" % (hidden, kind, "relu" if relu else "softplus", " dist_alpha" if dist_alpha else "", n_rays, n, w64, wf,
                                      float(out[:, 1].min()), float(out[:, 1].max())))
    assert w64 <= BAR and wf <= BAR

    # ops.render_depth is that entry point; two runs agree bit for bit
    again = ops.render_depth(o, d, lo, hi, jit, net.weights(), net.biases(), hidden=hidden, **_flags(dist_alpha, relu))
    assert again.shape == (n_rays, 2) and torch.equal(_bits(again), _bits(out))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R%dxC%d" % s)
@pytest.mark.parametrize("dist_alpha", [False, True], ids=["alpha", "dist_alpha"])
@pytest.mark.parametrize("relu", [False, True], ids=["softplus", "relu"])
@pytest.mark.parametrize("hidden", [128, 256])
def test_depth_kernel_on_random_networks(hidden, relu, dist_alpha, shape, capsys):
    _check(hidden, 'random', dist_alpha, relu, shape, capsys)


@pytest.mark.parametrize("shape", [(130, 64), (1023, 256)], ids=lambda s: "R%dxC%d" % s)
@pytest.mark.parametrize("dist_alpha", [False, True], ids=["alpha", "dist_alpha"])
@pytest.mark.parametrize("hidden", [128, 256])
def test_depth_kernel_on_rays_that_end_on_the_fitted_surface(hidden, dist_alpha, shape, capsys):
    out = _check(hidden, 'fitted', dist_alpha, False, shape, capsys)
    hit = out[:, 1] > 0.5
    assert bool(hit.any()), "no ray of the fitted scene ends on a surface: the fixture does not test what it is here for"
    assert float(out[hit, 0].min()) > 0.5 and float(out[hit, 0].max()) < 7.


@pytest.mark.parametrize("hidden", [128, 256])
@pytest.mark.parametrize("bad", [float('inf'), float('nan')])
def test_a_ray_that_is_not_finite_is_nan_and_its_workgroup_is_untouched(hidden, bad):
    net = _net(hidden, 'random')
    rays = _rays(7, 33, 'random')
    _, clean, _, _, _ = _depth_guarded(net, hidden, rays, False, False)
    o = rays[0].clone()
    o[5, 0] = bad                                                  # rays 4..6 share the second workgroup
    rc, out, guard, raw, zv = _depth_guarded(net, hidden, (o,) + rays[1:], False, False)
    assert rc == 0 and bool((guard == SENTINEL).all())
    assert bool(torch.isnan(out[5]).all()) and bool(torch.isnan(raw[5]).all())
    keep = [0, 1, 2, 3, 4, 6]
    assert torch.equal(_bits(out[keep]), _bits(clean[keep]))


def test_refused_configurations_are_unsupported():
    from nnr import lib as L
    net = _net(128, 'random')
    rays = _rays(6, 32, 'random')
    s2 = L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    rc, out, guard, _, _ = _depth_guarded(net, 128, rays, False, False, debug=False, n_samples=257)
    assert rc == E_UNSUPPORTED and bool((_bits(out) == SENTINEL).all()) and bool((guard == SENTINEL).all())
    for flags in (s2 | L.NNR_F_TRAIN, s2 | L.NNR_F_BF16, L.NNR_F_SPLIT3, 0):
        rc, out, guard, _, _ = _depth_guarded(net, 128, rays, False, False, debug=False, flags=flags)
        assert rc == E_UNSUPPORTED and bool((_bits(out) == SENTINEL).all()), flags
