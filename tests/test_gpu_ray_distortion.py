"""GPU (-m gpu): the ray-distortion regulariser (include/nnr_regularise.h) -- its two kernels alone on plain and strided
tensors against the float64 definition of tests/ray_distortion_ref.py, through nnr.render_rays against the live oracle, shard additivity, and
model.Trainer with training.ray_distortion_weight absent, 0 and 0.01."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nope-nerf_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import nerf_oracle as orc          # noqa: E402
import ray_distortion_ref as RD    # noqa: E402
import trace_util                  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4                         # tests/test_gpu_parity.py's
S_NEAR, S_INV = 0.01, 1.0 / 9.99   # the coarse range of the inputs below
SHAPES = [(1, 1), (1, 2), (5, 3), (4, 63), (7, 64), (3, 65), (9, 129), (2, 1024)]
FLAG_SETS = [(False, False), (True, False), (False, True), (True, True)]      # (dist_alpha, relu_sigma)
EPS32 = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _case(R, N, dist_alpha, relu_sigma):
    """Inputs and the float64 reference of one (shape, flags): made once, shared by every test that needs them, never written to."""
    raw, z = RD.make_inputs(R, N)
    g = torch.randn(R, generator=torch.Generator().manual_seed(R + N)) + 0.25
    loss, grad = RD.loss_and_grad(raw, z, S_NEAR, S_INV, dist_alpha, relu_sigma, g)
    return raw, z, g, loss, grad


def _strided(t, stride, fill):
    """t (R,N) as column 3 of an (R N, stride) tensor on the GPU -> (the whole tensor, the (R,N) view); stride 1: t itself."""
    t = t.cuda()
    if stride == 1:
        return t, t
    R, N = t.shape
    whole = torch.full((R * N, stride), fill, device="cuda") + torch.arange(R * N * stride, device="cuda").view(R * N, stride)
    whole[:, 3] = t.reshape(-1)
    return whole, whole[:, 3].view(R, N)


def _ratio_grad(got, ref):
    """Worst |got - ref| over the per-element bar 2^-23 |ref| + 1e-10 max_ray |ref| (one fp32 rounding of a float64 value, doubled, plus a
    floor four orders above what two float64 evaluations of the definition differ by).  Where the bar is 0 (a ray whose gradient is exactly 0:
    N = 1, or no mass under a ReLU density) the values must be equal."""
    got = got.detach().cpu().double()
    bar = EPS32 * ref.abs() + 1e-10 * ref.abs().amax(dim=1, keepdim=True)
    err = (got - ref).abs()
    assert (err[bar == 0] == 0).all()
    return float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0


def _ratio_loss(got, ref):
    got = got.detach().cpu().double()
    return float(((got - ref).abs() / (EPS32 * ref.abs() + 1e-10 * ref.abs() + 1e-12)).max())


# ------------------------------------------------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("dist_alpha,relu_sigma", FLAG_SETS)
@pytest.mark.parametrize("R,N", SHAPES)
def test_kernels_alone_against_the_float64_definition(R, N, dist_alpha, relu_sigma, stride, capsys):
    from nnr import ops
    raw, z, g, ref_loss, ref_grad = _case(R, N, dist_alpha, relu_sigma)
    raw_whole, raw_v = _strided(raw, stride, 100.0)
    raw_before = raw_whole.clone()
    zd, gd = z.cuda(), g.cuda()
    loss = ops.ray_distortion(raw_v, zd, S_NEAR, S_INV, dist_alpha, relu_sigma)
    out_whole, out_v = _strided(torch.full((R, N), -7.0), stride, -300.0)
    out_before = out_whole.clone()
    ops.ray_distortion_grad(raw_v, zd, S_NEAR, S_INV, dist_alpha, relu_sigma, gd, out=out_v)      # accumulate = 0: overwrites the -7
    torch.cuda.synchronize()
    r_loss, r_grad = _ratio_loss(loss, ref_loss), _ratio_grad(out_v, ref_grad)
    with capsys.disabled():
        print("\n  ray distortion (%d,%d) dist_alpha=%d relu=%d stride %d: worst error / bar  loss %.3f  gradient %.3f"
              % (R, N, dist_alpha, relu_sigma, stride, r_loss, r_grad))
    assert r_loss <= 1.0 and r_grad <= 1.0, (r_loss, r_grad)
    assert torch.equal(raw_whole, raw_before)                                      # inputs untouched
    if stride > 1:
        keep = [c for c in range(stride) if c != 3]
        assert torch.equal(out_whole[:, keep], out_before[:, keep])                # the other columns bit-identical
    if N == 1:
        assert (loss == 0).all() and (out_v == 0).all()                            # exact zeros
    if R >= 2:
        # the ray without mass, under every flag set.  sum_j alpha_j <= softplus(-30) (z_N - z_0) <= 9.4e-14 x 10 (without dist_alpha: N x 9.4e-14)
        # and every |m_i - m_j| <= 1, so L <= 2 sum_{j < last} w_j + (sum_{j < last} w_j)^2 <= 2e-12; |dL/draw_j| <= |dL/dalpha_j| dalpha_j/draw_j
        # <= 2 x 10 x 9.4e-14 (dist_alpha: the closing sample holds all the weight, |a_j| <= 2), times |g|
        assert float(loss[-1]) <= 2e-12 and float(out_v[-1].abs().max()) <= 2e-12 * max(1.0, abs(float(g[-1])))
    # two runs agree bit for bit
    loss2 = ops.ray_distortion(raw_v, zd, S_NEAR, S_INV, dist_alpha, relu_sigma)
    grad2 = ops.ray_distortion_grad(raw_v, zd, S_NEAR, S_INV, dist_alpha, relu_sigma, gd)
    assert torch.equal(loss, loss2) and torch.equal(out_v, grad2)


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("R,N,dist_alpha,relu_sigma", [(3, 65, True, False), (9, 129, False, False), (5, 3, False, True), (2, 1024, True, True)])
def test_accumulate_adds_to_what_is_there_in_double(R, N, dist_alpha, relu_sigma, stride):
    from nnr import ops
    raw, z, g, _, ref_grad = _case(R, N, dist_alpha, relu_sigma)
    before = 0.01 * torch.randn(R, N, generator=torch.Generator().manual_seed(3))
    out_whole, out_v = _strided(before, stride, 50.0)
    whole_before = out_whole.clone()
    ops.ray_distortion_grad(raw.cuda(), z.cuda(), S_NEAR, S_INV, dist_alpha, relu_sigma, g.cuda(), out=out_v, accumulate=True)
    assert _ratio_grad(out_v, before.double() + ref_grad) <= 1.0
    if stride > 1:
        assert torch.equal(out_whole[:, :3], whole_before[:, :3])
    # and accumulate = 0 on the same buffer overwrites: the sum is gone
    ops.ray_distortion_grad(raw.cuda(), z.cuda(), S_NEAR, S_INV, dist_alpha, relu_sigma, g.cuda(), out=out_v, accumulate=False)
    assert _ratio_grad(out_v, ref_grad) <= 1.0
    assert torch.equal(out_v, ops.ray_distortion_grad(raw.cuda(), z.cuda(), S_NEAR, S_INV, dist_alpha, relu_sigma, g.cuda()))


@pytest.mark.parametrize("dist_alpha,relu_sigma", FLAG_SETS)
def test_a_nan_stays_in_its_ray(dist_alpha, relu_sigma):
    from nnr import ops
    R, N = 6, 65      # rays 0..3 share a workgroup with the poisoned one, rays 4, 5 are the next, two of its four waves idle
    raw, z, g, _, _ = _case(R, N, dist_alpha, relu_sigma)
    args = (z.cuda(), S_NEAR, S_INV, dist_alpha, relu_sigma)
    clean_l = ops.ray_distortion(raw.cuda(), *args)
    clean_g = ops.ray_distortion_grad(raw.cuda(), *args, g.cuda())
    bad = raw.clone()
    bad[1, 10] = float("nan")
    out = torch.full((R, N), -7.0, device="cuda")
    loss = ops.ray_distortion(bad.cuda(), *args)
    ops.ray_distortion_grad(bad.cuda(), *args, g.cuda(), out=out)
    assert torch.isnan(loss[1]) and torch.isnan(out[1]).all()
    rest = [0, 2, 3, 4, 5]
    assert torch.equal(loss[rest], clean_l[rest]) and torch.equal(out[rest], clean_g[rest])


# ------------------------------------------------------------------------------------------------------------ through the operator
def _synthetic(D, R, N, seed):
    g = torch.Generator().manual_seed(seed)
    params = orc.init_params(D, seed + 1)
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    o = (torch.randn(3, generator=g) * 0.1).expand(R, 3).contiguous()
    z = torch.linspace(0, 1, N)
    z = 0.01 * (1 - z) + 10 * z
    mid = 0.5 * (z[1:] + z[:-1])
    return params, o, d, torch.cat([z[:1], mid]), torch.cat([mid, z[-1:]]), torch.rand(R, N, generator=g)


def _hip(params, o, d, lo, hi, jit, up, *, D, ray_distortion, **kw):
    """nnr.render_rays and the backward of sum(rgb d_rgb) + sum(dist d_dist) [+ sum(dloss g)] -> outputs and gradients by name."""
    import nnr
    from nnr import lib as L
    dev = torch.device("cuda")
    d_rgb, d_dist, g = up
    w = [params[n + ".weight"].to(dev).requires_grad_(True) for n in L.LAYER_NAMES]
    b = [params[n + ".bias"].to(dev).requires_grad_(True) for n in L.LAYER_NAMES]
    oo, dd, vv = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True), (-d).to(dev).requires_grad_(True)
    out = nnr.render_rays(oo, dd, vv, lo.to(dev), hi.to(dev), jit.to(dev), w, b, hidden=D, ray_distortion=ray_distortion, **kw)
    loss = (out[0] * d_rgb.to(dev)).sum().add((out[1] * d_dist.to(dev)).sum())
    got = {"rgb": out[0], "dist": out[1]}
    if ray_distortion is not None:
        assert len(out) == 5
        got["dloss"] = out[4]
        if g is not None:
            loss = loss.add((out[4] * g.to(dev)).sum())
    else:
        assert len(out) == 4
    loss.backward()
    got.update({"d pts_o": oo.grad, "d pts_d": dd.grad, "d view": vv.grad})
    for i, n in enumerate(L.LAYER_NAMES):
        got["dW " + n], got["db " + n] = w[i].grad, b[i].grad
    return {k: v.detach() for k, v in got.items()}


def _render_bf16_oracle(params, o, d, v, lo, hi, jit, *, dist_alpha, white_bg, relu_sigma):
    """tests/test_gpu_parity.py's bf16-arithmetic oracle of the render, returning alpha and z too."""
    R, N = o.shape[0], lo.shape[0]
    z = lo + (hi - lo) * jit.view(R, N)
    pts = (o.unsqueeze(1) + d.unsqueeze(1) * z.unsqueeze(-1)).reshape(-1, 3)
    view = v.unsqueeze(1).expand(R, N, 3).reshape(-1, 3)
    rgb, occ = orc.mlp_bf16(params, pts, view, dist_alpha=dist_alpha, occ_activation="relu" if relu_sigma else "softplus")
    alpha = occ.view(R, N)
    if dist_alpha:
        delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10)], dim=-1)
        alpha = 1 - torch.exp(-1.0 * alpha * delta)
        alpha = torch.cat([alpha[:, :-1], torch.ones(R, 1)], dim=-1)
    trans = torch.cumprod(torch.cat([torch.ones(R, 1), 1.0 - alpha + orc.EPS_T], -1), -1)[:, :-1]
    w = alpha * trans
    out = (w.unsqueeze(-1) * rgb.view(R, N, 3)).sum(-2)
    dist = (w * z).sum(-1)
    if white_bg:
        out = out + (1.0 - w.sum(-1, keepdim=True))
    return out, dist, alpha, z


def _oracle(params, o, d, lo, hi, jit, up, dt, *, dist_alpha, white_bg, relu_sigma, bf16=False):
    """The live oracle (its bf16-arithmetic flavour for the bf16 mode) plus the float64 definition of the distortion on ITS alpha and z."""
    from nnr import lib as L
    d_rgb, d_dist, g = up
    P = {k: v.clone().to(dt).requires_grad_(True) for k, v in params.items()}
    po, pd, pv = (t.clone().to(dt).requires_grad_(True) for t in (o, d, -d))
    kw = dict(dist_alpha=dist_alpha, white_bg=white_bg, relu_sigma=relu_sigma)
    if bf16:
        orgb, odist, alpha, z = _render_bf16_oracle(P, po, pd, pv, lo.to(dt), hi.to(dt), jit.to(dt), **kw)
    else:
        orgb, odist, t = trace_util.traced_render(P, po, pd, pv, lo.to(dt), hi.to(dt), jit.to(dt), **kw)
        alpha, z = t["alpha"], t["z"]
    dloss = RD.loss_from_alpha(alpha, z, S_NEAR, S_INV)
    ((orgb * d_rgb.to(dt)).sum().double() + (odist * d_dist.to(dt)).sum().double() + (dloss * g.double()).sum()).backward()
    out = {"rgb": orgb, "dist": odist, "dloss": dloss, "d pts_o": po.grad, "d pts_d": pd.grad, "d view": pv.grad}
    for n in L.LAYER_NAMES:
        out["dW " + n], out["db " + n] = P[n + ".weight"].grad, P[n + ".bias"].grad
    return {k: v.detach().double() for k, v in out.items()}


@pytest.mark.parametrize("D,R,N,dist_alpha,relu_sigma,bf16", [
    (128, 7, 17, False, False, False),
    (128, 33, 65, False, False, False),
    (256, 7, 17, False, False, False),      # 119 samples at D = 256: one class-A and one class-B workgroup in the weight gradient's plan
    (256, 33, 65, False, False, False),
    (256, 7, 17, True, False, False),       # dist_alpha
    (128, 33, 65, False, True, False),      # ReLU density
    (128, 33, 65, False, False, True),      # bf16 products in the MLP kernels; the regulariser is the same fp64-on-fp32 kernel
])
def test_operator_against_the_live_oracle(D, R, N, dist_alpha, relu_sigma, bf16):
    """Every output and every gradient of sum(rgb d_rgb) + sum(dist d_dist) + sum(dloss g).  fp32 modes: the rule of
    test_gpu_parity.py::test_ragged_shapes_and_every_flag_against_live_oracle, max(TOL scale, 4 x the fp32 oracle's own deviation from the fp64
    one).  bf16: the bars of that file's bf16 tests against the bf16-arithmetic oracle (outputs 3e-3 / 3e-4 on average of the largest value,
    gradients 3e-2 in relative L2, 1e-1 for the rays' own).  Then g = 0: the gradients of ray_distortion=None, bit for bit.
    (D = 256 at 7 x 17 is the shape that showed the weight-gradient kernel's overlapping private staging areas, DESIGN.md section 13: the
    fc_feature / rgb_layers.0 gradients of these cases, and the bit-identity of repeated runs, hold only with that fixed.)"""
    params, o, d, lo, hi, jit = _synthetic(D, R, N, seed=41 + R)
    gen = torch.Generator().manual_seed(5)
    up = (torch.randn(R, 3, generator=gen) / R, torch.randn(R, generator=gen) / R, torch.randn(R, generator=gen) / R + 1.0 / R)
    kw = dict(dist_alpha=dist_alpha, white_bg=False, relu_sigma=relu_sigma)
    got = _hip(params, o, d, lo, hi, jit, up, D=D, ray_distortion=(S_NEAR, S_INV), bf16=bf16, **kw)
    assert got["dloss"].shape == (R,) and bool((got["dloss"] >= 0).all())
    if not bf16:
        ref, ref32 = (_oracle(params, o, d, lo, hi, jit, up, dt, **kw) for dt in (torch.float64, torch.float32))
        for k, r in ref.items():
            scale = max(1.0, float(r.abs().max()))
            tol = max(TOL * scale, 4.0 * float((ref32[k] - r).abs().max()))
            err = float((got[k].cpu().double() - r).abs().max())
            assert err <= tol, (k, D, R, N, err, tol)
    else:
        ref = _oracle(params, o, d, lo, hi, jit, up, torch.float32, bf16=True, **kw)
        for k in ("rgb", "dist", "dloss"):
            err = (got[k].cpu().double() - ref[k]).abs().flatten() / max(1.0, float(ref[k].abs().max()))
            assert float(err.max()) <= 3e-3 and float(err.mean()) <= 3e-4, (k, float(err.max()), float(err.mean()))
        for k, r in ref.items():
            if k in ("rgb", "dist", "dloss"):
                continue
            if float(r.abs().max()) == 0:
                assert float(got[k].abs().max()) == 0, k
                continue
            l2 = float((got[k].cpu().double() - r).norm() / r.norm())
            assert l2 <= (1e-1 if k.startswith("d ") else 3e-2), (k, l2)
    # the term switched off by its upstream gradient, and by its absence
    zero = _hip(params, o, d, lo, hi, jit, (up[0], up[1], torch.zeros(R)), D=D, ray_distortion=(S_NEAR, S_INV), bf16=bf16, **kw)
    none = _hip(params, o, d, lo, hi, jit, (up[0], up[1], None), D=D, ray_distortion=(S_NEAR, S_INV), bf16=bf16, **kw)      # no gradient at all for dloss
    off = _hip(params, o, d, lo, hi, jit, (up[0], up[1], None), D=D, ray_distortion=None, bf16=bf16, **kw)
    assert torch.equal(zero["dloss"], got["dloss"])
    for k, v in off.items():
        assert torch.equal(zero[k], v) and torch.equal(none[k], v), k
    # only dloss has a gradient: d_rgb and d_dist are zero-filled, the result is the difference of the two runs above (to rounding)
    only = _hip_only_dloss(params, o, d, lo, hi, jit, up[2], D=D, bf16=bf16, **kw)
    for k in ("dW fc_density", "dW layers0.0", "d pts_d"):
        want = got[k].double() - off[k].double()
        scale = max(1.0, float(got[k].abs().max()), float(off[k].abs().max()))
        assert float((only[k].double() - want).abs().max()) <= (2e-2 if bf16 else 2e-5) * scale, k


def test_weight_gradient_at_d256_with_few_samples_without_the_term():
    """The defect the D = 256, 7 x 17 operator case ran into, shown on the plain render (ray_distortion=None): with 128 padded samples the weight
    gradient's plan is one class-A and one class-B workgroup, and in the latter a wave with the skip layer's position-encoding tile (36 KiB of
    private LDS staging) runs beside a wave with the merged colour tile (32 KiB); their areas overlapped by 8 KiB until both were laid out with
    one stride (nnr_wgrad.hip), and fc_feature / rgb_layers.0 (at times layers1.0) came out wrong and different from run to run -- max-abs
    errors 0.2 to 1.1 (dW fc_feature, the oracle's largest entry 4.7e-4), 0.6 to 8.6 (dW rgb_layers.0, 2.3e-2), 7 to 99 (db rgb_layers.0,
    1.5e-2) in six runs.  Every gradient against the live oracle at the rule of the test above, and three runs bit for bit."""
    D, R, N = 256, 7, 17
    params, o, d, lo, hi, jit = _synthetic(D, R, N, seed=41 + R)
    gen = torch.Generator().manual_seed(5)
    up = (torch.randn(R, 3, generator=gen) / R, torch.randn(R, generator=gen) / R, None)
    kw = dict(dist_alpha=False, white_bg=False, relu_sigma=False)
    runs = [_hip(params, o, d, lo, hi, jit, up, D=D, ray_distortion=None, **kw) for _ in range(3)]
    ref, ref32 = (_oracle(params, o, d, lo, hi, jit, (up[0], up[1], torch.zeros(R)), dt, **kw) for dt in (torch.float64, torch.float32))
    for k, v in runs[0].items():
        r = ref[k]
        tol = max(TOL * max(1.0, float(r.abs().max())), 4.0 * float((ref32[k] - r).abs().max()))
        err = float((v.cpu().double() - r).abs().max())
        assert err <= tol, (k, err, tol)
        assert torch.equal(runs[1][k], v) and torch.equal(runs[2][k], v), k


def _hip_only_dloss(params, o, d, lo, hi, jit, g, *, D, **kw):
    import nnr
    from nnr import lib as L
    dev = torch.device("cuda")
    w = [params[n + ".weight"].to(dev).requires_grad_(True) for n in L.LAYER_NAMES]
    b = [params[n + ".bias"].to(dev).requires_grad_(True) for n in L.LAYER_NAMES]
    oo, dd, vv = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True), (-d).to(dev).requires_grad_(True)
    out = nnr.render_rays(oo, dd, vv, lo.to(dev), hi.to(dev), jit.to(dev), w, b, hidden=D, ray_distortion=(S_NEAR, S_INV), **kw)
    (out[4] * g.to(dev)).sum().backward()
    got = {"d pts_d": dd.grad}
    for i, n in enumerate(L.LAYER_NAMES):
        got["dW " + n] = w[i].grad
    return got


def test_without_gradients_the_fifth_output_is_none_and_the_rest_is_the_plain_render():
    import nnr
    from nnr import lib as L
    D, R, N = 128, 7, 17
    params, o, d, lo, hi, jit = _synthetic(D, R, N, seed=3)
    dev = torch.device("cuda")
    w = [params[n + ".weight"].to(dev) for n in L.LAYER_NAMES]
    b = [params[n + ".bias"].to(dev) for n in L.LAYER_NAMES]
    a = (o.to(dev), d.to(dev), (-d).to(dev), lo.to(dev), hi.to(dev), jit.to(dev), w, b)
    kw = dict(hidden=D, dist_alpha=False, white_bg=False, relu_sigma=False)
    with torch.no_grad():
        plain = nnr.render_rays(*a, **kw)
        with_rd = nnr.render_rays(*a, ray_distortion=(S_NEAR, S_INV), **kw)
    assert len(plain) == 4 and len(with_rd) == 5 and with_rd[4] is None
    assert all(torch.equal(x, y) for x, y in zip(plain, with_rd[:4]))


def test_shard_additivity_with_the_term_on():
    """The gradients of the full batch are the sum of its two halves' (what data parallelism relies on): 2e-5 of max(1, max |full|), the bar of
    tests/test_gpu_parity.py::_full_size_properties."""
    D, R, N = 128, 10, 33
    params, o, d, lo, hi, jit = _synthetic(D, R, N, seed=9)
    gen = torch.Generator().manual_seed(5)
    up = (torch.randn(R, 3, generator=gen) / R, torch.randn(R, generator=gen) / R, torch.randn(R, generator=gen) / R + 1.0 / R)
    kw = dict(D=D, ray_distortion=(S_NEAR, S_INV), dist_alpha=False, white_bg=False, relu_sigma=False)
    full = _hip(params, o, d, lo, hi, jit, up, **kw)
    h = R // 2
    parts = [_hip(params, o[s], d[s], lo, hi, jit[s], tuple(u[s] for u in up), **kw) for s in (slice(0, h), slice(h, R))]
    for k, f in full.items():
        if k.startswith("dW") or k.startswith("db"):
            assert float((f - (parts[0][k] + parts[1][k])).abs().max()) <= 2e-5 * max(1.0, float(f.abs().max())), k
        else:
            assert torch.allclose(torch.cat([parts[0][k], parts[1][k]]), f, atol=1e-5, rtol=1e-5), k


# ------------------------------------------------------------------------------------------------------------ the trainer
class _Counting:
    """libnnr.so with every nnr_* call counted by name (each is one launch, or host-only): stands in for nnr.lib's loaded library."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("nnr_"):
            return f

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return f(*a)
        return counted


# entry points that launch nothing (sizes, plans, plane offsets: cached per shape by nnr/ops.py, so the first trainer of a process calls more)
HOST_ONLY = {"nnr_abi_version", "nnr_strerror", "nnr_last_hip_error", "nnr_packed_floats", "nnr_workspace_floats", "nnr_plan_bytes",
             "nnr_plan_counts", "nnr_plan_build", "nnr_ws_plane", "nnr_ws_plane_layout", "nnr_aux_workspace_floats",
             "nnr_randperm_scratch_bytes"}


def _three_steps(scene_dir, monkeypatch, weight):
    """Three Trainer.train_step on the small synthetic scene from one seed -> (parameters, calls into libnnr.so by name, loss_dict of the last)."""
    import dataloading as dl
    import train_scene
    from nnr import lib as L
    import numpy as np
    torch.manual_seed(7)
    np.random.seed(7)
    cfg = train_scene.scene_cfg(scene_dir, "toy", n_rays=96, n_samples=24, hidden=128, sample_rate=10 ** 6)
    if weight is not None:
        cfg["training"]["ray_distortion_weight"] = weight
    assert ("ray_distortion_weight" in cfg["training"]) == (weight is not None)
    loader, fields = dl.get_dataloader(cfg, mode="train", shuffle=False)
    trainer, pose, dist = train_scene.build(cfg, torch.device("cuda"), fields["img"].N_imgs)
    counting = _Counting(L.load())
    monkeypatch.setattr(L, "_lib", counting)
    losses = None
    for it, batch in zip(range(3), loader):
        losses = trainer.train_step(batch, it, 0, 10 ** 6, None)
    torch.cuda.synchronize()
    monkeypatch.undo()
    trainer.flush_nan_check()
    params = [p.detach().clone() for net in (trainer.model, pose, dist) for p in net.parameters()]
    for k, v in losses.items():      # the early copy of the logged scalars (model/training.py: _EarlyScalar) answers with the device's value
        if type(v).__name__ == "_EarlyScalar":
            assert v.item() == torch.Tensor.item(v.as_subclass(torch.Tensor)) or v.item() != v.item(), k
    kind = type(losses.get("loss_ray_distortion", losses["loss"])).__name__
    launches = {k: v for k, v in counting.calls.items() if k not in HOST_ONLY}
    return params, launches, {k: (v.item() if torch.is_tensor(v) and v.numel() == 1 else v) for k, v in losses.items()}, kind


def test_trainer_off_is_todays_step_and_on_adds_the_term(tmp_path, monkeypatch):
    import scene_writer
    scene_writer.write_scene(str(tmp_path), scene="toy", frames=4, size=(30, 40), seed=1)
    absent = _three_steps(str(tmp_path), monkeypatch, None)
    zero = _three_steps(str(tmp_path), monkeypatch, 0.0)
    on = _three_steps(str(tmp_path), monkeypatch, 0.01)
    # absent and 0.0: the same bits, the same launches, the same keys
    assert all(torch.equal(a, b) for a, b in zip(absent[0], zero[0]))
    assert absent[1] == zero[1] and sum(absent[1].values()) > 0
    assert not any("ray_distortion" in k for k in absent[1])
    assert list(absent[2]) == list(zero[2]) and "loss_ray_distortion" not in absent[2]
    assert absent[2]["loss"] == zero[2]["loss"]
    # 0.01: one forward and one backward launch more per step, nothing else differs in the launches; the term is reported and acts
    extra = {k: on[1].get(k, 0) - absent[1].get(k, 0) for k in set(on[1]) | set(absent[1])}
    assert {k: v for k, v in extra.items() if v} == {"nnr_ray_distortion_fwd": 3, "nnr_ray_distortion_bwd": 3}
    assert set(on[2]) == set(absent[2]) | {"loss_ray_distortion"}
    assert on[3] == "_EarlyScalar" and absent[3] == "_EarlyScalar"      # the term rides in the step's early copy like the other scalars
    rd = on[2]["loss_ray_distortion"]
    assert rd == rd and 0.0 < rd < float("inf")
    assert any(not torch.equal(a, b) for a, b in zip(on[0], absent[0]))
    assert all(torch.isfinite(p).all() for p in on[0])
