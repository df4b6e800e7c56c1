"""The sparse frozen-field render (include/nnr_frozen_sparse.h) restated in torch, in float64: the dense compositor on
planes in which a culled sample holds no matter -- its alpha is 0, its transmittance factor (1 - 0) + 1e-6 -- and what it hands back to the
MLP's outputs.  The cell rule, the bit layout and the LIVE rule are those of tests/sparse_ref.py.  No GPU, no libnnr."""
import torch

from sparse_ref import cell_ref, live_ref, pack_bits      # noqa: F401  (the grid's rules exist once)

F64 = torch.float64
EPS_T = 1e-6


def live_rule(live, dist_alpha):
    """the LIVE rule's one addition: under dist_alpha the last sample of every ray is always live"""
    live = live.detach().cpu().bool().clone()
    if dist_alpha:
        live[:, -1] = True
    return live


def alpha_ref(raw, z, dist_alpha, relu_sigma):
    """the compositor's alpha of every sample, float64, differentiable in raw (R,N) float64; z (R,N) fp32: the delta to the next sample is the
    FP32 difference the kernels take, the last one 1e10; under dist_alpha the last alpha is the constant 1"""
    zf = z.detach().cpu().float()
    delta = torch.cat([zf[:, 1:] - zf[:, :-1], torch.full_like(zf[:, :1], 1e10)], 1).to(F64)
    sigma = torch.relu(raw) if relu_sigma else torch.nn.functional.softplus(raw, beta=1, threshold=20)
    if not dist_alpha:
        return 1. - torch.exp(-sigma)
    a = 1. - torch.exp(-sigma * delta)
    return torch.cat([a[:, :-1], torch.ones_like(a[:, -1:])], 1)


def composite(rgb, raw, z, live, dist_alpha=False, relu_sigma=False, white_bg=False):
    """rgb (R,N,3), raw (R,N) float64 (may require grad), z (R,N), live (R,N) bool -> dict rgb (R,3), dist (R), alpha (R,N), w (R,N): the
    dense compositor with the culled samples substituted.  A culled sample's raw and colour are never looked at."""
    m = live.detach().cpu().bool()
    raw_s = torch.where(m, raw, torch.zeros_like(raw))      # (a culled sample's value may be NaN: never computed)
    a = torch.where(m, alpha_ref(raw_s, z, dist_alpha, relu_sigma), torch.zeros_like(raw))
    fac = (1. - a) + EPS_T
    T = torch.cumprod(torch.cat([torch.ones_like(a[:, :1]), fac[:, :-1]], 1), 1)
    w = a * T
    c = torch.where(m[..., None], rgb, torch.zeros_like(rgb))
    acc = w.sum(1)
    out = (w[..., None] * c).sum(1)
    if white_bg:
        out = out + (1. - acc)[:, None]
    return dict(rgb=out, dist=(w * z.detach().cpu().to(F64)).sum(1), alpha=a, w=w)


def render(out4, z, live, dist_alpha=False, relu_sigma=False, white_bg=False):
    """out4 (R,N,4) = (r, g, b, raw) per sample, fp32 as the kernels left it -> composite(...) in float64"""
    o = out4.detach().cpu().to(F64)
    return composite(o[..., :3], o[..., 3], z, live, dist_alpha, relu_sigma, white_bg)


def dout4(out4, z, live, d_rgb, d_dist, dist_alpha=False, relu_sigma=False, white_bg=False):
    """P_DOUT4 of the substituted compositor by autograd in float64: (R,N,4) = d L / d (rgb before the sigmoid, raw) with
    L = sum d_rgb . rgb + sum d_dist . dist; rows of culled samples are zero"""
    o = out4.detach().cpu().to(F64)
    m = live.detach().cpu().bool()
    c = torch.where(m[..., None], o[..., :3], torch.zeros_like(o[..., :3])).requires_grad_(True)
    raw = torch.where(m, o[..., 3], torch.zeros_like(o[..., 3])).requires_grad_(True)
    r = composite(c, raw, z, live, dist_alpha, relu_sigma, white_bg)
    L = (r["rgb"] * d_rgb.detach().cpu().to(F64)).sum() + (r["dist"] * d_dist.detach().cpu().to(F64)).sum()
    gc, graw = torch.autograd.grad(L, [c, raw])
    g = torch.cat([gc * (c * (1. - c)).detach(), graw[..., None]], -1)
    return torch.where(m[..., None], g, torch.zeros_like(g))
