"""The ray distortion of include/nnr_regularise.h in torch, float64 on float64 casts of the fp32 inputs: the reference of
tests/test_ray_distortion_cpu.py and tests/test_gpu_ray_distortion.py.  The loss in its O(N^2) pairwise form with autograd is the definition;
the O(N) prefix form and the closed-form gradient the kernels evaluate are restated beside it and compared with it on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

EPS_T = float(np.float32(1e-6))      # the compositor's transmittance epsilon: the fp32 constant, cast


def alpha_of(raw, z, dist_alpha, relu_sigma):
    """(R,N) alpha in float64 (differentiable in `raw`, which may be an fp32 tensor or a float64 leaf holding fp32 values) -- the compositor's:
    softplus (beta 1, threshold 20) or ReLU density; under dist_alpha 1 - exp(-sigma delta) with delta the FP32 difference of the fp32 depths
    and the last alpha 1, without a gradient; else 1 - exp(-sigma)."""
    assert z.dtype == torch.float32
    raw = raw.double()
    sigma = F.relu(raw) if relu_sigma else F.softplus(raw)
    if not dist_alpha:
        return 1.0 - torch.exp(-sigma)
    R, N = z.shape
    delta = torch.cat([(z[:, 1:] - z[:, :-1]).double(), torch.full((R, 1), 1e10, dtype=torch.float64)], dim=-1)
    alpha = 1.0 - torch.exp(-sigma * delta)
    return torch.cat([alpha[:, :-1], torch.ones(R, 1, dtype=torch.float64)], dim=-1)


def weights_of(alpha):
    """T_j = prod_{i<j} (1 - alpha_i + eps) and w_j = alpha_j T_j."""
    R = alpha.shape[0]
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=alpha.dtype), (1.0 - alpha) + EPS_T], dim=-1), dim=-1)[:, :-1]
    return T, alpha * T


def intervals(z, s_near, s_inv):
    """Centres m and lengths d of the samples' intervals in normalised depth s = (z - s_near) s_inv; the last sample: m = s, d = 0."""
    s = (z.double() - float(np.float32(s_near))) * float(np.float32(s_inv))
    m = torch.cat([0.5 * (s[:, :-1] + s[:, 1:]), s[:, -1:]], dim=-1)
    d = torch.cat([s[:, 1:] - s[:, :-1], torch.zeros_like(s[:, -1:])], dim=-1)
    return m, d


def loss_pairwise(w, m, d):
    """L = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i, per ray: the definition."""
    pair = (w.unsqueeze(2) * w.unsqueeze(1) * (m.unsqueeze(2) - m.unsqueeze(1)).abs()).sum(dim=(1, 2))
    return pair + (w * w * d).sum(dim=1) / 3.0


def _excl(x):
    return torch.cumsum(x, dim=-1) - x


def _excl_rev(x):
    return torch.flip(torch.cumsum(torch.flip(x, [-1]), dim=-1), [-1]) - x


def loss_prefix(w, m, d):
    """The O(N) form: 2 sum_k w_k (m_k W_<k - M_<k) + (1/3) sum_k w_k^2 d_k (m is non-decreasing)."""
    return (2.0 * w * (m * _excl(w) - _excl(w * m))).sum(dim=1) + (w * w * d).sum(dim=1) / 3.0


def loss_from_alpha(alpha, z, s_near, s_inv):
    """The definition on given alphas (any float dtype; evaluated in float64) and fp32 or float64 depths: what the operator tests apply to
    an oracle's alpha and z."""
    _, w = weights_of(alpha.double())
    m, d = intervals(z.detach(), s_near, s_inv)
    return loss_pairwise(w, m, d)


def loss(raw, z, s_near, s_inv, dist_alpha, relu_sigma, form="pairwise"):
    _, w = weights_of(alpha_of(raw, z, dist_alpha, relu_sigma))
    m, d = intervals(z, s_near, s_inv)
    return (loss_pairwise if form == "pairwise" else loss_prefix)(w, m, d)


def loss_and_grad(raw, z, s_near, s_inv, dist_alpha, relu_sigma, g=None):
    """(loss (R,), g_r dL_r/draw (R,N)) in float64: the pairwise form and autograd.  g defaults to ones."""
    leaf = raw.detach().double().requires_grad_(True)
    L = loss(leaf, z, s_near, s_inv, dist_alpha, relu_sigma)
    gd = torch.ones_like(L) if g is None else g.double()
    (grad,) = torch.autograd.grad((L * gd).sum(), leaf)
    return L.detach(), grad


def grad_closed_form(raw, z, s_near, s_inv, dist_alpha, relu_sigma):
    """dL/draw by the formulas the backward kernel evaluates: a_k = 2 [m_k (W_<k - W_>k) - M_<k + M_>k] + (2/3) w_k d_k,
    dL/dalpha_j = T_j a_j - B_j / (1 - alpha_j + eps) with B_j = sum_{m>j} w_m a_m, times dalpha/draw (autograd of alpha_of alone)."""
    leaf = raw.detach().double().requires_grad_(True)
    alpha = alpha_of(leaf, z, dist_alpha, relu_sigma)
    (dadr,) = torch.autograd.grad(alpha.sum(), leaf)      # alpha_j depends on raw_j alone
    alpha = alpha.detach()
    T, w = weights_of(alpha)
    m, d = intervals(z, s_near, s_inv)
    wm = w * m
    a = 2.0 * (m * (_excl(w) - _excl_rev(w)) - _excl(wm) + _excl_rev(wm)) + (2.0 / 3.0) * w * d
    B = _excl_rev(w * a)
    return (T * a - B / ((1.0 - alpha) + EPS_T)) * dadr


def make_inputs(R, N, seed=0):
    """The kernel tests' inputs, fp32 on the CPU: raw = 3 randn - 2 with one raw = 25 (ray 0: beyond the softplus threshold, 1 - alpha + eps
    about 1e-6 behind it) and, with two rays or more, a last ray of all -30 (no mass); z = jittered strata on (0.01, 10), one ray with two
    equal depths where it has three samples or more (a ray of two samples at ONE depth has no spread at all: loss and gradient are
    identically zero, any bar relative to them asks for exact zeros, and the closed form gives 1e-18 there, not 0).  That ray is ray 1
    where there are three rays or more, so that it is neither the ray without mass nor ray 0: in a ray of three samples the raw = 25
    sample behind a zero-length one (alpha 0, no gradient) would leave the ray one gradient of 1e-64 and two of 0, and a bar relative to
    the ray's largest gradient then asks fp32 for a number below its smallest."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * R + N)
    raw = 3.0 * torch.randn(R, N, generator=gen) - 2.0
    raw[0, N // 2] = 25.0
    if R >= 2:
        raw[-1] = -30.0
    edges = torch.linspace(0.01, 10.0, N + 1)
    z = edges[:-1] + (edges[1:] - edges[:-1]) * torch.rand(R, N, generator=gen)
    if N >= 3:
        k, r = (N - 1) // 3, (1 if R >= 3 else 0)
        z[r, k + 1] = z[r, k]
    return raw.contiguous(), z.contiguous()
