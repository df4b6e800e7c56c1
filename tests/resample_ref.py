"""CPU restatement of nnr_resample (include/nnr.h) in torch, written from the definition -- NeRF's sample_pdf with
stratified u, merged with the coarse depths.  dtype selects the arithmetic: torch.float64 is the yardstick of tests/test_gpu_resample.py,
torch.float32 shows what single precision alone costs.  No libnnr.so; runs wherever its inputs live (tools/time_resample.py times it on the device)."""
import torch


def parts(alpha, z, dtype=torch.float64):
    """edges m (R, C-1) and cdf (R, C-1) of the definition."""
    a, zz = alpha.to(dtype), z.to(dtype)
    R = a.shape[0]
    keep = (1 - a) + 1e-6
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=dtype, device=a.device), keep[:, :-1]], dim=1), dim=1)      # T_i = prod_{j<i} (1 - a_j + 1e-6)
    w = a * T
    m = 0.5 * (zz[:, :-1] + zz[:, 1:])
    p = w[:, 1:-1] + 1e-5                                                                             # bins k = 0..C-3: p_k = w_{k+1} + 1e-5
    p = p / p.sum(dim=1, keepdim=True)
    cdf = torch.cat([torch.zeros(R, 1, dtype=dtype, device=a.device), torch.cumsum(p, dim=1)], dim=1)
    return m, cdf


def u_of(xi, R, F, dtype=torch.float64, device=None):
    xi = torch.full((R, F), 0.5, dtype=dtype, device=device) if xi is None else xi.to(dtype)
    return (torch.arange(F, dtype=dtype, device=xi.device).unsqueeze(0) + xi) / F


def resample_ref(alpha, z, xi, n_fine, dtype=torch.float64):
    """alpha, z (R,C), xi (R,F) or None -> z_all (R,C+F), fine (R,F) in `dtype`."""
    R, C = alpha.shape
    F = int(n_fine)
    assert C >= 3 and F >= 1
    zz = z.to(dtype)
    m, cdf = parts(alpha, z, dtype)
    u = u_of(xi, R, F, dtype, alpha.device)
    i = torch.searchsorted(cdf.contiguous(), u.contiguous(), right=True)                              # #{k : cdf_k <= u_j}
    below, above = (i - 1).clamp(min=0), i.clamp(max=C - 2)
    cb, ca = cdf.gather(1, below), cdf.gather(1, above)
    mb, ma = m.gather(1, below), m.gather(1, above)
    den = ca - cb
    den = torch.where(den < 1e-5, torch.ones_like(den), den)
    s = mb + (u - cb) / den * (ma - mb)
    s = torch.minimum(torch.maximum(s, mb), ma)          # inside its bin: a no-op in exact arithmetic, keeps rounded samples in order
    # merge: an element's position = its own index + its rank in the other list; coarse before fine on ties
    pos_c = torch.arange(C, device=s.device).unsqueeze(0) + torch.searchsorted(s.contiguous(), zz.contiguous(), right=False)      # #{fine < z_i}
    pos_f = torch.arange(F, device=s.device).unsqueeze(0) + torch.searchsorted(zz.contiguous(), s.contiguous(), right=True)       # #{coarse <= s_j}
    z_all = torch.empty(R, C + F, dtype=dtype, device=s.device)
    z_all.scatter_(1, pos_c, zz)
    z_all.scatter_(1, pos_f, s)
    bad = (torch.isnan(alpha) | torch.isnan(z)).any(dim=1)
    z_all[bad] = float('nan')
    s = s.clone()
    s[bad] = float('nan')
    return z_all, s


def cdf_distance(alpha, z, samples, u):
    """How far, in CDF space, each sample is from its u: the fp64 piecewise-linear CDF of (alpha, z) evaluated at samples (R,F), compared
    with u (R,F).  Where a sample sits exactly on an edge shared by zero-width bins (tied depths) the CDF jumps there and takes every value
    of the closed interval [cdf at the first such edge, cdf at the last]; the distance is to that interval."""
    d = torch.float64
    m, cdf = parts(alpha, z, d)
    s, u = samples.to(d).contiguous(), u.to(d)
    C1 = m.shape[1]
    n_lt = torch.searchsorted(m.contiguous(), s, right=False)      # edges < s
    n_le = torch.searchsorted(m.contiguous(), s, right=True)       # edges <= s
    k = (n_le - 1).clamp(0, C1 - 2)                                # the bin [m_k, m_{k+1}] a sample strictly inside belongs to
    m0, m1 = m.gather(1, k), m.gather(1, k + 1)
    c0, c1 = cdf.gather(1, k), cdf.gather(1, k + 1)
    width = m1 - m0
    t = torch.where(width > 0, (s - m0) / torch.where(width > 0, width, torch.ones_like(width)), torch.zeros_like(width)).clamp(0, 1)
    inside = c0 + t * (c1 - c0)
    on_edge = n_le > n_lt
    lo = torch.where(on_edge, cdf.gather(1, n_lt.clamp(max=C1 - 1)), inside)
    hi = torch.where(on_edge, cdf.gather(1, (n_le - 1).clamp(0, C1 - 1)), inside)
    return torch.maximum(torch.maximum(lo - u, u - hi), torch.zeros_like(u))


def make_inputs(R, C, seed, near=0.1, far=6.0):
    """Seeded coarse renders for the tests: stratified depths in [near, far] and, by ray index modulo 4: smooth random densities; one peaked
    surface (soft or opaque); an empty ray (all alpha 0 but a last alpha of 1); random densities with runs of exactly tied depths."""
    g = torch.Generator().manual_seed(seed)
    edges = torch.linspace(near, far, C + 1)
    z = edges[:-1] + (edges[1:] - edges[:-1]) * torch.rand(R, C, generator=g)
    alpha = 1 - torch.exp(-torch.rand(R, C, generator=g) * 0.3)
    kind = torch.arange(R) % 4
    centre = torch.randint(1, C - 1, (R, 1), generator=g)
    idx = torch.arange(C).unsqueeze(0)
    peaked = torch.where((idx - centre).abs() <= 1, torch.full((R, C), 0.9), torch.full((R, C), 1e-4))
    # every other peaked ray is an opaque surface in empty space: alphas (0.9, 1, 0.9), exactly 0 elsewhere.  The weights then sum to 1, every
    # other bin holds the bare floor, 1e-5 / (1 + (C - 2) 1e-5) < 1e-5 after normalisation, and the definition's `den` guard fires there
    hard = torch.where((idx - centre).abs() <= 1, torch.full((R, C), 0.9), torch.zeros(R, C))
    hard = torch.where(idx == centre, torch.ones(R, C), hard)
    peaked = torch.where(((torch.arange(R) // 4) % 2 == 0).unsqueeze(1), hard, peaked)
    empty = torch.zeros(R, C)
    empty[:, -1] = 1.0
    alpha = torch.where((kind == 1).unsqueeze(1), peaked, alpha)
    alpha = torch.where((kind == 2).unsqueeze(1), empty, alpha)
    if C >= 8:      # ties: depths [c, c + 3] of those rays take the value of stratum c + 1 (zero-width bins between equal edges); every bin of
        # positive width stays at least half a stratum wide, as in any stratified render -- a sliver bin that holds real mass would turn
        # the half-ulp rounding of an fp32 depth into more than the CDF bound, in the kernel and in any fp32 implementation alike
        start = torch.randint(0, C - 4, (R, 1), generator=g)
        tied = (idx >= start) & (idx <= start + 3) & (kind == 3).unsqueeze(1)
        z = torch.where(tied, z.gather(1, start + 1).expand(R, C), z)
    elif C == 3:
        z = torch.where((kind == 3).unsqueeze(1) & (idx == 1), z[:, :1].expand(R, C), z)
    return alpha.float().contiguous(), z.float().contiguous()
