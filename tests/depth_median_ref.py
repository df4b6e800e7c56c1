"""The quantile (median) depth of include/nnr_depth_median.h restated in torch, in float64, from (raw, z, flags, level)
and a mask of the evaluated samples, on top of tests/fusion_ref.py (alpha of a raw density); the forward error terms the GPU test bounds the
kernels' fp32 quotient with; and the torch formula of render_depth_maps' fallback branch (geometry.quantile_depth).  No GPU, no libnnr."""
import torch

import fusion_ref as FR

F64 = torch.float64
U = 2. ** -24            # the unit roundoff of fp32
E_FACTOR = 8. * U        # the absolute error of one fp32 factor (1 - alpha) + 1e-6 against float64 (tests/test_gpu_depth_median.py derives it)


def quantile_ref(alpha, z, mask, level):
    """alpha (R,C) -- each sample's alpha in the dense render, NaN allowed --, z (R,C), mask (R,C) bool: the evaluated samples, level ->
    a dict of float64 / int64 tensors on the CPU:
      q      (R)    z_m + (z_next - z_m) (T_m - level) / (T_m - T_{m+1}); +inf without a crossing, NaN where the final product is NaN
      m      (R)    the first evaluated sample with T_{m+1} < level, -1 without one
      T      (R,C+1) T_0 = 1, T_{i+1} = T_i (1 - alpha_i + 1e-6) over the evaluated samples (an absent sample leaves T as it is)
      gap    (R)    z_next - z_m: z_next the depth of sample m + 1 of the ORIGINAL row, z_m behind the last; 0 without a crossing
      T0, T1 (R)    T_m, T_{m+1}; 1 and 1 without a crossing"""
    a = alpha.detach().cpu().to(F64)
    zz = z.detach().cpu().to(F64).expand_as(a)
    mk = mask.detach().cpu().bool()
    R, Cn = a.shape
    fac = torch.where(mk, (1. - a) + 1e-6, torch.ones_like(a))
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=F64), fac], 1), 1)
    crossed = mk & (T[:, 1:] < level)                       # (a NaN never crosses)
    hit = crossed.any(1)
    m = crossed.to(torch.int8).argmax(1, keepdim=True)      # the first True; 0 without one
    z_m = zz.gather(1, m)
    z_n = zz.gather(1, (m + 1).clamp(max=Cn - 1))
    T0, T1 = T.gather(1, m), T.gather(1, m + 1)
    q = (z_m + (z_n - z_m) * ((T0 - level) / (T0 - T1)))[:, 0]
    none = torch.where(torch.isnan(T[:, -1]), torch.full((R,), float("nan"), dtype=F64), torch.full((R,), float("inf"), dtype=F64))
    one = torch.ones(R, dtype=F64)
    return dict(q=torch.where(hit, q, none), m=torch.where(hit, m[:, 0], torch.full((R,), -1, dtype=torch.int64)), T=T,
                gap=torch.where(hit, (z_n - z_m)[:, 0], torch.zeros(R, dtype=F64)), T0=torch.where(hit, T0[:, 0], one),
                T1=torch.where(hit, T1[:, 0], one))


def from_raw(raw, z, mask, level, dist_alpha=False, relu_sigma=False):
    """quantile_ref on raw densities: alpha as the compositor makes it (fusion_ref.alpha_ref).  A raw density that was never written (NaN at a
    sample that is not evaluated) does not matter: the sample is absent."""
    return quantile_ref(FR.alpha_ref(raw, z, dist_alpha, relu_sigma), z, mask, level)


def error_terms(alpha, mask, ref, level):
    """What fp32 may make of the float64 T of quantile_ref (its dict `ref`), first order, per ray:
      E (R,C+1): |T^_k - T_k| <= A_k + (n_k + 8) U T_k, where A_{k+1} = A_k f_k + T_k E_FACTOR collects one absolute error E_FACTOR per
                 evaluated factor f_k and n_k counts the evaluated factors in front of boundary k (one rounding per product, eight to spare
                 for the order of a scan);
      kappa (R): the bound on |r^ - r| of the quotient r = (T_m - level) / (T_m - T_{m+1}) (derivation: tests/test_gpu_depth_median.py);
                 0 without a crossing, inf where the errors reach the denominator;
      near (R) bool: some evaluated boundary lies within its E of level -- fp32 may place the crossing elsewhere."""
    a = alpha.detach().cpu().to(F64)
    mk = mask.detach().cpu().bool()
    R, Cn = a.shape
    T = ref["T"]
    fac = torch.where(mk, (1. - a) + 1e-6, torch.ones_like(a))
    A = torch.zeros(R, Cn + 1, dtype=F64)
    for k in range(Cn):
        A[:, k + 1] = torch.where(mk[:, k], A[:, k] * fac[:, k].abs() + T[:, k].abs() * E_FACTOR, A[:, k])
    n = torch.cat([torch.zeros(R, 1, dtype=F64), mk.to(F64).cumsum(1)], 1)
    E = A + (n + 8.) * U * T.abs()
    near = (mk & ((T[:, 1:] - level).abs() <= E[:, 1:])).any(1)      # (a NaN boundary is never near)
    hit = ref["m"] >= 0
    m = ref["m"].clamp(min=0)[:, None]
    E0, E1 = E.gather(1, m)[:, 0], E.gather(1, m + 1)[:, 0]
    D, N = ref["T0"] - ref["T1"], ref["T0"] - level
    dN, dD = E0 + U * N.abs(), E0 + E1 + U * D.abs()
    left = D - dD
    r = torch.where(hit, N / D, torch.zeros_like(D))
    kappa = torch.where(left > 0, (dN + r.abs() * dD) / left + U * r.abs(), torch.full_like(D, float("inf")))
    return E, torch.where(hit, kappa, torch.zeros_like(D)), near


def torch_quantile(alpha, z, level):
    """render_depth_maps' fallback above 256 samples, the formula of model/geometry.py: quantile_depth, restated here so that the CPU tests
    compare the two: every sample evaluated, the tensors' own dtype"""
    z = z.expand_as(alpha)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), (1. - alpha) + 1e-6], 1), 1)
    crossed = T[:, 1:] < level
    m = crossed.to(torch.int8).argmax(1, keepdim=True)
    z_m, z_n = z.gather(1, m), z.gather(1, (m + 1).clamp(max=z.shape[1] - 1))
    T0, T1 = T.gather(1, m), T.gather(1, m + 1)
    q = (z_m + (z_n - z_m) * ((T0 - level) / (T0 - T1)))[:, 0]
    none = torch.where(torch.isnan(T[:, -1]), torch.full_like(q, float('nan')), torch.full_like(q, float('inf')))
    return torch.where(crossed.any(1), q, none)
