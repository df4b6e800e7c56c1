"""The stopping rule of the sparse inference render (include/nnr_sparse_stop.h) restated in torch, in float64, on top
of tests/sparse_ref.py: the transmittance of a ray at every pass boundary, the passes a workgroup runs, the samples it evaluates, what
stopping may cost, and a threshold that keeps clear of every boundary value.  No GPU, no libnnr."""
import math

import torch

F64 = torch.float64
CHUNK = 32      # kChunk: samples of one ray per pass
WAVES = 4       # rays per workgroup


def boundaries(alpha, live):
    """alpha (R,C) -- each sample's alpha in the dense render --, live (R,C) bool -> (T (R,B) float64, n_live (R) int64), B = ceil(C / 32):
    T[r, p] = the product of (1 - alpha + 1e-6) over the first min(n_r, 32 (p + 1)) live samples of ray r, the kernel's carry after pass p (past
    the ray's last pass it keeps its final value).  A NaN alpha makes every boundary behind it NaN."""
    a = alpha.detach().cpu().to(F64)
    m = live.detach().cpu().bool()
    R, Cn = a.shape
    B = (Cn + CHUNK - 1) // CHUNK
    fac = torch.where(m, (1. - a) + 1e-6, torch.ones_like(a))
    rank = m.to(torch.int64).cumsum(1) - 1          # a live sample's place in its ray's list
    n_live = m.sum(1)
    T = torch.ones(R, B, dtype=F64)
    for p in range(B):
        part = torch.where(m & (rank < CHUNK * (p + 1)), fac, torch.ones_like(fac))
        T[:, p] = part.prod(1)
    return T, n_live


def passes_ref(T, n_live, t_min, R):
    """P_g of every ray's workgroup, (R) int64: workgroup g holds rays 4g .. 4g + 3, a wave past the last ray repeats ray R - 1; wave r is done
    after pass p iff 32 (p + 1) >= n_r or T[r, p] < t_min (a NaN is never below); P_g is the smallest p + 1 with all four done, 0 where no ray
    of g has a live sample."""
    T = T.detach().cpu().to(F64)
    n = [int(v) for v in n_live.tolist()]
    out = torch.zeros(R, dtype=torch.int64)
    for g in range((R + WAVES - 1) // WAVES):
        rays = [min(WAVES * g + w, R - 1) for w in range(WAVES)]
        n_pass = max((n[r] + CHUNK - 1) // CHUNK for r in rays)
        P = 0
        for p in range(n_pass):
            P = p + 1
            if all(CHUNK * (p + 1) >= n[r] or bool(T[r, p] < t_min) for r in rays):
                break
        out[WAVES * g:min(WAVES * g + WAVES, R)] = P
    return out


def ran_mask(live, passes):
    """the evaluated samples, (R,C) bool: the first min(n_r, 32 P_g) of every ray's live samples"""
    m = live.detach().cpu().bool()
    rank = m.to(torch.int64).cumsum(1) - 1
    return m & (rank < CHUNK * passes.detach().cpu().to(torch.int64)[:, None])


def stop_bound(T_stop, C):
    """what a ray may lose that stopped with the transmittance T_stop: the dropped weights alpha_k T_k = T_k - T_{k+1} + 1e-6 T_k telescope to
    at most T_stop + 1e-6 C max T_k, and no T_k behind the stop exceeds T_stop (1 + 1e-6)^C"""
    return T_stop * (1. + C * 1e-6 * (1. + 1e-6) ** C)


def pick_t_min(T, around):
    """(t_min, margin): among 64 geometrically spaced candidates in [around / 2, 2 around] the one that maximises margin = min |ln(T / t)| over
    all finite non-zero boundary values (inf where there is none).  The caller asserts margin >= 1e-3."""
    v = T.detach().cpu().to(F64).reshape(-1)
    v = v[torch.isfinite(v) & (v != 0.)]
    lv = v.abs().log()
    best, best_margin = None, -1.
    for i in range(64):
        t = float(torch.tensor((around / 2.) * 4. ** (i / 63.), dtype=torch.float32))      # what the entry point is given: an fp32
        margin = float((lv - math.log(t)).abs().min()) if lv.numel() else float("inf")
        if margin > best_margin:
            best, best_margin = t, margin
    return best, best_margin
