"""The sparse depth render (include/nnr_depth_sparse.h) restated in torch, in float64, on top of tests/sparse_ref.py
(cells, liveness, the compositing of a masked list), tests/sparse_stop_ref.py (pass boundaries, passes run, the evaluated set) and
tests/fusion_ref.py (alpha of a raw density).  No GPU, no libnnr."""
import torch

import fusion_ref as FR
import sparse_ref as SR
import sparse_stop_ref as ST

F64 = torch.float64


def depth_sparse_ref(alpha, z, live, t_min):
    """alpha (R,C) -- each sample's alpha in the DENSE depth render (the delta to the next sample of the original row) --, z (R,C), live (R,C)
    bool, t_min -> (out (R,2) float64: depth, acc over the evaluated samples; passes (R) int64: P_g of the ray's workgroup; ran (R,C) bool:
    the evaluated samples, the first min(n_r, 32 P_g) live ones).  A culled or unevaluated sample is absent, whatever its alpha."""
    R = alpha.shape[0]
    T, n_live = ST.boundaries(alpha, live)
    passes = ST.passes_ref(T, n_live, t_min, R)
    ran = ST.ran_mask(live, passes)
    a = alpha.detach().cpu().to(F64)
    out = SR.composite_masked(a, torch.zeros(a.shape + (3,), dtype=F64), z, ran)[:, 3:5]
    return out, passes, ran


def from_raw(raw, z, live, t_min, dist_alpha=False, relu_sigma=False):
    """depth_sparse_ref on raw densities: alpha as the compositor makes it (fusion_ref.alpha_ref).  A raw density that was never written (NaN
    at a sample that is not evaluated) does not matter: the sample is absent."""
    return depth_sparse_ref(FR.alpha_ref(raw, z, dist_alpha, relu_sigma), z, live, t_min)
