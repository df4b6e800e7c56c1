"""The sparse proposal (include/nnr_propose_sparse.h) restated in torch from its definition: the dense proposal's
alphas, masked by the liveness of tests/sparse_ref.py (cell_ref, live_ref), fed to the resampling of tests/resample_ref.py.  No GPU, no
libnnr."""
import torch

import resample_ref as RR
import sparse_ref as SR


def points(pts_o, pts_d, z):
    """p = o + d z of every sample, (R,C,3), formed in fp32 with an unfused multiply and add (torch rounds each elementwise op)."""
    o, d, zz = pts_o.detach().cpu().float(), pts_d.detach().cpu().float(), z.detach().cpu().float()
    return o[:, None, :] + d[:, None, :] * zz[..., None]


def live_of(pts_o, pts_d, z, grid_lo, grid_inv_step, grid_dims, bits):
    """(live (R,C) bool, cell (R,C) int64, near (R,C) bool) of the samples at depths z: cell_ref on p, live_ref on its cells."""
    cell, near = SR.cell_ref(points(pts_o, pts_d, z), grid_lo, grid_inv_step, grid_dims)
    return SR.live_ref(bits, cell, grid_dims), cell, near


def masked_alpha(alpha, live):
    """alpha' of the definition: the dense alpha where the sample is live, exactly 0 where it is culled -- a select, so that a culled
    sample's NaN never reaches the row."""
    return torch.where(live.to(alpha.device), alpha, torch.zeros_like(alpha))


def propose_sparse_ref(alpha, z, live, xi, n_fine, dtype=torch.float64):
    """alpha (R,C): the DENSE proposal's alphas; z (R,C); live (R,C) bool -> (z_all (R,C+F), fine (R,F)) of resample_ref on (alpha', z)."""
    return RR.resample_ref(masked_alpha(alpha, live), z, xi, n_fine, dtype)


def passes_ref(count, n_rays):
    """count (R) live samples per ray -> (R) the passes of 32 the ray's workgroup of four rays runs: the largest ceil(count / 32) of the
    workgroup (a wave past the last ray repeats the last ray, which therefore only counts once)."""
    c = count.detach().cpu().to(torch.int64)
    per = (c + 31) // 32
    out = torch.empty(n_rays, dtype=torch.int64)
    for g0 in range(0, n_rays, 4):
        out[g0:g0 + 4] = per[g0:g0 + 4].max()
    return out
