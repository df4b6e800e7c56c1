"""The sparse inference render (include/nnr_sparse.h) restated in torch, in float64: the cell of a point, the bit of a cell,
the compacted list of a ray's live samples and the compositing of a masked sample list.  No GPU, no libnnr."""
import numpy as np
import torch

F64 = torch.float64


def cell_ref(pts, lo, inv_step, dims):
    """pts (..., 3) -> (cell (...) int64: (i_z n_y + i_y) n_x + i_x or -1 outside the grid, near (...) bool: some float64 coordinate
    (p_c - lo_c) inv_step_c of the point lies within 1e-3 cells of an integer -- where fp32 may round to the neighbouring cell, or across the
    grid's border).  inside iff 0 <= f_c < n_c on all three axes; a NaN is outside."""
    p = pts.detach().cpu().to(F64)
    f = (p - torch.tensor([float(v) for v in lo], dtype=F64)) * torch.tensor([float(v) for v in inv_step], dtype=F64)
    n = torch.tensor([int(v) for v in dims], dtype=F64)
    inside = ((f >= 0.) & (f < n)).all(-1)
    i = torch.where(inside[..., None], f, torch.zeros_like(f)).floor().to(torch.int64)
    cell = (i[..., 2] * int(dims[1]) + i[..., 1]) * int(dims[0]) + i[..., 0]
    near = ((f - f.round()).abs() <= 1e-3).any(-1)
    return torch.where(inside, cell, torch.full_like(cell, -1)), near


def bit_ref(bits, cell, dims):
    """the bit of every cell index (-1: False): word (i_z n_y + i_y) w_x + (i_x >> 5), bit i_x & 31 of the uint32 words held as int32"""
    nx = int(dims[0])
    wx = (nx + 31) // 32
    words = bits.detach().cpu().reshape(-1).to(torch.int64) & 0xFFFFFFFF
    c = cell.clamp(min=0)
    row, ix = c // nx, c % nx
    return (((words[row * wx + (ix >> 5)] >> (ix & 31)) & 1) == 1) & (cell >= 0)


def live_ref(bits, cell, dims):
    """a sample is live iff it is outside the grid or its cell's bit is set"""
    return (cell < 0) | bit_ref(bits, cell, dims)


def compact_ref(live_row):
    """the kernel's list of one ray: the live indices in increasing order"""
    return [j for j, v in enumerate(live_row.tolist()) if v]


def pack_bits(occ):
    """occ (n_z, n_y, n_x) bool -> (n_z, n_y, ceil(n_x / 32)) int32: a loop-free restatement for test inputs (numpy)"""
    o = occ.detach().cpu().numpy().astype(bool)
    nz, ny, nx = o.shape
    wx = (nx + 31) // 32
    pad = np.zeros((nz, ny, wx * 32), dtype=np.uint64)
    pad[..., :nx] = o
    w = (pad.reshape(nz, ny, wx, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return torch.from_numpy(w.view(np.int32).copy())


def composite_masked(alpha, rgb, z, live, white_bg=False):
    """Compositing of the live samples alone, float64: alpha (R,C) -- each sample's alpha IN THE DENSE RENDER (its delta is to the next sample
    of the original list) --, rgb (R,C,3), z (R,C), live (R,C) bool -> (R,5): r, g, b, sum w z, sum w.  A culled sample is absent: factor 1,
    weight 0.  T_k = prod over the live i < k of (1 - alpha_i + 1e-6)."""
    a = alpha.detach().cpu().to(F64)
    z = z.detach().cpu().to(F64)
    c = rgb.detach().cpu().to(F64)
    m = live.detach().cpu().bool()
    fac = torch.where(m, (1. - a) + 1e-6, torch.ones_like(a))
    T = torch.cumprod(torch.cat([torch.ones_like(a[:, :1]), fac[:, :-1]], 1), 1)
    w = torch.where(m, a * T, torch.zeros_like(a))
    cm = torch.where(m[..., None], c, torch.zeros_like(c))      # (a culled sample's colour may be NaN: never computed)
    zm = torch.where(m, z, torch.zeros_like(z))
    acc = w.sum(1)
    out_rgb = (w[..., None] * cm).sum(1)
    if white_bg:
        out_rgb = out_rgb + (1. - acc)[:, None]
    return torch.cat([out_rgb, (w * zm).sum(1, keepdim=True), acc[:, None]], 1)


def culling_bound(alpha, live):
    """sum over the culled samples of max(alpha_k, 1e-6), + 1e-6: what |sparse - dense| may reach per ray for rgb (values in [0,1]) and acc;
    times the largest z for sum w z"""
    a = alpha.detach().cpu().to(F64)
    m = live.detach().cpu().bool()
    return torch.where(m, torch.zeros_like(a), a.clamp(min=1e-6)).sum(1) + 1e-6
