"""Exact references and seeded inputs for the exhaustive nearest-neighbour search (csrc/nnr_pointcloud.hip).  CPU only.

On clouds whose coordinates are integers, every step of the kernel's arithmetic is exact in fp32 as long as the squared distance stays
below 2^24: the differences, their squares and the chain fma(dz,dz, fma(dy,dy, dx*dx)) are integers that fp32 represents, and the square
root of a representable value has ONE correctly rounded fp32 value.  lattice_nearest is therefore plain integer arithmetic -- no fma is
emulated, nothing depends on how a CPU vectorises a norm, and ties are decided exactly.  Scaling every coordinate by 2^e keeps the indices
and multiplies the distances by 2^e, exactly (while d2 * 4^e stays representable): the same reference serves tiny and huge clouds."""
import numpy as np
import torch

NO_MATCH = 0xFFFFFFFF      # the decoded index of a source that no destination matched (NaN / infinite coordinates)


def rounded_sqrt(n):
    """n: int64 tensor of integers below 2^24 -> (r, top): r = the correctly rounded fp32 square root of n, top = the largest integer
    whose rounded root is r.  The rounding is VERIFIED, not trusted: a library's vectorised sqrt need not be correctly rounded (torch's
    CPU sqrt is not, on large tensors), so r must satisfy lo^2 <= n < hi^2 for the midpoints lo, hi between r and its fp32 neighbours --
    exact in float64: a midpoint has 25 significant bits, its square 50.  (hi^2 is never an integer: an integer's root is an integer or
    irrational, and a midpoint below 2^12 is no integer.)"""
    n = torch.as_tensor(n)
    assert n.dtype == torch.int64 and int(n.min()) >= 0 and int(n.max()) < 2 ** 24
    r = np.sqrt(n.numpy().astype(np.float64)).astype(np.float32)
    lo = (r.astype(np.float64) + np.nextafter(r, np.float32(0)).astype(np.float64)) / 2
    hi = (r.astype(np.float64) + np.nextafter(r, np.float32(np.inf)).astype(np.float64)) / 2
    nf = n.numpy().astype(np.float64)
    assert bool(np.all(lo * lo <= nf)) and bool(np.all(nf < hi * hi)), "sqrt is not correctly rounded here"
    return torch.from_numpy(r), torch.from_numpy(np.floor(hi * hi).astype(np.int64))


def lattice_nearest(xi, yi, chunk=None):
    """xi (S,3), yi (D,3) int64 -> (idx int64 (S,), dist float32 (S,)): the lexicographic minimum of (fp32 sqrt(d2), index).
    The rounded root is monotone in d2: the minimum root is the root of the minimum d2, and the destinations that share it are those
    with d2 <= top (rounded_sqrt) -- integer compares on the distance matrix, one verified square root per source.
    chunk: sources per block of the distance matrix (default: blocks of ~4 M pairs)."""
    xi, yi = torch.as_tensor(xi), torch.as_tensor(yi)
    assert xi.dtype == torch.int64 and yi.dtype == torch.int64 and xi.shape[1:] == (3,) and yi.shape[1:] == (3,)
    D = yi.shape[0]
    chunk = chunk or max(1, min(1024, (1 << 22) // D))
    ar = torch.arange(D, dtype=torch.int64)
    idx, dist = [], []
    for sec in torch.split(xi, chunk):
        d2 = torch.zeros(sec.shape[0], D, dtype=torch.int64)
        for c in range(3):
            d = sec[:, c, None] - yi[None, :, c]
            d2 += d * d
        assert int(d2.max()) < 2 ** 24, "d2 must stay exact in fp32"
        best, top = rounded_sqrt(d2.min(dim=1).values)
        idx.append(torch.where(d2 <= top[:, None], ar[None, :], D).min(dim=1).values)      # first index among equal rounded roots
        dist.append(best)
    return torch.cat(idx), torch.cat(dist)


def lattice_d2(xi, yi, idx):
    """Integer squared distance of every source to the destination idx names."""
    d = torch.as_tensor(xi) - torch.as_tensor(yi)[idx]
    return (d * d).sum(dim=1)


def min_d2(xi, yi, chunk=256):
    """Per source: the minimum integer d2 and how many destinations attain it."""
    xi, yi = torch.as_tensor(xi), torch.as_tensor(yi)
    lo, cnt = [], []
    for sec in torch.split(xi, chunk):
        d = sec[:, None, :] - yi[None, :, :]
        d2 = (d * d).sum(dim=2)
        m = d2.min(dim=1).values
        lo.append(m)
        cnt.append((d2 == m[:, None]).sum(dim=1))
    return torch.cat(lo), torch.cat(cnt)


def error_grads_fp64(src, dst, idx, g):
    """Gradients of g * mean_s ||src_s - dst_idx(s)|| for the given match, in float64; rows with a zero distance are zero.
    -> g_src (S,3), g_dst (D,3), m (D,) matched sources per destination, sum_abs (D,3) = sum over those sources of |term|."""
    src, dst = torch.as_tensor(src).double(), torch.as_tensor(dst).double()
    idx = torch.as_tensor(idx).long()
    S, D = src.shape[0], dst.shape[0]
    diff = src - dst[idx]
    dist = diff.norm(dim=1, keepdim=True)
    term = torch.where(dist > 0, float(g) / S * diff / dist.clamp_min(1e-300), torch.zeros_like(diff))
    g_dst = torch.zeros(D, 3, dtype=torch.float64).index_add_(0, idx, -term)
    sum_abs = torch.zeros(D, 3, dtype=torch.float64).index_add_(0, idx, term.abs())
    m = torch.bincount(idx, minlength=D)
    return term, g_dst, m, sum_abs


# ---- inputs: every one from a seed ----

def lattice_cloud(n, hi, seed):
    """n points with integer coordinates in [0, hi).  hi = 6: 216 cells, ties everywhere; hi = 512: sparse, ties rare."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, hi, (n, 3), generator=g, dtype=torch.int64)


def lattice_pair(S, D, hi, seed=0):
    return lattice_cloud(S, hi, 1000 * seed + 17 * hi + 1), lattice_cloud(D, hi, 1000 * seed + 17 * hi + 2)


def collision_plane(X, seed=1):
    """Sources: the 1024 cells (0, y, z), y, z < 32.  Destinations: (X, y, z) for a shuffled half of the cells.  d2 = X^2 + dy^2 + dz^2
    near X^2 (7.8 M at X = 2800), where consecutive integers share one rounded fp32 square root: the (sqrt, index) winner is often NOT a
    destination of minimum d2."""
    yz = torch.stack(torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij"), dim=-1).reshape(-1, 2)
    src = torch.cat([torch.zeros(1024, 1, dtype=torch.int64), yz], dim=1)
    g = torch.Generator().manual_seed(seed)
    half = torch.randperm(1024, generator=g)[:512]
    dst = src[half].clone()
    dst[:, 0] = X
    return src, dst


def triplicated_pair(S, n_unique, hi, seed=0):
    """Destinations: n_unique lattice points, each three times at scattered indices.  Sources: the first half coincide with destinations."""
    base = lattice_cloud(n_unique, hi, 1000 * seed + 31)
    g = torch.Generator().manual_seed(1000 * seed + 32)
    dst = base.repeat(3, 1)[torch.randperm(3 * n_unique, generator=g)]
    src = lattice_cloud(S, hi, 1000 * seed + 33)
    pick = torch.randint(0, n_unique, (S // 2,), generator=g)
    src[: S // 2] = base[pick]
    return src, dst


def float_pair(S, D, seed=0):
    """Two noisy samplings of one surface in general position (no ties): the trainer's kind of clouds."""
    g = torch.Generator().manual_seed(seed)
    n = max(S, D)
    surf = torch.rand(n, 3, generator=g) * torch.tensor([6.0, 4.0, 2.0])
    x = surf[:S] + 0.01 * torch.randn(S, 3, generator=g)
    y = surf[torch.randperm(n, generator=g)[:D]] + 0.01 * torch.randn(D, 3, generator=g)
    return x.contiguous(), y.contiguous()


def scaled(pts, e):
    """Integer lattice points times 2^e as float32 (exact)."""
    out = (torch.as_tensor(pts).double() * 2.0 ** e).float()
    assert torch.equal(out.double() * 2.0 ** -e, torch.as_tensor(pts).double())
    return out.contiguous()
