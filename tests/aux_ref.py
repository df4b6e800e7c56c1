"""A plain definition of the per-image losses between a frame and its neighbour (csrc/nnr_aux.hip, nnr_aux_terms_fwd / _bwd of
include/nnr.h), the seeded inputs of the cases that tests/test_gpu_aux_direct.py runs on the kernels, and the rounding noise of the
operation on each of them.  CPU only; every gradient comes from autograd.

Per point i = y wr + x of the (hr, wr) sampling grid, x' = 2x/(wr-1) - 1, y' = 2y/(hr-1) - 1:
  d1 = the nearest-resized d1_img at i (optionally distorted: d s + t, or (d + t) s), raised to nearest_limit where it is below it
       (no gradient there); d2 likewise
  pc1 = Kinv[:3] (x' d1, y' d1, d1, 1), pc2 likewise;  rot = rel[:3] (pc1, 1);  X = rot / scale2, Y = pc2 / scale2
  loss_pc = (sum_s |X_s - Y_nn(s)| + sum_s |Y_s - X_nn(s)|) / S, nn = the nearest point of the other cloud (first index on ties)
  rot' = (nl, nl, nl) where -rot.z < nl;  xy = (K[:3] (rot', 1)).xy / .z;  valid = max|xy| <= 1
  term = clamp(|img1r(x', y') - img2r(xy)|, 0, 1) per channel (bilinear, align_corners, zero padding), with ssim
         0.15 term + 0.85 ssim_dissimilarity over (grid x, colour channel), the way the reference hands its (1, hr, wr, 3) tensors over
  loss_rgb_s = sum over the valid points and 3 channels of term / (3 n_valid)
A shard (lo, hi) restricts the SUMS to the source points [lo, hi): the normalisers S and n_valid stay global, and with ssim a point
outside the shard still receives gradient through the windows of its neighbours inside it."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F


def nearest_indices(hd, wd, hr, wr):
    """Flat index into an (hd, wd) map of the pixel that F.interpolate(mode='nearest') reads for each point of the (hr, wr) grid."""
    src = torch.arange(hd * wd, dtype=torch.float32).view(1, 1, hd, wd)      # (exact in fp32: fewer than 2^24 pixels)
    return F.interpolate(src, (hr, wr), mode="nearest").view(-1).long()


def _rows3(m, p):
    """m (4, 4), p (3, S) -> the first three rows of m [p; 1], (3, S).  Broadcast products and a sum over four terms: no BLAS call whose
    order of operations could depend on the machine."""
    p4 = torch.cat([p, torch.ones_like(p[:1])], 0)
    return (m[:3, :, None] * p4[None]).sum(1)


def _ssim_raw(x, y):
    """(1 - SSIM) / 2 before its clamp, on (1, hr, wr, 3) tensors read as NCHW: 3 x 3 reflect-padded means over (grid x, channel)."""
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    x, y = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    pool = lambda t: F.avg_pool2d(t, 3, 1)
    mu_x, mu_y = pool(x), pool(y)
    sigma_x, sigma_y = pool(x * x) - mu_x * mu_x, pool(y * y) - mu_y * mu_y
    sigma_xy = pool(x * y) - mu_x * mu_y
    n = (2 * mu_x * mu_y + c1) * (2 * sigma_xy + c2)
    d = (mu_x * mu_x + mu_y * mu_y + c1) * (sigma_x + sigma_y + c2)
    return (1 - n / d) / 2


def _fmin(t):
    return float(t.detach().min()) if t.numel() else math.inf


def aux_ref(d1_img, d2_img, rel, scale2, img1r, img2r, K, Kinv, res, nearest_limit, *, rgb_s, pc, scale_pcs, detach_rgbs_scale, ssim,
            shard=(0, 0), aff=None, shift_first=False):
    """d1_img, d2_img (hd, wd); rel, K, Kinv (4, 4); scale2 a scalar tensor; img1r, img2r (3, hr, wr); aff (4,) = (scale1, shift1,
    scale2, shift2) or None.  Computes in the dtype of d1_img.  Returns (loss_pc, loss_rgb_s, n_valid, margins): margins maps the name
    of every decision that fp32 could take the other way to the smallest distance of this evaluation from its threshold (inf where
    the decision does not occur), and "n_*" to the number of points in each branch."""
    dt = d1_img.dtype
    hr, wr = int(res[0]), int(res[1])
    S = hr * wr
    hd, wd = d1_img.shape[-2:]
    lo, hi = (0, S) if tuple(shard) == (0, 0) else (int(shard[0]), int(shard[1]))
    mine = torch.zeros(S, dtype=torch.bool)
    mine[lo:hi] = True
    nl = torch.tensor(nearest_limit, dtype=torch.float32).to(dt)      # the fp32 value the C ABI receives
    zero = torch.zeros((), dtype=dt)
    margins = {}

    src = nearest_indices(hd, wd, hr, wr)
    d1, d2 = d1_img.reshape(-1)[src], d2_img.reshape(-1)[src]
    if aff is not None:
        s1, t1, s2a, t2 = aff.reshape(4).unbind()
        d1 = (d1 + t1) * s1 if shift_first else d1 * s1 + t1
        d2 = (d2 + t2) * s2a if shift_first else d2 * s2a + t2
    margins["depth1"], margins["depth2"] = _fmin((d1 - nl).abs()), _fmin((d2 - nl).abs())
    clamp1, clamp2 = d1 < nl, d2 < nl
    margins["n_clamp1"], margins["n_clamp2"] = int(clamp1.sum()), int(clamp2.sum())
    d1, d2 = torch.where(clamp1, nl, d1), torch.where(clamp2, nl, d2)      # a constant where clamped: no gradient

    ys, xs = torch.meshgrid(torch.arange(hr, dtype=dt), torch.arange(wr, dtype=dt), indexing="ij")
    xp, yp = (2 * xs / (wr - 1) - 1).reshape(-1), (2 * ys / (hr - 1) - 1).reshape(-1)
    lift = lambda d: (Kinv[:3, :, None] * torch.stack([xp * d, yp * d, d, torch.ones_like(d)], 0)[None]).sum(1)
    pc1, pc2 = lift(d1), lift(d2)

    loss_pc = zero
    margins["nn_xy"] = margins["nn_yx"] = math.inf
    if pc:
        s2 = scale2.reshape(()) if scale_pcs else 1.0
        X, Y = _rows3(rel, pc1) / s2, pc2 / s2

        def one_way(a, b):      # sum over this shard's sources of the distance to the nearest point of b, and the nearest/second gap
            with torch.no_grad():
                dm = (a[:, :, None] - b[:, None, :]).pow(2).sum(0).sqrt()
                j = torch.argmin(dm, dim=1)
                two = torch.topk(dm[mine], 2, dim=1, largest=False).values
                gap = _fmin((two[:, 1] - two[:, 0]) / two[:, 0])
            return (torch.linalg.norm(a - b[:, j], dim=0) * mine).sum(), gap

        sxy, margins["nn_xy"] = one_way(X, Y)
        syx, margins["nn_yx"] = one_way(Y, X)
        loss_pc = (sxy + syx) / S

    loss_rgb_s, n_valid = zero, torch.zeros((), dtype=torch.int64)
    for k in ("behind", "mask", "pixel", "absdiff", "ssim"):
        margins[k] = math.inf
    margins["n_behind"] = margins["n_valid"] = margins["n_centre_col0"] = margins["n_centre_last_col"] = margins["n_centre_block_edge"] = 0
    if rgb_s:
        rot = _rows3(rel, pc1.detach() if detach_rgbs_scale else pc1)
        behind = -rot[2] < nl
        margins["behind"], margins["n_behind"] = _fmin((-rot[2] - nl).abs()), int(behind.sum())
        q = _rows3(K, torch.where(behind[None], nl, rot))
        xy = q[:2] / q[2:3]
        reach = xy.abs().max(0).values
        valid = reach <= 1
        n_valid = valid.sum()
        margins["mask"], margins["n_valid"] = _fmin((reach - 1).abs()), int(n_valid)
        sample = lambda img, g: F.grid_sample(img[None], g.t().reshape(1, 1, S, 2), mode="bilinear", padding_mode="zeros",
                                              align_corners=True)[0, :, 0].t()      # (S, 3)
        c1, c2 = sample(img1r, torch.stack([xp, yp], 0)), sample(img2r, xy)
        u = c1 - c2
        term = u.abs().clamp(0, 1)
        centre = valid & mine
        if ssim:
            raw = _ssim_raw(c1.view(1, hr, wr, 3), c2.view(1, hr, wr, 3)).view(S, 3)
            term = 0.15 * term + 0.85 * raw.clamp(0, 1)
            margins["ssim"] = _fmin(torch.minimum(raw.abs(), (raw - 1).abs())[centre])
        if int(n_valid) > 0:
            loss_rgb_s = (term * centre[:, None]).sum() / (3 * n_valid)
        # where the colour of a point matters: at the valid points, with ssim at every point whose bilinear footprint meets the image
        # (it enters its neighbours' windows); there the sampled pixel coordinate must not sit on an integer
        pix = torch.stack([(xy[0] + 1) / 2 * (wr - 1), (xy[1] + 1) / 2 * (hr - 1)], 0).detach()
        touch = (pix[0] > -1.5) & (pix[0] < wr + 0.5) & (pix[1] > -1.5) & (pix[1] < hr + 0.5) if ssim else valid
        margins["pixel"] = _fmin((pix - pix.round()).abs()[:, touch])
        au = u.detach().abs()[valid]
        margins["absdiff"] = _fmin(torch.minimum(au, (au - 1).abs()))
        col = torch.arange(S) % wr
        margins["n_centre_col0"], margins["n_centre_last_col"] = int((centre & (col == 0)).sum()), int((centre & (col == wr - 1)).sum())
        margins["n_centre_block_edge"] = int(centre[255:257].sum())      # the two points at the boundary of the 256-thread blocks
    return loss_pc, loss_rgb_s, n_valid, margins


def decision_margin(margins):
    """The smallest margin of an evaluation (the nearest-neighbour gaps are relative, everything else absolute)."""
    return min(v for k, v in margins.items() if not k.startswith("n_"))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
NL = 0.05                                             # nearest_limit of every case
K_SKEW = [[1.3, 0.07, 0.11, 0.0], [0.0, -2.2, -0.05, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]      # skew and a principal point
AFF = (1.1, -0.02, 0.9, -0.03)                        # (scale1, shift1, scale2, shift2) of the cases that distort in the kernels
SCALE2 = 1.3
G_OUT = (0.7, -1.3)                                   # upstream gradients of (loss_pc, loss_rgb_s)
POSE = ((0.1, 0.05, 1.0), -0.35, (-0.02, 0.04, 0.15))   # axis, angle (rad), translation of the relative transform
POSE_SMALL = ((1.0, 0.5, 0.3), 0.05, (0.05, -0.02, 0.03))
POSE_AWAY = ((0.2, 1.0, 0.1), 0.1, (6.0, 0.0, 0.15))  # every point projects outside [-1, 1]: the translation along x

# via: "abi" = nnr_aux_terms_fwd / _bwd through ctypes, "mats" / "weighted" = nnr.aux.aux_terms(mats=...) / (weights=...).
# rich: the inputs hold a patch of clamped depths in each map and a patch of points behind the second camera (13 x 21 grids only).
# weights = (w_pc, w_rgbs), g_w = dL/d out[3], extra = the coefficients of out[0] and out[1] in the loss next to out[3].
Case = namedtuple("Case", "name maps grid seed pose pc rgb_s scale_pcs detach ssim grad_k aff shift_first shard via rich weights g_w extra")


def _case(name, maps=(52, 84), grid=(13, 21), seed=0, pose=POSE, pc=True, rgb_s=True, scale_pcs=True, detach=False, ssim=False,
          grad_k=False, aff=False, shift_first=False, shard=(0, 0), via="abi", rich=True, weights=None, g_w=0.9, extra=(0.0, 0.0)):
    return Case(name, maps, grid, seed, pose, pc, rgb_s, scale_pcs, detach, ssim, grad_k, aff, shift_first, shard, via, rich, weights, g_w, extra)


_SHAPES = [("maps50x83", (50, 83), (13, 21), True), ("maps13x21", (13, 21), (13, 21), True), ("maps14x22", (14, 22), (13, 21), True),
           ("grid2x3", (5, 7), (2, 3), False), ("grid2x2", (5, 7), (2, 2), False)]
_SHARDS = [("shard_0_100", (0, 100)), ("shard_100_273", (100, 273)), ("shard_37_260", (37, 260))]

CASES = {c.name: c for c in [
    _case("pc_only", rgb_s=False), _case("rgbs_only", pc=False), _case("both"), _case("no_scale_pcs", scale_pcs=False),
    _case("detach", detach=True), _case("ssim", ssim=True), _case("ssim_detach", ssim=True, detach=True), _case("grad_k", grad_k=True),
    _case("affine", aff=True), _case("affine_shift_first", aff=True, shift_first=True), _case("mats", aff=True, via="mats"),
    _case("weighted_only", via="weighted", weights=(0.7, 1.3)), _case("weighted_mixed", via="weighted", weights=(0.7, 1.3), extra=(0.5, 0.25)),
] + [_case(n + s, maps=m, grid=g, ssim=bool(s), rich=r, pose=POSE if r else POSE_SMALL) for n, m, g, r in _SHAPES for s in ("", "_ssim")]
  + [_case(n + s, shard=sh, ssim=bool(s)) for n, sh in _SHARDS for s in ("", "_ssim")]
  + [_case("no_valid", pose=POSE_AWAY)]}
# (maps, grid, pose) -> seed of the inputs: the first one that keeps every decision of every case on these inputs 1e-4 away from its
# threshold (tests/test_aux_ref_cpu.py asserts it).  Cases on the same maps, grid and pose share their inputs: the shards add up.
SEEDS = {((52, 84), (13, 21), POSE): 1, ((50, 83), (13, 21), POSE): 7, ((14, 22), (13, 21), POSE): 1, ((52, 84), (13, 21), POSE_AWAY): 27}      # (0 for the rest)


def _rotation(axis, ang):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    k = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(ang) * k + (1 - math.cos(ang)) * (k @ k)


def case_inputs(case):
    """The fp32 inputs of a case from a seeded CPU generator: dict of d1_img, d2_img (hd, wd), img1r, img2r (3, hr, wr), K, Kinv, rel
    (4, 4), scale2 (), aff (4,) or None.  Depths: a smooth surface plus noise; rich cases overwrite three patches of the pixels the
    grid samples -- below the limit in map 1 (clamped, and behind the second camera), just above it in map 1 (behind only), below it
    in map 2.  Colours reach 1.5, so that some differences exceed the clamp at 1."""
    g = torch.Generator().manual_seed(1000 + SEEDS.get((case.maps, case.grid, case.pose), case.seed))
    (hd, wd), (hr, wr) = case.maps, case.grid
    ys, xs = torch.meshgrid(torch.linspace(0, 1, hd), torch.linspace(0, 1, wd), indexing="ij")
    depth = lambda: 2 + 0.6 * torch.sin(5 * xs + 0.3) * torch.cos(4 * ys) + 0.3 * torch.rand(hd, wd, generator=g)
    d1, d2 = depth(), depth()
    if case.rich:
        src = nearest_indices(hd, wd, hr, wr).view(hr, wr)
        patch = lambda r0, c0: src[r0:r0 + 2, c0:c0 + 7].reshape(-1)
        d1.view(-1)[patch(0, 0)] = 0.01 + 0.03 * torch.rand(14, generator=g)
        d1.view(-1)[patch(5, 0)] = 0.08 + 0.04 * torch.rand(14, generator=g)
        d2.view(-1)[patch(8, 10)] = 0.01 + 0.03 * torch.rand(14, generator=g)
    gy, gx = torch.meshgrid(torch.linspace(0, 1, hr), torch.linspace(0, 1, wr), indexing="ij")
    image = lambda: torch.stack([0.75 + 0.45 * torch.sin(7 * gx + c) * torch.cos(5 * gy - c) for c in range(3)]) \
        + 0.3 * (torch.rand(3, hr, wr, generator=g) - 0.5)
    img1, img2 = image(), image() * 0.8
    K = torch.tensor(K_SKEW, dtype=torch.float64)
    rel = torch.eye(4, dtype=torch.float64)
    rel[:3, :3] = _rotation(case.pose[0], case.pose[1])
    rel[:3, 3] = torch.tensor(case.pose[2], dtype=torch.float64)
    return dict(d1_img=d1, d2_img=d2, img1r=img1, img2r=img2, K=K.float(), Kinv=torch.linalg.inv(K).float(), rel=rel.float(),
                scale2=torch.tensor(SCALE2), aff=torch.tensor(AFF) if case.aff else None)


def upstream(case):
    """(dL/d loss_pc, dL/d loss_rgb_s) of the case's loss, as Python floats."""
    if case.weights is None:
        return G_OUT
    return (case.g_w * case.weights[0] + case.extra[0], case.g_w * case.weights[1] + case.extra[1])


def evaluate(case, dtype=torch.float64, shard=None):
    """The reference on a case in `dtype`: dict of loss_pc, loss_rgb_s, n_valid, margins and the gradients of upstream . losses --
    g_d1, g_d2 (hd, wd; None with aff), g_rel (12,), g_scale2, g_K, g_Kinv (12,), g_aff (4,; None without aff)."""
    inp = {k: (v.to(dtype).requires_grad_(True) if v is not None else None) for k, v in case_inputs(case).items()}
    l_pc, l_rgbs, n_valid, margins = aux_ref(
        inp["d1_img"], inp["d2_img"], inp["rel"], inp["scale2"], inp["img1r"], inp["img2r"], inp["K"], inp["Kinv"], case.grid, NL,
        rgb_s=case.rgb_s, pc=case.pc, scale_pcs=case.scale_pcs, detach_rgbs_scale=case.detach, ssim=case.ssim,
        shard=case.shard if shard is None else shard, aff=inp["aff"], shift_first=case.shift_first)
    g_pc, g_rgbs = upstream(case)
    loss = g_pc * l_pc + g_rgbs * l_rgbs
    if loss.requires_grad:
        loss.backward()
    grad = lambda k: inp[k].grad.detach() if inp[k].grad is not None else torch.zeros_like(inp[k].detach())
    out = dict(loss_pc=l_pc.detach(), loss_rgb_s=l_rgbs.detach(), n_valid=int(n_valid), margins=margins,
               g_rel=grad("rel")[:3].reshape(12), g_scale2=grad("scale2"), g_K=grad("K")[:3].reshape(12), g_Kinv=grad("Kinv")[:3].reshape(12))
    out["g_d1"], out["g_d2"] = (None, None) if case.aff else (grad("d1_img"), grad("d2_img"))
    out["g_aff"] = grad("aff") if case.aff else None
    return out


OUTPUTS = ("loss_pc", "loss_rgb_s", "g_d1", "g_d2", "g_rel", "g_scale2", "g_K", "g_Kinv", "g_aff")


def rounding_noise(case):
    """{output: largest |fp32 - fp64| of the reference on this case, relative to the output's largest fp64 magnitude} (0 where it is 0)."""
    lo, hi = evaluate(case, torch.float32), evaluate(case, torch.float64)
    assert lo["n_valid"] == hi["n_valid"]
    out = {}
    for k in OUTPUTS:
        if hi[k] is None:
            continue
        scale = float(hi[k].abs().max())
        out[k] = float((lo[k].double() - hi[k]).abs().max()) / scale if scale > 0 else 0.0
    return out


FP32_HALF_ULP = 2.0 ** -24


def tolerance(case_name, output):
    """What the kernels may deviate from the fp64 reference, relative to the output's largest magnitude: 8 x the rounding noise of the
    operation itself (they sum in another, fixed order and fuse a few operations), never more than the 1e-4 of scale that
    tests/test_aux_terms.py grants gradients against the golden.  Losses: the same 8 x, never more than 1e-5 absolute (the caller caps).
    The noise counts as at least half an fp32 ulp: no fp32 result can be expected closer to the fp64 value than that, and a measured
    deviation below it (a scalar whose fp32 roundings happened to cancel) says nothing about the operation."""
    return min(8.0 * max(NOISE[case_name][output], FP32_HALF_ULP), 1e-4)


# NOISE[case][output]: rounding_noise() as measured; tests/test_aux_ref_cpu.py re-measures it and fails if an entry is off by more than 2 x.
NOISE = {
    "pc_only": {"loss_pc": 2.4e-08, "loss_rgb_s": 0.0e+00, "g_d1": 7.2e-07, "g_d2": 6.4e-07, "g_rel": 1.1e-07, "g_scale2": 1.2e-07, "g_K": 0.0e+00, "g_Kinv": 3.3e-07},
    "rgbs_only": {"loss_pc": 0.0e+00, "loss_rgb_s": 9.8e-08, "g_d1": 2.8e-06, "g_d2": 0.0e+00, "g_rel": 2.5e-07, "g_scale2": 0.0e+00, "g_K": 3.4e-07, "g_Kinv": 3.7e-07},
    "both": {"loss_pc": 2.4e-08, "loss_rgb_s": 9.8e-08, "g_d1": 7.1e-07, "g_d2": 6.4e-07, "g_rel": 1.6e-07, "g_scale2": 1.2e-07, "g_K": 3.4e-07, "g_Kinv": 6.4e-07},
    "no_scale_pcs": {"loss_pc": 6.7e-08, "loss_rgb_s": 9.8e-08, "g_d1": 8.4e-07, "g_d2": 8.5e-07, "g_rel": 1.8e-07, "g_scale2": 0.0e+00, "g_K": 3.4e-07, "g_Kinv": 6.7e-07},
    "detach": {"loss_pc": 2.4e-08, "loss_rgb_s": 9.8e-08, "g_d1": 7.2e-07, "g_d2": 6.4e-07, "g_rel": 1.6e-07, "g_scale2": 1.2e-07, "g_K": 3.4e-07, "g_Kinv": 3.3e-07},
    "ssim": {"loss_pc": 2.4e-08, "loss_rgb_s": 9.5e-08, "g_d1": 1.5e-06, "g_d2": 6.4e-07, "g_rel": 2.1e-06, "g_scale2": 1.2e-07, "g_K": 3.3e-06, "g_Kinv": 3.1e-06},
    "ssim_detach": {"loss_pc": 2.4e-08, "loss_rgb_s": 9.5e-08, "g_d1": 7.2e-07, "g_d2": 6.4e-07, "g_rel": 2.1e-06, "g_scale2": 1.2e-07, "g_K": 3.3e-06, "g_Kinv": 3.3e-07},
    "grad_k": {"loss_pc": 2.4e-08, "loss_rgb_s": 9.8e-08, "g_d1": 7.1e-07, "g_d2": 6.4e-07, "g_rel": 1.6e-07, "g_scale2": 1.2e-07, "g_K": 3.4e-07, "g_Kinv": 6.4e-07},
    "affine": {"loss_pc": 7.7e-08, "loss_rgb_s": 1.2e-08, "g_rel": 4.2e-07, "g_scale2": 3.7e-07, "g_K": 4.3e-07, "g_Kinv": 4.8e-07, "g_aff": 5.2e-07},
    "affine_shift_first": {"loss_pc": 1.2e-08, "loss_rgb_s": 2.2e-08, "g_rel": 2.4e-07, "g_scale2": 7.1e-07, "g_K": 1.3e-07, "g_Kinv": 2.1e-07, "g_aff": 1.9e-07},
    "mats": {"loss_pc": 7.7e-08, "loss_rgb_s": 1.2e-08, "g_rel": 4.2e-07, "g_scale2": 3.7e-07, "g_K": 4.3e-07, "g_Kinv": 4.8e-07, "g_aff": 5.2e-07},
    "weighted_only": {"loss_pc": 2.4e-08, "loss_rgb_s": 9.8e-08, "g_d1": 7.2e-07, "g_d2": 6.2e-07, "g_rel": 1.9e-07, "g_scale2": 1.5e-08, "g_K": 3.6e-07, "g_Kinv": 3.6e-07},
    "weighted_mixed": {"loss_pc": 2.4e-08, "loss_rgb_s": 9.8e-08, "g_d1": 7.2e-07, "g_d2": 6.2e-07, "g_rel": 1.1e-07, "g_scale2": 5.0e-08, "g_K": 3.9e-07, "g_Kinv": 1.6e-07},
    "maps50x83": {"loss_pc": 1.5e-08, "loss_rgb_s": 1.6e-08, "g_d1": 7.3e-07, "g_d2": 1.3e-06, "g_rel": 4.2e-07, "g_scale2": 8.0e-09, "g_K": 3.3e-07, "g_Kinv": 5.8e-07},
    "maps50x83_ssim": {"loss_pc": 1.5e-08, "loss_rgb_s": 2.0e-07, "g_d1": 7.6e-07, "g_d2": 1.3e-06, "g_rel": 1.1e-06, "g_scale2": 8.0e-09, "g_K": 1.8e-06, "g_Kinv": 1.1e-06},
    "maps13x21": {"loss_pc": 5.9e-08, "loss_rgb_s": 6.2e-08, "g_d1": 2.0e-06, "g_d2": 2.0e-06, "g_rel": 3.4e-07, "g_scale2": 1.0e-07, "g_K": 5.8e-07, "g_Kinv": 9.9e-07},
    "maps13x21_ssim": {"loss_pc": 5.9e-08, "loss_rgb_s": 3.0e-07, "g_d1": 2.0e-06, "g_d2": 2.0e-06, "g_rel": 2.2e-06, "g_scale2": 1.0e-07, "g_K": 2.2e-06, "g_Kinv": 1.5e-06},
    "maps14x22": {"loss_pc": 5.4e-08, "loss_rgb_s": 1.0e-07, "g_d1": 1.6e-06, "g_d2": 1.5e-06, "g_rel": 3.6e-07, "g_scale2": 2.3e-07, "g_K": 4.0e-07, "g_Kinv": 4.9e-07},
    "maps14x22_ssim": {"loss_pc": 5.4e-08, "loss_rgb_s": 2.0e-07, "g_d1": 1.7e-06, "g_d2": 1.5e-06, "g_rel": 9.5e-07, "g_scale2": 2.3e-07, "g_K": 1.5e-06, "g_Kinv": 1.2e-06},
    "grid2x3": {"loss_pc": 2.7e-07, "loss_rgb_s": 9.2e-08, "g_d1": 1.5e-06, "g_d2": 1.3e-06, "g_rel": 1.7e-06, "g_scale2": 9.6e-07, "g_K": 1.5e-07, "g_Kinv": 6.5e-07},
    "grid2x3_ssim": {"loss_pc": 2.7e-07, "loss_rgb_s": 1.4e-06, "g_d1": 1.4e-06, "g_d2": 1.3e-06, "g_rel": 1.3e-06, "g_scale2": 9.6e-07, "g_K": 2.9e-07, "g_Kinv": 2.7e-07},
    "grid2x2": {"loss_pc": 1.6e-07, "loss_rgb_s": 1.6e-07, "g_d1": 4.4e-07, "g_d2": 4.1e-07, "g_rel": 1.9e-06, "g_scale2": 8.6e-07, "g_K": 1.8e-07, "g_Kinv": 3.4e-07},
    "grid2x2_ssim": {"loss_pc": 1.6e-07, "loss_rgb_s": 6.7e-07, "g_d1": 4.4e-07, "g_d2": 4.1e-07, "g_rel": 1.9e-06, "g_scale2": 8.6e-07, "g_K": 1.3e-06, "g_Kinv": 5.4e-07},
    "shard_0_100": {"loss_pc": 1.2e-07, "loss_rgb_s": 1.4e-07, "g_d1": 1.3e-06, "g_d2": 6.4e-07, "g_rel": 1.0e-06, "g_scale2": 2.7e-07, "g_K": 3.0e-07, "g_Kinv": 2.8e-07},
    "shard_0_100_ssim": {"loss_pc": 1.2e-07, "loss_rgb_s": 4.9e-07, "g_d1": 2.8e-06, "g_d2": 6.4e-07, "g_rel": 2.1e-06, "g_scale2": 2.7e-07, "g_K": 1.4e-06, "g_Kinv": 2.3e-06},
    "shard_100_273": {"loss_pc": 3.8e-08, "loss_rgb_s": 2.5e-08, "g_d1": 6.3e-07, "g_d2": 1.4e-06, "g_rel": 3.2e-07, "g_scale2": 2.0e-07, "g_K": 3.3e-07, "g_Kinv": 9.0e-07},
    "shard_100_273_ssim": {"loss_pc": 3.8e-08, "loss_rgb_s": 4.1e-08, "g_d1": 5.7e-07, "g_d2": 1.4e-06, "g_rel": 2.3e-06, "g_scale2": 2.0e-07, "g_K": 2.7e-06, "g_Kinv": 2.2e-06},
    "shard_37_260": {"loss_pc": 9.9e-08, "loss_rgb_s": 3.3e-08, "g_d1": 7.5e-07, "g_d2": 8.1e-07, "g_rel": 2.3e-07, "g_scale2": 4.8e-08, "g_K": 3.9e-07, "g_Kinv": 4.2e-07},
    "shard_37_260_ssim": {"loss_pc": 9.9e-08, "loss_rgb_s": 1.4e-07, "g_d1": 1.7e-06, "g_d2": 8.1e-07, "g_rel": 1.5e-06, "g_scale2": 4.8e-08, "g_K": 3.2e-06, "g_Kinv": 2.4e-06},
    "no_valid": {"loss_pc": 2.6e-08, "loss_rgb_s": 0.0e+00, "g_d1": 1.1e-07, "g_d2": 4.4e-07, "g_rel": 1.3e-07, "g_scale2": 3.5e-08, "g_K": 0.0e+00, "g_Kinv": 4.0e-07},
}
