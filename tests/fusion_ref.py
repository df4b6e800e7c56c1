"""References of the depth-fusion side of the geometry export, plain torch on the CPU:

    tsdf_integrate_ref   tsdf_integrate_kernel (csrc/nnr_tsdf.hip) restated in fp32 operation for operation: explicit multiplies and adds in the
                         kernel's order (never `@`: a matrix product may fuse and reorder), IEEE division, torch.round (half to even)
    fma32                fl32(a b + c) exactly: how hipcc compiles the render kernels' `z = z_lo + (z_hi - z_lo) jitter` and `p = o + d z`
    alpha_ref, composite_ref   the depth kernel's epilogue (csrc/nnr_depth_f16.hip) in float64
    sphere_scene         the analytic scene of the fusion tests: look-at cameras on a Fibonacci sphere around a sphere, exact depth maps
    mesh_topology        edge counts and the Euler characteristic of a quad mesh
"""
import math

import numpy as np
import torch

F32 = torch.float32


def _f(v):
    return torch.tensor(float(np.float32(v)), dtype=F32)


def voxel_points(origin, step, bricks):
    """(B,8,8,8) fp32 x, y, z of every brick voxel, [b][lz][ly][lx]: fl(origin_c + fl(step_c * (float)(8 b_c + l_c))), the index a uint32"""
    b = bricks.detach().cpu().to(torch.int64)
    B = b.shape[0]
    l = torch.arange(8, dtype=torch.int64)
    shapes = ((1, 1, 1, 8), (1, 1, 8, 1), (1, 8, 1, 1))
    out = []
    for c in range(3):
        i = ((8 * b[:, c]).view(B, 1, 1, 1) + l.view(shapes[c])) & 0xffffffff
        prod = _f(step[c]) * i.to(F32)
        out.append((_f(origin[c]) + prod).expand(B, 8, 8, 8).contiguous())
    return out


def tsdf_integrate_ref(origin, step, bricks, cams, depth, trunc, sum, weight, z_min=0.):
    """nnr.ops.tsdf_integrate on CPU tensors, in place: bricks (B,3) integer, cams (n,12) fp32, depth (n,H,W) fp32, sum / weight (B,8,8,8) fp32"""
    assert cams.dtype == F32 and depth.dtype == F32 and sum.dtype == F32 and weight.dtype == F32
    n, H, W = depth.shape
    px, py, pz = voxel_points(origin, step, bricks)
    cw, ch = _f((W - 1) / 2.), _f((H - 1) / 2.)
    trunc, z_min = _f(trunc), _f(z_min)
    one, neg1 = _f(1.), _f(-1.)
    s, w = sum.clone(), weight.clone()
    for c in range(n):
        P = cams[c]
        q = []
        for r in range(3):
            t0, t1, t2 = P[4 * r + 0] * px, P[4 * r + 1] * py, P[4 * r + 2] * pz
            q.append(((t0 + t1) + t2) + P[4 * r + 3])
        qx, qy, qz = q
        ok = qz > z_min
        u, v = qx / qz, qy / qz
        col, row = (u + one) * cw, (v + one) * ch
        cf, rf = torch.round(col), torch.round(row)
        ok = ok & (cf >= 0.) & (cf <= float(W - 1)) & (rf >= 0.) & (rf <= float(H - 1))
        ci = torch.where(ok, cf, torch.zeros_like(cf)).to(torch.int64)
        ri = torch.where(ok, rf, torch.zeros_like(rf)).to(torch.int64)
        d = depth[c][ri, ci]
        ok = ok & (d > 0.)
        sd = qz - d
        ok = ok & (sd <= trunc)
        t = torch.maximum(sd / trunc, neg1)
        s = torch.where(ok, s + t, s)
        w = torch.where(ok, w + one, w)
    sum.copy_(s)
    weight.copy_(w)
    return sum, weight


def fma32(a, b, c):
    """fl32(a * b + c) of fp32 numpy arrays (broadcast), rounded once, exactly.  The product of two fp32 is exact in float64 and the float64
    sum is rounded once; rounding that to fp32 is a second rounding, which differs from the single one only where the float64 sum sits
    exactly halfway between two fp32 values -- those few elements are redone in rational arithmetic."""
    from fractions import Fraction
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    out = s.astype(np.float32)
    tie = ((s.view(np.uint64) & np.uint64(0x1fffffff)) == np.uint64(0x10000000)) & np.isfinite(s)
    for i in zip(*np.nonzero(tie)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(out[i], np.float32(-np.inf)), np.nextafter(out[i], np.float32(np.inf))
        cands = sorted((abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1, float(v)) for v in (lo, out[i], hi))
        out[i] = np.float32(cands[0][2])      # the nearest; of two equally near the one with an even mantissa
    return out


def alpha_ref(raw, z, dist_alpha, relu_sigma):
    """the compositor's alpha (csrc/nnr_device.h: sample_alpha) of fp32 raw densities and depths (R,C), in float64; the deltas are the fp32
    differences the kernel forms, the last one 1e10"""
    raw64 = raw.detach().cpu().to(torch.float64)
    z32 = z.detach().cpu().to(F32)
    sigma = raw64.clamp(min=0.) if relu_sigma else torch.where(raw64 > 20., raw64, torch.log1p(torch.exp(raw64.clamp(max=20.))))
    if not dist_alpha:
        return 1. - torch.exp(-sigma)
    delta = torch.cat([(z32[:, 1:] - z32[:, :-1]).to(torch.float64), torch.full_like(raw64[:, :1], 1e10)], 1)
    alpha = 1. - torch.exp(-sigma * delta)
    alpha[:, -1] = 1.
    return alpha


def composite_ref(alpha, z):
    """(depth, acc) (R,2) float64: T_i = prod_{j<i} (1 - alpha_j + 1e-6), w_i = alpha_i T_i, depth = sum w_i z_i, acc = sum w_i"""
    a = alpha.detach().cpu().to(torch.float64)
    z = z.detach().cpu().to(torch.float64)
    T = torch.cumprod(torch.cat([torch.ones_like(a[:, :1]), (1. - a[:, :-1]) + 1e-6], 1), 1)
    w = a * T
    return torch.stack([(w * z).sum(1), w.sum(1)], 1)


# ---------------------------------------------------------------------------------------------------------------- the analytic scene
K_DIAG = (0.6, -0.6, -1., 1.)


def look_at_world_mats(n, radius):
    """n cameras on a Fibonacci sphere of `radius` looking at the origin along their -z (the project's convention: camera_mat = diag(f, -f, -1, 1))
    -> (n,4,4) float64 world -> camera matrices"""
    mats = []
    golden = math.pi * (3. - math.sqrt(5.))
    for i in range(n):
        zc = 1. - (2 * i + 1) / n
        r = math.sqrt(1. - zc * zc)
        c = radius * np.array([r * math.cos(golden * i), r * math.sin(golden * i), zc])
        back = c / np.linalg.norm(c)
        right = np.cross([0., 0., 1.], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, up, back, c
        mats.append(np.linalg.inv(c2w))
    return torch.from_numpy(np.stack(mats))


def pixel_rays(world_mat, H, W, f=K_DIAG[0]):
    """camera centre (3) and the (H,W,3) world rays of z-depth 1 through arange_pixels' pixel centres, float64 numpy"""
    c2w = np.linalg.inv(np.asarray(world_mat, dtype=np.float64))
    u = 2. * np.arange(W) / max(W - 1, 1) - 1.
    v = 2. * np.arange(H) / max(H - 1, 1) - 1.
    if W == 1:
        u = np.array([-1.])          # arange_pixels divides by W - 1; a 1-pixel axis is used by the tests with hand-made depth maps only
    if H == 1:
        v = np.array([-1.])
    uu, vv = np.meshgrid(u, v)
    d_cam = np.stack([uu / f, -vv / f, -np.ones_like(uu)], -1)      # K = diag(f, -f, -1, 1): q = (f x, -f y, -z), so at z = -1: u = f x, v = -f y
    return c2w[:3, 3], d_cam @ c2w[:3, :3].T


def sphere_depth_maps(world_mats, H, W, sphere_radius):
    """exact z-depth maps of the sphere |p| = sphere_radius, +inf where a ray misses -> (n,H,W) fp32"""
    maps = []
    for m in world_mats.numpy():
        o, d = pixel_rays(m, H, W)
        a = (d * d).sum(-1)
        b = 2. * (d * o).sum(-1)
        c = (o * o).sum() - sphere_radius ** 2
        disc = b * b - 4. * a * c
        t = (-b - np.sqrt(np.maximum(disc, 0.))) / (2. * a)
        maps.append(np.where((disc > 0.) & (t > 0.), t, np.inf))
    return torch.from_numpy(np.stack(maps).astype(np.float32))


def sphere_scene(n_cams=14, cam_radius=3., size=(24, 32), sphere_radius=0.8):
    """(camera_mat (4,4) float64, world_mats (n,4,4) float64, depth (n,H,W) fp32)"""
    K = torch.diag(torch.tensor(K_DIAG, dtype=torch.float64))
    Wm = look_at_world_mats(n_cams, cam_radius)
    return K, Wm, sphere_depth_maps(Wm, size[0], size[1], sphere_radius)


def mesh_topology(vertices, quads):
    """(V, E, F, the smallest and largest number of quads on an edge) of a quad mesh"""
    q = quads.cpu().numpy()
    e = np.concatenate([np.stack([q[:, k], q[:, (k + 1) % 4]], 1) for k in range(4)])
    e.sort(1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return vertices.shape[0], counts.shape[0], q.shape[0], int(counts.min()), int(counts.max())
