"""GPU (-m gpu): the depth-fusion kernel (nnr_tsdf.hip through nnr_tsdf_integrate / nnr.ops.tsdf_integrate) and the TSDF mesh on top of it
(model/geometry.py: extract_mesh_tsdf).  `sum` and `weight` against tests/fusion_ref.py's fp32 restatement BIT FOR BIT,
with guard bands of sentinel NaNs around both accumulators, on the analytic sphere of tests/test_fusion_cpu.py and on cases built for the
kernel's branches: a camera inside the grid, unobserved and free-space pixels, 1 x 1 and 5 x 7 images, a voxel on the last pixel column,
negative and anisotropic steps, repeated, unsorted and out-of-grid bricks, accumulators that start non-zero, cameras in chunks.  Then
render_depth_maps on either side of the depth kernel's sample limit, and end to end on the fitted D = 128 fixture: depth kernel -> fusion ->
refined mesh."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fusion_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(ROOT, "tests", "golden")
LAYERS = ("layers0.0", "layers0.2", "layers0.4", "layers0.6", "layers1.0", "layers1.2", "layers1.4", "layers1.6", "fc_density",
          "fc_feature", "rgb_layers.0", "fc_rgb")
GUARD = 512
SENTINEL = 0x7fc0beef
NAN, INF = float("nan"), float("inf")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _integrate_guarded(origin, step, bricks, cams, depth, trunc, start=None, z_min=0.):
    """nnr_tsdf_integrate through the C ABI, both accumulators in the middle of sentinel-filled buffers -> (sum, weight) (B,8,8,8) on the CPU"""
    from nnr import lib as L
    B = bricks.shape[0]
    V = 512 * B
    bufs = []
    for k in range(2):
        buf = torch.full((V + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        buf[GUARD:GUARD + V] = _bits(start[k].to(DEV)).view(-1) if start is not None else 0
        bufs.append(buf)
    n, H, W = depth.shape
    o3, s3 = (C.c_float * 3)(*origin), (C.c_float * 3)(*step)
    br, cm, dp = bricks.to(DEV).contiguous(), cams.to(DEV).contiguous(), depth.to(DEV).contiguous()
    L.check(L.load().nnr_tsdf_integrate(o3, s3, L.ptr(br), B, L.ptr(cm), n, L.ptr(dp), H, W, float(trunc), float(z_min),
                                        C.c_void_p(bufs[0].data_ptr() + 4 * GUARD), C.c_void_p(bufs[1].data_ptr() + 4 * GUARD), L.stream()),
            "nnr_tsdf_integrate")
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool((torch.cat([buf[:GUARD], buf[GUARD + V:]]) == SENTINEL).all()), "the kernel wrote outside an accumulator"
    return tuple(buf[GUARD:GUARD + V].view(torch.float32).view(B, 8, 8, 8).cpu() for buf in bufs)


def _against_ref(origin, step, bricks, cams, depth, trunc, start=None, z_min=0., what=""):
    B = bricks.shape[0]
    got = _integrate_guarded(origin, step, bricks, cams, depth, trunc, start, z_min)
    want = [t.clone() for t in start] if start is not None else [torch.zeros(B, 8, 8, 8), torch.zeros(B, 8, 8, 8)]
    R.tsdf_integrate_ref(origin, step, bricks.cpu(), cams.cpu(), depth.cpu(), trunc, want[0], want[1], z_min)
    for name, g, w in zip(("sum", "weight"), got, want):
        diff = _bits(g) != _bits(w)
        assert not bool(diff.any()), "%s %s: %d of %d voxels differ, worst |difference| %.3e" % (
            what, name, int(diff.sum()), g.numel(), float((g - w).abs().nan_to_num().max()))
    return got


def _all_bricks(dims):
    from model import geometry as G
    return G._all_bricks(dims, 'cpu')


def _f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------------------ the analytic sphere
SIZE, LO, HI, RADIUS = (24, 32), (-1.2,) * 3, (1.2,) * 3, 0.8


@functools.lru_cache(maxsize=None)
def _sphere():
    from model import geometry as G
    K, Wm, depth = R.sphere_scene(n_cams=14, cam_radius=3., size=SIZE, sphere_radius=RADIUS)
    origin, step, dims = G.grid_of(LO, HI, 17)
    return origin, step, dims, G.projection_rows(K, Wm), depth, K, Wm


def test_the_sphere_case_equals_the_reference_bit_for_bit():
    origin, step, dims, cams, depth, _, _ = _sphere()
    s, w = _against_ref(origin, step, _all_bricks(dims), cams, depth, 3 * step[0], what="sphere")
    assert float(w.max()) >= 3. and bool((w == 0).any()) and bool((s > 0).any()) and bool((s < 0).any())


def test_cameras_in_chunks_equal_one_call_bit_for_bit():
    origin, step, dims, cams, depth, _, _ = _sphere()
    bricks = _all_bricks(dims)
    trunc = 3 * step[0]
    start = torch.randn(2, bricks.shape[0], 8, 8, 8, generator=torch.Generator().manual_seed(3))
    one = _against_ref(origin, step, bricks, cams, depth, trunc, start, what="one call")
    first = _integrate_guarded(origin, step, bricks, cams[:3], depth[:3], trunc, start)
    two = _integrate_guarded(origin, step, bricks, cams[3:], depth[3:], trunc, first)
    assert not torch.equal(_bits(first[1]), _bits(one[1]))
    assert torch.equal(_bits(one[0]), _bits(two[0])) and torch.equal(_bits(one[1]), _bits(two[1]))


def test_ops_tsdf_integrate_is_the_entry_point_and_checks_its_tensors():
    from nnr import ops
    origin, step, dims, cams, depth, _, _ = _sphere()
    bricks = _all_bricks(dims).to(DEV)
    trunc = 3 * step[0]
    want = _integrate_guarded(origin, step, bricks, cams, depth, trunc)
    acc = torch.zeros(2, bricks.shape[0], 8, 8, 8, device=DEV)
    cm, dp = cams.to(DEV), depth.to(DEV)
    s, w = ops.tsdf_integrate(origin, step, bricks, cm, dp, trunc, acc[0], acc[1])
    assert s.data_ptr() == acc[0].data_ptr() and w.data_ptr() == acc[1].data_ptr()
    assert torch.equal(_bits(acc[0].cpu()), _bits(want[0])) and torch.equal(_bits(acc[1].cpu()), _bits(want[1]))
    for bad in (dict(bricks=bricks.to(torch.int64)), dict(bricks=bricks[:0]), dict(bricks=bricks.cpu()), dict(bricks=bricks[:, :2]),
                dict(cams=cm[:, :11]), dict(cams=cm[:3]), dict(depth=dp[0]), dict(depth=dp.double()), dict(sum=acc[0][:5]),
                dict(weight=acc[1].cpu())):
        a = dict(bricks=bricks, cams=cm, depth=dp, sum=acc[0], weight=acc[1])
        a.update(bad)
        with pytest.raises(ValueError):
            ops.tsdf_integrate(origin, step, a["bricks"], a["cams"], a["depth"], trunc, a["sum"], a["weight"])


# ------------------------------------------------------------------------------------------------------------ the kernel's branches
def _wild_cams(n, seed, inside=True):
    """look-at cameras at random places around (and, the first, inside) the grid, each with focal lengths of its own"""
    g = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        c = g.uniform(-0.4, 0.4, 3) if (inside and i == 0) else g.normal(size=3)
        if not (inside and i == 0):
            c = c / np.linalg.norm(c) * g.uniform(1.5, 3.)
        target = g.uniform(-0.3, 0.3, 3)
        back = (c - target) / np.linalg.norm(c - target)
        right = np.cross([0.1, 0.2, 1.], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, up, back, c
        K = np.diag([g.uniform(0.5, 1.5), -g.uniform(0.5, 1.5), -1., 1.])
        rows.append((K @ np.linalg.inv(c2w))[:3].reshape(12))
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def _wild_depth(n, H, W, seed):
    """depths between 0.2 and 3.5 with unobserved (NaN, 0, negative) and free-space (+inf) pixels among them"""
    g = torch.Generator().manual_seed(seed)
    d = 0.2 + 3.3 * torch.rand(n, H, W, generator=g)
    kind = torch.randint(0, 12, (n, H, W), generator=g)
    for k, v in ((0, NAN), (1, 0.), (2, -0.7), (3, INF), (4, -0.)):
        d[kind == k] = v
    return d


WILD = {
    # name: (origin, step, dims, image, cameras, z_min)
    "camera-inside-5x7": ((-1., -1., -1.), (2. / 23, 2. / 23, 2. / 23), (24, 24, 24), (5, 7), 5, 0.),
    "negative-anisotropic-steps": ((1., -0.9, 0.8), (-0.077, 0.11, -2. / 31), (24, 16, 32), (5, 7), 4, 0.05),
    "image-1x1": ((-1., -1., -1.), (0.125, 0.125, 0.125), (16, 16, 16), (1, 1), 3, 0.),
    "image-1x9": ((-1., -1., -1.), (0.125, 0.125, 0.125), (16, 16, 16), (1, 9), 3, 0.),
}


@pytest.mark.parametrize("case", list(WILD))
def test_the_kernels_branches_equal_the_reference_bit_for_bit(case):
    origin, step, dims, (H, W), n, z_min = WILD[case]
    origin, step = [_f32(v) for v in origin], [_f32(v) for v in step]
    cams = _wild_cams(n, 11)
    depth = _wild_depth(n, H, W, 12)
    bricks = _all_bricks(dims)
    trunc = 3 * max(abs(v) for v in step)
    s, w = _against_ref(origin, step, bricks, cams, depth, trunc, z_min=z_min, what=case)
    assert bool((w > 0).any()) and bool((w == 0).any())
    if case == "camera-inside-5x7":
        # voxels behind the first camera and at q_z near 0 exist and are skipped by it alone
        px, py, pz = R.voxel_points(origin, step, bricks)
        P = cams[0]
        qz = ((P[8] * px + P[9] * py) + P[10] * pz) + P[11]
        assert bool((qz < 0).any()) and bool((qz.abs() < 0.05).any()) and bool((qz > 0.5).any())
        only = _against_ref(origin, step, bricks, cams[:1], depth[:1], trunc, what=case + " first camera")
        assert not bool((only[1][qz <= 0] != 0).any()) and bool((only[1] > 0).any())


def test_repeated_unsorted_and_out_of_grid_bricks_on_non_zero_accumulators():
    origin, step, dims = [_f32(v) for v in (-1., -1., -1.)], [_f32(2. / 19)] * 3, (20, 20, 20)       # 3 bricks per axis, the last reaching past
    cams, depth = _wild_cams(5, 21), _wild_depth(5, 5, 7, 22)
    bricks = _all_bricks(dims)
    perm = torch.randperm(bricks.shape[0], generator=torch.Generator().manual_seed(4))
    bricks = torch.cat([bricks[perm], bricks[perm[3:5]], torch.tensor([[5, 0, 1], [0, 40, 0], [3, 3, 3]], dtype=torch.int32)])
    assert bricks.shape[0] == 32 and torch.unique(bricks, dim=0).shape[0] == 30
    start = torch.randn(2, 32, 8, 8, 8, generator=torch.Generator().manual_seed(5))
    start[1].abs_()
    s, w = _against_ref(origin, step, bricks, cams, depth, 3 * step[0], start, what="bricks")
    assert not torch.equal(_bits(w), _bits(start[1]))
    # a repeated brick is integrated in both of its places, each from its own accumulators
    a, b = 3, 27
    assert torch.equal(bricks[a], bricks[b])
    assert torch.equal(w[a] - start[1][a] > 0, w[b] - start[1][b] > 0)


def test_a_voxel_on_the_last_pixel_column_is_gathered_and_one_past_it_is_not():
    """camera at the origin looking down -z with K = diag(1, -1, -1, 1): u = x / -z.  The dyadic grid holds the voxel (1, y, -1): u = 1 exactly,
    col = (1 + 1) (W - 1) / 2 = W - 1.  Only the last column of the depth map is observed."""
    H, W = 5, 8
    origin, step = (-1., -1., -2.), (0.25, 0.25, 0.25)
    bricks = torch.tensor([[1, 0, 0], [0, 0, 0]], dtype=torch.int32)
    cams = torch.tensor([[1., 0, 0, 0, 0, -1., 0, 0, 0, 0, -1., 0]])
    depth = torch.full((1, H, W), NAN)
    depth[0, :, W - 1] = 1.
    s, w = _against_ref(origin, step, bricks, cams, depth, 0.75, what="last column")
    # brick (1,0,0): ix = 8 + lx; x = 1 at lx = 0; z = -1 at lz = 4; y = 0 at ly = 4 (row = (0 + 1) 2 = 2)
    assert w[0, 4, 4, 0] == 1. and s[0, 4, 4, 0] == 0.
    # x = 1.25 at the same depth: u = 1.25, col = 7.875 -> 8 > W - 1: outside; x = 0.75: col = 6.125 -> 6, unobserved
    assert w[0, 4, 4, 1] == 0. and w[1, 4, 4, 7] == 0.
    assert float(w.sum()) > 1.


# ------------------------------------------------------------------------------------------------------------ end to end on the fitted fixture
def _cfg(hidden, num_points=128):
    return {'model': {'hidden_dim': hidden, 'pos_enc_levels': 10, 'dir_enc_levels': 4, 'occ_activation': 'softplus'},
            'rendering': {'type': 'nope_nerf', 'n_max_network_queries': 64000, 'white_background': False, 'radius': 4.0,
                          'num_points': num_points, 'depth_range': [0.1, 7], 'dist_alpha': False, 'use_ray_dir': True,
                          'normalise_ray': True, 'normal_loss': False, 'sample_option': 'uniform', 'outside_steps': 0},
            'depth': {'type': 'None'}, 'distortion': {'fix_scaleN': True}}


@functools.lru_cache(maxsize=None)
def _fitted_renderer(hidden, num_points=128):
    import model as mdl
    gold = np.load(os.path.join(GOLDEN, "phong_d%d.npz" % hidden))
    cfg = _cfg(hidden, num_points)
    net = mdl.OfficialStaticNerf(cfg)
    sd = {}
    for n in LAYERS:
        q, e = torch.from_numpy(gold[n + ".q"].astype(np.float32)), torch.from_numpy(gold[n + ".e"].astype(np.float32))
        sd[n + ".weight"] = q * torch.exp2(e)[:, None]
        sd[n + ".bias"] = torch.from_numpy(gold[n + ".bias"])
    net.load_state_dict(sd)
    return mdl.Renderer(net, cfg['rendering'], device=torch.device(DEV))


def _shape_distance(p):
    """the distance of points to the surface of the shape the fixture was fitted to (tools/gen_golden_phong.py: a sphere of radius 1.2 at
    the origin united with a box at (1.2, 0.4, 0.3), half extents (0.6, 0.5, 0.7)): |signed distance of the union|, exact outside the shape"""
    p = p.double().cpu()
    sphere = p.norm(dim=-1) - 1.2
    q = (p - torch.tensor([1.2, 0.4, 0.3], dtype=torch.float64)).abs() - torch.tensor([0.6, 0.5, 0.7], dtype=torch.float64)
    box = q.clamp_min(0).norm(dim=-1) + q.max(dim=-1).values.clamp_max(0)
    return torch.minimum(sphere, box).abs()


@pytest.mark.parametrize("num_points", [256, 288])
def test_depth_maps_on_either_side_of_the_kernels_sample_limit(num_points):
    """C = 256 is the depth kernel's, C = 288 nnr.render_rays' forward-only depth with the accumulated weight made from its alphas: both
    against the renderer's own evaluation depth at the output bar, and both masked by min_acc (no ray accumulates more than 1 + 256e-6)"""
    from model import geometry as G
    from model import imaging
    renderer = _fitted_renderer(128, num_points)
    H, W = 12, 16
    K = torch.diag(torch.tensor(R.K_DIAG, dtype=torch.float64))
    Wm = R.look_at_world_mats(14, 3.5)[[2, 9]]
    maps = G.render_depth_maps(renderer, K, Wm, (H, W), min_acc=0., chunk=100)          # (chunks that are no multiple of anything)
    assert maps.shape == (2, H, W) and bool(torch.isfinite(maps).all())
    dev = torch.device(DEV)
    for i in range(2):
        _, fwd = imaging.render_full_image(renderer, (H, W), K.float().to(dev)[None], Wm[i].float().to(dev)[None], torch.eye(4, device=dev)[None],
                                           'nope_nerf', dev)
        ref = torch.from_numpy(np.asarray(fwd)).double()
        assert float(((maps[i].double().cpu() - ref).abs() / ref.abs().clamp(min=1.)).max()) <= 1e-4
    masked = G.render_depth_maps(renderer, K, Wm, (H, W), min_acc=1.01)
    assert bool(torch.isinf(masked).all()) and bool((masked > 0).all())
    half = G.render_depth_maps(renderer, K, Wm, (H, W), min_acc=0.5)
    keep = torch.isfinite(half)
    assert torch.equal(half[keep], maps[keep])


def test_fitted_scene_end_to_end(capsys):
    from model import geometry as G
    from model import imaging
    from nnr import ops
    renderer = _fitted_renderer(128)
    H, W = 24, 32
    K = torch.diag(torch.tensor(R.K_DIAG, dtype=torch.float64))
    Wm = R.look_at_world_mats(14, 3.5)
    cams = G.Cameras(K, Wm, (H, W))
    lo, hi, coarse, refine = (-2.4,) * 3, (2.4,) * 3, 17, 4
    depth = G.render_depth_maps(renderer, K, Wm, (H, W))
    assert depth.shape == (14, H, W) and depth.is_cuda and not bool(torch.isnan(depth).any())
    assert bool(torch.isfinite(depth).any())

    # the depth kernel's maps against the forward's, unmasked, at the output bar
    raw_maps = G.render_depth_maps(renderer, K, Wm[:3], (H, W), min_acc=0.)
    dev = torch.device(DEV)
    worst = 0.
    for i in range(3):
        _, fwd = imaging.render_full_image(renderer, (H, W), K.float().to(dev)[None], Wm[i].float().to(dev)[None], torch.eye(4, device=dev)[None],
                                           'nope_nerf', dev)
        ref = torch.from_numpy(np.asarray(fwd)).double()
        worst = max(worst, float(((raw_maps[i].double().cpu() - ref).abs() / ref.abs().clamp(min=1.)).max()))
    assert worst <= 1e-4, worst

    calls = []

    def integrate(o, s, br, cm, dp, tr, sm, wt):
        ops.tsdf_integrate(o, s, br, cm, dp, tr, sm, wt)
        calls.append((o, s, br.cpu(), cm.cpu(), tr, sm.cpu().clone(), wt.cpu().clone()))

    mesh = G.extract_mesh_tsdf(renderer, cams, lo, hi, coarse, refine=refine, depth_maps=depth, integrate=integrate)
    assert len(calls) == 2 and mesh.dims == (65, 65, 65) and mesh.refine == refine and 0 < mesh.n_bricks < 9 ** 3
    host_depth = depth.cpu()
    for o, s, br, cm, tr, sm, wt in calls:                          # the GPU volumes are the reference's on the downloaded maps
        want = torch.zeros(2, br.shape[0], 8, 8, 8)
        R.tsdf_integrate_ref(o, s, br, cm, host_depth, tr, want[0], want[1])
        assert torch.equal(_bits(sm), _bits(want[0])) and torch.equal(_bits(wt), _bits(want[1]))
    V = mesh.vertices.shape[0]
    assert V > 0 and mesh.quads.shape[0] > 0
    assert mesh.normals.shape == (V, 3) and mesh.colours.shape == (V, 3)

    # every vertex lies within trunc + sqrt(3) h in z of a depth some camera that observes it saw
    h = max(abs(v) for v in mesh.step)
    trunc = calls[1][4]
    assert abs(trunc - 3 * h) < 1e-6
    v = mesh.vertices.double().cpu()
    P = calls[1][3].double().view(14, 3, 4)
    q = torch.einsum('crk,vk->cvr', P[:, :, :3], v) + P[:, None, :, 3]                       # (14, V, 3)
    qz = q[..., 2]
    ci, ri = torch.round((q[..., 0] / qz + 1) * (W - 1) / 2), torch.round((q[..., 1] / qz + 1) * (H - 1) / 2)
    seen = (qz > 0) & (ci >= 0) & (ci <= W - 1) & (ri >= 0) & (ri <= H - 1)
    d = host_depth.double()[torch.arange(14)[:, None], ri.clamp(0, H - 1).long(), ci.clamp(0, W - 1).long()]
    seen = seen & torch.isfinite(d) & (d > 0)
    gap = torch.where(seen, (qz - d).abs(), torch.full_like(qz, INF)).min(0).values
    dist = _shape_distance(mesh.vertices)
    with capsys.disabled():
        print("\nTSDF mesh of the fitted D = 128 fixture, coarse %d^3 x %d from 14 cameras of %d x %d: %d bricks, %d vertices, %d quads; depth "
              "kernel against render_rays worst %.3e; worst vertex %.3f h in z from an observed depth (bound %.3f h); distance to the analytic "
              "shape: median %.3f h, 95 %% %.3f h, worst %.3f h (h = %.4f)"
              % (coarse, refine, H, W, mesh.n_bricks, V, mesh.quads.shape[0], worst, float(gap.max()) / h, (trunc + math.sqrt(3.) * h) / h,
                 float(dist.median()) / h, float(dist.quantile(0.95)) / h, float(dist.max()) / h, h))
    assert bool((gap <= trunc + math.sqrt(3.) * h).all()), "%d vertices further than trunc + sqrt(3) h from every observed depth" % int(
        (gap > trunc + math.sqrt(3.) * h).sum())
