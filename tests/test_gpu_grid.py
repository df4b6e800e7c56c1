"""GPU (-m gpu): the fused density-grid kernel (nnr_grid_f16.hip through nnr.ops.density_grid) and the mesh extraction on top of it
(model/geometry.py).  The kernel against the path a user had before it, nnr.ops.mlp_points on the same points built on the host in fp32 (bit
for bit: the same trunk text and head code on the same point bits), at the sizes where the indexing can go wrong, with a guard band around the
output; slabs, determinism, negative and anisotropic steps, the fp16-range rule; extract_mesh on a fitted network."""
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

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(ROOT, "tests", "golden")
H, W = 54, 96                     # the fitted phong fixtures' frame (tests/golden/phong_d{128,256}.npz)
LAYERS = ("layers0.0", "layers0.2", "layers0.4", "layers0.6", "layers1.0", "layers1.2", "layers1.4", "layers1.6", "fc_density",
          "fc_feature", "rgb_layers.0", "fc_rgb")
GUARD = 512                       # floats on either side of the output
SENTINEL = 0x7fc0beef             # a NaN with a payload no kernel writes


def _cfg(hidden):
    return {'model': {'hidden_dim': hidden, 'pos_enc_levels': 10, 'dir_enc_levels': 4, 'occ_activation': 'softplus'},
            'rendering': {'type': 'nope_nerf', 'n_max_network_queries': 64000, 'white_background': False, 'radius': 4.0,
                          'num_points': 64, 'depth_range': [0.01, 10], 'dist_alpha': False, 'use_ray_dir': True,
                          'normalise_ray': True, 'normal_loss': False, 'sample_option': 'uniform', 'outside_steps': 0},
            'depth': {'type': 'None'}, 'distortion': {'fix_scaleN': True}}


def _fitted_renderer(hidden):
    """the network fitted to a sphere and a box that the phong goldens were rendered from (weights stored as integer mantissa q and
    per-row exponent e) -> (Renderer on the GPU, the fixture with its two cameras K{0,1} / world_mat{0,1})"""
    import model as mdl
    gold = np.load(os.path.join(GOLDEN, "phong_d%d.npz" % hidden))
    cfg = _cfg(hidden)
    net = mdl.OfficialStaticNerf(cfg)
    sd = {}
    for n in LAYERS:
        q, e = torch.from_numpy(gold[n + ".q"].astype(np.float32)), torch.from_numpy(gold[n + ".e"].astype(np.float32))
        sd[n + ".weight"] = q * torch.exp2(e)[:, None]
        sd[n + ".bias"] = torch.from_numpy(gold[n + ".bias"])
    net.load_state_dict(sd)
    return mdl.Renderer(net, cfg['rendering'], device=torch.device(DEV)), gold


def _active_cells(vol, level):
    """(V,3) (cx, cy, cz) of the cells whose 8 corners straddle the level and hold no NaN, in cell order (x fastest) -- numpy restatement"""
    v = vol.numpy().astype(np.float64)
    nz, ny, nx = v.shape
    corner = lambda a: [a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    cnt = sum(w.astype(np.int32) for w in corner(v > level))
    cz, cy, cx = np.nonzero((cnt > 0) & (cnt < 8) & ~np.any(corner(np.isnan(v)), axis=0))
    return np.stack([cx, cy, cz], 1)


@functools.lru_cache(maxsize=None)
def _net(hidden, kind='random'):
    """'random': a fresh network.  'hot': its first layer times 64 -- activations 64 times larger all the way down: inside fp16's range near
    the origin, outside it a few thousand units away (the identity block of the position encoding grows with the point).  'loud': the first
    layer times 2e5, the construction of tests/test_gpu_split3.py::test_two_term_forward_activation_beyond_fp16_range_is_loud: hidden 1 at
    ~1e5 wherever a unit of it is active."""
    import model as mdl
    torch.manual_seed(23 + hidden)
    net = mdl.OfficialStaticNerf(_cfg(hidden))
    with torch.no_grad():
        if kind == 'hot':
            net.layers0[0].weight.mul_(64.0)
        elif kind == 'loud':
            net.layers0[0].weight.mul_(2.0e5)
    return net.to(DEV)


def _host_points(origin, step, dims):
    """the kernel's points restated in numpy fp32: the product rounded, then the sum; (V,3), x fastest"""
    nx, ny, nz = dims
    ax = [np.float32(origin[c]) + np.float32(step[c]) * np.arange(n, dtype=np.float32) for c, n in enumerate(dims)]
    assert all(a.dtype == np.float32 for a in ax)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return torch.from_numpy(np.stack([x, y, z], -1).reshape(-1, 3)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _grid_guarded(net, hidden, origin, step, dims):
    """nnr_density_grid through the C ABI into the middle of a sentinel-filled buffer -> (volume (nz, ny, nx), the buffer's two guard bands)"""
    from nnr import lib as L
    from nnr import ops
    nx, ny, nz = dims
    V = nx * ny * nz
    cfg = ops.split2_cfg(V, 1, hidden)
    packed = ops._packed_for(cfg, net.weights(), net.biases())
    buf = torch.full((V + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    o3, s3, d3 = (C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*dims)
    L.check(L.load().nnr_density_grid(C.byref(cfg), o3, s3, d3, L.ptr(packed), C.c_void_p(buf.data_ptr() + 4 * GUARD), L.stream()),
            "nnr_density_grid")
    torch.cuda.synchronize()
    return buf[GUARD:GUARD + V].view(torch.float32).view(nz, ny, nx), torch.cat([buf[:GUARD], buf[GUARD + V:]])


def _mlp_points_raw(net, hidden, pts):
    from nnr import ops
    return ops.mlp_points(pts, torch.zeros_like(pts), net.weights(), net.biases(), hidden=hidden, split2=True)[1]


# 128-voxel blocks per case and the launcher's rule (nnr_grid_f16.hip: passes = clamp(blocks / 1024, 1, 32)):
#   (1,1,1), (127,1,1), (129,1,1): one voxel; either side of one block (the second has a one-voxel second block)
#   (5,7,3): ragged in every axis, part of one wave's row
#   (129,41,50): 264 450 voxels = 2067 blocks -> 2 passes per workgroup, 1034 workgroups, the last with ONE pass, its block 2 voxels full
#   (64,64,64): 2048 blocks -> 2 passes in each of 1024 workgroups, no tail
# origins and steps: negative, anisotropic and non-dyadic among them
CASES = [((1, 1, 1), (0.3, -0.2, 0.1), (0.1, 0.1, 0.1)),
         ((127, 1, 1), (-1.0, 0.25, -0.5), (2.0 / 126, 1.0, 1.0)),
         ((129, 1, 1), (1.0, 0.25, -0.5), (-2.0 / 128, 1.0, 1.0)),
         ((5, 7, 3), (-0.7, 0.9, -0.3), (0.31, -0.27, 0.33)),
         ((129, 41, 50), (-1.0, -0.8, 1.1), (2.0 / 128, 0.037, -0.043)),
         ((64, 64, 64), (-1.0, -1.0, -1.0), (2.0 / 63, 2.0 / 63, 2.0 / 63))]


@pytest.mark.parametrize("hidden", [128, 256])
@pytest.mark.parametrize("dims,origin,step", CASES, ids=["x".join(map(str, c[0])) for c in CASES])
def test_grid_equals_mlp_points_bit_for_bit(hidden, dims, origin, step):
    net = _net(hidden)
    vol, guard = _grid_guarded(net, hidden, origin, step, dims)
    assert bool((guard == SENTINEL).all()), "the kernel wrote outside its output"
    assert not bool((_bits(vol) == SENTINEL).any()), "a voxel was not written"
    ref = _mlp_points_raw(net, hidden, _host_points(origin, step, dims)).view(dims[2], dims[1], dims[0])
    assert torch.isfinite(ref).all()
    diff = (_bits(vol) != _bits(ref))
    assert not bool(diff.any()), "%d of %d voxels differ, worst |difference| %.3e" % (int(diff.sum()), vol.numel(),
                                                                                     float((vol - ref).abs().max()))


def test_ops_density_grid_is_the_entry_point_and_two_runs_agree():
    from nnr import ops
    dims, origin, step = CASES[4]
    net = _net(128)
    a = ops.density_grid(origin, step, dims, net.weights(), net.biases(), hidden=128)
    b = ops.density_grid(origin, step, dims, net.weights(), net.biases(), hidden=128)
    raw, _ = _grid_guarded(net, 128, origin, step, dims)
    assert a.shape == (dims[2], dims[1], dims[0]) and a.dtype == torch.float32
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(raw))
    with pytest.raises(ValueError):
        ops.density_grid(origin, step, (4, 0, 4), net.weights(), net.biases(), hidden=128)


class _R:      # what density_volume needs of a Renderer
    def __init__(self, net):
        self.model = net


@pytest.mark.parametrize("hidden,lo,hi,res,slab", [(128, (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8), (20, 24, 37), 5),
                                                   (256, (0.7, -0.5, 1.3), (-0.7, 0.5, -1.1), (24, 20, 33), 8),
                                                   (128, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (16, 16, 33), 1)])
def test_slabbed_volume_equals_the_single_call(hidden, lo, hi, res, slab):
    from model import geometry as G
    r = _R(_net(hidden))
    whole = G.density_volume(r, lo, hi, res)
    slabbed = G.density_volume(r, lo, hi, res, slab=slab)
    assert whole.shape == (res[2], res[1], res[0]) and torch.isfinite(whole).all()
    assert torch.equal(_bits(whole), _bits(slabbed))
    # and the volume is what the documented grid says: mlp_points on grid_of's points
    origin, step, dims = G.grid_of(lo, hi, res)
    ref = _mlp_points_raw(r.model, hidden, _host_points(origin, step, dims)).view_as(whole)
    assert torch.equal(_bits(whole), _bits(ref))


def _max_activation(net, pts):
    """the largest hidden activation of the trunk per point, in float64 torch (the quantity left_f16_range looks at, up to rounding)"""
    from model.official_nerf import POS_LEVELS, encode_position
    x = encode_position(pts.double(), levels=POS_LEVELS, inc_input=True)
    p = x
    h, mx = x, torch.zeros(p.shape[0], dtype=torch.float64, device=pts.device)
    for i in range(4):
        h = torch.relu(torch.nn.functional.linear(h, net.layers0[2 * i].weight.double(), net.layers0[2 * i].bias.double()))
        mx = torch.maximum(mx, h.amax(1))
    h = torch.cat([h, x], -1)                                  # the skip connection: [h, posenc]
    for i in range(4):
        h = torch.relu(torch.nn.functional.linear(h, net.layers1[2 * i].weight.double(), net.layers1[2 * i].bias.double()))
        mx = torch.maximum(mx, h.amax(1))
    return mx


@pytest.mark.parametrize("hidden,kind,dims,origin,step", [(128, 'hot', (160, 3, 2), (-2.0e4, 0.1, -0.2), (250.0, 0.3, 0.4)),
                                                          (256, 'hot', (160, 3, 2), (-2.0e4, 0.1, -0.2), (250.0, 0.3, 0.4)),
                                                          (128, 'loud', (33, 9, 5), (-1.0, -1.0, -1.0), (2.0 / 32, 0.25, 0.5))])
def test_activations_beyond_fp16_range_give_nan_and_only_there(hidden, kind, dims, origin, step):
    """A voxel whose trunk activations leave fp16's range is NaN (it would otherwise come out finite and wrong: ReLU turns the NaN products
    into zeros); every other voxel is what mlp_points gives, bit for bit.  Which voxels those are is decided by a float64 restatement of the
    trunk with 5 % of room either side of the bound, 65520."""
    net = _net(hidden, kind)
    vol, guard = _grid_guarded(net, hidden, origin, step, dims)
    assert bool((guard == SENTINEL).all())
    pts = _host_points(origin, step, dims)
    with torch.no_grad():
        mx = _max_activation(net, pts).view_as(vol)
    nan = torch.isnan(vol)
    print("\n%s, D = %d: %d of %d voxels NaN; restated activations %.3g .. %.3g" % (kind, hidden, int(nan.sum()), vol.numel(), float(mx.min()),
                                                                                  float(mx.max())))
    assert bool(nan[mx > 1.05 * 65520.].all()) and not bool(nan[mx < 0.95 * 65520.].any())
    assert bool((mx > 1.05 * 65520.).any())
    if kind == 'hot':
        assert bool((mx < 0.95 * 65520.).any())
    ref = _mlp_points_raw(net, hidden, pts).view_as(vol)      # (NaN there as well, and where the colour branch leaves the range)
    both = ~nan & ~torch.isnan(ref)
    assert torch.equal(_bits(vol)[both], _bits(ref)[both])
    assert not bool((nan & ~torch.isnan(ref)).any())
    assert not bool(torch.isinf(vol).any())


def test_extract_mesh_on_the_fitted_scene(capsys):
    """Structure of the mesh of the fitted phong fixture (a sphere and a box) at 48^3 inside the renderer's sphere, and -- a measurement, not
    a bar -- how many of the phong renderer's surface points have a mesh vertex within a cell's diagonal."""
    from model import geometry as G
    from model.common import arange_pixels
    from nnr import camera
    renderer, gold = _fitted_renderer(128)
    rad = float(renderer.cfg['radius'])
    half = rad / math.sqrt(3.)                                 # the cube inscribed in the sphere the phong renderer marches in
    lo, hi, n = (-half,) * 3, (half,) * 3, 48
    mesh = G.extract_mesh(renderer, lo, hi, n)
    V, Q = mesh.vertices.shape[0], mesh.quads.shape[0]
    assert V > 0 and Q > 0
    assert mesh.level == G.level_for(renderer.cfg, renderer.model.occ_activation)
    q = mesh.quads
    assert int(q.min()) >= 0 and int(q.max()) < V
    qs = q.sort(1).values
    assert bool((qs[:, 1:] != qs[:, :-1]).all())                # four distinct corners
    # every vertex inside its cell (cells restated in numpy from the same volume; slack: fp32 rounding of a coordinate below 4)
    vol = G.density_volume(renderer, lo, hi, n)
    cells = _active_cells(vol.cpu(), mesh.level)
    assert cells.shape[0] == V
    o, s = np.array(mesh.origin), np.array(mesh.step)
    v = mesh.vertices.double().cpu().numpy()
    slack = 4 * 4 * 2. ** -24
    assert (v >= o + s * cells - slack).all() and (v <= o + s * (cells + 1) + slack).all()
    nrm = mesh.normals
    assert nrm.shape == (V, 3) and not bool(torch.isnan(nrm).any())
    assert float((nrm.norm(2, 1) - 1).abs().max()) < 1e-5
    assert mesh.colours.shape == (V, 3) and float(mesh.colours.min()) >= 0. and float(mesh.colours.max()) <= 1.
    no_colour = G.extract_mesh(renderer, lo, hi, n, colour=False, volume=vol)      # the volume handed in: the same mesh
    assert no_colour.colours is None and torch.equal(no_colour.vertices, mesh.vertices) and torch.equal(no_colour.quads, mesh.quads)
    with pytest.raises(ValueError):
        G.extract_mesh(renderer, lo, hi, n, volume=vol[1:])
    # the measurement: phong hits of both fixture cameras against the mesh
    h = float(np.linalg.norm(s))                               # = sqrt(3) h for this cubic grid
    lines = []
    pixels = arange_pixels(resolution=(H, W))[1].to(DEV)
    for ci in (0, 1):
        K, Wm, S = torch.from_numpy(gold["K%d" % ci]).to(DEV), torch.from_numpy(gold["world_mat%d" % ci]).to(DEV), torch.eye(4)[None].to(DEV)
        origin, ray, _, _, _, _ = camera.ray_setup(pixels, None, K, Wm, S, True, True)
        with torch.no_grad():
            d = renderer.ray_marching(origin.unsqueeze(0), ray.unsqueeze(0), renderer.model, n_secant_steps=8, n_steps=[512, 513], rad=rad)[0]
        hit = torch.isfinite(d) & (d != 0)
        pts = (origin + ray * d.unsqueeze(-1))[hit]
        inside = (pts.abs() <= half).all(1)
        near = torch.cdist(pts, mesh.vertices).amin(1) <= h if pts.shape[0] else torch.zeros(0, dtype=torch.bool, device=DEV)
        lines.append("camera %d: %d phong hits, %d inside the cube; within sqrt(3) h = %.4f of a mesh vertex: %.4f of all hits, %.4f of those "
                     "inside the cube" % (ci, int(hit.sum()), int(inside.sum()), h, float(near.float().mean()) if pts.shape[0] else float('nan'),
                                          float(near[inside].float().mean()) if int(inside.sum()) else float('nan')))
    with capsys.disabled():
        print("\nextract_mesh, fitted D = 128, 48^3 in [-%.3f, %.3f]^3: %d vertices, %d quads, level %.4f" % (half, half, V, Q, mesh.level))
        print("\n".join(lines))
