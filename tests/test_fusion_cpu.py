"""CPU: the depth-fusion side of the geometry export without a GPU -- where the two entry points are declared and listed,
every error return of both reached with fake device pointers before anything is dereferenced or launched, the wrappers' refusal of CPU tensors
(what the build script holds the two kernels to: test_build_cpu.py), and the host side of model/geometry.py (extract_mesh_tsdf, tsdf_select_cells) on the reference
integrator of tests/fusion_ref.py: an analytic sphere seen from 14 cameras."""
import ctypes as C
import functools
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fusion_ref as R      # noqa: E402

OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3
INF, NAN = float("inf"), float("nan")


def _p(addr):
    return C.c_void_p(addr)


def _lib():
    from nnr import lib as L
    return L, L.load()


# ------------------------------------------------------------------------------------------------------------ header and exports
def test_the_entry_points_live_in_the_fusion_header_under_abi_8():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "nnr.h")).read()
    geo = open(os.path.join(ROOT, "include", "nnr_geometry.h")).read()
    fus = open(os.path.join(ROOT, "include", "nnr_fusion.h")).read()
    code = re.sub(r"/\*.*?\*/", "", fus, flags=re.S)
    assert lib.nnr_abi_version() == L.ABI_VERSION == int(re.search(r"#define NNR_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert "NNR_ABI_VERSION" not in code and '#include "nnr.h"' in code
    assert L.FUSION_EXPORTS == ("nnr_render_depth", "nnr_tsdf_integrate")
    assert L.GEOMETRY_EXPORTS == ("nnr_density_bricks",) and len(L.EXPORTS) == 50
    for name in L.FUSION_EXPORTS:
        assert name not in L.EXPORTS and name not in L.GEOMETRY_EXPORTS and hasattr(lib, name)
        assert name not in hdr and name not in geo
    protos = dict(re.findall(r"\bint\s+(nnr_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S))
    assert set(protos) == set(L.FUSION_EXPORTS)
    for name, params in protos.items():
        assert len(getattr(lib, name).argtypes) == params.count(",") + 1, name
    assert len(lib.nnr_render_depth.argtypes) == 11 and len(lib.nnr_tsdf_integrate.argtypes) == 14


# ------------------------------------------------------------------------------------------------------------ nnr_render_depth: error returns
D_PTRS = dict(pts_o=0x10000, pts_d=0x20000, z_lo=0x30000, z_hi=0x40000, jitter=0x50000, packed=0x60000, out=0x70000, opt_raw=0x80000,
              opt_z=0x90000)


def _depth(n_rays=5, n_samples=64, hidden=256, flags=None, cfg=True, **ptrs):
    L, lib = _lib()
    flags = (L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2) if flags is None else flags
    c = L.Cfg(n_rays, n_samples, hidden, flags)
    a = dict(D_PTRS)
    a.update(ptrs)
    v = {k: (None if x is None else _p(x)) for k, x in a.items()}
    return lib.nnr_render_depth(C.byref(c) if cfg else None, v["pts_o"], v["pts_d"], v["z_lo"], v["z_hi"], v["jitter"], v["packed"], v["out"],
                                v["opt_raw"], v["opt_z"], None)


def test_render_depth_rejects_null_pointers_and_sizes_below_one():
    assert _depth(cfg=False) == E_BADCFG
    for name in ("pts_o", "pts_d", "z_lo", "z_hi", "packed", "out"):
        assert _depth(**{name: None}) == E_BADCFG, name
    for n in (0, -1, -2 ** 31):
        assert _depth(n_rays=n) == E_BADCFG and _depth(n_samples=n) == E_BADCFG
    # jitter and the two test outputs may be null: such a call reaches the alignment check
    assert _depth(jitter=None, opt_raw=None, opt_z=None, packed=0x60008) == E_ALIGN


def test_render_depth_limits_samples_width_and_flags():
    L, _ = _lib()
    s2 = L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    assert _depth(n_samples=257) == E_UNSUPPORTED and _depth(n_samples=2 ** 31 - 1) == E_UNSUPPORTED
    assert _depth(n_samples=256, packed=0x60004) == E_ALIGN and _depth(n_samples=1, packed=0x60004) == E_ALIGN
    for hidden in (64, 192, 512, 0):
        assert _depth(hidden=hidden) == E_UNSUPPORTED
    assert _depth(hidden=128, packed=0x60004) == E_ALIGN
    for flags in (0, L.NNR_F_SPLIT3, L.NNR_F_SPLIT2, s2 | L.NNR_F_TRAIN, s2 | L.NNR_F_BF16, L.NNR_F_BF16, s2 | L.NNR_F_TRAIN | L.NNR_F_DIST_ALPHA):
        assert _depth(flags=flags) == E_UNSUPPORTED, flags
    for flags in (s2, s2 | L.NNR_F_DIST_ALPHA, s2 | L.NNR_F_RELU_SIGMA, s2 | L.NNR_F_DIST_ALPHA | L.NNR_F_RELU_SIGMA, s2 | L.NNR_F_WHITE_BG):
        assert _depth(flags=flags, packed=0x60008) == E_ALIGN, flags


def test_render_depth_rejects_misaligned_pointers():
    for addr in (0x60001, 0x60002, 0x60004, 0x60008, 0x6000c):
        assert _depth(packed=addr) == E_ALIGN, hex(addr)
    for name in ("pts_o", "pts_d", "z_lo", "z_hi", "jitter", "out", "opt_raw", "opt_z"):
        for off in (1, 2, 3):
            assert _depth(**{name: D_PTRS[name] + off}) == E_ALIGN, (name, off)
    # (out is two floats per ray, written one by one: 4-byte alignment is all it needs -- an 8-byte-odd address reaches the next check)
    assert _depth(out=0x70004, packed=0x60004) == E_ALIGN and _depth(out=0x70004, n_samples=257) == E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------ nnr_tsdf_integrate: error returns
T_PTRS = dict(bricks=0x10000, cams=0x20000, depth=0x30000, sum=0x40000, weight=0x50000)


def _tsdf(n_bricks=3, n_cams=2, H=5, W=7, trunc=0.1, z_min=0., origin=(0., 0., 0.), step=(1., 1., 1.), null=(), **ptrs):
    _, lib = _lib()
    a = dict(T_PTRS)
    a.update(ptrs)
    v = {k: (None if (x is None or k in null) else _p(x)) for k, x in a.items()}
    o3 = None if "origin" in null else (C.c_float * 3)(*origin)
    s3 = None if "step" in null else (C.c_float * 3)(*step)
    return lib.nnr_tsdf_integrate(o3, s3, v["bricks"], n_bricks, v["cams"], n_cams, v["depth"], H, W, trunc, z_min, v["sum"], v["weight"], None)


def test_tsdf_integrate_rejects_null_pointers_and_sizes_below_one():
    for name in ("origin", "step", "bricks", "cams", "depth", "sum", "weight"):
        assert _tsdf(null=(name,)) == E_BADCFG, name
    for n in (0, -1, -2 ** 31):
        assert _tsdf(n_bricks=n) == E_BADCFG and _tsdf(n_cams=n) == E_BADCFG and _tsdf(H=n) == E_BADCFG and _tsdf(W=n) == E_BADCFG
    assert _tsdf(n_bricks=1, n_cams=1, H=1, W=1, sum=0x40002) == E_ALIGN          # the smallest sizes pass


@pytest.mark.parametrize("bad", [INF, -INF, NAN])
def test_tsdf_integrate_rejects_non_finite_values(bad):
    for axis in range(3):
        v = [0.5, 0.5, 0.5]
        v[axis] = bad
        assert _tsdf(origin=v) == E_BADCFG and _tsdf(step=v) == E_BADCFG
    assert _tsdf(trunc=bad) == E_BADCFG and _tsdf(z_min=bad) == E_BADCFG


def test_tsdf_integrate_wants_a_positive_truncation_and_a_non_negative_near_bound():
    for trunc in (0., -0., -1e-3, -1.):
        assert _tsdf(trunc=trunc) == E_BADCFG
    assert _tsdf(z_min=-1e-6) == E_BADCFG
    assert _tsdf(trunc=1e-30, z_min=0., sum=0x40001) == E_ALIGN and _tsdf(z_min=2.5, sum=0x40001) == E_ALIGN


def test_tsdf_integrate_limits_the_voxel_and_pixel_counts():
    for n in (2 ** 22, 2 ** 22 + 1, 2 ** 31 - 1):
        assert _tsdf(n_bricks=n) == E_UNSUPPORTED
    assert _tsdf(n_bricks=2 ** 22 - 1, sum=0x40001) == E_ALIGN                     # 512 (2^22 - 1) = 2^31 - 512 voxels
    assert _tsdf(n_cams=2 ** 11, H=2 ** 10, W=2 ** 10) == E_UNSUPPORTED            # 2^31 pixels
    assert _tsdf(n_cams=2 ** 11, H=2 ** 10, W=2 ** 10 - 1, sum=0x40001) == E_ALIGN
    assert _tsdf(n_cams=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1) == E_UNSUPPORTED  # (no overflow in the product)
    assert _tsdf(n_cams=1, H=1, W=2 ** 24 + 1) == E_UNSUPPORTED and _tsdf(n_cams=1, H=2 ** 24 + 1, W=1) == E_UNSUPPORTED
    assert _tsdf(n_cams=1, H=1, W=2 ** 24, sum=0x40001) == E_ALIGN                 # a pixel index is compared as an exact fp32


def test_tsdf_integrate_rejects_misaligned_pointers():
    for name in T_PTRS:
        for off in (1, 2, 3):
            assert _tsdf(**{name: T_PTRS[name] + off}) == E_ALIGN, (name, off)
    assert _tsdf(bricks=0x10004, cams=0x20004, depth=0x30004, sum=0x40004, weight=0x50002) == E_ALIGN


# ------------------------------------------------------------------------------------------------------------ the wrappers
def _net(hidden=128):
    import model as mdl
    return mdl.OfficialStaticNerf({'model': {'hidden_dim': hidden, 'pos_enc_levels': 10, 'dir_enc_levels': 4, 'occ_activation': 'softplus'},
                                   'rendering': {'white_background': False, 'dist_alpha': False}})


def test_the_ops_wrappers_raise_on_cpu_tensors():
    from nnr import ops
    net = _net()
    z = torch.linspace(0.1, 2., 8)
    with pytest.raises(RuntimeError):
        ops.render_depth(torch.zeros(4, 3), torch.ones(4, 3), z, z, None, net.weights(), net.biases(), hidden=128, dist_alpha=False,
                         relu_sigma=False)
    acc = torch.zeros(2, 2, 8, 8, 8)
    with pytest.raises(RuntimeError):
        ops.tsdf_integrate((0., 0., 0.), (.1, .1, .1), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(1, 12), torch.ones(1, 4, 4), 0.3,
                           acc[0], acc[1])


def test_the_gpu_only_geometry_functions_say_so_on_the_cpu():
    import model as mdl
    from model import geometry as G
    cfg = {'type': 'nope_nerf', 'n_max_network_queries': 64000, 'white_background': False, 'radius': 4.0, 'num_points': 64,
           'depth_range': [0.01, 10], 'dist_alpha': False, 'use_ray_dir': True, 'normalise_ray': True, 'normal_loss': False,
           'sample_option': 'uniform', 'outside_steps': 0}
    K, Wm, depth = _scene()
    renderer = mdl.Renderer(_net(), cfg, device=torch.device('cpu'))
    with pytest.raises(NotImplementedError, match="GPU"):
        G.render_depth_maps(renderer, K, Wm, (4, 4))
    with pytest.raises(NotImplementedError, match="GPU"):
        G.extract_mesh_tsdf(renderer, G.Cameras(K, Wm, SIZE), LO, HI, 9)
    ndc = mdl.Renderer(_net(), dict(cfg, sample_option='ndc'), device=torch.device('cpu'))
    with pytest.raises(NotImplementedError, match="NDC"):
        G.render_depth_maps(ndc, K, Wm, (4, 4))


# ------------------------------------------------------------------------------------------------------------ the reference alone: a sphere
RADIUS, SIZE, LO, HI = 0.8, (24, 32), (-1.2,) * 3, (1.2,) * 3


@functools.lru_cache(maxsize=None)
def _scene():
    return R.sphere_scene(n_cams=14, cam_radius=3., size=SIZE, sphere_radius=RADIUS)


def _mesh(resolution, refine=None, **kw):
    from model import geometry as G
    K, Wm, depth = _scene()
    return G.extract_mesh_tsdf(None, G.Cameras(K, Wm, SIZE), LO, HI, resolution, refine=refine, integrate=R.tsdf_integrate_ref,
                               depth_maps=depth, **kw)


def test_the_depth_maps_of_the_scene_are_what_the_projection_sees():
    """the scene's own consistency: a surface point of a pixel's ray projects (projection_rows, the integrator's arithmetic in float64) back
    onto that pixel with the map's depth"""
    from model import geometry as G
    K, Wm, depth = _scene()
    rows = G.projection_rows(K, Wm)
    assert rows.shape == (14, 12) and rows.dtype == torch.float32
    assert torch.equal(rows, (K @ Wm)[:, :3].reshape(14, 12).to(torch.float32))
    H, W = SIZE
    for c in (0, 5, 13):
        o, d = R.pixel_rays(Wm[c].numpy(), H, W)
        hit = torch.isfinite(depth[c])
        assert 8 < int(hit.sum()) < H * W
        P = rows[c].double().view(3, 4).numpy()
        p = o + d * np.where(hit.numpy(), depth[c].double().numpy(), 1.)[..., None]
        q = np.where(hit.numpy()[..., None], p @ P[:, :3].T + P[:, 3], 1.)
        col, row = (q[..., 0] / q[..., 2] + 1) * (W - 1) / 2, (q[..., 1] / q[..., 2] + 1) * (H - 1) / 2
        jj, ii = np.meshgrid(np.arange(W), np.arange(H))
        m = hit.numpy()
        assert np.abs(col - jj)[m].max() < 1e-4 and np.abs(row - ii)[m].max() < 1e-4
        assert np.abs(q[..., 2] - depth[c].numpy())[m].max() < 1e-5
        assert np.abs(np.linalg.norm(p[m], axis=-1) - RADIUS).max() < 1e-5


def test_the_dense_tsdf_mesh_of_a_sphere_is_a_closed_sphere():
    mesh = _mesh(17)
    h = 2.4 / 16
    assert mesh.dims == (17, 17, 17) and mesh.level == 0. and mesh.n_bricks == 27 and abs(mesh.step[0] - h) < 1e-7
    V, E, F, lo, hi = R.mesh_topology(mesh.vertices, mesh.quads)
    assert V > 100 and len(np.unique(mesh.quads.numpy())) == V                   # every vertex is used
    assert lo == 2 and hi == 2, "an edge with %d / %d quads: the mesh is not closed" % (lo, hi)
    assert V - E + F == 2
    dist = (mesh.vertices.double().norm(2, 1) - RADIUS).abs().max().item()
    print("dense TSDF sphere: %d vertices, %d quads, worst vertex %.3f h from the sphere" % (V, F, dist / h))
    assert dist <= math.sqrt(3.) * h
    # the normals point outwards: inside is positive
    q = mesh.vertices[mesh.quads].double()
    n = torch.cross(q[:, 1] - q[:, 0], q[:, 3] - q[:, 0], dim=1)
    assert bool(((n * q.mean(1)).sum(1) > 0).all())


def test_tsdf_volume_and_select_cells_ignore_unobserved_space_and_dilate():
    from model import geometry as G
    s = torch.tensor([[1., -2.], [0., 3.]])
    w = torch.tensor([[2., 4.], [0., 1.]])
    v = G.tsdf_volume(s, w)
    assert v[0, 0] == 0.5 and v[0, 1] == -0.5 and torch.isnan(v[1, 0]) and v[1, 1] == 3.
    vol = torch.full((6, 6, 6), NAN)
    assert not bool(G.tsdf_select_cells(vol, 0).any()) and bool(G.select_cells(vol, 0., 0).all())
    vol[0, 0, 0] = 1.                                              # one finite corner, or finite corners on one side: no crossing
    vol[0, 0, 1] = 0.5
    assert not bool(G.tsdf_select_cells(vol, 1).any())
    vol[3, 3, 3], vol[3, 3, 4] = 0.25, -0.25                       # a crossing between two finite corners, NaN all around
    sel = G.tsdf_select_cells(vol, 0)
    want = torch.zeros(5, 5, 5, dtype=torch.bool)
    want[2:4, 2:4, 3] = True                                       # the four cells that hold both ends of that edge
    assert torch.equal(sel, want)
    vol[3, 3, 4] = 0.                                              # zero is outside, as in surface_nets (inside is > 0)
    assert torch.equal(G.tsdf_select_cells(vol, 0), want)
    sel1 = G.tsdf_select_cells(vol, 1)
    want1 = torch.zeros(5, 5, 5, dtype=torch.bool)
    want1[1:5, 1:5, 2:5] = True
    assert torch.equal(sel1, want1)
    with pytest.raises(ValueError):
        G.tsdf_select_cells(vol, -1)
    assert G.tsdf_select_cells(torch.zeros(1, 4, 4), 1).shape == (0, 3, 3)


def _rows(t):
    return [r.tobytes() for r in np.ascontiguousarray(t.cpu().numpy())]


@pytest.mark.parametrize("coarse,refine", [(9, 4), (17, 2)])
def test_the_refined_tsdf_mesh_is_the_dense_fine_one(coarse, refine):
    """the sparse mesh against surface_nets of the dense fine TSDF (the same depth maps, the same truncation in fine steps): every vertex
    and quad is one of the dense mesh's, and for the sphere with dilate = 1 the two are equal outright"""
    from model import geometry as G
    K, Wm, depth = _scene()
    mesh = _mesh(coarse, refine)
    origin, step_c, dims_c, step_f, dims_f = G.refined_grid(LO, HI, coarse, refine)
    assert mesh.dims == dims_f == (33, 33, 33) and mesh.refine == refine and 0 < mesh.n_bricks < 125
    bricks = G._all_bricks(dims_f, 'cpu')
    acc = torch.zeros(2, 125, 8, 8, 8)
    R.tsdf_integrate_ref(origin, step_f, bricks, G.projection_rows(K, Wm), depth, 3 * max(step_f), acc[0], acc[1])
    fine = G._dense_from_bricks(G.tsdf_volume(acc[0], acc[1]), dims_f)
    assert fine.shape == (33, 33, 33) and bool(torch.isnan(fine).any()) and bool((fine > 0).any()) and bool((fine < 0).any())
    verts, quads = G.surface_nets(fine, 0., origin, step_f)
    where = {r: i for i, r in enumerate(_rows(verts))}
    to_dense = np.array([where.get(r, -1) for r in _rows(mesh.vertices)], dtype=np.int64)
    assert (to_dense >= 0).all() and (np.diff(to_dense) > 0).all()
    dense_q = {r: i for i, r in enumerate(_rows(quads))}
    at = np.array([dense_q.get(r, -1) for r in _rows(torch.from_numpy(to_dense)[mesh.quads])], dtype=np.int64)
    assert (at >= 0).all() and (np.diff(at) > 0).all()
    assert torch.equal(mesh.vertices.view(torch.int32), verts.view(torch.int32)) and torch.equal(mesh.quads, quads)
    with pytest.raises(ValueError, match=str(mesh.n_bricks)):
        _mesh(coarse, refine, max_bricks=mesh.n_bricks - 1)


def test_cameras_in_chunks_give_the_one_call_result_bit_for_bit():
    from model import geometry as G
    K, Wm, depth = _scene()
    origin, step, dims = G.grid_of(LO, HI, 17)
    bricks = G._all_bricks(dims, 'cpu')
    cams = G.projection_rows(K, Wm)
    trunc = 3 * step[0]
    start = torch.randn(2, 27, 8, 8, 8, generator=torch.Generator().manual_seed(3))
    one, two = start.clone(), start.clone()
    R.tsdf_integrate_ref(origin, step, bricks, cams, depth, trunc, one[0], one[1])
    R.tsdf_integrate_ref(origin, step, bricks, cams[:3], depth[:3], trunc, two[0], two[1])
    assert not torch.equal(one, two)
    R.tsdf_integrate_ref(origin, step, bricks, cams[3:], depth[3:], trunc, two[0], two[1])
    assert torch.equal(one.view(torch.int32), two.view(torch.int32)) and not torch.equal(one, start)


# ------------------------------------------------------------------------------------------------------------ checkpoints
def test_train_scene_checkpoints_load_in_extract_mesh(tmp_path):
    """tools/train_scene.py: save_checkpoints -> tools/extract_mesh.py: CheckpointIO(...).load('model.pt') as load_renderer does, and
    load_pose_table: a tiny network and a pose table come back bit for bit"""
    import model as mdl
    import extract_mesh
    import train_scene
    cfg = train_scene.scene_cfg(str(tmp_path), "none", hidden=128, n_samples=16)
    cfg['training']['out_dir'] = str(tmp_path / "run")
    dev = torch.device('cpu')
    torch.manual_seed(5)
    nope = mdl.get_model(mdl.Renderer(mdl.OfficialStaticNerf(cfg), cfg['rendering'], device=dev), cfg, device=dev)
    pose = mdl.LearnPose(5, True, True, cfg, init_c2w=None)
    with torch.no_grad():
        pose.r.copy_(0.1 * torch.randn(5, 3))
        pose.t.copy_(torch.randn(5, 3))
    train_scene.save_checkpoints(cfg['training']['out_dir'], nope, pose, epoch_it=3, it=41)
    assert sorted(os.listdir(cfg['training']['out_dir'])) == ["model.pt", "model_pose.pt"]
    torch.manual_seed(6)
    nope2 = mdl.get_model(mdl.Renderer(mdl.OfficialStaticNerf(cfg), cfg['rendering'], device=dev), cfg, device=dev)
    assert not all(torch.equal(a, b) for a, b in zip(nope.state_dict().values(), nope2.state_dict().values()))
    scalars = mdl.CheckpointIO(cfg['training']['out_dir'], model=nope2).load('model.pt')
    assert scalars == {'epoch_it': 3, 'it': 41}
    for (ka, a), (kb, b) in zip(nope.state_dict().items(), nope2.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
    pose2 = extract_mesh.load_pose_table(cfg['training']['out_dir'], 5, cfg, dev)
    assert torch.equal(pose2.r, pose.r) and torch.equal(pose2.t, pose.t)
    for i in range(5):
        assert torch.equal(pose2(i), pose(i))
    focal = mdl.LearnFocal(True, False)
    train_scene.save_checkpoints(cfg['training']['out_dir'], nope, pose, focal=focal)
    assert "model_focal.pt" in os.listdir(cfg['training']['out_dir'])
