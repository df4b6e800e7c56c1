"""CPU: the sparse frozen-field render (include/nnr_frozen_sparse.h) without a GPU -- its float64 restatement
(tests/frozen_sparse_ref.py) against the sparse inference render's (tests/sparse_ref.py), where its entry points are declared and listed,
its workspace, every error return reached with fake device pointers, and the key parsing of the operator and of Trainer_pose."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nope-nerf_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import frozen_sparse_ref as FS      # noqa: E402
import sparse_ref as SR             # noqa: E402

OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3
P_OUT4, P_Z, P_DOUT4, P_DPTS, P_DVIEW, P_XE, P_XF, P_MASK = 0, 1, 2, 3, 4, 10, 19, 25
F64 = torch.float64


def _lib():
    from nnr import lib as L
    return L, L.load()


def _cfg(R, N, D, flags=None):
    L, _ = _lib()
    return L.Cfg(R, N, D, (L.NNR_F_TRAIN | L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2) if flags is None else flags)


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("dist_alpha,relu_sigma,white_bg", [(False, False, False), (True, False, True), (False, True, False), (True, True, False)])
def test_the_restatement_is_the_masked_composite_up_to_one_epsilon_per_culled_sample(dist_alpha, relu_sigma, white_bg):
    """A culled sample is ABSENT from tests/sparse_ref.py's product (factor 1) and PRESENT with alpha 0 here (factor (1 - 0) + 1e-6): a live
    sample's weight is the masked one times (1 + 1e-6)^k, k <= n_culled the culled samples in front of it.  So every output differs from the
    masked composite by at most ((1 + 1e-6)^n_culled - 1) sum w |value| -- n_culled 1e-6 relative -- and never by more."""
    g = torch.Generator().manual_seed(5)
    R, N = 9, 70
    raw = torch.randn(R, N, generator=g, dtype=F64) * 3.0
    rgb = torch.rand(R, N, 3, generator=g, dtype=F64)
    z = torch.sort(torch.rand(R, N, generator=g) * 6.0, dim=1).values
    live = FS.live_rule(torch.rand(R, N, generator=g) < 0.6, dist_alpha)
    live[0] = True
    live[1] = False
    live = FS.live_rule(live, dist_alpha)
    got = FS.composite(rgb, raw, z, live, dist_alpha, relu_sigma, white_bg)
    alpha = FS.alpha_ref(raw, z, dist_alpha, relu_sigma)
    want = SR.composite_masked(alpha, rgb, z, live, white_bg)
    n_culled = (~live).sum(1).to(F64)
    rel = (1. + 1e-6) ** n_culled - 1.
    assert float(rel.max()) <= 1.001e-6 * float(n_culled.max()) and float(n_culled.max()) >= 20
    w = torch.where(live, got["w"], torch.zeros_like(got["w"]))
    # (under white_bg the background term 1 - sum w moves by the weights' change as well)
    bound_rgb = rel[:, None] * ((w[..., None] * rgb).sum(1) + (w.sum(1)[:, None] if white_bg else 0.)) + 1e-15
    assert ((got["rgb"] - want[:, :3]).abs() <= bound_rgb).all()
    assert ((got["dist"] - want[:, 3]).abs() <= rel * (w * z.to(F64)).sum(1) + 1e-15).all()
    assert torch.equal(got["alpha"][~live], torch.zeros(int((~live).sum()), dtype=F64))      # a culled sample's alpha is 0
    assert torch.equal(got["rgb"][0], want[0, :3]) and torch.equal(got["dist"][0], want[0, 3])      # nothing culled: the same product
    if not dist_alpha:      # a ray without a live sample: the background
        assert torch.equal(got["rgb"][1], torch.full((3,), 1. if white_bg else 0., dtype=F64)) and float(got["dist"][1]) == 0.
    assert float((got["rgb"] - want[:, :3]).abs().max()) > 0.      # (and the two definitions do differ)


def test_the_substitute_gives_alpha_zero_and_derivative_zero():
    """E = -inf: the compositor's alpha and its derivative in the raw density are exactly 0 under softplus and ReLU, with and without
    dist_alpha -- the arithmetic of sample_alpha (csrc/nnr_device.h) on IEEE values, here in fp32 and in float64."""
    for dt in (torch.float32, F64):
        e = torch.tensor(float("-inf"), dtype=dt)
        softplus, dsoft = torch.log1p(torch.exp(e)), 1. / (1. + torch.exp(-e))
        relu, drelu = torch.clamp(e, min=0.), (e > 0).to(dt)
        for sigma, dsig in ((softplus, dsoft), (relu, drelu)):
            for delta in (None, torch.tensor(3e-2, dtype=dt), torch.tensor(1e10, dtype=dt)):
                ex = torch.exp(-sigma * (delta if delta is not None else 1.))
                alpha, dalpha = 1. - ex, (delta if delta is not None else 1.) * ex * dsig
                assert float(alpha) == 0. and float(dalpha) == 0.
    assert "0xff800000" in open(os.path.join(ROOT, "include", "nnr_frozen_sparse.h")).read()


# ------------------------------------------------------------------------------------------------------------ header and exports
def test_the_entry_points_live_in_their_own_header_under_abi_8():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "nnr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnr_frozen_sparse.h")).read(), flags=re.S)
    assert lib.nnr_abi_version() == L.ABI_VERSION == 8 and "NNR_ABI_VERSION" not in code and '#include "nnr_frozen.h"' in code
    assert L.FROZEN_SPARSE_EXPORTS == ("nnr_frozen_sparse_workspace_floats", "nnr_frozen_sparse_ws_plane", "nnr_frozen_sparse_fwd",
                                       "nnr_frozen_sparse_bwd")
    others = L.EXPORTS + L.GEOMETRY_EXPORTS + L.FUSION_EXPORTS + L.SPARSE_EXPORTS + L.REGULARISE_EXPORTS + L.FROZEN_EXPORTS
    for name in L.FROZEN_SPARSE_EXPORTS:
        assert name not in others and hasattr(lib, name) and name not in hdr
        assert name not in open(os.path.join(ROOT, "include", "nnr_frozen.h")).read() and name not in open(os.path.join(ROOT, "include", "nnr_sparse.h")).read()
    protos = dict(re.findall(r"\b(?:int|size_t|int64_t)\s+(nnr_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S))
    assert set(protos) == set(L.FROZEN_SPARSE_EXPORTS)
    for name, params in protos.items():
        assert len(getattr(lib, name).argtypes) == params.count(",") + 1, name
    assert len(lib.nnr_frozen_sparse_fwd.argtypes) == 21 and len(lib.nnr_frozen_sparse_bwd.argtypes) == 9
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert lib.nnr_frozen_sparse_fwd.argtypes[7:10] == [f32p, f32p, i32p]      # the grid's three host arrays
    assert lib.nnr_frozen_sparse_workspace_floats.restype is C.c_size_t and lib.nnr_frozen_sparse_ws_plane.restype is C.c_int64


@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("R,N", [(4, 64), (5, 130), (3, 33), (1, 1)])
def test_the_workspace_is_the_frozen_one_and_the_list_behind_it(D, R, N):
    L, lib = _lib()
    c = _cfg(R, N, D)
    s_pad = (R * N + 127) // 128 * 128
    frozen = lib.nnr_frozen_workspace_floats(C.byref(c))
    assert frozen > 0 and lib.nnr_frozen_sparse_workspace_floats(C.byref(c)) == frozen + s_pad + R + 1 + R + 32 * R
    for plane in (P_OUT4, P_Z, P_DOUT4, P_DPTS, P_DVIEW, P_XE, P_XF, P_MASK, 11, 20, 31, 40, -1, 5):      # the frozen planes, and its absences
        p0, p1 = C.c_int32(-1), C.c_int32(-1)
        assert lib.nnr_frozen_sparse_ws_plane(C.byref(c), plane, C.byref(p0)) == lib.nnr_frozen_ws_plane(C.byref(c), plane, C.byref(p1))
        assert p0.value == p1.value
    off = frozen
    for plane, size, pitch in ((L.FS_LIVE, s_pad, 1), (L.FS_RAY_OFF, R, 1), (L.FS_N_LIVE, 1, 1), (L.FS_RAY_COUNT, R, 1), (L.FS_RAY_MASK, 32 * R, 32)):
        got = C.c_int32(-1)
        assert lib.nnr_frozen_sparse_ws_plane(C.byref(c), plane, C.byref(got)) == off and got.value == pitch, plane
        off += size
    assert lib.nnr_frozen_sparse_ws_plane(C.byref(c), 105, None) == -1 and lib.nnr_frozen_sparse_ws_plane(C.byref(c), 99, None) == -1


# ------------------------------------------------------------------------------------------------------------ error returns
FWD = ("pts_o", "pts_d", "view_d", "z_lo", "z_hi", "jitter", "grid_lo", "grid_inv_step", "grid_dims", "bits", "packed", "rgb", "dist", "opt_alpha",
       "opt_z", "opt_count", "opt_live", "opt_n_live", "ws")
BWD = ("packed", "d_rgb", "d_dist", "d_pts_o", "d_pts_d", "d_view", "ws")
OPTIONAL = ("jitter", "opt_alpha", "opt_z", "opt_count", "opt_live", "opt_n_live")


def _call(which, cfg, null=(), lo=(-1., -1., -1.), inv=(8., 8., 8.), dims=(16, 16, 16), **ptrs):
    """nnr_frozen_sparse_fwd / _bwd with fake, 16-byte aligned device pointers and a real host grid -> the return code (never a launch)."""
    _, lib = _lib()
    names = FWD if which == "fwd" else BWD
    a = {k: 0x10000 * (i + 1) for i, k in enumerate(names)}
    a.update(ptrs)
    host = dict(grid_lo=(C.c_float * 3)(*lo), grid_inv_step=(C.c_float * 3)(*inv), grid_dims=(C.c_int32 * 3)(*dims))
    v = [None if k in null else host[k] if k in host else C.c_void_p(a[k]) for k in names]
    rc = getattr(lib, "nnr_frozen_sparse_" + which)(C.byref(cfg) if cfg is not None else None, *v, None)
    assert rc != OK, "a call with fake device pointers must not get as far as a launch"
    return rc


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_the_frozen_paths_refusals_apply(which):
    L, lib = _lib()
    need = L.NNR_F_TRAIN | L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    for flags in (need | L.NNR_F_BF16, L.NNR_F_TRAIN, L.NNR_F_TRAIN | L.NNR_F_SPLIT3, L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2):
        c = _cfg(4, 64, 256, flags)
        assert _call(which, c) == E_UNSUPPORTED, flags
        assert lib.nnr_frozen_sparse_workspace_floats(C.byref(c)) == 0 and lib.nnr_frozen_sparse_ws_plane(C.byref(c), L.FS_LIVE, None) == -1
    assert _call(which, _cfg(4, 64, 192)) == E_UNSUPPORTED and _call(which, _cfg(4, 1025, 256)) == E_UNSUPPORTED
    assert _call(which, _cfg(2 ** 21 + 1, 1024, 256)) == E_UNSUPPORTED      # more than 2^31 - 1 padded samples: the list holds int32
    assert _call(which, None) == E_BADCFG and lib.nnr_frozen_sparse_workspace_floats(None) == 0
    for n in (0, -1):
        assert _call(which, _cfg(n, 64, 256)) == E_BADCFG and _call(which, _cfg(4, n, 256)) == E_BADCFG
    c = _cfg(5, 130, 128, need | L.NNR_F_DIST_ALPHA | L.NNR_F_RELU_SIGMA | L.NNR_F_WHITE_BG)
    for name in (FWD if which == "fwd" else BWD):
        if name not in OPTIONAL:
            assert _call(which, c, null=(name,)) == E_BADCFG, name
    assert _call(which, c, packed=0x80008) == E_ALIGN and _call(which, c, ws=0x90008) == E_ALIGN


def test_the_sparse_paths_grid_refusals_apply():
    c = _cfg(5, 130, 128)
    assert _call("fwd", c, null=OPTIONAL, ws=0x90004) == E_ALIGN      # the optional ones may be null: such a call reaches the alignment check
    assert _call("fwd", c, dims=(16, 0, 16)) == E_BADCFG
    assert _call("fwd", c, lo=(float("nan"), 0., 0.)) == E_BADCFG and _call("fwd", c, lo=(0., float("inf"), 0.)) == E_BADCFG
    assert _call("fwd", c, inv=(1., 0., 1.)) == E_BADCFG and _call("fwd", c, inv=(1., 1., -2.)) == E_BADCFG
    assert _call("fwd", c, inv=(1., float("inf"), 1.)) == E_BADCFG
    assert _call("fwd", c, dims=(2 ** 16, 2 ** 16, 2)) == E_UNSUPPORTED      # more than 2^31 - 1 cells
    assert _call("fwd", c, dims=(32, 2 ** 16, 2 ** 16)) == E_UNSUPPORTED      # ... rows
    for name in ("bits", "opt_count", "opt_live", "opt_n_live"):
        assert _call("fwd", c, **{name: 0x70002}) == E_ALIGN, name


# ------------------------------------------------------------------------------------------------------------ the operator and the trainer
def test_occupancy_needs_a_frozen_call_and_says_so_before_any_gpu_call():
    import nnr
    from nnr import ops
    t = torch.zeros(4, 3)
    z = torch.linspace(0.0, 1.0, 32)
    kw = dict(hidden=128, dist_alpha=False, white_bg=False, relu_sigma=False)
    grid = object()
    with pytest.raises(ValueError, match="occupancy"):
        nnr.render_rays(t, t, t, z, z, None, [], [], occupancy=grid, **kw)
    with pytest.raises(ValueError, match="occupancy"):
        nnr.render_rays(t, t, t, z, z, None, [], [], frozen=False, occupancy=grid, **kw)
    with nnr.frozen_field():
        with pytest.raises(ValueError, match="occupancy"):      # frozen=False wins over the context
            nnr.render_rays(t, t, t, z, z, None, [], [], frozen=False, occupancy=grid, **kw)
    with nnr.frozen_field(occupancy=grid):
        assert ops._frozen_state.grid is grid
        with nnr.frozen_field():
            assert ops._frozen_state.grid is None      # nests: the inner block has no grid
        assert ops._frozen_state.grid is grid and ops._frozen_state.on
    assert ops._frozen_state.grid is None and ops._frozen_state.on is False


def test_trainer_pose_reads_the_occupancy_key():
    import model as mdl
    base = {"n_points": 8, "type": "nope_nerf"}
    for cfg, want in ((base, False), (dict(base, occupancy=False), False), (dict(base, occupancy=None), False), (dict(base, occupancy=True), True),
                      (dict(base, occupancy=True, frozen_field=True), True)):
        tp = mdl.Trainer_pose(None, cfg)
        assert tp.occupancy is want and tp.occupancy_grid is None and tp.occupancy_builds == 0 and tp.frozen_field is True
    with pytest.raises(ValueError, match="frozen_field"):
        mdl.Trainer_pose(None, dict(base, occupancy=True, frozen_field=False))
