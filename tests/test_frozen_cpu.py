"""CPU: the frozen-field render (include/nnr_frozen.h) without a GPU -- where its entry points are declared and
listed, the size and the planes of the frozen workspace against the plane list written out here, every error return reached with fake
device pointers, and the one argument check of the Python operator that needs no device."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))

OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3
# plane ids of nnr_ws_plane (nnr_layout.h) and the floats per sample of the eight planes the frozen workspace holds, in its order
P_OUT4, P_Z, P_DOUT4, P_DPTS, P_DVIEW, P_XE, P_XH1, P_XF, P_XG, P_MASK, P_DH1, P_DG = 0, 1, 2, 3, 4, 10, 11, 19, 20, 25, 31, 40


def _widths(D):
    return [(P_OUT4, 4), (P_Z, 1), (P_DOUT4, 4), (P_DPTS, 4), (P_DVIEW, 4), (P_XE, 64), (P_XF, 32), (P_MASK, 18 * D // 64)]


ABSENT = list(range(P_XH1, P_XH1 + 8)) + [P_XG] + list(range(P_DH1, P_DH1 + 8)) + [P_DG]
SHAPES = [(4, 64), (5, 130), (3, 33)]


def _lib():
    from nnr import lib as L
    return L, L.load()


def _cfg(R, N, D, flags=None):
    L, _ = _lib()
    return L.Cfg(R, N, D, (L.NNR_F_TRAIN | L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2) if flags is None else flags)


# ------------------------------------------------------------------------------------------------------------ header and exports
def test_the_entry_points_live_in_the_frozen_header_under_abi_8():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "nnr.h")).read()
    others = [open(os.path.join(ROOT, "include", n)).read() for n in ("nnr_geometry.h", "nnr_fusion.h", "nnr_sparse.h", "nnr_regularise.h")]
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnr_frozen.h")).read(), flags=re.S)
    assert lib.nnr_abi_version() == L.ABI_VERSION == int(re.search(r"#define NNR_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert "NNR_ABI_VERSION" not in code and '#include "nnr.h"' in code
    assert L.FROZEN_EXPORTS == ("nnr_frozen_workspace_floats", "nnr_frozen_ws_plane", "nnr_frozen_fwd", "nnr_frozen_bwd")
    for name in L.FROZEN_EXPORTS:
        assert name not in L.EXPORTS + L.GEOMETRY_EXPORTS + L.FUSION_EXPORTS + L.SPARSE_EXPORTS + L.REGULARISE_EXPORTS and hasattr(lib, name)
        assert name not in hdr and all(name not in o for o in others)
    protos = dict(re.findall(r"\b(?:int|size_t|int64_t)\s+(nnr_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S))
    assert set(protos) == set(L.FROZEN_EXPORTS)
    for name, params in protos.items():
        assert len(getattr(lib, name).argtypes) == params.count(",") + 1, name
    assert len(lib.nnr_frozen_fwd.argtypes) == 14 and len(lib.nnr_frozen_bwd.argtypes) == 9


# ------------------------------------------------------------------------------------------------------------ sizes and planes
@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("R,N", SHAPES)
def test_the_frozen_workspace_is_its_eight_planes_and_nothing_else(D, R, N):
    _, lib = _lib()
    c = _cfg(R, N, D)
    s_pad = (R * N + 127) // 128 * 128
    per_sample = 4 + 1 + 4 + 4 + 4 + 64 + 32 + 18 * D // 64
    assert per_sample == {256: 185, 128: 149}[D]
    total = lib.nnr_frozen_workspace_floats(C.byref(c))
    assert total == per_sample * s_pad      # no maxima tail, no slots, no merged-matrix scratch
    full = lib.nnr_workspace_floats(C.byref(c))
    assert 0 < 10 * total < full
    off = 0
    for plane, width in _widths(D):      # the planes lie in this order, back to back
        pitch = C.c_int32(-1)
        assert lib.nnr_frozen_ws_plane(C.byref(c), plane, C.byref(pitch)) == off and pitch.value == width, plane
        assert lib.nnr_frozen_ws_plane(C.byref(c), plane, None) == off
        assert (4 * off) % 16 == 0
        off += width * s_pad
    assert off == total
    held = {p for p, _ in _widths(D)}
    for plane in ABSENT + [-1, 5, 21, 22, 41, 47, 1000]:
        assert plane not in held and lib.nnr_frozen_ws_plane(C.byref(c), plane, None) == -1, plane


def test_the_plane_list_gives_a_24th_and_a_15th_of_the_training_planes():
    """The ratio the issue quotes (1 / 24 at D = 256, 1 / 15 at D = 128), on the plane lists alone: the training workspace's planes per sample
    are 4 + 1 + 4 + 4 + 4 + 64 + 8 D + 32 + D / 2 + 18 D / 64 + 8 D + D / 2 (nnr_layout.h)."""
    for D, want in ((256, 24), (128, 15)):
        train = 4 + 1 + 4 + 4 + 4 + 64 + 8 * D + 32 + D // 2 + 18 * D // 64 + 8 * D + D // 2
        frozen = sum(w for _, w in _widths(D))
        assert train // frozen == want      # (24.5 and 15.6)
        _, lib = _lib()
        c = _cfg(1024, 128, D)
        assert lib.nnr_workspace_floats(C.byref(c)) >= train * 1024 * 128 and lib.nnr_frozen_workspace_floats(C.byref(c)) == frozen * 1024 * 128


# ------------------------------------------------------------------------------------------------------------ error returns
FWD = ("pts_o", "pts_d", "view_d", "z_lo", "z_hi", "jitter", "packed", "rgb", "dist", "opt_alpha", "opt_z", "ws")
BWD = ("packed", "d_rgb", "d_dist", "d_pts_o", "d_pts_d", "d_view", "ws")


def _call(which, cfg, null=(), **ptrs):
    """nnr_frozen_fwd / nnr_frozen_bwd with fake, 16-byte aligned device pointers -> the return code (never a launch: asserted)."""
    _, lib = _lib()
    names = FWD if which == "fwd" else BWD
    a = {k: 0x10000 * (i + 1) for i, k in enumerate(names)}
    a.update(ptrs)
    v = [None if k in null else C.c_void_p(a[k]) for k in names]
    rc = getattr(lib, "nnr_frozen_" + which)(C.byref(cfg) if cfg is not None else None, *v, None)
    assert rc != OK, "a call with fake device pointers must not get as far as a launch"
    return rc


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_a_cfg_without_frozen_kernels_is_unsupported(which):
    L, lib = _lib()
    need = L.NNR_F_TRAIN | L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    for flags in (need | L.NNR_F_BF16, L.NNR_F_TRAIN | L.NNR_F_BF16, L.NNR_F_TRAIN, L.NNR_F_TRAIN | L.NNR_F_SPLIT3, L.NNR_F_TRAIN | L.NNR_F_SPLIT2,
                  L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2):
        c = _cfg(4, 64, 256, flags)
        assert _call(which, c) == E_UNSUPPORTED, flags
        assert lib.nnr_frozen_workspace_floats(C.byref(c)) == 0 and lib.nnr_frozen_ws_plane(C.byref(c), P_OUT4, None) == -1
    assert _call(which, _cfg(4, 64, 192)) == E_UNSUPPORTED          # another width
    assert _call(which, _cfg(4, 1025, 256)) == E_UNSUPPORTED        # more samples than a training cfg may have
    # the rendering switches are honoured, not refused: such a call gets as far as the alignment check
    c = _cfg(4, 64, 256, need | L.NNR_F_DIST_ALPHA | L.NNR_F_RELU_SIGMA | L.NNR_F_WHITE_BG)
    assert _call(which, c, packed=0x80008) == E_ALIGN


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_null_pointers_and_sizes_below_one_are_a_bad_cfg(which):
    _, lib = _lib()
    assert _call(which, None) == E_BADCFG
    assert lib.nnr_frozen_workspace_floats(None) == 0 and lib.nnr_frozen_ws_plane(None, P_OUT4, None) == -1
    for n in (0, -1):
        assert _call(which, _cfg(n, 64, 256)) == E_BADCFG and _call(which, _cfg(4, n, 256)) == E_BADCFG
    c = _cfg(5, 130, 128)
    optional = ("jitter", "opt_alpha", "opt_z")
    for name in (FWD if which == "fwd" else BWD):
        if name not in optional:
            assert _call(which, c, null=(name,)) == E_BADCFG, name
    if which == "fwd":      # the optional ones may be null: such a call reaches the alignment check
        assert _call(which, c, null=optional, ws=0x90004) == E_ALIGN
    assert _call(which, c, packed=0x80008) == E_ALIGN and _call(which, c, ws=0x90008) == E_ALIGN


# ------------------------------------------------------------------------------------------------------------ the operator
def test_frozen_takes_no_ray_distortion_and_says_so_before_any_gpu_call():
    """CPU tensors: any step past the argument check would raise RuntimeError (no CPU render path), not ValueError."""
    import nnr
    t = torch.zeros(4, 3)
    z = torch.linspace(0.0, 1.0, 32)
    kw = dict(hidden=128, dist_alpha=False, white_bg=False, relu_sigma=False)
    with pytest.raises(ValueError, match="ray_distortion"):
        nnr.render_rays(t, t, t, z, z, None, [], [], frozen=True, ray_distortion=(0.0, 1.0), **kw)
    with nnr.frozen_field():
        with pytest.raises(ValueError, match="ray_distortion"):
            nnr.render_rays(t, t, t, z, z, None, [], [], ray_distortion=(0.0, 1.0), **kw)
        with nnr.frozen_field():
            pass
        with pytest.raises(ValueError, match="ray_distortion"):      # still on after a nested block ended
            nnr.render_rays(t, t, t, z, z, None, [], [], ray_distortion=(0.0, 1.0), **kw)
        with pytest.raises(RuntimeError):      # frozen=False wins over the context: today's path, which refuses CPU tensors
            nnr.render_rays(t, t, t, z, z, None, [torch.zeros(1)] * 12, [torch.zeros(1)] * 12, frozen=False, ray_distortion=(0.0, 1.0), **kw)
    with pytest.raises(RuntimeError):          # and the context is off again behind the block
        nnr.render_rays(t, t, t, z, z, None, [torch.zeros(1)] * 12, [torch.zeros(1)] * 12, ray_distortion=(0.0, 1.0), **kw)


def test_the_context_is_per_thread():
    import threading
    from nnr import ops
    seen = {}
    with ops.frozen_field():
        th = threading.Thread(target=lambda: seen.setdefault("other", getattr(ops._frozen_state, "on", False)))
        th.start()
        th.join()
        seen["here"] = ops._frozen_state.on
    assert seen == {"other": False, "here": True} and ops._frozen_state.on is False


def test_trainer_pose_reads_the_key():
    import model as mdl
    base = {"n_points": 8, "type": "nope_nerf"}
    assert mdl.Trainer_pose(None, base).frozen_field is True
    assert mdl.Trainer_pose(None, dict(base, frozen_field=True)).frozen_field is True
    assert mdl.Trainer_pose(None, dict(base, frozen_field=False)).frozen_field is False
