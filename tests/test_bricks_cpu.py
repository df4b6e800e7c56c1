"""CPU: the density-bricks entry point of the C ABI (nnr_density_bricks, include/nnr_geometry.h, added under ABI 8) -- where it is declared and
listed, version agreement, every error return reached with fake device pointers before anything is dereferenced or launched, and the Python
wrapper's refusal of CPU weights.  (What the build script holds the kernel to: test_build_cpu.py.)"""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3
PACKED, OUT, BRICKS = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000)      # fake device addresses
INF, NAN = float("inf"), float("nan")


def _lib():
    from nnr import lib as L
    return L, L.load()


def _call(n_bricks=3, n_rays=None, n_samples=1, hidden=256, flags=None, origin=(0., 0., 0.), step=(1., 1., 1.), bricks=BRICKS, packed=PACKED,
          out=OUT, null=()):
    L, lib = _lib()
    flags = (L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2) if flags is None else flags
    cfg = L.Cfg(512 * n_bricks if n_rays is None else n_rays, n_samples, hidden, flags)
    o3, s3 = (C.c_float * 3)(*origin), (C.c_float * 3)(*step)
    args = dict(cfg=C.byref(cfg), origin=o3, step=s3, bricks=bricks, packed=packed, out=out)
    for n in null:
        args[n] = None
    return lib.nnr_density_bricks(args["cfg"], args["origin"], args["step"], args["bricks"], n_bricks, args["packed"], args["out"], None)


def test_abi_version_stays_8_and_the_entry_point_lives_in_the_geometry_header():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "nnr.h")).read()
    geo = open(os.path.join(ROOT, "include", "nnr_geometry.h")).read()
    assert lib.nnr_abi_version() == L.ABI_VERSION == int(re.search(r"#define NNR_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert "NNR_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", geo, flags=re.S)                 # one version, nnr.h's
    assert re.search(r"\bint nnr_density_bricks\(", geo) and '#include "nnr.h"' in geo
    assert not re.search(r"nnr_density_bricks\s*\(", hdr)                                     # nnr.h's set of functions is EXPORTS, as before
    assert L.GEOMETRY_EXPORTS == ("nnr_density_bricks",) and "nnr_density_bricks" not in L.EXPORTS and len(L.EXPORTS) == 50
    assert hasattr(lib, "nnr_density_bricks") and len(lib.nnr_density_bricks.argtypes) == 8
    # the header's prototypes are exactly GEOMETRY_EXPORTS, with the binding's arity
    protos = dict(re.findall(r"\bint\s+(nnr_\w+)\s*\(([^;{]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", geo, flags=re.S), flags=re.S))
    assert set(protos) == set(L.GEOMETRY_EXPORTS)
    for name, params in protos.items():
        assert len(getattr(lib, name).argtypes) == params.count(",") + 1, name


@pytest.mark.parametrize("name", ["cfg", "origin", "step", "bricks", "packed", "out"])
def test_null_pointers_are_rejected(name):
    assert _call(null=(name,)) == E_BADCFG


@pytest.mark.parametrize("n_bricks", [0, -1, -2 ** 31])
def test_a_brick_count_below_one_is_rejected(n_bricks):
    assert _call(n_bricks=n_bricks, n_rays=512) == E_BADCFG


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("bad", [INF, -INF, NAN])
def test_non_finite_origin_or_step_is_rejected(axis, bad):
    v = [0.5, 0.5, 0.5]
    v[axis] = bad
    assert _call(origin=v) == E_BADCFG
    assert _call(step=v) == E_BADCFG


@pytest.mark.parametrize("n_rays", [0, 3, 1535, 1537, -1536, 512])
def test_n_rays_must_be_the_voxel_count(n_rays):
    assert _call(n_bricks=3, n_rays=n_rays) == E_BADCFG
    assert _call(n_bricks=3, n_rays=1536, packed=C.c_void_p(0x10004)) == E_ALIGN      # (1536 itself passes this check)


@pytest.mark.parametrize("n_samples", [0, 2, -1])
def test_n_samples_must_be_one(n_samples):
    assert _call(n_samples=n_samples) == E_BADCFG


@pytest.mark.parametrize("n_bricks", [2 ** 22, 2 ** 22 + 1, 2 ** 31 - 1])
def test_more_than_int32_voxels_is_unsupported(n_bricks):
    assert _call(n_bricks=n_bricks, n_rays=2 ** 31 - 1) == E_UNSUPPORTED


def test_the_largest_brick_list_passes_the_size_check():
    assert _call(n_bricks=2 ** 22 - 1, packed=C.c_void_p(0x10004)) == E_ALIGN           # 512 (2^22 - 1) = 2^31 - 512 voxels


def test_hidden_width_is_checked():
    assert _call(hidden=192) == E_UNSUPPORTED
    assert _call(hidden=64) == E_UNSUPPORTED
    assert _call(hidden=128, out=C.c_void_p(0x20002)) == E_ALIGN


def test_flags_are_checked():
    """The kernel exists in the two-term fp16 arithmetic only, forward-only; the rendering switches do not matter to the raw density and are
    accepted (they reach the alignment check behind the flag check)."""
    L, _ = _lib()
    s2 = L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    for flags in (0, L.NNR_F_SPLIT3, L.NNR_F_SPLIT2, s2 | L.NNR_F_TRAIN, s2 | L.NNR_F_BF16, L.NNR_F_BF16):
        assert _call(flags=flags) == E_UNSUPPORTED, flags
    for flags in (s2, s2 | L.NNR_F_DIST_ALPHA, s2 | L.NNR_F_RELU_SIGMA, s2 | L.NNR_F_WHITE_BG):
        assert _call(flags=flags, packed=C.c_void_p(0x10008)) == E_ALIGN, flags


def test_misaligned_pointers_are_rejected():
    for addr in (0x10001, 0x10002, 0x10004, 0x10008, 0x1000c):      # packed: the kernel's 16-byte accesses
        assert _call(packed=C.c_void_p(addr)) == E_ALIGN, hex(addr)
    for addr in (0x20001, 0x20002, 0x20003):                        # out: one float per voxel
        assert _call(out=C.c_void_p(addr)) == E_ALIGN, hex(addr)
    for addr in (0x30001, 0x30002, 0x30003):                        # bricks: int32 coordinates
        assert _call(bricks=C.c_void_p(addr)) == E_ALIGN, hex(addr)
    for addr in (0x30004, 0x30008, 0x3000c):                        # ... and no more than that: these reach the next check
        assert _call(bricks=C.c_void_p(addr), out=C.c_void_p(0x20001)) == E_ALIGN and _call(bricks=C.c_void_p(addr), n_rays=1) == E_BADCFG


def test_ops_density_bricks_raises_on_cpu_weights():
    import model as mdl
    from nnr import ops
    net = mdl.OfficialStaticNerf({'model': {'hidden_dim': 128, 'pos_enc_levels': 10, 'dir_enc_levels': 4, 'occ_activation': 'softplus'},
                                  'rendering': {'white_background': False, 'dist_alpha': False}})
    with pytest.raises(RuntimeError):
        ops.density_bricks((0., 0., 0.), (.1, .1, .1), torch.zeros(2, 3, dtype=torch.int32), net.weights(), net.biases(), hidden=128)
