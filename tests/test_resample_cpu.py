"""CPU: the hierarchical-sampling entry point of the C ABI (nnr_resample, ABI 8) -- version agreement, argument validation before any
device work, the Python wrapper's refusal of CPU tensors -- and the properties of the CPU restatement tests/resample_ref.py that the GPU
tests lean on."""
import ctypes as C
import os
import re

import pytest
import torch

import resample_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3


def _lib():
    from nnr import lib as L
    return L, L.load()


def test_abi_version_is_8_everywhere():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "nnr.h")).read()
    assert lib.nnr_abi_version() == 8
    assert L.ABI_VERSION == 8
    assert int(re.search(r"#define NNR_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert "nnr_resample" in L.EXPORTS and "nnr_resample" in hdr and hasattr(lib, "nnr_resample")


# fake device addresses: every call below must be rejected before anything is dereferenced or launched
A, B, X, Z, Fp = (C.c_void_p(0x10000 + 0x1000 * i) for i in range(5))


def _call(lib, R, Cn, F, alpha=A, z=B, xi=X, z_all=Z, fine=Fp):
    return lib.nnr_resample(R, Cn, F, alpha, z, xi, z_all, fine, None)


@pytest.mark.parametrize("R,Cn,F,code", [(16, 2, 8, E_BADCFG), (16, 0, 8, E_BADCFG), (16, -1, 8, E_BADCFG),      # C < 3
                                         (16, 64, 0, E_BADCFG), (16, 64, -3, E_BADCFG),                          # F < 1
                                         (0, 64, 128, E_BADCFG), (-1, 64, 128, E_BADCFG),                        # no rays
                                         (16, 64, 961, E_UNSUPPORTED), (16, 1024, 1, E_UNSUPPORTED),             # C + F > 1024
                                         (16, 2 ** 30, 2 ** 30, E_UNSUPPORTED)])
def test_sizes_are_rejected(R, Cn, F, code):
    _, lib = _lib()
    assert _call(lib, R, Cn, F) == code


def test_null_pointers_are_rejected():
    _, lib = _lib()
    assert _call(lib, 16, 64, 128, alpha=None) == E_BADCFG
    assert _call(lib, 16, 64, 128, z=None) == E_BADCFG
    assert _call(lib, 16, 64, 128, z_all=None) == E_BADCFG


def test_misaligned_pointers_are_rejected():
    _, lib = _lib()
    off = C.c_void_p(0x20004)
    for name in ("alpha", "z", "xi", "z_all", "fine"):
        assert _call(lib, 16, 64, 128, **{name: off}) == E_ALIGN, name


def test_ops_resample_raises_on_cpu_tensors():
    from nnr import ops
    a, z = rr.make_inputs(4, 16, seed=0)
    with pytest.raises(RuntimeError):
        ops.resample(a, z, None, 8)


def test_renderer_with_num_fine_refuses_cpu_tensors():
    """A CPU render with rendering.num_fine > 0 says what is missing instead of failing deep inside the operators."""
    import model as mdl
    from test_host_logic import make_cfg
    cfg = make_cfg(128, num_fine=16)
    renderer = mdl.Renderer(mdl.OfficialStaticNerf(cfg), cfg['rendering'], device='cpu')
    pixels, depth = torch.zeros(1, 8, 2), torch.ones(1, 8, 1)
    eye = torch.eye(4).unsqueeze(0)
    with pytest.raises(NotImplementedError, match="num_fine"):
        renderer.nope_nerf(pixels, depth, eye, eye, eye, add_noise=False)


SHAPES = [(64, 128), (128, 64), (32, 992), (3, 1), (16, 5)]


@pytest.mark.parametrize("Cn,F", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restatement_is_sorted_and_is_the_union(Cn, F, dtype):
    R = 257
    a, z = rr.make_inputs(R, Cn, seed=Cn * 1000 + F)
    xi = torch.rand(R, F, generator=torch.Generator().manual_seed(5))
    z_all, fine = rr.resample_ref(a, z, xi, F, dtype)
    assert z_all.shape == (R, Cn + F) and fine.shape == (R, F)
    assert bool((z_all[:, 1:] >= z_all[:, :-1]).all())
    assert bool((fine[:, 1:] >= fine[:, :-1]).all())
    union = torch.sort(torch.cat([z.to(dtype), fine], dim=1), dim=1).values
    assert torch.equal(union, z_all)      # bitwise: the merge moves values, it computes none
    # coarse before fine on ties: every coarse depth sits at its own index + the number of fine samples strictly below it
    pos = torch.arange(Cn).unsqueeze(0) + (fine.unsqueeze(1) < z.to(dtype).unsqueeze(2)).sum(dim=2)
    assert torch.equal(z_all.gather(1, pos), z.to(dtype))
    # samples stay inside the edges
    m, _ = rr.parts(a, z, dtype)
    assert bool((fine >= m[:, :1]).all()) and bool((fine <= m[:, -1:]).all())


@pytest.mark.parametrize("Cn,F", SHAPES)
def test_restatement_fp32_and_fp64_agree_in_cdf_space(Cn, F):
    """Positions are ill-conditioned where a bin holds only the 1e-5 floor, so the two precisions are compared where they are not: the
    fp64 CDF at every sample against its u.  fp64 inverts it to rounding; fp32 within the definition's own slack (the `den` guard lets
    (u - cdf_below)(1 - den) < 1e-5 through) plus fp32 rounding of the CDF and of the depth -- 3e-5 is the bound the GPU test uses."""
    R = 1023
    a, z = rr.make_inputs(R, Cn, seed=Cn * 1000 + F)
    xi = torch.rand(R, F, generator=torch.Generator().manual_seed(6))
    u = rr.u_of(xi, R, F)
    _, s64 = rr.resample_ref(a, z, xi, F, torch.float64)
    _, s32 = rr.resample_ref(a, z, xi, F, torch.float32)
    d64 = float(rr.cdf_distance(a, z, s64, u).max())
    d32 = float(rr.cdf_distance(a, z, s32, u).max())
    print("C=%d F=%d: CDF distance fp64 %.2e, fp32 %.2e; z median |fp32 - fp64| %.2e" % (Cn, F, d64, d32, float((s32.double() - s64).abs().median())))
    assert d64 <= 1.1e-5      # the guard's slack alone; everything else is 1e-15
    assert d32 <= 3e-5
    assert float((s32.double() - s64).abs().median()) <= 1e-6


def test_restatement_nan_poisons_its_ray_only():
    a, z = rr.make_inputs(8, 16, seed=1)
    a[3, 5] = float('nan')
    z[6, 0] = float('nan')
    z_all, fine = rr.resample_ref(a, z, None, 8, torch.float32)
    bad = torch.isnan(z_all).all(dim=1)
    assert bad.tolist() == [False, False, False, True, False, False, True, False]
    assert not torch.isnan(z_all[~bad]).any() and torch.isnan(fine[bad]).all()
