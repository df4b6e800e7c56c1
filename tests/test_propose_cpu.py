"""CPU: the fused proposal entry point of the C ABI (nnr_propose, added under ABI 8) -- version agreement, argument validation before any
device work, the Python wrapper's refusal of CPU tensors -- and the `rendering.proposal` key of the Renderer where no GPU is needed."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3


def _lib():
    from nnr import lib as L
    return L, L.load()


def test_abi_version_stays_8_and_the_entry_point_is_everywhere():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "nnr.h")).read()
    assert lib.nnr_abi_version() == L.ABI_VERSION == int(re.search(r"#define NNR_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert "nnr_propose" in L.EXPORTS and re.search(r"\bint nnr_propose\(", hdr) and hasattr(lib, "nnr_propose")
    assert len(lib.nnr_propose.argtypes) == 14


# fake device addresses: every call below must be rejected before anything is dereferenced or launched
NAMES = ("pts_o", "pts_d", "z_lo", "z_hi", "jitter", "xi", "packed", "z_all", "opt_alpha", "opt_z", "opt_fine")
FAKE = {n: C.c_void_p(0x10000 + 0x1000 * i) for i, n in enumerate(NAMES)}
REQUIRED = ("pts_o", "pts_d", "z_lo", "z_hi", "packed", "z_all")
WIDE = ("packed", "z_all")      # the kernel's 16-byte accesses


def _call(lib, R, Cn, F, hidden=256, flags=None, **over):
    L, _ = _lib()
    flags = (L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2) if flags is None else flags
    cfg = L.Cfg(R, Cn, hidden, flags)
    p = dict(FAKE, **over)
    return lib.nnr_propose(C.byref(cfg), F, *[p[n] for n in NAMES], None)


@pytest.mark.parametrize("R,Cn,F,code", [(16, 2, 8, E_BADCFG), (16, 0, 8, E_BADCFG), (16, -1, 8, E_BADCFG),      # C < 3
                                         (16, 64, 0, E_BADCFG), (16, 64, -3, E_BADCFG),                          # F < 1
                                         (0, 64, 128, E_BADCFG), (-1, 64, 128, E_BADCFG),                        # no rays
                                         (16, 64, 961, E_UNSUPPORTED), (16, 256, 769, E_UNSUPPORTED),            # C + F > 1024
                                         (16, 257, 8, E_UNSUPPORTED), (16, 1024, 1, E_UNSUPPORTED),              # C > 256: the LDS staging
                                         (16, 2 ** 30, 2 ** 30, E_UNSUPPORTED)])
def test_sizes_are_rejected(R, Cn, F, code):
    _, lib = _lib()
    assert _call(lib, R, Cn, F) == code


def test_hidden_width_is_checked():
    _, lib = _lib()
    assert _call(lib, 16, 64, 128, hidden=192) == E_UNSUPPORTED
    assert lib.nnr_propose(None, 8, *[FAKE[n] for n in NAMES], None) == E_BADCFG


def test_flags_are_checked():
    """The kernel exists in the two-term fp16 arithmetic only, forward-only; the rendering switches of the density are accepted (they reach
    the alignment check behind the flag check)."""
    L, lib = _lib()
    s2 = L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    for flags in (0, L.NNR_F_SPLIT3, L.NNR_F_SPLIT2, s2 | L.NNR_F_TRAIN, s2 | L.NNR_F_BF16, L.NNR_F_BF16):
        assert _call(lib, 16, 64, 128, flags=flags) == E_UNSUPPORTED, flags
    for flags in (s2, s2 | L.NNR_F_DIST_ALPHA, s2 | L.NNR_F_RELU_SIGMA, s2 | L.NNR_F_WHITE_BG):
        assert _call(lib, 16, 64, 128, flags=flags, packed=C.c_void_p(0x20004)) == E_ALIGN, flags


def test_null_pointers_are_rejected():
    _, lib = _lib()
    for name in REQUIRED:
        assert _call(lib, 16, 64, 128, **{name: None}) == E_BADCFG, name


def test_misaligned_pointers_are_rejected():
    _, lib = _lib()
    for name in NAMES:
        assert _call(lib, 16, 64, 128, **{name: C.c_void_p(0x20002)}) == E_ALIGN, name
    for name in WIDE:
        assert _call(lib, 16, 64, 128, **{name: C.c_void_p(0x20004)}) == E_ALIGN, name


def test_ops_propose_raises_on_cpu_tensors():
    import model as mdl
    from nnr import ops
    from test_host_logic import make_cfg
    net = mdl.OfficialStaticNerf(make_cfg(128))
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    z = torch.linspace(0.1, 1.0, 16)
    with pytest.raises(RuntimeError):
        ops.propose(o, d, z, z, None, None, 8, net.weights(), net.biases(), hidden=128, dist_alpha=False, relu_sigma=False)


def _cpu_render(**rendering):
    import model as mdl
    from test_host_logic import make_cfg
    cfg = make_cfg(128, **rendering)
    torch.manual_seed(4)
    renderer = mdl.Renderer(mdl.OfficialStaticNerf(cfg), cfg['rendering'], device='cpu')
    g = torch.Generator().manual_seed(1)
    pixels, depth = torch.rand(1, 8, 2, generator=g) * 2 - 1, 1 + torch.rand(1, 8, 1, generator=g)
    eye = torch.eye(4).unsqueeze(0)
    return renderer, (pixels, depth, eye, eye, eye)


def test_renderer_rejects_an_unknown_proposal():
    """Checked before the CPU refusal of num_fine > 0: a typo in the key is reported as such wherever the render runs."""
    renderer, args = _cpu_render(num_fine=16, proposal='bogus')
    with pytest.raises(ValueError, match="proposal"):
        renderer.nope_nerf(*args, add_noise=False)


@pytest.mark.parametrize("proposal", ["render", "density"])
def test_cpu_refusal_of_num_fine_stays(proposal):
    renderer, args = _cpu_render(num_fine=16, proposal=proposal)
    with pytest.raises(NotImplementedError, match="num_fine"):
        renderer.nope_nerf(*args, add_noise=False)


def _try_render(renderer, args):
    """The CPU render where it exists (there is no CPU fallback for the HIP render path): its outputs, or the exception it raises."""
    try:
        out = renderer.nope_nerf(*args, add_noise=False)
    except Exception as e:      # noqa: BLE001 -- compared by type and text below
        return type(e), str(e)
    return out['rgb'].detach().clone(), out['dist_dense'].detach().clone()


@pytest.mark.parametrize("extra", [dict(num_fine=0, proposal='density'), dict(proposal='density'), dict(num_fine=0, proposal='bogus')])
def test_proposal_is_ignored_without_num_fine(extra):
    """With num_fine 0 or absent the key is not even looked at: a CPU call behaves exactly as with the key absent -- where the render path has
    no CPU fallback that is the same refusal, and in particular no ValueError for 'bogus'.  The bitwise comparison of the renders is the GPU
    test tests/test_gpu_propose.py::test_proposal_is_ignored_without_num_fine."""
    plain = _try_render(*_cpu_render())
    keyed = _try_render(*_cpu_render(**extra))
    assert type(plain) is type(keyed)
    for a, b in zip(plain, keyed):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
