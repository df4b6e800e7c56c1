"""CPU: the ray-distortion regulariser without a GPU -- where its two entry points are declared and listed, every error
return reached with fake device pointers and host-side outputs that must stay untouched, the wrappers' refusal of CPU tensors
(the build's scratch entries: test_build_cpu.py), and the float64 reference of tests/ray_distortion_ref.py against itself: the O(N) prefix form is the pairwise definition and
the closed-form gradient the backward kernel evaluates is autograd's."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ray_distortion_ref as RD      # noqa: E402

OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3
INF, NAN = float("inf"), float("nan")
SENTINEL = 0x7fc0beef
FLAG_SETS = [(False, False), (True, False), (False, True), (True, True)]      # (dist_alpha, relu_sigma)


def _lib():
    from nnr import lib as L
    return L, L.load()


# ------------------------------------------------------------------------------------------------------------ header and exports
def test_the_entry_points_live_in_the_regularise_header_under_abi_8():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "nnr.h")).read()
    others = [open(os.path.join(ROOT, "include", n)).read() for n in ("nnr_geometry.h", "nnr_fusion.h", "nnr_sparse.h")]
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnr_regularise.h")).read(), flags=re.S)
    assert lib.nnr_abi_version() == L.ABI_VERSION == int(re.search(r"#define NNR_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert "NNR_ABI_VERSION" not in code and '#include "nnr.h"' in code
    assert L.REGULARISE_EXPORTS == ("nnr_ray_distortion_fwd", "nnr_ray_distortion_bwd")
    assert L.SPARSE_EXPORTS == ("nnr_render_sparse",)
    assert L.FUSION_EXPORTS == ("nnr_render_depth", "nnr_tsdf_integrate")
    assert L.GEOMETRY_EXPORTS == ("nnr_density_bricks",) and len(L.EXPORTS) == 50
    for name in L.REGULARISE_EXPORTS:
        assert name not in L.EXPORTS + L.GEOMETRY_EXPORTS + L.FUSION_EXPORTS + L.SPARSE_EXPORTS and hasattr(lib, name)
        assert name not in hdr and all(name not in o for o in others)
    protos = dict(re.findall(r"\bint\s+(nnr_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S))
    assert set(protos) == set(L.REGULARISE_EXPORTS)
    for name, params in protos.items():
        assert len(getattr(lib, name).argtypes) == params.count(",") + 1, name
    assert len(lib.nnr_ray_distortion_fwd.argtypes) == 8 and len(lib.nnr_ray_distortion_bwd.argtypes) == 11


# ------------------------------------------------------------------------------------------------------------ error returns
PTRS = dict(raw=0x10000, z=0x20000, g=0x30000)


def _call(which, n_rays=5, n_samples=64, hidden=256, flags=0, cfg=True, raw_stride=1, d_raw_stride=1, s_near=0.01, s_inv=0.1, accumulate=0,
          null=(), off=0, **ptrs):
    """nnr_ray_distortion_fwd / _bwd with fake device inputs and a HOST buffer full of a sentinel as the output -> the return code; asserts
    that no output word changed.  null: names passed as NULL ("out": the output); off: bytes to misalign the output by."""
    L, lib = _lib()
    c = L.Cfg(n_rays, n_samples, hidden, flags)
    a = dict(PTRS)
    a.update(ptrs)
    v = {k: (None if (x is None or k in null) else C.c_void_p(x)) for k, x in a.items()}
    buf = np.full(64, SENTINEL, dtype=np.int32)
    out = None if "out" in null else C.c_void_p(buf.ctypes.data + 64 + off)
    cp = C.byref(c) if cfg else None
    if which == "fwd":
        rc = lib.nnr_ray_distortion_fwd(cp, v["raw"], raw_stride, v["z"], s_near, s_inv, out, None)
    else:
        rc = lib.nnr_ray_distortion_bwd(cp, v["raw"], raw_stride, v["z"], s_near, s_inv, v["g"], out, d_raw_stride, accumulate, None)
    assert rc != OK, "a call with fake device pointers must not get as far as a launch"
    assert (buf == SENTINEL).all()
    return rc


BOTH = pytest.mark.parametrize("which", ["fwd", "bwd"])
MISALIGNED = dict(raw=0x10002)      # what turns an otherwise valid call into NNR_E_ALIGN: the last check before a launch


@BOTH
def test_null_pointers_sizes_and_strides_below_one_are_bad(which):
    assert _call(which, cfg=False) == E_BADCFG
    for name in ("raw", "z", "out") + (("g",) if which == "bwd" else ()):
        assert _call(which, null=(name,)) == E_BADCFG, name
    for n in (0, -1, -2 ** 31):
        assert _call(which, n_rays=n) == E_BADCFG and _call(which, n_samples=n) == E_BADCFG and _call(which, raw_stride=n) == E_BADCFG
        if which == "bwd":
            assert _call(which, d_raw_stride=n) == E_BADCFG
    # the smallest sizes, any stride and either accumulate value pass these checks
    assert _call(which, n_rays=1, n_samples=1, **MISALIGNED) == E_ALIGN
    assert _call(which, raw_stride=4, d_raw_stride=7, accumulate=1, **MISALIGNED) == E_ALIGN
    assert _call(which, raw_stride=2 ** 31 - 1, accumulate=-5, **MISALIGNED) == E_ALIGN


@BOTH
def test_the_depth_range_must_be_finite_and_its_inverse_positive(which):
    for bad in (INF, -INF, NAN):
        assert _call(which, s_near=bad) == E_BADCFG and _call(which, s_inv=bad) == E_BADCFG
    for s in (0.0, -0.0, -1e-3, -4.0):
        assert _call(which, s_inv=s) == E_BADCFG
    assert _call(which, s_near=-1e30, s_inv=1e-30, **MISALIGNED) == E_ALIGN
    assert _call(which, s_near=0.0, s_inv=1e30, **MISALIGNED) == E_ALIGN


@BOTH
def test_more_than_1024_samples_are_unsupported_and_other_flags_and_widths_ignored(which):
    L, _ = _lib()
    assert _call(which, n_samples=1025) == E_UNSUPPORTED and _call(which, n_samples=2 ** 31 - 1) == E_UNSUPPORTED
    assert _call(which, n_samples=1024, **MISALIGNED) == E_ALIGN
    every = L.NNR_F_DIST_ALPHA | L.NNR_F_WHITE_BG | L.NNR_F_RELU_SIGMA | L.NNR_F_TRAIN | L.NNR_F_BF16 | L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    for flags in (0, every, L.NNR_F_BF16 | L.NNR_F_TRAIN, L.NNR_F_SPLIT3, L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2 | L.NNR_F_TRAIN):
        for hidden in (0, 64, 128, 256, -1):
            assert _call(which, flags=flags, hidden=hidden, **MISALIGNED) == E_ALIGN, (flags, hidden)
    # a bad value beats an unsupported one, an unsupported one a misaligned one
    assert _call(which, n_samples=1025, s_inv=0.0) == E_BADCFG and _call(which, n_samples=1025, **MISALIGNED) == E_UNSUPPORTED


@BOTH
def test_misaligned_pointers(which):
    for name in ("raw", "z") + (("g",) if which == "bwd" else ()):
        for off in (1, 2, 3):
            assert _call(which, **{name: PTRS[name] + off}) == E_ALIGN, (name, off)
    for off in (1, 2, 3):
        assert _call(which, off=off) == E_ALIGN


# ------------------------------------------------------------------------------------------------------------ wrappers
def test_the_wrappers_refuse_cpu_tensors_and_bad_arguments():
    import nnr
    from nnr import ops
    raw, z = RD.make_inputs(3, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ray_distortion(raw, z, 0.01, 0.1, False, False)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ray_distortion_grad(raw, z, 0.01, 0.1, False, False, torch.ones(3))
    w = [torch.zeros(1)] * 12
    with pytest.raises(RuntimeError, match="GPU"):
        nnr.render_rays(torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(8), torch.ones(8), None, w, w, hidden=128,
                        dist_alpha=False, white_bg=False, relu_sigma=False, ray_distortion=(0.01, 0.1))
    for bad in ((0.0, 0.0), (0.0, -1.0), (NAN, 1.0), (0.0, INF)):      # refused before anything else is looked at
        with pytest.raises(ValueError):
            nnr.render_rays(torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(8), torch.ones(8), None, w, w, hidden=128,
                            dist_alpha=False, white_bg=False, relu_sigma=False, ray_distortion=bad)


def test_the_renderer_refuses_the_term_on_cpu_tensors_and_the_trainer_reads_its_key():
    import model as mdl
    from test_host_logic import make_cfg
    cfg = make_cfg(128, num_points=8)
    net = mdl.OfficialStaticNerf(cfg)
    r = mdl.Renderer(net, cfg['rendering'])
    assert r.ray_distortion is False
    r.ray_distortion = True
    pix = torch.zeros(1, 4, 2)
    with pytest.raises(NotImplementedError, match="ray_distortion_weight"):
        r(pix, torch.ones(1, 4, 1), torch.eye(4)[None], torch.eye(4)[None], torch.eye(4)[None], 'nope_nerf')
    src = open(os.path.join(ROOT, "nope-nerf_amd", "model", "training.py")).read()
    assert "cfg.get('ray_distortion_weight'" in src and "cfg['ray_distortion_weight']" not in src      # read with .get: absent = off


# ------------------------------------------------------------------------------------------------------------ the float64 reference
SHAPES = [(1, 1), (1, 2), (5, 3), (3, 65), (4, 192), (2, 1024)]


@pytest.mark.parametrize("dist_alpha,relu_sigma", FLAG_SETS)
@pytest.mark.parametrize("R,N", SHAPES)
def test_prefix_form_is_the_pairwise_definition_and_the_closed_form_gradient_is_autograd(R, N, dist_alpha, relu_sigma):
    """In float64 both pairs differ by rounding alone.  Bars: the loss to 1e-12 of itself plus 1e-15 (a sum of up to 2^20 terms of one
    sign, each good to 1e-16 of the sum); the gradient to 1e-10 of the ray's largest entry, the floor the GPU tests use for the same
    comparison (B / (1 - alpha + eps) amplifies a rounding of B a million times behind the raw = 25 sample)."""
    raw, z = RD.make_inputs(R, N)
    s_near, s_inv = 0.01, 1.0 / 9.99
    pair = RD.loss(raw, z, s_near, s_inv, dist_alpha, relu_sigma, "pairwise")
    pre = RD.loss(raw, z, s_near, s_inv, dist_alpha, relu_sigma, "prefix")
    assert torch.isfinite(pair).all() and (pair >= 0).all()
    assert ((pair - pre).abs() <= 1e-12 * pair.abs() + 1e-15).all(), float((pair - pre).abs().max())
    _, auto = RD.loss_and_grad(raw, z, s_near, s_inv, dist_alpha, relu_sigma)
    closed = RD.grad_closed_form(raw, z, s_near, s_inv, dist_alpha, relu_sigma)
    bar = 1e-10 * auto.abs().amax(dim=1, keepdim=True)
    assert ((auto - closed).abs() <= bar).all(), float(((auto - closed).abs() / bar.clamp_min(1e-300)).max())
    if N == 1:
        assert (pair == 0).all() and (auto == 0).all() and (closed == 0).all()
    if R >= 2 and not (dist_alpha and N > 1):      # the ray without mass: no loss (under dist_alpha its last sample takes all of it: one spike, no spread)
        assert float(pair[-1]) <= 1e-18


def test_the_loss_is_what_it_says_on_cases_done_by_hand():
    # two samples of weights w0, w1 at normalised depths 0.25 and 0.75: intervals [0.25, 0.75] (m 0.5, d 0.5) and the last (m 0.75, d 0)
    z = torch.tensor([[0.25, 0.75]])
    alpha = torch.tensor([[0.5, 0.5]], dtype=torch.float64)
    T, w = RD.weights_of(alpha)
    assert T[0, 0] == 1.0 and abs(float(T[0, 1]) - (0.5 + RD.EPS_T)) < 1e-15
    want = 2 * float(w[0, 0] * w[0, 1]) * 0.25 + float(w[0, 0]) ** 2 * 0.5 / 3
    assert abs(float(RD.loss_from_alpha(alpha, z, 0.0, 1.0)) - want) < 1e-15
    # normalisation: the same ray seen on (1, 3) through s_near = 1, s_inv = 1/2 is the same loss
    assert abs(float(RD.loss_from_alpha(alpha, 1.0 + 2.0 * z, 1.0, 0.5)) - want) < 1e-15
