"""CPU: the sparse inference render without a GPU -- where the entry point is declared and listed, every error return
reached with fake device pointers and host-side outputs that must stay untouched, the host side of model/geometry.py (occupancy_bits,
level_for_alpha) against loop restatements, and the float64 reference of tests/sparse_ref.py: nothing culled is the dense compositing, and
what culling may cost is bounded by the culled samples' alphas."""
import ctypes as C
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

import fusion_ref as FR      # noqa: E402
import sparse_ref as SR      # noqa: E402

OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3
INF, NAN = float("inf"), float("nan")
SENTINEL = 0x7fc0beef


def _lib():
    from nnr import lib as L
    return L, L.load()


# ------------------------------------------------------------------------------------------------------------ header and exports
def test_the_entry_point_lives_in_the_sparse_header_under_abi_8():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "nnr.h")).read()
    others = [open(os.path.join(ROOT, "include", n)).read() for n in ("nnr_geometry.h", "nnr_fusion.h")]
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnr_sparse.h")).read(), flags=re.S)
    assert lib.nnr_abi_version() == L.ABI_VERSION == int(re.search(r"#define NNR_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert "NNR_ABI_VERSION" not in code and '#include "nnr.h"' in code
    assert L.SPARSE_EXPORTS == ("nnr_render_sparse",)
    assert L.FUSION_EXPORTS == ("nnr_render_depth", "nnr_tsdf_integrate")
    assert L.GEOMETRY_EXPORTS == ("nnr_density_bricks",) and len(L.EXPORTS) == 50
    for name in L.SPARSE_EXPORTS:
        assert name not in L.EXPORTS + L.GEOMETRY_EXPORTS + L.FUSION_EXPORTS and hasattr(lib, name)
        assert name not in hdr and all(name not in o for o in others)
    protos = dict(re.findall(r"\bint\s+(nnr_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S))
    assert set(protos) == set(L.SPARSE_EXPORTS)
    for name, params in protos.items():
        assert len(getattr(lib, name).argtypes) == params.count(",") + 1, name
    assert len(lib.nnr_render_sparse.argtypes) == 17


# ------------------------------------------------------------------------------------------------------------ error returns
PTRS = dict(pts_o=0x10000, pts_d=0x20000, view_d=0x30000, z_lo=0x40000, z_hi=0x50000, jitter=0x60000, bits=0x70000, packed=0x80000)
OUTS = ("out", "opt_count", "opt_cell", "opt_out4")


def _sparse(n_rays=5, n_samples=64, hidden=256, flags=None, cfg=True, lo=(-1., -1., -1.), inv=(4., 4., 4.), dims=(8, 8, 8), null=(), off=None,
            **ptrs):
    """nnr_render_sparse with fake device inputs and HOST buffers full of a sentinel as its four outputs -> the return code; asserts that
    no output word changed.  null: names passed as NULL; off: {output name: bytes} to misalign an output."""
    L, lib = _lib()
    flags = (L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2) if flags is None else flags
    c = L.Cfg(n_rays, n_samples, hidden, flags)
    a = dict(PTRS)
    a.update(ptrs)
    v = {k: (None if (x is None or k in null) else C.c_void_p(x)) for k, x in a.items()}
    bufs = {k: np.full(64, SENTINEL, dtype=np.int32) for k in OUTS}
    o = {k: (None if k in null else C.c_void_p(bufs[k].ctypes.data + 64 + (off or {}).get(k, 0))) for k in OUTS}
    lo3 = None if "lo" in null else (C.c_float * 3)(*lo)
    is3 = None if "inv" in null else (C.c_float * 3)(*inv)
    d3 = None if "dims" in null else (C.c_int32 * 3)(*dims)
    rc = lib.nnr_render_sparse(C.byref(c) if cfg else None, v["pts_o"], v["pts_d"], v["view_d"], v["z_lo"], v["z_hi"], v["jitter"], lo3, is3, d3,
                               v["bits"], v["packed"], o["out"], o["opt_count"], o["opt_cell"], o["opt_out4"], None)
    assert rc != OK, "a call with fake device pointers must not get as far as a launch"
    for k in OUTS:
        assert (bufs[k] == SENTINEL).all(), k
    return rc


def test_render_sparse_rejects_null_pointers_sizes_and_dims_below_one():
    assert _sparse(cfg=False) == E_BADCFG
    for name in ("pts_o", "pts_d", "view_d", "z_lo", "z_hi", "bits", "packed", "out", "lo", "inv", "dims"):
        assert _sparse(null=(name,)) == E_BADCFG, name
    for n in (0, -1, -2 ** 31):
        assert _sparse(n_rays=n) == E_BADCFG and _sparse(n_samples=n) == E_BADCFG
        for axis in range(3):
            d = [8, 8, 8]
            d[axis] = n
            assert _sparse(dims=d) == E_BADCFG
    # jitter and the three test outputs may be null: such a call reaches the alignment check
    assert _sparse(null=("jitter", "opt_count", "opt_cell", "opt_out4"), packed=0x80008) == E_ALIGN
    assert _sparse(n_rays=1, n_samples=1, dims=(1, 1, 1), packed=0x80008) == E_ALIGN      # the smallest sizes pass


@pytest.mark.parametrize("bad", [INF, -INF, NAN])
def test_render_sparse_rejects_a_grid_that_is_not_finite(bad):
    for axis in range(3):
        v = [0.5, 0.5, 0.5]
        v[axis] = bad
        assert _sparse(lo=v) == E_BADCFG and _sparse(inv=v) == E_BADCFG


def test_render_sparse_wants_a_positive_inverse_step():
    for s in (0., -0., -1e-3, -4.):
        for axis in range(3):
            v = [4., 4., 4.]
            v[axis] = s
            assert _sparse(inv=v) == E_BADCFG
    assert _sparse(inv=(1e-30, 1e30, 4.), packed=0x80008) == E_ALIGN


def test_render_sparse_limits_samples_width_flags_and_grid_size():
    L, _ = _lib()
    s2 = L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    assert _sparse(n_samples=257) == E_UNSUPPORTED and _sparse(n_samples=2 ** 31 - 1) == E_UNSUPPORTED
    assert _sparse(n_samples=256, packed=0x80004) == E_ALIGN
    for hidden in (64, 192, 512, 0):
        assert _sparse(hidden=hidden) == E_UNSUPPORTED
    assert _sparse(hidden=128, packed=0x80004) == E_ALIGN
    for flags in (0, L.NNR_F_SPLIT3, L.NNR_F_SPLIT2, s2 | L.NNR_F_TRAIN, s2 | L.NNR_F_BF16, L.NNR_F_BF16, s2 | L.NNR_F_TRAIN | L.NNR_F_WHITE_BG):
        assert _sparse(flags=flags) == E_UNSUPPORTED, flags
    for flags in (s2, s2 | L.NNR_F_DIST_ALPHA, s2 | L.NNR_F_RELU_SIGMA, s2 | L.NNR_F_WHITE_BG, s2 | L.NNR_F_DIST_ALPHA | L.NNR_F_WHITE_BG):
        assert _sparse(flags=flags, packed=0x80008) == E_ALIGN, flags
    # words = n_z n_y ceil(n_x / 32): 2^31 of them is one too many, 2^31 - 2^16 pass; so is a grid of more than 2^31 - 1 cells
    assert _sparse(dims=(32, 2 ** 16, 2 ** 15)) == E_UNSUPPORTED
    assert _sparse(dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)) == E_UNSUPPORTED
    assert _sparse(dims=(1, 2 ** 16, 2 ** 15)) == E_UNSUPPORTED           # 2^31 words of one cell each
    assert _sparse(dims=(1, 2 ** 16, 2 ** 15 - 1), packed=0x80008) == E_ALIGN
    assert _sparse(dims=(64, 2 ** 16, 2 ** 10)) == E_UNSUPPORTED          # 2^27 words, 2^32 cells: opt_cell is int32
    # a bad value beats an unsupported one, an unsupported one a misaligned one
    assert _sparse(n_samples=257, dims=(0, 8, 8)) == E_BADCFG and _sparse(n_samples=257, packed=0x80004) == E_UNSUPPORTED


def test_render_sparse_rejects_misaligned_pointers():
    for addr in (0x80001, 0x80002, 0x80004, 0x80008, 0x8000c):
        assert _sparse(packed=addr) == E_ALIGN, hex(addr)
    for name in ("pts_o", "pts_d", "view_d", "z_lo", "z_hi", "jitter", "bits"):
        for off in (1, 2, 3):
            assert _sparse(**{name: PTRS[name] + off}) == E_ALIGN, (name, off)
    for name in OUTS:
        for off in (1, 2, 3):
            assert _sparse(off={name: off}) == E_ALIGN, (name, off)


def test_the_wrapper_refuses_cpu_tensors():
    from nnr import ops
    from model import geometry as G
    t = torch.zeros(4, 3)
    grid = G.OccupancyGrid((0., 0., 0.), (1., 1., 1.), (2, 2, 2), torch.zeros(2, 2, 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_sparse(t, t, t, torch.zeros(8), torch.ones(8), None, grid, [], [], hidden=128, dist_alpha=False, white_bg=False, relu_sigma=False)


# ------------------------------------------------------------------------------------------------------------ occupancy_bits
def _bits_by_loops(vol, level, dilate):
    v = vol.numpy()
    nz, ny, nx = v.shape
    cz, cy, cx = nz - 1, ny - 1, nx - 1
    occ = np.zeros((cz, cy, cx), dtype=bool)
    for iz in range(cz):
        for iy in range(cy):
            for ix in range(cx):
                corners = v[iz:iz + 2, iy:iy + 2, ix:ix + 2].ravel()
                occ[iz, iy, ix] = any((c >= level) or math.isnan(c) for c in corners)
    out = np.zeros_like(occ)
    for iz in range(cz):
        for iy in range(cy):
            for ix in range(cx):
                out[iz, iy, ix] = occ[max(iz - dilate, 0):iz + dilate + 1, max(iy - dilate, 0):iy + dilate + 1,
                                      max(ix - dilate, 0):ix + dilate + 1].any()
    wx = (cx + 31) // 32
    words = np.zeros((cz, cy, wx), dtype=np.uint32)
    for iz in range(cz):
        for iy in range(cy):
            for ix in range(cx):
                if out[iz, iy, ix]:
                    words[iz, iy, ix >> 5] |= np.uint32(1) << np.uint32(ix & 31)
    return out, words


@pytest.mark.parametrize("dilate", [0, 1, 2])
@pytest.mark.parametrize("seed", [0, 1])
def test_occupancy_bits_agrees_with_a_loop_restatement(seed, dilate):
    from model import geometry as G
    g = torch.Generator().manual_seed(seed)
    vol = torch.randn(5, 6, 37, generator=g)      # 4 x 5 x 36 cells: n_x is no multiple of 32, two words per row
    vol[2, 3, 33] = NAN
    level = 1.6                                   # about 5 % of the points: some cells of each kind
    occ, words = _bits_by_loops(vol, level, dilate)
    got = G.occupancy_bits(vol, level, dilate)
    assert got.dtype == torch.int32 and tuple(got.shape) == (4, 5, 2)
    assert np.array_equal(got.numpy().view(np.uint32), words)
    assert 0 < occ.sum() < occ.size or dilate == 2
    assert occ[1:3, 2:4, 32:34].all(), "the cells around the NaN corner are occupied"
    assert np.array_equal(SR.pack_bits(torch.from_numpy(occ)).numpy().view(np.uint32), words)
    # the reference's bit lookup reads them back
    cells = torch.arange(4 * 5 * 36)
    assert np.array_equal(SR.bit_ref(got, cells, (36, 5, 4)).numpy(), occ.ravel())
    assert abs(float(G.occupied_share(got, (36, 5, 4))) - occ.mean()) < 1e-6


def test_occupancy_bits_sets_bit_31_and_nothing_past_the_last_cell():
    from model import geometry as G
    vol = torch.full((2, 2, 34), 5.)       # 33 cells, all occupied: a full word (its sign bit too) and one bit of the next
    got = G.occupancy_bits(vol, 0., 0).numpy().view(np.uint32)
    assert got.tolist() == [[[0xFFFFFFFF, 1]]]


# ------------------------------------------------------------------------------------------------------------ level_for_alpha
@pytest.mark.parametrize("act", ["softplus", "relu"])
@pytest.mark.parametrize("delta", [None, 0.05, 1.0, 7.5])
@pytest.mark.parametrize("alpha_min", [1e-4, 1e-3, 1e-2, 0.5])
def test_level_for_alpha_round_trips_through_the_alpha_formula(alpha_min, delta, act):
    from model import geometry as G
    raw = G.level_for_alpha(alpha_min, delta, act)
    n = 3
    raws = torch.full((1, n), raw, dtype=torch.float64)
    z = torch.arange(n, dtype=torch.float64)[None] * (delta if delta is not None else 1.)
    alpha = FR.alpha_ref(raws, z, delta is not None, act == "relu")[0, 0]
    tol = 1e-6 if delta is not None else 1e-12      # (alpha_ref forms its deltas from fp32 depths)
    assert abs(float(alpha) - alpha_min) <= tol * alpha_min + 1e-15
    # monotone: a lower raw density has a lower alpha
    lower = FR.alpha_ref(raws - 0.1, z, delta is not None, act == "relu")[0, 0]
    assert float(lower) < float(alpha)
    for bad in (0., 1., -0.1, NAN):
        with pytest.raises(ValueError):
            G.level_for_alpha(bad, delta, act)


# ------------------------------------------------------------------------------------------------------------ the reference itself
def _random_rows(n_rows, n, seed):
    g = torch.Generator().manual_seed(seed)
    # alphas of every size: many tiny, some large, a few exactly 0 or 1
    alpha = torch.rand(n_rows, n, generator=g, dtype=torch.float64) ** torch.randint(1, 12, (n_rows, 1), generator=g).double()
    alpha[torch.rand(n_rows, n, generator=g) < 0.02] = 1.
    alpha[torch.rand(n_rows, n, generator=g) < 0.05] = 0.
    rgb = torch.rand(n_rows, n, 3, generator=g, dtype=torch.float64)
    z = torch.sort(torch.rand(n_rows, n, generator=g, dtype=torch.float64) * 6. + 0.1, dim=1)[0]
    return alpha, rgb, z, g


def test_nothing_culled_is_the_dense_compositing():
    alpha, rgb, z, _ = _random_rows(200, 48, 3)
    live = torch.ones(200, 48, dtype=torch.bool)
    for white in (False, True):
        got = SR.composite_masked(alpha, rgb, z, live, white)
        T = torch.cumprod(torch.cat([torch.ones(200, 1, dtype=torch.float64), 1. - alpha[:, :-1] + 1e-6], 1), 1)
        w = alpha * T
        want_rgb = (w[..., None] * rgb).sum(1) + ((1. - w.sum(1))[:, None] if white else 0.)
        assert torch.equal(got[:, :3], want_rgb)
        assert torch.equal(got[:, 3:], FR.composite_ref(alpha, z))
    assert [SR.compact_ref(r) for r in torch.tensor([[True, False, True], [False, False, False]])] == [[0, 2], []]


def test_what_culling_costs_is_bounded_by_the_culled_alphas():
    alpha, rgb, z, g = _random_rows(4000, 64, 7)
    # cull at random, and preferably the small alphas, as a grid would
    live = (torch.rand(4000, 64, generator=g) < 0.5) | (alpha > torch.rand(4000, 1, generator=g).double() * 0.1)
    live[:50] = False
    live[50:100] = True
    dense = SR.composite_masked(alpha, rgb, z, torch.ones_like(live))
    sparse = SR.composite_masked(alpha, rgb, z, live)
    bound = SR.culling_bound(alpha, live)
    err = (sparse - dense).abs()
    assert bool((err[:, :3] <= bound[:, None]).all()) and bool((err[:, 4] <= bound).all())
    assert bool((err[:, 3] <= bound * z.max(1)[0]).all())
    assert bool((err[50:100] == 0).all()) and bool((sparse[:50] == 0).all())
    assert float(err.max()) > 0.1, "the random culling never cost anything: the bound was not tested"
    # a NaN in a culled sample does not reach the ray
    rgb2, alpha2 = rgb.clone(), alpha.clone()
    rgb2[~live] = NAN
    assert torch.equal(SR.composite_masked(alpha, rgb2, z, live), sparse)


def test_cell_ref_follows_the_header():
    lo, inv, dims = (-1., -2., 0.), (2., 1., 4.), (4, 4, 3)
    pts = torch.tensor([[-1., -2., 0.], [0.99, 1.99, 0.74], [1., 0., 0.], [0., 2., 0.], [0., 0., 0.75], [-1.001, 0.5, 0.1], [NAN, 0.5, 0.1],
                        [-0.26, -0.5, 0.3]], dtype=torch.float64)
    cell, near = SR.cell_ref(pts, lo, inv, dims)
    assert cell.tolist() == [0, (2 * 4 + 3) * 4 + 3, -1, -1, -1, -1, -1, (1 * 4 + 1) * 4 + 1]
    assert near.tolist() == [True, False, True, True, True, False, False, False]
