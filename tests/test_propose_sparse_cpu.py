"""CPU: the sparse proposal (include/nnr_propose_sparse.h) without a GPU -- where the entry point is declared and
listed, every error return reached with fake device pointers and host-side outputs that must stay untouched, what the build lists and
checks for the new unit, the reference of tests/propose_sparse_ref.py itself, and the renderer's key `rendering.occupancy.proposal` where
no GPU is needed."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nope-nerf_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import propose_sparse_ref as PS      # noqa: E402
import resample_ref as RR            # noqa: E402
import sparse_ref as SR              # noqa: E402

OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3
INF, NAN = float("inf"), float("nan")
SENTINEL = 0x7fc0beef


def _lib():
    from nnr import lib as L
    return L, L.load()


def _build():
    spec = importlib.util.spec_from_file_location("nnr_build_ps", os.path.join(CSRC, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


# ------------------------------------------------------------------------------------------------------------ header and exports
def _params(header, name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return [re.sub(r"\s+", " ", p.strip()) for p in re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, code, flags=re.S).group(1).split(",")]


def test_the_entry_point_lives_in_its_own_header_under_abi_8():
    L, lib = _lib()
    inc = os.path.join(ROOT, "include")
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nnr_propose_sparse.h")).read(), flags=re.S)
    assert lib.nnr_abi_version() == L.ABI_VERSION == 8
    assert "NNR_ABI_VERSION" not in code and '#include "nnr.h"' in code
    assert L.PROPOSE_SPARSE_EXPORTS == ("nnr_propose_sparse",)
    assert L.SPARSE_EXPORTS == ("nnr_render_sparse",) and L.SPARSE_STOP_EXPORTS == ("nnr_render_sparse_stop",) and len(L.EXPORTS) == 50
    others = (L.EXPORTS + L.GEOMETRY_EXPORTS + L.FUSION_EXPORTS + L.SPARSE_EXPORTS + L.SPARSE_STOP_EXPORTS + L.REGULARISE_EXPORTS
              + L.FROZEN_EXPORTS + L.FROZEN_SPARSE_EXPORTS)
    for name in L.PROPOSE_SPARSE_EXPORTS:
        assert name not in others and hasattr(lib, name)
        for h in sorted(os.listdir(inc)):
            if h != "nnr_propose_sparse.h":
                assert name not in open(os.path.join(inc, h)).read(), h
    protos = dict(re.findall(r"\bint\s+(nnr_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S))
    assert set(protos) == set(L.PROPOSE_SPARSE_EXPORTS)
    params = _params("nnr_propose_sparse.h", "nnr_propose_sparse")
    assert len(params) == len(lib.nnr_propose_sparse.argtypes) == 21
    # nnr_propose's parameters in its order, the grid arguments of the sparse render between xi and packed, the three new outputs in
    # front of the stream
    dense = _params("nnr.h", "nnr_propose")
    sparse = _params("nnr_sparse.h", "nnr_render_sparse")
    assert len(dense) == 14 and params[:8] + params[12:17] + params[20:] == dense
    assert params[8:12] == sparse[7:11] and [p.split()[-1] for p in params[8:12]] == ["grid_lo[3]", "grid_inv_step[3]", "grid_dims[3]", "bits"]
    assert params[17:20] == ["int32_t* opt_count", "int32_t* opt_cell", "int32_t* opt_passes"]


# ------------------------------------------------------------------------------------------------------------ error returns
PTRS = dict(pts_o=0x10000, pts_d=0x20000, z_lo=0x30000, z_hi=0x40000, jitter=0x50000, xi=0x60000, bits=0x70000, packed=0x80000)
OUTS = ("z_all", "opt_alpha", "opt_z", "opt_fine", "opt_count", "opt_cell", "opt_passes")
OPTIONAL = ("jitter", "xi", "opt_alpha", "opt_z", "opt_fine", "opt_count", "opt_cell", "opt_passes")


def _call(n_rays=5, n_samples=64, n_fine=128, hidden=256, flags=None, cfg=True, lo=(-1., -1., -1.), inv=(4., 4., 4.), dims=(8, 8, 8), null=(),
          off=None, **ptrs):
    """nnr_propose_sparse with fake device inputs and HOST buffers full of a sentinel as its outputs -> the return code; asserts that no
    output word changed.  null: names passed as NULL; off: {output name: bytes} to misalign an output."""
    L, lib = _lib()
    flags = (L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2) if flags is None else flags
    c = L.Cfg(n_rays, n_samples, hidden, flags)
    a = dict(PTRS)
    a.update(ptrs)
    v = {k: (None if k in null else C.c_void_p(x)) for k, x in a.items()}
    bufs = {k: np.full(64, SENTINEL, dtype=np.int32) for k in OUTS}
    o = {k: (None if k in null else C.c_void_p(bufs[k].ctypes.data + 64 + (off or {}).get(k, 0))) for k in OUTS}
    lo3 = None if "lo" in null else (C.c_float * 3)(*lo)
    is3 = None if "inv" in null else (C.c_float * 3)(*inv)
    d3 = None if "dims" in null else (C.c_int32 * 3)(*dims)
    rc = lib.nnr_propose_sparse(C.byref(c) if cfg else None, n_fine, v["pts_o"], v["pts_d"], v["z_lo"], v["z_hi"], v["jitter"], v["xi"], lo3, is3,
                                d3, v["bits"], v["packed"], *[o[k] for k in OUTS], None)
    assert rc != OK, "a call with fake device pointers must not get as far as a launch"
    for k in OUTS:
        assert (bufs[k] == SENTINEL).all(), k
    return rc


def _reaches_the_alignment_check(**kw):
    """a call that every value check accepts: told apart from a refusal by the one thing still wrong, a `packed` that is 8-byte aligned"""
    return _call(packed=0x80008, **kw) == E_ALIGN


def test_bad_sizes_and_null_pointers_are_bad_values():
    assert _call(cfg=False) == E_BADCFG
    for name in ("pts_o", "pts_d", "z_lo", "z_hi", "bits", "packed", "z_all", "lo", "inv", "dims"):
        assert _call(null=(name,)) == E_BADCFG, name
    for n in (0, -1, -2 ** 31):
        assert _call(n_rays=n) == E_BADCFG and _call(n_fine=n) == E_BADCFG and _call(n_samples=n) == E_BADCFG
    assert _call(n_samples=2) == E_BADCFG and _call(n_samples=1) == E_BADCFG      # nnr_propose's C >= 3
    assert _reaches_the_alignment_check(null=OPTIONAL)
    assert _reaches_the_alignment_check(n_rays=1, n_samples=3, n_fine=1, dims=(1, 1, 1))


def test_the_grid_checks_are_the_sparse_renders():
    for n in (0, -1, -2 ** 31):
        for axis in range(3):
            d = [8, 8, 8]
            d[axis] = n
            assert _call(dims=tuple(d)) == E_BADCFG
    for bad in (INF, -INF, NAN):
        for axis in range(3):
            v = [0.5, 0.5, 0.5]
            v[axis] = bad
            assert _call(lo=tuple(v)) == E_BADCFG and _call(inv=tuple(v)) == E_BADCFG
    for s in (0., -0., -1e-3, -4.):
        for axis in range(3):
            v = [4., 4., 4.]
            v[axis] = s
            assert _call(inv=tuple(v)) == E_BADCFG
    assert _reaches_the_alignment_check(inv=(1e-30, 1e30, 4.))
    for dims in ((32, 2 ** 16, 2 ** 15), (2 ** 31 - 1,) * 3, (1, 2 ** 16, 2 ** 15), (64, 2 ** 16, 2 ** 10)):      # rows, words or cells past int32
        assert _call(dims=dims) == E_UNSUPPORTED, dims
    assert _reaches_the_alignment_check(dims=(1, 2 ** 16, 2 ** 15 - 1))


def test_sizes_widths_and_flags_the_kernel_does_not_have_are_unsupported():
    L, _ = _lib()
    s2 = L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    for Cn, F in ((257, 8), (1024, 1), (64, 961), (256, 769), (2 ** 30, 2 ** 30), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert _call(n_samples=Cn, n_fine=F) == E_UNSUPPORTED, (Cn, F)
    assert _reaches_the_alignment_check(n_samples=256, n_fine=768) and _reaches_the_alignment_check(n_samples=64, n_fine=960)
    for h in (64, 192, 512, 0):
        assert _call(hidden=h) == E_UNSUPPORTED, h
    assert _reaches_the_alignment_check(hidden=128)
    for f in (0, L.NNR_F_SPLIT3, L.NNR_F_SPLIT2, s2 | L.NNR_F_TRAIN, s2 | L.NNR_F_BF16, L.NNR_F_BF16, s2 | L.NNR_F_TRAIN | L.NNR_F_DIST_ALPHA):
        assert _call(flags=f) == E_UNSUPPORTED, f
    for f in (s2, s2 | L.NNR_F_DIST_ALPHA, s2 | L.NNR_F_RELU_SIGMA, s2 | L.NNR_F_WHITE_BG, s2 | L.NNR_F_DIST_ALPHA | L.NNR_F_RELU_SIGMA):
        assert _reaches_the_alignment_check(flags=f), f


def test_misaligned_pointers_are_refused():
    for a in (0x80001, 0x80002, 0x80004, 0x80008, 0x8000c):
        assert _call(packed=a) == E_ALIGN, a
    for name in ("pts_o", "pts_d", "z_lo", "z_hi", "jitter", "xi", "bits"):
        for off in (1, 2, 3):
            assert _call(**{name: PTRS[name] + off}) == E_ALIGN, (name, off)
    for name in OUTS:
        for off in (1, 2, 3):
            assert _call(off={name: off}) == E_ALIGN, (name, off)
    for off in (4, 8, 12):      # z_all: the kernel's 16-byte stores
        assert _call(off={"z_all": off}) == E_ALIGN, off


def test_precedence_bad_value_then_unsupported_then_misaligned():
    assert _call(n_samples=2, hidden=64) == E_BADCFG and _call(n_fine=0, n_samples=257) == E_BADCFG
    assert _call(null=("bits",), n_samples=257) == E_BADCFG and _call(dims=(0, 8, 8), n_samples=257) == E_BADCFG
    assert _call(inv=(NAN, 4., 4.), packed=0x80004) == E_BADCFG
    assert _call(n_samples=257, packed=0x80004) == E_UNSUPPORTED and _call(n_samples=64, n_fine=961, off={"opt_passes": 1}) == E_UNSUPPORTED
    assert _call(dims=(32, 2 ** 16, 2 ** 15), off={"opt_cell": 2}) == E_UNSUPPORTED


def test_the_wrapper_refuses_cpu_tensors():
    from nnr import ops
    from model import geometry as G
    t = torch.zeros(4, 3)
    grid = G.OccupancyGrid((0., 0., 0.), (1., 1., 1.), (2, 2, 2), torch.zeros(2, 2, 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.propose_sparse(t, t, torch.zeros(8), torch.ones(8), None, None, 4, grid, [], [], hidden=128, dist_alpha=False, relu_sigma=False)
    assert ops.frozen_occupancy() is None
    with ops.frozen_field(occupancy=grid):
        assert ops.frozen_occupancy() is grid
        with ops.frozen_field():
            assert ops.frozen_occupancy() is None
        assert ops.frozen_occupancy() is grid
    assert ops.frozen_occupancy() is None


# ------------------------------------------------------------------------------------------------------------ the build
MANGLED = "_ZN3nnr25propose_sparse_f16_kernelILi%dEEEvNS_17ProposeSparseArgsE"
REMARK = "remark: Function Name: %s\nremark:     ScratchSize [bytes/lane]: %d\n"


def test_sources_holds_the_new_entry_once_with_an_object_of_its_own():
    b = _build()
    entry = ("nnr_propose_f16.hip", ("NNR_PROPOSE_SPARSE=1",))
    assert b.SOURCES.count(entry) == 1 and b.SOURCES.count(("nnr_propose_f16.hip", ())) == 1
    names = [b._obj_name(s, d) for s, d in b.SOURCES]
    assert names.count(b._obj_name(*entry)) == 1 and b._obj_name(*entry) != b._obj_name("nnr_propose_f16.hip", ())
    assert len({s for s, _ in b.SOURCES}) == 31      # no new source file


def test_the_build_holds_the_kernel_to_no_scratch():
    b = _build()
    assert b.SCRATCH_LIMIT["25propose_sparse_f16_kernelI"] == 0 and b.SCRATCH_LIMIT["18propose_f16_kernelI"] == 0
    for D in (128, 256):
        b.check_resources(REMARK % (MANGLED % D, 0), "test")
        for size in (1, 16):
            with pytest.raises(RuntimeError, match="scratch"):
                b.check_resources(REMARK % (MANGLED % D, size), "test")


def _users(b, path):
    sources = {s for s, _ in b.SOURCES}
    return {src for src in sources if any(os.path.samefile(d, path) for d in b.deps(src))}


def test_the_new_headers_make_exactly_their_users_stale():
    b = _build()
    assert _users(b, os.path.join(CSRC, "nnr_cell_rule.h")) == {"nnr_sparse_f16.hip", "nnr_frozen_sparse.hip", "nnr_propose_f16.hip"}
    assert _users(b, os.path.join(CSRC, "nnr_propose_sparse_kernels.h")) == {"nnr_propose_f16.hip", "nnr_sparse_api.cpp"}
    assert _users(b, os.path.join(ROOT, "include", "nnr_propose_sparse.h")) == {"nnr_sparse_api.cpp"}
    # the files that name nnr_sparse_cell.h are the two that did, and the rule's text exists once
    naming, defining = set(), set()
    for f in sorted(os.listdir(CSRC)):
        if os.path.isfile(os.path.join(CSRC, f)) and f.endswith((".hip", ".cpp", ".h", ".inc")):
            text = open(os.path.join(CSRC, f)).read()
            if re.search(r'#\s*include\s+"nnr_sparse_cell\.h"', text):
                naming.add(f)
            if re.search(r"\bint\s+sparse_cell\s*\(", text):
                defining.add(f)
    assert naming == {"nnr_sparse_f16.hip", "nnr_frozen_sparse.hip"} and defining == {"nnr_cell_rule.h"}
    api = open(os.path.join(CSRC, "nnr_sparse_api.cpp")).read()
    assert "nnr_layout.h" not in api and "nnr_kernels.h" not in re.sub(r"nnr_(propose_)?sparse_kernels\.h", "", api)
    own = open(os.path.join(CSRC, "nnr_propose_sparse_kernels.h")).read()
    assert not re.search(r'#\s*include\s+"', own)      # self-contained: the toolchain's headers only


# ------------------------------------------------------------------------------------------------------------ the reference itself
def _grid16(lo, hi, occ):
    dims = (16, 16, 16)
    inv = [16. / (hi - lo)] * 3
    return [lo] * 3, inv, dims, SR.pack_bits(occ)


def _rows(R, Cn, seed):
    alpha, z = RR.make_inputs(R, Cn, seed, near=1.0, far=4.0)
    g = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 2.5
    d = torch.nn.functional.normalize(-o + 0.3 * torch.randn(R, 3, generator=g), dim=-1)
    xi = torch.rand(R, 24, generator=g)
    return alpha, z, o, d, xi


def test_nothing_culled_is_resample_ref():
    alpha, z, o, d, xi = _rows(23, 40, 5)
    lo, inv, dims, bits = _grid16(-8., 8., torch.ones(16, 16, 16, dtype=torch.bool))
    live, cell, _ = PS.live_of(o, d, z, lo, inv, dims, bits)
    assert bool(live.all()) and bool((cell >= 0).all())
    got, want = PS.propose_sparse_ref(alpha, z, live, xi, 24), RR.resample_ref(alpha, z, xi, 24)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a grid that holds none of the samples culls nothing either, whatever its bits
    lo, inv, dims, bits = _grid16(20., 21., torch.zeros(16, 16, 16, dtype=torch.bool))
    live, cell, _ = PS.live_of(o, d, z, lo, inv, dims, bits)
    assert bool(live.all()) and bool((cell == -1).all())


def test_all_culled_gives_the_uniform_row():
    alpha, z, o, d, xi = _rows(23, 40, 6)
    z = z.sort(dim=1)[0]
    lo, inv, dims, bits = _grid16(-8., 8., torch.zeros(16, 16, 16, dtype=torch.bool))
    live, _, _ = PS.live_of(o, d, z, lo, inv, dims, bits)
    assert not bool(live.any())
    z_all, fine = PS.propose_sparse_ref(alpha, z, live, xi, 24)
    assert bool(torch.isfinite(z_all).all()) and bool((z_all[:, 1:] >= z_all[:, :-1]).all())
    # every bin holds the floor alone: the CDF is linear in the bin index, the fine samples interpolate the edges m at t = u (C - 2)
    m = 0.5 * (z.double()[:, :-1] + z.double()[:, 1:])
    t = RR.u_of(xi, 23, 24) * (40 - 2)
    k = t.floor().clamp(max=40 - 3).long()
    want = m.gather(1, k) + (t - k) * (m.gather(1, k + 1) - m.gather(1, k))
    assert float((fine - want).abs().max()) <= 1e-9
    assert PS.passes_ref(live.sum(1), 23).tolist() == [0] * 23


def test_a_culled_nan_alpha_does_not_poison_the_row():
    alpha, z, o, d, xi = _rows(9, 40, 7)
    occ = torch.rand(16, 16, 16, generator=torch.Generator().manual_seed(1)) < 0.5
    lo, inv, dims, bits = _grid16(-4., 4., occ)      # cells of 0.5: a ray crosses some eight of them
    live, _, _ = PS.live_of(o, d, z, lo, inv, dims, bits)
    assert bool((~live).any(1).all()) and bool(live.any(1).all())
    clean = PS.propose_sparse_ref(alpha, z, live, xi, 24)
    dirty = torch.where(live, alpha, torch.full_like(alpha, NAN))      # every culled sample's dense alpha is NaN
    got = PS.propose_sparse_ref(dirty, z, live, xi, 24)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[1], clean[1]) and bool(torch.isfinite(got[0]).all())
    # a LIVE NaN does: its ray alone
    j = int(live[4].nonzero()[0])
    dirty[4, j] = NAN
    got = PS.propose_sparse_ref(dirty, z, live, xi, 24)
    assert bool(torch.isnan(got[0][4]).all()) and torch.equal(got[0][:4], clean[0][:4]) and torch.equal(got[0][5:], clean[0][5:])


def test_pass_counts_follow_the_workgroups_largest_list():
    assert PS.passes_ref(torch.tensor([0, 1, 32, 33, 64, 65, 0, 0, 0]), 9).tolist() == [2] * 4 + [3] * 4 + [0]
    assert PS.passes_ref(torch.tensor([0, 0, 0, 0, 256]), 5).tolist() == [0] * 4 + [8]


# ------------------------------------------------------------------------------------------------------------ the renderer's key on the CPU
OCC = dict(resolution=8, alpha_min=0.01)


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


def _try_render(renderer, args):
    try:
        with torch.no_grad():
            out = renderer.nope_nerf(*args, add_noise=False)
    except Exception as e:      # noqa: BLE001 -- compared by type and text below
        return type(e), str(e)
    return out['rgb'].detach().clone(), out['dist_dense'].detach().clone()


def _same(a, b):
    assert type(a) is type(b)
    for x, y in zip(a, b):
        assert torch.equal(x, y) if torch.is_tensor(x) else x == y


def test_render_proposal_with_the_key_raises_naming_both_keys():
    for proposal in ('render', None):      # (absent = 'render')
        extra = dict(proposal=proposal) if proposal else {}
        renderer, args = _cpu_render(num_fine=16, occupancy=dict(OCC, proposal=True), **extra)
        with pytest.raises(ValueError) as e:
            renderer.nope_nerf(*args, add_noise=False)
        assert "rendering.occupancy.proposal" in str(e.value) and "rendering.proposal" in str(e.value)


def test_key_absent_equals_false_on_the_cpu():
    """With num_fine > 0 both are the CPU refusal of hierarchical sampling, word for word; true with 'density' is that refusal too (the key
    is a setting of a GPU launch); an unknown rendering.proposal is still reported first."""
    for proposal in ('render', 'density'):
        absent = _try_render(*_cpu_render(num_fine=16, proposal=proposal, occupancy=dict(OCC)))
        false = _try_render(*_cpu_render(num_fine=16, proposal=proposal, occupancy=dict(OCC, proposal=False)))
        _same(absent, false)
        assert absent[0] is NotImplementedError and "num_fine" in absent[1]
    assert _try_render(*_cpu_render(num_fine=16, proposal='density', occupancy=dict(OCC, proposal=True)))[0] is NotImplementedError
    assert _try_render(*_cpu_render(num_fine=16, proposal='bogus', occupancy=dict(OCC, proposal=True)))[0] is ValueError


@pytest.mark.parametrize("extra", [dict(), dict(num_fine=0), dict(num_fine=0, proposal='render'), dict(proposal='render')])
def test_the_key_is_ignored_without_num_fine(extra):
    plain = _try_render(*_cpu_render(occupancy=dict(OCC), **extra))
    for value in (True, False):
        _same(plain, _try_render(*_cpu_render(occupancy=dict(OCC, proposal=value), **extra)))
