"""CPU: the sparse depth render (include/nnr_depth_sparse.h) without a GPU -- where the entry point is declared and
listed, every error return reached with fake device pointers and host-side outputs that must stay untouched, what the build lists and
checks for the new unit, the wrappers' refusals, the mesh tool's argument errors and the reference of tests/depth_sparse_ref.py itself."""
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
for p in ("nope-nerf_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import depth_sparse_ref as DS        # noqa: E402
import fusion_ref as FR              # noqa: E402
import sparse_ref as SR              # noqa: E402
import sparse_stop_ref as ST         # noqa: E402

OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3
INF, NAN = float("inf"), float("nan")
SENTINEL = 0x7fc0beef


def _lib():
    from nnr import lib as L
    return L, L.load()


def _build():
    spec = importlib.util.spec_from_file_location("nnr_build_ds", os.path.join(CSRC, "build.py"))
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
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nnr_depth_sparse.h")).read(), flags=re.S)
    assert lib.nnr_abi_version() == L.ABI_VERSION == 8 and len(L.EXPORTS) == 50
    assert "NNR_ABI_VERSION" not in code and '#include "nnr.h"' in code
    assert L.DEPTH_SPARSE_EXPORTS == ("nnr_render_depth_sparse",)
    others = (L.EXPORTS + L.GEOMETRY_EXPORTS + L.FUSION_EXPORTS + L.SPARSE_EXPORTS + L.SPARSE_STOP_EXPORTS + L.PROPOSE_SPARSE_EXPORTS
              + L.REGULARISE_EXPORTS + L.FROZEN_EXPORTS + L.FROZEN_SPARSE_EXPORTS)
    for name in L.DEPTH_SPARSE_EXPORTS:
        assert name not in others and hasattr(lib, name)
        for h in sorted(os.listdir(inc)):
            if h != "nnr_depth_sparse.h":
                assert name not in open(os.path.join(inc, h)).read(), h
    protos = dict(re.findall(r"\bint\s+(nnr_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S))
    assert set(protos) == set(L.DEPTH_SPARSE_EXPORTS)
    params = _params("nnr_depth_sparse.h", "nnr_render_depth_sparse")
    assert len(params) == len(lib.nnr_render_depth_sparse.argtypes) == 18
    # nnr_render_depth's rays and tables, the grid arguments of the sparse render, the stop's t_min, then packed, out and the debug outputs
    dense = _params("nnr_fusion.h", "nnr_render_depth")
    sparse = _params("nnr_sparse.h", "nnr_render_sparse")
    assert params[:6] == dense[:6] and params[6:10] == sparse[7:11]
    assert params[10:] == ["float t_min", "const float* packed", "float* out", "float* opt_raw", "int32_t* opt_count", "int32_t* opt_cell",
                           "int32_t* opt_passes", "void* stream"]


# ------------------------------------------------------------------------------------------------------------ error returns
PTRS = dict(pts_o=0x10000, pts_d=0x20000, z_lo=0x30000, z_hi=0x40000, jitter=0x50000, bits=0x70000, packed=0x80000)
OUTS = ("out", "opt_raw", "opt_count", "opt_cell", "opt_passes")
OPTIONAL = ("jitter", "opt_raw", "opt_count", "opt_cell", "opt_passes")


def _call(n_rays=5, n_samples=64, hidden=256, flags=None, cfg=True, lo=(-1., -1., -1.), inv=(4., 4., 4.), dims=(8, 8, 8), t_min=1e-3, null=(),
          off=None, **ptrs):
    """nnr_render_depth_sparse with fake device inputs and HOST buffers full of a sentinel as its outputs -> the return code; asserts that
    no output word changed.  null: names passed as NULL; off: {output name: bytes} to misalign an output."""
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
    rc = lib.nnr_render_depth_sparse(C.byref(c) if cfg else None, v["pts_o"], v["pts_d"], v["z_lo"], v["z_hi"], v["jitter"], lo3, is3, d3,
                                     v["bits"], t_min, v["packed"], *[o[k] for k in OUTS], None)
    assert rc != OK, "a call with fake device pointers must not get as far as a launch"
    for k in OUTS:
        assert (bufs[k] == SENTINEL).all(), k
    return rc


def _reaches_the_alignment_check(**kw):
    """a call that every value check accepts: told apart from a refusal by the one thing still wrong, a `packed` that is 8-byte aligned"""
    return _call(packed=0x80008, **kw) == E_ALIGN


def test_bad_sizes_null_pointers_and_thresholds_are_bad_values():
    assert _call(cfg=False) == E_BADCFG
    for name in ("pts_o", "pts_d", "z_lo", "z_hi", "bits", "packed", "out", "lo", "inv", "dims"):
        assert _call(null=(name,)) == E_BADCFG, name
    for n in (0, -1, -2 ** 31):
        assert _call(n_rays=n) == E_BADCFG and _call(n_samples=n) == E_BADCFG
    for t in (-1e-9, 1.0, NAN, INF, -INF, -1., 2.):
        assert _call(t_min=t) == E_BADCFG, t
    for t in (0., 1e-30, 1e-3, 0.999999):
        assert _reaches_the_alignment_check(t_min=t), t
    assert _reaches_the_alignment_check(null=OPTIONAL)
    assert _reaches_the_alignment_check(n_rays=1, n_samples=1, dims=(1, 1, 1))      # nnr_render_depth's C >= 1


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
    for Cn in (257, 288, 1024, 2 ** 30, 2 ** 31 - 1):
        assert _call(n_samples=Cn) == E_UNSUPPORTED, Cn
    assert _reaches_the_alignment_check(n_samples=256)
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
    for name in ("pts_o", "pts_d", "z_lo", "z_hi", "jitter", "bits"):
        for off in (1, 2, 3):
            assert _call(**{name: PTRS[name] + off}) == E_ALIGN, (name, off)
    for name in OUTS:
        for off in (1, 2, 3):
            assert _call(off={name: off}) == E_ALIGN, (name, off)


def test_precedence_bad_value_then_unsupported_then_misaligned():
    assert _call(n_samples=0, hidden=64) == E_BADCFG and _call(n_rays=0, n_samples=257) == E_BADCFG
    assert _call(null=("bits",), n_samples=257) == E_BADCFG and _call(dims=(0, 8, 8), n_samples=257) == E_BADCFG
    assert _call(inv=(NAN, 4., 4.), packed=0x80004) == E_BADCFG
    assert _call(t_min=1.0, n_samples=257) == E_BADCFG and _call(t_min=NAN, hidden=64, packed=0x80004) == E_BADCFG
    assert _call(t_min=-1e-9, dims=(32, 2 ** 16, 2 ** 15)) == E_BADCFG
    assert _call(n_samples=257, packed=0x80004) == E_UNSUPPORTED and _call(hidden=64, off={"opt_passes": 1}) == E_UNSUPPORTED
    assert _call(dims=(32, 2 ** 16, 2 ** 15), off={"opt_cell": 2}) == E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------ the wrappers
def _grid():
    from model import geometry as G
    return G.OccupancyGrid((0., 0., 0.), (1., 1., 1.), (2, 2, 2), torch.zeros(2, 2, 1, dtype=torch.int32))


def test_the_wrapper_refuses_cpu_tensors_and_bad_thresholds():
    from nnr import ops
    t = torch.zeros(4, 3)
    kw = dict(hidden=128, dist_alpha=False, relu_sigma=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_depth_sparse(t, t, torch.zeros(8), torch.ones(8), None, _grid(), [], [], **kw)
    for bad in (-1e-9, 1.0, NAN, INF):
        with pytest.raises(ValueError, match="t_min"):
            ops.render_depth_sparse(t, t, torch.zeros(8), torch.ones(8), None, _grid(), [], [], t_min=bad, **kw)
    assert ops.depth_sparse_tally is None


def _cpu_renderer():
    import model as mdl
    from test_host_logic import make_cfg
    cfg = make_cfg(128)
    torch.manual_seed(4)
    return mdl.Renderer(mdl.OfficialStaticNerf(cfg), cfg['rendering'], device='cpu')


def test_render_depth_maps_refuses_a_threshold_without_a_grid():
    from model import geometry as G
    renderer = _cpu_renderer()
    eye = torch.eye(4)
    with pytest.raises(ValueError, match="t_min.*occupancy"):
        G.render_depth_maps(renderer, eye, eye[None], (2, 2), t_min=1e-3)
    cams = G.Cameras(eye, eye[None], (2, 2))
    with pytest.raises(NotImplementedError):      # (the GPU refusal first, as before the arguments existed)
        G.extract_mesh_tsdf(renderer, cams, (-1.,) * 3, (1.,) * 3, 8, t_min=1e-3)
    with pytest.raises(NotImplementedError):      # t_min = 0 without a grid is today's call: the CPU refusal
        G.render_depth_maps(renderer, eye, eye[None], (2, 2), t_min=0.)
    with pytest.raises(NotImplementedError):
        G.render_depth_maps(renderer, eye, eye[None], (2, 2), occupancy=_grid(), t_min=1e-3)


@pytest.mark.parametrize("argv,said", [(["--occupancy", "64", "0.01"], "--method tsdf"),
                                       (["--t-min", "1e-3"], "--method tsdf"),
                                       (["--occupancy-dilate", "2"], "--method tsdf"),
                                       (["--occupancy-bounds", "-1", "1"], "--method tsdf"),
                                       (["--method", "density", "--occupancy", "64", "0.01", "--t-min", "1e-3"], "--method tsdf"),
                                       (["--method", "tsdf", "--t-min", "1e-3"], "--occupancy"),
                                       (["--method", "tsdf", "--occupancy-dilate", "2"], "--occupancy"),
                                       (["--method", "tsdf", "--occupancy-bounds", "-1", "1"], "--occupancy"),
                                       (["--method", "tsdf", "--occupancy", "64", "0.01", "--t-min", "1.0"], "--t-min"),
                                       (["--method", "tsdf", "--occupancy", "64", "0.01", "--t-min", "0"], "--t-min"),
                                       (["--method", "tsdf", "--occupancy", "64"], "--occupancy"),
                                       (["--method", "tsdf", "--occupancy", "0", "0.01"], "--occupancy")])
def test_the_mesh_tools_argument_errors_fire(argv, said, monkeypatch, capsys):
    import extract_mesh
    monkeypatch.setattr(sys, "argv", ["extract_mesh.py", "no_such_config.yaml"] + argv)
    with pytest.raises(SystemExit) as e:
        extract_mesh.main()
    assert e.value.code == 2 and said in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------------ the build
MANGLED = "_ZN3nnr23depth_sparse_f16_kernelILi%dEEEvNS_15DepthSparseArgsE"
REMARK = "remark: Function Name: %s\nremark:     ScratchSize [bytes/lane]: %d\n"


def test_sources_holds_the_new_entry_once_with_an_object_of_its_own():
    b = _build()
    entry = ("nnr_propose_f16.hip", ("NNR_PROPOSE_SPARSE=1", "NNR_PROPOSE_DEPTH=1"))
    assert b.SOURCES.count(entry) == 1
    assert b.SOURCES.count(("nnr_propose_f16.hip", ())) == 1 and b.SOURCES.count(("nnr_propose_f16.hip", ("NNR_PROPOSE_SPARSE=1",))) == 1
    names = [b._obj_name(s, d) for s, d in b.SOURCES]
    assert names.count(b._obj_name(*entry)) == 1 and len(set(names)) == len(names)
    assert len({s for s, _ in b.SOURCES}) == 31      # no new source file
    assert not [d for s, ds in b.SOURCES for d in ds if d.startswith("NNR_PROPOSE_DEPTH") and "NNR_PROPOSE_SPARSE=1" not in ds]
    text = open(os.path.join(CSRC, "nnr_propose_f16.hip")).read()
    assert re.search(r"#if NNR_PROPOSE_DEPTH && !NNR_PROPOSE_SPARSE\s*\n#error", text)


def test_the_build_holds_the_kernel_to_no_scratch():
    b = _build()
    assert b.SCRATCH_LIMIT["23depth_sparse_f16_kernelI"] == 0
    assert b.SCRATCH_LIMIT["25propose_sparse_f16_kernelI"] == 0 and b.SCRATCH_LIMIT["16depth_f16_kernelI"] == 0
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
    assert _users(b, os.path.join(CSRC, "nnr_depth_sparse_kernels.h")) == {"nnr_propose_f16.hip", "nnr_sparse_api.cpp"}
    assert _users(b, os.path.join(ROOT, "include", "nnr_depth_sparse.h")) == {"nnr_sparse_api.cpp"}
    own = open(os.path.join(CSRC, "nnr_depth_sparse_kernels.h")).read()
    assert not re.search(r'#\s*include\s+"', own)      # self-contained: the toolchain's headers only
    assert re.search(r"\bint\s+launched\s*\(\s*hipError_t", own)
    naming = {f for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f)) and f.endswith((".hip", ".cpp", ".h", ".inc"))
              and re.search(r'#\s*include\s+"nnr_depth_sparse_kernels\.h"', open(os.path.join(CSRC, f)).read())}
    assert naming == {"nnr_propose_f16.hip", "nnr_sparse_api.cpp"}
    # the dense depth unit is what it was: its own two headers and the shared pass
    dense = re.findall(r'#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, "nnr_depth_f16.hip")).read())
    assert dense == ["nnr_trunk_f16.h", "nnr_fusion_kernels.h", "nnr_density_setup_f16.inc", "nnr_density_pass_f16.inc"]
    api = open(os.path.join(CSRC, "nnr_sparse_api.cpp")).read()
    assert "nnr_layout.h" not in api and "nnr_fusion_kernels.h" not in api


# ------------------------------------------------------------------------------------------------------------ the reference itself
def _rows(R, Cn, seed):
    g = torch.Generator().manual_seed(seed)
    alpha = torch.rand(R, Cn, generator=g, dtype=torch.float64) * 0.2
    z = (1. + 3. * torch.rand(R, Cn, generator=g, dtype=torch.float64)).sort(1)[0]
    return alpha, z


def test_nothing_culled_without_a_threshold_is_fusion_refs_compositing():
    for R, Cn in ((1, 1), (5, 33), (9, 100)):
        alpha, z = _rows(R, Cn, 3)
        live = torch.ones(R, Cn, dtype=torch.bool)
        out, passes, ran = DS.depth_sparse_ref(alpha, z, live, 0.)
        assert bool(ran.all()) and passes.tolist() == [(Cn + 31) // 32] * R
        assert float((out - FR.composite_ref(alpha, z)).abs().max()) <= 1e-14
    # through raw densities: the compositor's alpha
    raw, z = torch.randn(4, 40), _rows(4, 40, 5)[1].float()
    for da, relu in ((False, False), (True, False), (False, True)):
        out, _, _ = DS.from_raw(raw, z, torch.ones(4, 40, dtype=torch.bool), 0., da, relu)
        assert float((out - FR.composite_ref(FR.alpha_ref(raw, z, da, relu), z)).abs().max()) <= 1e-14


def test_all_culled_gives_zero_with_no_pass():
    alpha, z = _rows(6, 40, 7)
    out, passes, ran = DS.depth_sparse_ref(alpha, z, torch.zeros(6, 40, dtype=torch.bool), 1e-3)
    assert not bool(ran.any()) and passes.tolist() == [0] * 6 and bool((out == 0.).all())


def test_a_culled_or_unevaluated_nan_does_not_poison_and_a_live_one_poisons_its_ray_alone():
    alpha, z = _rows(8, 64, 9)
    live = torch.rand(8, 64, generator=torch.Generator().manual_seed(2)) < 0.5
    clean, passes, ran = DS.depth_sparse_ref(alpha, z, live, 0.)
    dirty = torch.where(live, alpha, torch.full_like(alpha, NAN))
    got, _, _ = DS.depth_sparse_ref(dirty, z, live, 0.)
    assert torch.equal(got, clean) and bool(torch.isfinite(got).all())
    j = int(live[5].nonzero()[0])
    dirty[5, j] = NAN
    got, _, _ = DS.depth_sparse_ref(dirty, z, live, 0.)
    assert bool(torch.isnan(got[5]).all()) and torch.equal(got[:5], clean[:5]) and torch.equal(got[6:], clean[6:])
    # behind the stop: every sample opaque, so one pass runs; a NaN in the second pass's part of the list is never evaluated
    opaque = torch.full((4, 64), 0.9, dtype=torch.float64)
    all_live = torch.ones(4, 64, dtype=torch.bool)
    first, passes, ran = DS.depth_sparse_ref(opaque, z[:4], all_live, 1e-3)
    assert passes.tolist() == [1] * 4 and torch.equal(ran, torch.arange(64)[None].expand(4, 64) < 32)
    opaque[2, 40] = NAN
    got, passes, _ = DS.depth_sparse_ref(opaque, z[:4], all_live, 1e-3)
    assert passes.tolist() == [1] * 4 and torch.equal(got, first)
    # in the first pass it is: its carry is NaN, never below the threshold -- its workgroup runs to the end of its list
    opaque[2, 3] = NAN
    got, passes, _ = DS.depth_sparse_ref(opaque, z[:4], all_live, 1e-3)
    assert passes.tolist() == [2] * 4 and bool(torch.isnan(got[2]).all()) and bool(torch.isfinite(got[[0, 1, 3]]).all())


def test_pass_counts_follow_the_workgroups_largest_list_and_the_stop_rule():
    z = _rows(9, 96, 11)[1]
    live = torch.zeros(9, 96, dtype=torch.bool)
    for r, n in enumerate([0, 1, 32, 33, 64, 65, 0, 0, 0]):
        live[r, :n] = True
    thin = torch.full((9, 96), 1e-3, dtype=torch.float64)
    _, passes, ran = DS.depth_sparse_ref(thin, z, live, 1e-3)      # nobody is ever opaque: the largest list of four decides
    assert passes.tolist() == [2] * 4 + [3] * 4 + [0] and torch.equal(ran, live)
    # ray 5 (65 live) is opaque after its first pass, ray 4 (64 live) never: two passes end ray 4's list, ray 5 is done by transmittance
    a = thin.clone()
    a[5] = 0.5
    out, passes, ran = DS.depth_sparse_ref(a, z, live, 1e-3)
    assert passes.tolist() == [2] * 4 + [2] * 4 + [0] and int(ran[5].sum()) == 64 and int(ran[4].sum()) == 64
    # the hand-worked value of a two-sample ray: w_0 = a_0, w_1 = a_1 (1 - a_0 + 1e-6)
    al = torch.tensor([[0.25, 0.5]], dtype=torch.float64)
    zz = torch.tensor([[1., 3.]], dtype=torch.float64)
    out, passes, _ = DS.depth_sparse_ref(al, zz, torch.ones(1, 2, dtype=torch.bool), 0.)
    w1 = 0.5 * (0.75 + 1e-6)
    assert passes.tolist() == [1] and abs(float(out[0, 0]) - (0.25 * 1. + w1 * 3.)) <= 1e-15 and abs(float(out[0, 1]) - (0.25 + w1)) <= 1e-15
    # culling the first: the second stands alone
    out, _, _ = DS.depth_sparse_ref(al, zz, torch.tensor([[False, True]]), 0.)
    assert out.tolist() == [[1.5, 0.5]]
    # what stopping may cost is bounded by the stopped transmittance
    assert ST.stop_bound(1e-3, 256) < 1.001e-3
