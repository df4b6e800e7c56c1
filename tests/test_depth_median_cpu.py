"""CPU: the quantile (median) depth (include/nnr_depth_median.h) without a GPU -- where the two entry points are
declared and listed, every error return of both reached with fake device pointers and host-side outputs that must stay untouched, what the
build lists and checks for the two new units, the reference of tests/depth_median_ref.py on hand-made rows, and render_depth_maps' argument
checks and call pattern on stubs of the renderer and of nnr.ops."""
import ctypes as C
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nope-nerf_amd", "csrc")
for p in ("nope-nerf_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import depth_median_ref as DM        # noqa: E402
import fusion_ref as FR              # noqa: E402

OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3
INF, NAN = float("inf"), float("nan")
SENTINEL = 0x7fc0beef
HEADER = "nnr_depth_median.h"


def _lib():
    from nnr import lib as L
    return L, L.load()


def _build():
    spec = importlib.util.spec_from_file_location("nnr_build_dm", os.path.join(CSRC, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


# ------------------------------------------------------------------------------------------------------------ header and exports
def _params(header, name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return [re.sub(r"\s+", " ", p.strip()) for p in re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, code, flags=re.S).group(1).split(",")]


def test_the_entry_points_live_in_their_own_header_under_abi_8():
    L, lib = _lib()
    inc = os.path.join(ROOT, "include")
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, HEADER)).read(), flags=re.S)
    assert lib.nnr_abi_version() == L.ABI_VERSION == 8 and len(L.EXPORTS) == 50
    assert "NNR_ABI_VERSION" not in code and '#include "nnr.h"' in code
    assert "nnr_fusion.h" not in code and "nnr_depth_sparse.h" not in code
    assert L.DEPTH_MEDIAN_EXPORTS == ("nnr_render_depth_median", "nnr_render_depth_median_sparse")
    # the pinned tuples are what they were
    assert L.FUSION_EXPORTS == ("nnr_render_depth", "nnr_tsdf_integrate") and L.DEPTH_SPARSE_EXPORTS == ("nnr_render_depth_sparse",)
    assert L.SPARSE_EXPORTS == ("nnr_render_sparse",) and L.SPARSE_STOP_EXPORTS == ("nnr_render_sparse_stop",)
    assert L.PROPOSE_SPARSE_EXPORTS == ("nnr_propose_sparse",) and L.GEOMETRY_EXPORTS == ("nnr_density_bricks",)
    others = (L.EXPORTS + L.GEOMETRY_EXPORTS + L.FUSION_EXPORTS + L.SPARSE_EXPORTS + L.SPARSE_STOP_EXPORTS + L.PROPOSE_SPARSE_EXPORTS
              + L.DEPTH_SPARSE_EXPORTS + L.REGULARISE_EXPORTS + L.FROZEN_EXPORTS + L.FROZEN_SPARSE_EXPORTS)
    for name in L.DEPTH_MEDIAN_EXPORTS:
        assert name not in others and hasattr(lib, name)
        for h in sorted(os.listdir(inc)):
            if h != HEADER:
                assert name not in open(os.path.join(inc, h)).read(), h
    protos = dict(re.findall(r"\bint\s+(nnr_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S))
    assert set(protos) == set(L.DEPTH_MEDIAN_EXPORTS)
    # the dense entry: nnr_render_depth's parameters with `level` in front of packed
    dense, parent = _params(HEADER, "nnr_render_depth_median"), _params("nnr_fusion.h", "nnr_render_depth")
    assert len(dense) == len(lib.nnr_render_depth_median.argtypes) == 12
    assert dense[:6] == parent[:6] and dense[6] == "float level" and dense[7:] == parent[6:]
    assert lib.nnr_render_depth_median.argtypes[6] is C.c_float
    # the sparse entry: nnr_render_depth_sparse's parameters with `level` behind t_min
    sparse, parent = _params(HEADER, "nnr_render_depth_median_sparse"), _params("nnr_depth_sparse.h", "nnr_render_depth_sparse")
    assert len(sparse) == len(lib.nnr_render_depth_median_sparse.argtypes) == 19
    assert sparse[:11] == parent[:11] and sparse[10] == "float t_min" and sparse[11] == "float level" and sparse[12:] == parent[11:]
    assert lib.nnr_render_depth_median_sparse.argtypes[10] is C.c_float and lib.nnr_render_depth_median_sparse.argtypes[11] is C.c_float


# ------------------------------------------------------------------------------------------------------------ error returns
PTRS = dict(pts_o=0x10000, pts_d=0x20000, z_lo=0x30000, z_hi=0x40000, jitter=0x50000, bits=0x70000, packed=0x80000)
OUTS = {"dense": ("out", "opt_raw", "opt_z"), "sparse": ("out", "opt_raw", "opt_count", "opt_cell", "opt_passes")}
OPTIONAL = {"dense": ("jitter", "opt_raw", "opt_z"), "sparse": ("jitter", "opt_raw", "opt_count", "opt_cell", "opt_passes")}
BOTH = ("dense", "sparse")


def _call(which, n_rays=5, n_samples=64, hidden=256, flags=None, cfg=True, lo=(-1., -1., -1.), inv=(4., 4., 4.), dims=(8, 8, 8), t_min=1e-3,
          level=0.5, null=(), off=None, **ptrs):
    """One of the two entries with fake device inputs and HOST buffers full of a sentinel as its outputs -> the return code; asserts that no
    output word changed.  null: names passed as NULL; off: {output name: bytes} to misalign an output."""
    L, lib = _lib()
    flags = (L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2) if flags is None else flags
    c = L.Cfg(n_rays, n_samples, hidden, flags)
    a = dict(PTRS)
    a.update(ptrs)
    v = {k: (None if k in null else C.c_void_p(x)) for k, x in a.items()}
    outs = OUTS[which]
    bufs = {k: np.full(64, SENTINEL, dtype=np.int32) for k in outs}
    o = {k: (None if k in null else C.c_void_p(bufs[k].ctypes.data + 64 + (off or {}).get(k, 0))) for k in outs}
    if which == "dense":
        rc = lib.nnr_render_depth_median(C.byref(c) if cfg else None, v["pts_o"], v["pts_d"], v["z_lo"], v["z_hi"], v["jitter"], level, v["packed"],
                                         *[o[k] for k in outs], None)
    else:
        lo3 = None if "lo" in null else (C.c_float * 3)(*lo)
        is3 = None if "inv" in null else (C.c_float * 3)(*inv)
        d3 = None if "dims" in null else (C.c_int32 * 3)(*dims)
        rc = lib.nnr_render_depth_median_sparse(C.byref(c) if cfg else None, v["pts_o"], v["pts_d"], v["z_lo"], v["z_hi"], v["jitter"], lo3, is3, d3,
                                                v["bits"], t_min, level, v["packed"], *[o[k] for k in outs], None)
    assert rc != OK, "a call with fake device pointers must not get as far as a launch"
    for k in outs:
        assert (bufs[k] == SENTINEL).all(), k
    return rc


def _reaches_the_alignment_check(which, **kw):
    """a call that every value check accepts: told apart from a refusal by the one thing still wrong, a `packed` that is 8-byte aligned"""
    return _call(which, packed=0x80008, **kw) == E_ALIGN


@pytest.mark.parametrize("which", BOTH)
def test_bad_sizes_null_pointers_and_levels_are_bad_values(which):
    assert _call(which, cfg=False) == E_BADCFG
    names = ("pts_o", "pts_d", "z_lo", "z_hi", "packed", "out") + (("bits", "lo", "inv", "dims") if which == "sparse" else ())
    for name in names:
        assert _call(which, null=(name,)) == E_BADCFG, name
    for n in (0, -1, -2 ** 31):
        assert _call(which, n_rays=n) == E_BADCFG and _call(which, n_samples=n) == E_BADCFG
    for lv in (0., -0., 1., -1e-9, 1.5, -0.5, NAN, INF, -INF):
        assert _call(which, level=lv, t_min=0.) == E_BADCFG, lv
    for lv in (1e-30, 0.1, 0.5, 0.9, 0.999999):
        assert _reaches_the_alignment_check(which, level=lv, t_min=0.), lv
    assert _reaches_the_alignment_check(which, null=OPTIONAL[which])
    assert _reaches_the_alignment_check(which, n_rays=1, n_samples=1, dims=(1, 1, 1))


def test_the_sparse_entry_refuses_a_threshold_above_the_level_and_the_parents_bad_ones():
    for t in (-1e-9, 1.0, NAN, INF, -INF, -1., 2.):
        assert _call("sparse", t_min=t) == E_BADCFG, t
    for t, lv in ((0.5000001, 0.5), (0.9, 0.5), (0.11, 0.1), (0.999, 0.9)):
        assert _call("sparse", t_min=t, level=lv) == E_BADCFG, (t, lv)
    for t, lv in ((0., 0.5), (1e-3, 0.5), (0.5, 0.5), (0.1, 0.1), (0.9, 0.9), (0.4999999, 0.5)):
        assert _reaches_the_alignment_check("sparse", t_min=t, level=lv), (t, lv)


def test_the_grid_checks_are_the_sparse_depth_renders():
    for n in (0, -1, -2 ** 31):
        for axis in range(3):
            d = [8, 8, 8]
            d[axis] = n
            assert _call("sparse", dims=tuple(d)) == E_BADCFG
    for bad in (INF, -INF, NAN):
        for axis in range(3):
            v = [0.5, 0.5, 0.5]
            v[axis] = bad
            assert _call("sparse", lo=tuple(v)) == E_BADCFG and _call("sparse", inv=tuple(v)) == E_BADCFG
    for s in (0., -0., -1e-3, -4.):
        assert _call("sparse", inv=(4., s, 4.)) == E_BADCFG
    for dims in ((32, 2 ** 16, 2 ** 15), (2 ** 31 - 1,) * 3, (1, 2 ** 16, 2 ** 15), (64, 2 ** 16, 2 ** 10)):      # rows, words or cells past int32
        assert _call("sparse", dims=dims) == E_UNSUPPORTED, dims
    assert _reaches_the_alignment_check("sparse", dims=(1, 2 ** 16, 2 ** 15 - 1))


@pytest.mark.parametrize("which", BOTH)
def test_sizes_widths_and_flags_the_kernels_do_not_have_are_unsupported(which):
    L, _ = _lib()
    s2 = L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    for Cn in (257, 288, 1024, 2 ** 30, 2 ** 31 - 1):
        assert _call(which, n_samples=Cn) == E_UNSUPPORTED, Cn
    assert _reaches_the_alignment_check(which, n_samples=256)
    for h in (64, 192, 512, 0):
        assert _call(which, hidden=h) == E_UNSUPPORTED, h
    assert _reaches_the_alignment_check(which, hidden=128)
    for f in (0, L.NNR_F_SPLIT3, L.NNR_F_SPLIT2, s2 | L.NNR_F_TRAIN, s2 | L.NNR_F_BF16, L.NNR_F_BF16, s2 | L.NNR_F_TRAIN | L.NNR_F_DIST_ALPHA):
        assert _call(which, flags=f) == E_UNSUPPORTED, f
    for f in (s2, s2 | L.NNR_F_DIST_ALPHA, s2 | L.NNR_F_RELU_SIGMA, s2 | L.NNR_F_WHITE_BG, s2 | L.NNR_F_DIST_ALPHA | L.NNR_F_RELU_SIGMA):
        assert _reaches_the_alignment_check(which, flags=f), f


@pytest.mark.parametrize("which", BOTH)
def test_misaligned_pointers_are_refused(which):
    for a in (0x80001, 0x80002, 0x80004, 0x80008, 0x8000c):
        assert _call(which, packed=a) == E_ALIGN, a
    for name in ("pts_o", "pts_d", "z_lo", "z_hi", "jitter") + (("bits",) if which == "sparse" else ()):
        for off in (1, 2, 3):
            assert _call(which, **{name: PTRS[name] + off}) == E_ALIGN, (name, off)
    for name in OUTS[which]:
        for off in (1, 2, 3):
            assert _call(which, off={name: off}) == E_ALIGN, (name, off)


@pytest.mark.parametrize("which", BOTH)
def test_precedence_bad_value_then_unsupported_then_misaligned(which):
    assert _call(which, n_samples=0, hidden=64) == E_BADCFG and _call(which, n_rays=0, n_samples=257) == E_BADCFG
    assert _call(which, null=("z_hi",), n_samples=257) == E_BADCFG
    assert _call(which, level=1.0, n_samples=257) == E_BADCFG and _call(which, level=NAN, hidden=64, packed=0x80004) == E_BADCFG
    assert _call(which, level=0., off={"out": 2}) == E_BADCFG
    assert _call(which, n_samples=257, packed=0x80004) == E_UNSUPPORTED and _call(which, hidden=64, off={"opt_raw": 1}) == E_UNSUPPORTED
    if which == "sparse":
        assert _call(which, null=("bits",), n_samples=257) == E_BADCFG and _call(which, dims=(0, 8, 8), n_samples=257) == E_BADCFG
        assert _call(which, inv=(NAN, 4., 4.), packed=0x80004) == E_BADCFG
        assert _call(which, t_min=0.6, level=0.5, n_samples=257) == E_BADCFG and _call(which, t_min=0.6, level=0.5, packed=0x80004) == E_BADCFG
        assert _call(which, t_min=0.6, level=0.5, dims=(32, 2 ** 16, 2 ** 15)) == E_BADCFG
        assert _call(which, t_min=1.0, level=0.5, hidden=64) == E_BADCFG
        assert _call(which, dims=(32, 2 ** 16, 2 ** 15), off={"opt_cell": 2}) == E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------ the wrappers
def _grid():
    from model import geometry as G
    return G.OccupancyGrid((0., 0., 0.), (1., 1., 1.), (2, 2, 2), torch.zeros(2, 2, 1, dtype=torch.int32))


def test_the_wrappers_refuse_bad_levels_before_anything_else():
    from nnr import ops
    t = torch.zeros(4, 3)
    kw = dict(hidden=128, dist_alpha=False, relu_sigma=False)
    for bad in (0., 1., -0.1, 1.5, NAN, INF, 1e-60):      # (1e-60: its fp32 is 0)
        with pytest.raises(ValueError, match="quantile_level"):
            ops.render_depth(t, t, torch.zeros(8), torch.ones(8), None, [], [], quantile_level=bad, **kw)
        with pytest.raises(ValueError, match="quantile_level"):
            ops.render_depth_sparse(t, t, torch.zeros(8), torch.ones(8), None, _grid(), [], [], quantile_level=bad, **kw)
    with pytest.raises(ValueError, match="t_min.*quantile_level"):
        ops.render_depth_sparse(t, t, torch.zeros(8), torch.ones(8), None, _grid(), [], [], t_min=0.6, quantile_level=0.5, **kw)
    for level in (None, 0.5):      # a good level, or none: the parent's refusal of CPU tensors
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.render_depth(t, t, torch.zeros(8), torch.ones(8), None, [], [], quantile_level=level, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.render_depth_sparse(t, t, torch.zeros(8), torch.ones(8), None, _grid(), [], [], t_min=0.5 if level else 0., quantile_level=level, **kw)


# ------------------------------------------------------------------------------------------------------------ the build
DENSE_ENTRY = ("nnr_depth_f16.hip", ("NNR_DEPTH_MEDIAN=1",))
SPARSE_ENTRY = ("nnr_propose_f16.hip", ("NNR_PROPOSE_SPARSE=1", "NNR_PROPOSE_DEPTH=2"))
MANGLED = ("_ZN3nnr23depth_median_f16_kernelILi%dEEEvNS_15DepthMedianArgsE", "_ZN3nnr30depth_sparse_median_f16_kernelILi%dEEEvNS_21DepthSparseMedianArgsE")
REMARK = "remark: Function Name: %s\nremark:     ScratchSize [bytes/lane]: %d\n"


def test_sources_holds_the_two_new_entries_once_with_objects_of_their_own():
    b = _build()
    for entry in (DENSE_ENTRY, SPARSE_ENTRY):
        assert b.SOURCES.count(entry) == 1, entry
    for old in (("nnr_depth_f16.hip", ()), ("nnr_propose_f16.hip", ()), ("nnr_propose_f16.hip", ("NNR_PROPOSE_SPARSE=1",)),
                ("nnr_propose_f16.hip", ("NNR_PROPOSE_SPARSE=1", "NNR_PROPOSE_DEPTH=1"))):
        assert b.SOURCES.count(old) == 1, old
    names = [b._obj_name(s, d) for s, d in b.SOURCES]
    assert len(set(names)) == len(names)
    assert len({b._obj_name(*e) for e in (DENSE_ENTRY, SPARSE_ENTRY, ("nnr_depth_f16.hip", ()),
                                          ("nnr_propose_f16.hip", ("NNR_PROPOSE_SPARSE=1", "NNR_PROPOSE_DEPTH=1")))}) == 4
    assert len({s for s, _ in b.SOURCES}) == 31      # no new source file
    text = open(os.path.join(CSRC, "nnr_propose_f16.hip")).read()
    assert re.search(r"#if NNR_PROPOSE_DEPTH && !NNR_PROPOSE_SPARSE\s*\n#error", text)


def test_the_build_holds_the_two_kernels_to_no_scratch():
    b = _build()
    assert b.SCRATCH_LIMIT["23depth_median_f16_kernelI"] == 0 and b.SCRATCH_LIMIT["30depth_sparse_median_f16_kernelI"] == 0
    assert b.SCRATCH_LIMIT["16depth_f16_kernelI"] == 0 and b.SCRATCH_LIMIT["23depth_sparse_f16_kernelI"] == 0
    for mangled in MANGLED:
        for D in (128, 256):
            b.check_resources(REMARK % (mangled % D, 0), "test")
            for size in (1, 16):
                with pytest.raises(RuntimeError, match="scratch"):
                    b.check_resources(REMARK % (mangled % D, size), "test")


def test_the_argument_blocks_sit_in_the_parents_headers():
    b = _build()
    sources = {s for s, _ in b.SOURCES}

    def users(path):
        return {src for src in sources if any(os.path.samefile(d, path) for d in b.deps(src))}

    assert "struct DepthMedianArgs" in open(os.path.join(CSRC, "nnr_fusion_kernels.h")).read()
    assert "struct DepthSparseMedianArgs" in open(os.path.join(CSRC, "nnr_depth_sparse_kernels.h")).read()
    assert users(os.path.join(CSRC, "nnr_fusion_kernels.h")) == {"nnr_depth_f16.hip", "nnr_tsdf.hip", "nnr_fusion_api.cpp"}
    assert users(os.path.join(CSRC, "nnr_depth_sparse_kernels.h")) == {"nnr_propose_f16.hip", "nnr_sparse_api.cpp"}
    assert users(os.path.join(ROOT, "include", HEADER)) == {"nnr_fusion_api.cpp", "nnr_sparse_api.cpp"}


# ------------------------------------------------------------------------------------------------------------ the reference itself
def _row(alpha, z, level, mask=None):
    a = torch.tensor([alpha], dtype=torch.float64)
    zz = torch.tensor([z], dtype=torch.float64)
    mk = torch.ones_like(a, dtype=torch.bool) if mask is None else torch.tensor([mask])
    return DM.quantile_ref(a, zz, mk, level)


def test_the_two_surface_row_has_its_expected_depth_in_the_air_and_its_median_on_the_wall():
    """40 % of the weight on an edge at z = 1, the rest on a wall at z = 3 (the closing sample takes everything that is left)"""
    alpha, z = [0., 0.4, 0., 0., 1.], [0.5, 1.0, 2.0, 3.0, 3.0]
    expected = FR.composite_ref(torch.tensor([alpha]), torch.tensor([z]))[0]
    assert abs(float(expected[0]) - 2.2) < 1e-5 and abs(float(expected[1]) - 1.) < 1e-5
    r = _row(alpha, z, 0.5)
    assert int(r["m"]) == 4 and float(r["q"]) == 3.0                       # the wall; its z_next is z_m: the last sample
    r = _row(alpha, z, 0.7)                                                # the 30 % quantile lies on the edge: between samples 1 and 2
    assert int(r["m"]) == 1 and 1.0 <= float(r["q"]) <= 2.0
    T1, T2 = 1. + 1e-6, (1. + 1e-6) * (0.6 + 1e-6)
    assert abs(float(r["q"]) - (1.0 + 1.0 * (T1 - 0.7) / (T1 - T2))) < 1e-12
    assert not 1.0 <= float(expected[0]) <= 1.0 + 1e-9 and not float(expected[0]) >= 3.0      # the expected depth is on neither surface


@pytest.mark.parametrize("level", [0.1, 0.5, 0.9])
def test_crossings_at_the_first_and_the_last_sample_and_none(level):
    z = [1., 2., 4.]
    r = _row([0.95, 0.5, 0.5], z, level)                                   # sample 0 crosses every level
    assert int(r["m"]) == 0 and float(r["T0"]) == 1.0
    assert abs(float(r["q"]) - (1. + 1. * (1. - level) / (1. - (0.05 + 1e-6)))) < 1e-12
    r = _row([0., 0., 0.95], z, level)                                     # the last sample: z_next = z_m
    assert int(r["m"]) == 2 and float(r["q"]) == 4.0 and float(r["gap"]) == 0.0
    r = _row([0.01, 0.01, 0.01], z, level)                                 # no crossing
    assert int(r["m"]) == -1 and float(r["q"]) == INF
    r = _row([0.3, 0.3, 0.3], z, level)                                    # T = 0.7, 0.49, 0.343: the first boundary below the level
    want = {0.9: 0, 0.5: 1, 0.1: -1}[level]
    assert int(r["m"]) == want and (want >= 0 or float(r["q"]) == INF)


@pytest.mark.parametrize("level", [0.1, 0.5, 0.9])
def test_a_nan_in_front_of_the_crossing_is_nan_and_behind_it_nothing(level):
    z = [1., 2., 3., 4.]
    clean = _row([0.2, 0.95, 0.5, 0.5], z, level)
    assert int(clean["m"]) in (0, 1)
    behind = _row([0.2, 0.95, NAN, 0.5], z, level)
    assert float(behind["q"]) == float(clean["q"]) and int(behind["m"]) == int(clean["m"])
    front = _row([NAN, 0.95, 0.5, 0.5], z, level)
    assert int(front["m"]) == -1 and np.isnan(float(front["q"]))
    # a sample that is not evaluated is absent: its NaN does not count, its depth still is the next sample's
    masked = _row([NAN, 0.95, 0.5, 0.5], z, level, mask=[False, True, True, True])
    assert int(masked["m"]) == 1 and abs(float(masked["q"]) - (2. + 1. * (1. - level) / (1. - (0.05 + 1e-6)))) < 1e-12
    culled_next = _row([0.95, 0.5, 0.5, 0.5], z, level, mask=[True, False, True, True])
    assert int(culled_next["m"]) == 0 and float(culled_next["gap"]) == 1.0      # z_next: sample 1 of the original row, culled or not


def test_the_error_terms_are_small_positive_and_flag_a_boundary_at_the_level():
    g = torch.Generator().manual_seed(5)
    alpha = torch.rand(64, 100, generator=g, dtype=torch.float64) * 0.2
    z = torch.linspace(1., 4., 100, dtype=torch.float64)[None].expand(64, 100)
    mask = torch.ones(64, 100, dtype=torch.bool)
    ref = DM.quantile_ref(alpha, z, mask, 0.5)
    E, kappa, near = DM.error_terms(alpha, mask, ref, 0.5)
    assert bool((ref["m"] >= 0).all()) and bool((E > 0).all()) and float(E.max()) < 1e-4
    assert bool((kappa > 0).all()) and bool(torch.isfinite(kappa).all()) and float(kappa.max()) < 1e-2 and int(near.sum()) <= 1
    hit = DM.quantile_ref(alpha, z, mask, float(ref["T"][3, 20]) * (1. + 1e-9))      # a level a hair above a boundary of ray 3
    assert bool(DM.error_terms(alpha, mask, hit, float(ref["T"][3, 20]) * (1. + 1e-9))[2][3])


def test_the_fallback_formula_is_the_reference_with_every_sample_evaluated():
    from model import geometry as G
    g = torch.Generator().manual_seed(9)
    alpha = torch.rand(40, 300, generator=g, dtype=torch.float64) * 0.05
    alpha[7] = 0.                                                          # never crosses
    alpha[9, 4] = NAN                                                      # NaN in front of every crossing
    z = torch.linspace(0.5, 6., 300, dtype=torch.float64)
    for level in (0.1, 0.5, 0.9):
        ref = DM.quantile_ref(alpha, z[None].expand(40, 300), torch.ones(40, 300, dtype=torch.bool), level)["q"]
        for fn in (G.quantile_depth, DM.torch_quantile):
            got = fn(alpha, z, level)
            assert float(got[7]) == INF and np.isnan(float(got[9]))
            ok = torch.isfinite(ref)
            assert torch.equal(torch.isfinite(got), ok) and float((got[ok] - ref[ok]).abs().max()) < 1e-12
        got32 = G.quantile_depth(alpha.float(), z.float(), level)
        assert got32.dtype == torch.float32 and float(got32[7]) == INF


# ------------------------------------------------------------------------------------------------------------ render_depth_maps on stubs
class _FakeWeight:
    is_cuda = True
    device = torch.device("cpu")


def _stub_renderer(n_samples=16, normalise=True):
    cfg = {'sample_option': 'uniform', 'num_points': n_samples, 'outside_steps': 0, 'normalise_ray': normalise, 'use_ray_dir': True,
           'dist_alpha': False}
    net = types.SimpleNamespace(weights=lambda: [_FakeWeight()], biases=lambda: [_FakeWeight()], hidden_dim=128, occ_activation='softplus')
    z = torch.linspace(1., 4., n_samples)
    return types.SimpleNamespace(cfg=cfg, model=net, depth_range=(1., 4.), _z_tables=lambda n, near, far, strat, dev: (z, z.clone()))


class _Ops:
    """a call-recording stand-in for nnr.ops' two depth operators: (R,2) or (R,3) of recognisable values"""
    def __init__(self):
        self.calls = []

    def _out(self, name, o, kw):
        self.calls.append((name, int(o.shape[0]), dict(kw)))
        R = o.shape[0]
        cols = [torch.full((R,), 2.), torch.linspace(0., 1., R), torch.where(torch.arange(R) % 3 == 0, torch.full((R,), INF), torch.full((R,), 3.))]
        return torch.stack(cols[:3 if kw.get("quantile_level") is not None else 2], 1)

    def render_depth(self, o, d, z_lo, z_hi, jit, w, b, **kw):
        return self._out("dense", o, kw)

    def render_depth_sparse(self, o, d, z_lo, z_hi, jit, grid, w, b, **kw):
        return self._out("sparse", o, kw)


def _stubbed(monkeypatch):
    from model import geometry as G
    from nnr import camera
    ops = _Ops()
    monkeypatch.setattr(G, "_nnr_ops", ops)

    def ray_setup(pixels, depth, K, Wm, S, normalise, use_dir):
        R = pixels.shape[1]
        return torch.zeros(R, 3), torch.ones(R, 3), torch.ones(R, 3), torch.full((R,), 2.), None, None
    monkeypatch.setattr(camera, "ray_setup", ray_setup)
    return G, ops


def test_render_depth_maps_checks_its_median_arguments_before_any_device_work():
    from model import geometry as G
    renderer, eye = _stub_renderer(), torch.eye(4)
    for bad in (0., 1., -0.1, 1.5, NAN):
        with pytest.raises(ValueError, match="min_acc"):
            G.render_depth_maps(renderer, eye, eye[None], (2, 2), min_acc=bad, depth_mode='median')
    with pytest.raises(ValueError, match="t_min.*level"):
        G.render_depth_maps(renderer, eye, eye[None], (2, 2), occupancy=_grid(), t_min=0.6, depth_mode='median')
    with pytest.raises(ValueError, match="t_min.*level"):
        G.render_depth_maps(renderer, eye, eye[None], (2, 2), min_acc=0.9, occupancy=_grid(), t_min=0.2, depth_mode='median')
    with pytest.raises(ValueError, match="t_min.*occupancy"):      # without a grid t_min != 0 raises as it does in expected mode
        G.render_depth_maps(renderer, eye, eye[None], (2, 2), t_min=1e-3, depth_mode='median')
    with pytest.raises(ValueError, match="depth_mode"):
        G.render_depth_maps(renderer, eye, eye[None], (2, 2), depth_mode='mode')
    assert G.median_level(0.5) == 0.5 and G.median_level(0.9) == float(np.float32(1. - 0.9))
    renderer.cfg['sample_option'] = 'ndc'
    with pytest.raises(NotImplementedError, match="ndc"):
        G.render_depth_maps(renderer, eye, eye[None], (2, 2), depth_mode='median')


def test_expected_mode_makes_exactly_todays_calls(monkeypatch):
    G, ops = _stubbed(monkeypatch)
    renderer, eye, grid = _stub_renderer(), torch.eye(4), _grid()
    today = dict(hidden=128, dist_alpha=False, relu_sigma=False)
    for kw in ({}, dict(depth_mode='expected')):
        ops.calls.clear()
        maps = G.render_depth_maps(renderer, eye, torch.stack([eye, eye]), (3, 4), chunk=8, **kw)
        assert ops.calls == [("dense", 8, today), ("dense", 4, today)] * 2
        acc = torch.linspace(0., 1., 8)
        assert torch.equal(maps[0].view(-1)[:8], torch.where(acc < 0.5, torch.full((8,), INF), torch.full((8,), 1.)))      # 2 / ray_norm
        ops.calls.clear()
        G.render_depth_maps(renderer, eye, eye[None], (3, 4), occupancy=grid, t_min=1e-3, **kw)
        assert ops.calls == [("sparse", 12, dict(today, t_min=1e-3))]
        ops.calls.clear()
        G.render_depth_maps(renderer, eye, eye[None], (3, 4), occupancy=grid, **kw)
        assert ops.calls == [("sparse", 12, dict(today, t_min=0.))]


def test_median_mode_asks_for_the_level_and_stops_there_by_default(monkeypatch):
    G, ops = _stubbed(monkeypatch)
    renderer, eye, grid = _stub_renderer(), torch.eye(4), _grid()
    today = dict(hidden=128, dist_alpha=False, relu_sigma=False)
    maps = G.render_depth_maps(renderer, eye, eye[None], (3, 4), depth_mode='median')
    assert ops.calls == [("dense", 12, dict(today, quantile_level=0.5))]
    want = torch.where(torch.arange(12) % 3 == 0, torch.full((12,), INF), torch.full((12,), 1.5))      # q / ray_norm; +inf stays
    assert torch.equal(maps.view(-1), want)
    renderer.cfg['normalise_ray'] = False
    assert torch.equal(G.render_depth_maps(renderer, eye, eye[None], (3, 4), depth_mode='median').view(-1), 2. * want)
    renderer.cfg['normalise_ray'] = True
    level9 = float(np.float32(1. - 0.1))
    for kw, t, level in ((dict(), 0.5, 0.5), (dict(t_min=1e-3), 1e-3, 0.5), (dict(t_min=0.), 0., 0.5), (dict(t_min=0.5), 0.5, 0.5),
                         (dict(min_acc=0.1), level9, level9)):
        ops.calls.clear()
        G.render_depth_maps(renderer, eye, eye[None], (3, 4), occupancy=grid, depth_mode='median', **kw)
        assert ops.calls == [("sparse", 12, dict(today, t_min=t, quantile_level=level))], kw


def test_extract_mesh_tsdf_passes_the_mode_on(monkeypatch):
    from model import geometry as G
    seen = []

    def maps(renderer, K, Wm, size, **kw):
        seen.append(kw)
        raise KeyboardInterrupt      # (the call is what is under test)
    monkeypatch.setattr(G, "render_depth_maps", maps)
    net = types.SimpleNamespace(weights=lambda: [_FakeWeight()])
    cams = G.Cameras(torch.eye(4), torch.eye(4)[None], (2, 2))
    for kw in (dict(), dict(depth_mode='median'), dict(depth_mode='median', occupancy=_grid(), t_min=0.1, min_acc=0.3)):
        with pytest.raises(KeyboardInterrupt):
            G.extract_mesh_tsdf(types.SimpleNamespace(model=net), cams, (-1.,) * 3, (1.,) * 3, 8, **kw)
    assert "depth_mode" not in seen[0] and seen[0]["t_min"] is None and seen[0]["occupancy"] is None and seen[0]["min_acc"] == 0.5
    assert seen[1]["depth_mode"] == 'median' and seen[1]["t_min"] is None
    assert seen[2]["depth_mode"] == 'median' and seen[2]["t_min"] == 0.1 and seen[2]["min_acc"] == 0.3 and seen[2]["occupancy"] is not None


def test_the_fallback_branch_above_256_samples_is_the_torch_formula(monkeypatch):
    import nnr
    G, ops = _stubbed(monkeypatch)
    renderer, eye = _stub_renderer(300, normalise=False), torch.eye(4)
    g = torch.Generator().manual_seed(3)
    alpha = torch.rand(12, 300, generator=g) * 0.05

    def render_rays(o, d, v, z_lo, z_hi, jit, w, b, **kw):
        assert kw["samples"] is True and kw["white_bg"] is False
        return None, torch.zeros(o.shape[0]), alpha[:o.shape[0]], None
    monkeypatch.setattr(nnr, "render_rays", render_rays)
    maps = G.render_depth_maps(renderer, eye, eye[None], (3, 4), depth_mode='median')
    assert ops.calls == []
    assert torch.equal(maps.view(-1), DM.torch_quantile(alpha, torch.linspace(1., 4., 300), 0.5))


@pytest.mark.parametrize("argv,said", [(["--depth-mode", "median"], "--method tsdf"),
                                       (["--method", "tsdf", "--depth-mode", "median", "--min-acc", "1.0"], "--min-acc"),
                                       (["--method", "tsdf", "--depth-mode", "mode"], "--depth-mode")])
def test_the_mesh_tools_argument_errors_fire(argv, said, monkeypatch, capsys):
    import extract_mesh
    monkeypatch.setattr(sys, "argv", ["extract_mesh.py", "no_such_config.yaml"] + argv)
    with pytest.raises(SystemExit) as e:
        extract_mesh.main()
    assert e.value.code == 2 and said in capsys.readouterr().err
