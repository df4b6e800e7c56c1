"""CPU: the stopping sparse inference render (include/nnr_sparse_stop.h) without a GPU -- where the entry point is
declared and listed, every error return reached with fake device pointers and host-side outputs that must stay untouched (every refusal of
nnr_render_sparse with that function's code, the bad t_min kinds, the precedence), the wrapper's refusals, and the float64 reference of
tests/sparse_stop_ref.py itself: t_min = 0 is the masked compositing, what stopping costs is within the bound, the pass counts of
hand-written cases."""
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

import sparse_ref as SR           # noqa: E402
import sparse_stop_ref as ST      # noqa: E402
from test_sparse_cpu import _random_rows      # noqa: E402  (the rows the sparse reference is tested on)

OK, E_BADCFG, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3
INF, NAN = float("inf"), float("nan")
SENTINEL = 0x7fc0beef


def _lib():
    from nnr import lib as L
    return L, L.load()


# ------------------------------------------------------------------------------------------------------------ header and exports
def test_the_entry_point_lives_in_its_own_header_under_abi_8():
    L, lib = _lib()
    inc = os.path.join(ROOT, "include")
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nnr_sparse_stop.h")).read(), flags=re.S)
    assert lib.nnr_abi_version() == L.ABI_VERSION == 8
    assert "NNR_ABI_VERSION" not in code and '#include "nnr_sparse.h"' in code
    assert L.SPARSE_STOP_EXPORTS == ("nnr_render_sparse_stop",)
    assert L.SPARSE_EXPORTS == ("nnr_render_sparse",) and len(L.EXPORTS) == 50
    others = (L.EXPORTS + L.GEOMETRY_EXPORTS + L.FUSION_EXPORTS + L.SPARSE_EXPORTS + L.REGULARISE_EXPORTS + L.FROZEN_EXPORTS
              + L.FROZEN_SPARSE_EXPORTS)
    for name in L.SPARSE_STOP_EXPORTS:
        assert name not in others and hasattr(lib, name)
        for h in sorted(os.listdir(inc)):
            if h != "nnr_sparse_stop.h":
                assert name not in open(os.path.join(inc, h)).read(), h
    protos = dict(re.findall(r"\bint\s+(nnr_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S))
    assert set(protos) == set(L.SPARSE_STOP_EXPORTS)
    params = [p.strip() for p in protos["nnr_render_sparse_stop"].split(",")]
    assert len(params) == len(lib.nnr_render_sparse_stop.argtypes) == 19
    assert params[12] == "float t_min" and params[11].endswith("packed") and params[17] == "int32_t* opt_passes" and params[16].endswith("opt_out4")
    assert lib.nnr_render_sparse_stop.argtypes[12] is C.c_float
    # the parent's parameters, in its order, around the two additions
    parent = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nnr_sparse.h")).read(), flags=re.S)
    pp = [p.strip() for p in re.search(r"\bint\s+nnr_render_sparse\s*\(([^;{]*?)\)\s*;", parent, flags=re.S).group(1).split(",")]
    assert params[:12] + params[13:17] + params[18:] == pp and len(pp) == 17


# ------------------------------------------------------------------------------------------------------------ error returns
PTRS = dict(pts_o=0x10000, pts_d=0x20000, view_d=0x30000, z_lo=0x40000, z_hi=0x50000, jitter=0x60000, bits=0x70000, packed=0x80000)
OUTS = ("out", "opt_count", "opt_cell", "opt_out4", "opt_passes")


def _call(entry, n_rays=5, n_samples=64, hidden=256, flags=None, cfg=True, lo=(-1., -1., -1.), inv=(4., 4., 4.), dims=(8, 8, 8), null=(), off=None,
          t_min=1e-3, **ptrs):
    """`entry` ("stop" or "parent") with fake device inputs and HOST buffers full of a sentinel as its outputs -> the return code; asserts
    that no output word changed.  null: names passed as NULL; off: {output name: bytes} to misalign an output."""
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
    head = (C.byref(c) if cfg else None, v["pts_o"], v["pts_d"], v["view_d"], v["z_lo"], v["z_hi"], v["jitter"], lo3, is3, d3, v["bits"], v["packed"])
    if entry == "stop":
        rc = lib.nnr_render_sparse_stop(*head, t_min, o["out"], o["opt_count"], o["opt_cell"], o["opt_out4"], o["opt_passes"], None)
    else:
        rc = lib.nnr_render_sparse(*head, o["out"], o["opt_count"], o["opt_cell"], o["opt_out4"], None)
    assert rc != OK, "a call with fake device pointers must not get as far as a launch"
    for k in OUTS:
        assert (bufs[k] == SENTINEL).all(), k
    return rc


def _stop(**kw):
    return _call("stop", **kw)


def _parent_refusals():
    """every kind of call tests/test_sparse_cpu.py makes of the parent entry, as keyword sets"""
    from nnr import lib as L
    s2 = L.NNR_F_SPLIT3 | L.NNR_F_SPLIT2
    calls = [dict(cfg=False)]
    calls += [dict(null=(name,)) for name in ("pts_o", "pts_d", "view_d", "z_lo", "z_hi", "bits", "packed", "out", "lo", "inv", "dims")]
    for n in (0, -1, -2 ** 31):
        calls += [dict(n_rays=n), dict(n_samples=n)]
        for axis in range(3):
            d = [8, 8, 8]
            d[axis] = n
            calls.append(dict(dims=tuple(d)))
    calls += [dict(null=("jitter", "opt_count", "opt_cell", "opt_out4"), packed=0x80008), dict(n_rays=1, n_samples=1, dims=(1, 1, 1), packed=0x80008)]
    for bad in (INF, -INF, NAN):
        for axis in range(3):
            v = [0.5, 0.5, 0.5]
            v[axis] = bad
            calls += [dict(lo=tuple(v)), dict(inv=tuple(v))]
    for s in (0., -0., -1e-3, -4.):
        for axis in range(3):
            v = [4., 4., 4.]
            v[axis] = s
            calls.append(dict(inv=tuple(v)))
    calls.append(dict(inv=(1e-30, 1e30, 4.), packed=0x80008))
    calls += [dict(n_samples=257), dict(n_samples=2 ** 31 - 1), dict(n_samples=256, packed=0x80004), dict(hidden=128, packed=0x80004)]
    calls += [dict(hidden=h) for h in (64, 192, 512, 0)]
    calls += [dict(flags=f) for f in (0, L.NNR_F_SPLIT3, L.NNR_F_SPLIT2, s2 | L.NNR_F_TRAIN, s2 | L.NNR_F_BF16, L.NNR_F_BF16,
                                      s2 | L.NNR_F_TRAIN | L.NNR_F_WHITE_BG)]
    calls += [dict(flags=f, packed=0x80008) for f in (s2, s2 | L.NNR_F_DIST_ALPHA, s2 | L.NNR_F_RELU_SIGMA, s2 | L.NNR_F_WHITE_BG,
                                                      s2 | L.NNR_F_DIST_ALPHA | L.NNR_F_WHITE_BG)]
    calls += [dict(dims=(32, 2 ** 16, 2 ** 15)), dict(dims=(2 ** 31 - 1,) * 3), dict(dims=(1, 2 ** 16, 2 ** 15)),
              dict(dims=(1, 2 ** 16, 2 ** 15 - 1), packed=0x80008), dict(dims=(64, 2 ** 16, 2 ** 10))]
    calls += [dict(n_samples=257, dims=(0, 8, 8)), dict(n_samples=257, packed=0x80004)]
    calls += [dict(packed=a) for a in (0x80001, 0x80002, 0x80004, 0x80008, 0x8000c)]
    calls += [dict(**{name: PTRS[name] + off}) for name in ("pts_o", "pts_d", "view_d", "z_lo", "z_hi", "jitter", "bits") for off in (1, 2, 3)]
    calls += [dict(off={name: off}) for name in OUTS[:4] for off in (1, 2, 3)]
    return calls


def test_every_refusal_of_the_parent_comes_back_with_the_parents_code():
    calls = _parent_refusals()
    seen = set()
    for kw in calls:
        want = _call("parent", **kw)
        seen.add(want)
        for t in (0., 1e-3, 0.5):
            assert _stop(t_min=t, **kw) == want, (kw, t)
    assert seen == {E_BADCFG, E_UNSUPPORTED, E_ALIGN} and len(calls) > 120


@pytest.mark.parametrize("bad", [NAN, -1e-3, -0.5, -INF, 1., 1.5, INF])
def test_a_t_min_that_is_nan_negative_or_not_below_one_is_a_bad_value(bad):
    assert _stop(t_min=bad) == E_BADCFG
    assert _stop(t_min=bad, null=("jitter", "opt_count", "opt_cell", "opt_out4", "opt_passes")) == E_BADCFG


def test_the_edges_of_the_t_min_range_pass_the_value_check():
    below_one = float(np.nextafter(np.float32(1.), np.float32(0.)))
    for t in (0., -0., 1e-30, 1e-3, below_one):
        assert _stop(t_min=t, packed=0x80008) == E_ALIGN, t      # such a call reaches the alignment check


def test_precedence_bad_value_then_unsupported_then_misaligned():
    # a bad t_min beats an unsupported cfg and a misaligned pointer; an unsupported cfg beats a misaligned opt_passes
    assert _stop(t_min=NAN, n_samples=257) == E_BADCFG and _stop(t_min=1., hidden=64) == E_BADCFG
    assert _stop(t_min=-1., packed=0x80004) == E_BADCFG and _stop(t_min=NAN, off={"opt_passes": 2}) == E_BADCFG
    assert _stop(t_min=2., dims=(64, 2 ** 16, 2 ** 10)) == E_BADCFG
    assert _stop(n_samples=257, off={"opt_passes": 1}) == E_UNSUPPORTED and _stop(n_samples=257, packed=0x80004) == E_UNSUPPORTED
    assert _stop(dims=(32, 2 ** 16, 2 ** 15), off={"opt_passes": 1}) == E_UNSUPPORTED
    assert _stop(n_samples=257, dims=(0, 8, 8)) == E_BADCFG


def test_a_misaligned_opt_passes_is_refused_and_a_null_one_is_not():
    for off in (1, 2, 3):
        assert _stop(off={"opt_passes": off}) == E_ALIGN, off
    assert _stop(null=("opt_passes",), packed=0x80008) == E_ALIGN      # (null passes: the call gets as far as `packed`)


def test_the_wrapper_refuses_cpu_tensors_and_bad_values():
    from nnr import ops
    from model import geometry as G
    t = torch.zeros(4, 3)
    grid = G.OccupancyGrid((0., 0., 0.), (1., 1., 1.), (2, 2, 2), torch.zeros(2, 2, 1, dtype=torch.int32))
    kw = dict(hidden=128, dist_alpha=False, white_bg=False, relu_sigma=False)
    for t_min in (0., 1e-3):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.render_sparse(t, t, t, torch.zeros(8), torch.ones(8), None, grid, [], [], t_min=t_min, **kw)
    for bad in (NAN, -1e-3, 1., 2., INF, -INF):
        with pytest.raises(ValueError, match="t_min"):
            ops.render_sparse(t, t, t, torch.zeros(8), torch.ones(8), None, grid, [], [], t_min=bad, **kw)


# ------------------------------------------------------------------------------------------------------------ the reference itself
def test_t_min_zero_is_the_masked_compositing():
    alpha, rgb, z, g = _random_rows(203, 70, 3)      # 203 rays: a short last workgroup; 70 samples: three passes, the last of 6
    live = torch.rand(203, 70, generator=g) < 0.7
    live[:4] = False
    T, n_live = ST.boundaries(alpha, live)
    assert tuple(T.shape) == (203, 3) and torch.equal(n_live, live.sum(1))
    P = ST.passes_ref(T, n_live, 0., 203)
    for g0 in range(0, 203, 4):
        assert P[g0:g0 + 4].tolist() == [int((n_live[g0:g0 + 4].max() + 31) // 32)] * len(P[g0:g0 + 4])
    assert P[:4].tolist() == [0] * 4
    ran = ST.ran_mask(live, P)
    assert torch.equal(ran, live)
    for white in (False, True):
        assert torch.equal(SR.composite_masked(alpha, rgb, z, ran, white), SR.composite_masked(alpha, rgb, z, live, white))
    # the boundaries are the running product of the compositing at the pass ends
    fac = torch.where(live, 1. - alpha + 1e-6, torch.ones_like(alpha))
    for r in (4, 17, 202):
        idx = SR.compact_ref(live[r])
        for p in range(3):
            want = float(torch.prod(fac[r, idx[:32 * (p + 1)]]))
            assert abs(float(T[r, p]) - want) <= 1e-12 * want + 1e-300


def test_what_stopping_costs_is_within_the_bound():
    n_rows, n = 4000, 64
    alpha, rgb, z, g = _random_rows(n_rows, n, 11)
    alpha[torch.rand(n_rows, n, generator=g) < 0.15] *= 1e-3      # translucent stretches: rays that are still alive after a pass
    live = (torch.rand(n_rows, n, generator=g) < 0.8)
    T, n_live = ST.boundaries(alpha, live)
    full = {w: SR.composite_masked(alpha, rgb, z, live, w) for w in (False, True)}
    worst, stopped = 0., 0
    slack = 64 * 2. ** -52 * 7.      # float64 rounding of two sums of 64 terms, each partial sum below 7 (z < 6.1): far below any loss that counts
    for t_min in (1e-4, 1e-2, 0.3):
        P = ST.passes_ref(T, n_live, t_min, n_rows)
        ran = ST.ran_mask(live, P)
        T_stop = torch.where(P > 0, T[torch.arange(n_rows), (P - 1).clamp(min=0)], torch.ones(n_rows, dtype=torch.float64))
        bound = ST.stop_bound(T_stop, n)
        lost = (live & ~ran).any(1)
        stopped += int(lost.sum())
        # a ray that lost samples was done by transmittance, or its workgroup would have gone on
        assert bool((T_stop[lost] < t_min).all())
        for white in (False, True):
            err = (SR.composite_masked(alpha, rgb, z, ran, white) - full[white]).abs()
            assert bool((err[:, :3] <= bound[:, None] + slack).all()) and bool((err[:, 4] <= bound + slack).all()), (t_min, white)
            assert bool((err[:, 3] <= bound * z.max(1)[0] + slack).all())
            assert bool((err[~lost] == 0).all())
            worst = max(worst, float(err.max()))
    assert stopped > 100 and worst > 1e-4, "stopping never cost anything: the bound was not tested (%d rays, worst %.3e)" % (stopped, worst)


def _rows(counts, T_rows):
    n_live = torch.tensor(counts)
    T = torch.tensor(T_rows, dtype=torch.float64)
    return T, n_live


def test_pass_counts_of_hand_written_workgroups():
    o = 0.5      # "still transparent"
    # a wave with an empty list beside full ones: done from the start, the others decide
    T, n = _rows([0, 96, 96, 96], [[1., 1., 1.], [o, 1e-5, 1e-9], [o, o, 1e-9], [1e-5, 1e-9, 1e-9]])
    assert ST.passes_ref(T, n, 1e-3, 4).tolist() == [3] * 4
    assert ST.passes_ref(T, n, 0.6, 4).tolist() == [1] * 4
    assert ST.passes_ref(T, n, 0., 4).tolist() == [3] * 4
    # all done after pass 0, by transmittance or by exhaustion (32 live samples are exhausted after one pass, 33 are not)
    T, n = _rows([96, 32, 7, 96], [[1e-4, 0., 0.], [o, o, o], [o, o, o], [9e-4, 0., 0.]])
    assert ST.passes_ref(T, n, 1e-3, 4).tolist() == [1] * 4
    T, n = _rows([96, 33, 7, 96], [[1e-4, 0., 0.], [o, o, o], [o, o, o], [9e-4, 0., 0.]])
    assert ST.passes_ref(T, n, 1e-3, 4).tolist() == [2] * 4
    # the comparison is strict
    T, n = _rows([64, 64, 64, 64], [[1e-3, 0.]] * 4)
    assert ST.passes_ref(T, n, 1e-3, 4).tolist() == [2] * 4
    # one slow ray holds its workgroup, and only its own: two workgroups
    T, n = _rows([96] * 8, [[1e-6, 0., 0.]] * 3 + [[o, o, 1e-9]] + [[1e-6, 0., 0.]] * 4)
    assert ST.passes_ref(T, n, 1e-3, 8).tolist() == [3] * 4 + [1] * 4
    # a NaN carry is never done by transmittance: it ends by exhaustion
    T, n = _rows([96, 96, 96, 40], [[1e-6, 0., 0.]] * 3 + [[NAN, NAN, NAN]])
    assert ST.passes_ref(T, n, 1e-3, 4).tolist() == [2] * 4
    # R % 4 != 0: the short last workgroup repeats ray R - 1, which therefore only counts once
    T, n = _rows([96, 96, 96, 96, 96, 64], [[1e-6, 0., 0.]] * 4 + [[1e-6, 0., 0.], [o, 1e-9, 1e-9]])
    assert ST.passes_ref(T, n, 1e-3, 6).tolist() == [1] * 4 + [2] * 2
    T, n = _rows([96, 96, 96, 96, 0], [[o, o, o]] * 4 + [[1., 1., 1.]])
    assert ST.passes_ref(T, n, 1e-3, 5).tolist() == [3] * 4 + [0]
    # ran_mask: the first 32 P live samples
    live = torch.zeros(2, 96, dtype=torch.bool)
    live[0, ::2] = True          # 48 live
    live[1, 10:] = True          # 86 live
    ran = ST.ran_mask(live, torch.tensor([1, 2]))
    assert ran[0].nonzero().flatten().tolist() == list(range(0, 64, 2)) and ran[1].nonzero().flatten().tolist() == list(range(10, 74))


def test_pick_t_min_keeps_clear_of_every_boundary_value():
    T = torch.tensor([[1e-3, 0.], [1.02e-3, NAN], [0.98e-3, 5e-4], [2e-3, INF]], dtype=torch.float64)
    t, margin = ST.pick_t_min(T, 1e-3)
    assert 0.5e-3 <= t <= 2e-3 and margin >= 1e-3 and t == float(np.float32(t))
    assert abs(margin - min(abs(np.log(v / t)) for v in (1e-3, 1.02e-3, 0.98e-3, 5e-4, 2e-3))) < 1e-12
    assert ST.pick_t_min(torch.zeros(3, 2, dtype=torch.float64), 1e-2)[1] == INF
    assert ST.stop_bound(0., 256) == 0. and 1e-3 < ST.stop_bound(1e-3, 256) < 1.001e-3
