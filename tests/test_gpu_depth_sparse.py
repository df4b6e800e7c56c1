"""GPU (-m gpu): the sparse depth render (nnr_propose_f16.hip under NNR_PROPOSE_SPARSE=1 NNR_PROPOSE_DEPTH=1 through nnr_render_depth_sparse /
nnr.ops.render_depth_sparse; geometry.render_depth_maps(occupancy=...)), on the fixtures of the sibling tests: the
networks and rays of tests/test_gpu_propose.py, the 16^3 grids of tests/test_gpu_propose_sparse.py, the guard bands of tests/test_gpu_depth.py.
  * bit for bit columns 3:5, count, cell and passes of the stopping sparse render, at t_min = 0 and at a threshold picked at least 1e-3
    (in ln) away from every pass-boundary transmittance (tests/sparse_stop_ref.py), so that fp32 and float64 decide alike;
  * with every bit set the raw densities of the dense depth kernel bit for bit and its (depth, acc) at the output bar 1e-4 max(1, |ref|);
  * independently of the parent: cells, counts, passes, the evaluated set and (depth, acc) against the float64 restatement
    (tests/depth_sparse_ref.py), and against t_min = 0 within stop_bound + bar;
  * empty workgroups, the NaN rule, guard bands, determinism, and the plumbing through render_depth_maps and extract_mesh_tsdf."""
import ctypes as C
import functools
import logging
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nope-nerf_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import depth_sparse_ref as DS            # noqa: E402
import fusion_ref as FR                  # noqa: E402
import propose_sparse_ref as PS          # noqa: E402
import sparse_ref as SR                  # noqa: E402
import sparse_stop_ref as ST             # noqa: E402
import test_gpu_depth as td              # noqa: E402 -- the guard bands, _worst, the random network of the stop tests
import test_gpu_propose as tp            # noqa: E402 -- _net, _inputs
import test_gpu_propose_sparse as tps    # noqa: E402 -- _grid, _liveness

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = td.BAR
GUARD, SENTINEL = td.GUARD, td.SENTINEL
NAN_FILL = 0x7fc00000      # the bits of the NaN the wrapper pre-fills raw with
_bits = tp._bits


def _kw(mode):
    return dict(dist_alpha=mode == 'dist_alpha', relu_sigma=mode == 'relu')


def _sparse_depth(net, hidden, inp, grid, mode='softplus', t_min=0.):
    from nnr import ops
    o, d, z_lo, z_hi, jit = inp[:5]
    return ops.render_depth_sparse(o, d, z_lo, z_hi, jit, grid, net.weights(), net.biases(), hidden=hidden, t_min=t_min, debug=True, **_kw(mode))


def _parent(net, hidden, inp, view, grid, mode, t_min, white):
    from nnr import ops
    o, d, z_lo, z_hi, jit = inp[:5]
    return ops.render_sparse(o, d, view, z_lo, z_hi, jit, grid, net.weights(), net.biases(), hidden=hidden, white_bg=white, t_min=t_min,
                             debug=True, **_kw(mode))


def _dense(net, hidden, inp, mode='softplus'):
    from nnr import ops
    o, d, z_lo, z_hi, jit = inp[:5]
    return ops.render_depth(o, d, z_lo, z_hi, jit, net.weights(), net.biases(), hidden=hidden, debug=True, **_kw(mode))


def _view(R, seed):
    """a random unit view direction per ray: the depth render has none, the parent's columns 3:5 do not depend on it"""
    g = torch.Generator().manual_seed(900 + seed)
    return torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(DEV)


# (hidden, net, C, R, mode, jitter, pattern): every R, C, mode and pattern at least twice and at both widths
CASES = [(128, 'fitted', 32, 67, 'softplus', True, 'ball'), (256, 'fitted', 32, 5, 'dist_alpha', True, 'random'),
         (128, 'random', 33, 5, 'dist_alpha', True, 'random'), (256, 'fitted', 33, 67, 'softplus', False, 'ball'),
         (128, 'fitted', 1, 1, 'softplus', False, 'all'), (256, 'random', 1, 5, 'relu', True, 'random'),
         (128, 'random', 3, 67, 'relu', True, 'random'), (256, 'fitted', 3, 1, 'dist_alpha', False, 'ball'),
         (128, 'fitted', 100, 67, 'relu', True, 'random'), (256, 'random', 100, 5, 'softplus', False, 'ball'),
         (128, 'fitted', 256, 5, 'dist_alpha', True, 'ball'), (256, 'fitted', 256, 67, 'softplus', True, 'random'),
         (256, 'random', 256, 1, 'relu', False, 'none'), (128, 'random', 100, 1, 'dist_alpha', True, 'all'),
         (256, 'fitted', 100, 67, 'softplus', True, 'all'), (128, 'random', 32, 5, 'softplus', True, 'none')]
WHITE = (256, 'fitted', 256, 67, 'softplus', True, 'random')      # the one case whose parent renders on the white background
ALL_SET = [(128, 'fitted', 32, 67, 'softplus', True), (256, 'random', 33, 5, 'dist_alpha', True), (128, 'random', 1, 1, 'relu', False),
           (256, 'fitted', 3, 5, 'softplus', False), (128, 'fitted', 100, 67, 'relu', True), (256, 'fitted', 256, 67, 'softplus', True),
           (128, 'fitted', 256, 1, 'dist_alpha', True)]


@functools.lru_cache(maxsize=None)
def _case(hidden, kind, Cn, R, mode, jitter, pattern):
    """One case's inputs and every run its tests share, computed once and left unchanged: the kernel at t_min = 0, the pass boundaries made
    from that run's own raw densities, the picked threshold, the kernel at that threshold."""
    net, grid = tp._net(hidden, kind), tps._grid(pattern)
    inp = tp._inputs(R, Cn, 1, jitter, False)
    zv = _dense(net, hidden, inp, mode)[2]
    full = _sparse_depth(net, hidden, inp, grid, mode, 0.)
    live = tps._liveness(inp, zv, full[3], grid)
    alpha = FR.alpha_ref(full[1], zv, **_kw(mode))      # (NaN at the culled samples: every user masks them with `live`)
    T, n_live = ST.boundaries(alpha, live)
    t_min, margin = ST.pick_t_min(T, 1e-3 if mode != 'dist_alpha' else 0.4)
    assert margin >= 1e-3, "no threshold keeps clear of the boundary values (margin %.2e)" % margin
    stop = _sparse_depth(net, hidden, inp, grid, mode, t_min)
    return dict(net=net, grid=grid, inp=inp, zv=zv, full=full, live=live, alpha=alpha, T=T, n_live=n_live, t_min=t_min, stop=stop)


# ---------------------------------------------------------------------------------------------------------------- 1. the parent, bitwise
@pytest.mark.parametrize("hidden,kind,Cn,R,mode,jitter,pattern", CASES)
def test_out_count_cell_and_passes_are_the_stopping_sparse_renders(hidden, kind, Cn, R, mode, jitter, pattern):
    c = _case(hidden, kind, Cn, R, mode, jitter, pattern)
    white = (hidden, kind, Cn, R, mode, jitter, pattern) == WHITE
    view = _view(R, Cn)
    for t, got in ((0., c["full"]), (c["t_min"], c["stop"])):
        out, raw, count, cell, passes = got
        assert out.shape == (R, 2) and raw.shape == cell.shape == (R, Cn) and count.dtype == cell.dtype == passes.dtype == torch.int32
        par = _parent(c["net"], hidden, c["inp"], view, c["grid"], mode, t, white)
        assert torch.equal(_bits(out[:, 0]), _bits(par[1])) and torch.equal(_bits(out[:, 1]), _bits(par[2])), "t_min %g" % t
        assert torch.equal(count, par[3]) and torch.equal(cell, par[4])
        want_passes = par[6] if t > 0. else PS.passes_ref(count, R).to(DEV, torch.int32)      # (t_min = 0: the parent's own pass count)
        assert torch.equal(passes, want_passes)
        ran = ST.ran_mask(c["live"], passes).to(DEV)
        assert torch.equal(_bits(raw[ran]), _bits(par[5][..., 3][ran]))
        assert bool((_bits(raw[~ran]) == NAN_FILL).all()), "a raw density was written at a sample that was not evaluated"
        assert not bool(torch.isnan(par[5][..., 3][ran]).any())


# ---------------------------------------------------------------------------------------------------------------- 2. every bit set
@pytest.mark.parametrize("hidden,kind,Cn,R,mode,jitter", ALL_SET)
def test_with_every_bit_set_the_raw_densities_are_the_dense_depth_kernels(hidden, kind, Cn, R, mode, jitter, capsys):
    net = tp._net(hidden, kind)
    inp = tp._inputs(R, Cn, 1, jitter, False)
    out, raw, count, cell, passes = _sparse_depth(net, hidden, inp, tps._grid('all'), mode, 0.)
    dense, raw_d, zv = _dense(net, hidden, inp, mode)
    assert torch.equal(_bits(raw), _bits(raw_d)) and bool(torch.isfinite(raw).all())
    assert count.tolist() == [Cn] * R and passes.tolist() == [(Cn + 31) // 32] * R and bool((cell >= 0).all())
    ref = FR.composite_ref(FR.alpha_ref(raw, zv, **_kw(mode)), zv)
    w64, wd = td._worst(out, ref), td._worst(out, dense)
    with capsys.disabled():
        print("\ndepth_sparse all-set D=%d %s %s R=%d C=%d: worst |x - ref| / max(1, |ref|) %.3e against float64, %.3e against the dense kernel"
              % (hidden, kind, mode, R, Cn, w64, wd))
    assert w64 <= BAR and wd <= BAR


# ---------------------------------------------------------------------------------------------------------------- 3. without the parent
@pytest.mark.parametrize("hidden,kind,Cn,R,mode,jitter,pattern", CASES)
def test_passes_and_outputs_are_the_float64_restatements(hidden, kind, Cn, R, mode, jitter, pattern, capsys):
    c = _case(hidden, kind, Cn, R, mode, jitter, pattern)      # (_case: the cells against the float64 rule, tps._liveness's condition)
    out0, raw0, count0, cell0, passes0 = c["full"]
    out1, raw1, count1, cell1, passes1 = c["stop"]
    assert torch.equal(count0.cpu().to(torch.int64), c["live"].sum(1)) and torch.equal(count1, count0) and torch.equal(cell1, cell0)
    ref0, P0, ran0 = DS.depth_sparse_ref(c["alpha"], c["zv"], c["live"], 0.)
    ref1, P1, ran1 = DS.depth_sparse_ref(c["alpha"], c["zv"], c["live"], c["t_min"])
    assert torch.equal(passes0.cpu().to(torch.int64), P0) and torch.equal(P0, PS.passes_ref(count0, R))
    assert torch.equal(passes1.cpu().to(torch.int64), P1), "opt_passes differs from the float64 restatement on %d rays" % int(
        (passes1.cpu().to(torch.int64) != P1).sum())
    assert torch.equal((_bits(raw1) != NAN_FILL).cpu(), ran1) and torch.equal((_bits(raw0) != NAN_FILL).cpu(), c["live"])
    assert torch.equal(_bits(raw1[ran1.to(DEV)]), _bits(raw0[ran1.to(DEV)]))
    assert bool(torch.isfinite(out0).all()) and bool(torch.isfinite(out1).all())
    w0, w1 = td._worst(out0, ref0), td._worst(out1, ref1)
    rows = torch.arange(R)
    T_stop = torch.where(P1 > 0, c["T"][rows, (P1 - 1).clamp(min=0)], torch.zeros(R, dtype=torch.float64))
    bound = ST.stop_bound(T_stop, Cn)
    a0, a1 = out0.double().cpu(), out1.double().cpu()
    err, bar = (a1 - a0).abs(), BAR * a0.abs().clamp(min=1.)
    zmax = c["zv"].double().cpu().max(1)[0]
    with capsys.disabled():
        print("\ndepth_sparse D=%d %s %s R=%d C=%d %s t_min %.4e: live %.3f, passes %d / %d / dense %d; worst |x - ref| / max(1, |ref|) %.3e "
              "(t_min 0) %.3e (stopped); |stop - full| acc %.3e depth %.3e, largest bound %.3e"
              % (hidden, kind, mode, R, Cn, pattern, c["t_min"], float(c["live"].float().mean()), int(P1[::4].sum()), int(P0[::4].sum()),
                 ((R + 3) // 4) * ((Cn + 31) // 32), w0, w1, float(err[:, 1].max()), float(err[:, 0].max()), float(bound.max())))
    assert w0 <= BAR and w1 <= BAR
    assert bool((err[:, 1] <= bound + bar[:, 1]).all()) and bool((err[:, 0] <= bound * zmax + bar[:, 0]).all())
    full = (P1 == P0).to(DEV)      # a workgroup that ran its whole lists is the t_min = 0 run, bit for bit
    assert torch.equal(_bits(out1[full]), _bits(out0[full]))


def test_the_cases_cull_and_stop():
    culled = stopped = 0
    for case in CASES:
        c = _case(*case)
        culled += int((~c["live"]).sum())
        stopped += int((c["stop"][4] < c["full"][4]).sum())
        if case[-1] == 'none':
            assert c["full"][2].tolist() == [0] * case[3]
    assert culled > 0 and stopped > 0, "the cases culled %d samples and stopped %d rays early: they tested nothing" % (culled, stopped)


# ---------------------------------------------------------------------------------------------------------------- 4. nothing live
@pytest.mark.parametrize("hidden,Cn,R,mode", [(128, 33, 5, 'softplus'), (256, 100, 67, 'dist_alpha'), (128, 256, 1, 'relu'), (256, 1, 5, 'softplus')])
def test_rays_without_a_live_sample_get_zero_and_run_no_pass(hidden, Cn, R, mode):
    net = tp._net(hidden, 'fitted')
    inp = tp._inputs(R, Cn, 1, True, False)
    for t in (0., 1e-3):
        out, raw, count, cell, passes = _sparse_depth(net, hidden, inp, tps._grid('none'), mode, t)
        assert bool((cell >= 0).all()) and count.tolist() == [0] * R and passes.tolist() == [0] * R
        assert bool((_bits(out) == 0).all()) and bool((_bits(raw) == NAN_FILL).all())


@pytest.mark.parametrize("hidden,Cn", [(128, 33), (256, 100)])
def test_a_workgroup_with_one_live_ray_and_three_empty_ones(hidden, Cn):
    """four rays under a grid without a set bit; ray 1 starts outside the grid and leaves it further: all its samples are live"""
    net = tp._net(hidden, 'random')
    o, d, z_lo, z_hi, jit, _ = tp._inputs(4, Cn, 1, True, False)
    o, d = o.clone(), d.clone()
    o[1] = torch.tensor([20., 1., -2.], device=DEV)
    d[1] = torch.tensor([1., 0., 0.], device=DEV)
    inp = (o, d, z_lo, z_hi, jit)
    out, raw, count, cell, passes = _sparse_depth(net, hidden, inp, tps._grid('none'))
    assert count.tolist() == [0, Cn, 0, 0] and passes.tolist() == [(Cn + 31) // 32] * 4 and bool((cell[1] == -1).all())
    empty = torch.tensor([True, False, True, True], device=DEV)
    assert bool((_bits(out[empty]) == 0).all()) and bool((_bits(raw[empty]) == NAN_FILL).all())
    alone = _sparse_depth(net, hidden, (o[1:2], d[1:2], z_lo, z_hi, jit[1:2]), tps._grid('none'))
    assert torch.equal(_bits(out[1:2]), _bits(alone[0])) and torch.equal(_bits(raw[1:2]), _bits(alone[1])) and bool(torch.isfinite(out[1]).all())
    assert float(out[1, 1]) > 0.


# ---------------------------------------------------------------------------------------------------------------- 5. NaN
@pytest.mark.parametrize("hidden,Cn", [(128, 33), (256, 64)])
def test_an_infinite_origin_poisons_exactly_its_ray(hidden, Cn):
    """ray 5 of 7: its points are not finite, hence outside the grid, hence live -- (NaN, NaN); the other rays keep their bits"""
    net, grid = tp._net(hidden, 'fitted'), tps._grid('ball')
    inp = tp._inputs(7, Cn, 1, True, False)
    clean = _sparse_depth(net, hidden, inp, grid)
    o2 = inp[0].clone()
    o2[5, 1] = float('inf')
    out, raw, count, cell, passes = _sparse_depth(net, hidden, (o2,) + inp[1:], grid)
    bad = torch.zeros(7, dtype=torch.bool, device=DEV)
    bad[5] = True
    assert bool(torch.isnan(out[5]).all()) and int(count[5]) == Cn and cell[5].tolist() == [-1] * Cn
    assert passes[4:].tolist() == [(Cn + 31) // 32] * 3 and torch.equal(passes[:4], clean[4][:4])
    assert torch.equal(_bits(out[~bad]), _bits(clean[0][~bad])) and bool(torch.isfinite(out[~bad]).all())
    assert torch.equal(_bits(raw[~bad]), _bits(clean[1][~bad])) and torch.equal(count[~bad], clean[2][~bad])


@pytest.mark.parametrize("hidden", [128, 256])
def test_an_activation_outside_fp16_range_counts_only_where_the_sample_is_live_and_evaluated(hidden):
    from model import geometry as G
    Cn = 64
    hot = tp._net(hidden, 'hot')
    inp = tp._inputs(6, Cn, 1, True, False, seed=3)
    clean = _sparse_depth(hot, hidden, inp, tps._grid('all'))
    assert bool(torch.isfinite(clean[0]).all())
    o2 = inp[0].clone()
    o2[2] = torch.tensor([3e4, -2e4, 1e4], device=DEV)
    far = (o2,) + inp[1:]
    bad = torch.zeros(6, dtype=torch.bool, device=DEV)
    bad[2] = True
    here = _sparse_depth(hot, hidden, far, tps._grid('all'))      # the far ray is outside [-8, 8]^3: live, and its activations overflow
    assert here[2].tolist() == [Cn] * 6 and bool(torch.isnan(here[0][2]).all())
    c = [3e4, -2e4, 1e4]
    moved = G.OccupancyGrid(tuple(v - 16. for v in c), (0.5,) * 3, (16, 16, 16), torch.zeros(16, 16, 1, dtype=torch.int32, device=DEV))
    there = _sparse_depth(hot, hidden, far, moved)               # its samples lie in cleared cells: not evaluated
    assert there[2].tolist() == [Cn, Cn, 0, Cn, Cn, Cn] and bool((_bits(there[0][2]) == 0).all()) and bool((_bits(there[1][2]) == NAN_FILL).all())
    for res in (here, there):
        assert torch.equal(_bits(res[0][~bad]), _bits(clean[0][~bad]))
    # behind the stop: the second pass's samples sit 3e4 away (outside the grid, live, overflowing).  Without a threshold every ray is NaN;
    # with one between the transmittance after the first pass and 1 the workgroup stops in front of them and every ray is finite
    o, d, z_lo, z_hi, _ = tp._inputs(4, 32, 1, False, False, seed=5)[:5]
    near = _sparse_depth(hot, hidden, (o, d, z_lo, z_hi, None), tps._grid('all'))
    T0 = ST.boundaries(FR.alpha_ref(near[1], _dense(hot, hidden, (o, d, z_lo, z_hi, None))[2], False, False), torch.ones(4, 32, dtype=torch.bool))[0]
    assert float(T0.max()) < 0.9, "the four rays are not opaque enough after 32 samples for this test: T %s" % T0[:, 0].tolist()
    t = float(torch.tensor(0.5 * (1. + float(T0.max())), dtype=torch.float32))
    z2 = torch.cat([z_lo, torch.linspace(3e4, 3.1e4, 32, device=DEV)])
    full = _sparse_depth(hot, hidden, (o, d, z2, z2.clone(), None), tps._grid('all'), t_min=0.)
    assert full[4].tolist() == [2] * 4 and bool(torch.isnan(full[0]).all())
    stop = _sparse_depth(hot, hidden, (o, d, z2, z2.clone(), None), tps._grid('all'), t_min=t)
    assert stop[4].tolist() == [1] * 4 and bool(torch.isfinite(stop[0]).all())
    assert bool((_bits(stop[1][:, 32:]) == NAN_FILL).all()) and torch.equal(_bits(stop[1][:, :32]), _bits(near[1]))
    assert torch.equal(_bits(stop[0]), _bits(near[0]))      # (softplus alphas do not depend on the delta: the first pass is the 32-sample run)


# ---------------------------------------------------------------------------------------------------------------- 6. guard bands
def _guarded(n_words):
    buf = torch.full((n_words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, C.c_void_p(buf.data_ptr() + 4 * GUARD)


@pytest.mark.parametrize("hidden,kind,Cn,R,mode,jitter,pattern", [CASES[2], CASES[3], CASES[8], CASES[11], CASES[12]])
def test_the_entry_point_writes_inside_its_outputs_and_twice_the_same(hidden, kind, Cn, R, mode, jitter, pattern):
    from nnr import lib as L
    from nnr import ops
    c = _case(hidden, kind, Cn, R, mode, jitter, pattern)
    o, d, z_lo, z_hi, jit = c["inp"][:5]
    grid = c["grid"]
    cfg = ops.split2_cfg(R, Cn, hidden, **_kw(mode))
    packed = ops._packed_for(ops.split2_cfg(R, Cn, hidden), c["net"].weights(), c["net"].biases())
    lo3, is3, d3 = (C.c_float * 3)(*grid.lo), (C.c_float * 3)(*grid.inv_step), (C.c_int32 * 3)(*grid.dims)
    sizes = dict(out=2 * R, raw=R * Cn, count=R, cell=R * Cn, passes=R)
    for t, want in ((0., c["full"]), (c["t_min"], c["stop"])):
        runs = []
        for _ in range(2):
            bufs = {k: _guarded(v) for k, v in sizes.items()}
            rc = L.load().nnr_render_depth_sparse(C.byref(cfg), L.ptr(o), L.ptr(d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), lo3, is3, d3,
                                                  L.ptr(grid.bits), float(t), L.ptr(packed), bufs["out"][1], bufs["raw"][1], bufs["count"][1],
                                                  bufs["cell"][1], bufs["passes"][1], L.stream())
            torch.cuda.synchronize()
            assert rc == 0
            for k, n in sizes.items():
                buf = bufs[k][0]
                assert bool((torch.cat([buf[:GUARD], buf[GUARD + n:]]) == SENTINEL).all()), "the kernel wrote outside " + k
            runs.append({k: bufs[k][0][GUARD:GUARD + n].clone() for k, n in sizes.items()})
        for k in sizes:
            assert torch.equal(runs[0][k], runs[1][k]), k
        got = runs[0]
        assert not bool((got["out"] == SENTINEL).any()) and not bool((got["passes"] == SENTINEL).any()), "a ray was not written"
        assert torch.equal(got["out"].view(R, 2), _bits(want[0])) and torch.equal(got["count"], want[2])
        assert torch.equal(got["cell"].view(R, Cn), want[3]) and torch.equal(got["passes"], want[4])
        written = got["raw"].view(R, Cn) != SENTINEL      # untouched where not evaluated: the sentinel is still there
        assert torch.equal(written, _bits(want[1]) != NAN_FILL) and torch.equal(got["raw"].view(R, Cn)[written], _bits(want[1])[written])
    plain = ops.render_depth_sparse(o, d, z_lo, z_hi, jit, grid, c["net"].weights(), c["net"].biases(), hidden=hidden, t_min=c["t_min"], **_kw(mode))
    assert torch.is_tensor(plain) and plain.shape == (R, 2) and torch.equal(_bits(plain), _bits(c["stop"][0]))


# ---------------------------------------------------------------------------------------------------------------- 7. the stop bites
@pytest.mark.parametrize("hidden", [128, 256])
def test_one_pass_of_eight_runs_on_the_stop_tests_opaque_rays(hidden):
    """the 256-sample rays of tests/test_gpu_sparse_stop.py's one-pass case (its random softplus network, every bit set), two workgroups"""
    import test_gpu_sparse as tsp
    from nnr import ops
    R, Cn = 8, 256
    net, grid = td._net(hidden, 'random'), tsp._grid("set")
    o, d, view, lo, hi, jit = tsp._scene(R, Cn, 'random', "set")
    inp = (o, d, lo, hi, jit)
    full = _sparse_depth(net, hidden, inp, grid)
    zv = _dense(net, hidden, inp)[2]
    live = (_bits(full[1]) != NAN_FILL).cpu()
    T, _ = ST.boundaries(FR.alpha_ref(full[1], zv, False, False), live)
    t_min, margin = ST.pick_t_min(T, 1e-3)
    assert margin >= 1e-3
    stop = _sparse_depth(net, hidden, inp, grid, t_min=t_min)
    kw = dict(hidden=hidden, dist_alpha=False, white_bg=False, relu_sigma=False)
    par = ops.render_sparse(o, d, view, lo, hi, jit, grid, net.weights(), net.biases(), t_min=t_min, debug=True, **kw)
    assert full[2].tolist() == [Cn] * R and full[4].tolist() == [(Cn + 31) // 32] * R
    assert stop[4].tolist() == [1] * R and torch.equal(stop[4], par[6])
    assert torch.equal(_bits(stop[0][:, 0]), _bits(par[1])) and torch.equal(_bits(stop[0][:, 1]), _bits(par[2]))


# ---------------------------------------------------------------------------------------------------------------- 8. plumbing
def _maps_by_hand(renderer, K, Wm, size, min_acc, grid, t_min):
    """render_depth_maps spelled out with the public operators: ray_setup, the z tables, ops.render_depth[_sparse], ray_norm, the +inf rule"""
    from nnr import camera, ops
    from model.common import arange_pixels
    H, W = size
    dev = torch.device(DEV)
    cfg, net = renderer.cfg, renderer.model
    n = int(cfg['num_points']) - int(cfg['outside_steps'])
    pixels = arange_pixels((H, W), device=dev)[1]
    kw = dict(hidden=net.hidden_dim, dist_alpha=bool(cfg['dist_alpha']), relu_sigma=False)
    maps = []
    with torch.no_grad():
        z_lo, z_hi = renderer._z_tables(n, renderer.depth_range[0], renderer.depth_range[1], False, dev)
        for i in range(Wm.shape[0]):
            origin, ray, _, ray_norm, _, _ = camera.ray_setup(pixels, None, K.float().to(dev)[None], Wm[i].float().to(dev)[None],
                                                              torch.eye(4, device=dev)[None], bool(cfg['normalise_ray']), bool(cfg['use_ray_dir']))
            if grid is None:
                da = ops.render_depth(origin, ray, z_lo, z_hi, None, net.weights(), net.biases(), **kw)
            else:
                da = ops.render_depth_sparse(origin, ray, z_lo, z_hi, None, grid, net.weights(), net.biases(), t_min=t_min, **kw)
            depth = da[:, 0] / ray_norm if cfg['normalise_ray'] else da[:, 0]
            maps.append(torch.where(da[:, 1] < min_acc, torch.full_like(depth, float('inf')), depth).view(H, W))
    return torch.stack(maps)


@pytest.mark.parametrize("size", [(5, 7), (24, 32)])
def test_render_depth_maps_with_a_grid_is_the_hand_made_composition(size):
    import test_gpu_fusion as tf
    from model import geometry as G
    renderer = tf._fitted_renderer(128)
    K = torch.diag(torch.tensor(FR.K_DIAG, dtype=torch.float64))
    Wm = FR.look_at_world_mats(14, 3.5)[[2, 9]]
    grid = tps._grid('ball')
    got = G.render_depth_maps(renderer, K, Wm, size, occupancy=grid, t_min=1e-3, chunk=100)
    want = _maps_by_hand(renderer, K, Wm, size, 0.5, grid, 1e-3)
    assert got.shape == (2,) + size and torch.equal(_bits(got), _bits(want))
    assert bool(torch.isinf(got).any()) and bool(torch.isfinite(got).any()) and not bool(torch.isnan(got).any())
    # without a grid: the same launches and bits as before the arguments existed -- ops.render_depth directly
    plain = G.render_depth_maps(renderer, K, Wm, size, chunk=100)
    assert torch.equal(_bits(plain), _bits(_maps_by_hand(renderer, K, Wm, size, 0.5, None, 0.)))
    assert torch.equal(_bits(G.render_depth_maps(renderer, K, Wm, size, occupancy=None, t_min=0.)), _bits(plain))
    with pytest.raises(ValueError, match="t_min.*occupancy"):
        G.render_depth_maps(renderer, K, Wm, size, t_min=1e-3)
    # an all-set grid without a threshold: the dense maps at the output bar, the same pixels +inf up to acc within the bar of min_acc
    full = G.render_depth_maps(renderer, K, Wm, size, min_acc=0., occupancy=tps._grid('all'))
    dense = G.render_depth_maps(renderer, K, Wm, size, min_acc=0.)
    assert td._worst(full, dense) <= BAR


def test_more_than_256_samples_with_a_grid_take_the_render_rays_branch_and_say_so_once(caplog, monkeypatch):
    import test_gpu_fusion as tf
    from model import geometry as G
    from nnr import ops
    renderer = tf._fitted_renderer(128, 288)
    K = torch.diag(torch.tensor(FR.K_DIAG, dtype=torch.float64))
    Wm = FR.look_at_world_mats(14, 3.5)[[2, 9]]
    monkeypatch.setattr(ops, "render_depth_sparse", lambda *a, **k: pytest.fail("the sparse depth kernel takes at most 256 samples"))
    monkeypatch.setattr(ops, "render_depth", lambda *a, **k: pytest.fail("the dense depth kernel takes at most 256 samples"))
    with caplog.at_level(logging.INFO, logger=G.__name__):
        got = G.render_depth_maps(renderer, K, Wm, (5, 7), occupancy=tps._grid('ball'), t_min=1e-3, chunk=16)
    said = [r for r in caplog.records if r.name == G.__name__ and "occupancy grid ignored" in r.getMessage()]
    assert len(said) == 1 and "288" in said[0].getMessage() and "256" in said[0].getMessage()
    caplog.clear()
    with caplog.at_level(logging.INFO, logger=G.__name__):
        want = G.render_depth_maps(renderer, K, Wm, (5, 7), chunk=16)
    assert not [r for r in caplog.records if "occupancy grid ignored" in r.getMessage()]
    assert torch.equal(_bits(got), _bits(want))


def test_extract_mesh_tsdf_with_an_all_set_grid_selects_the_same_bricks():
    import test_gpu_fusion as tf
    from model import geometry as G
    from nnr import ops
    renderer = tf._fitted_renderer(128)
    H, W = 24, 32
    K = torch.diag(torch.tensor(FR.K_DIAG, dtype=torch.float64))
    Wm = FR.look_at_world_mats(14, 3.5)
    cams = G.Cameras(K, Wm, (H, W))
    lo, hi, coarse, refine = (-2.4,) * 3, (2.4,) * 3, 17, 4
    grid = tps._grid('all')
    res = {}
    for key, kw in (("dense", {}), ("sparse", dict(occupancy=grid, t_min=0.))):
        calls = []

        def integrate(o, s, br, cm, dp, tr, sm, wt):
            ops.tsdf_integrate(o, s, br, cm, dp, tr, sm, wt)
            calls.append((br.cpu().clone(), cm.cpu(), tr, dp))
        mesh = G.extract_mesh_tsdf(renderer, cams, lo, hi, coarse, refine=refine, integrate=integrate, colour=False, **kw)
        res[key] = (mesh, calls)
    (mesh_d, calls_d), (mesh_s, calls_s) = res["dense"], res["sparse"]
    assert len(calls_d) == len(calls_s) == 2 and mesh_s.n_bricks == mesh_d.n_bricks > 0
    assert torch.equal(calls_s[1][0], calls_d[1][0]), "the all-set grid selected other bricks"
    depth = calls_s[0][3]
    assert torch.equal(_bits(depth), _bits(G.render_depth_maps(renderer, K, Wm, (H, W), occupancy=grid, t_min=0.)))
    both = torch.isfinite(depth) & torch.isfinite(calls_d[0][3])      # (the maps agree at the bar; bitwise equality is not promised)
    assert bool(both.any()) and td._worst(depth[both], calls_d[0][3][both]) <= BAR
    # every vertex lies within trunc + sqrt(3) h in z of a depth some camera that observes it saw (tests/test_gpu_fusion.py's bound)
    V = mesh_s.vertices.shape[0]
    assert V > 0 and mesh_s.quads.shape[0] > 0
    h = max(abs(v) for v in mesh_s.step)
    trunc = calls_s[1][2]
    assert abs(trunc - 3 * h) < 1e-6
    v = mesh_s.vertices.double().cpu()
    P = calls_s[1][1].double().view(14, 3, 4)
    q = torch.einsum('crk,vk->cvr', P[:, :, :3], v) + P[:, None, :, 3]
    qz = q[..., 2]
    ci, ri = torch.round((q[..., 0] / qz + 1) * (W - 1) / 2), torch.round((q[..., 1] / qz + 1) * (H - 1) / 2)
    seen = (qz > 0) & (ci >= 0) & (ci <= W - 1) & (ri >= 0) & (ri <= H - 1)
    dm = depth.double().cpu()[torch.arange(14)[:, None], ri.clamp(0, H - 1).long(), ci.clamp(0, W - 1).long()]
    seen = seen & torch.isfinite(dm) & (dm > 0)
    gap = torch.where(seen, (qz - dm).abs(), torch.full_like(qz, float('inf'))).min(0).values
    assert bool((gap <= trunc + math.sqrt(3.) * h).all()), "%d vertices further than trunc + sqrt(3) h from every observed depth" % int(
        (gap > trunc + math.sqrt(3.) * h).sum())
