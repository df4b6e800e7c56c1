"""GPU (-m gpu): the quantile (median) depth of the two depth kernels (include/nnr_depth_median.h): nnr_depth_f16.hip
under NNR_DEPTH_MEDIAN=1 and nnr_propose_f16.hip under NNR_PROPOSE_SPARSE=1 NNR_PROPOSE_DEPTH=2, through nnr.ops.render_depth[_sparse]
(quantile_level=...) and geometry.render_depth_maps(depth_mode='median'), on the fixtures of the sibling tests: the networks and rays of
tests/test_gpu_propose.py, the 16^3 grids of tests/test_gpu_propose_sparse.py, the guard bands of tests/test_gpu_depth.py.

The bound of q against float64 (tests 4 and 5), derived here and not tuned to the kernels.  u = 2^-24.
  * A factor.  f_i = (1 - alpha_i) + 1e-6 in fp32 from the fp32 alpha.  alpha = 1 - exp(-sigma delta): sigma (softplus, or max(raw, 0)) carries a
    relative error of at most 3 u, which moves exp(-x) by at most 3 u x exp(-x) <= 1.2 u; expf itself at most 2 u exp(-x) <= 2 u; the
    subtraction from 1, the second one and the sum with 1e-6 round once each, every result at most about 1: 3 u.  |f^_i - f_i| <= 6.2 u,
    taken as E_FACTOR = 8 u, ABSOLUTE (a factor may be as small as 1e-6).
  * A product.  T_k multiplies the n_k evaluated factors in front of boundary k.  To first order each factor's error enters once, scaled by
    the product of the others: A_{k+1} = A_k f_k + T_k E_FACTOR; each multiplication rounds once, and a scan multiplies along a tree
    whose depth is below that of the chain, the sparse kernel once more for carry times scan: (n_k + 8) u T_k is generous.
    E_k = A_k + (n_k + 8) u T_k bounds |T^_k - T_k| whatever the order of the products.
  * The quotient.  r = N / D, N = T_m - level, D = T_m - T_{m+1}; level is an fp32 on both sides.  |N^ - N| <= E_m + u |N| = dN,
    |D^ - D| <= E_m + E_{m+1} + u D = dD, and with 0 <= r <= 1
        |N^ / D^ - r| = |(N^ - N) - r (D^ - D)| / D^ <= (dN + r dD) / (D - dD),
    plus the division's own rounding u r: kappa = (dN + r dD) / (D - dD) + u r (depth_median_ref.error_terms).  The errors of T^_m and
    T^_{m+1} are taken as independent, which they are not: an over-estimate.  A ray whose D - dD <= 0 has kappa = inf and counts as left out.
  * q = z_m + gap r: the roundings of gap, of the product and of the sum are a few u max(gap, |q|), far inside the output bar.
    |q - ref| <= 1e-4 max(1, |ref|) + gap kappa.
  * Left out: a ray with an evaluated boundary within E_k of level (fp32 may place the crossing one sample off), or with kappa = inf;
    more than 2 % of a case's rays left out fails the case."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nope-nerf_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import depth_median_ref as DM            # noqa: E402
import fusion_ref as FR                  # noqa: E402
import test_gpu_depth as td              # noqa: E402 -- the guard bands, the random network of the stop tests
import test_gpu_depth_sparse as tds      # noqa: E402 -- _kw, _maps_by_hand
import test_gpu_propose as tp            # noqa: E402 -- _net, _inputs
import test_gpu_propose_sparse as tps    # noqa: E402 -- _grid

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = td.BAR
GUARD, SENTINEL = td.GUARD, td.SENTINEL
NAN_FILL = tds.NAN_FILL
INF = float("inf")
_bits = tp._bits
_kw = tds._kw


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _dense(net, hidden, inp, mode, level):
    """(out (R,3), raw, z) of the median build, or (out (R,2), raw, z) of the parent for level None"""
    from nnr import ops
    o, d, z_lo, z_hi, jit = inp[:5]
    return ops.render_depth(o, d, z_lo, z_hi, jit, net.weights(), net.biases(), hidden=hidden, debug=True, quantile_level=level, **_kw(mode))


def _sparse(net, hidden, inp, grid, mode, t_min, level):
    """(out, raw, count, cell, passes) of the median build, or of the parent for level None"""
    from nnr import ops
    o, d, z_lo, z_hi, jit = inp[:5]
    return ops.render_depth_sparse(o, d, z_lo, z_hi, jit, grid, net.weights(), net.biases(), hidden=hidden, t_min=t_min, debug=True,
                                   quantile_level=level, **_kw(mode))


# (hidden, net, C, R, mode, jitter, pattern, level): every C, R, mode, level and pattern at both widths; C = 1: one sample; 33, 65: a partial
# last pass, per = 1 and 2; 256: per = 4; R = 1, 5: a partial workgroup and waves past the last ray; 130: 33 workgroups, the last one partial
CASES = [(128, 'fitted', 1, 1, 'softplus', False, 'all', 0.5), (256, 'random', 1, 5, 'dist_alpha', True, 'random', 0.9),
         (128, 'random', 33, 5, 'dist_alpha', True, 'random', 0.1), (256, 'fitted', 33, 130, 'softplus', False, 'ball', 0.5),
         (128, 'fitted', 64, 130, 'softplus', True, 'ball', 0.9), (256, 'random', 64, 1, 'relu', True, 'all', 0.5),
         (128, 'random', 65, 130, 'relu', False, 'random', 0.5), (256, 'fitted', 65, 5, 'dist_alpha', True, 'ball', 0.1),
         (128, 'fitted', 256, 5, 'dist_alpha', True, 'random', 0.9), (256, 'fitted', 256, 130, 'softplus', True, 'ball', 0.1),
         (128, 'random', 256, 130, 'softplus', True, 'all', 0.5), (256, 'random', 256, 1, 'relu', False, 'random', 0.1)]
ALL_SET = [(128, 'fitted', 33, 130, 'softplus', True, 0.5), (256, 'random', 65, 5, 'dist_alpha', True, 0.1), (128, 'random', 1, 1, 'relu', False, 0.9),
           (256, 'fitted', 256, 130, 'softplus', True, 0.9), (128, 'fitted', 256, 5, 'dist_alpha', False, 0.5), (256, 'random', 64, 130, 'relu', True, 0.1)]


@functools.lru_cache(maxsize=None)
def _case(hidden, kind, Cn, R, mode, jitter, pattern, level):
    """One case's inputs and every run its tests share, computed once and left unchanged"""
    net, grid = tp._net(hidden, kind), tps._grid(pattern)
    inp = tp._inputs(R, Cn, 1, jitter, False)
    level = _f32(level)
    return dict(net=net, grid=grid, inp=inp, level=level, dense=_dense(net, hidden, inp, mode, level),
                full=_sparse(net, hidden, inp, grid, mode, 0., level), stop=_sparse(net, hidden, inp, grid, mode, level, level))


# ---------------------------------------------------------------------------------------------------------------- 1. the dense columns
@pytest.mark.parametrize("hidden,kind,Cn,R,mode,jitter,pattern,level", CASES)
def test_dense_columns_0_and_1_are_the_depth_kernels(hidden, kind, Cn, R, mode, jitter, pattern, level):
    c = _case(hidden, kind, Cn, R, mode, jitter, pattern, level)
    out, raw, zv = c["dense"]
    par = _dense(c["net"], hidden, c["inp"], mode, None)
    assert out.shape == (R, 3) and par[0].shape == (R, 2)
    assert torch.equal(_bits(out[:, :2]), _bits(par[0])) and torch.equal(_bits(raw), _bits(par[1])) and torch.equal(_bits(zv), _bits(par[2]))
    assert not bool(torch.isnan(out).any())


# ---------------------------------------------------------------------------------------------------------------- 2. the sparse columns
@pytest.mark.parametrize("hidden,kind,Cn,R,mode,jitter,pattern,level", CASES)
def test_sparse_columns_counts_cells_and_passes_are_the_sparse_depth_kernels(hidden, kind, Cn, R, mode, jitter, pattern, level):
    c = _case(hidden, kind, Cn, R, mode, jitter, pattern, level)
    runs = [(0., c["full"]), (c["level"], c["stop"])]
    if c["level"] > 1e-3:
        runs.append((1e-3, _sparse(c["net"], hidden, c["inp"], c["grid"], mode, 1e-3, c["level"])))
    for t, got in runs:
        par = _sparse(c["net"], hidden, c["inp"], c["grid"], mode, t, None)
        assert got[0].shape == (R, 3) and par[0].shape == (R, 2)
        assert torch.equal(_bits(got[0][:, :2]), _bits(par[0])), "t_min %g" % t
        for k in (1, 2, 3, 4):      # raw (NaN-filled where not evaluated), count, cell, passes
            assert torch.equal(_bits(got[k]), _bits(par[k])), (t, k)


# ---------------------------------------------------------------------------------------------------------------- 3. exact under the stop
@pytest.mark.parametrize("hidden,kind,Cn,R,mode,jitter,pattern,level", CASES)
def test_stopping_at_the_level_leaves_q_bit_for_bit(hidden, kind, Cn, R, mode, jitter, pattern, level):
    c = _case(hidden, kind, Cn, R, mode, jitter, pattern, level)
    assert torch.equal(_bits(c["stop"][0][:, 2]), _bits(c["full"][0][:, 2]))
    assert bool((c["stop"][4] <= c["full"][4]).all()) and torch.equal(c["stop"][2], c["full"][2])


@pytest.mark.parametrize("hidden", [128, 256])
@pytest.mark.parametrize("level", [0.1, 0.5, 0.9])
def test_one_pass_of_eight_runs_on_the_stop_tests_opaque_rays_with_the_same_q(hidden, level):
    """the 256-sample rays of tests/test_gpu_sparse_stop.py's one-pass case (its random softplus network, every bit set), two workgroups"""
    import test_gpu_sparse as tsp
    R, Cn = 8, 256
    net, grid = td._net(hidden, 'random'), tsp._grid("set")
    o, d, view, lo, hi, jit = tsp._scene(R, Cn, 'random', "set")
    inp, level = (o, d, lo, hi, jit), _f32(level)
    full = _sparse(net, hidden, inp, grid, 'softplus', 0., level)
    stop = _sparse(net, hidden, inp, grid, 'softplus', level, level)
    assert full[4].tolist() == [8] * R and stop[4].tolist() == [1] * R
    assert torch.equal(_bits(stop[0][:, 2]), _bits(full[0][:, 2])) and bool(torch.isfinite(full[0][:, 2]).all())


def test_the_cases_cull_stop_and_cross():
    culled = stopped = crossed = 0
    for case in CASES:
        c = _case(*case)
        culled += int((_bits(c["full"][1]) == NAN_FILL).sum())
        stopped += int((c["stop"][4] < c["full"][4]).sum())
        crossed += int(torch.isfinite(c["full"][0][:, 2]).sum()) + int(torch.isfinite(c["dense"][0][:, 2]).sum())
    assert min(culled, stopped, crossed) > 0, "culled %d samples, stopped %d rays early, %d crossings: the cases test nothing" % (
        culled, stopped, crossed)


# ---------------------------------------------------------------------------------------------------------------- 4. against float64
def _against_ref(q, raw, zv, mask, level, mode, what, capsys, other=None):
    """q (R) of a kernel against the float64 restatement on the kernel's own raw densities and depths, at the bound of this file's docstring;
    other: a second kernel's q held to the same bound of the first (test 5).  -> the share of rays left out"""
    alpha = FR.alpha_ref(raw, zv, **_kw(mode))
    ref = DM.quantile_ref(alpha, zv, mask, level)
    E, kappa, near = DM.error_terms(alpha, mask, ref, level)
    out = near | torch.isinf(kappa)
    R = q.shape[0]
    got, want = q.double().cpu(), ref["q"]
    special = ~torch.isfinite(want)
    bound = BAR * want.abs().clamp(min=1.) + ref["gap"].abs() * kappa
    keep = ~out & ~special
    err = (got - want).abs()
    worst = float((err[keep] / bound[keep]).max()) if bool(keep.any()) else 0.
    with capsys.disabled():
        print("\ndepth_median %s: %d rays, %d finite, %d left out (%.2f %%), worst |q - ref| / bound %.3e, worst |q - ref| %.3e, largest kappa %.3e"
              % (what, R, int((~special).sum()), int(out.sum()), 100. * float(out.sum()) / R, worst,
                 float(err[keep].max()) if bool(keep.any()) else 0., float(kappa[keep].max()) if bool(keep.any()) else 0.))
    assert int(out.sum()) <= 0.02 * R, "%d of %d rays left out: more than 2 %%" % (int(out.sum()), R)
    sp = special & ~out      # where the reference is +inf or NaN, q is the same special value
    assert torch.equal(torch.isinf(got[sp]), torch.isinf(want[sp])) and torch.equal(torch.isnan(got[sp]), torch.isnan(want[sp]))
    assert bool((got[sp & torch.isinf(want)] > 0).all())
    assert bool(torch.isfinite(got[keep]).all()) and bool((err[keep] <= bound[keep]).all()), "worst |q - ref| / bound %.3e" % worst
    if other is not None:
        o = other.double().cpu()
        d = (o - got).abs()
        b = BAR * got.abs().clamp(min=1.) + ref["gap"].abs() * kappa
        assert torch.equal(torch.isfinite(o[~out]), torch.isfinite(got[~out])) and bool((d[keep] <= b[keep]).all())
    return float(out.sum()) / R


@pytest.mark.parametrize("hidden,kind,Cn,R,mode,jitter,pattern,level", CASES)
def test_q_is_the_float64_restatement_on_the_kernels_own_samples(hidden, kind, Cn, R, mode, jitter, pattern, level, capsys):
    c = _case(hidden, kind, Cn, R, mode, jitter, pattern, level)
    what = "D=%d %s %s R=%d C=%d %s level %g" % (hidden, kind, mode, R, Cn, pattern, level)
    out, raw, zv = c["dense"]
    _against_ref(out[:, 2], raw, zv, torch.ones(R, Cn, dtype=torch.bool), c["level"], mode, "dense " + what, capsys)
    for name, run in (("sparse t_min 0 ", c["full"]), ("sparse stopped ", c["stop"])):
        ran = (_bits(run[1]) != NAN_FILL).cpu()      # the evaluated samples: where a raw density was written
        _against_ref(run[0][:, 2], run[1], zv, ran, c["level"], mode, name + what, capsys)


# ---------------------------------------------------------------------------------------------------------------- 5. dense against sparse
@pytest.mark.parametrize("hidden,kind,Cn,R,mode,jitter,level", ALL_SET)
def test_with_every_bit_set_the_sparse_q_is_within_the_bound_of_the_dense_q(hidden, kind, Cn, R, mode, jitter, level, capsys):
    net = tp._net(hidden, kind)
    inp = tp._inputs(R, Cn, 1, jitter, False)
    level = _f32(level)
    dense, raw_d, zv = _dense(net, hidden, inp, mode, level)
    sparse = _sparse(net, hidden, inp, tps._grid('all'), mode, 0., level)
    assert torch.equal(_bits(sparse[1]), _bits(raw_d)) and sparse[2].tolist() == [Cn] * R
    _against_ref(dense[:, 2], raw_d, zv, torch.ones(R, Cn, dtype=torch.bool), level, mode,
                 "all-set D=%d %s %s R=%d C=%d level %g" % (hidden, kind, mode, R, Cn, level), capsys, other=sparse[0][:, 2])


# ---------------------------------------------------------------------------------------------------------------- 6. where the crossing falls
def _between(T, r, m):
    """an fp32 level strictly between T[r, m + 1] and T[r, m], at their geometric mean, or None where the two are too close or it is not in (0, 1)"""
    hi, lo = float(T[r, m]), float(T[r, m + 1])
    if not (lo > 0. and hi > lo * 1.01):
        return None
    level = _f32((hi * lo) ** 0.5)
    return level if (0. < level < 1. and lo * 1.001 < level < hi / 1.001) else None


def _place(T, m, rays=None):
    """(ray, level): the ray whose boundary pair around sample m is widest, and a level inside it"""
    best = None
    for r in (range(T.shape[0]) if rays is None else rays):
        level = _between(T, r, m)
        if level is not None and (best is None or float(T[r, m] / T[r, m + 1]) > best[2]):
            best = (r, level, float(T[r, m] / T[r, m + 1]))
    assert best is not None, "no ray of the batch has a usable pair of boundaries around sample %d" % m
    return best[0], best[1]


def _inward_rays(R, seed):
    """R rays from the shell of radius 2.5 straight at the origin: the fitted scene's sphere (radius 1.2) begins at z = 1.3"""
    g = torch.Generator().manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    return (2.5 * u).to(DEV), (-u).to(DEV), u


def _row_with_matter_from(Cn, m):
    """depths whose first m samples lie in front of the fitted scene (z in [0.05, 0.9] of an inward ray) and whose others lie inside its sphere
    (z in [2, 3]): the transmittance falls steeply at sample m"""
    z = torch.cat([torch.linspace(0.05, 0.9, m), torch.linspace(2.0, 3.0, Cn - m)]) if m else torch.linspace(2.0, 3.0, Cn)
    return z.to(DEV), z.clone().to(DEV)


@pytest.mark.parametrize("hidden,Cn,mode", [(128, 65, 'softplus'), (256, 256, 'softplus'), (128, 33, 'dist_alpha'), (256, 64, 'dist_alpha')])
def test_crossings_at_the_first_the_last_and_the_last_lanes_samples(hidden, Cn, mode, capsys):
    """levels chosen between two of a ray's own boundaries, on rows built so that the transmittance falls at the wanted sample: sample 0; the
    last sample (z_next = z_m: q is z_m bit for bit); the first sample of the last lane that owns one (dense: lane ceil(C / per) - 1); list
    slots 31 and 32, either side of the sparse kernel's pass boundary (every bit set: slot = sample)"""
    R = 130
    net, grid = tp._net(hidden, 'fitted'), tps._grid('all')
    o, d, _ = _inward_rays(R, 70 + Cn)
    ones = torch.ones(R, Cn, dtype=torch.bool)
    per = (Cn + 63) // 64
    wanted = {"first": 0, "last": Cn - 1, "last lane": per * ((Cn + per - 1) // per - 1), "slot 31": 31, "slot 32": 32}
    for name, m in wanted.items():
        z_lo, z_hi = _row_with_matter_from(Cn, m)
        inp = (o, d, z_lo, z_hi, None)
        _, raw, zv = _dense(net, hidden, inp, mode, 0.5)
        alpha = FR.alpha_ref(raw, zv, **_kw(mode))
        r, level = _place(DM.quantile_ref(alpha, zv, ones, 0.5)["T"], m)
        ref = DM.quantile_ref(alpha, zv, ones, level)
        assert int(ref["m"][r]) == m
        _, kappa, near = DM.error_terms(alpha, ones, ref, level)
        assert not bool(near[r]) and float(kappa[r]) < INF
        bound = BAR * max(1., abs(float(ref["q"][r]))) + abs(float(ref["gap"][r])) * float(kappa[r])
        qd = _dense(net, hidden, inp, mode, level)[0][:, 2]
        qs = _sparse(net, hidden, inp, grid, mode, 0., level)[0][:, 2]
        with capsys.disabled():
            print("\ndepth_median placement D=%d C=%d %s %s: ray %d sample %d level %.6g q dense %.7g sparse %.7g ref %.7g bound %.3e"
                  % (hidden, Cn, mode, name, r, m, level, float(qd[r]), float(qs[r]), float(ref["q"][r]), bound))
        for which, q in (("dense", qd), ("sparse", qs)):
            assert abs(float(q[r]) - float(ref["q"][r])) <= bound, (name, which, float(q[r]), float(ref["q"][r]))
            assert float(zv[r, m]) <= float(q[r]) <= float(zv[r, min(m + 1, Cn - 1)]), (name, which)
            if m == Cn - 1:
                assert _bits(q[r:r + 1]).item() == _bits(zv[r, m:m + 1]).item(), (name, which)


@pytest.mark.parametrize("hidden,Cn", [(128, 33), (256, 100)])
def test_a_ray_that_never_crosses_shares_its_workgroup_with_three_that_do(hidden, Cn):
    """three rays through the fitted scene's sphere and, in wave 1, one that passes it by (from the same shell, at a right angle to the
    others' direction): the level lies between their final transmittances"""
    net = tp._net(hidden, 'fitted')
    o, d, u = _inward_rays(4, 11 + Cn)
    side = torch.nn.functional.normalize(torch.linalg.cross(u[1], torch.tensor([0.3, -0.5, 0.8])), dim=-1)
    d = d.clone()
    d[1] = side.to(DEV)
    z_lo, z_hi = tp._tables(Cn, True, near=0.5, far=3.5)
    jit = torch.rand(4, Cn, generator=torch.Generator().manual_seed(Cn)).to(DEV)
    inp = (o, d, z_lo, z_hi, jit)
    _, raw, zv = _dense(net, hidden, inp, 'softplus', 0.5)
    T_end = DM.quantile_ref(FR.alpha_ref(raw, zv, False, False), zv, torch.ones(4, Cn, dtype=torch.bool), 0.5)["T"][:, -1]
    hi, lo = float(T_end[1]), float(T_end[[0, 2, 3]].max())
    assert 0.49 * hi > lo, "the passing ray is not clearly more transparent than the three through the sphere: T %s" % T_end.tolist()
    level = _f32(0.5 * hi)
    assert 0. < level < 1.
    qd = _dense(net, hidden, inp, 'softplus', level)[0]
    qs = _sparse(net, hidden, inp, tps._grid('all'), 'softplus', level, level)[0]
    for q in (qd, qs):
        assert float(q[1, 2]) == INF and bool(torch.isfinite(q[[0, 2, 3], 2]).all()) and bool(torch.isfinite(q[:, :2]).all())
    # with a grid that culls everything: (0, 0, +inf) for all four
    empty = _sparse(net, hidden, inp, tps._grid('none'), 'softplus', level, level)[0]
    assert bool((_bits(empty[:, :2]) == 0).all()) and empty[:, 2].tolist() == [INF] * 4
    # and with the fitted ball's cells alone set the passing ray is culled where the others still cross
    ball = _sparse(net, hidden, inp, tps._grid('ball'), 'softplus', level, level)[0]
    assert float(ball[1, 2]) == INF and bool(torch.isfinite(ball[[0, 2, 3], 2]).all())


# ---------------------------------------------------------------------------------------------------------------- 7. NaN, guard bands, determinism
@pytest.mark.parametrize("hidden,Cn", [(128, 33), (256, 64)])
def test_an_infinite_origin_poisons_exactly_its_ray(hidden, Cn):
    net, grid = tp._net(hidden, 'fitted'), tps._grid('ball')
    inp = tp._inputs(7, Cn, 1, True, False)
    o2 = inp[0].clone()
    o2[5, 1] = INF
    bad = torch.zeros(7, dtype=torch.bool, device=DEV)
    bad[5] = True
    clean, dirty = _dense(net, hidden, inp, 'softplus', 0.5)[0], _dense(net, hidden, (o2,) + inp[1:], 'softplus', 0.5)[0]
    assert bool(torch.isnan(dirty[5]).all()) and torch.equal(_bits(dirty[~bad]), _bits(clean[~bad])) and not bool(torch.isnan(clean).any())
    clean, dirty = _sparse(net, hidden, inp, grid, 'softplus', 0.5, 0.5)[0], _sparse(net, hidden, (o2,) + inp[1:], grid, 'softplus', 0.5, 0.5)[0]
    assert bool(torch.isnan(dirty[5]).all()) and torch.equal(_bits(dirty[~bad]), _bits(clean[~bad])) and not bool(torch.isnan(clean).any())


@pytest.mark.parametrize("hidden", [128, 256])
def test_an_activation_outside_fp16_range_behind_the_crossing_leaves_q_finite(hidden):
    """tests/test_gpu_depth_sparse.py's rays: 32 samples in the scene, 32 more 3e4 away (outside the grid, live, overflowing).  The level lies
    between the transmittance after the first pass and 1: every ray crosses in the first pass.  Unstopped, depth and acc are NaN and q is the
    stopped run's bit for bit; the dense kernel calls the whole ray bad."""
    hot = tp._net(hidden, 'hot')
    grid = tps._grid('all')
    o, d, z_lo, z_hi, _ = tp._inputs(4, 32, 1, False, False, seed=5)[:5]
    near = _sparse(hot, hidden, (o, d, z_lo, z_hi, None), grid, 'softplus', 0., 0.5)
    zv = _dense(hot, hidden, (o, d, z_lo, z_hi, None), 'softplus', 0.5)[2]
    T_end = DM.quantile_ref(FR.alpha_ref(near[1], zv, False, False), zv, torch.ones(4, 32, dtype=torch.bool), 0.5)["T"][:, -1]
    assert float(T_end.max()) < 0.9, "the four rays are not opaque enough after 32 samples for this test: T %s" % T_end.tolist()
    level = _f32(0.5 * (1. + float(T_end.max())))
    z2 = torch.cat([z_lo, torch.linspace(3e4, 3.1e4, 32, device=DEV)])
    far = (o, d, z2, z2.clone(), None)
    full = _sparse(hot, hidden, far, grid, 'softplus', 0., level)
    stop = _sparse(hot, hidden, far, grid, 'softplus', level, level)
    assert full[4].tolist() == [2] * 4 and stop[4].tolist() == [1] * 4
    assert bool(torch.isnan(full[0][:, :2]).all()) and bool(torch.isfinite(full[0][:, 2]).all()) and bool(torch.isfinite(stop[0]).all())
    assert torch.equal(_bits(full[0][:, 2]), _bits(stop[0][:, 2]))
    assert bool((full[0][:, 2] >= z2[0]).all()) and bool((full[0][:, 2] <= z2[32]).all())      # (sample 31's neighbour is the first far one)
    assert bool(torch.isnan(_dense(hot, hidden, far, 'softplus', level)[0]).all())


def _guarded(n_words):
    buf = torch.full((n_words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, C.c_void_p(buf.data_ptr() + 4 * GUARD)


@pytest.mark.parametrize("hidden,kind,Cn,R,mode,jitter,pattern,level", [CASES[1], CASES[2], CASES[6], CASES[9], CASES[11]])
def test_the_entry_points_write_inside_their_outputs_and_twice_the_same(hidden, kind, Cn, R, mode, jitter, pattern, level):
    from nnr import lib as L
    from nnr import ops
    c = _case(hidden, kind, Cn, R, mode, jitter, pattern, level)
    o, d, z_lo, z_hi, jit = c["inp"][:5]
    grid, level = c["grid"], c["level"]
    cfg = ops.split2_cfg(R, Cn, hidden, **_kw(mode))
    packed = ops._packed_for(ops.split2_cfg(R, Cn, hidden), c["net"].weights(), c["net"].biases())
    lo3, is3, d3 = (C.c_float * 3)(*grid.lo), (C.c_float * 3)(*grid.inv_step), (C.c_int32 * 3)(*grid.dims)

    def check(sizes, launch, want):
        runs = []
        for _ in range(2):
            bufs = {k: _guarded(v) for k, v in sizes.items()}
            rc = launch(bufs)
            torch.cuda.synchronize()
            assert rc == 0
            for k, n in sizes.items():
                buf = bufs[k][0]
                assert bool((torch.cat([buf[:GUARD], buf[GUARD + n:]]) == SENTINEL).all()), "the kernel wrote outside " + k
            runs.append({k: bufs[k][0][GUARD:GUARD + n].clone() for k, n in sizes.items()})
        for k in sizes:
            assert torch.equal(runs[0][k], runs[1][k]), k
        assert not bool((runs[0]["out"] == SENTINEL).any()), "a ray was not written"
        assert torch.equal(runs[0]["out"].view(R, 3), _bits(want))
        return runs[0]

    got = check(dict(out=3 * R, raw=R * Cn, z=R * Cn),
                lambda b: L.load().nnr_render_depth_median(C.byref(cfg), L.ptr(o), L.ptr(d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), level, L.ptr(packed),
                                                           b["out"][1], b["raw"][1], b["z"][1], L.stream()), c["dense"][0])
    assert torch.equal(got["raw"].view(R, Cn), _bits(c["dense"][1])) and torch.equal(got["z"].view(R, Cn), _bits(c["dense"][2]))
    for t, want in ((0., c["full"]), (level, c["stop"])):
        got = check(dict(out=3 * R, raw=R * Cn, count=R, cell=R * Cn, passes=R),
                    lambda b: L.load().nnr_render_depth_median_sparse(C.byref(cfg), L.ptr(o), L.ptr(d), L.ptr(z_lo), L.ptr(z_hi), L.ptr(jit), lo3,
                                                                      is3, d3, L.ptr(grid.bits), float(t), level, L.ptr(packed), b["out"][1],
                                                                      b["raw"][1], b["count"][1], b["cell"][1], b["passes"][1], L.stream()),
                    want[0])
        assert torch.equal(got["count"], want[2]) and torch.equal(got["cell"].view(R, Cn), want[3]) and torch.equal(got["passes"], want[4])
        written = got["raw"].view(R, Cn) != SENTINEL      # untouched where not evaluated: the sentinel is still there
        assert torch.equal(written, _bits(want[1]) != NAN_FILL) and torch.equal(got["raw"].view(R, Cn)[written], _bits(want[1])[written])
    plain = ops.render_depth_sparse(o, d, z_lo, z_hi, jit, grid, c["net"].weights(), c["net"].biases(), hidden=hidden, t_min=level,
                                    quantile_level=level, **_kw(mode))
    assert torch.is_tensor(plain) and plain.shape == (R, 3) and torch.equal(_bits(plain), _bits(c["stop"][0]))


# ---------------------------------------------------------------------------------------------------------------- 8. the depth maps
def _median_maps_by_hand(renderer, K, Wm, size, level, grid, t_min):
    """render_depth_maps(depth_mode='median') spelled out with the public operators: ray_setup, the z tables, the op with quantile_level,
    column 2 over ray_norm"""
    from nnr import camera, ops
    from model.common import arange_pixels
    H, W = size
    dev = torch.device(DEV)
    cfg, net = renderer.cfg, renderer.model
    n = int(cfg['num_points']) - int(cfg['outside_steps'])
    pixels = arange_pixels((H, W), device=dev)[1]
    kw = dict(hidden=net.hidden_dim, dist_alpha=bool(cfg['dist_alpha']), relu_sigma=False, quantile_level=level)
    maps = []
    with torch.no_grad():
        z_lo, z_hi = renderer._z_tables(n, renderer.depth_range[0], renderer.depth_range[1], False, dev)
        for i in range(Wm.shape[0]):
            origin, ray, _, ray_norm, _, _ = camera.ray_setup(pixels, None, K.float().to(dev)[None], Wm[i].float().to(dev)[None],
                                                              torch.eye(4, device=dev)[None], bool(cfg['normalise_ray']), bool(cfg['use_ray_dir']))
            if grid is None:
                q = ops.render_depth(origin, ray, z_lo, z_hi, None, net.weights(), net.biases(), **kw)[:, 2]
            else:
                q = ops.render_depth_sparse(origin, ray, z_lo, z_hi, None, grid, net.weights(), net.biases(), t_min=t_min, **kw)[:, 2]
            maps.append((q / ray_norm if cfg['normalise_ray'] else q).view(H, W))
    return torch.stack(maps)


def test_render_depth_maps_in_median_mode_is_the_hand_made_composition():
    import test_gpu_fusion as tf
    from model import geometry as G
    renderer = tf._fitted_renderer(128)
    size = (24, 32)
    K = torch.diag(torch.tensor(FR.K_DIAG, dtype=torch.float64))
    Wm = FR.look_at_world_mats(14, 3.5)[[2, 9]]
    grid = tps._grid('ball')
    got = G.render_depth_maps(renderer, K, Wm, size, depth_mode='median', chunk=100)
    assert got.shape == (2,) + size and torch.equal(_bits(got), _bits(_median_maps_by_hand(renderer, K, Wm, size, 0.5, None, 0.)))
    assert bool(torch.isfinite(got).any()) and not bool(torch.isnan(got).any())
    with_grid = G.render_depth_maps(renderer, K, Wm, size, occupancy=grid, depth_mode='median', chunk=100)      # t_min: the level
    assert torch.equal(_bits(with_grid), _bits(_median_maps_by_hand(renderer, K, Wm, size, 0.5, grid, 0.5)))
    assert bool(torch.isinf(with_grid).any()) and bool(torch.isfinite(with_grid).any()) and not bool(torch.isnan(with_grid).any())
    for t in (0., 1e-3):      # a caller's smaller threshold is kept, and the maps are the same bits
        assert torch.equal(_bits(G.render_depth_maps(renderer, K, Wm, size, occupancy=grid, t_min=t, depth_mode='median')), _bits(with_grid))
    level3 = G.median_level(0.3)
    other = G.render_depth_maps(renderer, K, Wm, size, min_acc=0.3, occupancy=grid, depth_mode='median')
    assert torch.equal(_bits(other), _bits(_median_maps_by_hand(renderer, K, Wm, size, level3, grid, level3)))
    finite = torch.isfinite(other) & torch.isfinite(with_grid)
    assert bool((other[finite] <= with_grid[finite]).all())      # the 30 % quantile is not behind the median
    # the finite pixels are the observed ones of expected mode, up to rays whose acc lies within the bar of min_acc
    expected = G.render_depth_maps(renderer, K, Wm, size)
    acc_far = G.render_depth_maps(renderer, K, Wm, size, min_acc=0.5 + 1e-3)
    sure = torch.isfinite(acc_far)
    assert bool(torch.isfinite(got[sure]).all()) and int((torch.isfinite(got) != torch.isfinite(expected)).sum()) <= 0.02 * got.numel()


def test_expected_mode_is_bit_for_bit_the_parents_code_path():
    import test_gpu_fusion as tf
    from model import geometry as G
    renderer = tf._fitted_renderer(128)
    size = (24, 32)
    K = torch.diag(torch.tensor(FR.K_DIAG, dtype=torch.float64))
    Wm = FR.look_at_world_mats(14, 3.5)[[2, 9]]
    grid = tps._grid('ball')
    for kw in (dict(), dict(depth_mode='expected')):
        plain = G.render_depth_maps(renderer, K, Wm, size, chunk=100, **kw)
        assert torch.equal(_bits(plain), _bits(tds._maps_by_hand(renderer, K, Wm, size, 0.5, None, 0.)))
        sparse = G.render_depth_maps(renderer, K, Wm, size, occupancy=grid, t_min=1e-3, chunk=100, **kw)
        assert torch.equal(_bits(sparse), _bits(tds._maps_by_hand(renderer, K, Wm, size, 0.5, grid, 1e-3)))
        full = G.render_depth_maps(renderer, K, Wm, size, occupancy=grid, **kw)
        assert torch.equal(_bits(full), _bits(tds._maps_by_hand(renderer, K, Wm, size, 0.5, grid, 0.)))
