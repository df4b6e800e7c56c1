"""The exhaustive nearest-neighbour search (csrc/nnr_pointcloud.hip: nnr_pc_nearest) against the exact integer reference of
tests/pc_ref.py, bit for bit, and its backward (nnr_pc_error_bwd) against float64 with a derived bound.

This search is the product path of the point-cloud loss outside the fused per-image block AND the yardstick of every test of the
ray-aware search (tests/test_gpu_pc_search.py), so it is checked here on inputs that reach its edges: ties at the minimum and rounded
square roots that collide (the (sqrt bits, index) order), destination ranges of several LDS tiles with padded tails, tiny shapes,
subnormal d2, exact duplicates, sources without a match, and -- in child processes -- its other configurations (NNR_PC_WGS, NNR_PC_SEED,
NNR_PC_PER, each read once per process)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pc_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (5, 3), (63, 7), (256, 8), (257, 255), (300, 256), (300, 257), (700, 7), (700, 1023), (700, 1025),
          (1300, 2100), (300, 2500)]      # (300, 2500): with NNR_PC_WGS=1 one range of 1024 + 1024 + 452 points (452 = 56 * 8 + 4)


def _nearest(x, y):
    from nnr import pointcloud
    idx, dist = pointcloud.nearest(x.cuda(), y.cuda())
    return idx.cpu(), dist.cpu()


def _assert_same(idx, dist, ref_idx, ref_dist, what=""):
    bad = idx != ref_idx
    assert not bad.any(), "%s: %d of %d indices differ, first at source %d: got %d, expected %d" % (
        what, int(bad.sum()), idx.numel(), int(bad.nonzero()[0]), int(idx[bad][0]), int(ref_idx[bad][0]))
    assert torch.equal(dist.view(torch.int32), ref_dist.view(torch.int32)), "%s: distance bits differ" % what


@functools.lru_cache(maxsize=None)
def _lattice_case(S, D, hi):
    xi, yi = pc_ref.lattice_pair(S, D, hi)
    return (xi, yi) + pc_ref.lattice_nearest(xi, yi)


# ---- forward ----

@pytest.mark.parametrize("hi", [6, 512])
@pytest.mark.parametrize("S,D", SHAPES)
def test_fwd_shape_edges(S, D, hi):
    xi, yi, ref_idx, ref_dist = _lattice_case(S, D, hi)
    idx, dist = _nearest(xi.float(), yi.float())
    _assert_same(idx, dist, ref_idx, ref_dist, "%d x %d, coordinates < %d" % (S, D, hi))


@pytest.mark.parametrize("X", [2800, 2801, 3500])
def test_fwd_collision_plane(X):
    """Different d2 under one rounded square root: the lower index wins, not the lower d2 (tests/test_pc_ref_cpu.py counts the sources
    where the two differ).  Both directions."""
    src, dst = pc_ref.collision_plane(X)
    for a, b, what in ((src, dst, "plane -> half"), (dst, src, "half -> plane")):
        _assert_same(*_nearest(a.float(), b.float()), *pc_ref.lattice_nearest(a, b), what="X = %d, %s" % (X, what))


def test_fwd_exact_duplicates():
    src, dst = pc_ref.triplicated_pair(600, 500, 512)
    ref_idx, ref_dist = pc_ref.lattice_nearest(src, dst)
    idx, dist = _nearest(src.float(), dst.float())
    _assert_same(idx, dist, ref_idx, ref_dist, "triplicated destinations")
    # the reference's own answer is the lowest of the three copies, at distance +0.0 where the source is one of them
    first = {}
    for j, p in enumerate(map(tuple, dst.tolist())):
        first.setdefault(p, j)
    assert all(int(idx[s]) == first[tuple(src[s].tolist())] for s in range(300))
    assert torch.equal(dist[:300].view(torch.int32), torch.zeros(300, dtype=torch.int32))


@pytest.mark.parametrize("e", [-70, -20, 50])
@pytest.mark.parametrize("hi", [6, 512])
def test_fwd_scales(hi, e):
    """Coordinates times 2^e: the same indices, the distances times 2^e.  At 2^-70 d2 = n * 2^-140 is subnormal up to n < 2^14 (all of
    the tie lattice, the near pairs of the sparse one) and still exact; the kernel's pruning threshold must not cut them off."""
    xi, yi, ref_idx, ref_dist = _lattice_case(700, 3000, hi)
    want = (ref_dist.double() * 2.0 ** e).float()
    assert torch.equal(want.double(), ref_dist.double() * 2.0 ** e)
    idx, dist = _nearest(pc_ref.scaled(xi, e), pc_ref.scaled(yi, e))
    _assert_same(idx, dist, ref_idx, want, "coordinates < %d, scale 2^%d" % (hi, e))


def test_fwd_general_position_against_the_oracle():
    """Random float clouds: the indices of the oracle (the reference's own expression).  The distance is held to float64 within
    3 * 2^-24: d2 carries the roundings of the three differences (2 * 2^-24 on each square) and of the product and the two fmas
    (3 * 2^-24), the square root halves that and adds its own 2^-25."""
    import nerf_oracle as orc
    for S, D in ((700, 650), (1300, 2100)):
        x, y = pc_ref.float_pair(S, D, seed=S)
        idx, dist = _nearest(x, y)
        assert torch.equal(idx, orc.closest_idx(x.t(), y.t())), (S, D)
        want = (x.double() - y.double()[idx]).norm(dim=1)
        assert bool(((dist.double() - want).abs() <= 3 * 2.0 ** -24 * want).all()), (S, D)


def test_fwd_no_match():
    """A source with a NaN or an infinite coordinate matches nothing: index 0xffffffff; every other source is unaffected.  Forward only:
    the backward's guard against this index (it would be a read tens of GB past the destination cloud) is not exercised on the GPU."""
    xi, yi, ref_idx, ref_dist = _lattice_case(700, 1025, 512)
    x = xi.float()
    bad = torch.tensor([0, 1, 255, 256, 300, 511, 698, 699])
    fill = [float("nan"), float("inf"), -float("inf"), float("nan")]
    for n, s in enumerate(bad.tolist()):
        x[s, n % 3] = fill[n % 4]
    idx, dist = _nearest(x, yi.float())
    assert bool((idx[bad] == pc_ref.NO_MATCH).all()), idx[bad]
    keep = torch.ones(700, dtype=torch.bool)
    keep[bad] = False
    _assert_same(idx[keep], dist[keep], ref_idx[keep], ref_dist[keep], "the sources beside the unmatched ones")


def test_yardstick_size():
    """32 400 x 32 400 (the first training phase's clouds), coordinates < 48: the kernel runs every source, the reference the first 256,
    the last 256 and 4096 random ones."""
    n = 32400
    xi, yi = pc_ref.lattice_pair(n, n, 48)
    g = torch.Generator().manual_seed(9)
    sel = torch.cat([torch.arange(256), torch.arange(n - 256, n), torch.randperm(n, generator=g)[:4096]])
    idx, dist = _nearest(xi.float(), yi.float())
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    _assert_same(idx[sel], dist[sel], *pc_ref.lattice_nearest(xi[sel], yi), what="32 400 x 32 400")


# ---- backward ----

def _bwd(x, y, g=1.0, want_src=True, want_dst=True, prefill=None):
    """nnr_pc_error_bwd through the C ABI on the kernel's own match -> (idx, g_src | None, g_dst | None), on the host."""
    from nnr import lib as L
    from nnr import pointcloud
    lib = L.load()
    xd, yd = x.cuda().contiguous(), y.cuda().contiguous()
    idx, dist = pointcloud.nearest(xd, yd)
    assert int(idx.max()) < y.shape[0]                      # every source matched: nothing below reads past the destinations
    gl = torch.tensor([g], dtype=torch.float32, device="cuda")
    g_src = torch.full_like(xd, float("nan")) if want_src else None      # written, never accumulated: the NaN must be gone
    g_dst = (torch.zeros_like(yd) if prefill is None else prefill.cuda().clone()) if want_dst else None
    L.check(lib.nnr_pc_error_bwd(L.ptr(xd), L.ptr(yd), L.ptr(idx), L.ptr(dist), L.ptr(gl), x.shape[0], y.shape[0], L.ptr(g_src),
                                 L.ptr(g_dst), L.stream()), "nnr_pc_error_bwd")
    torch.cuda.synchronize()
    return idx.cpu(), None if g_src is None else g_src.cpu(), None if g_dst is None else g_dst.cpu()


def _check_bwd(x, y, g=1.0, want_src=True, want_dst=True, prefill=None):
    idx, g_src, g_dst = _bwd(x, y, g, want_src, want_dst, prefill)
    r_src, r_dst, m, sum_abs = pc_ref.error_grads_fp64(x, y, idx, g)
    u = 2.0 ** -24
    if want_src:
        # g/(S dist) (src - dst): the distance (3 u, see the forward), S * dist, the quotient, the difference and the product (u each):
        # 7 u, bounded by 8 u of the element, plus one fp32 ulp of the row's largest element
        assert bool(torch.isfinite(g_src).all())
        ulp = torch.from_numpy(np.spacing(r_src.abs().max(dim=1, keepdim=True).values.float().numpy())).double()
        err = (g_src.double() - r_src).abs()
        assert bool((err <= 8 * u * r_src.abs() + ulp).all()), "g_src: %.3g over the bound" % float((err - 8 * u * r_src.abs() - ulp).max())
        zero = (x.double() - y.double()[idx]).norm(dim=1) == 0
        assert not g_src[zero].any()
    if want_dst:
        # m sequential fp32 additions of terms that carry 7 u each: (m + 8) u * sum |term|
        assert bool(torch.isfinite(g_dst).all())
        bound = (m[:, None].double() + 8) * u * sum_abs
        got = g_dst.double()
        if prefill is not None:
            # g_dst += acc: one more rounding, of the sum (at most u (|prefill| + |acc|)); the float64 difference below is exact
            bound = bound + u * (prefill.double().abs() + sum_abs)
            got = got - prefill.double()
        err = (got - r_dst).abs()
        assert bool((err <= bound).all()), "g_dst: %.3g over the bound" % float((err - bound).max())
        if prefill is None:
            assert not g_dst[m == 0].any()
    return idx, m


def test_bwd_many_sources_per_destination_over_four_tiles():
    x, y = pc_ref.float_pair(1000, 3, seed=21)
    idx, m = _check_bwd(x, y)
    assert int(m.min()) >= 100                              # hundreds of terms per destination, spread over the four tiles of 256 matches
    for j in range(3):
        assert len(set((idx == j).nonzero().flatten().div(256, rounding_mode="floor").tolist())) == 4


def test_bwd_one_destination():
    x, y = pc_ref.float_pair(700, 1, seed=22)
    _check_bwd(x, y)


def test_bwd_one_source_and_threads_beyond_it():
    x, y = pc_ref.float_pair(1, 700, seed=23)
    _check_bwd(x, y)


def test_bwd_general_position_and_upstream_gradient():
    x, y = pc_ref.float_pair(700, 650, seed=24)
    _check_bwd(x, y)
    _check_bwd(x, y, g=3.0)


def test_bwd_zero_distances_give_zero_rows():
    src, dst = pc_ref.triplicated_pair(600, 100, 512, seed=2)      # the first 300 sources coincide with destinations
    idx, _ = _check_bwd(src.float(), dst.float())
    assert int((pc_ref.lattice_d2(src, dst, idx) == 0).sum()) >= 300


def test_bwd_one_gradient_only():
    x, y = pc_ref.float_pair(700, 650, seed=25)
    _check_bwd(x, y, want_dst=False)
    _check_bwd(x, y, want_src=False)
    _check_bwd(*pc_ref.float_pair(300, 700, seed=26), want_src=False)      # more destinations than sources


def test_bwd_accumulates_into_g_dst():
    x, y = pc_ref.float_pair(700, 650, seed=27)
    g = torch.Generator().manual_seed(28)
    _check_bwd(x, y, g=3.0, prefill=1e-3 * torch.randn(650, 3, generator=g))


# ---- the kernel's other configurations ----

#: (environment, seconds).  A child took 4.1 - 4.5 s on an MI355X machine when this was written (2.3 - 2.6 s of it pytest's own): the limit
#: leaves a factor of ~14 for a busy host
VARIANTS = [({"NNR_PC_WGS": "1"}, 60), ({"NNR_PC_SEED": "0"}, 60), ({"NNR_PC_SEED": "1"}, 60), ({"NNR_PC_PER": "2"}, 60),
            ({"NNR_PC_PER": "2", "NNR_PC_WGS": "1"}, 60)]


def test_other_configurations_in_child_processes():
    """NNR_PC_WGS=1: ONE destination range, so D = 2100 / 2500 run tiles of 1024 + 1024 + a remainder that is no multiple of 8.
    NNR_PC_SEED=0 / 1: ranges that start from +infinity / from the key already there (the default also seeds from the points around the
    source's own index).  NNR_PC_PER=2: the two-sources-per-lane kernel.  The knobs are read once per process: the forward cases above
    again (without the 32 400 one), one child at a time, nothing more started after a child that did not end with 0."""
    for extra, limit in VARIANTS:
        env = dict(os.environ)
        for k in ("NNR_PC_WGS", "NNR_PC_SEED", "NNR_PC_PER"):
            env.pop(k, None)
        env.update(extra)
        try:
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "test_fwd_",
                                "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired as ex:
            pytest.fail("%s: no end after %d s\n%s" % (extra, limit, (ex.stdout or "")[-3000:]))
        assert r.returncode == 0, "%s: exit %d\n%s%s" % (extra, r.returncode, r.stdout[-3000:], r.stderr[-2000:])
        assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-3000:]
        print("%s: %s" % (extra, r.stdout.strip().splitlines()[-1]))
