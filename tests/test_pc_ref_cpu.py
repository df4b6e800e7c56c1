"""The exact integer reference of tests/pc_ref.py against the oracle, and the conditions that make the lattice inputs of
tests/test_gpu_pc_nearest.py worth running (ties at the minimum; rounded square roots that collide).  No GPU."""
import pytest
import torch

import pc_ref


@pytest.mark.parametrize("hi", [6, 512, 2300])
def test_lattice_reference_equals_the_oracle(hi):
    import nerf_oracle as orc
    xi, yi = pc_ref.lattice_pair(700, 3000, hi)
    idx, dist = pc_ref.lattice_nearest(xi, yi)
    x, y = xi.float(), yi.float()
    assert torch.equal(idx, orc.closest_idx(x.t(), y.t()))
    assert torch.equal(dist, pc_ref.rounded_sqrt(pc_ref.lattice_d2(xi, yi, idx))[0])
    # chunking over the sources changes nothing
    idx_c, dist_c = pc_ref.lattice_nearest(xi, yi, chunk=37)
    assert torch.equal(idx, idx_c) and torch.equal(dist, dist_c)


def test_rounded_sqrt_is_the_correctly_rounded_root_and_top_its_last_integer():
    """rounded_sqrt verifies its own rounding (midpoints squared, exactly); here `top` against the definition, on the ranges the inputs
    live in: small d2, and d2 near 7.8 M and 12 M where several integers share one root."""
    for lo, hi in ((0, 200000), (2800 ** 2 - 50000, 2800 ** 2 + 50000), (3500 ** 2 - 50000, 3500 ** 2 + 50000), (2 ** 24 - 100000, 2 ** 24)):
        n = torch.arange(lo, hi, dtype=torch.int64)
        r, top = pc_ref.rounded_sqrt(n)
        assert bool((r[1:] >= r[:-1]).all())                                      # monotone
        last = torch.cat([r[1:] > r[:-1], torch.tensor([False])])                 # n is the last integer of its root
        assert bool((top[last] == n[last]).all()) and bool((top >= n).all())
        same = r[1:] == r[:-1]
        assert bool((top[1:][same] == top[:-1][same]).all())
    assert int((pc_ref.rounded_sqrt(torch.arange(7840000, 7840100))[0].unique()).numel()) < 100      # roots do collide there


def test_tie_lattice_has_ties_at_the_minimum():
    xi, yi = pc_ref.lattice_pair(700, 3000, 6)
    _, cnt = pc_ref.min_d2(xi[:256], yi)
    n = int((cnt >= 2).sum())
    print("tie lattice: %d of 256 sources have >= 2 destinations at the minimum d2" % n)
    assert n == 256


@pytest.mark.parametrize("X", [2800, 2801, 3500])
def test_collision_plane_winner_is_often_not_a_minimum_of_d2(X):
    """A search that ordered candidates by d2 (first index among the minima of d2) answers differently on exactly these sources."""
    src, dst = pc_ref.collision_plane(X)
    assert src.shape == (1024, 3) and dst.shape == (512, 3)
    idx, _ = pc_ref.lattice_nearest(src, dst)
    lo, _ = pc_ref.min_d2(src, dst)
    n = int((pc_ref.lattice_d2(src, dst, idx) > lo).sum())
    print("collision plane X = %d: the (sqrt, index) winner of %d of 1024 sources has a d2 above the minimum" % (X, n))
    assert n >= 100


def test_error_grads_fp64_equal_autograd():
    x, y = pc_ref.float_pair(300, 40, seed=2)
    x[:5] = y[:5]                                            # zero distances: zero rows
    idx = torch.cdist(x.double(), y.double()).argmin(dim=1)
    g_src, g_dst, m, sum_abs = pc_ref.error_grads_fp64(x, y, idx, 3.0)
    xa, ya = x.double().requires_grad_(True), y.double().requires_grad_(True)
    (3.0 * (xa - ya[idx]).norm(dim=1).mean()).backward()
    assert torch.allclose(g_src, xa.grad, rtol=1e-12, atol=1e-15) and torch.allclose(g_dst, ya.grad, rtol=1e-12, atol=1e-15)
    assert not g_src[:5].any() and int(m.sum()) == 300 and bool((sum_abs >= g_dst.abs() - 1e-15).all())
