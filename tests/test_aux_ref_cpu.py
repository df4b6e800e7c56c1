"""Pins tests/aux_ref.py, the fp64 definition that tests/test_gpu_aux_direct.py holds the per-image loss kernels against.  No GPU.
  * composed with the oracle's poses, distortions and image resize it reproduces the step recorded from the reference project
    (tests/golden/aux_terms.npz): the definition is tied to the reference, not to this project's kernels;
  * every GPU case keeps every decision (clamps, the behind test, the mask, nearest neighbours, pixel cells, |u| and SSIM clamps) at
    least 1e-4 away from its threshold, so fp32 kernels and the fp64 reference take the same branches at every point;
  * every case holds enough points of each branch;
  * the recorded fp32-vs-fp64 noise of the reference, which the GPU tolerances are multiples of, is current."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aux_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "aux_terms.npz"))


@functools.lru_cache(maxsize=None)
def _eval(name):
    return R.evaluate(R.CASES[name])


def _golden_chain(name, ssim, pieces=torch.float32):
    """The recorded step through the oracle's pieces and the reference.  The pieces -- poses, matrix inverses, distortions, the image
    resize, the relative transform -- run in `pieces`: fp32 is how the recording formed them (its inverses alone put 3e-6 between an
    all-fp64 chain and the recorded gradients); the reference itself always runs in fp64, and autograd carries its gradients back
    through the casts into the pieces."""
    import nerf_oracle as orc
    inp = lambda k: torch.from_numpy(GOLD[f"{name}.in.{k}"]).to(pieces)
    cam, ref = int(GOLD[f"{name}.cam"]), int(GOLD[f"{name}.ref"])
    leaves = {k: inp(k).requires_grad_(True) for k in ("pose_r", "pose_t", "scales", "shifts")}
    n_cams = leaves["pose_r"].shape[0]
    dpt, ref_dpt, img, ref_img, K = inp("dpt")[0], inp("ref_dpt")[0], inp("img"), inp("ref_img"), inp("K")[0]
    # the inputs of the per-image terms as aux_scope forms them (model/training.py:238-313): this frame's world matrix and distorted depth,
    # the detached reference side, the relative transform and the roles of the two frames (swapped for the last camera)
    world = torch.inverse(orc.pose_c2w(leaves["pose_r"][cam], leaves["pose_t"][cam]))
    sc, sh = orc.distortion(leaves["scales"], leaves["shifts"], cam, n_cams)
    depth = dpt * sc + sh
    sc_r, sh_r = orc.distortion(leaves["scales"], leaves["shifts"], ref, n_cams)
    ref_rt = torch.inverse(orc.pose_c2w(leaves["pose_r"][ref], leaves["pose_t"][ref]).detach())
    depth_r, sc_r = (sc_r * ref_dpt + sh_r).detach(), sc_r.detach()
    if cam < n_cams - 1:
        d1, d2, i1, i2, rel, scale2 = depth, depth_r, img, ref_img, ref_rt @ torch.inverse(world), sc_r
    else:
        d1, d2, i1, i2, rel, scale2 = depth_r, depth, ref_img, img, world @ torch.inverse(ref_rt), sc
    res = (dpt.shape[-2] // 4, dpt.shape[-1] // 4)
    i1, i2 = F.interpolate(i1, res, mode="bilinear")[0], F.interpolate(i2, res, mode="bilinear")[0]
    f64 = lambda t: t.double()
    l_pc, l_rgbs, _, _ = R.aux_ref(f64(d1), f64(d2), f64(rel), f64(scale2), f64(i1), f64(i2), f64(K), f64(torch.inverse(K)), res, 0.01,
                                   rgb_s=True, pc=True, scale_pcs=True, detach_rgbs_scale=False, ssim=ssim)
    (l_pc + l_rgbs).backward()
    return l_pc, l_rgbs, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in leaves.items()}


@pytest.mark.parametrize("name", ["mid", "last"])
def test_reference_chained_to_the_oracle_inputs_reproduces_the_recorded_losses(name):
    l_pc, l_rgbs, _ = _golden_chain(name, False)
    np.testing.assert_allclose(l_pc.item(), float(GOLD[f"{name}.out.loss_pc"]), rtol=0, atol=1e-6)
    np.testing.assert_allclose(l_rgbs.item(), float(GOLD[f"{name}.out.loss_rgb_s"]), rtol=0, atol=1e-6)


@pytest.mark.parametrize("name", ["mid", "last"])
def test_reference_chained_to_the_oracle_inputs_reproduces_the_recorded_gradients(name):
    """At 2e-6, the tolerance tests/test_aux_terms.py uses for the fp32 oracle.  Measured: at most 7.2e-7 (mid: scales, last: pose_t
    and shifts)."""
    _, _, grads = _golden_chain(name, False)
    for k, g in grads.items():
        np.testing.assert_allclose(g, GOLD[f"{name}.gaux.{k}"], rtol=0, atol=2e-6, err_msg=k)


@pytest.mark.parametrize("name,ssim", [("mid", False), ("last", False), ("mid", True), ("last", True)])
def test_reference_equals_the_oracles_expression_evaluated_in_fp64(name, ssim, monkeypatch):
    """aux_scope is the reference project's own expression.  Its pixel grid holds fp32 values whatever the dtype (6e-8 off the exact
    x' = 2x/(wr-1) - 1); with the exact grid in its place nothing but fp64 rounding is left between the two."""
    import nerf_oracle as orc
    l_pc, l_rgbs, grads = _golden_chain(name, ssim, pieces=torch.float64)

    def exact_grid(h, w):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
        return torch.stack([2 * xs / (w - 1) - 1, 2 * ys / (h - 1) - 1], dim=-1).reshape(1, -1, 2)

    monkeypatch.setattr(orc, "pixel_grid", exact_grid)
    torch.set_default_dtype(torch.float64)
    try:
        inp = {k: torch.from_numpy(GOLD[f"{name}.in.{k}"]).double() for k in ("K", "img", "ref_img", "dpt", "ref_dpt", "pose_r", "pose_t", "scales", "shifts")}
        leaves = {k: inp[k].clone().requires_grad_(True) for k in ("pose_r", "pose_t", "scales", "shifts")}
        aux, o_pc, o_rgbs = orc.aux_scope(leaves["pose_r"], leaves["pose_t"], leaves["scales"], leaves["shifts"], int(GOLD[f"{name}.cam"]),
                                          int(GOLD[f"{name}.ref"]), inp["K"], inp["dpt"].unsqueeze(1), inp["ref_dpt"].unsqueeze(1), inp["img"],
                                          inp["ref_img"], with_ssim=ssim)
        aux.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    assert abs(float(o_pc) - float(l_pc)) <= 1e-12 and abs(float(o_rgbs) - float(l_rgbs)) <= 1e-12
    for k, g in grads.items():
        og = leaves[k].grad.numpy() if leaves[k].grad is not None else np.zeros_like(g)
        np.testing.assert_allclose(g, og, rtol=0, atol=1e-10, err_msg=k)


def test_reference_with_ssim_reproduces_the_recorded_step():
    """The expected gradients as test_aux_terms.py derives them: the recorded step with SSIM minus the render part of the plain step."""
    l_pc, l_rgbs, grads = _golden_chain("mid", True)
    np.testing.assert_allclose(l_pc.item(), float(GOLD["mid_ssim.out.loss_pc"]), rtol=0, atol=1e-6)
    np.testing.assert_allclose(l_rgbs.item(), float(GOLD["mid_ssim.out.loss_rgb_s"]), rtol=0, atol=1e-6)
    for k, g in grads.items():
        want = GOLD[f"mid_ssim.g.{k}"] - (GOLD[f"mid.g.{k}"] - GOLD[f"mid.gaux.{k}"])
        np.testing.assert_allclose(g, want, rtol=0, atol=5e-6, err_msg=k)


@pytest.mark.parametrize("name", list(R.CASES))
def test_no_decision_of_a_gpu_case_lies_within_1e_4_of_its_threshold(name):
    """A condition on the inputs (seeds and poses are chosen to meet it): no point is excluded from any comparison on the GPU."""
    m = _eval(name)["margins"]
    close = {k: v for k, v in m.items() if not k.startswith("n_") and v < 1e-4}
    assert not close, close


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_case_holds_enough_points_of_each_branch(name):
    c, m = R.CASES[name], _eval(name)["margins"]
    S = c.grid[0] * c.grid[1]
    if c.rich:
        assert m["n_clamp1"] >= 10 and m["n_clamp2"] >= 10, m
    if c.rich and c.rgb_s:
        assert 10 <= m["n_behind"] <= S - 10, m
        if c.pose is R.POSE_AWAY:
            assert m["n_valid"] == 0, m      # (and S - n_behind points in front of the camera project outside too)
        else:
            assert 0.3 * S <= m["n_valid"] <= 0.8 * S, m
            if c.ssim and c.shard == (0, 0):
                assert m["n_centre_col0"] >= 1 and m["n_centre_last_col"] >= 1, m
                assert m["n_centre_block_edge"] == 2, m      # points 255 and 256: each gathers from a centre in the other block
    if not c.rich and c.rgb_s:      # the 2 x 3 and 2 x 2 grids: some point valid, some not
        assert 1 <= m["n_valid"] < S, m
    if c.rgb_s and c.shard != (0, 0):      # a shard that holds no re-projection term would test nothing
        assert float(_eval(name)["loss_rgb_s"]) > 0.01


@pytest.mark.parametrize("name", list(R.CASES))
def test_recorded_rounding_noise_is_current(name):
    got, table = R.rounding_noise(R.CASES[name]), R.NOISE[name]
    assert set(got) == set(table)
    for k, v in got.items():
        assert (v == 0.0 and table[k] == 0.0) or 0.5 * table[k] <= v <= 2.0 * table[k], (k, v, table[k])


@pytest.mark.parametrize("ssim", ["", "_ssim"])
def test_shards_of_the_reference_add_up_to_the_whole(ssim):
    whole, a, b = _eval("ssim" if ssim else "both"), _eval("shard_0_100" + ssim), _eval("shard_100_273" + ssim)
    for k in R.OUTPUTS:
        if whole[k] is not None:
            assert float((a[k] + b[k] - whole[k]).abs().max()) <= 1e-12 * max(1.0, float(whole[k].abs().max())), k


def test_nearest_indices_are_those_of_interpolate_on_the_map_itself():
    g = torch.Generator().manual_seed(0)
    for (hd, wd), (hr, wr) in [((52, 84), (13, 21)), ((50, 83), (13, 21)), ((13, 21), (13, 21)), ((14, 22), (13, 21)), ((5, 7), (2, 3))]:
        d = torch.rand(hd, wd, generator=g)
        idx = R.nearest_indices(hd, wd, hr, wr)
        assert torch.equal(d.view(-1)[idx], F.interpolate(d[None, None], (hr, wr), mode="nearest").view(-1))
        assert torch.equal(d.double().view(-1)[idx], F.interpolate(d.double()[None, None], (hr, wr), mode="nearest").view(-1))
        assert idx.unique().numel() == hr * wr      # a map at least as fine as the grid: every point reads a pixel of its own
