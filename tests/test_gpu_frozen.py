"""GPU (-m gpu): the frozen-field render (include/nnr_frozen.h) against the training path it replaces for test-time
pose refinement.  Statement throughout: BIT equality -- the frozen kernels are the training kernels without their stash stores, the
arithmetic of a sample is the same instruction sequence -- for the outputs and the ray gradients, through the C ABI with own buffers, through
nnr.render_rays, through model.Trainer_pose against the reference's golden, and over a 20-step refinement run."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nope-nerf_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

import nerf_oracle as orc      # noqa: E402

pytestmark = pytest.mark.gpu
SENTINELS = 4096
# (rays, samples, dist_alpha, relu_sigma, jitter): ray mode in one pass and in two, flat mode with padded chunks; each switch on once
CASES = [(8, 32, False, False, True), (4, 64, True, False, False), (5, 130, False, True, True), (3, 33, False, False, False)]
IDS = ["ray_8x32_jitter", "ray_4x64_dist_alpha", "flat_5x130_relu_sigma_jitter", "flat_3x33"]
OUT_KEYS = ("rgb", "dist", "alpha", "z", "d_pts_o", "d_pts_d", "d_view")


def _inputs(R, N, jitter, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    o = torch.randn(R, 3, generator=g) * 0.1
    z = torch.linspace(0, 1, N)
    z = 0.01 * (1 - z) + 10 * z
    mid = 0.5 * (z[1:] + z[:-1])
    # upstream gradients over fourteen orders of magnitude from ray to ray, as the compositing weights make them
    mag = 10.0 ** (torch.rand(R, 1, generator=g) * 14.0 - 12.0)
    t = dict(pts_o=o, pts_d=d, view_d=-d, z_lo=torch.cat([z[:1], mid]), z_hi=torch.cat([mid, z[-1:]]),
             jitter=torch.rand(R, N, generator=g) if jitter else None,
             d_rgb=torch.randn(R, 3, generator=g) * mag, d_dist=torch.randn(R, generator=g) * mag[:, 0])
    return {k: (v.cuda().contiguous() if v is not None else None) for k, v in t.items()}


def _params(D, seed, scale=None):
    from nnr import lib as L
    p = orc.init_params(D, seed)
    for k, s in (scale or {}).items():
        for name in p:
            if name.startswith(k) and name.endswith(".weight"):
                p[name] = p[name] * s
    return [p[n + ".weight"].cuda().contiguous() for n in L.LAYER_NAMES], [p[n + ".bias"].cuda().contiguous() for n in L.LAYER_NAMES]


def _render(D, R, N, dist_alpha, relu_sigma, inp, w, b, frozen, guard=False):
    """nnr_render_fwd + nnr_render_bwd on a training workspace (frozen=False) or nnr_frozen_fwd + nnr_frozen_bwd on a frozen one, own
    buffers -> the seven results.  guard: the frozen workspace starts as NaN with SENTINELS floats behind its end, which must survive."""
    from nnr import lib as L
    from nnr import ops
    lib = L.load()
    dev = torch.device("cuda")
    cfg = L.make_cfg(R, N, D, dist_alpha=dist_alpha, relu_sigma=relu_sigma, train=True)
    assert cfg.flags & L.NNR_F_SPLIT2
    st = L.stream()
    packed = torch.empty(lib.nnr_packed_floats(C.byref(cfg)), device=dev)
    L.check(lib.nnr_pack_weights(C.byref(cfg), C.byref(L.params_struct(w, b)), L.ptr(packed), st), "pack")
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(rgb=torch.empty(R, 3, **f32), dist=torch.empty(R, **f32), alpha=torch.empty(R, N, **f32), z=torch.empty(R, N, **f32),
               d_pts_o=torch.empty(R, 3, **f32), d_pts_d=torch.empty(R, 3, **f32), d_view=torch.empty(R, 3, **f32))
    fwd_in = [L.ptr(inp[k]) for k in ("pts_o", "pts_d", "view_d", "z_lo", "z_hi", "jitter")]
    if frozen:
        n = lib.nnr_frozen_workspace_floats(C.byref(cfg))
        assert n > 0
        buf = torch.full((n + SENTINELS,), float("nan") if guard else 0.0, **f32)
        mark = torch.arange(SENTINELS, **f32) + 0.5
        buf[n:] = mark
        ws = buf[:n]
        L.check(lib.nnr_frozen_fwd(C.byref(cfg), *fwd_in, L.ptr(packed), L.ptr(out["rgb"]), L.ptr(out["dist"]), L.ptr(out["alpha"]), L.ptr(out["z"]),
                                   L.ptr(ws), st), "nnr_frozen_fwd")
        L.check(lib.nnr_frozen_bwd(C.byref(cfg), L.ptr(packed), L.ptr(inp["d_rgb"]), L.ptr(inp["d_dist"]), L.ptr(out["d_pts_o"]),
                                   L.ptr(out["d_pts_d"]), L.ptr(out["d_view"]), L.ptr(ws), st), "nnr_frozen_bwd")
        torch.cuda.synchronize()
        assert torch.equal(buf[n:], mark), "the frozen path wrote behind its workspace"
    else:
        ws = torch.zeros(lib.nnr_workspace_floats(C.byref(cfg)), **f32)
        gw, gb = [torch.empty_like(x) for x in w], [torch.empty_like(x) for x in b]
        L.check(lib.nnr_render_fwd(C.byref(cfg), *fwd_in, L.ptr(packed), L.ptr(out["rgb"]), L.ptr(out["dist"]), L.ptr(out["alpha"]), L.ptr(out["z"]),
                                   L.ptr(ws), st), "nnr_render_fwd")
        L.check(lib.nnr_render_bwd(C.byref(cfg), L.ptr(packed), L.ptr(inp["d_rgb"]), L.ptr(inp["d_dist"]), C.byref(L.params_struct(gw, gb)),
                                   L.ptr(out["d_pts_o"]), L.ptr(out["d_pts_d"]), L.ptr(out["d_view"]), L.ptr(ops._plan_for(cfg, dev)), L.ptr(ws), st),
                "nnr_render_bwd")
        torch.cuda.synchronize()
    return out


_memo = {}


def _pair(D, case):
    """(training path, frozen path) of one case, computed once for the tests that share it."""
    key = (D,) + tuple(case)
    if key not in _memo:
        R, N, dist_alpha, relu_sigma, jitter = case
        inp = _inputs(R, N, jitter, seed=100 * D + R)
        w, b = _params(D, seed=D + N)
        _memo[key] = (inp, w, b, _render(D, R, N, dist_alpha, relu_sigma, inp, w, b, False), _render(D, R, N, dist_alpha, relu_sigma, inp, w, b, True))
    return _memo[key]


# ------------------------------------------------------------------------------------------------------------ 1, 2: the C ABI
@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("D", [128, 256])
def test_frozen_entry_points_equal_the_training_path_bit_for_bit(D, case):
    _, _, _, train, frozen = _pair(D, case)
    for k in OUT_KEYS:
        assert torch.isfinite(train[k]).all(), k
        assert torch.equal(train[k], frozen[k]), (k, float((train[k] - frozen[k]).abs().max()))
    assert float(train["d_pts_d"].abs().max()) > 0.0 and float(train["d_view"].abs().max()) > 0.0      # (the comparison is not of zeros)


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("D", [128, 256])
def test_frozen_path_reads_nothing_it_did_not_write_and_writes_nothing_outside(D, case):
    inp, w, b, train, frozen = _pair(D, case)
    R, N, dist_alpha, relu_sigma, _ = case
    guarded = _render(D, R, N, dist_alpha, relu_sigma, inp, w, b, True, guard=True)      # (asserts the sentinels itself)
    for k in OUT_KEYS:
        assert torch.equal(guarded[k], frozen[k]) and torch.equal(guarded[k], train[k]), k


# ------------------------------------------------------------------------------------------------------------ 3: range behaviour
@pytest.mark.parametrize("D", [128, 256])
def test_samples_that_leave_fp16_range_are_the_training_paths(D):
    """First-layer weights scaled until SOME samples' activations leave fp16's range on the training path (the scale is chosen on that path
    alone): the frozen forward makes the same samples NaN, and everything downstream is equal NaN for NaN."""
    R, N = 8, 64
    inp = _inputs(R, N, True, seed=7 + D)
    for scale in (1e4, 2e4, 4e4, 8e4, 1.6e5, 3.2e5):
        w, b = _params(D, seed=77, scale={"layers0.0": scale})
        train = _render(D, R, N, False, False, inp, w, b, False)
        bad = torch.isnan(train["alpha"])
        if 0 < int(bad.sum()) < bad.numel():
            break
    else:
        pytest.fail("no scale of the first layer puts some, not all, samples outside fp16's range: the test's inputs need another look")
    frozen = _render(D, R, N, False, False, inp, w, b, True, guard=True)
    assert torch.equal(torch.isnan(frozen["alpha"]), bad)
    for k in OUT_KEYS:
        assert torch.equal(torch.isnan(train[k]), torch.isnan(frozen[k])), k
        assert torch.allclose(train[k], frozen[k], rtol=0.0, atol=0.0, equal_nan=True), k


@pytest.mark.parametrize("D", [128, 256])
def test_frozen_input_gradient_survives_amplifying_layers(D):
    """The weights of tests/test_gpu_split3.py::test_two_term_input_gradient_survives_amplifying_layers (hidden weights x 6: every layer
    amplifies the gradient by ~2.5): the per-sample scale and its re-centring are untouched by the missing stores."""
    R, N = 64, 64
    inp = _inputs(R, N, True, seed=4242 + D)
    w, b = _params(D, seed=4242 + D, scale={"layers": 6.0})
    train = _render(D, R, N, False, False, inp, w, b, False)
    frozen = _render(D, R, N, False, False, inp, w, b, True, guard=True)
    for k in OUT_KEYS:
        assert torch.isfinite(frozen[k]).all(), k
        assert torch.equal(train[k], frozen[k]), k
    assert float(frozen["d_pts_o"].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------ 4: the operator
class _Counting:
    """libnnr.so with every call counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


@pytest.fixture
def counted(monkeypatch):
    from nnr import lib as L
    proxy = _Counting(L.load())
    monkeypatch.setattr(L, "_lib", proxy)
    return proxy


def _operator(D, R, N, *, frozen, bf16=False, context=False, seed=5):
    import contextlib
    import nnr
    inp = _inputs(R, N, True, seed=seed)
    w, b = _params(D, seed=seed + 1)
    for t in w + b:
        t.requires_grad_(True)
    rays = [inp[k].clone().requires_grad_(True) for k in ("pts_o", "pts_d", "view_d")]
    with (nnr.frozen_field() if context else contextlib.nullcontext()):
        rgb, dist, alpha, z = nnr.render_rays(*rays, inp["z_lo"], inp["z_hi"], inp["jitter"], w, b, hidden=D, dist_alpha=False, white_bg=False,
                                              relu_sigma=False, bf16=bf16, frozen=frozen)
    ((rgb * inp["d_rgb"]).sum() + (dist * inp["d_dist"]).sum()).backward()
    torch.cuda.synchronize()
    return dict(rgb=rgb.detach(), dist=dist.detach(), alpha=alpha, z=z, grads=[r.grad for r in rays], wgrads=[t.grad for t in w + b])


@pytest.mark.parametrize("R,N", [(8, 32), (5, 130)], ids=["ray", "flat"])
@pytest.mark.parametrize("D", [128, 256])
def test_operator_frozen_true_and_the_context_manager(D, R, N, counted):
    plain = _operator(D, R, N, frozen=None)
    assert all(g is not None for g in plain["wgrads"]) and counted.calls.get("nnr_mlp_wgrad") == 1 and "nnr_frozen_fwd" not in counted.calls
    for how in (dict(frozen=True), dict(frozen=None, context=True)):
        counted.calls.clear()
        got = _operator(D, R, N, **how)
        assert counted.calls.get("nnr_frozen_fwd") == 1 and counted.calls.get("nnr_frozen_bwd") == 1, counted.calls
        for name in ("nnr_mlp_wgrad", "nnr_render_fwd", "nnr_render_bwd", "nnr_mlp_fwd", "nnr_mlp_dgrad", "nnr_workspace_floats", "nnr_plan_build"):
            assert name not in counted.calls, (name, counted.calls)
        assert all(g is None for g in got["wgrads"])
        for k in ("rgb", "dist", "alpha", "z"):
            assert torch.equal(got[k], plain[k]), k
        for g, want in zip(got["grads"], plain["grads"]):
            assert torch.equal(g, want)


def test_operator_frozen_with_bf16_runs_todays_kernels_without_a_weight_gradient(counted, caplog):
    import logging
    from nnr import ops
    ops._frozen_said.clear()
    with caplog.at_level(logging.INFO, logger="nnr"):
        got = _operator(256, 8, 64, frozen=True, bf16=True)
        _operator(256, 8, 64, frozen=True, bf16=True)
    assert "nnr_frozen_fwd" not in counted.calls and "nnr_mlp_wgrad" not in counted.calls
    assert counted.calls.get("nnr_render_fwd") == 2 and counted.calls.get("nnr_mlp_dgrad") == 2
    assert all(g is None for g in got["wgrads"]) and all(g is not None and torch.isfinite(g).all() for g in got["grads"])
    said = [r.getMessage() for r in caplog.records if "frozen" in r.getMessage()]
    assert len(said) == 1 and "bf16" in said[0]      # one line, however many calls


def test_operator_frozen_without_a_ray_gradient_is_a_plain_forward(counted):
    import nnr
    inp = _inputs(8, 32, False, seed=3)
    w, b = _params(128, seed=4)
    for t in w + b:
        t.requires_grad_(True)
    rgb, dist, _, _ = nnr.render_rays(inp["pts_o"], inp["pts_d"], inp["view_d"], inp["z_lo"], inp["z_hi"], None, w, b, hidden=128, dist_alpha=False,
                                      white_bg=False, relu_sigma=False, frozen=True)
    assert not rgb.requires_grad and not dist.requires_grad and "nnr_frozen_fwd" not in counted.calls and counted.calls.get("nnr_render_fwd") == 1


# ------------------------------------------------------------------------------------------------------------ 5: Trainer_pose, the golden
def _golden_step(monkeypatch, frozen_field):
    """tests/test_eval_focal.py::test_pose_optimisation_step_matches_the_reference on the GPU, eval_pose.frozen_field as given (None: absent)."""
    import model as mdl
    import test_eval_focal as tf
    from test_aux_terms import _trainer
    G = tf.GOLD
    dev = torch.device("cuda")
    inp = {k: torch.from_numpy(G["init." + k]) for k in ("pose_r", "pose_t", "scales", "shifts")}
    tr, _, _ = _trainer(inp, dev)
    pose = mdl.LearnPose(3, True, True, {"pose": {}}, init_c2w=torch.from_numpy(G["pose_opt.c2w0"]).to(dev)).to(dev)
    with torch.no_grad():
        pose.r.copy_(inp["pose_r"][:3]); pose.t.copy_(inp["pose_t"][:3])
    cfg = {"n_points": tf.R, "type": "nope_nerf"}
    if frozen_field is not None:
        cfg["frozen_field"] = frozen_field
    tp = mdl.Trainer_pose(tr.model, cfg, device=dev, optimizer_pose=torch.optim.SGD(pose.parameters(), lr=0.0), pose_param_net=pose)
    tf._replay_perm(monkeypatch, torch.from_numpy(G["pose_opt.ray_idx"]))
    frame = int(G["pose_opt.frame"])
    data = {"img": torch.from_numpy(G["imgs"][frame:frame + 1]), "img.idx": torch.tensor([int(G["pose_opt.view"])]),
            "img.camera_mat": torch.from_numpy(G["K"]), "img.scale_mat": torch.eye(4).unsqueeze(0)}
    for p in tr.model.parameters():
        p.grad = None
    ld = tp.train_step(data)
    torch.cuda.synchronize()
    return float(ld["loss"].detach()), pose.r.grad.clone(), pose.t.grad.clone(), [p.grad for p in tr.model.parameters()]


def test_trainer_pose_takes_the_frozen_path_by_default_and_meets_the_reference(monkeypatch, counted):
    import test_eval_focal as tf
    G = tf.GOLD
    loss, g_r, g_t, wg = _golden_step(monkeypatch, None)
    assert counted.calls.get("nnr_frozen_fwd") == 1 and counted.calls.get("nnr_frozen_bwd") == 1, counted.calls
    assert "nnr_mlp_wgrad" not in counted.calls and "nnr_render_fwd" not in counted.calls
    assert abs(loss - float(G["pose_opt.loss"])) <= 1e-6      # the bars of tests/test_eval_focal.py
    assert tf._close(g_r, G["pose_opt.g.r"], 1e-4 * float(np.abs(G["pose_opt.g.r"]).max()))
    assert tf._close(g_t, G["pose_opt.g.t"], 1e-4 * float(np.abs(G["pose_opt.g.t"]).max()))
    assert all(g is None for g in wg)
    counted.calls.clear()
    loss0, g_r0, g_t0, wg0 = _golden_step(monkeypatch, False)
    assert "nnr_frozen_fwd" not in counted.calls and counted.calls.get("nnr_mlp_wgrad") == 1 and counted.calls.get("nnr_render_fwd") == 1
    assert loss0 == loss and torch.equal(g_r0, g_r) and torch.equal(g_t0, g_t)
    assert all(g is not None and torch.isfinite(g).all() for g in wg0) and any(float(g.abs().max()) > 0 for g in wg0)


# ------------------------------------------------------------------------------------------------------------ 6: a refinement run
def _refine(scene_dir, n_samples, frozen_field, steps=20):
    import dataloading as dl
    import model as mdl
    import train_scene
    torch.manual_seed(11)
    np.random.seed(11)
    dev = torch.device("cuda")
    cfg = train_scene.scene_cfg(scene_dir, "toy", n_rays=96, n_samples=n_samples, hidden=128, sample_rate=10 ** 6)
    loader, fields = dl.get_dataloader(cfg, mode="train", shuffle=False)
    trainer, _, _ = train_scene.build(cfg, dev, fields["img"].N_imgs)
    pose = mdl.LearnPose(fields["img"].N_imgs, True, True, cfg, init_c2w=None).to(dev)
    opt = torch.optim.Adam(pose.parameters(), lr=1e-3)
    tp = mdl.Trainer_pose(trainer.model, {"n_points": 96, "type": "nope_nerf", "frozen_field": frozen_field}, device=dev, optimizer_pose=opt,
                          pose_param_net=pose)
    done, losses = 0, []
    while done < steps:
        for batch in loader:
            losses.append(tp.train_step(batch)["loss"].detach())
            done += 1
            if done == steps:
                break
    torch.cuda.synchronize()
    return pose.r.detach().clone(), pose.t.detach().clone(), torch.stack(losses)


@pytest.mark.parametrize("n_samples", [32, 24], ids=["ray_mode_32", "flat_mode_24"])
def test_twenty_refinement_steps_end_at_the_same_poses(tmp_path, n_samples, counted):
    import scene_writer
    scene_writer.write_scene(str(tmp_path), scene="toy", frames=4, size=(30, 40), seed=0)
    r1, t1, l1 = _refine(str(tmp_path), n_samples, True)
    assert counted.calls.get("nnr_frozen_fwd") == 20 and counted.calls.get("nnr_frozen_bwd") == 20 and "nnr_mlp_wgrad" not in counted.calls
    counted.calls.clear()
    r0, t0, l0 = _refine(str(tmp_path), n_samples, False)
    assert counted.calls.get("nnr_mlp_wgrad") == 20 and "nnr_frozen_fwd" not in counted.calls
    assert torch.isfinite(r1).all() and torch.isfinite(t1).all() and float(r1.abs().max()) > 0.0      # the poses moved
    assert torch.equal(l1, l0) and torch.equal(r1, r0) and torch.equal(t1, t0)
