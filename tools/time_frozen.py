"""Timings of the frozen-field render (nnr.render_rays(frozen=True) / nnr.frozen_field()) beside the training path it
replaces in test-time pose refinement.

    python tools/time_frozen.py --out DIR           # device-event timings, then a rocprofv3 --kernel-trace --stats pass of its own
    python tools/time_frozen.py --inner             # the workload the trace pass runs (also usable on its own)

Shapes: 1024 rays x 192 samples at D = 256, and 1024 x 128 (the eval_pose defaults: n_points 1024) at D = 128 and 256.  Per shape, in one
process (and one trace), three ways:
    full      the operator's full training path: weights with requires_grad, stashes, weight gradient -- what Trainer_pose ran before the
              frozen mode existed (eval_pose.frozen_field: false)
    detached  today's kernels with the weights detached: stashes written, no weight-gradient launch
    frozen    the frozen kernels on the frozen workspace
for (a) `render`: one nnr.render_rays forward and backward on synthetic rays, upstream gradients given, and (b) `step`: the whole
model.Trainer_pose.train_step (pose table -> rays -> render -> MSE -> backward -> Adam on the poses) on a synthetic scene of
tools/scene_writer.py.  Timed in ROUNDS rounds that alternate the three ways (tools/time_grid.py), so that the run-to-run spread of each
figure stands beside it.  Random-init networks (the kernels' times do not depend on the weights).  Also reports the two workspaces' bytes.
Reports JSON lines and DIR/time_frozen.json; the trace pass gives the per-kernel figures (the events include launch gaps):
DIR/frozen_kernel_stats.csv is rocprofv3's own table, DIR/frozen_kernel_trace_summary.json the count / min / median / max duration per kernel
and grid size.  Nothing is gated.  GPU only."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
sys.path.insert(0, HERE)

from time_grid import ROUNDS, _events, _net, summarise_trace      # noqa: E402  (the same networks, event windows and trace summary)

SHAPES = ((1024, 192, 256), (1024, 128, 128), (1024, 128, 256))      # (rays, samples, hidden)
WAYS = ("full", "detached", "frozen")
REPS = 10


def _rounds(report, jobs, what, **shape):
    for _, fn in jobs:      # warm up every way: packs, workspaces, plans
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in jobs}
    for _ in range(ROUNDS):
        for name, fn in jobs:
            ms[name].append(_events(fn, REPS))
    full = statistics.median(ms["full"])
    for name, _ in jobs:
        t = ms[name]
        report("%s_%s" % (what, name), reps_per_round=REPS, rounds=ROUNDS, ms_min=min(t), ms_median=statistics.median(t), ms_max=max(t),
               spread=max(t) / min(t), over_full=statistics.median(t) / full, **shape)


def _render_jobs(R, N, hidden):
    import nnr
    net = _net(hidden)
    g = torch.Generator().manual_seed(R + N)
    o = ((torch.rand(R, 3, generator=g) - 0.5)).cuda().requires_grad_(True)
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).cuda().requires_grad_(True)
    v = (-d.detach()).requires_grad_(True)
    z = torch.linspace(0.05, 3.4, N).cuda()
    d_rgb, d_dist = torch.randn(R, 3, generator=g).cuda(), torch.randn(R, generator=g).cuda()
    kw = dict(hidden=hidden, dist_alpha=False, white_bg=False, relu_sigma=False)

    def run(way):
        w, b = net.weights(), net.biases()
        if way == "detached":
            w, b = [t.detach() for t in w], [t.detach() for t in b]
        rgb, dist, _, _ = nnr.render_rays(o, d, v, z, z, None, w, b, frozen=(way == "frozen"), **kw)
        torch.autograd.backward([rgb, dist], [d_rgb, d_dist])
    return [(way, lambda way=way: run(way)) for way in WAYS]


def _step_jobs(scene_dir, R, N, hidden):
    import dataloading as dl
    import model as mdl
    import train_scene
    cfg = train_scene.scene_cfg(scene_dir, "toy", n_rays=R, n_samples=N, hidden=hidden, sample_rate=10 ** 6)
    loader, fields = dl.get_dataloader(cfg, mode="train", shuffle=False)
    batch = next(iter(loader))
    torch.manual_seed(hidden)
    trainer, _, _ = train_scene.build(cfg, torch.device("cuda"), fields["img"].N_imgs)
    jobs = []
    for way in WAYS:
        pose = mdl.LearnPose(fields["img"].N_imgs, True, True, cfg, init_c2w=None).cuda()
        tp = mdl.Trainer_pose(trainer.model, {"n_points": R, "type": "nope_nerf", "frozen_field": way == "frozen"}, device=torch.device("cuda"),
                              optimizer_pose=torch.optim.Adam(pose.parameters(), lr=1e-3), pose_param_net=pose)

        def run(tp=tp, way=way):
            for p in trainer.model.parameters():      # `detached`: the field's parameters ask for no gradient, nothing else changes
                p.requires_grad_(way != "detached")
            tp.train_step(batch)
        jobs.append((way, run))
    return jobs


def workload(report):
    import scene_writer
    from nnr import lib as L
    L.set_fp32_products("split2")
    lib = L.load()
    with tempfile.TemporaryDirectory() as tmp:
        scene_writer.write_scene(tmp, scene="toy", frames=2, size=(60, 80), seed=0)      # 4800 pixels: n_points 1024 of them per step
        for R, N, hidden in SHAPES:
            shape = dict(rays=R, samples_per_ray=N, hidden=hidden)
            cfg = L.make_cfg(R, N, hidden, train=True)
            full, frozen = 4 * lib.nnr_workspace_floats(C.byref(cfg)), 4 * lib.nnr_frozen_workspace_floats(C.byref(cfg))
            report("workspace", training_bytes=full, frozen_bytes=frozen, ratio=full / frozen, **shape)
            _rounds(report, _render_jobs(R, N, hidden), "render", **shape)
            _rounds(report, _step_jobs(tmp, R, N, hidden), "step", **shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--out", help="directory for time_frozen.json and the trace's summaries (required unless --inner)")
    args = ap.parse_args()
    if not args.inner and not args.out:
        ap.error("--out DIR is required")
    if not torch.cuda.is_available():
        sys.exit("time_frozen: needs a GPU; a CPU run measures nothing about the kernels")
    lines = []

    def report(name, **kv):
        line = dict(name=name, **{k: round(v, 5) if isinstance(v, float) else v for k, v in kv.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    workload(report)
    if args.inner:
        return
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_frozen.json"), "w") as f:
        json.dump(lines, f, indent=1)
    # the trace pass: a fresh child process under rocprofv3 (never this process, which has the GPU open)
    trace = os.path.join(args.out, "frozen_trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "frozen", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if r.returncode:
        sys.exit("time_frozen: the rocprofv3 pass failed with status %d\n%s" % (r.returncode, r.stderr[-2000:]))
    summarise_trace(args.out, prefix="frozen_")


if __name__ == "__main__":
    main()
