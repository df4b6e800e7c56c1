"""Timings of the sparse frozen-field render (nnr.render_rays(frozen=True, occupancy=grid)) beside the dense frozen
render it thins out (section 14).

    python tools/time_frozen_sparse.py --out DIR    # device-event timings, then a rocprofv3 --kernel-trace --stats pass of its own
    python tools/time_frozen_sparse.py --inner      # the workload the trace pass runs (also usable on its own)

tools/time_frozen.py's protocol: per shape, in one process (and one trace), rounds that alternate the ways, median and range of each.
Shapes: 1024 rays x 192 and x 128 samples, D = 256 and 128.  Ways, for `render` (one nnr.render_rays forward and backward on synthetic rays,
upstream gradients given): `dense` (the frozen render) and the sparse frozen render on five grids of 64^3 cells over the cube the rays stay
in -- `set` (every bit: the path's overhead), `live50` / `live25` / `live10` (random cells, that share of them set) and `slab` (the cells
of a slab |z| < 0.5).  The share of samples each grid leaves live is reported with it.  For `step`: the whole model.Trainer_pose.train_step
on a synthetic scene of tools/scene_writer.py without and with eval_pose.occupancy (an untrained field: alpha_min 0.5 makes its grid cull).
The compaction's three launches are reported separately by the trace pass (the events cannot tell them from the forward): per kernel and
grid size, count / min / median / max duration in DIR/frozen_sparse_kernel_trace_summary.json, rocprofv3's own table in
DIR/frozen_sparse_kernel_stats.csv.  Event timings: JSON lines and DIR/time_frozen_sparse.json.  Nothing is gated.  GPU only."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
sys.path.insert(0, HERE)

from time_grid import ROUNDS, _events, _net, summarise_trace      # noqa: E402  (the same networks, event windows and trace summary)

SHAPES = ((1024, 192, 256), (1024, 192, 128), (1024, 128, 256), (1024, 128, 128))      # (rays, samples, hidden)
GRIDS = ("set", "live50", "live25", "live10", "slab")
REPS = 10
CELLS, HALF = 64, 4.0      # the grid: CELLS^3 cells over [-HALF, HALF]^3 (|o| <= 0.5 sqrt 3 / 2 and z <= 3.4: every sample inside)


class Grid:
    def __init__(self, occ):
        self.lo, self.inv_step, self.dims = (-HALF,) * 3, (CELLS / (2 * HALF),) * 3, (CELLS,) * 3
        o = occ.numpy().astype(bool)      # (n_z, n_y, n_x) -> (n_z, n_y, n_x / 32) words, bit i_x & 31 (include/nnr_sparse.h)
        w = (o.reshape(CELLS, CELLS, CELLS // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
        self.bits = torch.from_numpy(w.view(np.int32).copy()).cuda()


def _grid(kind):
    g = torch.Generator().manual_seed(7)
    if kind == "set":
        return Grid(torch.ones(CELLS, CELLS, CELLS, dtype=torch.bool))
    if kind == "slab":
        zc = (torch.arange(CELLS) + 0.5) * (2 * HALF / CELLS) - HALF
        return Grid((zc.abs() < 0.5)[:, None, None].expand(CELLS, CELLS, CELLS).contiguous())
    return Grid(torch.rand(CELLS, CELLS, CELLS, generator=g) < int(kind[4:]) / 100.)


def _rounds(report, jobs, what, base, extra, **shape):
    for _, fn in jobs:      # warm up every way: packs, workspaces
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in jobs}
    for _ in range(ROUNDS):
        for name, fn in jobs:
            ms[name].append(_events(fn, REPS))
    ref = statistics.median(ms[base])
    for name, _ in jobs:
        t = ms[name]
        report("%s_%s" % (what, name), reps_per_round=REPS, rounds=ROUNDS, ms_min=min(t), ms_median=statistics.median(t), ms_max=max(t),
               spread=max(t) / min(t), over_dense=statistics.median(t) / ref, **extra.get(name, {}), **shape)


def _render_jobs(R, N, hidden):
    import nnr
    from nnr import ops
    net = _net(hidden)
    g = torch.Generator().manual_seed(R + N)
    o = ((torch.rand(R, 3, generator=g) - 0.5)).cuda().requires_grad_(True)
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).cuda().requires_grad_(True)
    v = (-d.detach()).requires_grad_(True)
    z = torch.linspace(0.05, 3.4, N).cuda()
    d_rgb, d_dist = torch.randn(R, 3, generator=g).cuda(), torch.randn(R, generator=g).cuda()
    kw = dict(hidden=hidden, dist_alpha=False, white_bg=False, relu_sigma=False)
    w, b = net.weights(), net.biases()
    grids = {k: _grid(k) for k in GRIDS}
    extra = {}
    for k, grid in grids.items():      # the share of samples the grid leaves live, counted once by the plain-tensor op
        res = ops.render_frozen_sparse(o, d, v, z, z, None, grid, w, b, debug=True, **kw)
        extra["sparse_" + k] = dict(live_share=float(res["n_live"]) / (R * N))

    def run(grid):
        rgb, dist, _, _ = nnr.render_rays(o, d, v, z, z, None, w, b, frozen=True, occupancy=grid, **kw)
        torch.autograd.backward([rgb, dist], [d_rgb, d_dist])
    return [("dense", lambda: run(None))] + [("sparse_" + k, lambda grid=grid: run(grid)) for k, grid in grids.items()], extra


def _step_jobs(scene_dir, R, N, hidden):
    import dataloading as dl
    import model as mdl
    import train_scene
    cfg = train_scene.scene_cfg(scene_dir, "toy", n_rays=R, n_samples=N, hidden=hidden, sample_rate=10 ** 6)
    cfg["rendering"]["occupancy"] = {"resolution": 64, "alpha_min": 0.5}      # (an untrained field: its alpha sits near 0.5)
    loader, fields = dl.get_dataloader(cfg, mode="train", shuffle=False)
    batch = next(iter(loader))
    torch.manual_seed(hidden)
    trainer, _, _ = train_scene.build(cfg, torch.device("cuda"), fields["img"].N_imgs)
    jobs, extra = [], {}
    for way in ("dense", "occupancy"):
        pose = mdl.LearnPose(fields["img"].N_imgs, True, True, cfg, init_c2w=None).cuda()
        tp = mdl.Trainer_pose(trainer.model, {"n_points": R, "type": "nope_nerf", "occupancy": way == "occupancy"}, device=torch.device("cuda"),
                              optimizer_pose=torch.optim.Adam(pose.parameters(), lr=1e-3), pose_param_net=pose)
        jobs.append((way, lambda tp=tp: tp.train_step(batch)))
        if way == "occupancy":
            tp.train_step(batch)      # builds the grid
            extra[way] = dict(cells_occupied=float(tp.occupancy_grid.occupied), grid_builds=tp.occupancy_builds)
    return jobs, extra


def workload(report):
    import scene_writer
    from nnr import lib as L
    L.set_fp32_products("split2")
    with tempfile.TemporaryDirectory() as tmp:
        scene_writer.write_scene(tmp, scene="toy", frames=2, size=(60, 80), seed=0)      # 4800 pixels: n_points 1024 of them per step
        for R, N, hidden in SHAPES:
            shape = dict(rays=R, samples_per_ray=N, hidden=hidden)
            jobs, extra = _render_jobs(R, N, hidden)
            _rounds(report, jobs, "render", "dense", extra, **shape)
            jobs, extra = _step_jobs(tmp, R, N, hidden)
            _rounds(report, jobs, "step", "dense", extra, **shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--out", help="directory for time_frozen_sparse.json and the trace's summaries (required unless --inner)")
    args = ap.parse_args()
    if not args.inner and not args.out:
        ap.error("--out DIR is required")
    if not torch.cuda.is_available():
        sys.exit("time_frozen_sparse: needs a GPU; a CPU run measures nothing about the kernels")
    lines = []

    def report(name, **kv):
        line = dict(name=name, **{k: round(v, 5) if isinstance(v, float) else v for k, v in kv.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    workload(report)
    if args.inner:
        return
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_frozen_sparse.json"), "w") as f:
        json.dump(lines, f, indent=1)
    # the trace pass: a fresh child process under rocprofv3 (never this process, which has the GPU open)
    trace = os.path.join(args.out, "frozen_sparse_trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "frozen_sparse", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if r.returncode:
        sys.exit("time_frozen_sparse: the rocprofv3 pass failed with status %d\n%s" % (r.returncode, r.stderr[-2000:]))
    summarise_trace(args.out, prefix="frozen_sparse_")


if __name__ == "__main__":
    main()
