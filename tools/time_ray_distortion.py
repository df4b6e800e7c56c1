"""Timings of the ray-distortion regulariser (nnr_ray_distortion.hip): its two kernels alone, and the render operator's
forward + backward with and without the term.

    python tools/time_ray_distortion.py --out DIR       # device-event timings, then a rocprofv3 --kernel-trace --stats pass of its own
    python tools/time_ray_distortion.py --inner         # the workload the trace pass runs (also usable on its own)

The kernels alone, at 1024 rays x 192 samples and 4096 x 128: ray_distortion_fwd_kernel and ray_distortion_bwd_kernel (accumulate = 1) on column
3 of an (R N, 4) tensor -- the stride at which they read sigma_raw from, and add into, a training workspace -- with random densities and
jittered depths.  The operator, at 1024 x 192, D = 256 (the shape of BASELINE configs[1]) and at 4096 x 128, D = 128: nnr.render_rays forward
and the backward of sum(rgb) + sum(dist), without the term and with sum(dloss) added.  Timed in ROUNDS rounds that alternate the jobs
(tools/time_grid.py), so that the run-to-run spread of each figure stands beside it; random-init networks.  Reports JSON lines and
DIR/time_ray_distortion.json; the trace pass gives the per-kernel figures (the events include launch gaps):
DIR/ray_distortion_kernel_stats.csv is rocprofv3's own table, DIR/ray_distortion_kernel_trace_summary.json the count / min / median / max
duration per kernel and grid size.  Recorded, not gated.  GPU only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
sys.path.insert(0, HERE)

from time_grid import ROUNDS, _events, _net      # noqa: E402  (the same networks and event windows)
from time_grid import summarise_trace            # noqa: E402

KERNEL_SHAPES = ((1024, 192), (4096, 128))
OPERATOR_SHAPES = ((1024, 192, 256), (4096, 128, 128))
NEAR, FAR = 0.01, 10.0


def _depths(R, N, g):
    edges = torch.linspace(NEAR, FAR, N + 1)
    return (edges[:-1] + (edges[1:] - edges[:-1]) * torch.rand(R, N, generator=g)).contiguous().cuda()


def _rounds(report, jobs, base=None, **extra):
    for _, fn, _ in jobs:
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in jobs}
    for _ in range(ROUNDS):       # alternating: every round times every job once
        for name, fn, reps in jobs:
            ms[name].append(_events(fn, reps))
    for name, _, reps in jobs:
        t = ms[name]
        more = dict(over_base=statistics.median(t) / statistics.median(ms[base])) if base else {}
        report(name, reps_per_round=reps, rounds=ROUNDS, ms_min=min(t), ms_median=statistics.median(t), ms_max=max(t), spread=max(t) / min(t),
               **more, **extra)


def workload(report):
    import nnr
    import nnr.ops as ops
    s_near, s_inv = NEAR, 1.0 / (FAR - NEAR)
    for R, N in KERNEL_SHAPES:
        g = torch.Generator().manual_seed(R)
        out4 = torch.zeros(R * N, 4).cuda()
        out4[:, 3] = (3.0 * torch.randn(R * N, generator=g) - 2.0).cuda()
        raw = out4[:, 3].view(R, N)
        z = _depths(R, N, g)
        up = torch.ones(R).cuda()
        dout4 = torch.zeros(R * N, 4).cuda()
        d_raw = dout4[:, 3].view(R, N)
        jobs = [("kernel_fwd_%dx%d" % (R, N), lambda raw=raw, z=z: ops.ray_distortion(raw, z, s_near, s_inv, False, False), 200),
                ("kernel_bwd_%dx%d" % (R, N),
                 lambda raw=raw, z=z, up=up, d_raw=d_raw: ops.ray_distortion_grad(raw, z, s_near, s_inv, False, False, up, out=d_raw, accumulate=True), 200)]
        _rounds(report, jobs, rays=R, samples_per_ray=N)
    for R, N, hidden in OPERATOR_SHAPES:
        net = _net(hidden)
        w, b = net.weights(), net.biases()
        g = torch.Generator().manual_seed(R + 1)
        o = ((torch.rand(R, 3, generator=g) - 0.5) * 0.2).cuda()
        d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).cuda()
        jit = torch.rand(R, N, generator=g).cuda()
        zt = torch.linspace(NEAR, FAR, N)
        mid = 0.5 * (zt[1:] + zt[:-1])
        lo, hi = torch.cat([zt[:1], mid]).cuda(), torch.cat([mid, zt[-1:]]).cuda()
        kw = dict(hidden=hidden, dist_alpha=False, white_bg=False, relu_sigma=False)

        def step(rd):
            for p in list(w) + list(b):
                p.grad = None
            out = nnr.render_rays(o, d, -d, lo, hi, jit, w, b, ray_distortion=rd, **kw)
            loss = out[0].sum() + out[1].sum()
            if rd is not None:
                loss = loss + 0.01 * out[4].sum()
            loss.backward()
        tag = "%dx%d_d%d" % (R, N, hidden)
        jobs = [("operator_off_" + tag, lambda: step(None), 10), ("operator_on_" + tag, lambda: step((s_near, s_inv)), 10)]
        _rounds(report, jobs, base="operator_off_" + tag, rays=R, samples_per_ray=N, hidden=hidden)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--out", help="directory for time_ray_distortion.json and the trace's summaries (required unless --inner)")
    args = ap.parse_args()
    if not args.inner and not args.out:
        ap.error("--out DIR is required")
    if not torch.cuda.is_available():
        sys.exit("time_ray_distortion: needs a GPU; a CPU run measures nothing about the kernels")
    lines = []

    def report(name, **kv):
        line = dict(name=name, **{k: round(v, 5) if isinstance(v, float) else v for k, v in kv.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    workload(report)
    if args.inner:
        return
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_ray_distortion.json"), "w") as f:
        json.dump(lines, f, indent=1)
    # the trace pass: a fresh child process under rocprofv3 (never this process, which has the GPU open)
    trace = os.path.join(args.out, "ray_distortion_trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "ray_distortion", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if r.returncode:
        sys.exit("time_ray_distortion: the rocprofv3 pass failed with status %d\n%s" % (r.returncode, r.stderr[-2000:]))
    summarise_trace(args.out, prefix="ray_distortion_")


if __name__ == "__main__":
    main()
