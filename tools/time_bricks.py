"""Timings of the density-bricks kernel (nnr_bricks_f16.hip through nnr.ops.density_bricks).

    python tools/time_bricks.py --out DIR           # device-event timings, then a rocprofv3 --kernel-trace --stats pass of its own
    python tools/time_bricks.py --inner             # the workload the trace pass runs (also usable on its own)

For D = 256 and D = 128, in one process (and one trace), at the same voxel counts: bricks_f16_kernel on all 4096 bricks of a 128^3 grid and
all 32768 of a 256^3 grid (sorted as geometry.bricks_for sorts them), grid_f16_kernel on those two grids, and nnr.ops.mlp_points(split2=True)
on the points of the 4096 bricks, built on the host -- the brick path a user had without the kernel (the whole forward, 24 bytes read and 16
written per point).  The sizes are timed in ROUNDS rounds that alternate the kernels (tools/time_grid.py), so that the run-to-run spread of
each figure stands beside it: the margin of the brick kernel's ns per voxel over the grid kernel's is the grid kernel's own spread.
Random-init networks (the time does not depend on the weights).
Reports JSON lines and DIR/time_bricks.json; the trace pass gives the per-kernel figures (the events include launch gaps):
DIR/bricks_kernel_stats.csv is rocprofv3's own table, DIR/bricks_kernel_trace_summary.json the count / min / median / max duration per kernel
and grid size from its kernel trace (the trace itself is removed).  Exits non-zero if the trace pass fails.  GPU only."""
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

from time_grid import ROUNDS, _events, _net, summarise_trace      # noqa: E402  (the same networks, event windows and trace summary)


def _bricks_of(n):
    """all (n / 8)^3 bricks of an n^3 grid, (bz, by, bx) ascending -> (B,3) int32 (bx, by, bz)"""
    k = torch.arange(n // 8)
    bz, by, bx = torch.meshgrid(k, k, k, indexing="ij")
    return torch.stack([bx, by, bz], -1).reshape(-1, 3).to(torch.int32).cuda()


def workload(report):
    import nnr.ops as ops
    for hidden in (256, 128):
        net = _net(hidden)
        w, b = net.weights(), net.biases()
        kw = dict(hidden=hidden)
        grid_of = lambda n: ((-1., -1., -1.), (2. / (n - 1),) * 3)
        grid = {n: (lambda n=n: ops.density_grid(*grid_of(n), (n, n, n), w, b, **kw)) for n in (128, 256)}
        lists = {n: _bricks_of(n) for n in (128, 256)}
        bricks = {n: (lambda n=n: ops.density_bricks(*grid_of(n), lists[n], w, b, **kw)) for n in (128, 256)}
        # the 128^3 bricks' points in the bricks' order, as a host-side brick path would build them
        l = torch.arange(8, dtype=torch.float32)
        idx = 8. * lists[128].cpu().float()[:, :, None] + l[None, None]                       # (B,3,8)
        ax = -1. + (2. / 127) * idx
        B = idx.shape[0]
        pts = torch.stack([ax[:, 0, None, None, :].expand(B, 8, 8, 8), ax[:, 1, None, :, None].expand(B, 8, 8, 8),
                           ax[:, 2, :, None, None].expand(B, 8, 8, 8)], -1).reshape(-1, 3).cuda()
        zeros = torch.zeros_like(pts)
        points = lambda: ops.mlp_points(pts, zeros, w, b, split2=True, **kw)
        # (name, call, calls per window, points per call): windows of about 0.25 s at 2 to 4 ns per point
        jobs = [("bricks_4096", bricks[128], 50, 128 ** 3), ("grid_128", grid[128], 50, 128 ** 3), ("bricks_32768", bricks[256], 6, 256 ** 3),
                ("grid_256", grid[256], 6, 256 ** 3), ("mlp_points_4096_bricks", points, 30, 128 ** 3)]
        for _, fn, _, _ in jobs:      # warm up every shape of the timed window
            fn()
            fn()
        torch.cuda.synchronize()
        ns = {name: [] for name, _, _, _ in jobs}
        for _ in range(ROUNDS):       # alternating: every round times every kernel once
            for name, fn, reps, count in jobs:
                ns[name].append(_events(fn, reps) * 1e6 / count)
        for name, _, reps, count in jobs:
            v = ns[name]
            report("%s_d%d" % (name, hidden), points=count, reps_per_round=reps, rounds=ROUNDS, ns_per_point_min=min(v),
                   ns_per_point_median=statistics.median(v), ns_per_point_max=max(v), ms_median=statistics.median(v) * count / 1e6)
        med = {k: statistics.median(v) for k, v in ns.items()}
        report("ratios_d%d" % hidden, bricks_over_grid_128=med["bricks_4096"] / med["grid_128"],
               bricks_over_grid_256=med["bricks_32768"] / med["grid_256"], grid_128_spread=max(ns["grid_128"]) / min(ns["grid_128"]),
               grid_256_spread=max(ns["grid_256"]) / min(ns["grid_256"]), mlp_points_over_bricks=med["mlp_points_4096_bricks"] / med["bricks_4096"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--out", help="directory for time_bricks.json and the trace's summaries (required unless --inner)")
    args = ap.parse_args()
    if not args.inner and not args.out:
        ap.error("--out DIR is required")
    if not torch.cuda.is_available():
        sys.exit("time_bricks: needs a GPU; a CPU run measures nothing about the kernel")
    lines = []

    def report(name, **kv):
        line = dict(name=name, **{k: round(v, 5) if isinstance(v, float) else v for k, v in kv.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    workload(report)
    if args.inner:
        return
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_bricks.json"), "w") as f:
        json.dump(lines, f, indent=1)
    # the trace pass: a fresh child process under rocprofv3 (never this process, which has the GPU open)
    trace = os.path.join(args.out, "bricks_trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "bricks", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if r.returncode:
        sys.exit("time_bricks: the rocprofv3 pass failed with status %d\n%s" % (r.returncode, r.stderr[-2000:]))
    summarise_trace(args.out, prefix="bricks_")


if __name__ == "__main__":
    main()
