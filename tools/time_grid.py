"""Timings of the density-grid kernel (nnr_grid_f16.hip through nnr.ops.density_grid).

    python tools/time_grid.py --out DIR             # device-event timings, then a rocprofv3 --kernel-trace --stats pass of its own
    python tools/time_grid.py --inner               # the workload the trace pass runs (also usable on its own)

For D = 256 and D = 128, in one process (and one trace): grid_f16_kernel at 128^3 and 256^3, march_f16_kernel's ray mode at 1024 rays x 512
steps (the same MACs per point: trunk and density head), and nnr.ops.mlp_points(split2=True) on the 128^3 grid's points (the path a user had
before the kernel: the whole forward, 24 bytes read and 16 written per point).  The sizes are timed in ROUNDS rounds that alternate the
kernels, so that the run-to-run spread of each figure (min / median / max over the rounds) stands beside it: the allowance of the grid's
ns per voxel over the march's ns per sample is that spread.  Every round's window of every kernel is about a quarter of a second of device
work.  Random-init networks (the time does not depend on the weights).
Reports JSON lines and DIR/time_grid.json; the trace pass gives the per-kernel figures (the events include launch gaps): DIR/kernel_stats.csv
is rocprofv3's own table, DIR/kernel_trace_summary.json the count / min / median / max duration per kernel and grid size from its kernel
trace (the trace itself is removed: tens of megabytes).  Exits non-zero if the trace pass fails.  GPU only."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))

ROUNDS = 7


def _net(hidden):
    import model as mdl
    cfg = {'model': {'hidden_dim': hidden, 'pos_enc_levels': 10, 'dir_enc_levels': 4, 'occ_activation': 'softplus'},
           'rendering': {'white_background': False, 'dist_alpha': False}}
    torch.manual_seed(hidden)
    return mdl.OfficialStaticNerf(cfg).cuda()


def _events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps      # ms


def workload(report):
    import nnr.ops as ops
    for hidden in (256, 128):
        net = _net(hidden)
        w, b = net.weights(), net.biases()
        kw = dict(hidden=hidden)
        grid = {n: (lambda n=n: ops.density_grid((-1., -1., -1.), (2. / (n - 1),) * 3, (n, n, n), w, b, **kw)) for n in (128, 256)}
        R, N = 1024, 512
        g = torch.Generator().manual_seed(1)
        o = (torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 2.5).cuda()
        d = torch.nn.functional.normalize(-o + 0.3 * torch.randn(R, 3, generator=g).cuda(), dim=-1)
        t = torch.linspace(0, 1, N).cuda()
        march = lambda: ops.ray_march(o, d, t, w, b, radius=4.0, n_secant=0, **kw)
        ax = -1. + (2. / 127) * torch.arange(128, dtype=torch.float32)
        zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
        pts = torch.stack([xx, yy, zz], -1).reshape(-1, 3).cuda()
        zeros = torch.zeros_like(pts)
        points = lambda: ops.mlp_points(pts, zeros, w, b, split2=True, **kw)
        # (name, call, calls per window, points per call): windows of about 0.25 s at 2 to 4 ns per point
        jobs = [("grid_128", grid[128], 50, 128 ** 3), ("grid_256", grid[256], 6, 256 ** 3), ("march_1024x512", march, 200, R * N),
                ("mlp_points_128", points, 30, 128 ** 3)]
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
        report("ratios_d%d" % hidden,
               grid_256_over_march=statistics.median(ns["grid_256"]) / statistics.median(ns["march_1024x512"]),
               march_spread=max(ns["march_1024x512"]) / min(ns["march_1024x512"]),
               grid_256_spread=max(ns["grid_256"]) / min(ns["grid_256"]),
               mlp_points_over_grid_128=statistics.median(ns["mlp_points_128"]) / statistics.median(ns["grid_128"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--out", help="directory for time_grid.json and the trace (required unless --inner)")
    args = ap.parse_args()
    if not args.inner and not args.out:
        ap.error("--out DIR is required")
    if not torch.cuda.is_available():
        sys.exit("time_grid: needs a GPU; a CPU run measures nothing about the kernel")
    lines = []

    def report(name, **kv):
        line = dict(name=name, **{k: round(v, 5) if isinstance(v, float) else v for k, v in kv.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    workload(report)
    if args.inner:
        return
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_grid.json"), "w") as f:
        json.dump(lines, f, indent=1)
    # the trace pass: a fresh child process under rocprofv3 (never this process, which has the GPU open)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(args.out, "trace"), "-o", "grid", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if r.returncode:
        sys.exit("time_grid: the rocprofv3 pass failed with status %d\n%s" % (r.returncode, r.stderr[-2000:]))
    summarise_trace(args.out)


def summarise_trace(out, prefix=""):
    """rocprofv3's files under OUT/<prefix>trace -> OUT/<prefix>kernel_stats.csv (copied) and OUT/<prefix>kernel_trace_summary.json;
    OUT/<prefix>trace is removed (prefix: tools/time_bricks.py keeps its files beside this tool's)"""
    trace = os.path.join(out, prefix + "trace")
    stats = glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True)
    traces = glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True)
    if len(stats) != 1 or len(traces) != 1:
        sys.exit("expected one kernel_stats.csv and one kernel_trace.csv under %s, found %r and %r" % (trace, stats, traces))
    shutil.copyfile(stats[0], os.path.join(out, prefix + "kernel_stats.csv"))
    ns = {}
    with open(traces[0], newline="") as f:
        for row in csv.DictReader(f):
            threads = (int(row["Grid_Size_X"]) * int(row["Grid_Size_Y"]) * int(row["Grid_Size_Z"]) if "Grid_Size_X" in row
                       else int(row["Grid_Size"]))
            ns.setdefault((row["Kernel_Name"], threads), []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    summary = [dict(kernel=k, grid_threads=g, calls=len(v), ns_min=min(v), ns_median=statistics.median(v), ns_max=max(v), ns_total=sum(v))
               for (k, g), v in sorted(ns.items(), key=lambda kv: -sum(kv[1]))]
    with open(os.path.join(out, prefix + "kernel_trace_summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    shutil.rmtree(trace)
    for line in summary[:12]:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
