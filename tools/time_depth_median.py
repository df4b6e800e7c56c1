"""Timings of the two quantile-depth kernels (nnr_depth_f16.hip under NNR_DEPTH_MEDIAN=1, nnr_propose_f16.hip under NNR_PROPOSE_SPARSE=1
NNR_PROPOSE_DEPTH=2, through nnr.ops.render_depth[_sparse](quantile_level=...)), each beside its parent kernel.

    python tools/time_depth_median.py --out DIR      # device-event timings, then a rocprofv3 --kernel-trace --stats pass of its own

In one process, for D = 256 and D = 128, on the rays, samples, network and grids of tools/time_depth_sparse.py (256 x 256 rays of one pinhole
camera in image order, C = 128 and C = 256, an untrained softplus network whose samples have an alpha of about one half, grids of 64^3 cells
over [-4, 4]^3), with level = 0.5:
  (a) depth_median_f16_kernel against depth_f16_kernel on the same rays;
  (b) depth_sparse_median_f16_kernel against depth_sparse_f16_kernel at equal t_min: at t_min = 0 under every bit set and the slabs that
      leave about 50, 25 and 10 % of the samples live, and at t_min = 1e-3 under every bit set;
  (c) depth_sparse_median_f16_kernel at t_min = level against depth_sparse_f16_kernel at t_min = 1e-3, on every one of those grids: what the
      median mode's stop saves over the expected mode's.
Beside every sparse time: the share of samples live and the passes run (a debug call outside the timed window).  Device events, a warm-up,
ROUNDS rounds that alternate the variants.  Then the same launches once more in a fresh child process under rocprofv3: the kernel time per
launch, variant by variant, as DIR/time_depth_median.json; DIR/kernel_stats.csv is rocprofv3's own table.  Nothing is gated here.  GPU only."""
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
sys.path.insert(0, HERE)

from time_grid import ROUNDS, _events, _net      # noqa: E402  (the same network and event windows)
from time_sparse import _grids, _image_rays      # noqa: E402  (the same grids and image rays)

KERNELS = {"dense": "depth_f16_kernel", "dense_median": "depth_median_f16_kernel", "parent": "depth_sparse_f16_kernel",
           "new": "depth_sparse_median_f16_kernel"}
TRACED = 12      # launches per variant in the trace pass; the first two are left out of the figures
LEVEL = 0.5
GRIDS = (("all", "cells_100"), ("slab_50", "slab_50"), ("slab_25", "slab_25"), ("slab_10", "slab_10"))
EQUAL = tuple((name, gname, 0.) for name, gname in GRIDS) + (("one_pass", "cells_100", 1e-3),)      # (b): label, grid, t_min of both


def _variants(hidden, Cn, with_info):
    """[(label, which kernel, call, info)] for one width and sample count; with_info: a debug call per sparse variant (launches of its own)"""
    import nnr.ops as ops
    net = _net(hidden)
    w, b = net.weights(), net.biases()
    kw = dict(hidden=hidden, dist_alpha=False, relu_sigma=False)
    grids = _grids("cuda")
    o, d = _image_rays(256)
    z = torch.linspace(0.05, 7.5, Cn).cuda()
    R, full = o.shape[0], (Cn + 31) // 32

    def sparse(label, which, grid, t, level):
        info = {}
        if with_info:
            _, _, count, _, passes = ops.render_depth_sparse(o, d, z, z, None, grid, w, b, t_min=t, debug=True, quantile_level=level, **kw)
            info = dict(t_min=t, live_share=float(count.double().sum()) / (R * Cn), passes_mean=float(passes[::4].double().mean()), passes_full=full)
        return (label, which, lambda: ops.render_depth_sparse(o, d, z, z, None, grid, w, b, t_min=t, quantile_level=level, **kw), info)

    out = [("dense", "dense", lambda: ops.render_depth(o, d, z, z, None, w, b, **kw), {}),
           ("dense_median", "dense_median", lambda: ops.render_depth(o, d, z, z, None, w, b, quantile_level=LEVEL, **kw), {})]
    for name, gname, t in EQUAL:
        out.append(sparse("parent_" + name, "parent", grids[gname], t, None))
        out.append(sparse("new_" + name, "new", grids[gname], t, LEVEL))
    for name, gname in GRIDS:
        out.append(sparse("parent_stop_" + name, "parent", grids[gname], 1e-3, None))
        out.append(sparse("new_stop_" + name, "new", grids[gname], LEVEL, LEVEL))
    return out, dict(rays=R, samples_per_ray=Cn, hidden=hidden, level=LEVEL)


def _ratios(report, tag, med, spread, shape):
    """(a), (b) and (c) from one set of per-variant medians; `spread`: max / min of every variant in the same set"""
    report("%s_a_median_over_dense" % tag, ratio=med["dense_median"] / med["dense"], parent_spread=spread["dense"], new_spread=spread["dense_median"],
           **shape)
    for name, _, _ in EQUAL:
        report("%s_b_new_over_parent_%s" % (tag, name), ratio=med["new_" + name] / med["parent_" + name], parent_spread=spread["parent_" + name],
               new_spread=spread["new_" + name], **shape)
    for name, _ in GRIDS:
        report("%s_c_level_over_1e-3_%s" % (tag, name), ratio=med["new_stop_" + name] / med["parent_stop_" + name],
               parent_spread=spread["parent_stop_" + name], new_spread=spread["new_stop_" + name], **shape)


def events(report):
    from nnr import lib as L
    L.set_fp32_products("split2")
    for hidden in (256, 128):
        for Cn in (128, 256):
            with torch.no_grad():
                jobs, shape = _variants(hidden, Cn, True)
                for _, _, fn, _ in jobs:
                    fn()
                    fn()
                torch.cuda.synchronize()
                ms = {label: [] for label, _, _, _ in jobs}
                for _ in range(ROUNDS):       # alternating: every round times every variant once
                    for label, _, fn, _ in jobs:
                        ms[label].append(_events(fn, 10))
            tag = "events_d%d_c%d" % (hidden, Cn)
            for label, _, _, info in jobs:
                t = ms[label]
                report("%s_%s" % (tag, label), reps_per_round=10, rounds=ROUNDS, ms_min=min(t), ms_median=statistics.median(t), ms_max=max(t),
                       spread=max(t) / min(t), **shape, **info)
            _ratios(report, tag, {k: statistics.median(t) for k, t in ms.items()}, {k: max(t) / min(t) for k, t in ms.items()}, shape)


def inner(plan_path):
    """the trace pass's child: every variant TRACED times in a row, the order written down for the parent process"""
    from nnr import lib as L
    L.set_fp32_products("split2")
    plan = []
    for hidden in (256, 128):
        for Cn in (128, 256):
            with torch.no_grad():
                jobs, _ = _variants(hidden, Cn, False)
                for label, which, fn, _ in jobs:
                    for _ in range(TRACED):
                        fn()
                    plan.append(dict(hidden=hidden, samples_per_ray=Cn, label=label, kernel=KERNELS[which], launches=TRACED))
            torch.cuda.synchronize()
    with open(plan_path, "w") as f:
        json.dump(plan, f)


def trace(report, out):
    """a fresh child process under rocprofv3 (never this process, which has the GPU open) -> kernel time per launch, variant by variant"""
    tdir, plan_path = os.path.join(out, "trace"), os.path.join(out, "trace_plan.json")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "depth_median", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--inner", plan_path]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if r.returncode:
        sys.exit("time_depth_median: the rocprofv3 pass failed with status %d\n%s" % (r.returncode, r.stderr[-2000:]))
    stats = glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True)
    traces = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
    if len(stats) != 1 or len(traces) != 1:
        sys.exit("expected one kernel_stats.csv and one kernel_trace.csv under %s, found %r and %r" % (tdir, stats, traces))
    shutil.copyfile(stats[0], os.path.join(out, "kernel_stats.csv"))
    with open(plan_path) as f:
        plan = json.load(f)
    os.remove(plan_path)
    rows = []
    with open(traces[0], newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            hit = [k for k in KERNELS.values() if "nnr::%s<" % k in name or "3nnr%d%sI" % (len(k), k) in name]      # demangled or mangled
            if hit:
                rows.append((int(row["Start_Timestamp"]), max(hit, key=len), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    shutil.rmtree(tdir)
    rows.sort()
    if len(rows) != sum(p["launches"] for p in plan):
        sys.exit("the trace holds %d launches of the four kernels, the plan %d" % (len(rows), sum(p["launches"] for p in plan)))
    at, med, spread = 0, {}, {}
    for p in plan:
        mine = rows[at:at + p["launches"]]
        at += p["launches"]
        if any(k != p["kernel"] for _, k, _ in mine):
            sys.exit("the trace's launches do not stand in the plan's order at %r" % (p,))
        us = [ns / 1e3 for _, _, ns in mine[2:]]
        key = (p["hidden"], p["samples_per_ray"])
        med.setdefault(key, {})[p["label"]] = statistics.median(us)
        spread.setdefault(key, {})[p["label"]] = max(us) / min(us)
        report("trace_d%d_c%d_%s" % (key + (p["label"],)), kernel=p["kernel"], launches=len(us), us_min=min(us), us_median=statistics.median(us),
               us_max=max(us), spread=max(us) / min(us), hidden=key[0], samples_per_ray=key[1])
    for key in med:
        _ratios(report, "trace_d%d_c%d" % key, med[key], spread[key], dict(hidden=key[0], samples_per_ray=key[1], level=LEVEL))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", metavar="PLAN", help="the trace pass's child: run the launches, write their order to PLAN")
    ap.add_argument("--out", help="directory for time_depth_median.json and kernel_stats.csv (required unless --inner)")
    args = ap.parse_args()
    if not args.inner and not args.out:
        ap.error("--out DIR is required")
    if not torch.cuda.is_available():
        sys.exit("time_depth_median: needs a GPU; a CPU run measures nothing about the kernels")
    if args.inner:
        return inner(args.inner)
    lines = []

    def report(name, **kv):
        line = dict(name=name, **{k: round(v, 5) if isinstance(v, float) else v for k, v in kv.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(args.out, exist_ok=True)
    for stage in (lambda: events(report), lambda: trace(report, args.out)):      # (the events' lines are kept if the trace pass fails)
        stage()
        with open(os.path.join(args.out, "time_depth_median.json"), "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
