"""Timings of the two kernels of the TSDF export (nnr_depth_f16.hip through nnr.ops.render_depth, nnr_tsdf.hip through
nnr.ops.tsdf_integrate).

    python tools/time_fusion.py --out DIR           # device-event timings, then a rocprofv3 --kernel-trace --stats pass of its own
    python tools/time_fusion.py --inner             # the workload the trace pass runs (also usable on its own)

(a) For D = 256 and D = 128, in one process (and one trace): depth_f16_kernel against the inference forward that a depth render ran before
(nnr.render_rays, samples=False: mlp_fwd_f16_kernel<D, false> with the compositing in its epilogue) on the same rays, at 1024 rays x 192
samples and at one 540 x 960 image x 192 samples, in ns per sample.  (b) tsdf_integrate_kernel on all bricks of a 128^3 and a 256^3 grid
with 16 and 64 cameras of 270 x 480 on a sphere around it, in ns per voxel-camera pair.  The sizes are timed in ROUNDS rounds that
alternate the kernels (tools/time_grid.py), so that the run-to-run spread of each figure stands beside it: the bar for the depth kernel is
"no slower per sample than the forward in the same run, beyond that run's own spread".  Random-init networks and constant depth maps (the
kernels' times depend on neither, beyond which voxels pass the kernel's tests: the maps put a surface through the grid).
Reports JSON lines and DIR/time_fusion.json; the trace pass gives the per-kernel figures (the events include launch gaps):
DIR/fusion_kernel_stats.csv is rocprofv3's own table, DIR/fusion_kernel_trace_summary.json the count / min / median / max duration per
kernel and grid size from its kernel trace (the trace itself is removed).  Exits non-zero if the trace pass fails.  GPU only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
sys.path.insert(0, HERE)

from time_bricks import _bricks_of                                 # noqa: E402
from time_grid import ROUNDS, _events, _net, summarise_trace      # noqa: E402  (the same networks, event windows and trace summary)


def _look_at_rows(n, radius, f=0.6):
    """rows 0..2 of K . world_mat of n cameras on a Fibonacci sphere looking at the origin, K = diag(f, -f, -1, 1) -> (n,12) fp32"""
    rows, golden = [], np.pi * (3. - np.sqrt(5.))
    for i in range(n):
        z = 1. - (2 * i + 1) / n
        r = np.sqrt(1. - z * z)
        c = radius * np.array([r * np.cos(golden * i), r * np.sin(golden * i), z])
        back = c / np.linalg.norm(c)
        right = np.cross([0., 0., 1.], back)
        right /= np.linalg.norm(right)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(back, right), back, c
        rows.append((np.diag([f, -f, -1., 1.]) @ np.linalg.inv(c2w))[:3].reshape(12))
    return torch.from_numpy(np.stack(rows).astype(np.float32)).cuda()


def _run(jobs, report, tag, unit):
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
        report("%s%s" % (name, tag), **{unit: count, "reps_per_round": reps, "rounds": ROUNDS, "ns_min": min(v), "ns_median": statistics.median(v),
                                       "ns_max": max(v), "ms_median": statistics.median(v) * count / 1e6})
    return ns


def workload(report):
    import nnr
    import nnr.ops as ops
    N = 192
    z = torch.linspace(0.01, 10., N).cuda()
    for hidden in (256, 128):
        net = _net(hidden)
        w, b = net.weights(), net.biases()
        jobs = []
        for name, R, reps in (("1024x192", 1024, 200), ("540x960x192", 540 * 960, 1)):
            g = torch.Generator().manual_seed(R)
            o = (torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 2.5).cuda()
            d = torch.nn.functional.normalize(-o + 0.3 * torch.randn(R, 3, generator=g).cuda(), dim=-1)
            v = -d
            depth = lambda o=o, d=d: ops.render_depth(o, d, z, z, None, w, b, hidden=hidden, dist_alpha=False, relu_sigma=False)
            fwd = lambda o=o, d=d, v=v: nnr.render_rays(o, d, v, z, z, None, w, b, hidden=hidden, dist_alpha=False, white_bg=False,
                                                        relu_sigma=False, samples=False)
            jobs += [("depth_" + name, depth, reps, R * N), ("forward_" + name, fwd, reps, R * N)]
        with torch.no_grad():
            ns = _run(jobs, report, "_d%d" % hidden, "samples")
        med = {k: statistics.median(v) for k, v in ns.items()}
        report("ratios_d%d" % hidden, depth_over_forward_1024=med["depth_1024x192"] / med["forward_1024x192"],
               depth_over_forward_image=med["depth_540x960x192"] / med["forward_540x960x192"],
               forward_1024_spread=max(ns["forward_1024x192"]) / min(ns["forward_1024x192"]),
               forward_image_spread=max(ns["forward_540x960x192"]) / min(ns["forward_540x960x192"]),
               depth_1024_spread=max(ns["depth_1024x192"]) / min(ns["depth_1024x192"]),
               depth_image_spread=max(ns["depth_540x960x192"]) / min(ns["depth_540x960x192"]))
    # (b) the fusion: a surface at depth 3 from every camera (a sphere-like shell through the grid), all bricks
    H, W = 270, 480
    jobs = []
    for n in (128, 256):
        bricks = _bricks_of(n)
        acc = torch.zeros(2, bricks.shape[0], 8, 8, 8, device="cuda")
        origin, step = (-1., -1., -1.), (2. / (n - 1),) * 3
        for n_cams in (16, 64):
            cams = _look_at_rows(n_cams, 3.)
            maps = torch.full((n_cams, H, W), 3., device="cuda")
            fn = lambda o=origin, s=step, br=bricks, cm=cams, mp=maps, a=acc: ops.tsdf_integrate(o, s, br, cm, mp, 3 * s[0], a[0], a[1])
            jobs.append(("tsdf_%d_cams%d" % (n, n_cams), fn, 20 if n == 128 else 3, n ** 3 * n_cams))
    _run(jobs, report, "", "voxel_camera_pairs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--out", help="directory for time_fusion.json and the trace's summaries (required unless --inner)")
    args = ap.parse_args()
    if not args.inner and not args.out:
        ap.error("--out DIR is required")
    if not torch.cuda.is_available():
        sys.exit("time_fusion: needs a GPU; a CPU run measures nothing about the kernels")
    lines = []

    def report(name, **kv):
        line = dict(name=name, **{k: round(v, 5) if isinstance(v, float) else v for k, v in kv.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    workload(report)
    if args.inner:
        return
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_fusion.json"), "w") as f:
        json.dump(lines, f, indent=1)
    # the trace pass: a fresh child process under rocprofv3 (never this process, which has the GPU open)
    trace = os.path.join(args.out, "fusion_trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "fusion", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if r.returncode:
        sys.exit("time_fusion: the rocprofv3 pass failed with status %d\n%s" % (r.returncode, r.stderr[-2000:]))
    summarise_trace(args.out, prefix="fusion_")


if __name__ == "__main__":
    main()
