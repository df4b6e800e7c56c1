"""Timings of the sparse inference render (nnr_sparse_f16.hip through nnr.ops.render_sparse) beside the dense
inference forward it restates.

    python tools/time_sparse.py --out DIR           # device-event timings, then a rocprofv3 --kernel-trace --stats pass of its own
    python tools/time_sparse.py --inner             # the workload the trace pass runs (also usable on its own)

For D = 256 and D = 128, in one process (and one trace), on the same 4096 rays x 128 samples: mlp_fwd_f16_kernel<D, false> with the compositing
in its epilogue (nnr.render_rays, samples=False, two-term products) against sparse_f16_kernel<D> with synthetic grids that leave about 100, 50,
25 and 10 % of the samples live, in two patterns: `cells` -- the bits of a 64^3 grid drawn at random, so that every ray keeps about that share of
its samples, scattered -- and `slab` -- the cells of a slab |x| < h set, so that a ray's live samples form one run, as behind a real surface, and
rays that miss the slab have none.  A second set, `image`: 256 x 256 rays of one pinhole camera in image order, the slab across its view --
neighbouring rays, as a frame's are, where the first set's rays are independent.  The live share of each grid is counted (a debug call) and reported beside its time.  Timed in ROUNDS rounds
that alternate the kernels (tools/time_grid.py), so that the run-to-run spread of each figure stands beside it.  Random-init networks (the
kernels' times do not depend on the weights).  Reports JSON lines and DIR/time_sparse.json; the trace pass gives the per-kernel figures (the
events include launch gaps): DIR/sparse_kernel_stats.csv is rocprofv3's own table, DIR/sparse_kernel_trace_summary.json the count / min /
median / max duration per kernel and grid size.  The 100 % ratio to the dense kernel is recorded, not gated.  GPU only."""
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

R, N = 4096, 128
IMAGE = 256      # the image set: IMAGE x IMAGE rays in image order
SHARES = (1.0, 0.5, 0.25, 0.1)


def _grids(device):
    """{name: OccupancyGrid}: 64^3 cells over [-4, 4]^3 (every sample of the rays below lies inside)"""
    from model import geometry as G
    n = 64
    g = torch.Generator().manual_seed(3)
    out = {}
    for p in SHARES:
        occ = torch.rand(n, n, n, generator=g) < p
        x = (torch.arange(n, dtype=torch.float32) + 0.5) / n * 8. - 4.
        slab = (x.abs() < 4. * p)[None, None, :].expand(n, n, n)
        for kind, cells in (("cells", occ), ("slab", slab)):
            bits = _pack(cells).to(device)      # (from the cells themselves: no volume, no dilation)
            out["%s_%d" % (kind, round(100 * p))] = G.OccupancyGrid((-4., -4., -4.), (8., 8., 8.), (n, n, n), bits)
    return out


def _pack(cells):
    """(n_z, n_y, n_x) bool -> the int32 words of include/nnr_sparse.h"""
    nz, ny, nx = cells.shape
    wx = (nx + 31) // 32
    pad = torch.zeros(nz, ny, wx * 32, dtype=torch.int64)
    pad[..., :nx] = cells.to(torch.int64)
    w = (pad.view(nz, ny, wx, 32) << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


def _image_rays(side):
    """side x side rays of a pinhole camera at (-3.9, 0, 0) looking along +x (half-angle atan(0.35)), in image order: the four rays of a
    workgroup are neighbouring pixels, and the `slab` grids (|x| < h) lie across the view like a surface's shell"""
    t = (torch.arange(side, dtype=torch.float32) + 0.5) / side * 0.7 - 0.35
    yy, zz = torch.meshgrid(t, t, indexing="ij")
    d = torch.nn.functional.normalize(torch.stack([torch.ones_like(yy), zz, yy], -1).view(-1, 3), dim=-1)
    o = torch.tensor([-3.9, 0., 0.]).expand_as(d).contiguous()
    return o.cuda(), d.cuda()


def _time(report, jobs, live, hidden, n_rays, tag):
    for _, fn, _ in jobs:      # warm up every shape of the timed window
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in jobs}
    for _ in range(ROUNDS):       # alternating: every round times every kernel once
        for name, fn, reps in jobs:
            ms[name].append(_events(fn, reps))
    fwd = statistics.median(ms["forward" + tag])
    for name, _, reps in jobs:
        t = ms[name]
        report("%s_d%d" % (name, hidden), rays=n_rays, samples_per_ray=N, reps_per_round=reps, rounds=ROUNDS, live_share=live.get(name, 1.0),
               ms_min=min(t), ms_median=statistics.median(t), ms_max=max(t), spread=max(t) / min(t),
               ns_per_sample_median=statistics.median(t) * 1e6 / (n_rays * N), over_forward=statistics.median(t) / fwd)


def workload(report):
    import nnr
    import nnr.ops as ops
    from nnr import lib as L
    L.set_fp32_products("split2")      # the dense kernel in the sparse kernel's arithmetic
    g = torch.Generator().manual_seed(R)
    o = ((torch.rand(R, 3, generator=g) - 0.5)).cuda()
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).cuda()
    oi, di = _image_rays(IMAGE)
    sets = (("", o, d, torch.linspace(0.05, 3.4, N).cuda(), 20, None), ("_image", oi, di, torch.linspace(0.05, 7.5, N).cuda(), 2, "slab"))
    grids = _grids("cuda")
    for hidden in (256, 128):
        net = _net(hidden)
        w, b = net.weights(), net.biases()
        kw = dict(hidden=hidden, dist_alpha=False, white_bg=False, relu_sigma=False)
        for tag, ro, rd, z, reps, only in sets:
            rv = -rd
            jobs = [("forward" + tag, lambda ro=ro, rd=rd, rv=rv, z=z: nnr.render_rays(ro, rd, rv, z, z, None, w, b, samples=False, **kw), reps)]
            live = {}
            with torch.no_grad():
                for name, grid in grids.items():
                    if only and not name.startswith(only):
                        continue
                    count = ops.render_sparse(ro, rd, rv, z, z, None, grid, w, b, debug=True, **kw)[3]
                    live["sparse%s_%s" % (tag, name)] = float(count.double().sum()) / (ro.shape[0] * N)
                    jobs.append(("sparse%s_%s" % (tag, name),
                                 lambda grid=grid, ro=ro, rd=rd, rv=rv, z=z: ops.render_sparse(ro, rd, rv, z, z, None, grid, w, b, **kw), reps))
                _time(report, jobs, live, hidden, ro.shape[0], tag)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--out", help="directory for time_sparse.json and the trace's summaries (required unless --inner)")
    args = ap.parse_args()
    if not args.inner and not args.out:
        ap.error("--out DIR is required")
    if not torch.cuda.is_available():
        sys.exit("time_sparse: needs a GPU; a CPU run measures nothing about the kernels")
    lines = []

    def report(name, **kv):
        line = dict(name=name, **{k: round(v, 5) if isinstance(v, float) else v for k, v in kv.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    workload(report)
    if args.inner:
        return
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_sparse.json"), "w") as f:
        json.dump(lines, f, indent=1)
    # the trace pass: a fresh child process under rocprofv3 (never this process, which has the GPU open)
    trace = os.path.join(args.out, "sparse_trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "sparse", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    if r.returncode:
        sys.exit("time_sparse: the rocprofv3 pass failed with status %d\n%s" % (r.returncode, r.stderr[-2000:]))
    summarise_trace(args.out, prefix="sparse_")


if __name__ == "__main__":
    main()
