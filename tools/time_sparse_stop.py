"""Timings of the stopping sparse inference render (nnr_sparse_f16.hip under NNR_SPARSE_STOP=1 through nnr.ops.render_sparse(t_min=...);
DESIGN.md section 12.1) beside the kernel it restates.

    python tools/time_sparse_stop.py --out DIR

For D = 256 and D = 128, in one process: sparse_f16_kernel<D> (t_min absent: nnr_render_sparse) against sparse_stop_f16_kernel<D> at t_min = 0,
1e-4, 1e-3 and 1e-2, on
  * random_4096x128, random_1024x256: the random-init network (raw about 0.1 everywhere: every ray is opaque after one pass) on independent
    rays, every bit of the grid set -- the most a stop can save;
  * fitted_1023x256: the network fitted to a sphere and a box (tests/golden/phong_d<D>.npz) on rays from a shell of radius 3.5 towards the
    shape, every bit set: rays that end on a surface beside rays that miss it, in one workgroup;
  * image_256x256: the random-init network on the rays of one pinhole camera in image order (tools/time_sparse.py), the slab grid that leaves
    about half the samples live.
Device events, ROUNDS rounds that alternate the kernels, so that the spread of each figure stands beside it.  Beside every time: the mean
passes run over the passes the parent runs, and the histogram of passes per workgroup (a debug call outside the timed window).  Reports JSON
lines and DIR/time_sparse_stop.json.  Nothing is gated here.  GPU only."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
sys.path.insert(0, HERE)

from time_grid import ROUNDS, _events, _net      # noqa: E402  (the same networks and event windows)
from time_sparse import _grids, _image_rays      # noqa: E402  (the same grids and image rays)

T_MINS = (0.0, 1e-4, 1e-3, 1e-2)
LAYERS = ("layers0.0", "layers0.2", "layers0.4", "layers0.6", "layers1.0", "layers1.2", "layers1.4", "layers1.6", "fc_density",
          "fc_feature", "rgb_layers.0", "fc_rgb")


def _fitted(hidden):
    """the network the phong goldens were rendered from: weights as (mantissa, exponent) pairs"""
    net = _net(hidden)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "phong_d%d.npz" % hidden))
    sd = {}
    for n in LAYERS:
        q, e = torch.from_numpy(gold[n + ".q"].astype(np.float32)), torch.from_numpy(gold[n + ".e"].astype(np.float32))
        sd[n + ".weight"] = q * torch.exp2(e)[:, None]
        sd[n + ".bias"] = torch.from_numpy(gold[n + ".bias"])
    net.load_state_dict(sd)
    return net.cuda()


def _sets(hidden):
    """(name, network, origins, directions, z, grid, calls per round)"""
    grids = _grids("cuda")
    rnd, fit = _net(hidden), _fitted(hidden)
    out = []
    for R, N, reps in ((4096, 128, 20), (1024, 256, 20)):
        g = torch.Generator().manual_seed(R)
        o = (torch.rand(R, 3, generator=g) - 0.5).cuda()
        d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).cuda()
        out.append(("random_%dx%d" % (R, N), rnd, o, d, torch.linspace(0.05, 3.4, N).cuda(), grids["cells_100"], reps))
    g = torch.Generator().manual_seed(1023)
    o = torch.nn.functional.normalize(torch.randn(1023, 3, generator=g), dim=1) * 3.5
    target = (torch.rand(1023, 3, generator=g) - 0.5) * 2.0
    d = torch.nn.functional.normalize(target - o, dim=1)
    out.append(("fitted_1023x256", fit, o.cuda(), d.cuda(), torch.linspace(0.1, 7.0, 256).cuda(), grids["cells_100"], 20))
    oi, di = _image_rays(256)
    out.append(("image_256x256", rnd, oi, di, torch.linspace(0.05, 7.5, 128).cuda(), grids["slab_50"], 2))
    return out


def workload(report):
    import nnr.ops as ops
    for hidden in (256, 128):
        kw = dict(hidden=hidden, dist_alpha=False, white_bg=False, relu_sigma=False)
        for name, net, o, d, z, grid, reps in _sets(hidden):
            w, b = net.weights(), net.biases()
            v = -d
            n_rays, n = o.shape[0], z.shape[0]

            def call(t_min=None, debug=False):
                extra = {} if t_min is None else {"t_min": t_min}
                return ops.render_sparse(o, d, v, z, z, None, grid, w, b, debug=debug, **extra, **kw)

            jobs, info = [("parent", call)], {}
            with torch.no_grad():
                count = call(debug=True)[3]
                pad = torch.cat([count, count[-1:].expand((-n_rays) % 4)]).view(-1, 4)
                parent_passes = (pad.max(1)[0] + 31) // 32
                info["parent"] = dict(passes_mean=float(parent_passes.double().mean()), passes_over_parent=1.0,
                                      histogram=torch.bincount(parent_passes.cpu().to(torch.int64)).tolist())
                for t in T_MINS:
                    tag = "t_min_%g" % t
                    if t > 0.:
                        ran = call(t, debug=True)[6][::4]
                        info[tag] = dict(passes_mean=float(ran.double().mean()),
                                         passes_over_parent=float(ran.double().sum()) / max(float(parent_passes.double().sum()), 1.),
                                         histogram=torch.bincount(ran.cpu().to(torch.int64)).tolist())
                        jobs.append((tag, lambda t=t: call(t)))
                    else:      # ops.render_sparse takes t_min = 0 to the parent's entry: the new entry at 0 is called directly
                        info[tag] = dict(info["parent"])
                        jobs.append((tag, _zero_call(ops, o, d, v, z, grid, w, b, hidden)))
                for _, fn in jobs:      # warm up every variant of the timed window
                    fn()
                    fn()
                torch.cuda.synchronize()
                ms = {k: [] for k, _ in jobs}
                for _ in range(ROUNDS):       # alternating: every round times every variant once
                    for k, fn in jobs:
                        ms[k].append(_events(fn, reps))
            base = statistics.median(ms["parent"])
            for k, _ in jobs:
                t = ms[k]
                report("%s_%s_d%d" % (name, k, hidden), rays=n_rays, samples_per_ray=n, live_share=float(count.double().sum()) / (n_rays * n),
                       reps_per_round=reps, rounds=ROUNDS, ms_min=min(t), ms_median=statistics.median(t), ms_max=max(t), spread=max(t) / min(t),
                       over_parent=statistics.median(t) / base, **info[k])


def _zero_call(ops, o, d, v, z, grid, w, b, hidden):
    """nnr_render_sparse_stop at t_min = 0 on render_sparse's own inputs: what one more barrier per pass costs"""
    import ctypes as C
    from nnr import lib as L
    R, n = o.shape[0], z.shape[0]
    cfg = ops.split2_cfg(R, n, hidden)
    packed = ops._packed_for(cfg, list(w), list(b))
    lo3, is3, d3, bits = ops._grid_args(grid, o.device, "time_sparse_stop")
    out = torch.empty(R, 5, dtype=torch.float32, device=o.device)
    keep = (cfg, packed, lo3, is3, d3, bits, out)

    def fn():
        L.check(L.load().nnr_render_sparse_stop(C.byref(cfg), L.ptr(o), L.ptr(d), L.ptr(v), L.ptr(z), L.ptr(z), None, lo3, is3, d3, L.ptr(bits),
                                                L.ptr(packed), 0.0, L.ptr(out), None, None, None, None, L.stream()), "nnr_render_sparse_stop")
        return keep
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="directory for time_sparse_stop.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_sparse_stop: needs a GPU; a CPU run measures nothing about the kernels")
    lines = []

    def report(name, **kv):
        line = dict(name=name, **{k: round(v, 5) if isinstance(v, float) else v for k, v in kv.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    workload(report)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_sparse_stop.json"), "w") as f:
        json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
