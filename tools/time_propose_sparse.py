"""Timings of the sparse proposal stage of hierarchical sampling (nnr_propose_f16.hip under NNR_PROPOSE_SPARSE=1 through
nnr.ops.propose_sparse; rendering.occupancy.proposal) beside the dense proposal it restates.

    python tools/time_propose_sparse.py --out DIR

In one process, for D = 256 and D = 128:
  * kernel: propose_f16_kernel<D> (nnr.ops.propose) against propose_sparse_f16_kernel<D> at C = 64 (+ 128 fine) and C = 256 (+ 256 fine), on
    the rays of one pinhole camera in image order (tools/time_sparse.py: 256 x 256 rays at C = 64, 128 x 128 at C = 256), the network fitted
    to a sphere and a box (tests/golden/phong_d<D>.npz), under these grids of 64^3 cells over [-4, 4]^3: every bit set; the fitted scene's own
    grid (geometry.occupancy_grid at raw level -3, one cell of dilation); the slabs |x| < 4 p that leave about p = 50, 25 and 10 % of the
    samples live; no bit set (0 %: no pass, no weight read).  Beside every time: the share of samples live and the passes run over the
    passes the dense kernel runs, ceil(C / 32) per workgroup (a debug call outside the timed window).
  * frame: a whole 256 x 256 sparse hierarchical frame, 64 + 128 -- the proposal and nnr.ops.render_sparse at the 192 sorted depths, the two
    launches model/rendering.py makes under rendering.occupancy with rendering.proposal 'density' -- with rendering.occupancy.proposal off
    (nnr.ops.propose) and on, under the scene's own grid and the 25 % slab; each launch alone is timed beside them (the proposal's share
    of the frame), and the share of the 192 samples the render evaluates is counted behind either proposal.
  * step: one model.Trainer_pose.train_step with eval_pose.occupancy (64 + 128 samples, 1024 rays, an untrained field with alpha_min at
    its median density) with the key off and on.
Device events, a warm-up, ROUNDS rounds that alternate the variants, so that the spread of each figure stands beside it.  Reports JSON lines
and DIR/time_propose_sparse.json.  Nothing is gated here.  GPU only."""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))
sys.path.insert(0, HERE)

from time_grid import ROUNDS, _events      # noqa: E402  (the same event windows)
from time_sparse import _grids, _image_rays, _pack      # noqa: E402  (the same grids and image rays)
from time_sparse_stop import _fitted      # noqa: E402  (the fitted network)

SHAPES = ((64, 128, 256), (256, 256, 128))      # (C, F, image side)


def _scene_grids(net, hidden):
    """{name: OccupancyGrid}, all 64^3 cells over [-4, 4]^3: every sample of the image rays lies inside"""
    import model as mdl
    from model import geometry as G
    grids = _grids("cuda")
    cfg = {'n_max_network_queries': 64000, 'white_background': False, 'radius': 4.0, 'num_points': 64, 'depth_range': [0.05, 7.5],
           'dist_alpha': False, 'use_ray_dir': True, 'normalise_ray': True, 'normal_loss': False, 'sample_option': 'uniform', 'outside_steps': 0}
    renderer = mdl.Renderer(net, cfg, device=torch.device("cuda"))
    none = G.OccupancyGrid((-4., -4., -4.), (8., 8., 8.), (64, 64, 64), _pack(torch.zeros(64, 64, 64, dtype=torch.bool)).cuda())
    return {"all": grids["cells_100"], "scene": G.occupancy_grid(renderer, [-4.] * 3, [4.] * 3, 64, -3.0, dilate=1),
            "slab_50": grids["slab_50"], "slab_25": grids["slab_25"], "slab_10": grids["slab_10"], "none": none}


def _rounds(report, jobs, group, base, info, **shape):
    """jobs [(name, fn, reps)]: warm-up, ROUNDS alternating rounds, one line per job with its time over the job `base`'s"""
    for _, fn, _ in jobs:
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in jobs}
    for _ in range(ROUNDS):
        for name, fn, reps in jobs:
            ms[name].append(_events(fn, reps))
    ref = statistics.median(ms[base])
    for name, _, reps in jobs:
        t = ms[name]
        report("%s_%s" % (group, name), reps_per_round=reps, rounds=ROUNDS, ms_min=min(t), ms_median=statistics.median(t), ms_max=max(t),
               spread=max(t) / min(t), **{"over_" + base: statistics.median(t) / ref}, **shape, **info.get(name, {}))
    return {name: statistics.median(t) for name, t in ms.items()}


def _kernel(report, hidden, net, grids):
    import nnr.ops as ops
    w, b = net.weights(), net.biases()
    kw = dict(hidden=hidden, dist_alpha=False, relu_sigma=False)
    for Cn, F, side in SHAPES:
        o, d = _image_rays(side)
        R = o.shape[0]
        z = torch.linspace(0.05, 7.5, Cn).cuda()
        dense_passes = (Cn + 31) // 32
        jobs, info = [("propose", lambda: ops.propose(o, d, z, z, None, None, F, w, b, **kw), 5)], {}
        for name, grid in grids.items():
            res = ops.propose_sparse(o, d, z, z, None, None, F, grid, w, b, debug=True, **kw)
            count, passes = res[4], res[6][::4]
            info["sparse_" + name] = dict(live_share=float(count.double().sum()) / (R * Cn), passes_mean=float(passes.double().mean()),
                                          passes_over_dense=float(passes.double().mean()) / dense_passes,
                                          histogram=torch.bincount(passes.cpu().to(torch.int64), minlength=dense_passes + 1).tolist())
            jobs.append(("sparse_" + name, lambda grid=grid: ops.propose_sparse(o, d, z, z, None, None, F, grid, w, b, **kw), 5))
        _rounds(report, jobs, "kernel_d%d_c%d" % (hidden, Cn), "propose", info, rays=R, coarse=Cn, fine=F, hidden=hidden)


def _frame(report, hidden, net, grids):
    """the two launches of a sparse hierarchical frame, as model/rendering.py issues them (tests/test_gpu_propose_sparse.py holds the
    renderer to this composition bit for bit)"""
    import nnr.ops as ops
    w, b = net.weights(), net.biases()
    kw = dict(hidden=hidden, dist_alpha=False, relu_sigma=False)
    Cn, F = 64, 128
    o, d = _image_rays(256)
    v = -d
    z = torch.linspace(0.05, 7.5, Cn).cuda()
    zero, one = torch.zeros(Cn + F, device="cuda"), torch.ones(Cn + F, device="cuda")
    for gname in ("scene", "slab_25"):
        grid = grids[gname]

        def frame(sparse):
            z_all = (ops.propose_sparse(o, d, z, z, None, None, F, grid, w, b, **kw) if sparse
                     else ops.propose(o, d, z, z, None, None, F, w, b, **kw))
            return ops.render_sparse(o, d, v, zero, one, z_all, grid, w, b, white_bg=False, **kw)
        # the share of the 192 samples the render evaluates depends on where the proposal put the fine ones: counted for both proposals
        z_on, _, _, _, coarse, _, _ = ops.propose_sparse(o, d, z, z, None, None, F, grid, w, b, debug=True, **kw)
        z_off = ops.propose(o, d, z, z, None, None, F, w, b, **kw)
        live = [float(ops.render_sparse(o, d, v, zero, one, z_all, grid, w, b, white_bg=False, debug=True, **kw)[3].double().sum())
                / (o.shape[0] * (Cn + F)) for z_all in (z_off, z_on)]
        share = dict(coarse_live_share=float(coarse.double().sum()) / (o.shape[0] * Cn), render_live_share_key_off=live[0],
                     render_live_share_key_on=live[1])
        with torch.no_grad():
            render = lambda z_all: ops.render_sparse(o, d, v, zero, one, z_all, grid, w, b, white_bg=False, **kw)      # noqa: E731
            jobs = [("key_off", lambda: frame(False), 2), ("key_on", lambda: frame(True), 2),
                    ("propose_alone", lambda: ops.propose(o, d, z, z, None, None, F, w, b, **kw), 2),
                    ("propose_sparse_alone", lambda: ops.propose_sparse(o, d, z, z, None, None, F, grid, w, b, **kw), 2),
                    ("render_alone_key_off", lambda: render(z_off), 2), ("render_alone_key_on", lambda: render(z_on), 2)]
            med = _rounds(report, jobs, "frame_d%d_%s" % (hidden, gname), "key_off", {}, rays=o.shape[0], coarse=Cn, fine=F, hidden=hidden, **share)
        report("frame_d%d_%s_shares" % (hidden, gname), dense_proposal_share_of_key_off_frame=med["propose_alone"] / med["key_off"],
               sparse_proposal_share_of_key_on_frame=med["propose_sparse_alone"] / med["key_on"], key_on_over_key_off=med["key_on"] / med["key_off"])


def _step(report, scene_dir, hidden, R=1024):
    import dataloading as dl
    import model as mdl
    import train_scene
    cfg = train_scene.scene_cfg(scene_dir, "toy", n_rays=R, n_samples=64, hidden=hidden, sample_rate=10 ** 6, num_fine=128, proposal='density')
    loader, fields = dl.get_dataloader(cfg, mode="train", shuffle=False)
    batch = next(iter(loader))
    torch.manual_seed(hidden)
    trainer, _, _ = train_scene.build(cfg, torch.device("cuda"), fields["img"].N_imgs)
    renderer = trainer.model.renderer
    # an untrained field has no empty space: alpha_min is put at the alpha of its MEDIAN raw density over the grid's points, without dilation,
    # so that a good part of the cells is culled (tests/test_gpu_frozen_sparse.py does the same)
    from model import geometry
    vol = geometry.density_volume(renderer, [-4.] * 3, [4.] * 3, (33,) * 3)
    alpha_min = 1. - math.exp(-float(torch.nn.functional.softplus(vol.flatten().nanmedian().double())))
    jobs, info, keys = [], {}, {}
    for way in ("key_off", "key_on"):
        pose = mdl.LearnPose(fields["img"].N_imgs, True, True, cfg, init_c2w=None).cuda()
        tp = mdl.Trainer_pose(trainer.model, {"n_points": R, "type": "nope_nerf", "occupancy": True}, device=torch.device("cuda"),
                              optimizer_pose=torch.optim.Adam(pose.parameters(), lr=1e-3), pose_param_net=pose)
        keys[way] = {"resolution": 64, "alpha_min": alpha_min, "dilate": 0, "proposal": way == "key_on"}

        def step(tp=tp, way=way):
            renderer.cfg["occupancy"] = keys[way]      # (the renderer is shared: each variant sets its own key for its step)
            return tp.train_step(batch)
        step()      # builds the grid
        info[way] = dict(cells_occupied=float(tp.occupancy_grid.occupied), grid_builds=tp.occupancy_builds)
        jobs.append((way, step, 3))
    _rounds(report, jobs, "step_d%d" % hidden, "key_off", info, rays=R, coarse=64, fine=128, hidden=hidden)


def workload(report):
    import scene_writer
    from nnr import lib as L
    L.set_fp32_products("split2")
    with tempfile.TemporaryDirectory() as tmp:
        scene_writer.write_scene(tmp, scene="toy", frames=2, size=(60, 80), seed=0)      # 4800 pixels: n_points 1024 of them per step
        for hidden in (256, 128):
            net = _fitted(hidden)
            with torch.no_grad():
                grids = _scene_grids(net, hidden)
                _kernel(report, hidden, net, grids)
            _frame(report, hidden, net, grids)
            _step(report, tmp, hidden)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="directory for time_propose_sparse.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_propose_sparse: needs a GPU; a CPU run measures nothing about the kernels")
    lines = []

    def report(name, **kv):
        line = dict(name=name, **{k: round(v, 5) if isinstance(v, float) else v for k, v in kv.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    workload(report)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_propose_sparse.json"), "w") as f:
        json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
