#!/usr/bin/env python
"""Joint pose + radiance-field training on a scene in the reference's on-disk layout, through this repository's `dataloading`,
`model` and `utils_poses` packages -- the loop of reference train.py:198-300 without its logging / checkpoint plumbing, used for
the offline convergence runs of SURVEY.md 8(d) (configs 4-5) and to time the loop with the host loader against the HBM-resident
one.  GPU only (the render path has no CPU fallback).

    python tools/scene_writer.py /tmp/scenes --frames 16 --size 120 160
    python tools/train_scene.py /tmp/scenes synthetic --epochs 200 [--style tanks|llff] [--host-loader] [--out result.json]
                                [--checkpoint-dir DIR] [--occupancy RES ALPHA_MIN [ALPHA_MIN ...]] [--ray-distortion W]

--occupancy: after the last epoch render full frames of training views dense and through rendering.occupancy (the sparse inference render) and
print, per ALPHA_MIN, the share of samples culled and the PSNR of the sparse against the dense frames (style tanks: the grid covers the cube
of rendering.radius).

--sparse-proposal (with --occupancy or --frozen-occupancy, together with --num-fine F --proposal density): rendering.occupancy.proposal:
true, the proposal of hierarchical sampling skips the coarse samples the grid calls empty.  With --occupancy the
frames are the sparse hierarchical render's, once with the dense and once with the sparse proposal: per ALPHA_MIN the share of coarse samples
culled and the PSNR of the sparse-proposal frames against the dense-proposal frames.  With --frozen-occupancy the second pose refinement
proposes through its grid and reports the share of coarse samples culled.

--ray-distortion W: training.ray_distortion_weight = W, the weight of the ray distortion of the compositing weights (DESIGN.md section 13;
0 = off, the default; the paper's example is 0.01).  The last logged line then carries the epoch's mean loss_ray_distortion.

--checkpoint-dir: after the last epoch write model.pt, model_pose.pt (and model_focal.pt where a focal is learnt) there through
CheckpointIO, in the layout train.py writes and tools/extract_mesh.py loads (save_checkpoints), next to config.yaml: the run's whole
configuration with training.out_dir = DIR, which that tool takes as its config (with --default pointing at no file).

Reported per run: PSNR of the training rays (from l2_mean, as train.py:283-285 does), ATE / RPE of the learned poses against the
scene's ground truth after sim(3) alignment (train.py:270-281), loop throughput in steps/s and rays/s.  One host sync per epoch
(the reference's loop calls .item() three times per step, train.py:212-214)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))

import numpy as np
import torch


def scene_cfg(path, scene, style="tanks", n_rays=1024, n_samples=128, hidden=256, resident=True, aux=True, resize_factor=None,
              sample_rate=8, workers=0, mfma_dtype="fp32", num_fine=0, proposal=None, ray_distortion=0.0):
    """The keys configs/default.yaml + configs/Tanks/*.yaml (style 'tanks') or configs/LLFF/fern.yaml (style 'llff') would set."""
    llff = style == "llff"
    on = [1.0, 0.0] if aux else [0.0, 0.0]
    return {
        "model": {"hidden_dim": hidden, "pos_enc_levels": 10, "dir_enc_levels": 4, "occ_activation": "softplus",
                  "network_type": "official"},
        "dataloading": {"dataset_name": "any", "path": path, "scene": [scene], "batchsize": 1, "n_workers": workers, "with_depth": False,
                        "spherify": True, "customized_poses": False, "customized_focal": False, "resize_factor": resize_factor,
                        "depth_net": "dpt", "crop_size": 0, "random_ref": 1, "norm_depth": False, "load_colmap_poses": True,
                        "shuffle": True, "sample_rate": sample_rate, "resident": resident},
        "rendering": {"type": "nope_nerf", "n_max_network_queries": 64000, "white_background": False, "radius": 4.0,
                      "num_points": n_samples, "depth_range": [0.0, 1.0] if llff else [0.01, 10], "dist_alpha": llff,
                      "use_ray_dir": True, "normalise_ray": True, "normal_loss": False,
                      "sample_option": "ndc" if llff else "uniform", "outside_steps": 0, "mfma_dtype": mfma_dtype,
                      **({"num_fine": int(num_fine)} if num_fine else {}),
                      **({"proposal": str(proposal)} if proposal else {})},      # hierarchical sampling: num_points coarse + num_fine fine
        "depth": {"type": "None"},
        "pose": {"learn_pose": True, "learn_R": True, "learn_t": True, "init_pose": False, "learn_focal": False},
        "distortion": {"learn_distortion": True, "fix_scaleN": True, "learn_scale": True, "learn_shift": True},
        "training": {
            "type": "nope_nerf", "n_training_points": n_rays, "vis_geo": False, "detach_gt_depth": False, "pc_ratio": 4,
            "match_method": "dense", "shift_first": False, "detach_ref_img": True, "scale_pcs": True, "detach_rgbs_scale": False,
            "vis_reprojection_every": 10 ** 9, "nearest_limit": 0.01, "annealing_epochs": 2000, "rgb_weight": [1.0, 1.0],
            "depth_weight": [0.04, 0.0], "pc_weight": on, "rgb_s_weight": on, "depth_consistency_weight": [0.0, 0.0],
            "weight_dist_2nd_loss": [0.0, 0.0], "weight_dist_1st_loss": [0.0, 0.0], "depth_loss_type": "l1", "with_ssim": False,
            "with_auto_mask": False, "learning_rate": 1e-3, "pose_lr": 5e-4, "distortion_lr": 5e-4,
            **({"ray_distortion_weight": float(ray_distortion)} if ray_distortion else {}),
        },
    }


def num_fine_of(cfg):
    return int(cfg["rendering"].get("num_fine", 0) or 0)


def build(cfg, device, n_views):
    import model as mdl
    net = mdl.OfficialStaticNerf(cfg)
    nope = mdl.get_model(mdl.Renderer(net, cfg["rendering"], device=device), cfg, device=device)
    pose = mdl.LearnPose(n_views, True, True, cfg, init_c2w=None).to(device)
    dist = mdl.Learn_Distortion(n_views, True, True, cfg).to(device)
    t = cfg["training"]
    opt = torch.optim.Adam(nope.parameters(), lr=t["learning_rate"])
    opt_pose = torch.optim.Adam(pose.parameters(), lr=t["pose_lr"])
    opt_dist = torch.optim.Adam(dist.parameters(), lr=t["distortion_lr"])
    trainer = mdl.Trainer(nope, opt, t, device=device, optimizer_pose=opt_pose, pose_param_net=pose, optimizer_distortion=opt_dist,
                          distortion_net=dist, cfg_all=cfg)
    return trainer, pose, dist


def save_checkpoints(out_dir, nope, pose, focal=None, **scalars):
    """model.pt, model_pose.pt and, with a focal net, model_focal.pt in out_dir: one CheckpointIO file per module group, each registered as
    'model', as train.py writes them (tools/extract_mesh.py: load_pose_table reads the pose table back)."""
    import model as mdl
    mdl.CheckpointIO(out_dir, model=nope).save("model.pt", **scalars)
    mdl.CheckpointIO(out_dir, model=pose).save("model_pose.pt", **scalars)
    if focal is not None:
        mdl.CheckpointIO(out_dir, model=focal).save("model_focal.pt", **scalars)


def pose_errors(pose_net, gt_poses, n_views):
    from utils_poses.align_traj import align_ate_c2b_use_a2b
    from utils_poses.comp_ate import compute_ATE, compute_rpe
    with torch.no_grad():
        learned = torch.stack([pose_net(i) for i in range(n_views)])
    aligned = align_ate_c2b_use_a2b(learned, gt_poses).cpu().numpy()
    gt = gt_poses.cpu().numpy()
    rpe_t, rpe_r = compute_rpe(gt, aligned)
    return {"ate": float(compute_ATE(gt, aligned)), "rpe_trans_x100": float(rpe_t * 100), "rpe_rot_deg": float(np.degrees(rpe_r))}


def novel_view_eval(cfg, nope, pose, train_field, device, epochs, out_dir, n_points=1024, frozen_field=True, frozen_occupancy=None,
                    sparse_proposal=False):
    """What reference evaluation/eval.py:54-186 does for the held-out views: initialise their poses from the learned training
    trajectory (init_method 'pre': the training pose just before each held-out frame), optimise them against the frozen field
    (Trainer_pose, Adam 1e-3 halved five times), then render every held-out frame in full and score it.  LPIPS needs a VGG
    checkpoint and is reported as 0.  frozen_field (eval_pose.frozen_field; --no-frozen-eval: False): the refinement steps run the render
    operator's frozen-field mode -- same losses and poses, no weight gradient; the path taken is printed.
    frozen_occupancy = (resolution, alpha_min) (--frozen-occupancy; eval_pose.occupancy: true): the same refinement is run a second time from
    the same initial poses with an occupancy grid of the field, built once, the samples it calls empty skipped forward and backward
    (DESIGN.md section 15); the result carries the culled share, the largest distance between the two runs' refined poses and both PSNRs.
    sparse_proposal (--sparse-proposal; rendering.occupancy.proposal: true): that second refinement also proposes through the grid
    (DESIGN.md section 12.2); the result then carries the share of coarse samples its proposals culled."""
    import dataloading as dl
    import model as mdl
    from model.eval_images import Eval_Images
    loader, fields = dl.get_dataloader(cfg, mode="eval", shuffle=False)
    f = fields["img"]
    if f.N_imgs == 0:
        return None
    with torch.no_grad():
        learned = torch.stack([pose(i) for i in range(train_field.N_imgs)])
    sr = train_field.sample_rate
    init = learned[int(sr / 2) - 1::sr - 1][:f.N_imgs].clone()
    zero = lambda a, b, normalize=True: torch.zeros(())

    def refine_and_score(occupancy):
        eval_pose = mdl.LearnPose(f.N_imgs, True, True, cfg, init_c2w=init.clone()).to(device)
        opt = torch.optim.Adam(eval_pose.parameters(), lr=1e-3)
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(range(0, epochs, max(1, epochs // 5))), gamma=0.5)
        tp = mdl.Trainer_pose(nope, {"n_points": n_points, "type": "nope_nerf", "frozen_field": bool(frozen_field), "occupancy": bool(occupancy)},
                              device=device, optimizer_pose=opt, pose_param_net=eval_pose)
        print(json.dumps({"eval_pose_path": ("frozen field with an occupancy grid (nnr.frozen_field(occupancy=grid): known-empty samples skipped)"
                                             if tp.occupancy else "frozen field (nnr.frozen_field: no activation stash, no weight gradient)")
                          if tp.frozen_field else "full training path (eval_pose.frozen_field: false)"}), flush=True)
        first = last = None
        from nnr import ops
        ops.frozen_sparse_tally = [] if occupancy else None
        ops.propose_sparse_tally = [] if occupancy and sparse_proposal else None
        try:
            if occupancy:      # (the key is the renderer's; it is taken away again before the frames are rendered: those stay dense)
                nope.renderer.cfg["occupancy"] = {"resolution": int(frozen_occupancy[0]), "alpha_min": float(frozen_occupancy[1]),
                                                  **({"proposal": True} if sparse_proposal else {})}
            for e in range(epochs):
                l2 = torch.stack([tp.train_step(batch)["loss"].detach() for batch in loader]).mean()
                sched.step()
                if e in (0, epochs - 1):
                    v = float(l2)
                    first, last = (v, last) if e == 0 else (first, v)
        finally:
            tally, ops.frozen_sparse_tally = ops.frozen_sparse_tally, None
            ptally, ops.propose_sparse_tally = ops.propose_sparse_tally, None
            if occupancy:
                nope.renderer.cfg.pop("occupancy", None)
        eval_pose.eval()
        with torch.no_grad():
            c2ws = torch.stack([eval_pose(i) for i in range(f.N_imgs)])
        gen = Eval_Images(nope.renderer, dict(cfg, extract_images={"resolution": [f.H, f.W]}), use_learnt_poses=True, use_learnt_focal=False,
                          device=device, render_type="nope_nerf", c2ws=c2ws, img_list=f.img_list)
        t0 = time.perf_counter()
        rows = [gen.eval_images(batch, out_dir, None, zero, logger=None) for batch in loader]
        dt = time.perf_counter() - t0
        res = {"views": f.N_imgs, "pose_opt_epochs": epochs, "pose_opt_mse_first": first, "pose_opt_mse_last": last,
               "psnr": float(np.mean([r["psnr"] for r in rows])), "ssim": float(np.mean([r["ssim"] for r in rows])),
               "seconds_per_frame": dt / max(1, len(rows))}
        if tally:
            live, total = float(torch.stack([t[0] for t in tally]).sum()), float(sum(t[1] for t in tally))
            res.update(samples_culled=1. - live / total, grid_builds=tp.occupancy_builds,
                       cells_occupied=float(tp.occupancy_grid.occupied) if tp.occupancy_grid is not None else None)
        if ptally:
            live, total = float(torch.stack([t[0] for t in ptally]).sum()), float(sum(t[1] for t in ptally))
            res.update(coarse_samples_culled=1. - live / total)
        return res, c2ws

    dense, c2ws = refine_and_score(False)
    if frozen_occupancy is None or not frozen_field:
        return dense
    sparse, c2ws_s = refine_and_score(True)
    sparse["pose_distance_to_dense"] = {"rotation_max_abs": float((c2ws_s[:, :3, :3] - c2ws[:, :3, :3]).abs().max()),
                                        "translation_max_abs": float((c2ws_s[:, :3, 3] - c2ws[:, :3, 3]).abs().max())}
    return dict(dense, frozen_occupancy=sparse)


def occupancy_compare(cfg, nope, pose, loader, field, device, resolution, alpha_mins, dilate=1, bounds=None, frames=4, t_min=None):
    """Full frames of the first `frames` training views at their learned poses, rendered dense and with rendering.occupancy (the sparse
    inference render) for every alpha_min -> rows of {alpha_min, cells occupied, samples culled, PSNR of the sparse
    against the dense frames, seconds per frame of both}.  The culled share is counted by a debug call of nnr.ops.render_sparse on the
    frames' rays; the timed renders run without it.  t_min (rendering.occupancy.t_min: early ray termination): one more
    row per alpha_min, the same grid rendered with the stop -- the passes its workgroups run over the passes the sparse render runs, the PSNR
    of the stopped frames against the dense ones, seconds per frame."""
    import model as mdl
    from model import imaging
    from nnr import camera
    from nnr import ops
    from model.common import arange_pixels, mse2psnr
    base = nope.renderer
    base.eval()
    views = []
    for batch in loader:
        if len(views) >= frames:
            break
        views.append((batch["img.camera_mat"].to(device), batch["img.scale_mat"].to(device), int(batch["img.idx"])))
    with torch.no_grad():
        mats = [(cam, imaging.inverse_pose(pose(i)), scale) for cam, scale, i in views]
    size = (field.H, field.W)

    def frames_of(renderer):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [imaging.render_full_image(renderer, size, cam, world, scale, "nope_nerf", device)[0] for cam, world, scale in mats]
        torch.cuda.synchronize()
        return torch.stack(out), (time.perf_counter() - t0) / len(mats)

    frames_of(base)      # (lazy initialisations)
    dense, t_dense = frames_of(base)
    rows = []
    for alpha_min in alpha_mins:
        occ = {"resolution": int(resolution), "alpha_min": float(alpha_min), "dilate": int(dilate)}
        if bounds is not None:
            occ["bounds"] = list(bounds)
        sparse_r = mdl.Renderer(base.model, dict(cfg["rendering"], occupancy=occ), device=device)
        sparse_r.eval()
        frames_of(sparse_r)      # (builds the grid)
        sparse, t_sparse = frames_of(sparse_r)
        grid = sparse_r.__dict__["_occupancy_hit"][2]
        live = total = ran = parent_passes = 0
        if t_min:
            stop_r = mdl.Renderer(base.model, dict(cfg["rendering"], occupancy=dict(occ, t_min=float(t_min))), device=device)
            stop_r.eval()
            frames_of(stop_r)
            stopped, t_stop = frames_of(stop_r)
        with torch.no_grad():
            pixels = arange_pixels(resolution=size, device=device)[1]
            depth = torch.ones(1, pixels.shape[1], 1, device=device)
            for cam, world, scale in mats:
                origin, ray, view, _, _, _ = camera.ray_setup(pixels, depth, cam, world, scale, bool(cfg["rendering"]["normalise_ray"]),
                                                              bool(cfg["rendering"]["use_ray_dir"]))
                if cfg["rendering"]["sample_option"] == "ndc":
                    origin, ray = camera.ndc_rays(origin, ray, cam, 1.0)
                    z_lo, z_hi = sparse_r._z_tables(cfg["rendering"]["num_points"], 0., 1., False, device)
                else:
                    z_lo, z_hi = sparse_r._z_tables(cfg["rendering"]["num_points"], *base.depth_range, False, device)
                net = base.model
                kw = dict(hidden=net.hidden_dim, dist_alpha=bool(cfg["rendering"]["dist_alpha"]), white_bg=False,
                          relu_sigma=(net.occ_activation != "softplus"), debug=True)
                count = ops.render_sparse(origin, ray, view, z_lo, z_hi, None, grid, net.weights(), net.biases(), **kw)[3]
                live += int(count.sum())
                total += count.numel() * int(z_lo.shape[0])
                if t_min:      # per workgroup of four rays: the passes run with the stop, and the sparse render's own ceil(max live / 32)
                    passes = ops.render_sparse(origin, ray, view, z_lo, z_hi, None, grid, net.weights(), net.biases(), t_min=float(t_min), **kw)[6]
                    ran += int(passes[::4].sum())
                    pad = torch.cat([count, count[-1:].expand((-count.numel()) % 4)]).view(-1, 4)
                    parent_passes += int(((pad.max(1)[0] + 31) // 32).sum())
        mse = float(torch.nn.functional.mse_loss(sparse, dense))
        rows.append({"alpha_min": float(alpha_min), "resolution": int(resolution), "cells_occupied": float(grid.occupied),
                     "samples_culled": 1. - live / max(total, 1), "psnr_sparse_vs_dense": float(mse2psnr(mse)) if mse > 0. else float("inf"),
                     "seconds_per_frame_dense": t_dense, "seconds_per_frame_sparse": t_sparse, "frames": len(mats)})
        print(json.dumps({"occupancy": rows[-1]}), flush=True)
        if t_min:
            mse_s, mse_p = float(torch.nn.functional.mse_loss(stopped, dense)), float(torch.nn.functional.mse_loss(stopped, sparse))
            rows.append({"alpha_min": float(alpha_min), "resolution": int(resolution), "t_min": float(t_min),
                         "passes_run": ran, "passes_of_sparse": parent_passes, "passes_over_sparse": ran / max(parent_passes, 1),
                         "psnr_stop_vs_dense": float(mse2psnr(mse_s)) if mse_s > 0. else float("inf"),
                         "psnr_stop_vs_sparse": float(mse2psnr(mse_p)) if mse_p > 0. else float("inf"),
                         "seconds_per_frame_dense": t_dense, "seconds_per_frame_sparse": t_sparse, "seconds_per_frame_stop": t_stop,
                         "frames": len(mats)})
            print(json.dumps({"occupancy_stop": rows[-1]}), flush=True)
    return rows


def sparse_proposal_compare(cfg, nope, pose, loader, field, device, resolution, alpha_mins, dilate=1, bounds=None, frames=4):
    """--sparse-proposal with --occupancy: full frames of the first `frames` training views at their learned poses through the sparse
    hierarchical render (rendering.occupancy with rendering.num_fine and rendering.proposal 'density'), once with the dense proposal
    (rendering.occupancy.proposal absent) and once with the sparse one (true), for every alpha_min -> rows of
    {alpha_min, cells occupied, the share of coarse samples the proposal culled, PSNR of the sparse-proposal frames against the
    dense-proposal frames, seconds per frame of both}.  The culled share is tallied by nnr.ops.propose_sparse itself (propose_sparse_tally)."""
    import model as mdl
    from model import imaging
    from model.common import mse2psnr
    from nnr import ops
    base = nope.renderer
    views = []
    for batch in loader:
        if len(views) >= frames:
            break
        views.append((batch["img.camera_mat"].to(device), batch["img.scale_mat"].to(device), int(batch["img.idx"])))
    with torch.no_grad():
        mats = [(cam, imaging.inverse_pose(pose(i)), scale) for cam, scale, i in views]
    size = (field.H, field.W)

    def frames_of(renderer):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [imaging.render_full_image(renderer, size, cam, world, scale, "nope_nerf", device)[0] for cam, world, scale in mats]
        torch.cuda.synchronize()
        return torch.stack(out), (time.perf_counter() - t0) / len(mats)

    rows = []
    for alpha_min in alpha_mins:
        occ = {"resolution": int(resolution), "alpha_min": float(alpha_min), "dilate": int(dilate)}
        if bounds is not None:
            occ["bounds"] = list(bounds)
        res = {}
        for key in (False, True):
            r = mdl.Renderer(base.model, dict(cfg["rendering"], occupancy=dict(occ, proposal=True) if key else dict(occ)), device=device)
            r.eval()
            frames_of(r)      # (builds the grid; lazy initialisations)
            ops.propose_sparse_tally = [] if key else None
            try:
                res[key] = frames_of(r) + (r.__dict__["_occupancy_hit"][2],)
            finally:
                tally, ops.propose_sparse_tally = ops.propose_sparse_tally, None
        live, total = float(torch.stack([t[0] for t in tally]).sum()), float(sum(t[1] for t in tally))
        mse = float(torch.nn.functional.mse_loss(res[True][0], res[False][0]))
        rows.append({"alpha_min": float(alpha_min), "resolution": int(resolution), "cells_occupied": float(res[True][2].occupied),
                     "coarse_samples_culled": 1. - live / max(total, 1.),
                     "psnr_sparse_proposal_vs_dense_proposal": float(mse2psnr(mse)) if mse > 0. else float("inf"),
                     "seconds_per_frame_dense_proposal": res[False][1], "seconds_per_frame_sparse_proposal": res[True][1], "frames": len(mats)})
        print(json.dumps({"sparse_proposal": rows[-1]}), flush=True)
    return rows


def run(path, scene, style="tanks", epochs=100, seed=42, log_every=10, device=None, eval_epochs=0, eval_dir=None, checkpoint_dir=None,
        occupancy=None, frozen_eval=True, frozen_occupancy=None, t_min=None, sparse_proposal=False, **cfg_kw):
    """-> dict with the per-epoch PSNR / pose-error curve and the loop throughput (+ novel-view scores with eval_epochs > 0)."""
    import dataloading as dl
    from model.common import mse2psnr
    from nnr import parallel
    device = torch.device(device or "cuda")
    sync = torch.cuda.synchronize if device.type == "cuda" else (lambda: None)
    np.random.seed(seed)
    torch.manual_seed(seed)
    cfg = scene_cfg(path, scene, style=style, **cfg_kw)
    if sparse_proposal and not ((occupancy is not None or frozen_occupancy is not None) and num_fine_of(cfg)
                                and cfg["rendering"].get("proposal") == "density"):
        raise ValueError("--sparse-proposal goes with --occupancy or --frozen-occupancy, together with --num-fine and --proposal density")
    loader, fields = dl.get_dataloader(cfg, mode="train", shuffle=True)
    field = fields["img"]
    n_views = field.N_imgs
    trainer, pose, dist = build(cfg, device, n_views)
    gt = field.c2ws.to(device)
    curve = [dict(epoch=-1, psnr=None, **pose_errors(pose, gt, n_views))]
    it, t_loop, steps_timed = -1, 0.0, 0
    for epoch in range(epochs):
        l2, rd = [], []
        sync()
        t0 = time.perf_counter()
        for batch in loader:
            it += 1
            losses = trainer.train_step(batch, it, epoch, 10 ** 6, None)
            l2.append(losses["l2_mean"])
            if "loss_ray_distortion" in losses:
                rd.append(losses["loss_ray_distortion"])
        mse = float(torch.stack(l2).detach().mean())             # the epoch's only device->host sync
        if epoch > 0:                                            # epoch 0 pays the lazy initialisations
            t_loop += time.perf_counter() - t0
            steps_timed += len(l2)
        if epoch % log_every == 0 or epoch == epochs - 1:
            curve.append(dict(epoch=epoch, psnr=float(mse2psnr(mse)), **pose_errors(pose, gt, n_views),
                              **({"ray_distortion": float(torch.stack([torch.as_tensor(v).detach().reshape(()) for v in rd]).mean())} if rd else {})))
            if parallel.rank() == 0:
                print(json.dumps(curve[-1]), flush=True)
    trainer.flush_nan_check()        # the step's NaN check is one step late by design: look at the last one too
    n_rays = cfg["training"]["n_training_points"]
    if checkpoint_dir and parallel.is_writer():
        save_checkpoints(checkpoint_dir, trainer.model, pose, epoch_it=epochs - 1, it=it)
        import yaml
        full = json.loads(json.dumps(cfg))      # plain containers
        full["dataloading"]["path"] = os.path.abspath(path)
        full["training"]["out_dir"] = os.path.abspath(checkpoint_dir)
        with open(os.path.join(checkpoint_dir, "config.yaml"), "w") as fh:
            yaml.safe_dump(full, fh)
    novel = None
    if eval_epochs > 0:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            novel = novel_view_eval(cfg, trainer.model, pose, field, device, eval_epochs, eval_dir or tmp, n_points=min(1024, n_rays),
                                    frozen_field=frozen_eval, frozen_occupancy=frozen_occupancy, sparse_proposal=sparse_proposal)
    occ_rows = None
    if occupancy is not None and sparse_proposal:      # sparse hierarchical frames: the dense proposal against the sparse one
        occ_rows = sparse_proposal_compare(cfg, trainer.model, pose, loader, field, device, occupancy[0], occupancy[1],
                                           bounds=[[-1.5, -1.5, -1.], [1.5, 1.5, 1.]] if style == "llff" else None)
    elif occupancy is not None:      # (resolution, [alpha_min, ...]): dense against sparse evaluation frames
        if num_fine_of(cfg):
            raise ValueError("--occupancy compares plain renders: leave --num-fine off")
        occ_rows = occupancy_compare(cfg, trainer.model, pose, loader, field, device, occupancy[0], occupancy[1],
                                     bounds=[[-1.5, -1.5, -1.], [1.5, 1.5, 1.]] if style == "llff" else None, t_min=t_min)
    return {"novel_views": novel, "occupancy": occ_rows, "scene": scene, "style": style, "views": n_views, "image": [field.H, field.W], "rays_per_step": n_rays,
            "samples_per_ray": cfg["rendering"]["num_points"], "fine_samples_per_ray": cfg["rendering"].get("num_fine", 0), "proposal": cfg["rendering"].get("proposal", "render"), "hidden": cfg["model"]["hidden_dim"], "epochs": epochs,
            "steps": it + 1, "loader": "resident" if cfg["dataloading"]["resident"] else "host(workers=%d)" % cfg["dataloading"]["n_workers"],
            "aux_losses": cfg["training"]["pc_weight"][0] != 0.0, "ray_distortion_weight": cfg["training"].get("ray_distortion_weight", 0.0),
            "steps_per_s": steps_timed / t_loop if t_loop else None, "rays_per_s": steps_timed * n_rays / t_loop if t_loop else None,
            "curve": curve}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("path")
    ap.add_argument("scene")
    ap.add_argument("--style", choices=("tanks", "llff"), default="tanks")
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--factor", type=int, default=None)
    ap.add_argument("--host-loader", action="store_true")
    ap.add_argument("--workers", type=int, default=0, help="DataLoader worker processes of the host loader (reference default: 1)")
    ap.add_argument("--no-aux", action="store_true")
    ap.add_argument("--bf16", action="store_true", help="rendering.mfma_dtype: bf16 (bf16 MFMA products, fp32 accumulation)")
    ap.add_argument("--num-fine", type=int, default=0, help="rendering.num_fine: fine samples per ray drawn from the coarse pass's weights (0 = off)")
    ap.add_argument("--proposal", choices=("render", "density"), default=None,
                    help="rendering.proposal (with --num-fine): 'render' = coarse forward + resampling launch (default), 'density' = the fused proposal kernel")
    ap.add_argument("--occupancy", nargs="+", default=None, metavar=("RES", "ALPHA_MIN"),
                    help="after training: render evaluation frames dense and with rendering.occupancy {resolution: RES, alpha_min: ALPHA_MIN} "
                         "(several ALPHA_MIN: one row each); prints the culled share and the PSNR of the sparse against the dense frames")
    ap.add_argument("--t-min", type=float, default=None, metavar="T",
                    help="with --occupancy: also render with rendering.occupancy.t_min: T (early ray termination); one more row per ALPHA_MIN "
                         "with the passes run over the sparse render's and the PSNR of the stopped against the dense frames")
    ap.add_argument("--sparse-proposal", action="store_true",
                    help="rendering.occupancy.proposal: true (with --occupancy or --frozen-occupancy, --num-fine and --proposal density): the "
                         "proposal skips known-empty coarse samples; prints the share culled and the PSNR against dense-proposal frames")
    ap.add_argument("--ray-distortion", type=float, default=0.0, metavar="W",
                    help="training.ray_distortion_weight: the weight of the ray distortion of the compositing weights (0 = off; e.g. 0.01)")
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--eval-epochs", type=int, default=0, help="test-time pose optimisation epochs before scoring the held-out views")
    ap.add_argument("--no-frozen-eval", action="store_true",
                    help="eval_pose.frozen_field: false -- refine the held-out views' poses on the operator's full training path instead of its frozen-field mode")
    ap.add_argument("--frozen-occupancy", nargs=2, default=None, metavar=("RES", "ALPHA_MIN"),
                    help="eval_pose.occupancy: true -- refine the held-out poses a second time with an occupancy grid {resolution: RES, alpha_min: "
                         "ALPHA_MIN} of the frozen field, built once; prints the path taken, the culled share and both runs' poses and PSNR")
    ap.add_argument("--eval-dir", default=None, help="where the rendered held-out frames go (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--checkpoint-dir", default=None, help="write model.pt, model_pose.pt and config.yaml here after the last epoch (tools/extract_mesh.py takes DIR/config.yaml)")
    a = ap.parse_args()
    if a.occupancy is not None and len(a.occupancy) < 2:
        ap.error("--occupancy RES ALPHA_MIN [ALPHA_MIN ...]")
    occupancy = None if a.occupancy is None else (int(a.occupancy[0]), [float(v) for v in a.occupancy[1:]])
    if a.t_min is not None and (occupancy is None or not 0. < a.t_min < 1.):
        ap.error("--t-min T goes with --occupancy and lies in (0, 1)")
    if a.sparse_proposal and not ((occupancy is not None or a.frozen_occupancy is not None) and a.num_fine > 0 and a.proposal == "density"):
        ap.error("--sparse-proposal goes with --occupancy or --frozen-occupancy, together with --num-fine F and --proposal density")
    if a.sparse_proposal and a.t_min is not None:
        ap.error("--sparse-proposal compares the two proposals: leave --t-min off")
    res = run(a.path, a.scene, style=a.style, epochs=a.epochs, log_every=a.log_every, eval_epochs=a.eval_epochs, eval_dir=a.eval_dir, checkpoint_dir=a.checkpoint_dir, n_rays=a.rays, n_samples=a.samples,
              hidden=a.hidden, resident=not a.host_loader, aux=not a.no_aux, resize_factor=a.factor, workers=a.workers,
              mfma_dtype="bf16" if a.bf16 else "fp32", num_fine=a.num_fine, proposal=a.proposal, occupancy=occupancy,
              ray_distortion=a.ray_distortion, frozen_eval=not a.no_frozen_eval, t_min=a.t_min, sparse_proposal=a.sparse_proposal,
              frozen_occupancy=None if a.frozen_occupancy is None else (int(a.frozen_occupancy[0]), float(a.frozen_occupancy[1])))
    print(json.dumps({k: v for k, v in res.items() if k != "curve"}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
