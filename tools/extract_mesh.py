"""Write the learned geometry of a trained run as a PLY mesh (model/geometry.py).

    python tools/extract_mesh.py <config.yaml> [--default configs/default.yaml] [--resolution 256] [--lo X Y Z --hi X Y Z]
                                 [--level RAW] [--no-colour] [--slab LAYERS] [--out mesh.ply]
                                 [--refine {2,4,8} [--dilate N] [--max-bricks B]]
                                 [--method tsdf [--every N] [--trunc-voxels T] [--min-acc A]
                                                [--occupancy RES ALPHA_MIN [--occupancy-dilate N] [--occupancy-bounds LO HI] [--t-min T]]]

The checkpoint is found the way the image-extraction script finds it (vis/render.py of the upstream project, which runs against these
packages): the config layered over the defaults, OfficialStaticNerf + Renderer + get_model, CheckpointIO(training.out_dir).load(
extract_images.model_file, 'model.pt' where the key is absent).  Bounds default to the cube [-radius, radius]^3 of rendering.radius, the
sphere the phong renderer marches in; the level to the phong renderer's occ = 0.5 surface.  Needs a GPU: the density comes from the HIP
grid kernel.  Prints the voxel count, the vertex and face counts and the kernel time (device events around the volume's launches).

--refine R: the mesh of the grid R times finer than --resolution, evaluated only in the 8^3 bricks around the coarse cells the surface
crosses (geometry.extract_mesh_refined: the dense fine mesh restricted to what the coarse pass sees -- a component that crosses no coarse
cell within --dilate cells of a crossing one is absent).  Prints the coarse voxels, the selected cells, the bricks and their share of the
dense fine grid, both kernels' times between device events, and the peak device memory.

--method tsdf (default: density, everything above): the zero set of the truncated signed distance volume fused from the model's rendered
depth maps (geometry.extract_mesh_tsdf), seen from every --every'th frame of the training split at the learned
poses of model_pose.pt (and the learned focal of model_focal.pt where pose.learn_focal is set), the way the image-extraction scripts build
their cameras.  --resolution, --refine, --dilate, --max-bricks, --lo / --hi and --no-colour apply; --level and --slab do not.  Prints the
number of cameras, the time of the depth renders and of the fusion launches between device events, bricks, vertices and peak memory.

--occupancy RES ALPHA_MIN (with --method tsdf): the depth maps come from the sparse depth kernel
(geometry.render_depth_maps(occupancy=grid, t_min=T): nnr.ops.render_depth_sparse).  The flags become rendering.occupancy {resolution,
alpha_min, dilate, bounds} and the grid is built once with renderer.frozen_occupancy_grid: the checkpoint is a frozen field, this tool owns
the grid.  --t-min T (0 < T < 1, with --occupancy): a workgroup of four rays stops once each is below that transmittance.  No default
alpha_min or t_min is shipped.  For the first fused frame the tool prints the grid's occupied share, the mean share of live samples and
of passes run, the largest and median |depth_sparse - depth_dense| over the pixels finite in both and the number of pixels whose +inf
status differs: one extra dense frame."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nope-nerf_amd"))


def load_renderer(config, default, device):
    import model as mdl
    from dataloading import load_config
    cfg = load_config(config, default if default and os.path.isfile(default) else None)
    net = mdl.OfficialStaticNerf(cfg)
    renderer = mdl.Renderer(net, cfg['rendering'], device=device)
    nope = mdl.get_model(renderer, cfg, device=device)
    out_dir = cfg['training']['out_dir']
    scalars = mdl.CheckpointIO(out_dir, model=nope).load(cfg.get('extract_images', {}).get('model_file', 'model.pt'))
    return renderer, cfg, scalars


def load_pose_table(out_dir, n_views, cfg, device, init_c2w=None):
    """The learned poses of model_pose.pt (CheckpointIO, registered as 'model': train.py's and tools/train_scene.py's layout) -> LearnPose"""
    import model as mdl
    p = cfg.get('pose', {})
    pose = mdl.LearnPose(n_views, bool(p.get('learn_R', True)), bool(p.get('learn_t', True)), cfg, init_c2w=init_c2w).to(device)
    mdl.CheckpointIO(out_dir, model=pose).load('model_pose.pt')
    return pose


def load_cameras(cfg, device, every=1):
    """The training split's frames as geometry.Cameras at the learned poses (and the learned focal where the config learns one)"""
    import dataloading as dl
    import model as mdl
    from model import geometry as G
    from model import imaging
    _, fields = dl.get_dataloader(cfg, mode="train", shuffle=False)
    f = fields["img"]
    out_dir = cfg['training']['out_dir']
    init = f.c2ws.to(device) if cfg.get('pose', {}).get('init_pose', False) else None
    pose = load_pose_table(out_dir, f.N_imgs, cfg, device, init_c2w=init)
    K = torch.as_tensor(f.K, dtype=torch.float32).reshape(4, 4).to(device)
    if cfg.get('pose', {}).get('learn_focal', False):
        focal = mdl.LearnFocal(True, bool(cfg['pose'].get('fx_only', False)), order=int(cfg['pose'].get('focal_order', 2))).to(device)
        mdl.CheckpointIO(out_dir, model=focal).load('model_focal.pt')
        with torch.no_grad():
            K = imaging.camera_from_focal(focal(0), device)[0]
    with torch.no_grad():
        world = torch.cat([imaging.inverse_pose(pose(i)) for i in range(0, f.N_imgs, max(1, int(every)))])
    return G.Cameras(K, world, (int(f.H), int(f.W)))


def tsdf(args, G, renderer, cfg, scalars, lo, hi):
    """--method tsdf: extract_mesh_tsdf with the depth renders and the fusion launches wrapped in device events (its hooks)"""
    from nnr import ops
    device = torch.device("cuda")
    cams = load_cameras(cfg, device, args.every)
    n_cams, (H, W) = cams.world_mats.shape[0], cams.size
    G.render_depth_maps(renderer, cams.camera_mat, cams.world_mats[:1], (2, 2))      # loads the code object, packs the weights
    grid, t_min = None, 0. if args.t_min is None else args.t_min
    median = args.depth_mode == "median"      # the maps stop at the level (render_depth_maps' default with a grid); --t-min is the expected mode's
    maps = {}
    if args.occupancy is not None:
        occ = {"resolution": int(args.occupancy[0]), "alpha_min": float(args.occupancy[1]), "dilate": args.occupancy_dilate}
        if args.occupancy_bounds is not None:
            occ["bounds"] = [float(v) for v in args.occupancy_bounds]
        cfg['rendering']['occupancy'] = renderer.cfg['occupancy'] = occ
        grid = renderer.frozen_occupancy_grid(device)      # built once: the checkpoint is a frozen field, the grid is this tool's
        if grid is None:
            sys.exit("extract_mesh: rendering.occupancy %r gives no grid for this config (see the logged reason)" % (occ,))
        first = occupancy_report(G, ops, renderer, cams, grid, t_min, args.min_acc)
        if median:
            first_median = median_passes_report(G, ops, renderer, cams, grid, args.min_acc)
    torch.cuda.synchronize()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    render_ev, fuse_ev, pairs = ev(), [], [0]

    def depth_maps():
        render_ev[0].record()
        if median:
            d = G.render_depth_maps(renderer, cams.camera_mat, cams.world_mats, (H, W), min_acc=args.min_acc, occupancy=grid, depth_mode="median")
        else:
            d = G.render_depth_maps(renderer, cams.camera_mat, cams.world_mats, (H, W), min_acc=args.min_acc, occupancy=grid, t_min=t_min)
        render_ev[1].record()
        maps["depth"] = d
        return d

    def integrate(o, s, br, cm, dp, tr, sm, wt):
        fuse_ev.append(ev())
        fuse_ev[-1][0].record()
        ops.tsdf_integrate(o, s, br, cm, dp, tr, sm, wt)
        fuse_ev[-1][1].record()
        pairs[0] += 512 * br.shape[0] * cm.shape[0]

    n, r = args.resolution, args.refine
    mesh = G.extract_mesh_tsdf(renderer, cams, lo, hi, n, refine=r, trunc_voxels=args.trunc_voxels, dilate=args.dilate,
                               colour=not args.no_colour, integrate=integrate, depth_maps=depth_maps, max_bricks=args.max_bricks)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    out = args.out or os.path.join(cfg['training']['out_dir'], "extraction", "mesh_tsdf_%d%s.ply" % (n, "x%d" % r if r else ""))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    G.write_ply(out, mesh)
    samples = int(cfg['rendering']['num_points']) - int(cfg['rendering']['outside_steps'])
    ms_r = render_ev[0].elapsed_time(render_ev[1])
    ms_f = sum(a.elapsed_time(b) for a, b in fuse_ev)
    print("checkpoint: it %s" % scalars.get('it', '?'))
    print("cameras: %d of %d x %d (every %d), %d samples per ray, min acc %g" % (n_cams, H, W, args.every, samples, args.min_acc))
    print("depth renders: %.3f ms (%.3f ns per sample)%s" % (ms_r, ms_r * 1e6 / (n_cams * H * W * samples),
                                                           "" if grid is None else ", sparse depth kernel, t_min %g"
                                                           % (G.median_level(args.min_acc) if median else t_min)))
    if median:
        print("depth mode: median (level %g), %.4f %% of the pixels finite" % (G.median_level(args.min_acc),
                                                                            100. * float(torch.isfinite(maps["depth"]).float().mean())))
    if grid is not None:
        print("occupancy: %s, first frame: %s" % (occ, first))
        if median:
            print("median mode, first frame: %s; expected mode at t_min %g: %s passes" % (first_median, t_min, first.get("passes_run")))
    print("fusion: %d launches, %.3f ms (%.4f ns per voxel-camera pair), truncation %g voxels" % (len(fuse_ev), ms_f, ms_f * 1e6 / max(1, pairs[0]),
                                                                                            args.trunc_voxels))
    print("grid: %d x %d x %d in [%s] .. [%s]%s, %d bricks" % (tuple(mesh.dims) + (", ".join("%g" % v for v in lo), ", ".join("%g" % v for v in hi),
                                                                                  ", refined %d times" % r if r else "", mesh.n_bricks)))
    print("peak device memory: %.1f MB" % (peak / 1e6))
    print("mesh: %d vertices, %d quads = %d triangles -> %s" % (mesh.vertices.shape[0], mesh.quads.shape[0], 2 * mesh.quads.shape[0], out))


def check_occupancy_args(ap, args):
    """--occupancy and its companions go with --method tsdf, the companions with --occupancy; no GPU is needed to say so"""
    given = [n for n, v in (("--occupancy", args.occupancy), ("--occupancy-dilate", args.occupancy_dilate),
                            ("--occupancy-bounds", args.occupancy_bounds), ("--t-min", args.t_min)) if v is not None]
    if given and args.method != "tsdf":
        ap.error("%s: with --method tsdf only" % ", ".join(given))
    if given and args.occupancy is None:
        ap.error("%s: with --occupancy RES ALPHA_MIN only" % ", ".join(given))
    if args.occupancy is not None:
        try:
            ok = int(args.occupancy[0]) >= 1 and float(args.occupancy[1]) == float(args.occupancy[1])
        except ValueError:
            ok = False
        if not ok:
            ap.error("--occupancy RES ALPHA_MIN: a cell count and an alpha")
        if args.occupancy_dilate is None:
            args.occupancy_dilate = 1
        if args.occupancy_dilate < 0:
            ap.error("--occupancy-dilate N: a cell count >= 0")
    if args.t_min is not None and not 0. < args.t_min < 1.:
        ap.error("--t-min T lies in (0, 1)")
    if args.depth_mode != "expected" and args.method != "tsdf":
        ap.error("--depth-mode: with --method tsdf only")
    if args.depth_mode == "median" and not 0. < args.min_acc < 1.:
        ap.error("--depth-mode median: --min-acc lies in (0, 1), the quantile of the ray's weight")


def median_passes_report(G, ops, renderer, cams, grid, min_acc):
    """The first fused frame in median mode, stopped at its level -> the mean passes a ray's workgroup ran"""
    ops.depth_sparse_tally = []
    try:
        G.render_depth_maps(renderer, cams.camera_mat, cams.world_mats[:1], cams.size, min_acc=min_acc, occupancy=grid, depth_mode="median")
        tally = ops.depth_sparse_tally
    finally:
        ops.depth_sparse_tally = None
    res = {"t_min": G.median_level(min_acc)}
    if tally:      # (none above 256 samples per ray: the dense render ran)
        res["passes_run"] = round(sum(float(t[1]) for t in tally) / sum(t[3] for t in tally), 4)
    return res


def occupancy_report(G, ops, renderer, cams, grid, t_min, min_acc):
    """The first fused frame through the sparse depth kernel and once dense -> what --occupancy prints about it"""
    samples = int(renderer.cfg['num_points']) - int(renderer.cfg['outside_steps'])
    ops.depth_sparse_tally = []
    try:
        sparse = G.render_depth_maps(renderer, cams.camera_mat, cams.world_mats[:1], cams.size, min_acc=min_acc, occupancy=grid, t_min=t_min)
        tally = ops.depth_sparse_tally
    finally:
        ops.depth_sparse_tally = None
    dense = G.render_depth_maps(renderer, cams.camera_mat, cams.world_mats[:1], cams.size, min_acc=min_acc)
    res = {"cells_occupied": round(float(grid.occupied), 6)}
    if tally:      # (none above 256 samples per ray: the dense render ran)
        live, passes = sum(float(t[0]) for t in tally), sum(float(t[1]) for t in tally)
        total, rays = sum(t[2] for t in tally), sum(t[3] for t in tally)
        res.update(samples_live=round(live / total, 6), passes_run=round(passes / rays, 4), passes_full=(samples + 31) // 32)
    both = torch.isfinite(sparse) & torch.isfinite(dense)
    diff = (sparse - dense)[both].abs()
    res.update(depth_diff_max=float(diff.max()) if diff.numel() else None, depth_diff_median=float(diff.median()) if diff.numel() else None,
               inf_status_differs=int((torch.isinf(sparse) != torch.isinf(dense)).sum()), pixels=int(sparse.numel()))
    return res


def main():
    ap = argparse.ArgumentParser(description="Extract a surface-nets mesh of the learned density as a PLY file.")
    ap.add_argument("config")
    ap.add_argument("--default", default="configs/default.yaml", help="defaults the config is layered over (skipped if the file is absent)")
    ap.add_argument("--resolution", type=int, default=256, help="grid points per axis")
    ap.add_argument("--lo", type=float, nargs=3)
    ap.add_argument("--hi", type=float, nargs=3)
    ap.add_argument("--level", type=float, help="raw-density level (default: the phong renderer's occ = 0.5 surface)")
    ap.add_argument("--no-colour", action="store_true")
    ap.add_argument("--slab", type=int, help="most z-layers per kernel launch (default: the whole volume in one)")
    ap.add_argument("--refine", type=int, choices=(2, 4, 8), help="refine the mesh this many times in sparse bricks (default: the dense path)")
    ap.add_argument("--dilate", type=int, default=1, help="with --refine: coarse cells around a crossing one that are refined too")
    ap.add_argument("--max-bricks", type=int, help="with --refine: stop if more bricks than this are selected")
    ap.add_argument("--out", help="default: <training.out_dir>/extraction/mesh_<resolution>[x<refine>].ply")
    ap.add_argument("--method", choices=("density", "tsdf"), default="density",
                    help="density: a level set of the raw density (default); tsdf: the rendered depth maps of the learned cameras, fused")
    ap.add_argument("--every", type=int, default=1, help="with --method tsdf: fuse every N'th training frame")
    ap.add_argument("--trunc-voxels", type=float, default=3., help="with --method tsdf: the truncation distance in grid steps")
    ap.add_argument("--min-acc", type=float, default=0.5, help="with --method tsdf: a pixel whose accumulated weight is below this saw free space")
    ap.add_argument("--occupancy", nargs=2, default=None, metavar=("RES", "ALPHA_MIN"),
                    help="with --method tsdf: render the depth maps through the sparse depth kernel with an occupancy grid of RES cells per "
                         "axis, a cell empty where the alpha at the coarse sample spacing stays below ALPHA_MIN (rendering.occupancy)")
    ap.add_argument("--occupancy-dilate", type=int, default=None, metavar="N", help="with --occupancy: cells kept around an occupied one (default 1)")
    ap.add_argument("--occupancy-bounds", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="with --occupancy: the grid's box on every axis (default: the cube of rendering.radius)")
    ap.add_argument("--t-min", type=float, default=None, metavar="T",
                    help="with --occupancy: stop a workgroup of four rays once each is below this transmittance, 0 < T < 1")
    ap.add_argument("--depth-mode", choices=("expected", "median"), default="expected",
                    help="with --method tsdf: fuse the expected depth sum w z (default) or the depth at which a ray's accumulated weight "
                         "reaches --min-acc (the median at 0.5); with --occupancy the median maps stop at that level, --t-min is then the "
                         "expected mode's in the report")
    args = ap.parse_args()
    check_occupancy_args(ap, args)
    if not torch.cuda.is_available():
        sys.exit("extract_mesh: needs a GPU (the density volume comes from the HIP grid kernel; there is no CPU volume path)")
    from model import geometry as G
    device = torch.device("cuda")
    renderer, cfg, scalars = load_renderer(args.config, args.default, device)
    rad = float(cfg['rendering']['radius'])
    lo = tuple(args.lo) if args.lo else (-rad,) * 3
    hi = tuple(args.hi) if args.hi else (rad,) * 3
    n = args.resolution
    renderer.model.eval()
    if args.method == "tsdf":
        return tsdf(args, G, renderer, cfg, scalars, lo, hi)
    if args.refine:
        return refined(args, G, renderer, cfg, scalars, lo, hi)
    # the kernel time on its own: a 2^3 grid first (loads the code object, packs the weights), then the volume between device events
    G.density_volume(renderer, lo, hi, 2)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    volume = G.density_volume(renderer, lo, hi, n, slab=args.slab)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    mesh = G.extract_mesh(renderer, lo, hi, n, level=args.level, colour=not args.no_colour, volume=volume)
    out = args.out or os.path.join(cfg['training']['out_dir'], "extraction", "mesh_%d.ply" % n)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    G.write_ply(out, mesh)
    print("checkpoint: it %s" % scalars.get('it', '?'))
    print("volume: %d^3 = %d voxels in [%s] .. [%s], level %.6g" % (n, n ** 3, ", ".join("%g" % v for v in lo), ", ".join("%g" % v for v in hi),
                                                                   mesh.level))
    print("grid kernel: %.3f ms (%.3f ns per voxel)" % (ms, ms * 1e6 / n ** 3))
    print("mesh: %d vertices, %d quads = %d triangles -> %s" % (mesh.vertices.shape[0], mesh.quads.shape[0], 2 * mesh.quads.shape[0], out))


def refined(args, G, renderer, cfg, scalars, lo, hi):
    """--refine: extract_mesh_refined with the two kernels wrapped in device events (its `density=` hooks)"""
    from nnr import ops
    net = renderer.model
    w, b, n, r = net.weights(), net.biases(), args.resolution, args.refine
    G.density_volume(renderer, lo, hi, 2)      # loads the code object, packs the weights
    ops.density_bricks((0., 0., 0.), (1., 1., 1.), torch.zeros(1, 3, dtype=torch.int32, device=w[0].device), w, b, hidden=net.hidden_dim)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    events, seen = {}, {}

    def timed(name, fn):
        def call(*a):
            events[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            events[name][0].record()
            out = fn(*a)
            events[name][1].record()
            seen[name] = out
            return out
        return call

    density = (timed("grid", lambda o, s, d: ops.density_grid(o, s, d, w, b, hidden=net.hidden_dim)),
               timed("bricks", lambda o, s, br: ops.density_bricks(o, s, br, w, b, hidden=net.hidden_dim)))
    mesh = G.extract_mesh_refined(renderer, lo, hi, n, r, level=args.level, dilate=args.dilate, colour=not args.no_colour,
                                  max_bricks=args.max_bricks, density=density)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    out = args.out or os.path.join(cfg['training']['out_dir'], "extraction", "mesh_%dx%d.ply" % (n, r))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    G.write_ply(out, mesh)
    selected = int(G.select_cells(seen["grid"], mesh.level, args.dilate).sum())
    fine = mesh.dims[0] * mesh.dims[1] * mesh.dims[2]
    print("checkpoint: it %s" % scalars.get('it', '?'))
    print("coarse volume: %d^3 = %d voxels in [%s] .. [%s], level %.6g" % (n, n ** 3, ", ".join("%g" % v for v in lo),
                                                                            ", ".join("%g" % v for v in hi), mesh.level))
    print("selected: %d of %d coarse cells (dilate %d)" % (selected, (n - 1) ** 3, args.dilate))
    print("bricks: %d = %d voxels, %.4f %% of the dense fine grid %d x %d x %d" % ((mesh.n_bricks, 512 * mesh.n_bricks,
                                                                                   100. * 512 * mesh.n_bricks / fine) + tuple(mesh.dims)))
    ms = events["grid"][0].elapsed_time(events["grid"][1])
    print("grid kernel: %.3f ms (%.3f ns per voxel)" % (ms, ms * 1e6 / n ** 3))
    if "bricks" in events:
        ms = events["bricks"][0].elapsed_time(events["bricks"][1])
        print("brick kernel: %.3f ms (%.3f ns per voxel)" % (ms, ms * 1e6 / (512 * mesh.n_bricks)))
    print("peak device memory: %.1f MB" % (peak / 1e6))
    print("mesh: %d vertices, %d quads = %d triangles -> %s" % (mesh.vertices.shape[0], mesh.quads.shape[0], 2 * mesh.quads.shape[0], out))


if __name__ == "__main__":
    main()
