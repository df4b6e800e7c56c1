"""Write the learned geometry of a trained run as a PLY mesh (model/geometry.py).

    python tools/extract_mesh.py <config.yaml> [--default configs/default.yaml] [--resolution 256] [--lo X Y Z --hi X Y Z]
                                 [--level RAW] [--no-colour] [--slab LAYERS] [--out mesh.ply]
                                 [--refine {2,4,8} [--dilate N] [--max-bricks B]]
                                 [--method tsdf [--every N] [--trunc-voxels T] [--min-acc A]]

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
number of cameras, the time of the depth renders and of the fusion launches between device events, bricks, vertices and peak memory."""
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
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    render_ev, fuse_ev, pairs = ev(), [], [0]

    def depth_maps():
        render_ev[0].record()
        d = G.render_depth_maps(renderer, cams.camera_mat, cams.world_mats, (H, W), min_acc=args.min_acc)
        render_ev[1].record()
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
    print("depth renders: %.3f ms (%.3f ns per sample)" % (ms_r, ms_r * 1e6 / (n_cams * H * W * samples)))
    print("fusion: %d launches, %.3f ms (%.4f ns per voxel-camera pair), truncation %g voxels" % (len(fuse_ev), ms_f, ms_f * 1e6 / max(1, pairs[0]),
                                                                                            args.trunc_voxels))
    print("grid: %d x %d x %d in [%s] .. [%s]%s, %d bricks" % (tuple(mesh.dims) + (", ".join("%g" % v for v in lo), ", ".join("%g" % v for v in hi),
                                                                                  ", refined %d times" % r if r else "", mesh.n_bricks)))
    print("peak device memory: %.1f MB" % (peak / 1e6))
    print("mesh: %d vertices, %d quads = %d triangles -> %s" % (mesh.vertices.shape[0], mesh.quads.shape[0], 2 * mesh.quads.shape[0], out))


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
    args = ap.parse_args()
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
