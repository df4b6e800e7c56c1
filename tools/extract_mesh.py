"""Write the learned geometry of a trained run as a PLY mesh (model/geometry.py).

    python tools/extract_mesh.py <config.yaml> [--default configs/default.yaml] [--resolution 256] [--lo X Y Z --hi X Y Z]
                                 [--level RAW] [--no-colour] [--slab LAYERS] [--out mesh.ply]
                                 [--refine {2,4,8} [--dilate N] [--max-bricks B]]

The checkpoint is found the way the image-extraction script finds it (vis/render.py of the upstream project, which runs against these
packages): the config layered over the defaults, OfficialStaticNerf + Renderer + get_model, CheckpointIO(training.out_dir).load(
extract_images.model_file, 'model.pt' where the key is absent).  Bounds default to the cube [-radius, radius]^3 of rendering.radius, the
sphere the phong renderer marches in; the level to the phong renderer's occ = 0.5 surface.  Needs a GPU: the density comes from the HIP
grid kernel.  Prints the voxel count, the vertex and face counts and the kernel time (device events around the volume's launches).

--refine R: the mesh of the grid R times finer than --resolution, evaluated only in the 8^3 bricks around the coarse cells the surface
crosses (geometry.extract_mesh_refined: the dense fine mesh restricted to what the coarse pass sees -- a component that crosses no coarse
cell within --dilate cells of a crossing one is absent).  Prints the coarse voxels, the selected cells, the bricks and their share of the
dense fine grid, both kernels' times between device events, and the peak device memory."""
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
