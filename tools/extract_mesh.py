"""Write the learned geometry of a trained run as a PLY mesh (model/geometry.py).

    python tools/extract_mesh.py <config.yaml> [--default configs/default.yaml] [--resolution 256] [--lo X Y Z --hi X Y Z]
                                 [--level RAW] [--no-colour] [--slab LAYERS] [--out mesh.ply]

The checkpoint is found the way the image-extraction script finds it (vis/render.py of the upstream project, which runs against these
packages): the config layered over the defaults, OfficialStaticNerf + Renderer + get_model, CheckpointIO(training.out_dir).load(
extract_images.model_file, 'model.pt' where the key is absent).  Bounds default to the cube [-radius, radius]^3 of rendering.radius, the
sphere the phong renderer marches in; the level to the phong renderer's occ = 0.5 surface.  Needs a GPU: the density comes from the HIP
grid kernel.  Prints the voxel count, the vertex and face counts and the kernel time (device events around the volume's launches)."""
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
    ap.add_argument("--out", help="default: <training.out_dir>/extraction/mesh_<resolution>.ply")
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


if __name__ == "__main__":
    main()
