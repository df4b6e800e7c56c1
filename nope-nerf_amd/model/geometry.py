"""Geometry export: the learned density as a volume, a surface-nets mesh of one of its level sets, and a PLY file.

    density_volume   the raw density on a regular grid, in z-slabs of one launch of the fused grid kernel each (nnr.ops.density_grid)
    level_for        the raw-density value of the phong renderer's occ = tau surface
    surface_nets     volume -> (vertices, quads), plain torch, CPU or GPU tensors
    extract_mesh     volume -> surface nets -> normals (nnr.ops.density_grad) -> colours (nnr.ops.mlp_points); GPU only
    extract_mesh_refined   a coarse volume -> the 8^3 bricks of a 2, 4 or 8 times finer grid around the coarse cells the surface crosses
                     (refined_grid, select_cells, bricks_for; nnr.ops.density_bricks) -> surface nets on those bricks alone
                     (sparse_surface_nets) -> normals and colours in chunks: the dense fine mesh restricted to what the coarse pass sees
    extract_mesh_tsdf      the rendered depth maps of known cameras (render_depth_maps: nnr.ops.render_depth) fused into a truncated signed
                     distance volume in bricks (nnr.ops.tsdf_integrate; projection_rows, tsdf_volume, tsdf_select_cells) -> surface nets of its
                     zero set, dense or refined: no density level, surface only where some camera saw one
    write_ply / read_ply
    occupancy_bits / OccupancyGrid / occupancy_grid / level_for_alpha   the volume as a bitfield of cells that may hold matter, for the sparse
                     inference render (nnr.ops.render_sparse)

Grid conventions, shared with the kernel: a volume is (nz, ny, nx), x fastest; grid point (ix, iy, iz) sits at origin + step * (ix, iy, iz)
(fp32: the product rounded, then the sum).  There is no CPU volume path: the density comes from the HIP kernel or not at all."""
import logging
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from nnr import ops as _nnr_ops


# ----------------------------------------------------------------------------------------------------------------------
# the volume
# ----------------------------------------------------------------------------------------------------------------------
def _resolution3(resolution):
    r = (resolution,) * 3 if isinstance(resolution, int) else tuple(int(v) for v in resolution)
    if len(r) != 3 or min(r) < 2:
        raise ValueError("resolution: one int or (nx, ny, nz), every axis >= 2 grid points; got %r" % (resolution,))
    return r


def grid_of(lo, hi, resolution):
    """(origin, step, dims) of the grid with `resolution` points per axis whose first point is `lo` and whose last is `hi` up to rounding:
    step = (hi - lo) / (n - 1), rounded to fp32 once -- the grid is DEFINED by the fp32 origin and step, as the kernel sees them."""
    dims = _resolution3(resolution)
    origin = [float(np.float32(v)) for v in lo]
    step = [float(np.float32((float(h) - float(l)) / (n - 1))) for l, h, n in zip(lo, hi, dims)]
    return origin, step, dims


def density_volume(renderer, lo, hi, resolution, slab=None):
    """The raw density (before softplus / relu) of renderer.model on the grid grid_of(lo, hi, resolution) -> (nz, ny, nx) fp32 on the
    model's device.  slab: the most z-layers per kernel launch (None: the whole volume in one launch), which bounds what a launch writes.
    The slabbed result equals the one-call result bit for bit: a launch that starts at layer iz0 keeps the volume's step and takes
    origin_z = fl(lo_z + fl(step_z * iz0)), the z the kernel forms for that layer in the one-call run, and covers only layers for which
    its own fl(origin_z + fl(step_z * j)) is that run's fl(lo_z + fl(step_z * (iz0 + j))) -- checked on the host in fp32 (_slab_origins)."""
    net = renderer.model
    origin, step, dims = grid_of(lo, hi, resolution)
    nx, ny, nz = dims
    w, b = net.weights(), net.biases()
    if slab is None or slab >= nz:
        return _nnr_ops.density_grid(origin, step, dims, w, b, hidden=net.hidden_dim)
    if slab < 1:
        raise ValueError("slab: at least one z-layer per launch")
    out = torch.empty(nz, ny, nx, dtype=torch.float32, device=w[0].device)
    for iz0, n, oz in _slab_origins(origin[2], step[2], nz, int(slab)):
        out[iz0:iz0 + n] = _nnr_ops.density_grid([origin[0], origin[1], oz], step, (nx, ny, n), w, b, hidden=net.hidden_dim)
    return out


def _layer_z(oz, sz, i):
    """the kernel's z of layer i: fl(oz + fl(sz * (float) i)) in fp32"""
    return np.float32(oz) + np.float32(sz) * np.float32(i)


def _slab_origins(oz, sz, nz, slab):
    """Cut layers [0, nz) into runs (iz0, n, origin_z) of at most `slab` layers such that a launch with origin_z and the volume's step forms
    for its layer j exactly the one-call run's z of layer iz0 + j.  origin_z = fl(oz + fl(sz * iz0)) makes j = 0 exact by construction; the
    other layers of the run are checked here on the host in the same fp32 arithmetic, and a run is cut short at the first layer where the
    two roundings part (the next run then starts there, exact again).  With a step and an origin that are dyadic over the slab nothing is
    ever cut; in general a few runs come out shorter than `slab`, none longer."""
    runs, iz0 = [], 0
    with np.errstate(over='ignore'):
        while iz0 < nz:
            o = _layer_z(oz, sz, iz0)
            n = 1
            while n < slab and iz0 + n < nz and _layer_z(o, sz, n) == _layer_z(oz, sz, iz0 + n):
                n += 1
            runs.append((iz0, n, float(o)))
            iz0 += n
    return runs


def level_for(rendering_cfg, occ_activation, tau=0.5):
    """The raw-density value at which the phong renderer's occupancy equals tau (its surface is occ = 0.5, model/rendering.py:
    ray_marching).  OfficialStaticNerf's occupancy is occ = s(raw) with rendering.dist_alpha and 1 - exp(-s(raw)) without, s = softplus
    (model.occ_activation: 'softplus') or relu; all four are non-decreasing in raw, so {occ > tau} = {raw > level}:

        softplus               1 - exp(-softplus(raw)) = tau   ->   raw = log(tau / (1 - tau))      (0 at tau = 0.5)
        softplus + dist_alpha  softplus(raw) = tau             ->   raw = log(exp(tau) - 1)
        relu                   1 - exp(-relu(raw)) = tau       ->   raw = -log(1 - tau)
        relu + dist_alpha      relu(raw) = tau                 ->   raw = tau

    0 < tau (< 1 without dist_alpha)."""
    tau = float(tau)
    dist_alpha = bool(rendering_cfg['dist_alpha'])
    if not tau > 0. or (not dist_alpha and not tau < 1.):
        raise ValueError("tau = %r is not an occupancy the field can cross" % tau)
    if occ_activation == 'softplus':
        return math.log(math.expm1(tau)) if dist_alpha else math.log(tau / (1. - tau))
    return tau if dist_alpha else -math.log1p(-tau)


# ----------------------------------------------------------------------------------------------------------------------
# surface nets
# ----------------------------------------------------------------------------------------------------------------------
_CORNERS = [(k & 1, (k >> 1) & 1, (k >> 2) & 1) for k in range(8)]                              # corner k of a cell: (dx, dy, dz)
_EDGES = [(a, a | bit) for bit in (1, 2, 4) for a in range(8) if not a & bit]                  # its 12 edges as corner pairs


def _cell_vertices(val, cell, level, o, s):
    """The vertices of active cells, one row per cell: val (V,8) float64, the corner values in _CORNERS order; cell (V,3) int64, (cx, cy, cz);
    o, s the grid's origin and step as float64 tensors -> (V,3) float32.  The arithmetic of surface_nets and sparse_surface_nets, row by row:
    a cell's vertex depends on its own row alone, so the two agree bit for bit on a cell they both hold."""
    V, dev = val.shape[0], val.device
    side = val > level
    off = torch.tensor(_CORNERS, dtype=torch.float64, device=dev)
    acc = torch.zeros(V, 3, dtype=torch.float64, device=dev)
    cnt = torch.zeros(V, dtype=torch.float64, device=dev)
    for a, b in _EDGES:
        cross = side[:, a] != side[:, b]
        t = torch.where(cross, (level - val[:, a]) / torch.where(cross, val[:, b] - val[:, a], torch.ones_like(cnt)), torch.zeros_like(cnt))
        t = t.clamp(0., 1.)                                    # (an infinite corner value: the crossing at the finite end)
        t = torch.where(torch.isnan(t), torch.full_like(t, 0.5), t)      # (both ends infinite)
        acc += torch.where(cross.unsqueeze(1), off[a] + t.unsqueeze(1) * (off[b] - off[a]), torch.zeros_like(acc))
        cnt += cross
    local = acc / cnt.unsqueeze(1)
    return (o + s * (cell.to(torch.float64) + local)).to(torch.float32)


def surface_nets(volume, level, origin, step):
    """Naive surface nets of {volume = level}: volume (nz, ny, nx) (any float dtype, CPU or GPU), grid point (ix, iy, iz) at
    origin + step * (ix, iy, iz) -> (vertices (V,3) float32, quads (Q,4) int64) on the volume's device.  A corner is `inside` where
    volume > level.
      * one vertex per cell (8 neighbouring grid points) whose corners are not all on one side: the mean of the linearly interpolated
        crossings on those of its 12 edges whose ends differ -- so it lies in the cell;
      * one quad per grid edge whose ends differ and whose four neighbouring cells are inside the volume (edges on the volume's boundary
        make none: the mesh of a surface that leaves the volume is open there), joining those cells' vertices; its normal (right-hand rule
        over the corner order) points from the inside end to the outside end, whatever the signs of the steps;
      * a cell with a NaN corner makes no vertex and no quad touches it.
    No case table, no ambiguity handling: where a cell's corners alternate the mesh may be non-manifold, as surface nets are.
    Deterministic: vertices in cell order (z, y, x: x fastest), quads by edge direction (x, y, z) and then in grid order of the edge.
    The arithmetic is float64 whatever the input's dtype."""
    vol = volume.detach().to(torch.float64)
    dev = vol.device
    nz, ny, nx = vol.shape
    none = (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 4, dtype=torch.int64, device=dev))
    if min(nz, ny, nx) < 2:
        return none
    level = float(level)
    ins = vol > level
    nan = torch.isnan(vol)

    def cells(t, dx, dy, dz):       # the corner (dx, dy, dz) of every cell
        return t[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]

    n_in = sum(cells(ins, *c).to(torch.uint8) for c in _CORNERS)
    bad = cells(nan, *_CORNERS[0])
    for c in _CORNERS[1:]:
        bad = bad | cells(nan, *c)
    active = (n_in > 0) & (n_in < 8) & ~bad
    cell = active.nonzero()                                    # (V,3): (cz, cy, cx), in cell order
    V = cell.shape[0]
    if V == 0:
        return none
    cz, cy, cx = cell.unbind(1)
    val = torch.stack([vol[cz + dz, cy + dy, cx + dx] for dx, dy, dz in _CORNERS], 1)      # (V,8)
    o = torch.tensor([float(v) for v in origin], dtype=torch.float64, device=dev)
    s = torch.tensor([float(v) for v in step], dtype=torch.float64, device=dev)
    vertices = _cell_vertices(val, cell.flip(1), level, o, s)

    vid = torch.full((nz - 1, ny - 1, nx - 1), -1, dtype=torch.int64, device=dev)
    vid[cz, cy, cx] = torch.arange(V, dtype=torch.int64, device=dev)
    flip_all = (s[0] * s[1] * s[2]).item() < 0       # an odd number of negative steps mirrors the grid: the index-space winding is reversed
    quads = []
    # per direction: the edges with four cells around them, and those cells in right-hand order about the edge's +direction
    # (x: y then z; y: z then x; z: x then y) -- (-,-), (+,-), (+,+), (-,+)
    for axis in (0, 1, 2):
        if axis == 0:       # edge (z, y, x)-(z, y, x+1), 1 <= z <= nz-2, 1 <= y <= ny-2
            a, b = ins[1:nz - 1, 1:ny - 1, :-1], ins[1:nz - 1, 1:ny - 1, 1:]
            ring = ((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0))           # (dz, dy, dx) into vid
        elif axis == 1:     # edge (z, y, x)-(z, y+1, x), 1 <= z <= nz-2, 1 <= x <= nx-2
            a, b = ins[1:nz - 1, :-1, 1:nx - 1], ins[1:nz - 1, 1:, 1:nx - 1]
            ring = ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1))
        else:               # edge (z, y, x)-(z+1, y, x), 1 <= y <= ny-2, 1 <= x <= nx-2
            a, b = ins[:-1, 1:ny - 1, 1:nx - 1], ins[1:, 1:ny - 1, 1:nx - 1]
            ring = ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0))
        e = (a != b).nonzero()
        if e.shape[0] == 0:
            continue
        i, j, k = e.unbind(1)
        q = torch.stack([vid[i + dz, j + dy, k + dx] for dz, dy, dx in ring], 1)
        rev = ~a[i, j, k]                                      # the inside end is the far one: the normal points down the axis
        if flip_all:
            rev = ~rev
        q = torch.where(rev.unsqueeze(1), q[:, [0, 3, 2, 1]], q)
        quads.append(q[(q >= 0).all(1)])                       # a NaN reads as outside: such an edge's cells have no vertex
    quads = torch.cat(quads) if quads else none[1]
    return vertices, quads


# ----------------------------------------------------------------------------------------------------------------------
# the mesh
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Mesh:
    vertices: torch.Tensor                       # (V,3) float32
    quads: torch.Tensor                          # (Q,4) int64, normal by the right-hand rule from inside to outside
    normals: Optional[torch.Tensor] = None       # (V,3) float32, unit, -grad(raw) / |grad(raw)| (NaN where the gradient vanishes)
    colours: Optional[torch.Tensor] = None       # (V,3) float32 in [0,1]: the colour branch seen along -normal
    level: float = 0.
    origin: tuple = (0., 0., 0.)
    step: tuple = (1., 1., 1.)
    dims: tuple = (0, 0, 0)
    refine: int = 1                              # extract_mesh_refined: origin, step and dims are the FINE grid's, `refine` times the coarse one
    n_bricks: int = 0                            # ... and the 8^3 bricks of it that were evaluated

    def triangles(self):
        """(2Q,3): every quad (a, b, c, d) split along its a-c diagonal into (a, b, c), (a, c, d), the quad's winding kept"""
        q = self.quads
        return torch.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3)


def extract_mesh(renderer, lo, hi, resolution, level=None, colour=True, slab=None, volume=None):
    """The surface {raw density = level} of renderer.model inside the box [lo, hi] as a Mesh: density_volume -> surface_nets -> unit normals
    -grad(raw) / |grad(raw)| at the vertices (nnr.ops.density_grad: the phong renderer's normals) -> vertex colours, the colour branch at
    the vertex seen from outside along the normal (nnr.ops.mlp_points(v, view = -normal, split2=True), as the phong renderer's rgb_surf
    with view = -ray).  level None: the phong renderer's surface, level_for(renderer.cfg, model.occ_activation).  volume: the result of
    density_volume(renderer, lo, hi, resolution) where the caller has it already (None: computed here).  GPU only."""
    net = renderer.model
    w, b = net.weights(), net.biases()
    if not w[0].is_cuda:
        raise NotImplementedError("extract_mesh runs only on the GPU (HIP grid kernel, nnr_grid_f16.hip); there is no CPU volume path")
    if level is None:
        level = level_for(renderer.cfg, net.occ_activation)
    origin, step, dims = grid_of(lo, hi, resolution)
    with torch.no_grad():
        vol = density_volume(renderer, lo, hi, resolution, slab=slab) if volume is None else volume
        if tuple(vol.shape) != tuple(dims[::-1]):
            raise ValueError("volume: shape %r is not the grid's (nz, ny, nx) = %r" % (tuple(vol.shape), tuple(dims[::-1])))
        vertices, quads = surface_nets(vol, level, origin, step)
        mesh = Mesh(vertices, quads, level=float(level), origin=tuple(origin), step=tuple(step), dims=tuple(dims))
        if vertices.shape[0] == 0:
            mesh.normals = torch.zeros_like(vertices)
            mesh.colours = torch.zeros_like(vertices) if colour else None
            return mesh
        g = _nnr_ops.density_grad(vertices, w, b, net.hidden_dim).neg()
        mesh.normals = g / g.norm(2, 1, keepdim=True)
        if colour:
            view = torch.nan_to_num(-mesh.normals)             # (a vanishing gradient: no direction to look along)
            rgb, _ = _nnr_ops.mlp_points(vertices, view, w, b, hidden=net.hidden_dim, split2=True)
            mesh.colours = rgb.clamp(0., 1.)
    return mesh


# ----------------------------------------------------------------------------------------------------------------------
# the refined mesh: the fine grid evaluated in sparse bricks
# ----------------------------------------------------------------------------------------------------------------------
BRICK = 8      # grid points per brick and axis (nnr_bricks_f16.hip)


def refined_grid(lo, hi, resolution, refine):
    """The coarse grid of `resolution` points per axis over [lo, hi] and the `refine` (2, 4 or 8) times finer one that shares its points ->
    (origin, step_c, dims_c, step_f, dims_f).  dims_f = (n - 1) refine + 1; step_f = (hi - lo) / (n_f - 1), rounded to fp32 once, and
    step_c = refine * step_f, exact (a power of two): coarse point k and fine point refine * k have the same bits, in the kernels' own
    fl(origin + fl(step * i)).  (The coarse grid is therefore not grid_of(lo, hi, resolution) to the last bit: its step derives from the fine one.)"""
    if refine not in (2, 4, 8):
        raise ValueError("refine: 2, 4 or 8; got %r" % (refine,))
    dims_c = _resolution3(resolution)
    dims_f = tuple((n - 1) * refine + 1 for n in dims_c)
    origin = [float(np.float32(v)) for v in lo]
    step_f = [float(np.float32((float(h) - float(l)) / (n - 1))) for l, h, n in zip(lo, hi, dims_f)]
    step_c = [float(np.float32(refine) * np.float32(v)) for v in step_f]
    return origin, step_c, dims_c, step_f, dims_f


def select_cells(coarse_volume, level, dilate=1):
    """The coarse cells to refine -> bool (nz - 1, ny - 1, nx - 1): those whose eight corners are not all on one side of the level (`inside` is
    volume > level, as in surface_nets; a NaN corner counts as crossing: what lies there is not known), and the cells within `dilate` cells of
    one in the 26-neighbourhood."""
    vol = coarse_volume.detach()
    nz, ny, nx = vol.shape
    if min(nz, ny, nx) < 2:
        return torch.zeros(max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0), dtype=torch.bool, device=vol.device)
    ins, nan = vol > float(level), torch.isnan(vol)

    def cells(t, dx, dy, dz):
        return t[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]

    n_in = sum(cells(ins, *c).to(torch.uint8) for c in _CORNERS)
    sel = (n_in > 0) & (n_in < 8)
    for c in _CORNERS:
        sel = sel | cells(nan, *c)
    dilate = int(dilate)
    if dilate < 0:
        raise ValueError("dilate: a cell count >= 0")
    if dilate:
        sel = torch.nn.functional.max_pool3d(sel[None, None].to(torch.float32), 2 * dilate + 1, 1, dilate)[0, 0] > 0
    return sel


def _brick_dims(dims_f):
    return tuple((int(n) + BRICK - 1) // BRICK for n in dims_f)


def bricks_for(selected, refine, dims_f):
    """The bricks of the fine grid that hold any fine point of a selected coarse cell -- cell c's points are refine c .. refine c + refine per
    axis -> (B,3) int32, columns (bx, by, bz) as the kernel takes them, each brick once, sorted by (bz, by, bx) ascending."""
    nbx, nby, nbz = _brick_dims(dims_f)
    cell = selected.nonzero()                                  # (n,3): (cz, cy, cx)
    first = (cell * refine) // BRICK                           # refine <= BRICK: a cell's points lie in at most two bricks per axis
    last = (cell * refine + refine) // BRICK
    keys = []
    for dz, dy, dx in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
        bz, by, bx = (last if dz else first)[:, 0], (last if dy else first)[:, 1], (last if dx else first)[:, 2]
        keys.append((bz * nby + by) * nbx + bx)
    key = torch.unique(torch.cat(keys))                        # sorted
    return torch.stack([key % nbx, (key // nbx) % nby, key // (nbx * nby)], 1).to(torch.int32)


def sparse_surface_nets(values, bricks, level, origin, step, dims_f):
    """surface_nets on the part of a fine grid that was evaluated in bricks: values (B,8,8,8) (nnr.ops.density_bricks: [b][lz][ly][lx]),
    bricks (B,3) integer (bx, by, bz), each brick once, inside the grid; origin, step, dims_f = (nx, ny, nz) the fine grid ->
    (vertices (V,3) float32, quads (Q,4) int64) on the values' device.  A cell takes part where all of its eight corners lie inside dims_f
    and in an evaluated brick.  Vertices are ordered by global cell index (z, y, x), quads as surface_nets orders them, and a vertex is
    computed by the code surface_nets uses (_cell_vertices): where the bricks cover every cell the surface crosses, the result IS
    surface_nets(dense fine volume), vertex bits and quad rows; in general it is that mesh restricted to the covered cells (a quad needs its
    four cells covered).  Memory follows B: the brick lookup is one int32 per brick position of the fine grid, the working set 9^3 values
    per brick; no tensor of the fine grid's size is made."""
    dev = values.device
    none = (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 4, dtype=torch.int64, device=dev))
    B = bricks.shape[0]
    nx, ny, nz = (int(n) for n in dims_f)
    if B == 0 or min(nx, ny, nz) < 2:
        return none
    if tuple(values.shape) != (B, BRICK, BRICK, BRICK):
        raise ValueError("values: shape %r for %d bricks" % (tuple(values.shape), B))
    level = float(level)
    nbx, nby, nbz = _brick_dims(dims_f)
    bx, by, bz = (bricks[:, c].to(torch.int64) for c in range(3))
    if int(bx.min()) < 0 or int(by.min()) < 0 or int(bz.min()) < 0 or int(bx.max()) >= nbx or int(by.max()) >= nby or int(bz.max()) >= nbz:
        raise ValueError("bricks: a brick outside the fine grid's %d x %d x %d bricks" % (nbx, nby, nbz))
    lookup = torch.full((nbz + 1, nby + 1, nbx + 1), -1, dtype=torch.int32, device=dev)      # (+1: the far neighbours of the last bricks)
    lookup[bz, by, bx] = torch.arange(B, dtype=torch.int32, device=dev)
    if int((lookup >= 0).sum()) != B:
        raise ValueError("bricks: a brick is listed twice")

    # every brick with the first layer of its far neighbours: 9^3 values, and which of them exist (evaluated, and inside the grid)
    vol = values.detach().to(torch.float64)
    v9 = torch.zeros(B, BRICK + 1, BRICK + 1, BRICK + 1, dtype=torch.float64, device=dev)
    has = torch.zeros(B, BRICK + 1, BRICK + 1, BRICK + 1, dtype=torch.bool, device=dev)
    own, far, one = slice(0, BRICK), slice(BRICK, BRICK + 1), slice(0, 1)
    for oz, oy, ox in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
        nb = lookup[bz + oz, by + oy, bx + ox].to(torch.int64)
        dst = (slice(None), far if oz else own, far if oy else own, far if ox else own)
        src = (nb.clamp(min=0), one if oz else own, one if oy else own, one if ox else own)
        v9[dst] = vol[src]
        has[dst] = (nb >= 0).view(B, 1, 1, 1)
    k = torch.arange(BRICK + 1, dtype=torch.int64, device=dev)
    has &= ((BRICK * bz).view(B, 1, 1, 1) + k.view(1, -1, 1, 1) < nz) & ((BRICK * by).view(B, 1, 1, 1) + k.view(1, 1, -1, 1) < ny) & \
        ((BRICK * bx).view(B, 1, 1, 1) + k.view(1, 1, 1, -1) < nx)

    def cells(t, dx, dy, dz):       # the corner (dx, dy, dz) of every cell of every brick
        return t[:, dz:BRICK + dz, dy:BRICK + dy, dx:BRICK + dx]

    ins9, nan9 = v9 > level, torch.isnan(v9)
    n_in = sum(cells(ins9, *c).to(torch.uint8) for c in _CORNERS)
    ok = cells(has, *_CORNERS[0]) & ~cells(nan9, *_CORNERS[0])
    for c in _CORNERS[1:]:
        ok = ok & cells(has, *c) & ~cells(nan9, *c)
    at = ((n_in > 0) & (n_in < 8) & ok).nonzero()             # (V,4): (b, lz, ly, lx)
    if at.shape[0] == 0:
        return none
    b, lz, ly, lx = at.unbind(1)
    cz, cy, cx = BRICK * bz[b] + lz, BRICK * by[b] + ly, BRICK * bx[b] + lx
    key = (cz * (ny - 1) + cy) * (nx - 1) + cx                 # the cell's place in surface_nets' order
    key, order = key.sort()
    b, lz, ly, lx, cz, cy, cx = (t[order] for t in (b, lz, ly, lx, cz, cy, cx))
    V = key.shape[0]
    val = torch.stack([v9[b, lz + dz, ly + dy, lx + dx] for dx, dy, dz in _CORNERS], 1)      # (V,8)
    o = torch.tensor([float(v) for v in origin], dtype=torch.float64, device=dev)
    s = torch.tensor([float(v) for v in step], dtype=torch.float64, device=dev)
    vertices = _cell_vertices(val, torch.stack([cx, cy, cz], 1), level, o, s)

    # quads: the edge from a cell's corner 0 along `axis` is the grid edge whose (+,+) cell it is; the other three lie one cell back in the
    # two other axes (surface_nets' rings, seen from that cell).  A cell that is not active has no vertex, so only active cells own quads.
    side = val > level
    flip_all = (s[0] * s[1] * s[2]).item() < 0
    czyx = torch.stack([cz, cy, cx], 1)
    rings = (((-1, -1, 0), (-1, 0, 0), (0, 0, 0), (0, -1, 0)),          # (dz, dy, dx) from the owning cell; x: y then z
             ((-1, 0, -1), (0, 0, -1), (0, 0, 0), (-1, 0, 0)),          # y: z then x
             ((0, -1, -1), (0, -1, 0), (0, 0, 0), (0, 0, -1)))          # z: x then y
    quads = []
    for axis, ring in enumerate(rings):
        others = [c for c in (0, 1, 2) if c != 2 - axis]       # columns of czyx that are not the edge's direction
        e = ((side[:, 0] != side[:, 1 << axis]) & (czyx[:, others[0]] >= 1) & (czyx[:, others[1]] >= 1)).nonzero().squeeze(1)
        if e.shape[0] == 0:
            continue
        q = []
        for dz, dy, dx in ring:
            want = ((cz[e] + dz) * (ny - 1) + (cy[e] + dy)) * (nx - 1) + (cx[e] + dx)
            pos = torch.searchsorted(key, want).clamp(max=V - 1)
            q.append(torch.where(key[pos] == want, pos, torch.full_like(pos, -1)))
        q = torch.stack(q, 1)
        rev = ~side[e, 0]                                      # the inside end is the far one: the normal points down the axis
        if flip_all:
            rev = ~rev
        q = torch.where(rev.unsqueeze(1), q[:, [0, 3, 2, 1]], q)
        quads.append(q[(q >= 0).all(1)])
    quads = torch.cat(quads) if quads else none[1]
    return vertices, quads


def extract_mesh_refined(renderer, lo, hi, resolution, refine, level=None, dilate=1, colour=True, max_bricks=None, chunk=65536, density=None):
    """The surface {raw density = level} inside [lo, hi] on a grid `refine` (2, 4 or 8) times finer than `resolution`, at a cost that follows
    the surface: the coarse volume on refined_grid's coarse grid (one launch of the grid kernel) -> select_cells(dilate) -> bricks_for ->
    nnr.ops.density_bricks (one launch of the brick kernel) -> sparse_surface_nets -> normals and colours as extract_mesh makes them,
    `chunk` vertices per call (one call's workspace grows with its point count).  The Mesh's origin, step and dims are the fine grid's; it
    records `refine` and the brick count.

    GUARANTEE AND ITS LIMIT.  The result is the dense fine mesh -- surface_nets of the density on all of the fine grid, which is never made --
    restricted to what the coarse pass sees: every vertex and quad is one of that mesh's, bit for bit, and every fine cell inside a selected
    coarse cell is present.  It is never different from the dense fine mesh, only possibly smaller: a component of the surface that crosses
    no coarse cell within `dilate` cells of a crossing one -- a blob or a gap thinner than a coarse cell that falls between the coarse
    points -- is absent, at every `dilate`.

    more than max_bricks (None: no bound) selected: ValueError naming the count.  density: (coarse, bricks), two callables
    coarse(origin, step, dims) -> (nz, ny, nx) and bricks(origin, step, bricks (B,3) int32) -> (B,8,8,8) that stand in for the two kernels;
    with them the host side runs anywhere (the tests' analytic fields on the CPU); normals and colours are then made only where a renderer
    is given as well.  Without `density`: GPU only."""
    net = renderer.model if renderer is not None else None
    if density is None:
        w, b = net.weights(), net.biases()
        if not w[0].is_cuda:
            raise NotImplementedError("extract_mesh_refined runs only on the GPU (HIP kernels nnr_grid_f16.hip, nnr_bricks_f16.hip) unless "
                                      "`density` supplies the field")
        coarse_of = lambda o, s, d: _nnr_ops.density_grid(o, s, d, w, b, hidden=net.hidden_dim)
        bricks_of = lambda o, s, br: _nnr_ops.density_bricks(o, s, br, w, b, hidden=net.hidden_dim)
    else:
        coarse_of, bricks_of = density
    if level is None:
        level = level_for(renderer.cfg, net.occ_activation)
    if int(chunk) < 1:
        raise ValueError("chunk: at least one vertex per call")
    origin, step_c, dims_c, step_f, dims_f = refined_grid(lo, hi, resolution, refine)
    with torch.no_grad():
        coarse = coarse_of(origin, step_c, dims_c)
        if tuple(coarse.shape) != tuple(dims_c[::-1]):
            raise ValueError("coarse volume: shape %r is not the grid's (nz, ny, nx) = %r" % (tuple(coarse.shape), tuple(dims_c[::-1])))
        selected = select_cells(coarse, level, dilate)
        bricks = bricks_for(selected, refine, dims_f)
        n_bricks = int(bricks.shape[0])
        if max_bricks is not None and n_bricks > max_bricks:
            raise ValueError("extract_mesh_refined: %d bricks selected (%d coarse cells), more than max_bricks = %d"
                             % (n_bricks, int(selected.sum()), max_bricks))
        mesh = Mesh(torch.zeros(0, 3, dtype=torch.float32, device=coarse.device), torch.zeros(0, 4, dtype=torch.int64, device=coarse.device),
                    level=float(level), origin=tuple(origin), step=tuple(step_f), dims=tuple(dims_f), refine=int(refine), n_bricks=n_bricks)
        if n_bricks:
            mesh.vertices, mesh.quads = sparse_surface_nets(bricks_of(origin, step_f, bricks), bricks, level, origin, step_f, dims_f)
        if net is None or not net.weights()[0].is_cuda:
            return mesh
        mesh.normals, mesh.colours = _normals_and_colours(net, mesh.vertices, colour, int(chunk))
    return mesh


def _normals_and_colours(net, vertices, colour, chunk):
    """extract_mesh's normals and colours, `chunk` vertices per kernel call -> (normals (V,3), colours (V,3) or None)"""
    w, b = net.weights(), net.biases()
    normals = torch.zeros_like(vertices)
    colours = torch.zeros_like(vertices) if colour else None
    for i in range(0, vertices.shape[0], chunk):
        v = vertices[i:i + chunk]
        g = _nnr_ops.density_grad(v, w, b, net.hidden_dim).neg()
        normals[i:i + chunk] = g / g.norm(2, 1, keepdim=True)
        if colour:
            view = torch.nan_to_num(-normals[i:i + chunk])         # (a vanishing gradient: no direction to look along)
            rgb, _ = _nnr_ops.mlp_points(v, view, w, b, hidden=net.hidden_dim, split2=True)
            colours[i:i + chunk] = rgb.clamp(0., 1.)
    return normals, colours


# ----------------------------------------------------------------------------------------------------------------------
# the TSDF mesh: rendered depth maps fused into a truncated signed distance volume
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Cameras:
    """The views a TSDF is fused from: one intrinsic matrix, one world matrix (world -> camera) per view, the image size."""
    camera_mat: torch.Tensor                     # (4,4) or (1,4,4)
    world_mats: torch.Tensor                     # (n,4,4)
    size: tuple                                  # (H, W)
    scale_mat: Optional[torch.Tensor] = None     # (4,4) or (1,4,4); None: the identity


def _mat44(m, n=None):
    m = torch.as_tensor(m).detach().to('cpu', torch.float64)
    m = m.reshape(-1, 4, 4)
    if n is not None and m.shape[0] == 1:
        m = m.expand(n, 4, 4)
    return m


def projection_rows(camera_mat, world_mat, scale_mat=None):
    """Rows 0..2 of K . world_mat . scale_mat per camera -> (n,12) fp32 on the CPU, row-major: what transform_to_camera_space followed by
    project_to_cam (model/common.py) apply to a world point, as the one matrix nnr.ops.tsdf_integrate takes.  world_mat (n,4,4) or (4,4);
    camera_mat and scale_mat (4,4), (1,4,4) or one per camera; scale_mat None: the identity.  The product is formed in float64 and rounded
    to fp32 once."""
    W = _mat44(world_mat)
    n = W.shape[0]
    K = _mat44(camera_mat, n)
    S = _mat44(scale_mat, n) if scale_mat is not None else torch.eye(4, dtype=torch.float64).expand(n, 4, 4)
    if K.shape[0] != n or S.shape[0] != n:
        raise ValueError("projection_rows: %d camera and %d scale matrices for %d world matrices" % (K.shape[0], S.shape[0], n))
    return (K @ W @ S)[:, :3, :].reshape(n, 12).to(torch.float32).contiguous()


def quantile_depth(alpha, z, level):
    """The depth at which a ray's transmittance falls below `level`, from its per-sample alphas (R,C) and depths (R,C) or (C), in torch and in
    the tensors' dtype: include/nnr_depth_median.h's definition with T as the cumulative product -- T_0 = 1, T_{i+1} = T_i (1 - alpha_i +
    1e-6); m the first sample with T_{m+1} < level; q = z_m + (z_next - z_m) ((T_m - level) / (T_m - T_{m+1})), z_next = z_{m+1}, z_m
    behind the last sample.  No crossing: +inf, NaN where the row's product is NaN."""
    z = z.expand_as(alpha)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), (1. - alpha) + 1e-6], 1), 1)      # (R, C + 1)
    crossed = T[:, 1:] < level
    hit = crossed.any(1)
    m = crossed.to(torch.int8).argmax(1, keepdim=True)                                            # (the first True)
    z_m = z.gather(1, m)
    z_n = z.gather(1, (m + 1).clamp(max=z.shape[1] - 1))
    T0, T1 = T.gather(1, m), T.gather(1, m + 1)
    q = (z_m + (z_n - z_m) * ((T0 - level) / (T0 - T1)))[:, 0]
    none = torch.where(torch.isnan(T[:, -1]), torch.full_like(q, float('nan')), torch.full_like(q, float('inf')))
    return torch.where(hit, q, none)


def median_level(min_acc):
    """The transmittance level of depth_mode 'median': fp32(1 - float64(min_acc)), as a Python float; 0 < min_acc < 1"""
    min_acc = float(min_acc)
    if not 0. < min_acc < 1.:      # (a NaN fails)
        raise ValueError("depth_mode 'median': min_acc = %r must lie in (0, 1): the quantile of the ray's weight it asks for" % (min_acc,))
    level = float(np.float32(1. - min_acc))
    if not 0. < level < 1.:
        raise ValueError("depth_mode 'median': min_acc = %r leaves no fp32 level in (0, 1)" % (min_acc,))
    return level


def render_depth_maps(renderer, camera_mat, world_mats, size, min_acc=0.5, chunk=1 << 18, scale_mat=None, occupancy=None, t_min=None,
                      depth_mode='expected'):
    """The z-depth maps of renderer.model seen from the cameras (camera_mat, world_mats[i]) -> (n, H, W) fp32 on the model's device: what
    nope_nerf(eval_=True) reports as depth, without its colour.  Rays come from nnr.camera.ray_setup on arange_pixels((H, W)), the samples
    from the renderer's own z tables without noise; the rendered distance is divided by ray_norm under rendering.normalise_ray.
    Pixels whose accumulated weight is below min_acc (the phong renderer's tau) become +inf: the ray saw free space; NaN stays NaN.
    With C = num_points - outside_steps <= 256 samples the depth comes from the fused depth kernel (nnr.ops.render_depth: the density alone,
    8 bytes per ray), otherwise from nnr.render_rays' forward-only depth and its per-sample alphas.  chunk: rays per launch.
    occupancy: an OccupancyGrid of this (frozen) field, the caller's to keep valid.  With it and C <= 256 every chunk goes through the sparse
    depth kernel (nnr.ops.render_depth_sparse: samples in cells the grid calls empty are not evaluated, a workgroup of four rays stops once
    each is below the transmittance t_min); with C > 256 the grid is ignored and one logged line says so.  A culled sample is absent from
    the product, so the maps are the dense ones only as far as the grid's alpha_min is negligible.  t_min (0 <= t_min < 1; 0 or None: off; a
    ValueError without a grid): stopping drops weight and never adds any, it lowers a ray's acc by less than
    t_min (1 + C 1e-6 (1 + 1e-6)^C), about t_min, and moves its depth by at most that times the far depth.  Next to min_acc: a pixel whose
    full acc lies within that margin above min_acc can turn +inf, none turns finite; keep t_min well below min_acc (1e-3 against 0.5).
    min_acc, normalise_ray and the +inf rule are the same with and without a grid.
    depth_mode 'expected': all of the above.  'median' (DESIGN.md section 11.4): the pixel is q, the depth at which the ray's transmittance
    falls below level = fp32(1 - min_acc) -- where its accumulated weight reaches min_acc; 0 < min_acc < 1 --, divided by ray_norm as the
    depth is; +inf where it never does (the same event as `observed`), NaN stays NaN.  It lies on a surface the ray crosses, and the stop
    does not move it: with a grid t_min None means level (a smaller t_min is kept, a larger one is a ValueError), and the maps are
    bit for bit those of t_min = 0.  Above 256 samples quantile_depth of render_rays' alphas.
    sample_option 'ndc': NotImplementedError -- NDC depths are not world depths.  GPU only."""
    import nnr
    from nnr import camera as _camera
    from .common import arange_pixels
    if depth_mode not in ('expected', 'median'):
        raise ValueError("render_depth_maps: depth_mode %r is neither 'expected' nor 'median'" % (depth_mode,))
    median = depth_mode == 'median'
    level = median_level(min_acc) if median else None
    if t_min is None:      # expected: off; median: stop at the level, where a grid makes the stop available
        t_min = level if median and occupancy is not None else 0.
    t_min = float(t_min)
    if occupancy is None and t_min != 0.:
        raise ValueError("render_depth_maps: t_min = %r stops rays in the sparse depth kernel alone, which needs `occupancy`" % (t_min,))
    if median and float(np.float32(t_min)) > level:
        raise ValueError("render_depth_maps: t_min = %r above the median mode's level %r: a ray stopped there has not crossed it" % (t_min, level))
    cfg, net = renderer.cfg, renderer.model
    if cfg['sample_option'] == 'ndc':
        raise NotImplementedError("render_depth_maps: rendering.sample_option 'ndc' samples in NDC space, whose depths are not world depths")
    if cfg['sample_option'] != 'uniform':
        raise ValueError('unknown sample_option %r' % (cfg['sample_option'],))
    w, b = net.weights(), net.biases()
    dev = w[0].device
    if not w[0].is_cuda:
        raise NotImplementedError("render_depth_maps runs only on the GPU (HIP kernels nnr_depth_f16.hip / the render kernels)")
    H, W = (int(v) for v in size)
    if int(chunk) < 1:
        raise ValueError("chunk: at least one ray per launch")
    f32 = dict(dtype=torch.float32, device=dev)
    world_mats = torch.as_tensor(world_mats).detach().to(**f32).reshape(-1, 4, 4)
    n = world_mats.shape[0]
    K = torch.as_tensor(camera_mat).detach().to(**f32).reshape(-1, 4, 4)[:1]
    S = torch.as_tensor(scale_mat).detach().to(**f32).reshape(-1, 4, 4)[:1] if scale_mat is not None else torch.eye(4, **f32)[None]
    n_samples = int(cfg['num_points']) - int(cfg['outside_steps'])
    normalise, use_dir = bool(cfg['normalise_ray']), bool(cfg['use_ray_dir'])
    dist_alpha, relu_sigma = bool(cfg['dist_alpha']), net.occ_activation != 'softplus'
    pixels = arange_pixels((H, W), device=dev)[1]                                          # (1, H W, 2), row-major
    out = torch.empty(n, H * W, **f32)
    if occupancy is not None and n_samples > 256:
        logging.getLogger(__name__).info("render_depth_maps: occupancy grid ignored, dense render: %d samples per ray, the sparse depth kernel "
                                         "takes at most 256", n_samples)
    with torch.no_grad():
        z_lo, z_hi = renderer._z_tables(n_samples, renderer.depth_range[0], renderer.depth_range[1], False, dev)
        for i in range(n):
            origin, ray, view, ray_norm, _, _ = _camera.ray_setup(pixels, None, K, world_mats[i:i + 1], S, normalise, use_dir)
            for r0 in range(0, H * W, int(chunk)):
                sl = slice(r0, min(r0 + int(chunk), H * W))
                if median:
                    if n_samples <= 256 and occupancy is not None:
                        q = _nnr_ops.render_depth_sparse(origin[sl], ray[sl], z_lo, z_hi, None, occupancy, w, b, hidden=net.hidden_dim,
                                                         dist_alpha=dist_alpha, relu_sigma=relu_sigma, t_min=t_min, quantile_level=level)[:, 2]
                    elif n_samples <= 256:
                        q = _nnr_ops.render_depth(origin[sl], ray[sl], z_lo, z_hi, None, w, b, hidden=net.hidden_dim, dist_alpha=dist_alpha,
                                                  relu_sigma=relu_sigma, quantile_level=level)[:, 2]
                    else:
                        _, _, alpha, _ = nnr.render_rays(origin[sl], ray[sl], view[sl], z_lo, z_hi, None, w, b, hidden=net.hidden_dim,
                                                         dist_alpha=dist_alpha, white_bg=False, relu_sigma=relu_sigma, samples=True)
                        q = quantile_depth(alpha, z_lo, level)
                    out[i, sl] = q / ray_norm[sl] if normalise else q
                    continue
                if n_samples <= 256 and occupancy is not None:
                    da = _nnr_ops.render_depth_sparse(origin[sl], ray[sl], z_lo, z_hi, None, occupancy, w, b, hidden=net.hidden_dim,
                                                      dist_alpha=dist_alpha, relu_sigma=relu_sigma, t_min=t_min)
                    depth, acc = da[:, 0], da[:, 1]
                elif n_samples <= 256:
                    da = _nnr_ops.render_depth(origin[sl], ray[sl], z_lo, z_hi, None, w, b, hidden=net.hidden_dim, dist_alpha=dist_alpha,
                                               relu_sigma=relu_sigma)
                    depth, acc = da[:, 0], da[:, 1]
                else:
                    _, depth, alpha, _ = nnr.render_rays(origin[sl], ray[sl], view[sl], z_lo, z_hi, None, w, b, hidden=net.hidden_dim,
                                                         dist_alpha=dist_alpha, white_bg=False, relu_sigma=relu_sigma, samples=True)
                    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), (1. - alpha[:, :-1]) + 1e-6], 1), 1)
                    acc = (alpha * T).sum(1)
                if normalise:
                    depth = depth / ray_norm[sl]
                out[i, sl] = torch.where(acc < float(min_acc), torch.full_like(depth, float('inf')), depth)
    return out.view(n, H, W)


def tsdf_volume(sum, weight):
    """sum / weight of the accumulators nnr.ops.tsdf_integrate fills, NaN where the weight is 0: no camera observed the voxel"""
    return torch.where(weight > 0, sum / weight, torch.full_like(sum, float('nan')))


def tsdf_select_cells(volume, dilate=1):
    """The coarse cells of a TSDF volume to refine -> bool (nz - 1, ny - 1, nx - 1): those whose FINITE corners are not all on one side of 0
    (`inside` is volume > 0, as in surface_nets), and the cells within `dilate` cells of one in the 26-neighbourhood.  A NaN corner does not
    count as a crossing here -- the one deliberate difference from select_cells: unobserved space is most of a TSDF volume, and refining it
    all would make the sparse path dense."""
    vol = volume.detach()
    nz, ny, nx = vol.shape
    if min(nz, ny, nx) < 2:
        return torch.zeros(max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0), dtype=torch.bool, device=vol.device)
    ins, out = vol > 0., vol <= 0.                                 # (a NaN is neither)

    def cells(t, dx, dy, dz):
        return t[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]

    any_in, any_out = cells(ins, *_CORNERS[0]), cells(out, *_CORNERS[0])
    for c in _CORNERS[1:]:
        any_in, any_out = any_in | cells(ins, *c), any_out | cells(out, *c)
    sel = any_in & any_out
    dilate = int(dilate)
    if dilate < 0:
        raise ValueError("dilate: a cell count >= 0")
    if dilate:
        sel = torch.nn.functional.max_pool3d(sel[None, None].to(torch.float32), 2 * dilate + 1, 1, dilate)[0, 0] > 0
    return sel


def _all_bricks(dims, device):
    """every brick of the grid, (B,3) int32 (bx, by, bz), sorted by (bz, by, bx) ascending as bricks_for sorts"""
    nbx, nby, nbz = _brick_dims(dims)
    key = torch.arange(nbx * nby * nbz, dtype=torch.int64, device=device)
    return torch.stack([key % nbx, (key // nbx) % nby, key // (nbx * nby)], 1).to(torch.int32)


def _dense_from_bricks(values, dims):
    """(B,8,8,8) of _all_bricks(dims) -> the (nz, ny, nx) volume, cropped to the grid"""
    nbx, nby, nbz = _brick_dims(dims)
    nx, ny, nz = dims
    return values.view(nbz, nby, nbx, BRICK, BRICK, BRICK).permute(0, 3, 1, 4, 2, 5).reshape(BRICK * nbz, BRICK * nby, BRICK * nbx)[:nz, :ny, :nx]


def extract_mesh_tsdf(renderer, cameras, lo, hi, resolution, refine=None, trunc_voxels=3, dilate=1, colour=True, integrate=None,
                      depth_maps=None, min_acc=0.5, chunk=65536, max_bricks=None, occupancy=None, t_min=None, depth_mode='expected'):
    """The zero set of the truncated signed distance volume fused from the model's rendered depth maps of `cameras` (a Cameras) inside the box
    [lo, hi], as a Mesh at level 0 (Curless-Levoy with weight 1 per observation): what the model was trained on -- the rendered depth of
    its learned cameras -- and not a level of the raw density.  `inside` (positive) is behind the surfaces the cameras saw.

      refine None   the dense path: every brick of grid_of(lo, hi, resolution) is integrated (nnr.ops.tsdf_integrate), the accumulators
                    become sum / weight, NaN where unobserved (tsdf_volume), scattered into the (nz, ny, nx) volume -> surface_nets(., 0).
      refine 2|4|8  the refined path: that dense volume on refined_grid's coarse grid -> tsdf_select_cells(dilate) -> bricks_for ->
                    the same depth maps integrated on those fine bricks alone -> sparse_surface_nets(., 0).  As for extract_mesh_refined the
                    result is the dense fine mesh restricted to what the coarse pass sees.
      trunc_voxels  the truncation distance in steps of the grid that is being integrated (the largest |step| of its three): the coarse
                    volume is truncated at trunc_voxels coarse steps, the fine bricks at trunc_voxels fine steps.
      depth_maps    (n,H,W) z-depth maps on the integrator's device where the caller has them, or a callable () -> such maps (a timer's
                    hook); None: render_depth_maps(renderer, ...) with min_acc, occupancy and t_min (an OccupancyGrid of the frozen field
                    and the stop's transmittance: the sparse depth kernel, see there) and depth_mode ('expected', or 'median': the
                    depth at which the ray's accumulated weight reaches min_acc; with it t_min None stops at that level).
      integrate     a callable (origin, step, bricks, cams, depth, trunc, sum, weight) that stands in for nnr.ops.tsdf_integrate (the CPU
                    tests' reference integrator, a timer's hook); with it and depth_maps the host side runs anywhere, normals and colours
                    are then made only where a renderer on the GPU is given as well.
    Normals and colours are the density field's at the vertices, as the other two extractors make them (_normals_and_colours)."""
    net = renderer.model if renderer is not None else None
    on_gpu = net is not None and net.weights()[0].is_cuda
    if (integrate is None or depth_maps is None) and not on_gpu:
        raise NotImplementedError("extract_mesh_tsdf runs only on the GPU (HIP kernels nnr_depth_f16.hip, nnr_tsdf.hip) unless `integrate` and "
                                  "`depth_maps` supply the depth maps and their fusion")
    if not trunc_voxels > 0:
        raise ValueError("trunc_voxels: a positive number of grid steps")
    if integrate is None:
        integrate = lambda o, s, br, cm, dp, tr, sm, wt: _nnr_ops.tsdf_integrate(o, s, br, cm, dp, tr, sm, wt)
    with torch.no_grad():
        if depth_maps is None:
            if depth_mode == 'expected':
                depth = render_depth_maps(renderer, cameras.camera_mat, cameras.world_mats, cameras.size, min_acc=min_acc,
                                          scale_mat=cameras.scale_mat, occupancy=occupancy, t_min=t_min)
            else:
                depth = render_depth_maps(renderer, cameras.camera_mat, cameras.world_mats, cameras.size, min_acc=min_acc,
                                          scale_mat=cameras.scale_mat, occupancy=occupancy, t_min=t_min, depth_mode=depth_mode)
        else:
            depth = depth_maps() if callable(depth_maps) else depth_maps
        depth = depth.detach().to(torch.float32).contiguous()
        dev = depth.device
        cams = projection_rows(cameras.camera_mat, cameras.world_mats, cameras.scale_mat).to(dev)
        if depth.dim() != 3 or depth.shape[0] != cams.shape[0]:
            raise ValueError("depth maps: shape %r for %d cameras" % (tuple(depth.shape), cams.shape[0]))

        def fuse(origin, step, bricks):
            acc = torch.zeros(2, bricks.shape[0], BRICK, BRICK, BRICK, dtype=torch.float32, device=dev)
            trunc = float(np.float32(trunc_voxels) * np.float32(max(abs(v) for v in step)))
            integrate(origin, step, bricks, cams, depth, trunc, acc[0], acc[1])
            return tsdf_volume(acc[0], acc[1])

        if refine is None:
            origin, step, dims = grid_of(lo, hi, resolution)
            bricks = _all_bricks(dims, dev)
            vol = _dense_from_bricks(fuse(origin, step, bricks), dims)
            vertices, quads = surface_nets(vol, 0., origin, step)
            mesh = Mesh(vertices, quads, level=0., origin=tuple(origin), step=tuple(step), dims=tuple(dims), n_bricks=int(bricks.shape[0]))
        else:
            origin, step_c, dims_c, step, dims = refined_grid(lo, hi, resolution, refine)
            coarse = _dense_from_bricks(fuse(origin, step_c, _all_bricks(dims_c, dev)), dims_c)
            selected = tsdf_select_cells(coarse, dilate)
            bricks = bricks_for(selected, refine, dims)
            n_bricks = int(bricks.shape[0])
            if max_bricks is not None and n_bricks > max_bricks:
                raise ValueError("extract_mesh_tsdf: %d bricks selected (%d coarse cells), more than max_bricks = %d"
                                 % (n_bricks, int(selected.sum()), max_bricks))
            mesh = Mesh(torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 4, dtype=torch.int64, device=dev), level=0.,
                        origin=tuple(origin), step=tuple(step), dims=tuple(dims), refine=int(refine), n_bricks=n_bricks)
            if n_bricks:
                mesh.vertices, mesh.quads = sparse_surface_nets(fuse(origin, step, bricks), bricks, 0., origin, step, dims)
        if not on_gpu or not mesh.vertices.is_cuda:
            return mesh
        if mesh.vertices.shape[0] == 0:
            mesh.normals = torch.zeros_like(mesh.vertices)
            mesh.colours = torch.zeros_like(mesh.vertices) if colour else None
            return mesh
        mesh.normals, mesh.colours = _normals_and_colours(net, mesh.vertices, colour, int(chunk))
    return mesh


# ----------------------------------------------------------------------------------------------------------------------
# PLY
# ----------------------------------------------------------------------------------------------------------------------
def write_ply(path, mesh):
    """Binary little-endian PLY: vertices (x, y, z float32 [, nx, ny, nz float32] [, red, green, blue uint8 = round(255 colour)]) and
    triangular faces (uint8 count, 3 int32 indices), two per quad (Mesh.triangles)."""
    v = mesh.vertices.detach().cpu().numpy().astype('<f4')
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    cols = [v[:, 0], v[:, 1], v[:, 2]]
    if mesh.normals is not None:
        n = mesh.normals.detach().cpu().numpy().astype('<f4')
        fields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
        cols += [n[:, 0], n[:, 1], n[:, 2]]
    if mesh.colours is not None:
        c = colours_u8(mesh.colours).cpu().numpy()
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        cols += [c[:, 0], c[:, 1], c[:, 2]]
    rec = np.empty(v.shape[0], dtype=fields)
    for (name, _), col in zip(fields, cols):
        rec[name] = col
    tri = mesh.triangles().detach().cpu().numpy()
    if v.shape[0] > 2 ** 31 - 1:
        raise ValueError("write_ply: the face indices are int32")
    faces = np.empty(tri.shape[0], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    faces['n'] = 3
    faces['i'] = tri
    names = {'<f4': 'float', 'u1': 'uchar'}
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0]]
    header += ["property %s %s" % (names[t], name) for name, t in fields]
    header += ["element face %d" % tri.shape[0], "property list uchar int vertex_indices", "end_header"]
    with open(path, 'wb') as f:
        f.write(("\n".join(header) + "\n").encode('ascii'))
        f.write(rec.tobytes())
        f.write(faces.tobytes())


def colours_u8(colours):
    """[0,1] floats -> the 8-bit values write_ply stores"""
    return (colours.detach().clamp(0., 1.) * 255.).round().to(torch.uint8)


def read_ply(path):
    """What write_ply wrote -> dict(vertices (V,3) float32, normals (V,3) float32 or None, colours (V,3) uint8 or None, faces (F,3) int64),
    numpy arrays.  Reads this module's files (binary little-endian, float / uchar vertex properties, triangles), not PLY in general."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode('ascii').split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("%s: not a binary little-endian PLY file" % path)
    types = {'float': '<f4', 'uchar': 'u1'}
    fields, n_vert, n_face, element = [], 0, 0, None
    for line in lines[2:]:
        t = line.split()
        if t[:1] == ['element']:
            element = t[1]
            if element == 'vertex':
                n_vert = int(t[2])
            elif element == 'face':
                n_face = int(t[2])
        elif t[:1] == ['property'] and element == 'vertex':
            fields.append((t[2], types[t[1]]))
    rec = np.frombuffer(data, dtype=fields, count=n_vert, offset=end)
    faces = np.frombuffer(data, dtype=[('n', 'u1'), ('i', '<i4', (3,))], count=n_face, offset=end + rec.nbytes)
    if n_face and not (faces['n'] == 3).all():
        raise ValueError("%s: a face that is not a triangle" % path)
    have = {name for name, _ in fields}

    def cols(names, dtype):
        return np.stack([rec[n] for n in names], 1).astype(dtype) if set(names) <= have else None

    return dict(vertices=cols(('x', 'y', 'z'), np.float32), normals=cols(('nx', 'ny', 'nz'), np.float32),
                colours=cols(('red', 'green', 'blue'), np.uint8), faces=faces['i'].astype(np.int64))



# ----------------------------------------------------------------------------------------------------------------------
# the occupancy grid of the sparse inference render
# ----------------------------------------------------------------------------------------------------------------------
def level_for_alpha(alpha_min, delta, occ_activation):
    """The raw density whose compositor alpha at sample spacing `delta` is alpha_min: the inverse of the kernels' sample_alpha.

        sigma = -log(1 - alpha_min) / delta          rendering.dist_alpha: alpha = 1 - exp(-sigma delta)
        sigma = -log(1 - alpha_min)                  without it (delta None): alpha = 1 - exp(-sigma)
        raw = log(exp(sigma) - 1)                    occ_activation 'softplus': sigma = softplus(raw)
        raw = sigma                                  otherwise: sigma = relu(raw)

    alpha is non-decreasing in raw and in delta: a sample with raw < level at a spacing <= delta has alpha < alpha_min.  0 < alpha_min < 1."""
    alpha_min = float(alpha_min)
    if not 0. < alpha_min < 1.:
        raise ValueError("alpha_min = %r: an alpha strictly between 0 and 1" % alpha_min)
    sigma = -math.log1p(-alpha_min)
    if delta is not None:
        if not float(delta) > 0.:
            raise ValueError("delta = %r: a positive sample spacing (None without rendering.dist_alpha)" % (delta,))
        sigma = sigma / float(delta)
    if occ_activation == 'softplus':
        return math.log(math.expm1(sigma))
    return sigma


def occupancy_bits(volume, level, dilate=1):
    """The cells of a density volume that may hold matter, as the bitfield nnr_render_sparse reads (include/nnr_sparse.h): volume (nz, ny, nx)
    grid points -> int32 (nz - 1, ny - 1, w_x), w_x = ceil((nx - 1) / 32), on the volume's device.  Cell (i_x, i_y, i_z) spans the grid points
    i to i + 1 on every axis; it is occupied iff any of its 8 corners has raw >= level or is NaN (what lies there is not known), or if it lies
    within `dilate` cells of such a cell in the max norm.  Cell i_x is bit i_x & 31 of word [i_z][i_y][i_x >> 5]; the words are uint32 bit
    patterns held as int32 (bit 31 is the sign).  Plain torch, CPU or GPU tensors."""
    vol = volume.detach()
    nz, ny, nx = vol.shape
    if min(nz, ny, nx) < 2:
        raise ValueError("occupancy_bits: a volume of at least 2 grid points per axis; got %r" % ((nz, ny, nx),))
    dilate = int(dilate)
    if dilate < 0:
        raise ValueError("dilate: a cell count >= 0")
    hot = (vol >= float(level)) | torch.isnan(vol)
    occ = torch.zeros(nz - 1, ny - 1, nx - 1, dtype=torch.bool, device=vol.device)
    for dx, dy, dz in _CORNERS:
        occ = occ | hot[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    if dilate:
        occ = torch.nn.functional.max_pool3d(occ[None, None].to(torch.float32), 2 * dilate + 1, 1, dilate)[0, 0] > 0
    cx = nx - 1
    wx = (cx + 31) // 32
    padded = torch.zeros(nz - 1, ny - 1, wx * 32, dtype=torch.int64, device=vol.device)
    padded[..., :cx] = occ.to(torch.int64)
    words = (padded.view(nz - 1, ny - 1, wx, 32) << torch.arange(32, dtype=torch.int64, device=vol.device)).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)      # the uint32 pattern as int32
    return words.to(torch.int32).contiguous()


@dataclass
class OccupancyGrid:
    """What nnr.ops.render_sparse takes as `grid`: cell i_c of axis c spans [lo_c + i_c / inv_step_c, + 1 / inv_step_c); dims = (n_x, n_y, n_z)
    cells; bits as occupancy_bits packs them.  `occupied`: the share of cells whose bit is set (a 0-dim tensor on the bits' device)."""
    lo: tuple
    inv_step: tuple
    dims: tuple
    bits: torch.Tensor
    occupied: Optional[torch.Tensor] = None


def occupancy_grid(renderer, lo, hi, resolution, level, dilate=1, slab=None):
    """The occupancy grid of renderer.model over the box [lo, hi] with `resolution` CELLS per axis (one int or (n_x, n_y, n_z)): the raw density
    on the resolution + 1 grid points per axis (density_volume: the fused grid kernel, GPU only), thresholded at `level` (occupancy_bits).
    The kernel finds a sample's cell as (p - lo) * inv_step with inv_step = fl(1 / step) of the volume's fp32 step: a cell border may sit
    a few ulp from the grid point it stands for, which a dilation of one cell covers many times over."""
    cells = (int(resolution),) * 3 if isinstance(resolution, int) else tuple(int(v) for v in resolution)
    if len(cells) != 3 or min(cells) < 1:
        raise ValueError("resolution: one int or (n_x, n_y, n_z), at least one cell per axis; got %r" % (resolution,))
    points = tuple(n + 1 for n in cells)
    origin, step, _ = grid_of(lo, hi, points)
    if not all(s > 0. for s in step):
        raise ValueError("occupancy_grid: hi must exceed lo on every axis; got %r, %r" % (lo, hi))
    bits = occupancy_bits(density_volume(renderer, lo, hi, points, slab=slab), level, dilate)
    inv = tuple(float(np.float32(1.) / np.float32(s)) for s in step)
    return OccupancyGrid(tuple(origin), inv, cells, bits, occupied_share(bits, cells))


def occupied_share(bits, dims):
    """The share of a grid's cells whose bit is set -> 0-dim fp32 tensor on the bits' device (no host synchronisation)."""
    b = bits.to(torch.int64) & 0xFFFFFFFF
    ones = sum(((b >> k) & 1) for k in range(32)).sum()
    return ones.to(torch.float32) / float(int(dims[0]) * int(dims[1]) * int(dims[2]))
