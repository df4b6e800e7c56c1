"""CPU: the refined mesh extraction of model/geometry.py (refined_grid, select_cells, bricks_for, sparse_surface_nets, extract_mesh_refined)
on analytic fields through `density=`: the fields are evaluated in numpy at the kernels' fp32 points, so the whole host side runs without
a GPU.  The oracle is surface_nets on the dense fine volume.  Fields on [-1, 1]^3, level 0, positive inside; the shapes (coarse points per
axis, refine) = (17,4), (33,2), (9,8) give a 65^3 fine grid, (12,4) a 45^3 one -- neither a multiple of the 8-point brick.

The partial-coverage cases: without dilation the selected coarse cells hold 7360 of the 0.06 shell's 9616 active fine cells at (17,4) (see
that test for what the bricks then cover); the 0.05 blob at (9,8) has 50 active fine cells and no coarse cell sees it, at dilate 0, 1 and 2."""
import functools

import numpy as np
import pytest
import torch

from model import geometry as G

LO, HI = (-1., -1., -1.), (1., 1., 1.)
SHAPES = [(17, 4), (33, 2), (12, 4), (9, 8)]


def _axis(o, s, i):
    """the kernels' coordinate fl(o + fl(s * (float) i)) in numpy fp32"""
    return np.float32(o) + np.float32(s) * i.astype(np.float32)


def _sphere(x, y, z, c=(0., 0., 0.), r=0.6):
    return r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)


FIELDS = {
    'sphere': lambda x, y, z: _sphere(x, y, z),
    'two_spheres': lambda x, y, z: np.maximum(_sphere(x, y, z, (-0.4, -0.1, 0.05), 0.33), _sphere(x, y, z, (0.45, 0.2, -0.1), 0.27)),
    'torus': lambda x, y, z: 0.18 - np.sqrt((np.sqrt(x ** 2 + y ** 2) - 0.55) ** 2 + z ** 2),
    'shell': lambda x, y, z: 0.03 - np.abs(np.sqrt(x ** 2 + y ** 2 + z ** 2) - 0.5),          # thickness 0.06 at r = 0.5
    'blob': lambda x, y, z: _sphere(x, y, z, (0.13, 0.11, 0.09), 0.05),
}


def _density(field):
    """the `density=` pair of extract_mesh_refined for an analytic field: float64 arithmetic on the fp32 points, rounded to fp32"""
    def coarse(origin, step, dims):
        ax = [_axis(origin[c], step[c], np.arange(dims[c])).astype(np.float64) for c in range(3)]
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        return torch.from_numpy(field(x, y, z).astype(np.float32))

    def bricks(origin, step, br):
        b = br.numpy().astype(np.int64)
        ax = [_axis(origin[c], step[c], 8 * b[:, c, None] + np.arange(8)[None]).astype(np.float64) for c in range(3)]      # (B,8) each
        x, y, z = ax[0][:, None, None, :], ax[1][:, None, :, None], ax[2][:, :, None, None]
        return torch.from_numpy(field(x, y, z).astype(np.float32))

    return coarse, bricks


@functools.lru_cache(maxsize=None)
def _dense(field, nc, refine, lo=LO, hi=HI):
    """computed once per case and shared, never written to: (dense fine volume, its surface_nets mesh, its active cells (cz, cy, cx), the grid)"""
    origin, step_c, dims_c, step_f, dims_f = G.refined_grid(lo, hi, nc, refine)
    vol = _density(field)[0](origin, step_f, dims_f)
    verts, quads = G.surface_nets(vol, 0., origin, step_f)
    v = vol.numpy()
    nz, ny, nx = v.shape
    corner = lambda a: [a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    cnt = sum(w.astype(np.int32) for w in corner(v > 0.))
    cells = np.stack(np.nonzero((cnt > 0) & (cnt < 8) & ~np.any(corner(np.isnan(v)), axis=0)), 1)
    assert cells.shape[0] == verts.shape[0]
    return vol, verts, quads, cells, (origin, step_c, dims_c, step_f, dims_f)


def _selected(field, grid, dilate):
    origin, step_c, dims_c, _, _ = grid
    return G.select_cells(_density(field)[0](origin, step_c, dims_c), 0., dilate)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rows(a):
    return [r.tobytes() for r in np.ascontiguousarray(a)]


# ------------------------------------------------------------------------------------------------------------------ refined_grid
@pytest.mark.parametrize("lo,hi,res,refine", [(LO, HI, n, r) for n, r in SHAPES] + [((1., 0.5, 1.), (-1., -0.5, -1.), 17, 4),
                                                                                     ((-1., -0.3, 0.2), (0.7, 0.9, 1.3), (9, 12, 17), 8),
                                                                                     ((-4. / 3, 0.1, -2.), (1.7, 0.9, 2.2), (12, 9, 33), 2)])
def test_refined_grid_coarse_points_are_fine_points_bit_for_bit(lo, hi, res, refine):
    origin, step_c, dims_c, step_f, dims_f = G.refined_grid(lo, hi, res, refine)
    assert dims_f == tuple((n - 1) * refine + 1 for n in dims_c)
    for c in range(3):
        assert step_c[c] == refine * step_f[c] and np.float32(step_f[c]) == step_f[c] and np.float32(origin[c]) == origin[c]
        assert (step_f[c] < 0) == (hi[c] < lo[c])
        coarse = _axis(origin[c], step_c[c], np.arange(dims_c[c]))
        fine = _axis(origin[c], step_f[c], np.arange(dims_f[c]))
        assert coarse.dtype == fine.dtype == np.float32
        assert np.array_equal(coarse.view(np.int32), fine[::refine].view(np.int32))
        assert abs(float(fine[-1]) - hi[c]) <= 4 * abs(hi[c] - lo[c]) * 2. ** -24 * dims_f[c]      # the last point is `hi` up to rounding


def test_refined_grid_rejects_other_factors():
    for refine in (1, 3, 16, 0):
        with pytest.raises(ValueError):
            G.refined_grid(LO, HI, 9, refine)


# ------------------------------------------------------------------------------------------------------------------ full coverage
@pytest.mark.parametrize("nc,refine", SHAPES)
@pytest.mark.parametrize("name", ['sphere', 'two_spheres', 'torus', 'shell'])
def test_full_coverage_gives_the_dense_fine_mesh_exactly(name, nc, refine):
    field = FIELDS[name]
    vol, verts, quads, cells, grid = _dense(field, nc, refine)
    assert verts.shape[0] > 0 and quads.shape[0] > 0
    # 1. coverage: every active cell of the dense fine volume lies in a selected coarse cell
    sel = _selected(field, grid, 1)
    inside = sel[cells[:, 0] // refine, cells[:, 1] // refine, cells[:, 2] // refine]
    assert bool(inside.all()), "%d of %d active fine cells lie outside the selected coarse cells" % (int((~inside).sum()), cells.shape[0])
    # 2. then the sparse mesh is the dense one: vertex bits, quad rows, in order
    mesh = G.extract_mesh_refined(None, LO, HI, nc, refine, level=0., dilate=1, density=_density(field))
    assert mesh.vertices.dtype == torch.float32 and mesh.quads.dtype == torch.int64
    assert mesh.vertices.shape == verts.shape and torch.equal(_bits(mesh.vertices), _bits(verts))
    assert mesh.quads.shape == quads.shape and torch.equal(mesh.quads, quads)
    assert mesh.refine == refine and mesh.dims == grid[4] and mesh.step == tuple(grid[3]) and mesh.origin == tuple(grid[0])
    assert 0 < mesh.n_bricks < np.prod([(n + 7) // 8 for n in grid[4]])
    assert mesh.normals is None and mesh.colours is None      # (no renderer: nothing to take them from)


# ------------------------------------------------------------------------------------------------------------------ partial coverage
def _assert_is_part_of(mesh, verts, quads):
    """every sparse vertex and quad is one of the dense mesh's (vertex bits; quad rows through the vertex map), in the dense order"""
    where = {r: i for i, r in enumerate(_rows(verts.numpy()))}
    assert len(where) == verts.shape[0]
    to_dense = np.array([where.get(r, -1) for r in _rows(mesh.vertices.numpy())], dtype=np.int64)
    assert (to_dense >= 0).all() and (np.diff(to_dense) > 0).all()
    dense_q = {r: i for i, r in enumerate(_rows(quads.numpy()))}
    at = np.array([dense_q.get(r, -1) for r in _rows(to_dense[mesh.quads.numpy()])], dtype=np.int64) if mesh.quads.shape[0] else np.zeros(0, np.int64)
    assert (at >= 0).all() and (np.diff(at) > 0).all()
    return to_dense


@pytest.mark.parametrize("nc,refine,in_selected,active,strictly", [(17, 4, 7360, 9616, False), (9, 8, 4800, 9616, True)])
def test_a_thin_shell_without_dilation_is_partly_covered(nc, refine, in_selected, active, strictly, capsys):
    """The 0.06 shell passes between the coarse points, so without dilation the selected coarse cells hold only a part of its active fine
    cells: 7360 of 9616 at (17,4), 4800 of 9616 at (9,8).  The mesh is a part of the dense one and holds at least those cells.  How much more
    it holds is the bricks' doing: bricks_for takes whole 8-point bricks, and sparse_surface_nets meshes every cell they cover.  At (9,8) a
    brick is one coarse cell wide and the mesh is strictly smaller than the dense one (8324 of 9616 vertices, 8160 of 9612 quads).  At
    (17,4) a brick is two coarse cells wide and the bricks of the 7360 happen to cover all 9616: the mesh is the whole dense mesh there,
    NOT strictly smaller as the selected cells alone would suggest -- so that case asserts the cell figures and containment, not `<`."""
    field = FIELDS['shell']
    vol, verts, quads, cells, grid = _dense(field, nc, refine)
    mesh = G.extract_mesh_refined(None, LO, HI, nc, refine, level=0., dilate=0, density=_density(field))
    to_dense = _assert_is_part_of(mesh, verts, quads)
    sel = _selected(field, grid, 0)
    inside = sel[cells[:, 0] // refine, cells[:, 1] // refine, cells[:, 2] // refine].numpy()
    with capsys.disabled():
        print("\nshell, (%d,%d), dilate 0: %d of %d active fine cells in selected coarse cells, %d of %d vertices, %d of %d quads"
              % (nc, refine, int(inside.sum()), cells.shape[0], mesh.vertices.shape[0], verts.shape[0], mesh.quads.shape[0], quads.shape[0]))
    assert (int(inside.sum()), cells.shape[0]) == (in_selected, active)          # the coarse pass alone sees strictly less
    # every dense active cell inside a selected coarse cell is present (the bricks cover the selected cells and their far corners)
    assert np.isin(np.nonzero(inside)[0], to_dense).all()
    assert in_selected <= mesh.vertices.shape[0] <= active and 0 < mesh.quads.shape[0] <= quads.shape[0]
    if strictly:
        assert mesh.vertices.shape[0] < verts.shape[0] and mesh.quads.shape[0] < quads.shape[0]


def test_fewer_bricks_give_a_strictly_smaller_part_of_the_dense_mesh():
    """sparse_surface_nets on a part of the covering bricks (those with bx < 4: the half x < 0 of the torus, cut on a brick boundary)"""
    field = FIELDS['torus']
    vol, verts, quads, cells, grid = _dense(field, 17, 4)
    br = G.bricks_for(_selected(field, grid, 1), 4, grid[4])
    br = br[br[:, 0] < 4]
    mesh = G.Mesh(*G.sparse_surface_nets(_density(field)[1](grid[0], grid[3], br), br, 0., grid[0], grid[3], grid[4]))
    to_dense = _assert_is_part_of(mesh, verts, quads)
    covered = cells[:, 2] + 1 <= 31                             # the cells whose corners all lie at fine x index <= 31
    assert 0 < int(covered.sum()) < cells.shape[0] and np.array_equal(to_dense, np.nonzero(covered)[0])
    assert 0 < mesh.quads.shape[0] < quads.shape[0]


@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_a_blob_between_the_coarse_points_is_lost_at_every_dilate(dilate):
    nc, refine = 9, 8
    field = FIELDS['blob']
    vol, verts, quads, cells, grid = _dense(field, nc, refine)
    assert cells.shape[0] == 50 and quads.shape[0] > 0         # the dense fine mesh has it ...
    assert not bool(_selected(field, grid, dilate).any())       # ... no coarse cell sees it
    mesh = G.extract_mesh_refined(None, LO, HI, nc, refine, level=0., dilate=dilate, density=_density(field))
    assert mesh.n_bricks == 0 and mesh.vertices.shape == (0, 3) and mesh.quads.shape == (0, 4)


# ------------------------------------------------------------------------------------------------------------------ edge cases
def test_a_nan_region_is_refined_and_makes_no_vertex():
    """NaN in a corner box of the field: the coarse cells with a NaN corner count as crossing, so the region is evaluated finely; the fine
    cells with a NaN corner make no vertex, as in surface_nets -- the result is the dense fine mesh, which has the sphere cut open there."""
    def field(x, y, z):
        v = _sphere(x, y, z) + 0. * (x + y + z)
        return np.where((x > 0.2) & (y > 0.25) & (z > 0.3), np.nan, v)

    nc, refine = 17, 4
    vol, verts, quads, cells, grid = _dense(field, nc, refine)
    assert bool(torch.isnan(vol).any())
    whole = G.surface_nets(_density(FIELDS['sphere'])[0](grid[0], grid[3], grid[4]), 0., grid[0], grid[3])[0]
    assert 0 < verts.shape[0] < whole.shape[0]                  # the NaN box removed a part of the sphere
    sel = _selected(field, grid, 0)
    coarse = _density(field)[0](grid[0], grid[1], grid[2])
    k = torch.isnan(coarse).nonzero()[0]                        # a NaN coarse point: the cell it is corner 0 of is selected
    assert bool(sel[k[0], k[1], k[2]])
    mesh = G.extract_mesh_refined(None, LO, HI, nc, refine, level=0., dilate=1, density=_density(field))
    assert not bool(torch.isnan(mesh.vertices).any())
    assert torch.equal(_bits(mesh.vertices), _bits(verts)) and torch.equal(mesh.quads, quads)


def test_fine_dims_that_are_no_multiple_of_the_brick():
    """65 = 8 * 8 + 1: the ninth brick along an axis holds one valid layer, the rest lies past the grid and is evaluated but never used.  A
    plane close to the far faces puts the surface into those bricks."""
    field = lambda x, y, z: 0.98 - np.maximum(np.maximum(x, y), z) + 0. * (x + y + z)        # inside: the cube max(x, y, z) < 0.98
    nc, refine = 17, 4
    vol, verts, quads, cells, grid = _dense(field, nc, refine)
    assert grid[4] == (65, 65, 65) and cells.max() == 63        # active cells in the last layer of cells: corners at fine index 64
    sel = G.select_cells(_density(field)[0](grid[0], grid[1], grid[2]), 0., 1)
    br = G.bricks_for(sel, refine, grid[4])
    assert int(br.max()) == 8                                   # the bricks that start at fine index 64
    mesh = G.extract_mesh_refined(None, LO, HI, nc, refine, level=0., density=_density(field))
    assert torch.equal(_bits(mesh.vertices), _bits(verts)) and torch.equal(mesh.quads, quads)
    # values past the grid's end are never looked at: poison them
    vals = _density(field)[1](grid[0], grid[3], br)
    idx = 8 * br.to(torch.int64)[:, :, None] + torch.arange(8)[None, None]                    # (B,3,8): global indices per axis
    past = (idx[:, 2, :, None, None] > 64) | (idx[:, 1, None, :, None] > 64) | (idx[:, 0, None, None, :] > 64)
    assert bool(past.any())
    v2, q2 = G.sparse_surface_nets(torch.where(past, torch.full_like(vals, float('nan')), vals), br, 0., grid[0], grid[3], grid[4])
    assert torch.equal(_bits(v2), _bits(verts)) and torch.equal(q2, quads)


def test_max_bricks_names_the_count():
    field = FIELDS['sphere']
    mesh = G.extract_mesh_refined(None, LO, HI, 17, 4, level=0., density=_density(field))
    assert G.extract_mesh_refined(None, LO, HI, 17, 4, level=0., density=_density(field), max_bricks=mesh.n_bricks).n_bricks == mesh.n_bricks
    with pytest.raises(ValueError, match=str(mesh.n_bricks)):
        G.extract_mesh_refined(None, LO, HI, 17, 4, level=0., density=_density(field), max_bricks=mesh.n_bricks - 1)


@pytest.mark.parametrize("refine", [2, 4, 8])
def test_bricks_for_is_sorted_unique_and_holds_every_point_of_the_selected_cells(refine):
    g = torch.Generator().manual_seed(5)
    sel = torch.rand(6, 9, 11, generator=g) < 0.08              # (ncz - 1, ncy - 1, ncx - 1)
    dims_f = tuple(n * refine + 1 for n in (11, 9, 6))
    br = G.bricks_for(sel, refine, dims_f)
    assert br.dtype == torch.int32 and br.shape[1] == 3
    nb = [(n + 7) // 8 for n in dims_f]
    key = ((br[:, 2].long() * nb[1] + br[:, 1].long()) * nb[0] + br[:, 0].long()).numpy()
    assert (np.diff(key) > 0).all()                             # (bz, by, bx) ascending, each once
    assert int(br.min()) >= 0 and all(int(br[:, c].max()) < nb[c] for c in range(3))
    want = set()                                                # restated point by point
    for cz, cy, cx in sel.nonzero().tolist():
        for pz in range(refine * cz, refine * cz + refine + 1):
            for py in range(refine * cy, refine * cy + refine + 1):
                for px in range(refine * cx, refine * cx + refine + 1):
                    want.add((px // 8, py // 8, pz // 8))
    assert set(map(tuple, br.tolist())) == want


def test_select_cells_dilates_in_the_26_neighbourhood():
    vol = torch.full((8, 9, 10), -1.)
    vol[3, 4, 5] = 1.                                           # one inside point: the 8 cells around it cross
    s0 = G.select_cells(vol, 0., 0)
    assert s0.shape == (7, 8, 9) and int(s0.sum()) == 8 and bool(s0[2:4, 3:5, 4:6].all())
    s1 = G.select_cells(vol, 0., 1)
    assert int(s1.sum()) == 64 and bool(s1[1:5, 2:6, 3:7].all())             # corners included: the 26-neighbourhood
    s3 = G.select_cells(vol, 0., 3)
    assert int(s3.sum()) == 7 * 8 * 8 and bool(s3[:, :, 1:].all())           # z -1..6 and y 0..7 clipped at the volume, x 1..8
    with pytest.raises(ValueError):
        G.select_cells(vol, 0., -1)


def test_an_empty_selection_gives_an_empty_mesh():
    field = lambda x, y, z: -1. - 0. * (x + y + z)              # outside everywhere
    mesh = G.extract_mesh_refined(None, LO, HI, 9, 4, level=0., density=_density(field))
    assert mesh.n_bricks == 0 and mesh.vertices.shape == (0, 3) and mesh.quads.shape == (0, 4) and mesh.dims == (33, 33, 33)
    v, q = G.sparse_surface_nets(torch.zeros(0, 8, 8, 8), torch.zeros(0, 3, dtype=torch.int32), 0., (0., 0., 0.), (1., 1., 1.), (33, 33, 33))
    assert v.shape == (0, 3) and q.shape == (0, 4)
    # evaluated bricks that the surface does not cross: no vertex either
    br = torch.tensor([[0, 0, 0], [1, 0, 0]], dtype=torch.int32)
    v, q = G.sparse_surface_nets(torch.full((2, 8, 8, 8), -1.), br, 0., (0., 0., 0.), (1., 1., 1.), (33, 33, 33))
    assert v.shape == (0, 3) and q.shape == (0, 4)


def test_sparse_surface_nets_refuses_bad_brick_lists():
    vals = torch.full((2, 8, 8, 8), -1.)
    with pytest.raises(ValueError, match="twice"):
        G.sparse_surface_nets(vals, torch.tensor([[1, 1, 1], [1, 1, 1]], dtype=torch.int32), 0., (0., 0., 0.), (1., 1., 1.), (33, 33, 33))
    with pytest.raises(ValueError, match="outside"):
        G.sparse_surface_nets(vals, torch.tensor([[1, 1, 1], [5, 1, 1]], dtype=torch.int32), 0., (0., 0., 0.), (1., 1., 1.), (33, 33, 33))
    with pytest.raises(ValueError, match="outside"):
        G.sparse_surface_nets(vals, torch.tensor([[1, 1, 1], [-1, 1, 1]], dtype=torch.int32), 0., (0., 0., 0.), (1., 1., 1.), (33, 33, 33))
