"""CPU: model/geometry.py without a GPU -- surface nets on analytic fields (a sphere and a torus: containment, distance to the surface, closed
2-manifold, Euler characteristic, enclosed volume), orientation, empty volumes, NaN corners, float64 input, level_for against the occupancy
formula, the PLY round trip and the slab cuts of density_volume."""
import math
import os

import numpy as np
import pytest
import torch

from model import geometry as G

SQRT3 = math.sqrt(3.)
# the centre's offset from the grid, in cells: irrational, so that no grid point lies on the level set
OFFSET = np.array([math.sqrt(2.) - 1., math.pi - 3., math.e - 2.]) * 0.5


def _grid(n, lo=-1., hi=1.):
    origin, step, dims = G.grid_of((lo,) * 3, (hi,) * 3, n)
    ax = [origin[c] + step[c] * np.arange(dims[c], dtype=np.float64) for c in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return origin, step, np.stack([x, y, z], -1)      # (nz, ny, nx, 3)


def _sphere(n=32, r=0.6):
    origin, step, p = _grid(n)
    c = OFFSET * np.array(step)
    vol = r - np.linalg.norm(p - c, axis=-1)          # positive inside
    assert (vol != 0).all()
    return torch.from_numpy(vol.astype(np.float32)), origin, step, c


# the torus: 40 points per axis (h = 2 / 39): major radius 0.55, tube radius 0.22 -- the tube is 8.6 cells across, the hole 6.4 cells; at
# this resolution no cell face has the alternating corner pattern (checked below, on the CPU, by _ambiguous_faces), so surface nets are
# manifold on it
TORUS_N, TORUS_R, TORUS_r = 40, 0.55, 0.22


def _torus():
    origin, step, p = _grid(TORUS_N)
    q = p - OFFSET * np.array(step)
    vol = TORUS_r - np.sqrt((np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - TORUS_R) ** 2 + q[..., 2] ** 2)
    assert (vol != 0).all()
    return torch.from_numpy(vol.astype(np.float32)), origin, step, OFFSET * np.array(step)


def _ambiguous_faces(vol, level=0.):
    """cell faces whose four corners alternate around the face (in, out, in, out)"""
    s = vol.numpy() > level
    n = 0
    for axis in range(3):
        a, b = [ax for ax in range(3) if ax != axis]
        sl = lambda da, db: tuple(slice(da, s.shape[ax] - 1 + da) if ax == a else slice(db, s.shape[ax] - 1 + db) if ax == b else slice(None)
                                  for ax in range(3))
        c00, c10, c11, c01 = s[sl(0, 0)], s[sl(1, 0)], s[sl(1, 1)], s[sl(0, 1)]
        n += int(((c00 == c11) & (c10 == c01) & (c00 != c10)).sum())
    return n


def _active_cells(vol, level=0.):
    """(V,3) (cx, cy, cz) of the cells whose corners straddle the level, in cell order (x fastest) -- restated in numpy"""
    v = vol.numpy().astype(np.float64)
    s = v > level
    nz, ny, nx = v.shape
    views = [s[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    nans = [np.isnan(v)[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    cnt = sum(w.astype(np.int32) for w in views)
    act = (cnt > 0) & (cnt < 8) & ~np.any(nans, axis=0)
    cz, cy, cx = np.nonzero(act)
    return np.stack([cx, cy, cz], 1)


def _placement_bound(h, rho):
    """How far from the surface {f = 0} of a signed distance f a surface-nets vertex may lie, where no curvature radius of f's level sets
    within the cells is below rho.  An interpolated crossing x on an edge of length h has |f(x)| <= h^2 max|f''| / 8 <= h^2 / (8 rho) (the
    error of linear interpolation; f is 1-Lipschitz, so that is also x's distance to the surface).  The crossings of one cell lie within
    its diagonal sqrt(3) h of each other, so their mean leaves the surface by at most the sagitta of a chord of that length,
    3 h^2 / (8 rho), more.  Together h^2 / (2 rho): 0.07 h on the sphere and 0.2 h on the torus below, where a vertex at its cell's
    centre is up to sqrt(3) h / 2 = 0.87 h away."""
    return h * h / (2. * rho)


def _edges(quads):
    q = quads.numpy()
    d = np.concatenate([np.stack([q[:, i], q[:, (i + 1) % 4]], 1) for i in range(4)])      # directed
    return d


def _signed_volume(vertices, quads):
    v = vertices.double().numpy()
    q = quads.numpy()
    tri = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.)


def _check_closed_surface(vol, origin, step, euler):
    vertices, quads = G.surface_nets(vol, 0., origin, step)
    assert vertices.dtype == torch.float32 and vertices.shape[1:] == (3,) and quads.dtype == torch.int64 and quads.shape[1:] == (4,)
    V, Q = vertices.shape[0], quads.shape[0]
    assert V > 0 and Q > 0
    # every vertex lies inside its own cell: vertex k belongs to the k-th active cell (the result is sorted by cell index).  Slack: the
    # fp32 rounding of a coordinate of magnitude <= 1 (2^-24) and the float64 evaluation of the cell's walls, a few ulp together
    cells = _active_cells(vol)
    assert cells.shape[0] == V
    o, s = np.array(origin), np.array(step)
    lo, hi = o + s * cells, o + s * (cells + 1)
    v = vertices.double().numpy()
    slack = 4 * 2. ** -24
    assert (v >= lo - slack).all() and (v <= hi + slack).all()
    # a closed 2-manifold: every quad has four distinct corners, every edge is shared by exactly two quads, once in each direction
    q = quads.numpy()
    assert q.min() >= 0 and q.max() < V and all(len(set(row)) == 4 for row in q.tolist())
    d = _edges(quads)
    assert len({(a, b) for a, b in d.tolist()}) == d.shape[0]                        # no directed edge twice: consistently oriented
    und, counts = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    assert (counts == 2).all()
    assert np.unique(q).shape[0] == V                                                # every vertex is used
    assert V - und.shape[0] + Q == euler
    return vertices, quads


def test_sphere():
    vol, origin, step, c = _sphere()
    h, r = step[0], 0.6
    vertices, quads = _check_closed_surface(vol, origin, step, euler=2)
    dist = np.linalg.norm(vertices.double().numpy() - c, axis=1)
    assert np.abs(dist - r).max() <= SQRT3 * h                                       # the surface passes through the vertex's cell
    print("\nsphere: worst |dist - r| = %.4f h, placement bound %.4f h" % (np.abs(dist - r).max() / h, _placement_bound(h, r - SQRT3 * h) / h))
    assert np.abs(dist - r).max() <= _placement_bound(h, r - SQRT3 * h)              # and the vertex is the mean of the crossings
    vol_mesh = _signed_volume(vertices, quads)
    assert 4. / 3. * math.pi * (r - SQRT3 * h) ** 3 < vol_mesh < 4. / 3. * math.pi * (r + SQRT3 * h) ** 3


def test_torus():
    vol, origin, step, c = _torus()
    assert _ambiguous_faces(vol) == 0
    h = step[0]
    vertices, quads = _check_closed_surface(vol, origin, step, euler=0)
    p = vertices.double().numpy() - c
    dist = np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - TORUS_R) ** 2 + p[:, 2] ** 2)
    assert np.abs(dist - TORUS_r).max() <= SQRT3 * h
    # curvature radii of the distance's level sets inside the active cells: the tube's, >= r - sqrt(3) h, and the azimuthal one,
    # >= R - r - sqrt(3) h, which is the larger
    rho = min(TORUS_r, TORUS_R - TORUS_r) - SQRT3 * h
    print("\ntorus: worst |dist - r| = %.4f h, placement bound %.4f h" % (np.abs(dist - TORUS_r).max() / h, _placement_bound(h, rho) / h))
    assert np.abs(dist - TORUS_r).max() <= _placement_bound(h, rho)
    vol_mesh = _signed_volume(vertices, quads)
    assert 2. * math.pi ** 2 * TORUS_R * (TORUS_r - SQRT3 * h) ** 2 < vol_mesh < 2. * math.pi ** 2 * TORUS_R * (TORUS_r + SQRT3 * h) ** 2


def test_negated_field_flips_the_orientation():
    vol, origin, step, _ = _sphere()
    v0, q0 = G.surface_nets(vol, 0., origin, step)
    v1, q1 = G.surface_nets(-vol, 0., origin, step)
    assert torch.equal(v0, v1)
    assert torch.equal(q1, q0[:, [0, 3, 2, 1]])
    assert _signed_volume(v1, q1) == pytest.approx(-_signed_volume(v0, q0), rel=1e-12) and _signed_volume(v1, q1) < 0


@pytest.mark.parametrize("axes", [(0,), (1,), (2,), (0, 1), (0, 1, 2)])
def test_negative_steps_keep_the_normal_pointing_out(axes):
    """the same surface stored mirrored along some axes (origin at the far end, negative step): still inside -> outside"""
    vol, origin, step, _ = _sphere()
    dims = vol.shape[::-1]
    o, s = list(origin), list(step)
    for a in axes:
        o[a], s[a] = origin[a] + step[a] * (dims[a] - 1), -step[a]
    mirrored = vol.flip([2 - a for a in axes])
    v0, q0 = G.surface_nets(vol, 0., origin, step)
    v1, q1 = G.surface_nets(mirrored, 0., o, s)
    assert v1.shape == v0.shape and q1.shape == q0.shape
    assert _signed_volume(v1, q1) == pytest.approx(_signed_volume(v0, q0), rel=1e-5)


def test_anisotropic_grid():
    """different resolutions and steps per axis: the vertices still sit within a cell's diagonal of the sphere"""
    origin, step, dims = G.grid_of((-1., -0.9, -0.8), (1., 0.9, 0.8), (24, 30, 36))
    ax = [origin[c] + step[c] * np.arange(dims[c]) for c in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    c = OFFSET * np.array(step)
    vol = torch.from_numpy((0.6 - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32))
    assert vol.shape == (36, 30, 24)
    vertices, quads = _check_closed_surface(vol, origin, step, euler=2)
    dist = np.linalg.norm(vertices.double().numpy() - c, axis=1)
    assert np.abs(dist - 0.6).max() <= np.linalg.norm(step)


@pytest.mark.parametrize("fill", [-1., 1.])
def test_a_volume_on_one_side_gives_an_empty_mesh(fill):
    vertices, quads = G.surface_nets(torch.full((6, 7, 8), fill), 0., (0., 0., 0.), (1., 1., 1.))
    assert vertices.shape == (0, 3) and vertices.dtype == torch.float32 and quads.shape == (0, 4) and quads.dtype == torch.int64


def test_a_nan_corner_removes_exactly_the_cells_that_touch_it():
    vol, origin, step, _ = _sphere()
    v0, q0 = G.surface_nets(vol, 0., origin, step)
    cells = _active_cells(vol)
    k = cells.shape[0] // 2
    gx, gy, gz = (int(t) for t in cells[k] + 1)      # the far corner of an active cell: an interior grid point next to the surface
    holed = vol.clone()
    holed[gz, gy, gx] = float("nan")
    touch = np.all((cells >= np.array([gx - 1, gy - 1, gz - 1])) & (cells <= np.array([gx, gy, gz])), axis=1)
    assert 1 <= touch.sum() <= 8
    keep = torch.from_numpy(~touch)
    new_id = torch.cumsum(keep.to(torch.int64), 0) - 1
    q_keep = q0[keep[q0].all(1)]
    v1, q1 = G.surface_nets(holed, 0., origin, step)
    assert torch.equal(v1, v0[keep])
    assert torch.equal(q1, new_id[q_keep])
    assert q1.shape[0] < q0.shape[0]


def test_float64_input_gives_the_same_mesh():
    vol, origin, step, _ = _sphere()
    v0, q0 = G.surface_nets(vol, 0., origin, step)
    v1, q1 = G.surface_nets(vol.double(), 0., origin, step)
    assert torch.equal(v0, v1) and torch.equal(q0, q1)
    v2, q2 = G.surface_nets(vol, 0.05, origin, step)       # another level: another mesh
    assert v2.shape != v0.shape or not torch.equal(v2, v0)


def test_two_runs_are_identical():
    vol, origin, step, _ = _torus()
    a, b = G.surface_nets(vol, 0., origin, step), G.surface_nets(vol, 0., origin, step)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _occ64(raw, activation, dist_alpha):
    """OfficialStaticNerf's occupancy (model/official_nerf.py) in float64"""
    s = math.log1p(math.exp(raw)) if activation == "softplus" else max(raw, 0.)
    return s if dist_alpha else 1. - math.exp(-s)


@pytest.mark.parametrize("activation", ["softplus", "relu"])
@pytest.mark.parametrize("dist_alpha", [False, True])
@pytest.mark.parametrize("tau", [0.5, 0.25, 0.9])
def test_level_for(activation, dist_alpha, tau):
    level = G.level_for({"dist_alpha": dist_alpha}, activation, tau)
    assert _occ64(level, activation, dist_alpha) == pytest.approx(tau, abs=1e-14)
    closed = {("softplus", False): math.log(tau / (1. - tau)), ("softplus", True): math.log(math.exp(tau) - 1.),
              ("relu", False): -math.log(1. - tau), ("relu", True): tau}[(activation, dist_alpha)]
    assert level == pytest.approx(closed, abs=1e-14)
    # the occupancy is non-decreasing through the level: raw > level is the renderer's occ > tau
    assert _occ64(level + 1e-6, activation, dist_alpha) > tau > _occ64(level - 1e-6, activation, dist_alpha)


def test_level_for_defaults_to_the_phong_surface():
    assert G.level_for({"dist_alpha": False}, "softplus") == 0.
    assert G.level_for({"dist_alpha": True}, "relu") == 0.5


def test_ply_round_trip(tmp_path):
    vol, origin, step, c = _sphere(16)
    vertices, quads = G.surface_nets(vol, 0., origin, step)
    g = torch.Generator().manual_seed(3)
    normals = torch.nn.functional.normalize(vertices - torch.tensor(c, dtype=torch.float32), dim=1)
    colours = torch.rand(vertices.shape[0], 3, generator=g)
    mesh = G.Mesh(vertices, quads, normals=normals, colours=colours)
    path = os.path.join(str(tmp_path), "sphere.ply")
    G.write_ply(path, mesh)
    back = G.read_ply(path)
    assert back["vertices"].dtype == np.float32 and np.array_equal(back["vertices"], vertices.numpy())
    assert np.array_equal(back["normals"], normals.numpy())
    assert back["colours"].dtype == np.uint8 and np.array_equal(back["colours"], np.round(colours.numpy().astype(np.float64) * 255.).astype(np.uint8))
    q = quads.numpy()
    faces = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3)         # two triangles per quad, along the 0-2 diagonal
    assert back["faces"].shape == (2 * q.shape[0], 3) and np.array_equal(back["faces"], faces)
    # without normals and colours
    G.write_ply(path, G.Mesh(vertices, quads))
    bare = G.read_ply(path)
    assert bare["normals"] is None and bare["colours"] is None and np.array_equal(bare["vertices"], vertices.numpy())
    assert open(path, "rb").read().startswith(b"ply\nformat binary_little_endian 1.0\n")


@pytest.mark.parametrize("oz,sz,nz,slab", [(-1., 2. / 255., 256, 16), (-0.37, 0.0123, 100, 7), (1., -2. / 47., 48, 5), (0., 0.25, 64, 8),
                                           (3.7, 1e-3, 257, 64)])
def test_slab_cuts_reproduce_the_one_call_layers(oz, sz, nz, slab):
    """density_volume's slabs: every launch (iz0, n, origin_z) forms for its layer j, in the kernel's fp32 arithmetic (product, then sum), the
    bits the one-call run forms for layer iz0 + j; the runs tile [0, nz) in order and none is longer than `slab`."""
    oz, sz = float(np.float32(oz)), float(np.float32(sz))
    runs = G._slab_origins(oz, sz, nz, slab)
    whole = np.float32(oz) + np.float32(sz) * np.arange(nz, dtype=np.float32)
    assert whole.dtype == np.float32
    nxt = 0
    for iz0, n, o in runs:
        assert iz0 == nxt and 1 <= n <= slab
        mine = np.float32(o) + np.float32(sz) * np.arange(n, dtype=np.float32)
        assert mine.dtype == np.float32 and np.array_equal(mine.view(np.uint32), whole[iz0:iz0 + n].view(np.uint32))
        nxt = iz0 + n
    assert nxt == nz
    if (oz, sz) == (0., 0.25):
        assert [r[1] for r in runs] == [slab] * (nz // slab)      # dyadic origin and step: nothing is cut short
