"""The shell walk every grid search shares (-m gpu; csrc/knn_grid.h grid_shell_walk) on degenerate grids: the one-sided bounds
and the "whole grid visited" exit.

A cloud of 300 points in a 1 x 0.04 x 0.04 slab, the slab along each axis in turn, and in a 1 x 1 x 0.04 plate, with cell_size 0.05
(explicit, so the grid route runs below the automatic thresholds): the grid is 21 x 1 x 1 (or 21 x 21 x 1), every query's cell
touches the grid's edge on four (two) sides from shell 0 on, and a walk ends by the integer exit at the latest.  The cloud holds its
box's corners and points on exact cell faces origin + i * cell_size; the 130 queries (two full waves and a partial one on the
brute-force route; on the grid route they spread over the cells, so every wave is a cell's single, partial chunk — cells with several
chunks are test_chunks_of_one_cell's in test_gpu_metrics.py and test_gpu_mesh.py) hold the corners, points up to 10 extents outside
the box on each side, and points on the cell faces of both grids searched (the cloud's, and the one over the centroids of 300 thin
triangles built on the cloud's points).

Through knn_self_grid (k = 1, 11, 64), nn_cross and point_mesh the grid route must equal the brute-force route bit for bit, must
really have run (info[0] == 1), and must report the degenerate dimensions.  The inputs were checked on the CPU against the numpy
definitions (a brute-force kNN in the kernels' operation order, tests/mesh_ref.py): no query ties at its nearest point or face, and the
only exact ties in the self-kNN are eight in each slab, between the box's corners, which the key (d, index) resolves on both routes."""
import numpy as np
import pytest
import torch

import gpu_utils as U
import test_gpu_mesh as GM

pytestmark = pytest.mark.gpu

CELL = 0.05
N, NQ = 300, 130
CASES = {"slab-x": ((1.0, 0.04, 0.04), (0, 1, 2)), "slab-y": ((1.0, 0.04, 0.04), (2, 0, 1)), "slab-z": ((1.0, 0.04, 0.04), (1, 2, 0)),
         "plate-xy": ((1.0, 1.0, 0.04), (0, 1, 2))}
_CACHE = {}


def grid_dims(pts):
    """(origin, [gx, gy, gz]) of grid_setup_kernel for an explicit cell size CELL: floor(extent / h) + 1 per axis."""
    lo, hi = pts.min(0), pts.max(0)
    return lo, [int(np.floor(e / CELL)) + 1 for e in hi - lo]


def inputs(name):
    """(cloud [N,3], queries [NQ,3], vertices [3N,3], faces [N,3]) of a case, f64 / int32, built once."""
    if name in _CACHE:
        return _CACHE[name]
    ext, perm = CASES[name]
    ext = np.array(ext)
    rng = np.random.default_rng(sorted(CASES).index(name) + 40)
    corners = np.stack(np.meshgrid(*[(0.0, e) for e in ext], indexing="ij"), -1).reshape(8, 3)
    cloud = rng.uniform(size=(N, 3)) * ext
    cloud[:8] = corners                                          # the box, hence the grid's origin, is exact
    cloud[8:29, 0] = np.arange(21) * CELL                        # on the cell faces along the long axis
    # thin triangles: (p, p + 0.02 along x, p + 0.002 along y), signs mixed; the centroids' box stays below one cell where the cloud's is
    s = rng.choice([-1.0, 1.0], size=(N, 2))
    vb, vc = cloud.copy(), cloud.copy()
    vb[:, 0] += 0.02 * s[:, 0]
    vc[:, 1] += 0.002 * s[:, 1]
    vertices = np.concatenate([cloud, vb, vc])
    faces = np.stack([np.arange(N), np.arange(N) + N, np.arange(N) + 2 * N], -1).astype(np.int32)
    centroid = ((cloud + vb) + vc) / 3.0
    clo = centroid.min(0)
    q = rng.uniform(size=(NQ, 3)) * ext
    q[:8] = corners
    k = 8
    for axis in range(3):                                        # outside the box on each side: 0.5, 3 and 10 extents
        for side in (0, 1):
            for t in (0.5, 3.0, 10.0):
                q[k, axis] = ext[axis] + t if side else -t
                k += 1
    q[k:k + 21, 0] = np.arange(21) * CELL                        # the faces of the cloud's grid (origin 0) ...
    q[k + 21:k + 42, 0] = clo[0] + np.arange(21) * CELL          # ... and of the centroids' grid
    k += 42
    for j, (ix, iy, iz) in enumerate([(0, 0, 0), (1, 1, 1), (20, 0, 1), (21, 1, 0), (7, 0, 0), (13, 1, 1), (19, 0, 0), (10, 1, 0)]):
        q[k + j] = (np.array([0.0, 0.0, 0.0]) if j % 2 == 0 else clo) + np.array([ix, iy, iz]) * CELL      # lattice points
    out = tuple(np.ascontiguousarray(a[:, list(perm)]) for a in (cloud, q, vertices)) + (faces,)
    _CACHE[name] = out
    return out


def _dev(a):
    return torch.as_tensor(a).to(U.dev())


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _degenerate(name, dims):
    """A dimension is 1 exactly where the extent is below one cell; the long ones have about 1 / CELL cells."""
    ext, perm = CASES[name]
    assert [d == 1 for d in dims] == [ext[p] < CELL for p in perm] and all(d in (1, 20, 21) for d in dims), (name, dims)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("k", [1, 11, 64])
def test_knn_self_grid_equals_brute_force(name, k):
    from sapcu_amd import generation as gen
    cloud = _dev(inputs(name)[0])
    info = []
    idx, dist = gen.knn_self_grid(cloud, k, cell_size=CELL, info=info)
    ridx, rdist, _ = gen.knn_gather(cloud, cloud, k, want_dist=True, want_patch=False)
    assert info[0] == 1, (name, info)
    assert info[1:] == grid_dims(inputs(name)[0])[1]
    _degenerate(name, info[1:])
    assert torch.equal(idx, ridx) and torch.equal(_bits(dist), _bits(rdist)), (name, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_nn_cross_grid_equals_brute_force(name):
    from sapcu_amd import metrics
    cloud, q = _dev(inputs(name)[0]), _dev(inputs(name)[1])
    info, rinfo = [], []
    d, i = metrics.nearest(q, cloud, CELL, info)
    rd, ri = metrics.nearest(q, cloud, 0.0, rinfo)                # 300 points, automatic cell size: the brute-force route
    assert info[0] == 1 and rinfo[0] == 0, (name, info, rinfo)
    assert info[1:] == grid_dims(inputs(name)[0])[1]
    _degenerate(name, info[1:])
    assert torch.equal(i, ri) and torch.equal(_bits(d), _bits(rd)), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_point_mesh_grid_equals_brute_force(name):
    _, q, vertices, faces = inputs(name)
    g = GM.device_call(q, vertices, faces, cell=CELL)
    b = GM.device_call(q, vertices, faces, brute=True)
    assert g[3][0] == 1 and b[3][0] == 0 and g[3][5] == b[3][5] == 0, (name, g[3], b[3])
    centroid = ((vertices[:N] + vertices[N:2 * N]) + vertices[2 * N:]) / 3.0
    assert g[3][1:4] == grid_dims(centroid)[1]
    _degenerate(name, g[3][1:4])
    assert torch.equal(g[1], b[1]) and GM._same(g[0], b[0]) and GM._same(g[2], b[2]), name
