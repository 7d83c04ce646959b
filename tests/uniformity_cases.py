"""Cases shared by tests/test_uniformity_host.py and tests/test_gpu_uniformity.py: the fixture's cases with their targets (computed
once, never changed), and the analytic cases with references that use no window propagation: a flat grid (straight distance), a
plate with a hole and a notch (a visibility graph over the reflex corners), the unit cube (the minimum over its unfoldings)."""
import functools
import heapq
import math
import os

import numpy as np

import geodesic_ref as G
import mesh_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("ico", "box", "sheet", "torus", "bumpy", "plate")


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, "uniformity.npz")), np.load(os.path.join(GOLDEN, "mesh_p2f.npz"))


@functools.lru_cache(maxsize=None)
def case(name):
    """dict of one fixture case: vertices, faces, points, rows (the seed file's), radii and density as printed, counts, and the
    targets of the definition (tests/mesh_ref.py): tpoint, tface.  Read-only arrays."""
    fx, p2f = fixture()
    src = fx if name + "/vertices" in fx.files else p2f
    c = {"vertices": src[name + "/vertices"], "faces": src[name + "/faces"].astype(np.int64), "points": src[name + "/points"],
         "rows": fx[name + "/seeds"], "radii": fx[name + "/radii"], "density": fx[name + "/density"], "counts": fx[name + "/counts"]}
    _, tface, tpoint, _, _ = mesh_ref.point_mesh(c["points"], c["vertices"], c["faces"])
    c["tpoint"], c["tface"] = tpoint, tface
    for a in c.values():
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(counts [48,7], dist [48,nq]) of the definition on a fixture case, with the seeds as ``read_seeds`` gives them"""
    c = case(name)
    sf, sb = G.tool_rows_to_seeds(c["rows"])
    counts, dist = G.geodesic_disks(c["vertices"], c["faces"], c["tpoint"], c["tface"], sf, sb, G.disk_radii(c["vertices"], c["faces"]),
                                    return_dist=True)
    counts.setflags(write=False)
    dist.setflags(write=False)
    return counts, dist


# ------------------------------------------------------------------------------------------------------------ meshes
def grid_mesh(n, cells=None, z=None):
    xs = np.linspace(0.0, 1.0, n + 1)
    gx, gy = np.meshgrid(xs, xs, indexing="ij")
    v = np.stack([gx, gy, np.zeros_like(gx) if z is None else z(gx, gy)], -1).reshape(-1, 3)
    idx = lambda i, j: i * (n + 1) + j
    f = []
    for i, j in (cells if cells is not None else [(i, j) for i in range(n) for j in range(n)]):
        f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    f = np.array(f)
    used = np.unique(f)
    remap = -np.ones(len(v), np.int64)
    remap[used] = np.arange(len(used))
    return v[used], remap[f]


PLATE_N = 24
HOLE = ((8 / 24, 10 / 24), (14 / 24, 14 / 24))          # the open rectangle cut out of the plate
NOTCH = ((16 / 24, 16 / 24), (1.0, 1.0))


def plate_cells():
    return [(i, j) for i in range(PLATE_N) for j in range(PLATE_N) if not (8 <= i < 14 and 10 <= j < 14) and not (i >= 16 and j >= 16)]


def plate_mesh():
    return grid_mesh(PLATE_N, plate_cells())


def cube_mesh():
    v = np.array([[x, y, z] for z in (0.0, 1.0) for y in (0.0, 1.0) for x in (0.0, 1.0)])
    f = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2],
                  [1, 3, 7], [1, 7, 5]])
    return v, f


def tetrahedron():
    v = np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def locate(points, v, f):
    """(tpoint, tface) of points ON the mesh, by the definition of tests/mesh_ref.py"""
    _, tface, tpoint, _, _ = mesh_ref.point_mesh(np.asarray(points, np.float64), v, f)
    return tpoint, tface


def seeds_in_faces(v, f, faces, rng):
    w = rng.uniform(0.05, 1.0, (len(faces), 3))
    return np.asarray(faces, np.int64), w / w.sum(-1, keepdims=True)


def seed_points(v, f, sf, sb):
    return np.einsum("sk,skc->sc", sb, v[f[sf]])


# ------------------------------------------------------------------------------------------------------------ plate
def _blocked(p, q, rect):
    """does the open segment p-q pass through the open rectangle?"""
    (x0, y0), (x1, y1) = rect
    t0, t1 = 0.0, 1.0
    for d, a, lo, hi in ((q[0] - p[0], p[0], x0, x1), (q[1] - p[1], p[1], y0, y1)):
        if abs(d) < 1e-300:
            if not lo < a < hi:
                return False
            continue
        ta, tb = (lo - a) / d, (hi - a) / d
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    if t1 - t0 <= 1e-12:
        return False
    mx, my = p[0] + 0.5 * (t0 + t1) * (q[0] - p[0]), p[1] + 0.5 * (t0 + t1) * (q[1] - p[1])
    return x0 + 1e-12 < mx < x1 - 1e-12 and y0 + 1e-12 < my < y1 - 1e-12


def plate_distance(p, q):
    """the shortest path inside the plate between two of its points (2-D): Dijkstra on the visibility graph of p, q and the five
    reflex corners (the hole's four, the notch's inner one)"""
    (hx0, hy0), (hx1, hy1) = HOLE
    nodes = [tuple(p[:2]), tuple(q[:2]), (hx0, hy0), (hx1, hy0), (hx0, hy1), (hx1, hy1), NOTCH[0]]
    see = lambda a, b: not _blocked(a, b, HOLE) and not _blocked(a, b, NOTCH)
    best = {0: 0.0}
    heap = [(0.0, 0)]
    while heap:
        d, i = heapq.heappop(heap)
        if i == 1:
            return d
        if d > best.get(i, math.inf):
            continue
        for j in range(len(nodes)):
            if j != i and see(nodes[i], nodes[j]):
                nd = d + math.hypot(nodes[i][0] - nodes[j][0], nodes[i][1] - nodes[j][1])
                if nd < best.get(j, math.inf):
                    best[j] = nd
                    heapq.heappush(heap, (nd, j))
    return math.inf


@functools.lru_cache(maxsize=None)
def plate_case():
    """20 seeds beside the hole and the notch, 300 targets in the plate's cells, radii of 5 %, 15 % and 30 % of the area (paths bend), and
    the visibility-graph distances [ns, nq]"""
    v, f = plate_mesh()
    rng = np.random.default_rng(77)
    cells = plate_cells()
    pick = rng.integers(0, len(cells), 300)
    pts = np.array([[(cells[c][0] + rng.uniform(0.02, 0.98)) / PLATE_N, (cells[c][1] + rng.uniform(0.02, 0.98)) / PLATE_N, 0.0] for c in pick])
    tpoint, tface = locate(pts, v, f)
    cen = v[f].mean(1)
    box = lambda r: np.maximum(np.maximum(r[0][0] - cen[:, 0], cen[:, 0] - r[1][0]), np.maximum(r[0][1] - cen[:, 1], cen[:, 1] - r[1][1]))
    near = np.nonzero((box(HOLE) < 0.06) | (box(NOTCH) < 0.06))[0]              # faces within 0.06 of the hole or the notch
    sf, sb = seeds_in_faces(v, f, near[rng.integers(0, len(near), 20)], rng)
    radii = G.disk_radii(v, f, [0.05, 0.15, 0.3])
    sp = seed_points(v, f, sf, sb)
    ref = np.array([[plate_distance(s, t) for t in tpoint] for s in sp])
    return v, f, tpoint, tface, sf, sb, radii, ref


# ------------------------------------------------------------------------------------------------------------ cube
def cube_bottom_to_side(p, q):
    """the geodesic on the unit cube from p = (px, py, 0) on the bottom to q = (1, qy, qz) on the side x = 1: the minimum over the
    unfoldings across the shared edge, round the corner through the face y = 0 and round the corner through the face y = 1, each
    counted only where its straight line stays on the unfolded faces"""
    px, py, qy, qz = p[0], p[1], q[1], q[2]
    out = [math.hypot(1 + qz - px, qy - py)]                            # across x = 1: the line crosses it at a y between py and qy
    tx, ty = 1 + qy, -qz                                                # bottom -> face y = 0 -> side
    xa = px + (tx - px) * (py / (py - ty))                              # where it crosses y = 0
    yb = py + (ty - py) * ((1 - px) / (tx - px))                        # where it crosses x = 1
    if 0 <= xa <= 1 and -1 <= yb <= 0:
        out.append(math.hypot(tx - px, ty - py))
    tx, ty = 2 - qy, 1 + qz                                             # bottom -> face y = 1 -> side
    xa = px + (tx - px) * ((1 - py) / (ty - py))
    yb = py + (ty - py) * ((1 - px) / (tx - px))
    if 0 <= xa <= 1 and 1 <= yb <= 2:
        out.append(math.hypot(tx - px, ty - py))
    return min(out)


CUBE_PAIRS = (((0.8, 0.15, 0.0), (1.0, 0.1, 0.3)),       # straight across the edge
              ((0.9, 0.05, 0.0), (1.0, 0.05, 0.6)),      # shorter round the corner (1, 0, 0) through the face y = 0
              ((0.85, 0.93, 0.0), (1.0, 0.96, 0.7)),     # shorter round the corner (1, 1, 0) through the face y = 1
              ((0.3, 0.5, 0.0), (1.0, 0.45, 0.2)))


def cube_case():
    """(v, f, seeds as (faces, bary), tpoint, tface, reference [pairs]); seed i goes with target i"""
    v, f = cube_mesh()
    ps = np.array([p for p, _ in CUBE_PAIRS])
    qs = np.array([q for _, q in CUBE_PAIRS])
    _, sface = locate(ps, v, f)
    sb = np.array([np.linalg.solve(np.vstack([v[f[fa]].T, np.ones(3)])[[0, 1, 3]], [p[0], p[1], 1.0]) for p, fa in zip(ps, sface)])
    tpoint, tface = locate(qs, v, f)
    return v, f, sface.astype(np.int64), sb, tpoint, tface, np.array([cube_bottom_to_side(p, q) for p, q in CUBE_PAIRS])


def flat_case():
    """an 8 x 8 flat grid, 10 seeds, 200 targets: the geodesic is the straight distance"""
    v, f = grid_mesh(8)
    rng = np.random.default_rng(5)
    sf, sb = seeds_in_faces(v, f, rng.integers(0, len(f), 10), rng)
    pts = np.concatenate([rng.uniform(0.0, 1.0, (200, 2)), np.zeros((200, 1))], -1)
    tpoint, tface = locate(pts, v, f)
    sp = seed_points(v, f, sf, sb)
    return v, f, tpoint, tface, sf, sb, np.sqrt(((sp[:, None, :] - tpoint[None, :, :]) ** 2).sum(-1))


def agree(dist, ref, rmax, rtol):
    """dist equals ref at ``rtol`` where ref <= rmax and is +inf where ref > rmax; entries within 1e-9 of rmax are not judged"""
    dist, ref = np.asarray(dist), np.asarray(ref)
    inside, outside = ref <= rmax * (1 - 1e-9), ref > rmax * (1 + 1e-9)
    assert np.isfinite(dist[inside]).all(), "a target within the radius was not reached"
    assert np.isinf(dist[outside]).all(), "a target beyond the radius has a distance"
    err = np.abs(dist[inside] - ref[inside]) / np.maximum(ref[inside], 1e-300)
    assert err.size == 0 or err.max() <= rtol, err.max()
    return 0.0 if err.size == 0 else float(err.max())
