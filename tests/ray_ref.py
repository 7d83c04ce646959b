"""The definition of ray casting against a triangle mesh of this project, in numpy f64: what csrc/ray_cast.hip computes bit for bit.

Every operation is one separately rounded f64 operation.  ``dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z``, ``cross(a, b) =
(a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)``.  A ray is an origin o, a direction d (not necessarily unit; t is in
units of |d|) and a t_max >= 0 (+inf allowed).  For a face (a, b, c), Moeller-Trumbore in this order:

  1. e1 = b - a, e2 = c - a, h = cross(d, e2), det = dot(e1, h)
  2. inv = 1 / det, s = o - a, u = inv * dot(s, h)
  3. q = cross(s, e1), v = inv * dot(d, q), t = inv * dot(e2, q)

The face is hit iff det != 0 and det is finite, 0 <= u <= 1, v >= 0, u + v <= 1, 0 <= t <= t_max; a NaN anywhere is a miss, and so is
a t that overflowed to +inf (the value of a miss).  Two-sided.  A face with a vertex index outside [0, nv), or whose normal
n = cross(e1, e2) has dot(n, n) == 0 or not finite, is skipped.  A ray's result is the hit with the smallest t, the lowest face index
among equal t; hit point o + t*d per component; a ray that hits nothing gets +inf, -1, NaN.

``fd_samples`` restates the sampler of the reference's scripts/sample_mesh-rd.py with the draws as inputs (sapcu_amd/ray.py
``sample_fd_rays``, include/sapcu_ray.h)."""
import numpy as np

from mesh_ref import valid_faces

COS_1RAD = 0.5403023058681398


def _dot(ux, uy, uz, vx, vy, vz):
    return (ux * vx + uy * vy) + uz * vz


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx


def ray_triangle(o, d, t_max, a, b, c):
    """o, d, a, b, c: f64 [..., 3] and t_max [...], broadcast against each other -> (t [...], hit bool [...], u, v, det)."""
    o, d, a, b, c = (np.asarray(x, dtype=np.float64) for x in (o, d, a, b, c))
    t_max = np.asarray(t_max, dtype=np.float64)
    ox, oy, oz = o[..., 0], o[..., 1], o[..., 2]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    with np.errstate(all="ignore"):
        e1x, e1y, e1z = b[..., 0] - ax, b[..., 1] - ay, b[..., 2] - az
        e2x, e2y, e2z = c[..., 0] - ax, c[..., 1] - ay, c[..., 2] - az
        hx, hy, hz = _cross(dx, dy, dz, e2x, e2y, e2z)
        det = _dot(e1x, e1y, e1z, hx, hy, hz)
        inv = 1.0 / det
        sx, sy, sz = ox - ax, oy - ay, oz - az
        u = inv * _dot(sx, sy, sz, hx, hy, hz)
        qx, qy, qz = _cross(sx, sy, sz, e1x, e1y, e1z)
        v = inv * _dot(dx, dy, dz, qx, qy, qz)
        t = inv * _dot(e2x, e2y, e2z, qx, qy, qz)
        hit = ((det != 0) & np.isfinite(det) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= t_max) & (t < np.inf))
    return t, hit, u, v, det


def all_t(origins, dirs, vertices, faces, t_max=None):
    """t f64 [nq, nf] of every ray against every face, +inf where the face is not hit (or skipped)."""
    vertices = np.asarray(vertices, dtype=np.float64)
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    tm = np.full(len(origins), np.inf) if t_max is None else np.asarray(t_max, dtype=np.float64).reshape(-1)
    ok = valid_faces(vertices, faces)
    f = np.where(ok[:, None], np.asarray(faces).astype(np.int64), 0)
    t, hit, _, _, _ = ray_triangle(origins[:, None, :], dirs[:, None, :], tm[:, None], vertices[f[:, 0]][None], vertices[f[:, 1]][None],
                                   vertices[f[:, 2]][None])
    return np.where(hit & ok[None, :], t, np.inf)


def ray_mesh(origins, dirs, vertices, faces, t_max=None, pairs_per_chunk=400000):
    """The brute force over all faces, in chunks of rays -> (t f64 [nq], face int64 [nq], hit f64 [nq, 3], number of skipped faces)."""
    vertices = np.asarray(vertices, dtype=np.float64)
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64)
    nq = len(origins)
    tm = np.full(nq, np.inf) if t_max is None else np.asarray(t_max, dtype=np.float64).reshape(-1)
    ok = valid_faces(vertices, faces)
    keep = np.nonzero(ok)[0]
    t_out = np.full(nq, np.inf)
    face = np.full(nq, -1, dtype=np.int64)
    hit_out = np.full((nq, 3), np.nan)
    if len(keep) and nq:
        a, b, c = (vertices[faces[keep, k]][None] for k in range(3))
        step = max(1, pairs_per_chunk // len(keep))
        for s in range(0, nq, step):
            t, hit, _, _, _ = ray_triangle(origins[s:s + step, None, :], dirs[s:s + step, None, :], tm[s:s + step, None], a, b, c)
            tt = np.where(hit, t, np.inf)
            j = np.argmin(tt, axis=1)                           # the first of equal minima: kept faces are in index order
            rows = np.arange(len(j))
            best = tt[rows, j]
            got = best < np.inf
            sl = np.arange(s, s + len(j))[got]
            t_out[sl] = t[rows[got], j[got]]                    # the face's own t (a -0.0 stays a -0.0)
            face[sl] = keep[j[got]]
        got = face >= 0
        with np.errstate(all="ignore"):
            hit_out[got] = origins[got] + t_out[got, None] * dirs[got]
    return t_out, face, hit_out, int((~ok).sum())


def fd_rays(surf, g, w):
    """The sampler's rays from its draws: (points = surf + len*dir, normals = -dir, lens, t_max = len * (1 + 2^-20)), all f64."""
    surf, g, w = (np.asarray(x, dtype=np.float64) for x in (surf, g, w))
    with np.errstate(all="ignore"):
        s = 1.0 / np.sqrt(_dot(g[:, 0], g[:, 1], g[:, 2], g[:, 0], g[:, 1], g[:, 2]))
        d = g * s[:, None]
        lens = w * 0.027 + 0.003
        points = surf + lens[:, None] * d
    return points, -d, lens, lens * (1.0 + 2.0 ** -20)


def fd_samples(vertices, faces, surf, sface, g, w):
    """scripts/sample_mesh-rd.py with the draws as inputs -> dict: keep bool [n]; points, normals [n,3] and lens [n] f64 of EVERY
    sample; t f64 [n] and face int64 [n] of the cast back from the thrown point along -dir."""
    vertices = np.asarray(vertices, dtype=np.float64)
    faces = np.asarray(faces).astype(np.int64)
    sface = np.asarray(sface).astype(np.int64)
    points, normals, lens, tmax = fd_rays(surf, g, w)
    t, face, _, _ = ray_mesh(points, normals, vertices, faces, t_max=tmax)
    ok = valid_faces(vertices, faces)
    inside = (sface >= 0) & (sface < len(faces))
    sf = np.where(inside, sface, 0)
    a, b, c = vertices[faces[sf, 0]], vertices[faces[sf, 1]], vertices[faces[sf, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        nx, ny, nz = _cross(e1[:, 0], e1[:, 1], e1[:, 2], e2[:, 0], e2[:, 1], e2[:, 2])
        s = 1.0 / np.sqrt(_dot(nx, ny, nz, nx, ny, nz))
        cosang = _dot(nx * s, ny * s, nz * s, -normals[:, 0], -normals[:, 1], -normals[:, 2])
        keep = inside & ok[sf] & (face == sface) & (cosang > COS_1RAD)
    return {"keep": keep, "points": points, "normals": normals, "lens": lens, "t": t, "face": face}


# ------------------------------------------------------------------------------------------------------- test meshes
BOX_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
# two triangles per side, outward; every side's diagonal runs through its first and third corner
BOX_F = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [3, 6, 2], [3, 7, 6], [0, 7, 3], [0, 4, 7],
                  [1, 2, 6], [1, 6, 5]], dtype=np.int64)


def icosphere(level, radius=1.0):
    """The icosahedron subdivided `level` times, on the sphere: 20 * 4^level outward faces over 10 * 4^level + 2 vertices."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius, np.array(f, dtype=np.int64)


def torus(nu, nw, R=0.35, r=0.12):
    """A torus of 2 * nu * nw outward faces (nu around the axis, nw around the tube)."""
    u, w = np.arange(nu) * (2 * np.pi / nu), np.arange(nw) * (2 * np.pi / nw)
    gu, gw = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(gw)) * np.cos(gu), (R + r * np.cos(gw)) * np.sin(gu), r * np.sin(gw)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nw), indexing="ij")
    idx = lambda a, b: (a % nu) * nw + (b % nw)
    f = np.concatenate([np.stack([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], -1).reshape(-1, 3),
                        np.stack([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)], -1).reshape(-1, 3)])
    return v, f


def surface_points(vertices, faces, n, rng):
    """n points on the mesh (a face uniformly, a point uniformly on it) -> (points f64 [n,3], face int64 [n])."""
    fi = rng.integers(0, len(faces), n)
    r1, r2 = np.sqrt(rng.uniform(size=n)), rng.uniform(size=n)
    a, b, c = (vertices[faces[fi, k]] for k in range(3))
    return (1 - r1)[:, None] * a + (r1 * (1 - r2))[:, None] * b + (r1 * r2)[:, None] * c, fi
