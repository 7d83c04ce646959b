"""The definition of the point-to-surface distance (P2F) of this project, in numpy f64: what csrc/mesh_dist.hip computes bit for bit.

Every operation is one separately rounded f64 operation.  ``dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z``.  The closest point of a
triangle (a, b, c) to a query p is Ericson's, the first matching region wins:

  1. ab = b - a, ac = c - a, ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap); d1 <= 0 and d2 <= 0:               q = a
  2. bp = p - b, d3 = dot(ab, bp), d4 = dot(ac, bp); d3 >= 0 and d4 <= d3:                                      q = b
  3. vc = d1*d4 - d3*d2; vc <= 0 and d1 >= 0 and d3 <= 0:    v = d1 / (d1 - d3),                                q = a + v*ab
  4. cp = p - c, d5 = dot(ab, cp), d6 = dot(ac, cp); d6 >= 0 and d5 <= d6:                                      q = c
  5. vb = d5*d2 - d1*d6; vb <= 0 and d2 >= 0 and d6 <= 0:    w = d2 / (d2 - d6),                                q = a + w*ac
  6. va = d3*d6 - d5*d4; va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:  w = (d4 - d3) / ((d4 - d3) + (d5 - d6)),   q = b + w*(c - b)
  7. otherwise: den = 1 / ((va + vb) + vc), v = vb*den, w = vc*den,                                             q = (a + ab*v) + ac*w

r = p - q, d2 = dot(r, r).  A query's result is the face with the smallest d2, the lowest face index among bit-equal d2; the
distance is sqrt(d2).  A face with a vertex index outside [0, nv), or whose normal n = ab x ac has dot(n, n) == 0 or not finite,
is skipped; a query no face gives a finite d2 for gets NaN, face -1, NaN.  The selects below run in reverse priority."""
import numpy as np


def _dot(ux, uy, uz, vx, vy, vz):
    return (ux * vx + uy * vy) + uz * vz


def closest_point(p, a, b, c):
    """p, a, b, c: f64 [..., 3], broadcast against each other -> (q [..., 3], d2 [...], region [...] in 1..7)."""
    p, a, b, c = (np.asarray(x, dtype=np.float64) for x in (p, a, b, c))
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
    cx, cy, cz = c[..., 0], c[..., 1], c[..., 2]
    with np.errstate(all="ignore"):
        abx, aby, abz = bx - ax, by - ay, bz - az
        acx, acy, acz = cx - ax, cy - ay, cz - az
        apx, apy, apz = px - ax, py - ay, pz - az
        d1 = _dot(abx, aby, abz, apx, apy, apz)
        d2 = _dot(acx, acy, acz, apx, apy, apz)
        bpx, bpy, bpz = px - bx, py - by, pz - bz
        d3 = _dot(abx, aby, abz, bpx, bpy, bpz)
        d4 = _dot(acx, acy, acz, bpx, bpy, bpz)
        cpx, cpy, cpz = px - cx, py - cy, pz - cz
        d5 = _dot(abx, aby, abz, cpx, cpy, cpz)
        d6 = _dot(acx, acy, acz, cpx, cpy, cpz)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        # 7
        den = 1.0 / ((va + vb) + vc)
        v, w = vb * den, vc * den
        qx, qy, qz = (ax + abx * v) + acx * w, (ay + aby * v) + acy * w, (az + abz * v) + acz * w
        region = np.full(np.broadcast(qx, px).shape, 7, dtype=np.int8)
        qx, qy, qz = (np.broadcast_to(t, region.shape) for t in (qx, qy, qz))

        def put(cond, nx, ny, nz, k):
            nonlocal qx, qy, qz, region
            qx, qy, qz = np.where(cond, nx, qx), np.where(cond, ny, qy), np.where(cond, nz, qz)
            region = np.where(cond, np.int8(k), region)

        # 6
        e43, e56 = d4 - d3, d5 - d6
        w = e43 / (e43 + e56)
        put((va <= 0) & (e43 >= 0) & (e56 >= 0), bx + w * (cx - bx), by + w * (cy - by), bz + w * (cz - bz), 6)
        # 5
        w = d2 / (d2 - d6)
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), ax + w * acx, ay + w * acy, az + w * acz, 5)
        # 4
        put((d6 >= 0) & (d5 <= d6), cx, cy, cz, 4)
        # 3
        v = d1 / (d1 - d3)
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), ax + v * abx, ay + v * aby, az + v * abz, 3)
        # 2
        put((d3 >= 0) & (d4 <= d3), bx, by, bz, 2)
        # 1
        put((d1 <= 0) & (d2 <= 0), ax, ay, az, 1)
        rx, ry, rz = px - qx, py - qy, pz - qz
        dd = _dot(rx, ry, rz, rx, ry, rz)
    return np.stack([qx, qy, qz], -1), dd, region


def valid_faces(vertices, faces):
    """bool [nf]: the faces that take part (indices in range, dot(n, n) finite and non-zero for n = ab x ac)."""
    vertices = np.asarray(vertices, dtype=np.float64)
    faces = np.asarray(faces).astype(np.int64)
    nv = len(vertices)
    ok = ((faces >= 0) & (faces < nv)).all(1)
    f = np.where(ok[:, None], faces, 0)
    a, b, c = vertices[f[:, 0]], vertices[f[:, 1]], vertices[f[:, 2]]
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
        nn = _dot(nx, ny, nz, nx, ny, nz)
    return ok & np.isfinite(nn) & (nn != 0)


def all_d2(points, vertices, faces):
    """d2 f64 [nq, nf] of every query against every face (inf where the face is skipped or d2 is not finite), regions [nq, nf]."""
    vertices = np.asarray(vertices, dtype=np.float64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    ok = valid_faces(vertices, faces)
    f = np.where(ok[:, None], np.asarray(faces).astype(np.int64), 0)
    _, dd, region = closest_point(points[:, None, :], vertices[f[:, 0]][None], vertices[f[:, 1]][None], vertices[f[:, 2]][None])
    dd = np.where(np.isfinite(dd) & ok[None, :], dd, np.inf)
    return dd, region


def point_mesh(points, vertices, faces, pairs_per_chunk=400000):
    """The brute force over all faces, in chunks of queries -> (dist f64 [nq], face int64 [nq], closest f64 [nq, 3],
    region int8 [nq] (0 where no face), number of skipped faces)."""
    vertices = np.asarray(vertices, dtype=np.float64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64)
    ok = valid_faces(vertices, faces)
    keep = np.nonzero(ok)[0]
    nq = len(points)
    dist = np.full(nq, np.nan)
    face = np.full(nq, -1, dtype=np.int64)
    closest = np.full((nq, 3), np.nan)
    region = np.zeros(nq, dtype=np.int8)
    if len(keep) and nq:
        a, b, c = (vertices[faces[keep, k]][None] for k in range(3))
        step = max(1, pairs_per_chunk // len(keep))
        for s in range(0, nq, step):
            q, dd, reg = closest_point(points[s:s + step, None, :], a, b, c)
            dd = np.where(np.isfinite(dd), dd, np.inf)
            j = np.argmin(dd, axis=1)                           # the first of equal minima: kept faces are in index order
            rows = np.arange(len(j))
            best = dd[rows, j]
            hit = np.isfinite(best)
            sl = np.arange(s, s + len(j))[hit]
            dist[sl] = np.sqrt(best[hit])
            face[sl] = keep[j[hit]]
            closest[sl] = q[rows[hit], j[hit]]
            region[sl] = reg[rows[hit], j[hit]]
    return dist, face, closest, region, int((~ok).sum())
