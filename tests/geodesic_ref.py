"""The uniformity figure's definition in plain Python / numpy (include/sapcu_mesh.h, sapcu_amd/uniformity.py): exact geodesic
distances from a seed on a triangle mesh to points on its faces, by window propagation in the unfolded plane, in PRIORITY order
(a heap keyed by the nearest point of a window).  It shares no code with csrc/geodesic.hip: the mesh tables are dictionaries and
lists, the vertex fans are collected, not walked, and the queue is a heap, not a ring.

A window is (half-edge h it enters its face through, source image (sx, sy < 0) in the frame of h, interval [lo, hi] on the edge,
sigma).  The frame of half-edge h = 3 f + k of face f = (v0, v1, v2): a = v_k at the origin, b = v_(k+1) at (L, 0), c = v_(k+2) at
(cx, cy > 0).
"""
import heapq
import math

import numpy as np

TOOL_FRACTIONS = np.array([0.002, 0.004, 0.006, 0.008, 0.010, 0.012, 0.015], dtype=np.float32)
FILTER_SLACK = 1e-12
EDGE_EPS = 1e-12        # relative to the edge length: the slack of a visibility test, the narrowest window kept is a tenth of it


def disk_radii(vertices, faces, fractions=TOOL_FRACTIONS):
    """float32(sqrt(A * float32(fraction) / pi)) as f64, A the total area in f64: the tool's two roundings."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    area = float(np.sum(0.5 * np.sqrt(np.sum(n * n, -1))))
    pct = np.asarray(fractions, np.float32).astype(np.float64)
    return np.sqrt(area * pct / math.pi).astype(np.float32).astype(np.float64)


class Mesh:
    def __init__(self, vertices, faces):
        self.V = np.asarray(vertices, np.float64)
        self.F = np.asarray(faces, np.int64)
        V, F = self.V, self.F
        edge = {}
        for f in range(len(F)):
            a, b, c = F[f]
            n = np.cross(V[b] - V[a], V[c] - V[a])
            if not (np.isfinite(n @ n) and n @ n > 0):
                raise ValueError("face %d has zero area" % f)
            for k in range(3):
                key = (int(F[f, k]), int(F[f, (k + 1) % 3]))
                if key in edge:
                    raise ValueError("edge %s is traversed twice in one direction" % (key,))
                edge[key] = 3 * f + k
        self.twin = [edge.get((v, u), -1) for (u, v), _ in sorted(edge.items(), key=lambda kv: kv[1])]
        self.out = [[] for _ in range(len(V))]
        angle = np.zeros(len(V))
        boundary = np.zeros(len(V), bool)
        for h in range(3 * len(F)):
            f, k = divmod(h, 3)
            v, p, q = F[f, k], F[f, (k + 1) % 3], F[f, (k + 2) % 3]
            self.out[v].append(h)
            e1, e2 = V[p] - V[v], V[q] - V[v]
            angle[v] += math.atan2(np.linalg.norm(np.cross(e1, e2)), e1 @ e2)
            if self.twin[h] < 0:
                boundary[v] = boundary[p] = True
        self.pseudo = boundary | (angle >= 2 * math.pi - 1e-9)
        self.frames = {}

    def frame(self, h):
        """(a3, ex, ey, L, cx, cy) of half-edge h"""
        fr = self.frames.get(h)
        if fr is None:
            f, k = divmod(h, 3)
            a, b, c = (self.V[self.F[f, (k + i) % 3]] for i in range(3))
            L = math.sqrt((b - a) @ (b - a))
            ex = (b - a) / L
            cx = (c - a) @ ex
            perp = (c - a) - cx * ex
            cy = math.sqrt(perp @ perp)
            fr = self.frames[h] = (a, ex, perp / cy, L, cx, cy)
        return fr


def seed_point(mesh, face, bary):
    return sum(float(bary[k]) * mesh.V[mesh.F[face, k]] for k in range(3))


def geodesic_from_seed(mesh, face, bary, tpoint, tface, rmax, stats=None):
    """dist f64 [nq]: the geodesic distance from the seed to every target (a point tpoint[i] on face tface[i]), +inf where it is
    above rmax.  ``stats``, a dict, receives windows processed and the peak of the heap."""
    V, F, twin = mesh.V, mesh.F, mesh.twin
    s3 = seed_point(mesh, face, bary)
    tpoint = np.asarray(tpoint, np.float64)
    eu = np.sqrt(np.sum((tpoint - s3) ** 2, -1))
    cand = np.nonzero(eu <= rmax)[0]
    on_face = {}
    for i in cand:
        on_face.setdefault(int(tface[i]), []).append(int(i))
    dist = {int(i): math.inf for i in cand}
    d = {}
    heap = []
    count = [0, 0, 0]
    limit = rmax * (1 + 1e-12)

    def upd(v, val):
        if val < d.get(v, math.inf):
            d[v] = val
            if mesh.pseudo[v] and val <= limit:
                count[0] += 1
                heapq.heappush(heap, (val, count[0], -1, int(v), 0.0, 0.0, 0.0, 0.0, val))

    def push(h, sx, sy, lo, hi, sigma):
        near = math.hypot(sx - lo, sy) if sx < lo else (math.hypot(sx - hi, sy) if sx > hi else -sy)
        if sigma + near > limit:
            return
        count[0] += 1
        heapq.heappush(heap, (sigma + near, count[0], h, -1, sx, sy, lo, hi, sigma))

    def child(h, j, sx, sy, l, r, sigma, l_is_c, r_is_c):
        """the part [l, r] of a window on h goes through the far edge j of the face into the twin's face"""
        f, k = divmod(h, 3)
        t2 = twin[3 * f + j]
        if t2 < 0:
            return
        _, _, _, L, cx, cy = mesh.frame(h)
        P = {k: (0.0, 0.0), (k + 1) % 3: (L, 0.0), (k + 2) % 3: (cx, cy)}
        o, e = P[j], P[(j + 1) % 3]
        L2 = mesh.frame(t2)[3]
        ux, uy = (e[0] - o[0]), (e[1] - o[1])
        n = math.hypot(ux, uy)
        ux, uy = ux / n, uy / n

        def tr(px, py):
            qx, qy = px - o[0], py - o[1]
            return L2 - (qx * ux + qy * uy), -(-uy * qx + ux * qy)

        s2x, s2y = tr(sx, sy)
        if not s2y < 0:
            return

        def cross(x0):
            px, py = tr(x0, 0.0)
            den = py - s2y
            return px if den <= 0 else s2x + (px - s2x) * (-s2y) / den

        nl = 0.0 if l_is_c and j == (k + 1) % 3 else cross(l)
        nr = L2 if r_is_c and j == (k + 2) % 3 else cross(r)
        nl, nr = min(max(nl, 0.0), L2), min(max(nr, 0.0), L2)
        if nr - nl <= 0.1 * EDGE_EPS * L2:
            return
        push(t2, s2x, s2y, nl, nr, sigma)

    # the seed's own face
    for i in on_face.get(int(face), []):
        dist[i] = eu[i]
    for k in range(3):
        v = int(F[face, k])
        upd(v, math.sqrt((V[v] - s3) @ (V[v] - s3)))
    for k in range(3):
        h = 3 * int(face) + k
        t2 = twin[h]
        if t2 >= 0:
            a, ex, ey, L, _, _ = mesh.frame(h)
            push(t2, L - (s3 - a) @ ex, -((s3 - a) @ ey), 0.0, mesh.frame(t2)[3], 0.0)

    while heap:
        count[2] = max(count[2], len(heap))
        _, _, h, v, sx, sy, lo, hi, sigma = heapq.heappop(heap)
        count[1] += 1
        if h < 0:                                           # a pseudo-source vertex
            if sigma > d[v]:
                continue
            for h0 in mesh.out[v]:
                f, k = divmod(h0, 3)
                p, q = int(F[f, (k + 1) % 3]), int(F[f, (k + 2) % 3])
                upd(p, sigma + math.sqrt((V[p] - V[v]) @ (V[p] - V[v])))
                upd(q, sigma + math.sqrt((V[q] - V[v]) @ (V[q] - V[v])))
                h2 = 3 * f + (k + 1) % 3
                t2 = twin[h2]
                if t2 >= 0:
                    _, _, _, L2, cx, cy = mesh.frame(h2)
                    push(t2, L2 - cx, -cy, 0.0, L2, sigma)
            continue
        f, k = divmod(h, 3)
        a, b, c = (int(F[f, (k + i) % 3]) for i in range(3))
        a3, ex, ey, L, cx, cy = mesh.frame(h)
        to_lo, to_hi = math.hypot(sx - lo, sy), math.hypot(sx - hi, sy)
        if d.get(a, math.inf) + hi < sigma + to_hi - FILTER_SLACK:
            continue
        if d.get(b, math.inf) + (L - lo) < sigma + to_lo - FILTER_SLACK:
            continue
        upd(a, sigma + to_lo + lo)
        upd(b, sigma + to_hi + (L - hi))
        eps = EDGE_EPS * L
        for i in on_face.get(f, []):
            tx, ty = (tpoint[i] - a3) @ ex, (tpoint[i] - a3) @ ey
            den = ty - sy
            if den > 0:
                X = sx + (tx - sx) * (-sy) / den
                if lo - eps <= X <= hi + eps:
                    dist[i] = min(dist[i], sigma + math.hypot(tx - sx, ty - sy))
        Xc = sx + (cx - sx) * (-sy) / (cy - sy)
        if lo - eps <= Xc <= hi + eps:
            upd(c, sigma + math.hypot(cx - sx, cy - sy))
        if Xc < hi:
            child(h, (k + 1) % 3, sx, sy, max(lo, Xc), hi, sigma, Xc > lo, False)
        if Xc > lo:
            child(h, (k + 2) % 3, sx, sy, lo, min(hi, Xc), sigma, False, Xc < hi)

    out = np.full(len(tpoint), math.inf)
    for i in cand:
        i = int(i)
        f = int(tface[i])
        best = dist[i]
        if 0 <= f < len(F):
            for k in range(3):
                v = int(F[f, k])
                best = min(best, d.get(v, math.inf) + math.sqrt((V[v] - tpoint[i]) @ (V[v] - tpoint[i])))
        if best <= rmax:
            out[i] = best
    if stats is not None:
        stats["windows"], stats["peak"] = count[1], count[2]
    return out


def geodesic_disks(vertices, faces, tpoint, tface, seed_face, seed_bary, radii, return_dist=False):
    """counts int64 [ns, nr] of targets at geodesic distance <= radii[j] from each seed (and dist [ns, nq])."""
    mesh = vertices if isinstance(vertices, Mesh) else Mesh(vertices, faces)
    radii = np.asarray(radii, np.float64)
    counts = np.zeros((len(seed_face), len(radii)), np.int64)
    dists = np.full((len(seed_face), len(tpoint)), math.inf)
    for s in range(len(seed_face)):
        dists[s] = geodesic_from_seed(mesh, int(seed_face[s]), seed_bary[s], tpoint, tface, float(radii[-1]))
        counts[s] = (dists[s][:, None] <= radii[None, :]).sum(0)
    return (counts, dists) if return_dist else counts


def tool_rows_to_seeds(rows):
    """(faces int64 [n], bary f64 [n,3] in the face's own vertex order) from the tool's rows `id x1 x2 x3`: x1 weighs the face's
    third vertex, x2 its first, x3 its second."""
    rows = np.asarray(rows, np.float64).reshape(-1, 4)
    return rows[:, 0].astype(np.int64), np.stack([rows[:, 2], rows[:, 3], rows[:, 1]], -1)
