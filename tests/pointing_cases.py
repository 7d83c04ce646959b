"""Seeded inputs of the pointing tests (tests/test_pointing_host.py screens them with the definition alone, on the CPU;
tests/test_gpu_pointing.py runs them on the device).  A case is a dict: ``P`` f32 [n,3], the lattice (``origin``, ``step``,
``count``, ``near``), ``sub``, ``k``, ``band``, ``voxels`` (the definition's near_voxels) and ``jitter`` f64 [nv*sub^3,3] or None.
``plain`` cases are screened: no exact tie between the k-th and (k+1)-th neighbour, no d1 within 1e-12 of a band end, no zero len.
The ``made`` cases are built for exactly such properties."""
import functools

import numpy as np

import pointing_ref as R

F32 = np.float32
GRID_MIN_N = 4096              # csrc/knn_grid.h KNN_GRID_MIN_N: below it the automatic route is the brute force


def sphere(n, seed, radius=0.35, noise=0.0):
    rng = np.random.default_rng([17, seed])
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (radius + noise * rng.normal(size=(n, 1)))).astype(F32)


def torus(n, seed):
    """Uneven density and an off-centre, anisotropic box."""
    rng = np.random.default_rng([19, seed])
    u, v = rng.uniform(0, 2 * np.pi, (2, n))
    v = v * v / (2 * np.pi)
    p = np.stack([(0.3 + 0.1 * np.cos(v)) * np.cos(u) + 0.05, (0.3 + 0.1 * np.cos(v)) * np.sin(u) - 0.03, 0.1 * np.sin(v)], 1)
    return p.astype(F32)


def _case(name, P, origin, step, count, sub, k, band, jitter_seed=0, jitter_scale=0.01, near=None, voxels=None):
    P = np.ascontiguousarray(P, dtype=F32)
    near = step + 0.01 if near is None else near
    voxels = R.near_voxels(P, origin, step, count, near) if voxels is None else np.asarray(voxels, dtype=np.int64)
    jitter = None
    if jitter_seed is not None:
        jitter = np.random.default_rng([23, jitter_seed]).random((len(voxels) * sub ** 3, 3)) * jitter_scale
    return {"name": name, "P": P, "origin": origin, "step": step, "count": count, "near": near, "sub": sub, "k": k, "band": band,
            "voxels": voxels, "jitter": jitter}


def geometry(case):
    return {key: case[key] for key in ("origin", "step", "count", "sub", "k", "band")}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The definition's result for the case `name`, computed once per session and shared: treat it as read-only."""
    c = CASES[name]
    return R.export_pointing(c["P"], c["voxels"], c["jitter"], **geometry(c))


def _plain():
    out = [
        # below KNN_GRID_MIN_N: the automatic route is the brute force
        _case("sphere-500", sphere(500, 1), -0.5, 1.0 / 6, 6, 3, 10, (0.02, 0.12), 1),
        # above it: the grid.  The lattice reaches 0.25 beyond the sphere's box on every side
        _case("sphere-5000", sphere(5000, 2), -0.6, 0.15, 8, 3, 10, (0.01, 0.06), 2),
        _case("sphere-5000-k1", sphere(5000, 2), -0.6, 0.2, 6, 2, 1, (0.01, 0.08), 3),
        _case("sphere-5000-k6", sphere(5000, 2), -0.6, 0.2, 6, 2, 6, (0.01, 0.08), 4),
        _case("sphere-5000-k16", sphere(5000, 2), -0.6, 0.2, 6, 2, 16, (0.01, 0.08), 5),
        _case("torus-6000", torus(6000, 3), -0.5, 0.2, 5, 4, 10, (0.005, 0.05), 6),
        _case("noisy-4097-nojitter", sphere(4097, 4, noise=0.01), -0.45, 0.3, 3, 4, 10, (0.003, 0.1), None),
    ]
    return out


def _outward(v, f):
    """Faces of a convex mesh round the origin turned so that their normals point outwards."""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    flip = np.einsum("ij,ij->i", np.cross(b - a, c - a), a + b + c) < 0
    f = f.copy()
    f[flip] = f[flip][:, [0, 2, 1]]
    return v.astype(F32), f.astype(np.int32)


def octasphere(level=2, radius=0.35):
    """A watertight sphere mesh: an octahedron whose faces are split in four `level` times, 8 * 4^level faces."""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.array(p, np.float64) for p in v]
    for _ in range(level):
        mid, g = {}, []

        def half(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = half(a, b), half(b, c), half(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return _outward(np.array(v) * radius, np.array(f))


def box(hx=0.3, hy=0.2, hz=0.25):
    """A watertight box of 12 triangles."""
    v = np.array([[sx * hx, sy * hy, sz * hz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return _outward(v, f)


def lattice(side=12, a=0.125):
    """side^3 points on a lattice of spacing a (exact in f32), centred on 0 for an even side."""
    i = np.arange(side) - side // 2
    g = np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3)
    return (g * a).astype(F32)


def _made():
    # un-jittered queries at the centres of lattice cells (step2 = a, half2 = a / 2): eight points at one distance, so the k-th and
    # (k+1)-th neighbour tie exactly at k = 1 .. 7
    lat = lattice()
    out = [_case("lattice-tie-k%d" % k, lat, -0.5, 0.25, 4, 2, k, (0.0, 1.0), None) for k in (1, 6, 10)]
    # a query whose six nearest points surround it symmetrically: the f32 mean is the query itself, len = 0, a NaN row that stays
    q0 = np.array([-0.0625, -0.0625, -0.0625])
    ring = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) * 0.03125 + q0
    far = sphere(40, 5, radius=0.3)
    out.append(_case("zero-len-k6", np.concatenate([ring, far]), -0.375, 0.25, 3, 2, 6, (0.01, 0.2), None, voxels=[13]))
    out.append(_case("k-equals-n", sphere(7, 6), -0.5, 0.25, 4, 2, 7, (0.0, 1.0), 7))
    out.append(_case("one-point", np.array([[0.01, -0.02, 0.03]]), -0.3, 0.2, 3, 3, 1, (0.05, 0.2), 8))
    dup = sphere(300, 7)
    out.append(_case("duplicates", np.concatenate([dup, dup]), -0.5, 0.25, 4, 2, 9, (0.02, 0.15), 9))
    bad = sphere(200, 8).copy()
    bad[17, 1] = np.nan
    with np.errstate(over="ignore"):
        bad[101, 0] = F32(1e200)                                     # +inf as f32: its squared distance is no candidate either
    bad[150, 2] = -np.inf
    ok = np.isfinite(bad).all(1)
    out.append(_case("non-finite", bad, -0.5, 0.25, 4, 2, 10, (0.02, 0.15), 10, voxels=R.near_voxels(bad[ok], -0.5, 0.25, 4)))
    return out


_BOTH = (_plain(), _made())
PLAIN = tuple(c["name"] for c in _BOTH[0])
MADE = tuple(c["name"] for c in _BOTH[1])
CASES = {c["name"]: c for c in _BOTH[0] + _BOTH[1]}


def screen(name):
    """What the definition says about a case: {ties, band_edge, zero_len, kept, candidates, outside}; outside = the candidates
    reach beyond the cloud's bounding box on all six sides."""
    c, r = CASES[name], reference(name)
    k = c["k"]
    d2 = r["d2"]
    full = r["idx"][:, k - 1] >= 0
    ties = int(np.count_nonzero(full & (d2[:, k - 1] == d2[:, k])))
    edge = int(np.count_nonzero(np.minimum(np.abs(r["d1"] - c["band"][0]), np.abs(r["d1"] - c["band"][1])) <= 1e-12))
    P = c["P"][np.isfinite(c["P"]).all(1)].astype(np.float64)
    outside = bool((r["q"].min(0) < P.min(0)).all() and (r["q"].max(0) > P.max(0)).all())
    return {"ties": ties, "band_edge": edge, "zero_len": int(np.count_nonzero(r["length"] == 0)), "kept": r["count"],
            "candidates": len(r["keep"]), "outside": outside}
