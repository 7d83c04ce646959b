"""Clouds, queries and the numpy reference of the k-list sweeps (tests/test_klist_host.py checks their conditions without a GPU,
tests/test_gpu_klist.py runs them through the entry points).

Every coordinate is dyadic (an integer / 64, a query an integer / 128), so every squared distance is exact in f64 whatever the
order of its operations, and equal distances are equal bit for bit: which of two tied points comes first is then decided by the
(distance, index) rule alone, at every k.

The reference is ``oracle.geom_path.knn_bruteforce`` (a stable argsort in the kernels' operation order), extended here by the
rule for non-finite distances (csrc/wave_ops.h, include/sapcu.h): a candidate whose squared distance is NaN or +inf is not a
candidate; the list holds the finite ones in (distance, index) order, then empty entries: index -1, distance +inf, a NaN row."""
import functools

import numpy as np

from oracle import geom_path as G

K_MAX = 128
N_QUERIES = 9      # 4 per work group: the last group has idle waves


def _lattice(m, seed):
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    return g[np.random.default_rng(seed).permutation(len(g))] / 64.0


@functools.lru_cache(maxsize=None)
def cloud(name):
    """f64 [n,3], read-only."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "lattice7":                  # a shuffled 7^3 lattice: every distance is tied many times
        c = _lattice(7, 7)
    elif name == "lattice11":               # 1331 points: past KNN_TILE
        c = _lattice(11, 11)
    elif name == "dup4":                    # 80 points, each four times, shuffled: the lower index must come first
        base = rng.integers(0, 64, size=(80, 3)).astype(np.float64) / 64.0
        c = np.tile(base, (4, 1))[rng.permutation(320)]
    elif name == "line":                    # 300 equally spaced collinear points
        c = np.arange(300, dtype=np.float64)[:, None] * np.array([1.0, 2.0, 3.0]) / 64.0
    else:
        raise KeyError(name)
    c.setflags(write=False)
    return c


def dist2(cloud_, queries):
    """[b,n] f64 in the kernels' order, ((dx dx) + (dy dy)) + (dz dz)."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = queries[:, None, 0] - cloud_[None, :, 0]
        dy = queries[:, None, 1] - cloud_[None, :, 1]
        dz = queries[:, None, 2] - cloud_[None, :, 2]
        d = dx * dx
        d = d + dy * dy
        return d + dz * dz


def queries(c, lattice=0):
    """Nine queries of the cloud c: four cloud points; five centres.  A centre is the midpoint of a cloud point and the nearest
    point at another place, both of which are then its nearest points, at one distance: a tie inside the first two distances.  On a
    whole lattice of edge ``lattice`` three of the five are cell centres instead: eight-fold ties."""
    n = len(c)
    own = c[[0, n // 3, n // 2, n - 1]]
    mids = []
    for a in (1 % n, n // 5, (2 * n) // 5, (3 * n) // 5, (4 * n) // 5):
        d = dist2(c, c[a:a + 1])[0]
        d[d == 0] = np.inf
        mids.append((c[a] + c[int(np.argmin(d))]) / 2 if np.isfinite(d).any() else c[a] + 1.0 / 128)
    if lattice:
        for j, cell in enumerate(((0, 0, 0), (lattice - 2, lattice - 2, lattice - 2), (lattice // 2, 1, lattice - 2))):
            mids[j] = (np.array(cell, dtype=np.float64) + 0.5) / 64.0
    q = np.concatenate([own, np.array(mids)])
    assert q.shape == (N_QUERIES, 3)
    return q


def reference(c, q, k):
    """(idx int64 [b,k], dist f64 [b,k], patch f32 [b,k,3]) of knn_gather under the rule for non-finite distances."""
    d2 = dist2(c, q)
    finite = np.isfinite(d2)
    if finite.all():
        idx = G.knn_bruteforce(c, q, k)
    else:
        order = np.argsort(np.where(finite, d2, np.inf), axis=1, kind="stable")[:, :k]
        idx = np.where(np.take_along_axis(finite, order, axis=1), order, -1)
    empty = idx < 0
    safe = np.where(empty, 0, idx)
    dist = np.where(empty, np.inf, np.sqrt(np.take_along_axis(np.where(finite, d2, 0.0), safe, axis=1)))
    with np.errstate(over="ignore", invalid="ignore"):
        patch = G.gather_centre(c, q, safe).astype(np.float32)
    patch[empty] = np.nan
    return idx, dist, patch


def cuts(n_whole, k):
    """The sizes a small cloud runs at for one k: whole, and cut to k, 64 and 65 points (where k fits)."""
    return sorted({n for n in (n_whole, k, 64, 65) if k <= n <= n_whole})


def small_cases():
    """(cloud name, n, k) of the small-cloud sweep: every k in 1..min(128, n)."""
    for name in ("lattice7", "dup4", "line"):
        n_whole = len(cloud(name))
        for k in range(1, min(K_MAX, n_whole) + 1):
            for n in cuts(n_whole, k):
                yield name, n, k


TILE_N = (1023, 1024, 1025, 1331)            # KNN_TILE's edge
TILE_K = (1, 63, 64, 65, 127, 128)


def tile_cases():
    for n in TILE_N:
        for k in TILE_K:
            yield "lattice11", n, k


def grid_cases():
    """(cloud name, k) of the grid sweep: every k in 1..64, the whole cloud is the query set."""
    for name in ("lattice7", "dup4"):
        for k in range(1, 65):
            yield name, k


@functools.lru_cache(maxsize=None)
def cut_with_queries(name, n):
    """(cloud[:n], its nine queries, the reference at the largest k the cut runs at); computed once, read-only."""
    c = cloud(name)[:n]
    whole = n == len(cloud(name))
    q = queries(c, lattice={"lattice7": 7, "lattice11": 11}.get(name, 0) if whole else 0)
    ref = reference(c, q, min(K_MAX, n))
    for a in (q,) + ref:
        a.setflags(write=False)
    return c, q, ref


def reference_at(name, n, k):
    """The reference of one case: the first k columns of the cut's reference (a stable sort's prefix is the shorter sort)."""
    c, q, (idx, dist, patch) = cut_with_queries(name, n)
    return c, q, idx[:, :k], dist[:, :k], patch[:, :k]


def train_cloud():
    """f32 [1,193,3]: the dyadic cloud of the training-patch sweep (193 points: three full slabs and one lane)."""
    rng = np.random.default_rng(193)
    return (rng.integers(0, 9, size=(1, 193, 3)).astype(np.float32) / np.float32(64.0))


# ------------------------------------------------------------------------------------------------- non-finite candidates
BAD_N = (200, 64)
BAD_K = (1, 48, 64, 65, 100, 128)
BAD_KINDS = ("nan5", "nan70", "inf9", "huge11", "nan-query", "huge-query")
BAD_QUERY_ROW = 6


def bad_inputs(kind, n):
    """(cloud [n,3], queries [9,3], clean cloud, clean queries) of one non-finite case on the first n points of lattice7, or None
    where the case does not fit (index 70 of 64 points)."""
    c0, q0, _ = cut_with_queries("lattice7", n)
    c, q = c0.copy(), q0.copy()
    if kind == "nan5":
        c[5, 1] = np.nan                     # in the first slab: through the bitonic network
    elif kind == "nan70":
        if n <= 70:
            return None
        c[70, 0] = np.nan                    # past it: through the insertion
    elif kind == "inf9":
        c[9, 2] = np.inf
    elif kind == "huge11":
        c[11, 0] = 1e200                     # its squared distance overflows to +inf
    elif kind == "nan-query":
        q[BAD_QUERY_ROW] = np.nan            # no finite distance in the row: every entry empty
    elif kind == "huge-query":
        q[BAD_QUERY_ROW] = 1e200
    else:
        raise KeyError(kind)
    return c, q, c0, q0


def bad_cases():
    """(kind, n, k) of the non-finite sweep."""
    for n in BAD_N:
        for kind in BAD_KINDS:
            if bad_inputs(kind, n) is None:
                continue
            for k in BAD_K:
                if k <= n:
                    yield kind, n, k
