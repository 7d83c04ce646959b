"""The definition of this project's PCA normals and normal angles in numpy f64: what csrc/normals.hip computes (include/sapcu_normals.h),
vectorised over rows.  Every elementwise numpy operation below is one rounded f64 operation, in the order the kernel applies it, so
``pca_normals`` equals the device bit for bit on the same neighbour table, and ``angles`` equals the reference's
``angular_error_deg`` (scripts/old_metrics/eval_normals.py) bit for bit with ``oriented=False, clamp_eps=0``.

Also the cloud makers the normal tests share, and brute-force neighbour tables for clouds small enough."""
import numpy as np

SWEEPS = 8
MAX_K = 64
PAIRS = ((0, 1), (0, 2), (1, 2))
EPS = 2.0 ** -52


# ----------------------------------------------------------------------------------------------------------- definition
def covariances(pts, idx):
    """(C f64 [rows,3,3], mean f64 [rows,3]): steps 1 and 2 of the definition; idx int [rows,k] with every entry in [0, n)."""
    pts = np.asarray(pts, dtype=np.float64)
    idx = np.asarray(idx)
    rows, k = idx.shape
    mean = np.zeros((rows, 3))
    for j in range(k):
        mean = mean + pts[idx[:, j]]
    mean = mean / np.float64(k)
    s = np.zeros((rows, 3, 3))
    for j in range(k):
        d = pts[idx[:, j]] - mean
        s = s + d[:, :, None] * d[:, None, :]
    return s / np.float64(k - 1), mean


def jacobi(c, sweeps=SWEEPS, count=None):
    """(diagonal f64 [rows,3], V f64 [rows,3,3]) after `sweeps` cyclic Jacobi sweeps of the symmetric matrices c [rows,3,3]: step 3.
    A pair whose off-diagonal is exactly 0 changes nothing (np.where on every result, so that not even the sign of a zero moves).
    ``count``, a list, receives per sweep the number of rows that rotated in it."""
    a = np.array(c, dtype=np.float64)
    rows = len(a)
    v = np.zeros((rows, 3, 3))
    v[:, 0, 0] = v[:, 1, 1] = v[:, 2, 2] = 1.0
    for _ in range(sweeps):
        rotated = np.zeros(rows, dtype=bool)
        for p, q in PAIRS:
            r = 3 - p - q
            apq = a[:, p, q].copy()
            act = apq != 0.0
            rotated |= act
            with np.errstate(all="ignore"):
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                co = 1.0 / np.sqrt(t * t + 1.0)
                si = t * co
                tap = t * apq
                app, aqq = a[:, p, p] - tap, a[:, q, q] + tap
                arp = co * a[:, r, p] - si * a[:, r, q]
                arq = si * a[:, r, p] + co * a[:, r, q]
                vp = co[:, None] * v[:, :, p] - si[:, None] * v[:, :, q]
                vq = si[:, None] * v[:, :, p] + co[:, None] * v[:, :, q]
            a[:, p, p] = np.where(act, app, a[:, p, p])
            a[:, q, q] = np.where(act, aqq, a[:, q, q])
            a[:, p, q] = a[:, q, p] = np.where(act, 0.0, apq)
            a[:, r, p] = a[:, p, r] = np.where(act, arp, a[:, r, p])
            a[:, r, q] = a[:, q, r] = np.where(act, arq, a[:, r, q])
            v[:, :, p] = np.where(act[:, None], vp, v[:, :, p])
            v[:, :, q] = np.where(act[:, None], vq, v[:, :, q])
        if count is not None:
            count.append(int(rotated.sum()))
    return np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1), v


def smallest(diag, v):
    """(normal f64 [rows,3], evals f64 [rows,3] ascending): step 4, the column under the smallest diagonal entry, the lowest among
    equal ones; the other two entries in column order, swapped when the later one is smaller."""
    rows = np.arange(len(diag))
    col = np.zeros(len(diag), dtype=np.int64)
    lo = diag[:, 0].copy()
    for j in (1, 2):
        less = diag[:, j] < lo
        col = np.where(less, j, col)
        lo = np.where(less, diag[:, j], lo)
    x = np.where(col == 0, diag[:, 1], diag[:, 0])
    y = np.where(col == 2, diag[:, 1], diag[:, 2])
    swap = y < x
    return v[rows, :, col], np.stack([lo, np.where(swap, y, x), np.where(swap, x, y)], axis=1)


def oriented(normal, own, viewpoint=None):
    """Step 5: the sign rule.  own f64 [rows,3] = the row's own point pts[idx[row,0]] (used with a viewpoint only)."""
    if viewpoint is None:
        big = normal[:, 0].copy()
        for j in (1, 2):
            big = np.where(np.abs(normal[:, j]) > np.abs(big), normal[:, j], big)
        flip = big < 0.0
    else:
        vp = np.asarray(viewpoint, dtype=np.float64).reshape(3)
        d = (normal[:, 0] * (vp[0] - own[:, 0]) + normal[:, 1] * (vp[1] - own[:, 1])) + normal[:, 2] * (vp[2] - own[:, 2])
        flip = d < 0.0
    return np.where(flip[:, None], -normal, normal)


def pca_normals(pts, idx, viewpoint=None):
    """(normals f64 [rows,3], evals f64 [rows,3], bad entries): the whole definition on the table idx int64 [rows,k].  A row with an
    entry outside [0, n) is NaN and its bad entries are counted."""
    pts = np.asarray(pts, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    assert idx.ndim == 2 and 3 <= idx.shape[1] <= MAX_K and len(pts) >= 1
    wrong = (idx < 0) | (idx >= len(pts))
    bad_rows = wrong.any(axis=1)
    safe = np.where(bad_rows[:, None], 0, idx)
    c, _ = covariances(pts, safe)
    diag, v = jacobi(c)
    normal, evals = smallest(diag, v)
    normal = oriented(normal, pts[safe[:, 0]], viewpoint)
    normal[bad_rows] = np.nan
    evals[bad_rows] = np.nan
    return normal, evals, int(wrong.sum())


def angles(a, b, is_oriented=False, clamp_eps=0.0):
    """(deg f64 [rows], cos f64 [rows]): the angle of two normal tables in the script's operation order; cos is the clamped dot."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)

    def unit(x):
        norm = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]) + 1e-9
        return x / norm[:, None]

    an, bn = unit(a), unit(b)
    dot = (an[:, 0] * bn[:, 0] + an[:, 1] * bn[:, 1]) + an[:, 2] * bn[:, 2]
    lo, hi = np.float64(-1.0) + np.float64(clamp_eps), np.float64(1.0) - np.float64(clamp_eps)
    dot = np.where(dot < lo, lo, np.where(dot > hi, hi, dot))
    with np.errstate(invalid="ignore"):
        deg = np.arccos(dot if is_oriented else np.abs(dot)) * (180.0 / np.pi)
    return deg, dot


# ------------------------------------------------------------------------------------------------- residuals and bounds
def residual(c, vec, lam):
    """|C v - lam v| per row in np.longdouble, as f64."""
    L = np.longdouble
    cl, vl = np.asarray(c).astype(L), np.asarray(vec).astype(L)
    r = np.einsum("nij,nj->ni", cl, vl) - np.asarray(lam).astype(L)[:, None] * vl
    return np.sqrt((r * r).sum(axis=1)).astype(np.float64)


def sin_angle(u, w):
    """sin of the angle between the rows of u and w (both about unit length)."""
    return np.linalg.norm(np.cross(u, w), axis=1)


# ----------------------------------------------------------------------------------------------------------- the clouds
def shell(n, seed=5, noise=0.002, radius=0.5):
    """(points f64 [n,3], unit radial directions): a noisy sphere shell, the cloud of the committed fixture (same generator calls)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return radius * v + rng.normal(size=(n, 3)) * noise, v


def torus(n, seed=5, noise=0.002, big=0.35, small=0.15):
    rng = np.random.default_rng(seed + 1000)
    u, w = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    ring = big + small * np.cos(w)
    p = np.stack([ring * np.cos(u), ring * np.sin(u), small * np.sin(w)], axis=1)
    return p + rng.normal(size=(n, 3)) * noise


def dyadic_plane(n=1200, seed=7):
    """Distinct points (i/64, j/64, 0.25): every operation of the definition is exact on x and y, z - mean_z is exactly 0."""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(64 * 64)[:n]
    return np.stack([(cells % 64) / 64.0, (cells // 64) / 64.0, np.full(n, 0.25)], axis=1)


def tripled(n=1500, seed=8):
    """Every point of a shell three times, shuffled: at k = 3 each row's neighbours are one position.  The coordinates are multiples
    of 2^-20, so that (p + p + p) / 3 == p and the covariance is exactly zero ((x + x + x) / 3 != x for one f64 in seven)."""
    p = np.round(shell(n, seed)[0] * 2.0 ** 20) / 2.0 ** 20
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.repeat(p, 3, axis=0)[rng.permutation(3 * n)])


def lattice(m=16, seed=9):
    """A shuffled m^3 lattice of spacing 1/m: neighbour distances tie and eigenvalues coincide."""
    g = np.arange(m) / float(m)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(len(p))])


def collinear(n=500, seed=10):
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, n)
    return t[:, None] * np.array([[0.3, -0.5, 0.8]]) + np.array([[0.1, 0.2, -0.3]])


def jacobi_family(n=20000, seed=1):
    """The covariances the sweep count was fixed on: 16 normal points each, axis scales 1e-3 .. 1 (a quarter of them
    flattened by a further 1e-6: anisotropy down to 1e-9), each cloud offset by about 100."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 16, 3)) * rng.uniform(0.001, 1, size=(n, 1, 3))
    x[: n // 4, :, 2] *= 1e-6
    x = x + rng.normal(size=(n, 1, 3)) * 100
    flat = x.reshape(-1, 3)
    return covariances(flat, np.arange(n * 16).reshape(n, 16))[0]


_FIXTURE = {}


def fixture_case(name):
    """One cloud of tests/golden/pca_normals.npz, computed once per session and shared by the host and the device tests: a dict with
    ``points`` (f64 of the script's f32 points), ``script`` (its normals as f64), ``idx`` (brute-force table at the fixture's k),
    ``normals``, ``evals`` (the definition on that table), ``cov`` and ``B``.  Nothing in it is to be modified."""
    if name not in _FIXTURE:
        import os
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca_normals.npz")) as d:
            p = d[name + "/points"].astype(np.float64)
            script, k, b, min_gap = d[name + "/normals"].astype(np.float64), int(d["k"]), float(d["B"]), float(d[name + "/min_gap"])
        idx = brute_knn(p, k)
        normals, evals, bad = pca_normals(p, idx)
        assert bad == 0
        case = {"points": p, "script": script, "idx": idx, "normals": normals, "evals": evals, "cov": covariances(p, idx)[0], "B": b,
                "k": k, "min_gap": min_gap}
        for v in case.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FIXTURE[name] = case
    return _FIXTURE[name]


FIXTURE_GAP = 0.05            # rows with (l1 - l0) / l2 below it are not compared with the script (at most 1 % of a cloud)


def check_against_script(normals, case):
    """The comparison of the definition (or the device) with the reference's output: sin(angle) <= 4 B 2^-23 l2 / (l1 - l0) on every
    row with (l1 - l0) / l2 >= FIXTURE_GAP, at most 1 % of the rows left out.  Returns (worst ratio to the bound, rows left out)."""
    ev = case["evals"]
    gap = (ev[:, 1] - ev[:, 0]) / ev[:, 2]
    take = gap >= FIXTURE_GAP
    left_out = int((~take).sum())
    assert left_out <= 0.01 * len(gap), left_out
    sin = sin_angle(case["script"], normals)
    bound = 4.0 * case["B"] * 2.0 ** -23 / gap
    worst = float((sin[take] / bound[take]).max())
    assert (sin[take] <= bound[take]).all(), worst
    return worst, left_out


def brute_knn(pts, k):
    """Neighbour table int64 [n,k] by (squared distance, index), the order of the device search; for small clouds."""
    pts = np.asarray(pts, dtype=np.float64)
    out = np.empty((len(pts), k), dtype=np.int64)
    for i, q in enumerate(pts):
        d = q - pts
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out[i] = np.lexsort((np.arange(len(pts)), d2))[:k]
    return out
