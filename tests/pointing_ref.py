"""The definition of csrc/sapcu_pointing.h in numpy: the arithmetic of the reference's scripts/sample_mesh-fn.py export_pointing with
the neighbour order of include/sapcu.h ((distance, index) ascending; a NaN or +inf squared distance is no candidate).  Every
operation below is one rounded f64 (or, where said, f32) numpy operation; numpy fuses nothing."""
import numpy as np

F32, F64 = np.float32, np.float64
ROWS = 1024                    # queries per slab of the distance matrix


def dist2(q, P64):
    """[m,n] squared distances accumulated as csrc/wave_ops.h dist2_rn does: ((q-p)_x^2 + (q-p)_y^2) + (q-p)_z^2."""
    dx = q[:, None, 0] - P64[None, :, 0]
    dy = q[:, None, 1] - P64[None, :, 1]
    dz = q[:, None, 2] - P64[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def neighbours(P, q, k):
    """(idx int64 [m,k], dist f64 [m,k], d2 f64 [m,k+1]) of the k nearest rows of P (any float dtype, widened to f64) to every row
    of q, by np.lexsort on (index, squared distance); empty entries are idx -1, dist +inf.  d2 holds the squared distances of the
    k + 1 nearest (+inf where there is none): what the screening of tests/pointing_cases.py looks at."""
    P64 = np.asarray(P).astype(F64)
    q = np.asarray(q, dtype=F64)
    n, m = len(P64), len(q)
    kk = min(k + 1, n)
    idx = np.full((m, k), -1, np.int64)
    d2 = np.full((m, k + 1), np.inf)
    index = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, m, ROWS):
            d = dist2(q[a:a + ROWS], P64)
            d = np.where(d < np.inf, d, np.inf)                      # NaN and +inf: no candidate
            order = np.lexsort((np.broadcast_to(index, d.shape), d), axis=-1)[:, :kk]
            dd = np.take_along_axis(d, order, 1)
            d2[a:a + ROWS, :kk] = dd
            kc = min(k, kk)
            idx[a:a + ROWS, :kc] = np.where(dd[:, :kc] < np.inf, order[:, :kc], -1)
    return idx, np.sqrt(d2[:, :k]), d2


def corners(voxels, origin, step, count):
    """c1 [nv,3] of the voxels v = (ix*count + iy)*count + iz: i*step + origin per axis."""
    v = np.asarray(voxels, dtype=np.int64)
    i = np.stack([v // (count * count), (v // count) % count, v % count], 1)
    return i.astype(F64) * F64(step) + F64(origin)


def centres(origin, step, count):
    """The centres of all count^3 voxels in ascending v."""
    return corners(np.arange(count ** 3), origin, step, count) + F64(step) / 2


def near_voxels(P, origin, step, count, near=None):
    near = step + 0.01 if near is None else near
    _, dist, _ = neighbours(P, centres(origin, step, count), 1)
    return np.flatnonzero(dist[:, 0] < near).astype(np.int64)


def candidates(voxels, origin, step, count, sub, jitter=None):
    """q [nv*sub^3, 3]: ((c1 + jc*step2) + step2/2) + jitter, step2 = step / sub evaluated once in Python."""
    step2 = step / sub
    c1 = corners(voxels, origin, step, count)
    j = np.arange(sub ** 3)
    jc = np.stack([j // (sub * sub), (j // sub) % sub, j % sub], 1)
    q = ((c1[:, None, :] + (jc * step2)[None, :, :]) + step2 / 2).reshape(-1, 3)
    return q if jitter is None else q + np.asarray(jitter, dtype=F64)


def pointing(P32, idx, q):
    """Step 5 for rows whose k neighbours all exist: the f32 sum in list order, the f32 mean, w, len, w / len."""
    P32 = np.asarray(P32, dtype=F32)
    k = idx.shape[1]
    s = P32[idx[:, 0]]
    for j in range(1, k):                                            # (p0 + p1) + p2 ...: f32 additions
        s = s + P32[idx[:, j]]
    mean = s / F32(k)
    w = mean.astype(F64) - q
    length = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        return w / length[:, None], length


def export_pointing(P32, voxels, jitter=None, sub=10, k=10, band=(0.003, 0.03), origin=-1.0, step=0.05, count=50):
    """Steps 2 to 6 -> a dict: keep bool [m], d1 [m], idx int32 [m,k], q [m,3], d2 [m,k+1], and the compacted points, pointing,
    candidate, length (the len of step 5) and count."""
    P32 = np.asarray(P32, dtype=F32)
    q = candidates(voxels, origin, step, count, sub, jitter)
    idx, dist, d2 = neighbours(P32, q, k)
    d1 = dist[:, 0]
    keep = (idx[:, k - 1] >= 0) & (d1 >= band[0]) & (d1 <= band[1])
    rows = np.flatnonzero(keep)
    direction, length = pointing(P32, idx[rows], q[rows]) if len(rows) else (np.zeros((0, 3)), np.zeros((0,)))
    return {"keep": keep, "d1": d1, "idx": idx.astype(np.int32), "q": q, "d2": d2, "points": q[rows], "pointing": direction,
            "candidate": rows.astype(np.int64), "length": length, "count": len(rows)}
