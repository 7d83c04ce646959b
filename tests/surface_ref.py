"""The mesh sampler of include/sapcu_surface.h restated in numpy, one separately rounded operation per step.

It is the reference of tests/test_gpu_surface.py (``==`` on every output) and is itself pinned, bit for bit, to what the reference's
``PU1KMeshDataset._sample_points_from_mesh`` returned (tests/golden/surface_sample.npz, tests/test_surface_host.py).  numpy never
fuses a multiply into an add, so each line below is one operation of the header's list.  The two sums are written out as loops over
their fixed order — ``np_sum_f32`` is what ``ndarray.sum()`` does to a contiguous f32 vector (numpy 2.x), ``np.add.accumulate`` is
sequential by definition — so that nothing here depends on how the installed numpy happens to add."""
import numpy as np

F32, F64 = np.float32, np.float64
BUFSIZE = 8192                   # numpy's default ufunc buffer (np.getbufsize()): sum() adds the pairwise sums of such chunks in sequence


def face_tables(vertices, faces):
    """(normals f32 [F,3], areas f32 [F]) of a mesh (vertices f32 [nv,3], faces int [F,3])."""
    v = np.asarray(vertices, F32)
    f = np.asarray(faces, np.int64)
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    a, b = v1 - v0, v2 - v0
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]],
                 axis=1).astype(F32)
    sq = c * c
    length = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
    normals = c / np.maximum(length, F32(1e-8))[:, None]
    return normals.astype(F32), (F32(0.5) * length).astype(F32)


def np_leaf(a):
    """numpy's pairwise leaf (n <= 128): eight accumulators, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the rest in order."""
    n = len(a)
    if n < 8:
        res = a.dtype.type(0)
        for v in a:
            res = res + v
        return res
    r = a[:8].copy()
    i = 8
    while i < n - n % 8:
        r = r + a[i:i + 8]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[i:]:
        res = res + v
    return res


def np_pairwise(a):
    if len(a) <= 128:
        return np_leaf(a)
    n2 = len(a) // 2
    n2 -= n2 % 8
    return np_pairwise(a[:n2]) + np_pairwise(a[n2:])


def np_sum_f32(a):
    """``a.sum()`` of a contiguous f32 vector: the pairwise sums of BUFSIZE-element chunks, added in sequence from 0."""
    a = np.asarray(a, F32)
    total = F32(0)
    for c0 in range(0, len(a), BUFSIZE):
        total = total + np_pairwise(a[c0:c0 + BUFSIZE])
    return F32(total)


def cdf_table(areas):
    """(cdf f64 [F], area_sum f32, prob_sum f64): the table the legacy ``RandomState.choice(p=areas / (areas.sum() + 1e-8))``
    searches — p widened to f64, a sequential running sum, divided by its last entry."""
    areas = np.asarray(areas, F32)
    total = np_sum_f32(areas)
    denom = F32(total + F32(1e-8))
    p = (areas / denom).astype(F32).astype(F64)
    cdf = np.add.accumulate(p, dtype=F64)
    prob_sum = F64(cdf[-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return cdf / prob_sum, total, prob_sum


def tables(vertices, faces):
    """dict of the per-mesh constants: normals, areas, cdf, area_sum, prob_sum."""
    normals, areas = face_tables(vertices, faces)
    cdf, area_sum, prob_sum = cdf_table(areas)
    return {"normals": normals, "areas": areas, "cdf": cdf, "area_sum": area_sum, "prob_sum": prob_sum}


def select_faces(cdf, u):
    """The number of cdf entries <= u (searchsorted side='right'), clamped to the last face -> int32."""
    face = np.searchsorted(np.asarray(cdf, F64), np.asarray(u, F64), side="right")
    return np.minimum(face, len(cdf) - 1).astype(np.int32)


def sample(vertices, faces, tab, u, r1, r2):
    """(points f32 [n,3], normals f32 [n,3], faces int32 [n]) of one mesh from its tables and the draws u f64, r1 / r2 f32 [n]."""
    v = np.asarray(vertices, F32)
    f = np.asarray(faces, np.int64)
    r1, r2 = np.asarray(r1, F32), np.asarray(r2, F32)
    face = select_faces(tab["cdf"], u)
    s = np.sqrt(r1)
    a = F32(1) - s
    b = s * (F32(1) - r2)
    w = s * r2
    v0, v1, v2 = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    points = (a[:, None] * v0 + b[:, None] * v1) + w[:, None] * v2
    return points.astype(F32), tab["normals"][face], face


def batch(meshes, tabs, mesh_idx, u, r1, r2):
    """The stacked outputs of ``sample`` over a batch: meshes a list of (vertices, faces), tabs their ``tables``, draws [b,n]."""
    outs = [sample(meshes[m][0], meshes[m][1], tabs[m], u[i], r1[i], r2[i]) for i, m in enumerate(mesh_idx)]
    return tuple(np.stack([o[j] for o in outs]) for j in range(3))


def two_block_scan(p, split):
    """A running sum of p computed as two blocks (each summed in sequence, the second one offset by the first one's total): what a
    parallel scan would give.  The host tests show that it is NOT the sequential cdf on the fixture's torus."""
    p = np.asarray(p, F64)
    left = np.add.accumulate(p[:split], dtype=F64)
    right = np.add.accumulate(p[split:], dtype=F64)
    return np.concatenate([left, left[-1] + right])
