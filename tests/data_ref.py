"""The training-sample construction of include/sapcu_data.h restated in numpy, one separately rounded operation per step.

It is the reference of tests/test_gpu_data.py (``==`` on every output) and is itself pinned, bit for bit, to what the reference's
``PU1KDataset.__getitem__`` / ``PU1KMeshDataset.__getitem__`` returned (tests/golden/train_data.npz, tests/test_data_host.py).
numpy never fuses a multiply into an add and evaluates every ufunc call as one rounded operation per element, so each line below
is one operation of the header's list.  Neighbours come from a full distance table and a stable sort, not from a tree: the
(distance, index) order is then defined among ties too."""
import numpy as np

F32 = np.float32


def rotate(p, rot):
    """p [m,3] f32, rot [3,3] f32 row-major -> (x r[i][0] + y r[i][1]) + z r[i][2] (the plain order; the reference's p @ rot.T is a
    BLAS call whose order is not fixed, see tests/test_gpu_data.py for the measured bound between the two)."""
    p, rot = np.asarray(p, F32), np.asarray(rot, F32).reshape(3, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(x * rot[i, 0] + y * rot[i, 1]) + z * rot[i, 2] for i in range(3)], axis=1).astype(F32)


def augment(cloud, dense=None, normals=None, rot=None, scale=None, jitter=None):
    """Rotation on all three, scale on cloud and dense, jitter on the cloud -> (cloud, dense, normals), f32 copies."""
    cloud = np.array(cloud, F32)
    dense = None if dense is None else np.array(dense, F32)
    normals = None if normals is None else np.array(normals, F32)
    if rot is not None:
        cloud = rotate(cloud, rot)
        dense = None if dense is None else rotate(dense, rot)
        normals = None if normals is None else rotate(normals, rot)
    if scale is not None:
        cloud = cloud * F32(scale)
        dense = None if dense is None else dense * F32(scale)
    if jitter is not None:
        cloud = cloud + np.asarray(jitter, F32)
    return cloud, dense, normals


def centroid(cloud):
    """Row 0, + row 1, + ... in f32 (accumulate is sequential by definition), then / (float)n."""
    cloud = np.asarray(cloud, F32)
    return (np.add.accumulate(cloud, axis=0, dtype=F32)[-1] / F32(cloud.shape[0])).astype(F32)


def normalise(cloud, dense=None):
    """-> (cloud, dense, centroid, radius): centred on the cloud's centroid, divided by its largest radius when that is > 0."""
    cloud = np.asarray(cloud, F32)
    c = centroid(cloud)
    cloud = cloud - c
    dense = None if dense is None else np.asarray(dense, F32) - c
    sq = cloud * cloud
    radius = np.max(np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2]))
    if radius > 0:
        cloud = cloud / radius
        dense = None if dense is None else dense / radius
    return cloud, dense, c, F32(radius)


def renormalise(normals):
    n = np.asarray(normals, F32)
    sq = n * n
    return (n / (np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + F32(1e-8))[:, None]).astype(F32)


def dist2(q, pts):
    """[nq, n] f64: ((dx^2 + dy^2) + dz^2) on the f32 coordinates widened to f64."""
    q, pts = np.asarray(q, F32).astype(np.float64), np.asarray(pts, F32).astype(np.float64)
    d = q[:, None, :] - pts[None, :, :]
    d *= d
    return (d[..., 0] + d[..., 1]) + d[..., 2]


def nearest_len(cloud, dense, chunk=512):
    out = np.empty(len(cloud), F32)
    for c0 in range(0, len(cloud), chunk):
        out[c0:c0 + chunk] = np.sqrt(dist2(cloud[c0:c0 + chunk], dense).min(axis=1)).astype(F32)
    return out


def neighbours(cloud, centres, k, chunk=512, want_dist=False):
    """int32 [pc, k]: the k nearest cloud points of cloud[centres[c]] in (distance, index) ascending order (a stable sort by
    distance over ascending indices); with want_dist also the f64 squared distances [pc, k]."""
    centres = np.asarray(centres, np.int64)
    idx = np.empty((len(centres), k), np.int32)
    dist = np.empty((len(centres), k), np.float64)
    for c0 in range(0, len(centres), chunk):
        d2 = dist2(cloud[centres[c0:c0 + chunk]], cloud)
        order = np.argsort(d2, axis=1, kind="stable")[:, :k]
        idx[c0:c0 + chunk] = order
        dist[c0:c0 + chunk] = np.take_along_axis(d2, order, axis=1)
    return (idx, dist) if want_dist else idx


def sample(cloud, k, dense=None, normals=None, rot=None, scale=None, jitter=None, centres=None):
    """One batch entry of sapcu_train_patches_f32 -> dict of every output it can produce (None where the input is absent)."""
    cloud, dense, normals = augment(cloud, dense, normals, rot, scale, jitter)
    cloud, dense, c, radius = normalise(cloud, dense)
    normals = None if normals is None else renormalise(normals)
    centres = np.arange(len(cloud)) if centres is None else np.asarray(centres, np.int64)
    idx = neighbours(cloud, centres, k)
    return {"patches": cloud[idx], "idx": idx, "cloud": cloud, "dense": dense, "len": None if dense is None else nearest_len(cloud, dense),
            "normals": normals, "patch_normals": None if normals is None else normals[centres], "centroid": c, "radius": radius}


def batch(clouds, sample_idx, k, dense=None, normals=None, rot=None, scale=None, jitter=None, centres=None):
    """The stacked outputs of ``sample`` over a batch (data set arrays [S,...], per-entry draws [b,...])."""
    outs = []
    for i, s in enumerate(sample_idx):
        outs.append(sample(clouds[s], k, None if dense is None else dense[s], None if normals is None else normals[s],
                           None if rot is None else rot[i], None if scale is None else scale[i], None if jitter is None else jitter[i],
                           None if centres is None else centres[i]))
    return {key: (None if outs[0][key] is None else np.stack([o[key] for o in outs])) for key in outs[0]}


def rotation_ulps(raw, rot, product):
    """How far ``rotate(raw, rot)`` is from another evaluation of the same product (the reference's BLAS ``raw @ rot.T``), in ulps
    of |x r0| + |y r1| + |z r2| — the magnitude at which either order rounds its products and sums.  (An ulp of the RESULT would
    measure cancellation, not the product: where x cos - y sin is near zero, 6e-8 apart is hundreds of the result's ulps.)"""
    raw, rot = np.asarray(raw, F32), np.asarray(rot, F32).reshape(3, 3)
    a, r = np.abs(raw), np.abs(rot)
    mag = np.stack([(a[:, 0] * r[i, 0] + a[:, 1] * r[i, 1]) + a[:, 2] * r[i, 2] for i in range(3)], axis=1).astype(F32)
    diff = np.abs(rotate(raw, rot).astype(np.float64) - np.asarray(product, F32).astype(np.float64))
    return float((diff / np.spacing(mag).astype(np.float64)).max())
