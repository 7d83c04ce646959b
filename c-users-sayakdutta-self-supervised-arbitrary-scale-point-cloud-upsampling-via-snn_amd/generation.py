"""``Generator3D6`` — the reference's upsampling pipeline with its hot loops on the GPU.

Mirrors /root/reference/generation.py:50-187 (same constructor, same ``upsample(data)`` ->
``ndarray [M',3] float64``): outer kNN -> centred patches -> fn normals -> Rodrigues rotation ->
fd distances -> displacement ``p + n*d`` -> kNN-30 outlier filter.  Differences in mechanics,
not in results:

* both reference loops run as ONE device pass: the outer kNN is computed once and its index
  table reused for the fd pass (the reference queries the KD-tree twice for identical answers,
  generation.py:127,153);
* the cloud, seeds and every intermediate stay in HBM; only the refined cloud returns to the host;
* batches follow ``np.array_split(seeds, max(1, n // batch_size))`` exactly, because fn's
  shape-keyed neighbour cache makes results depend on the batch shapes (``knn_cache_mode``).

Seed generation (generation.py:112-118: the ``./dense`` subprocess and its text files) is outside
the GPU hot path; ``upsample`` generates the seeds in process (csrc/dense_seeds.cpp:
same seeds, same order), ``upsample_seeds`` takes a seed array directly.
"""
import math
import os

import numpy as np
import torch

from . import _lib


def split_batches(n, batch_size):
    """(start, end) of each chunk of np.array_split(range(n), max(1, n // batch_size))."""
    pp = max(1, n // batch_size)
    base, extra = divmod(n, pp)
    out, s = [], 0
    for i in range(pp):
        e = s + base + (1 if i < extra else 0)
        out.append((s, e))
        s = e
    return out


def dense_seeds(data, spacing):
    """Seed points of a cloud [N,3] (float64 host array) — in-process equivalent of `./dense spacing N` +
    np.loadtxt("target.xyz") (generation.py:114-118): same seeds, same order, same 6-decimal values."""
    import ctypes
    lib = _lib.load()
    cloud = np.ascontiguousarray(data, dtype=np.float64)
    cap = max(1 << 16, 128 * cloud.shape[0])
    while True:
        out = np.empty((cap, 3), dtype=np.float64)
        n = ctypes.c_int64(0)
        rc = lib.sapcu_dense_seeds_host(cloud.ctypes.data, cloud.shape[0], float(spacing), out.ctypes.data, cap,
                                        ctypes.byref(n))
        if rc == -2:                       # buffer too small: n holds the required count
            cap = int(n.value)
            continue
        _lib.check(rc)
        return out[: n.value].copy()


def seed_voxel_estimate(n, spacing):
    """First guess of the voxels a flood meets: a shell of thickness 0.03 + 2 cells (the band reaches 0.015 to either side of the
    surface and one ring beyond) around a surface of area 6 (a unit-cube-sized shape; a unit sphere has 3.14 and meets 1.76 M voxels
    at 0.004 against the 3.6 M of this formula).  Only a starting size: dense_seeds_device doubles it when the flood reports more."""
    cell = float(spacing)
    return int(min(max(6.0 * (0.03 + 2.0 * cell) / cell ** 3, 1 << 16, 8 * int(n)), 1 << 26))


def dense_seeds_device(data, spacing, device, max_voxels=None, capacity=None, stats=None):
    """``dense_seeds`` on the device (csrc/dense_seeds_dev.hip): the same seeds in the same order with the same 6-decimal values,
    as a torch f64 [n,3] tensor on ``device``.  ``data``: [N,3] host array or device tensor.  ``max_voxels`` / ``capacity``: starting
    sizes of the voxel table and the seed buffer (defaults: seed_voxel_estimate, and a quarter of it); both grow on
    SAPCU_ERR_WORKSPACE and the flood runs again.  ``stats``, a list, receives [levels, voxels evaluated, voxels recomputed on the
    host, table slots] of the run that succeeded."""
    import ctypes
    lib = _lib.load()
    dev = torch.device(device)
    if torch.is_tensor(data):
        cloud = data.to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()
    else:
        cloud = torch.as_tensor(np.ascontiguousarray(data, dtype=np.float64).reshape(-1, 3), device=dev)
    n = cloud.shape[0]
    maxv = int(max_voxels) if max_voxels is not None else seed_voxel_estimate(n, spacing)
    cap = int(capacity) if capacity is not None else max(1 << 16, maxv // 4)
    while True:
        nbytes = int(lib.sapcu_dense_seeds_workspace_bytes(n, maxv))
        if nbytes < 0:
            raise ValueError("dense_seeds_device: n=%d, max_voxels=%d out of range" % (n, maxv))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        out = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        count = ctypes.c_int64(0)
        st = (ctypes.c_int64 * 4)()
        with torch.cuda.device(dev):
            rc = lib.sapcu_dense_seeds_f64(_lib.ptr(cloud), n, float(spacing), _lib.ptr(out), cap, maxv, ctypes.byref(count), st,
                                           _lib.ptr(ws), nbytes, _lib.current_stream())
        if rc == -2:
            if count.value > cap:          # every seed was counted: the required size
                cap = int(count.value)
            else:                          # the voxel table was full
                maxv *= 2
            del ws, out
            continue
        _lib.check(rc)
        if stats is not None:
            stats[:] = list(st)
        return out[: count.value].clone()


def require_finite(name, arr):
    """sklearn's KDTree(data) and .query(q) raise ValueError on NaN or infinity (generation.py:110,127).  The entries that are
    handed a host array (Generator3D6.generateiopoint / upsample_seeds, dist.upsample_cloud_sharded) do the same on that array,
    before any launch; knn_gather and refine work on device tensors and follow the rule of include/sapcu.h instead."""
    if not np.isfinite(arr).all():
        raise ValueError("%s contains NaN or infinity" % name)


def knn_gather(cloud_dev, queries_dev, k, want_dist=False, want_patch=True):
    """Outer kNN on the device: (idx int64 [b,k], dist f64 [b,k] | None, patch f32 [b,k,3] | None).  No host check and no
    synchronisation: a cloud point at a NaN or +inf distance is no candidate, and a query with fewer than k finite distances
    gets empty entries behind them (idx -1, dist +inf, a NaN patch row), see include/sapcu.h."""
    lib = _lib.load()
    b, n = queries_dev.shape[0], cloud_dev.shape[0]
    if k > n:      # sklearn's KDTree.query raises the same way (generation.py:127)
        raise ValueError("k must be less than or equal to the number of training points (k=%d, N=%d)" % (k, n))
    dev = cloud_dev.device
    idx = torch.empty((b, k), dtype=torch.int64, device=dev)
    dist = torch.empty((b, k), dtype=torch.float64, device=dev) if want_dist else None
    patch = torch.empty((b, k, 3), dtype=torch.float32, device=dev) if want_patch else None
    with torch.cuda.device(dev):
        _lib.check(lib.sapcu_knn_gather_f64(_lib.ptr(cloud_dev), n, _lib.ptr(queries_dev), b, k, _lib.ptr(idx),
                                            _lib.ptr(dist), _lib.ptr(patch), _lib.current_stream()))
    return idx, dist, patch


def knn_self_grid(pts_dev, k, rows=None, cell_size=0.0, info=None):
    """Exact kNN of rows [row0, row1) of a point set f64 [n,3] against the whole set on a device cell grid
    (csrc/knn_grid.hip): (idx int64 [rows,k], dist f64 [rows,k]), bit for bit ``knn_gather(pts, pts[row0:row1], k,
    want_dist=True)``.  k <= 64; ``cell_size`` 0 = automatic (any value gives the same result).  ``info``, a list, receives
    [1 if the grid ran else 0 (brute force), gx, gy, gz].  Synchronises the current stream once (the grid size is read back)."""
    import ctypes
    lib = _lib.load()
    n = pts_dev.shape[0]
    r0, r1 = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
    if k > n:
        raise ValueError("k must be less than or equal to the number of training points (k=%d, N=%d)" % (k, n))
    pts_dev = pts_dev.contiguous()
    dev = pts_dev.device
    idx = torch.empty((r1 - r0, k), dtype=torch.int64, device=dev)
    dist = torch.empty((r1 - r0, k), dtype=torch.float64, device=dev)
    nbytes = int(lib.sapcu_knn_grid_workspace_bytes(n))
    ws = torch.empty((max(nbytes, 0),), dtype=torch.uint8, device=dev)
    out = (ctypes.c_int64 * 4)()
    with torch.cuda.device(dev):
        _lib.check(lib.sapcu_knn_self_grid_f64(_lib.ptr(pts_dev), n, r0, r1, k, float(cell_size), _lib.ptr(idx), _lib.ptr(dist),
                                               _lib.ptr(ws), nbytes, out, _lib.current_stream()))
    if info is not None:
        info[:] = list(out)
    return idx, dist


# -- the kNN-30 outlier filter on the device (generation.py:176-183).  Its keep decision is the f64 comparison
#    mean(row) < mean(all) * threshold, rounded as numpy 2.x's np.mean rounds (csrc/knn_grid.hip: row means = numpy's pairwise
#    leaf; the global sum = pairwise sums of np.getbufsize()-element chunks of the flattened [n, kk] table, added in sequence).
OUTLIER_K = 30


def outlier_row_align(kk, bufsize=None):
    """Rows per aligned block: a row range starting on a multiple of it (and ending on one, or at n) holds whole chunks of np.mean."""
    bufsize = np.getbufsize() if bufsize is None else int(bufsize)
    return bufsize // math.gcd(max(int(kk), 1), bufsize)


def outlier_chunk_count(rows, kk, bufsize=None):
    """Number of np.mean chunks in `rows` rows of a [*, kk] table that start on a chunk boundary."""
    bufsize = np.getbufsize() if bufsize is None else int(bufsize)
    return -(-int(rows) * int(kk) // bufsize)


def outlier_stats_device(dist_dev, bufsize=None):
    """(row means f64 [rows], chunk sums f64 [chunks]) of a distance table f64 [rows, kk] on the device, in numpy's order."""
    lib = _lib.load()
    bufsize = np.getbufsize() if bufsize is None else int(bufsize)
    dist_dev = dist_dev.contiguous()
    rows, kk = dist_dev.shape
    mean = torch.empty((rows,), dtype=torch.float64, device=dist_dev.device)
    sums = torch.empty((outlier_chunk_count(rows, kk, bufsize),), dtype=torch.float64, device=dist_dev.device)
    with torch.cuda.device(dist_dev.device):
        _lib.check(lib.sapcu_outlier_stats_f64(_lib.ptr(dist_dev), rows, kk, bufsize, _lib.ptr(mean), _lib.ptr(sums),
                                               _lib.current_stream()))
    return mean, sums


def outlier_global_mean(chunk_sums, count):
    """np.mean's total: the chunk sums (all of them, in order) added in sequence from 0.0 on the host, over the element count."""
    total = 0.0
    for s in chunk_sums.tolist():
        total += s
    return total / count


def outlier_keep_device(row_mean_dev, mean, threshold):
    """Device bool mask row_mean < mean * threshold (f64 product)."""
    lib = _lib.load()
    keep = torch.empty(row_mean_dev.shape, dtype=torch.bool, device=row_mean_dev.device)
    with torch.cuda.device(row_mean_dev.device):
        _lib.check(lib.sapcu_outlier_keep_f64(_lib.ptr(row_mean_dev), row_mean_dev.shape[0], float(mean), float(threshold),
                                              _lib.ptr(keep), _lib.current_stream()))
    return keep


def outlier_filter_range(n, rows, bufsize=None):
    """Checked (start, end) of a row range of the outlier filter over n points: an empty range, or one whose start and end
    (unless end = n) are multiples of ``outlier_row_align(min(30, n))`` rows — then it holds whole chunks of np.mean."""
    r0, r1 = int(rows[0]), int(rows[1])
    align = outlier_row_align(min(OUTLIER_K, n), bufsize)
    if not (0 <= r0 <= r1 <= n) or (r1 > r0 and (r0 % align or (r1 % align and r1 != n))):
        raise ValueError("outlier filter: rows [%d, %d) of %d are not aligned to %d-row blocks" % (r0, r1, n, align))
    return r0, r1


def outlier_filter_device(pts_dev, threshold, rows=None, gather_sums=None):
    """Keep mask of the kNN-30 outlier filter (generation.py:176-183) computed on the device: bool [n] on the device, equal to
    ``Generator3D6.outlier_filter``'s host result.

    For a row range ``rows = (start, end)`` (checked by ``outlier_filter_range``; may be empty) only those rows are searched:
    returns (keep bool [end-start] on the device, this range's chunk sums).  ``gather_sums(local_sums)`` must return the chunk
    sums of ALL rows in order (e.g. an all-gather over ranks, sapcu_amd/dist.py) and is called for an empty range too; without
    it the range must be all rows."""
    n = pts_dev.shape[0]
    kk = min(OUTLIER_K, n)
    bufsize = np.getbufsize()
    r0, r1 = (0, n) if rows is None else outlier_filter_range(n, rows, bufsize)
    if gather_sums is None and (r0, r1) != (0, n):
        raise ValueError("outlier_filter_device: a part of the rows needs gather_sums (the global mean covers every row)")
    _, dist = knn_self_grid(pts_dev, kk, (r0, r1))
    row_mean, sums = outlier_stats_device(dist, bufsize)
    all_sums = sums if gather_sums is None else gather_sums(sums)
    keep = outlier_keep_device(row_mean, outlier_global_mean(all_sums.cpu(), n * kk), threshold)
    return keep if rows is None else (keep, sums)


def gather_rotate(cloud_dev, queries_dev, idx, normals):
    lib = _lib.load()
    b, k = idx.shape
    patch = torch.empty((b, k, 3), dtype=torch.float32, device=cloud_dev.device)
    with torch.cuda.device(cloud_dev.device):
        _lib.check(lib.sapcu_gather_rotate_f64(_lib.ptr(cloud_dev), cloud_dev.shape[0], _lib.ptr(queries_dev), b,
                                               _lib.ptr(idx), k, _lib.ptr(normals), _lib.ptr(patch),
                                               _lib.current_stream()))
    return patch


def displace(queries_dev, normals, dist):
    lib = _lib.load()
    out = torch.empty_like(queries_dev)
    with torch.cuda.device(queries_dev.device):
        _lib.check(lib.sapcu_displace_f64(_lib.ptr(queries_dev), _lib.ptr(normals), _lib.ptr(dist),
                                          queries_dev.shape[0], _lib.ptr(out), _lib.current_stream()))
    return out


def l2_normalize3(x):
    lib = _lib.load()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(lib.sapcu_l2_normalize3(_lib.ptr(x), _lib.ptr(out), x.shape[0], _lib.current_stream()))
    return out


class Generator3D6(object):
    def __init__(self, model1, model2, device, k_neighbors=100, dense_spacing=0.004, outlier_threshold=1.5,
                 batch_size=400):
        self.model1 = model1        # fn: normals
        self.model2 = model2        # fd: distances
        self.device = torch.device(device)
        self.k_neighbors = k_neighbors
        self.dense_spacing = dense_spacing
        self.outlier_threshold = outlier_threshold
        self.batch_size = batch_size
        self.model1.eval()
        self.model2.eval()
        if self.device.type != "cuda":
            raise RuntimeError("Generator3D6 needs a ROCm device (got %s): no CPU path exists" % self.device)
        if not (1 <= k_neighbors <= 128):
            raise ValueError("k_neighbors must be in 1..128")

    # -- public, as the reference -------------------------------------------------------------
    def upsample(self, data):
        return self.generateiopoint(data)

    def generateiopoint(self, data):
        data = np.squeeze(data, 0) if np.ndim(data) == 3 else np.asarray(data)
        require_finite("the cloud", data)
        seeds = self._dense_seeds(data)
        return self.upsample_seeds(data, seeds)

    # -- seed generation (generation.py:112-118).  Default: in process (csrc/dense_seeds.cpp), identical seeds in
    #    identical order.  seed_source = "subprocess" keeps the reference's mechanics verbatim: os.system("./dense")
    #    in the working directory, which reads test.xyz and writes target.xyz.  "device": the same flood on the GPU
    #    (dense_seeds_device), the seeds stay in HBM and go to the refine as a device tensor.
    seed_source = "inprocess"

    def _dense_seeds(self, data):
        if self.seed_source == "inprocess":
            return dense_seeds(data, self.dense_spacing)
        if self.seed_source == "device":
            return dense_seeds_device(data, self.dense_spacing, self.device)
        if not os.path.exists("./dense"):
            raise FileNotFoundError("./dense not found in the working directory: the reference shells out to it "
                                    "(generation.py:114-116)")
        os.system("./dense %s %d" % (self.dense_spacing, data.shape[0]))
        return np.loadtxt("target.xyz")[:, 0:3]

    # -- the hot path --------------------------------------------------------------------------
    # Several reference batches run as ONE device pass of up to `fuse_queries` seeds: every kernel is per-patch (results do
    # not depend on which patches share a launch — tests/test_gpu_parity.py::test_chunking...), and the one coupling the
    # reference has between batches, fn's shape-keyed neighbour cache, is reproduced by handing the cached tables of the
    # first batch of a shape to all later batches of that shape.  Same refined cloud, bit for bit, as batch by batch;
    # the reference's default batch sizes (256-400) then run at the speed of large batches.  0 = one pass per batch.
    fuse_queries = 4096

    def _refine_pass(self, cloud_dev, q, knn_in=None):
        k = self.k_neighbors
        idx, _, patch = knn_gather(cloud_dev, q, k)
        if hasattr(self.model1, "reset_states"):
            self.model1.reset_states()
        raw = self.model1(patch, knn_in=knn_in) if knn_in is not None else self.model1(patch)
        nrm = l2_normalize3(raw)                                 # generation.py:138-139
        rot = gather_rotate(cloud_dev, q, idx, nrm)              # generation.py:154-160
        if hasattr(self.model2, "reset_states"):
            self.model2.reset_states()
        d = self.model2(rot)                                     # generation.py:169
        return displace(q, nrm, d), nrm, d                       # generation.py:171-172

    def refine(self, cloud_dev, seeds_dev):
        """Device pipeline on resident tensors: cloud f64 [N,3], seeds f64 [n,3] ->
        (refined f64 [n,3], normals f32 [n,3], dist f32 [n]).  Batch boundaries as the reference."""
        n = seeds_dev.shape[0]
        k = self.k_neighbors
        out = torch.empty((n, 3), dtype=torch.float64, device=cloud_dev.device)
        normals = torch.empty((n, 3), dtype=torch.float32, device=cloud_dev.device)
        dists = torch.empty((n,), dtype=torch.float32, device=cloud_dev.device)
        batches = split_batches(n, self.batch_size)
        mode = getattr(self.model1, "knn_cache_mode", None)
        can_fuse = self.fuse_queries and mode in ("reference", "fresh") and hasattr(self.model1, "tiled_knn_tables")
        i = 0
        while i < len(batches):
            s, e = batches[i]
            size = e - s
            j = i + 1
            if can_fuse:
                if mode == "reference" and (size, k) not in self.model1._knn_cache:
                    j = i + 1                                    # first batch of this shape: alone, it fills the cache
                else:
                    per = max(1, self.fuse_queries // max(size, 1))
                    while j < len(batches) and j - i < per and batches[j][1] - batches[j][0] == size:
                        j += 1
            e = batches[j - 1][1]
            knn_in = None
            if can_fuse and mode == "reference" and j - i > 1:
                knn_in = self.model1.tiled_knn_tables(size, k, j - i)
            out[s:e], normals[s:e], dists[s:e] = self._refine_pass(cloud_dev, seeds_dev[s:e], knn_in)
            i = j
        return out, normals, dists

    def check_numeric_guards(self):
        """Raise if a kernel-side assumption was violated during the forwards so far: an activation beyond the f16
        range of the split-f16 GEMMs, or an open refractory gate in fd (both counted on the device)."""
        for name, m in (("fn", self.model1), ("fd", self.model2)):
            if hasattr(m, "gemm_mode"):
                split, ovf = m.gemm_mode()
                if ovf:
                    raise RuntimeError("%s: %d activation values left the f16 range of the split-f16 GEMMs; "
                                       "set SAPCU_GEMM=f32 for exact-f32 kernels" % (name, ovf))
            if hasattr(m, "gate_violations") and m.gate_violations():
                raise RuntimeError("%s: refractory gate found open at t >= 1 (%d events)" % (name, m.gate_violations()))

    # -- the outlier filter (generation.py:176-183).  "host" (default): the kNN on the outer-kNN kernel, both means in numpy on
    #    the host.  "device": outlier_filter_device — grid kNN and the means in numpy's order on the device, the same keep set.
    outlier_filter_impl = "host"

    def outlier_filter(self, pts_dev):
        """Keep points whose mean distance to their 30 nearest (self included) is below
        outlier_threshold x the global mean (generation.py:176-183)."""
        if self.outlier_filter_impl == "device":
            return outlier_filter_device(pts_dev, self.outlier_threshold).cpu().numpy()
        if self.outlier_filter_impl != "host":
            raise ValueError("outlier_filter_impl must be 'host' or 'device' (got %r)" % (self.outlier_filter_impl,))
        kk = min(30, pts_dev.shape[0])
        _, dist, _ = knn_gather(pts_dev, pts_dev, kk, want_dist=True, want_patch=False)
        # the two means are host numpy on purpose: they decide membership by a float64 comparison and
        # must round exactly like np.mean does in the reference (this row is post-processing, §8f-3)
        dist = dist.cpu().numpy()
        keep = np.mean(dist, axis=1) < np.mean(dist) * self.outlier_threshold
        return keep

    def outlier_filter_rows(self, pts_dev, rows, gather_sums):
        """One rank's aligned rows of the device outlier filter (sapcu_amd/dist.py): (keep bool [rows] on the device, chunk sums)."""
        return outlier_filter_device(pts_dev, self.outlier_threshold, rows, gather_sums)

    def upsample_seeds(self, data, seeds, return_unfiltered=False):
        data = np.ascontiguousarray(data, dtype=np.float64)
        require_finite("the cloud", data)
        if not torch.is_tensor(seeds):
            seeds = np.ascontiguousarray(seeds, dtype=np.float64)
            require_finite("the seeds", seeds)
        cloud_dev = torch.as_tensor(data, device=self.device)
        if torch.is_tensor(seeds):          # seed_source = "device": already in HBM (flooded from the checked cloud)
            seeds_dev = seeds.to(device=self.device, dtype=torch.float64).contiguous()
        else:
            seeds_dev = torch.as_tensor(seeds, device=self.device)
        if seeds_dev.shape[0] == 0:        # nothing in the distance band (the reference fails inside np.loadtxt here)
            empty = np.zeros((0, 3), dtype=np.float64)
            return (empty, empty) if return_unfiltered else empty
        with torch.no_grad():
            refined, _, _ = self.refine(cloud_dev, seeds_dev)
            keep = self.outlier_filter(refined)
        self.check_numeric_guards()
        refined = refined.cpu().numpy()
        if return_unfiltered:
            return refined[keep], refined
        return refined[keep]


class SNNPointCloudGenerator(Generator3D6):
    """Multi-pass wrapper (generation.py:191-220)."""

    def __init__(self, model1, model2, device, **kwargs):
        self.upsampling_ratio = kwargs.pop("upsampling_ratio", 4)
        super().__init__(model1, model2, device, **kwargs)

    def multi_scale_upsample(self, data, num_passes=1):
        result = data
        for _ in range(num_passes):
            result = self.upsample(np.expand_dims(result, 0) if result.ndim == 2 else result)
        return result
