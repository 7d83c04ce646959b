"""Training batches of fd and fn built on the device from raw cloud pairs.

The reference builds a sample in ``Dataset.__getitem__`` on DataLoader workers with two ``scipy.spatial.cKDTree`` builds —
``fd/datacore.py`` ``PU1KDataset`` (:91-149: augment, normalise by the input cloud, distance of every input point to the denser
cloud, the k nearest input points of every input point) and ``fn/datacore.py`` ``PU1KMeshDataset`` (:201-258: the same on sampled
mesh points with their face normals, 64 random centres).  Here the data set is uploaded once and a whole batch is one call of
``sapcu_train_patches_f32`` (csrc/train_patches.hip, include/sapcu_data.h): three launches, no host read-back.  Given the same
augmentation draws every output equals the reference's bit for bit, up to its BLAS rotation product.

``PU1KPatches`` / ``MeshPatches`` / ``MeshSurfacePatches`` are iterables of stacked batch dicts with the reference's keys; they plug into
``train_step.run_epoch(trainer, loader)`` for ``fd_trainer`` / ``fn_trainer``.  The draws (angle, scale, jitter, centres, order) come
from a device ``torch.Generator`` seeded by (seed, epoch, batch): deterministic, and not the reference's numpy stream.
``FdRayPatches`` yields fd's ray samples of one mesh per item (the reference's ``scripts/sample_mesh-rd.py`` -> ``fd.npz``), sampled
and cast afresh on the device (``ray.sample_fd_rays``).  ``PoissonPU1KPatches`` yields ``PU1KPatches``'s batches from
meshes: both clouds of a sample are Poisson-disk sampled afresh on the device (``poisson.poisson_disk_sample``).
``FnPointingPatches`` and ``FdSeedPatches`` yield the batches of the reference's folder route (``fn/transform.py:Subsamplefn``,
``fd/transform.py:Subsamplerfd``): patches centred on a seed OFF the surface, cut by the calls inference itself makes
(``seed_patches``), from ``pointing.sample_fn_pointing`` and ``FdRayPatches.sample``.

No CPU path: the HIP library and a device are required.
"""
import functools
import math
import os

import numpy as np
import torch

from . import _inputs, _lib, generation, mesh as mesh_mod, pointing as pointing_mod, poisson as poisson_mod, ray as ray_mod, surface

MAX_N, MAX_G, MAX_K = 4096, 65536, 128


def clamp_k(k, n):
    """The neighbour count of a cloud of n points: min(k, n), as the reference's ``min(self.k_neighbors, len(input_pc))``."""
    if int(k) < 1:
        raise ValueError("k: need k >= 1, got %r" % (k,))
    k = min(int(k), int(n))
    if k > MAX_K:
        raise ValueError("k: at most %d neighbours, got %d" % (MAX_K, k))
    return k


def build_patches(clouds, sample_idx, k, dense=None, normals=None, rotation=None, scale=None, jitter=None, centres=None,
                  validate=True):
    """One batch from the device data set ``clouds`` f32 [S,n,3] (``dense`` [S,g,3], ``normals`` [S,n,3] optional).

    ``sample_idx`` int64 [b]: the samples (repeats allowed); ``rotation`` [b,3,3], ``scale`` [b], ``jitter`` [b,n,3]: the
    augmentation of every entry (each optional); ``centres`` int32 [b,pc]: the patch centres, None = every point in order;
    ``k`` is clamped to n as the reference's ``min(k, len)`` does.  -> dict of device tensors: ``patches`` [b,pc,k,3], ``idx``
    int32 [b,pc,k], ``cloud`` [b,n,3], with dense ``dense`` [b,g,3] and ``len`` [b,n], with normals ``normals`` [b,n,3] and
    ``patch_normals`` [b,pc,3].  Index VALUES are checked here (one synchronisation; ``validate=False`` skips it — the kernels
    then leave the rows of a bad index unwritten, NaN): ValueError.  CPU tensors: RuntimeError; bad shapes: ValueError."""
    clouds = _inputs.device_tensor(getattr(clouds, "device", None), "the clouds", clouds, "clouds", torch.float32, (None, None, 3))
    dev_tensor = functools.partial(_inputs.device_tensor, clouds.device, "the clouds", optional=True)
    S, n = clouds.shape[0], clouds.shape[1]
    if S < 1 or not 1 <= n <= MAX_N:
        raise ValueError("clouds: need at least one sample and 1 <= n <= %d points, got %s" % (MAX_N, list(clouds.shape)))
    dense = dev_tensor(dense, "dense", torch.float32, (S, None, 3))
    g = 0 if dense is None else dense.shape[1]
    if dense is not None and not 1 <= g <= MAX_G:
        raise ValueError("dense: need 1 <= g <= %d points, got %d" % (MAX_G, g))
    normals = dev_tensor(normals, "normals", torch.float32, (S, n, 3))
    sample_idx = dev_tensor(sample_idx, "sample_idx", torch.int64, (None,))
    b = sample_idx.shape[0]
    rotation = dev_tensor(rotation, "rotation", torch.float32, (b, 3, 3))
    scale = dev_tensor(scale, "scale", torch.float32, (b,))
    jitter = dev_tensor(jitter, "jitter", torch.float32, (b, n, 3))
    centres = dev_tensor(centres, "centres", torch.int32, (b, None))
    pc = n if centres is None else centres.shape[1]
    if pc < 1:
        raise ValueError("centres: need at least one centre per entry")
    k = clamp_k(k, n)
    if validate and b:
        bad = ((sample_idx < 0) | (sample_idx >= S)).sum()
        if centres is not None:
            bad = torch.stack([bad, ((centres < 0) | (centres >= n)).sum()])
        bad = bad.reshape(-1).tolist()
        if bad[0]:
            raise ValueError("sample_idx: %d indices outside [0, %d)" % (bad[0], S))
        if len(bad) > 1 and bad[1]:
            raise ValueError("centres: %d indices outside [0, %d)" % (bad[1], n))

    dev, nan = clouds.device, float("nan")
    out = {"patches": torch.full((b, pc, k, 3), nan, dtype=torch.float32, device=dev),
           "idx": torch.full((b, pc, k), -1, dtype=torch.int32, device=dev),
           "cloud": torch.full((b, n, 3), nan, dtype=torch.float32, device=dev)}
    if dense is not None:
        out["dense"] = torch.full((b, g, 3), nan, dtype=torch.float32, device=dev)
        out["len"] = torch.full((b, n), nan, dtype=torch.float32, device=dev)
    if normals is not None:
        out["normals"] = torch.full((b, n, 3), nan, dtype=torch.float32, device=dev)
        out["patch_normals"] = torch.full((b, pc, 3), nan, dtype=torch.float32, device=dev)
    if b == 0:
        return out
    ws, nbytes = _lib.workspace("sapcu_train_patches_workspace_bytes", (b,), dev,
                                "sample_idx: a batch of %d entries is outside the range of the call" % b)
    _lib.call("sapcu_train_patches_f32", dev, clouds, S, n, dense, g, normals, sample_idx, b, rotation, scale, jitter, centres, pc, k,
              out["patches"], out["idx"], out["cloud"], out.get("dense"), out.get("len"), out.get("normals"), out.get("patch_normals"),
              ws, nbytes)
    return out


# ------------------------------------------------------------------------------------------------------------ loaders
def split_range(total, split):
    """The reference's split: the first int(0.9 * total) samples train, the rest val (anything else: all)."""
    cut = int(total * 0.9)
    if split == "train":
        return 0, cut
    if split == "val":
        return cut, total
    return 0, total


def _array(x, key, name):
    """A data-set array from a numpy array, a tensor, or a path (.npy; .npz / h5 under the reference's key)."""
    if isinstance(x, (str, os.PathLike)):
        path = os.fspath(x)
        ext = os.path.splitext(path)[1].lower()
        if ext == ".npy":
            x = np.load(path)
        elif ext == ".npz":
            with np.load(path) as z:
                if key not in z:
                    raise ValueError("%s: %s holds no array %r" % (name, path, key))
                x = z[key]
        elif ext in (".h5", ".hdf5"):
            try:
                import h5py
            except ImportError as e:
                raise RuntimeError("%s: reading %s needs h5py, which is not installed (convert to .npz)" % (name, path)) from e
            with h5py.File(path, "r") as f:
                x = f[key][:]
        else:
            raise ValueError("%s: %s is neither .npy, .npz nor .h5" % (name, path))
    if torch.is_tensor(x):
        if not x.dtype.is_floating_point:
            raise ValueError("%s: expected a floating dtype" % name)
        t = x
    else:
        x = np.asarray(x)
        if x.dtype.kind != "f":
            raise ValueError("%s: expected a floating dtype" % name)
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("%s: expected [S, n, 3], got %s" % (name, list(t.shape)))
    return t


class _DeviceLoader(object):
    """What the two loaders share: the split, the resident arrays, the batch order and the augmentation draws."""

    JITTER_SIGMA = 0.002
    SCALE_RANGE = (0.8, 1.2)

    def __init__(self, first, second, names, split, k_neighbors, batch_size, shuffle, augment, seed, device, drop_last):
        a, b = first, second
        if a.shape[0] != b.shape[0]:
            raise ValueError("%s and %s: %d and %d samples" % (names[0], names[1], a.shape[0], b.shape[0]))
        lo, hi = self._configure(a.shape[0], a.shape[1], names[0], split, k_neighbors, batch_size, shuffle, augment, seed, device, drop_last)
        self._a = a[lo:hi].to(device=self.device, dtype=torch.float32).contiguous()       # uploaded once, kept in HBM
        self._b = b[lo:hi].to(device=self.device, dtype=torch.float32).contiguous()

    def _configure(self, total, n, name, split, k_neighbors, batch_size, shuffle, augment, seed, device, drop_last):
        """The checks and settings every loader shares, for a data set of `total` samples of n points -> the split's range."""
        if split not in ("train", "val", "all"):
            raise ValueError("split must be 'train', 'val' or 'all'")
        if int(batch_size) < 1 or int(k_neighbors) < 1:
            raise ValueError("batch_size and k_neighbors must be >= 1")
        if not 1 <= n <= MAX_N:
            raise ValueError("%s: need 1 <= n <= %d points per sample" % (name, MAX_N))
        lo, hi = split_range(total, split)
        if hi <= lo:
            raise ValueError("the %s split of %d samples is empty" % (split, total))
        clamp_k(k_neighbors, n)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("device %s: there is no CPU path" % dev)
        self.split, self.device = split, dev
        self._count, self._n = hi - lo, int(n)
        self.k_neighbors, self.batch_size, self.shuffle = int(k_neighbors), int(batch_size), bool(shuffle)
        self.augment = (split == "train") if augment is None else bool(augment)
        self.seed, self.epoch, self.drop_last = int(seed), 0, bool(drop_last)
        self.last_draws = None                                                    # the draws of the batch yielded last (tests, logs)
        return lo, hi

    @property
    def samples(self):
        return self._count

    def __len__(self):
        return self.samples // self.batch_size if self.drop_last else -(-self.samples // self.batch_size)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        return self

    def _generator(self, batch):
        gen = torch.Generator(device=self.device)
        gen.manual_seed(((self.seed * 1000003 + self.epoch) * 1000003 + batch + 1) & (2 ** 63 - 1))
        return gen

    def _draws(self, gen, b):
        """(rotation [b,3,3], scale [b], jitter [b,n,3], theta [b]) or four None."""
        if not self.augment:
            return None, None, None, None
        dev, n = self.device, self._n
        theta = torch.rand((b,), generator=gen, device=dev, dtype=torch.float64) * (2 * math.pi)
        lo, hi = self.SCALE_RANGE
        scale = (lo + (hi - lo) * torch.rand((b,), generator=gen, device=dev, dtype=torch.float64)).float()
        jitter = torch.randn((b, n, 3), generator=gen, device=dev, dtype=torch.float32) * self.JITTER_SIGMA
        c, s = torch.cos(theta).float(), torch.sin(theta).float()                 # the reference builds its f32 matrix from f64 cos / sin
        rot = torch.zeros((b, 3, 3), dtype=torch.float32, device=dev)
        rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = c, -s, s, c, 1.0
        return rot, scale, jitter, theta

    def __iter__(self):
        order_gen = self._generator(-1)
        S = self.samples
        order = torch.randperm(S, generator=order_gen, device=self.device) if self.shuffle else torch.arange(S, device=self.device)
        for bi in range(len(self)):
            idx = order[bi * self.batch_size:(bi + 1) * self.batch_size].to(torch.int64)
            yield self._batch(idx, self._generator(bi))


class PU1KPatches(_DeviceLoader):
    """The stacked batches of the reference's ``PU1KDataset`` (fd/datacore.py; the data set fd/config.py selects): ``input``
    [B,n,M,3] (M = min(k_neighbors, n)), ``len`` [B,n], ``cloud`` [B,n,3], ``points`` [B,g,3], f32 on the device, plus ``index``
    (the samples' positions in the split).  ``inputs`` [S,256,3] / ``dense`` [S,1024,3]: numpy arrays, tensors, or .npy / .npz (/ .h5
    where h5py imports) paths with the reference's keys ``poisson_256`` / ``poisson_1024``."""

    def __init__(self, inputs, dense, split="train", k_neighbors=32, batch_size=4, shuffle=True, augment=None, seed=0, device=None,
                 drop_last=False):
        a, b = _array(inputs, "poisson_256", "inputs"), _array(dense, "poisson_1024", "dense")
        if not 1 <= b.shape[1] <= MAX_G:
            raise ValueError("dense: need 1 <= g <= %d points per sample" % MAX_G)
        super().__init__(a, b, ("inputs", "dense"), split, k_neighbors, batch_size, shuffle, augment, seed, device, drop_last)

    def _batch(self, idx, gen):
        rot, scale, jitter, theta = self._draws(gen, idx.shape[0])
        self.last_draws = {"theta": theta, "rotation": rot, "scale": scale, "jitter": jitter}
        o = build_patches(self._a, idx, self.k_neighbors, dense=self._b, rotation=rot, scale=scale, jitter=jitter, validate=False)
        return {"input": o["patches"], "len": o["len"], "cloud": o["cloud"], "points": o["dense"], "index": idx}


class MeshPatches(_DeviceLoader):
    """The stacked batches of the reference's ``PU1KMeshDataset`` (fn/datacore.py) from pre-sampled ``points`` [S,n,3] and their
    face ``normals`` [S,n,3] (one fixed sampling per mesh; ``MeshSurfacePatches`` samples the meshes afresh): ``input`` [B,P,k,3], ``normal``
    [B,P,3], ``cloud`` [B,n,3], ``all_normals`` [B,n,3], plus ``centres`` [B,P] and ``index``.  P = num_patches centres drawn per
    sample without replacement, or every point in order when n <= num_patches."""

    def __init__(self, points, normals, split="train", num_patches=64, k_neighbors=12, batch_size=4, shuffle=True, augment=None, seed=0,
                 device=None, drop_last=False):
        a, b = _array(points, "points", "points"), _array(normals, "normals", "normals")
        if a.shape != b.shape:
            raise ValueError("points and normals: shapes %s and %s" % (list(a.shape), list(b.shape)))
        if int(num_patches) < 1:
            raise ValueError("num_patches must be >= 1")
        super().__init__(a, b, ("points", "normals"), split, k_neighbors, batch_size, shuffle, augment, seed, device, drop_last)
        self.num_patches = int(num_patches)

    def _batch(self, idx, gen):
        return self._patches(self._a, self._b, idx, idx, gen, {})

    def _patches(self, points, normals, rows, idx, gen, draws):
        """The augmentation and centre draws, then the batch of rows `rows` of points / normals [*,n,3]; `draws` joins last_draws."""
        b, n = idx.shape[0], self._n
        rot, scale, jitter, theta = self._draws(gen, b)
        centres = None
        if n > self.num_patches:                                                  # a random subset per sample: the first P of a random order
            keys = torch.rand((b, n), generator=gen, device=self.device)
            centres = torch.argsort(keys, dim=1)[:, :self.num_patches].to(torch.int32).contiguous()
        self.last_draws = dict(draws, theta=theta, rotation=rot, scale=scale, jitter=jitter, centres=centres)
        o = build_patches(points, rows, self.k_neighbors, normals=normals, rotation=rot, scale=scale, jitter=jitter, centres=centres,
                          validate=False)
        if centres is None:
            centres = torch.arange(n, dtype=torch.int32, device=self.device).expand(b, n)
        return {"input": o["patches"], "normal": o["patch_normals"], "cloud": o["cloud"], "all_normals": o["normals"],
                "centres": centres, "index": idx}


def mesh_files(folder):
    """The .off files of a mesh folder in the reference's order (fn/datacore.py:37-57): those of the category sub-folders when there
    are any, else the folder's own, sorted by path."""
    import glob
    folder = os.fspath(folder)
    categories = [d for d in os.listdir(folder) if os.path.isdir(os.path.join(folder, d))]
    if categories:
        files = [f for c in categories for f in glob.glob(os.path.join(folder, c, "*.off"))]
    else:
        files = glob.glob(os.path.join(folder, "*.off"))
    if not files:
        raise ValueError("no .off files found in %s" % folder)
    return sorted(files)


def _split_meshes(meshes, configure):
    """(names, pairs) of a split's meshes: ``meshes`` is a list of (vertices, faces) or a folder of ``.off`` files (``mesh_files``;
    polygons are fan-triangulated, vertices taken as f32), ``configure(total)`` gives the split's range [lo, hi)."""
    if isinstance(meshes, (str, os.PathLike)):
        files = mesh_files(meshes)
        lo, hi = configure(len(files))
        names = files[lo:hi]
        pairs = [mesh_mod.read_off(f, triangulate=True) for f in names]
        return names, [(v.astype(np.float32), f) for v, f in pairs]
    meshes = list(meshes)
    lo, hi = configure(len(meshes))
    return ["mesh %d" % i for i in range(lo, hi)], meshes[lo:hi]


class MeshSurfacePatches(MeshPatches):
    """The stacked batches of the reference's ``PU1KMeshDataset`` (fn/datacore.py) from the meshes themselves: every batch draws a NEW
    area-weighted sampling of ``num_points`` surface points with their face normals per mesh (``surface.sample_surface``: one launch),
    then augments, normalises and patches it as ``MeshPatches`` does — the same dict.  ``meshes``: a list of (vertices [nv,3], faces
    [nf,3]) or a folder of ``.off`` files laid out as the reference expects (``mesh_files``; polygons are fan-triangulated, vertices
    taken as f32); the split is the reference's, over the meshes.  The sampling tables are built once, here
    (``surface.build_surface_tables``: ValueError on an empty mesh, a bad face index, a mesh without area).  Per batch the draws are
    ``u`` (f64), ``r1``, ``r2`` (f64 rounded to f32, as the reference rounds them), then the augmentation's and the centres', in the
    reference's call order, all from the (seed, epoch, batch) generator; the val split samples too, without augmenting.
    ``last_draws`` holds them, with the selected ``faces``."""

    def __init__(self, meshes, num_points=512, num_patches=64, k_neighbors=12, split="train", batch_size=4, shuffle=True, augment=None,
                 seed=0, device=None, drop_last=False):
        if int(num_patches) < 1:
            raise ValueError("num_patches must be >= 1")
        names, pairs = _split_meshes(meshes, lambda total: self._configure(total, int(num_points), "num_points", split, k_neighbors, batch_size,
                                                                          shuffle, augment, seed, device, drop_last))
        self.num_patches = int(num_patches)
        self.tables = surface.build_surface_tables(pairs, device=self.device, names=names)

    def _batch(self, idx, gen):
        b, n, dev = idx.shape[0], self._n, self.device
        u = torch.rand((b, n), generator=gen, device=dev, dtype=torch.float64)
        r1 = torch.rand((b, n), generator=gen, device=dev, dtype=torch.float64).float()
        r2 = torch.rand((b, n), generator=gen, device=dev, dtype=torch.float64).float()
        points, normals, faces = surface.sample_surface(self.tables, idx, n, u, r1, r2, validate=False)
        rows = torch.arange(b, dtype=torch.int64, device=dev)
        return self._patches(points, normals, rows, idx, gen, {"u": u, "r1": r1, "r2": r2, "faces": faces})


class PoissonPU1KPatches(_DeviceLoader):
    """``PU1KPatches``'s batches — the data set fd/config.py selects — made from the meshes themselves: per batch entry a NEW
    Poisson-disk cloud of ``num_input`` points and, independently, one of ``num_dense`` points of the same mesh
    (``poisson.poisson_disk_sample``: ``oversample`` times as many area-weighted candidates, thinned to the exact count), then
    ``build_patches`` on the pair; the returned dict is ``PU1KPatches``'s (``input``, ``len``, ``cloud``, ``points``, ``index``).
    ``meshes``: a list of (vertices, faces) or a folder of ``.off`` files, handled and split as ``MeshSurfacePatches`` does, the
    sampling tables built once.

    What differs from the reference's h5 files: these clouds cover WHOLE meshes, not the patches PU-GAN cut from its meshes before
    sampling them, and the random streams are the device generator's, not those of the tool that wrote the files.  Per batch all
    draws come from the (seed, epoch, batch) generator: ``u`` (f64), ``r1``, ``r2`` (f64 rounded to f32) [b, oversample *
    num_input] of the input cloud, then the same for the dense cloud, then the augmentation's.  ``last_draws`` holds them
    (``u_input`` .. ``r2_dense``), with ``radius_*``, ``count_*`` and ``idx_*`` of both selections."""

    STEPS = 20

    def __init__(self, meshes, num_input=256, num_dense=1024, oversample=8, k_neighbors=32, split="train", batch_size=4, shuffle=True,
                 augment=None, seed=0, device=None, drop_last=False):
        if not 1 <= int(num_dense) <= MAX_G:
            raise ValueError("num_dense: need 1 <= num_dense <= %d points" % MAX_G)
        if int(oversample) < 1:
            raise ValueError("oversample must be >= 1")
        names, pairs = _split_meshes(meshes, lambda total: self._configure(total, int(num_input), "num_input", split, k_neighbors, batch_size,
                                                                          shuffle, augment, seed, device, drop_last))
        self.num_dense, self.oversample = int(num_dense), int(oversample)
        self.tables = surface.build_surface_tables(pairs, device=self.device, names=names)

    def _cloud(self, idx, n, gen, tag, draws):
        b, C, dev = idx.shape[0], self.oversample * n, self.device
        u = torch.rand((b, C), generator=gen, device=dev, dtype=torch.float64)
        r1 = torch.rand((b, C), generator=gen, device=dev, dtype=torch.float64).float()
        r2 = torch.rand((b, C), generator=gen, device=dev, dtype=torch.float64).float()
        points, _, _, radius, count, kept = poisson_mod.poisson_disk_sample(self.tables, idx, n, u, r1, r2, steps=self.STEPS, validate=False)
        draws.update({"u_" + tag: u, "r1_" + tag: r1, "r2_" + tag: r2, "radius_" + tag: radius, "count_" + tag: count, "idx_" + tag: kept})
        return points

    def _batch(self, idx, gen):
        draws = {}
        inputs = self._cloud(idx, self._n, gen, "input", draws)
        dense = self._cloud(idx, self.num_dense, gen, "dense", draws)
        rot, scale, jitter, theta = self._draws(gen, idx.shape[0])
        self.last_draws = dict(draws, theta=theta, rotation=rot, scale=scale, jitter=jitter)
        rows = torch.arange(idx.shape[0], dtype=torch.int64, device=self.device)
        o = build_patches(inputs, rows, self.k_neighbors, dense=dense, rotation=rot, scale=scale, jitter=jitter, validate=False)
        return {"input": o["patches"], "len": o["len"], "cloud": o["cloud"], "points": o["dense"], "index": idx}


class FdRayPatches(object):
    """fd's ray samples straight from meshes: one item per mesh of the split, each a FRESH run of the reference's
    ``scripts/sample_mesh-rd.py`` on the device (``ray.sample_fd_rays``: ``num_rays`` surface points thrown out along random unit
    directions by 0.003 .. 0.03 and cast back; the samples whose ray first meets the sampled face at less than 1 rad are kept) — what
    the reference stores once per mesh as ``fd.npz`` and ``fd/field.py:fdField`` loads.  ``meshes``: a list of (vertices [nv,3],
    faces [nf,3]) or a folder of ``.off`` files as for ``MeshSurfacePatches`` (vertices taken as f32).  An item is a dict of f32
    device tensors in ``fdField``'s keys: ``None`` (= ``input`` = ``cloud``) the K kept points [K,3], ``normal`` [K,3] the cast
    directions, ``len`` [K,3] the length repeated per component as the script writes it, plus ``index`` (the mesh) and ``keep``
    (bool [num_rays]).  The draws (``u``, ``r1``, ``r2``, ``g``, ``w``, in this order) come from a device generator seeded by
    (seed, epoch, item): deterministic, and not the reference's streams; ``last_draws`` holds them.  A mesh that is not watertight
    raises ``ValueError`` when it is sampled, unless ``allow_open``."""

    def __init__(self, meshes, num_rays=4096, split="train", shuffle=True, seed=0, device=None, allow_open=False):
        if split not in ("train", "val", "all"):
            raise ValueError("split must be 'train', 'val' or 'all'")
        if int(num_rays) < 1:
            raise ValueError("num_rays must be >= 1")
        if isinstance(meshes, (str, os.PathLike)):
            files = mesh_files(meshes)
            lo, hi = split_range(len(files), split)
            names = files[lo:hi]
            pairs = [mesh_mod.read_off(f, triangulate=True) for f in names]
            pairs = [(v.astype(np.float32), f) for v, f in pairs]
        else:
            meshes = list(meshes)
            lo, hi = split_range(len(meshes), split)
            names, pairs = ["mesh %d" % i for i in range(lo, hi)], meshes[lo:hi]
        if hi <= lo:
            raise ValueError("the %s split is empty" % split)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("device %s: there is no CPU path" % dev)
        self.split, self.device, self.num_rays = split, dev, int(num_rays)
        self.shuffle, self.seed, self.epoch, self.allow_open = bool(shuffle), int(seed), 0, bool(allow_open)
        self.last_draws = None
        self.tables = surface.build_surface_tables(pairs, device=dev, names=names)

    def __len__(self):
        return len(self.tables)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        return self

    def _generator(self, item):
        gen = torch.Generator(device=self.device)
        gen.manual_seed(((self.seed * 1000003 + self.epoch) * 1000003 + item + 1) & (2 ** 63 - 1))
        return gen

    def sample(self, m, item=None, gen=None):
        """The item of mesh m of the split, from the generator of (seed, epoch, item); item None = m.  ``gen``: the draws come from
        this device generator instead."""
        gen = self._generator(int(m) if item is None else int(item)) if gen is None else gen
        n, dev = self.num_rays, self.device
        u = torch.rand((n,), generator=gen, device=dev, dtype=torch.float64)
        r1 = torch.rand((n,), generator=gen, device=dev, dtype=torch.float64).float()
        r2 = torch.rand((n,), generator=gen, device=dev, dtype=torch.float64).float()
        g = torch.randn((n, 3), generator=gen, device=dev, dtype=torch.float64)
        w = torch.rand((n,), generator=gen, device=dev, dtype=torch.float64)
        self.last_draws = {"u": u, "r1": r1, "r2": r2, "g": g, "w": w}
        keep, points, normals, lens = ray_mod.sample_fd_rays(self.tables, int(m), u, r1, r2, g, w, allow_open=self.allow_open)
        return {None: points, "input": points, "cloud": points, "normal": normals, "len": lens.reshape(-1, 1).repeat(1, 3),
                "index": int(m), "keep": keep}

    def __iter__(self):
        S = len(self)
        order = torch.randperm(S, generator=self._generator(-1), device=self.device).tolist() if self.shuffle else list(range(S))
        for item, m in enumerate(order):
            yield self.sample(m, item)


# ------------------------------------------------------------------------------------------------- seed-centred loaders
def seed_patches(cloud_f32, queries, k, normals=None):
    """Patches centred on seeds that need not lie on the cloud, cut by the calls ``Generator3D6._refine_pass`` makes at inference:
    ``generation.knn_gather`` of ``queries`` f64 [P,3] in ``cloud_f32`` [n,3] widened to f64 -> f32 [P,k,3], the k nearest cloud
    points minus the seed; with ``normals`` f32 [P,3] the rows go through ``generation.gather_rotate`` instead, which turns every
    patch so that its normal lies on +x.  Device tensors; k > n: ValueError, as the reference's ``KDTree.query`` raises."""
    dev_tensor = functools.partial(_inputs.device_tensor, getattr(cloud_f32, "device", None), "the cloud")
    if not torch.is_tensor(cloud_f32):
        raise ValueError("cloud: expected a device tensor")
    if not cloud_f32.is_cuda:
        raise RuntimeError("cloud: a CPU tensor (there is no CPU path)")
    cloud = dev_tensor(cloud_f32, "cloud", torch.float32, (None, 3)).double()
    q = dev_tensor(queries, "queries", torch.float64, (None, 3))
    normals = dev_tensor(normals, "normals", torch.float32, (q.shape[0], 3), optional=True)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k: need 1 <= k <= %d, got %d" % (MAX_K, k))
    idx, _, patch = generation.knn_gather(cloud, q, k, want_patch=normals is None)
    return patch if normals is None else generation.gather_rotate(cloud, q, idx, normals)


def _seed_loader_checks(cloud_points, num_patches, k_neighbors):
    if int(num_patches) < 1:
        raise ValueError("num_patches must be >= 1")
    if int(k_neighbors) > int(cloud_points):
        raise ValueError("k_neighbors: %d neighbours of a cloud of %d points" % (int(k_neighbors), int(cloud_points)))


class FnPointingPatches(_DeviceLoader):
    """fn's batches of the reference's folder route, from the meshes themselves: ``fn/transform.py:Subsamplefn`` over what
    ``scripts/sample_mesh-fn.py`` stores per mesh.  Per mesh of the split a surface cloud of ``surface_points`` points and up to
    ``pointing_size`` pointing samples are made ONCE (``pointing.sample_fn_pointing``, on first use, from the generator of (seed,
    mesh); ``resample()`` has them made anew, from other draws); ``geometry`` holds that call's lattice arguments.  A batch entry draws
    ``cloud_points`` rows of the surface cloud and ``num_patches`` samples, both with replacement, and cuts the patches round the
    samples' points (taken as f32, as ``fn/field.py:fnField`` loads them) with ``seed_patches``: ``input`` f32 [B,P,k,3], ``normal``
    f32 [B,P,3] (the pointing directions), ``cloud`` f32 [B,cloud_points,3], ``index`` (the meshes' positions in the split).  The
    draws come from the (seed, epoch, batch) generator, per entry the cloud's rows, then the samples; ``last_draws`` holds them
    (``cloud_idx``, ``sample_idx``) with the ``queries`` f64 [B,P,3].  A mesh without a pointing sample: ValueError."""

    def __init__(self, meshes, surface_points=100000, pointing_size=50000, cloud_points=1024, num_patches=8, k_neighbors=64, split="train",
                 batch_size=4, shuffle=True, seed=0, device=None, drop_last=False, geometry=None):
        _seed_loader_checks(cloud_points, num_patches, k_neighbors)
        if int(surface_points) < 1 or int(pointing_size) < 1:
            raise ValueError("surface_points and pointing_size must be >= 1")
        geometry = dict(geometry or {})
        unknown = sorted(set(geometry) - set(pointing_mod.GEOMETRY))
        if unknown:
            raise ValueError("geometry: unknown arguments %s" % ", ".join(unknown))
        names, pairs = _split_meshes(meshes, lambda total: self._configure(total, int(cloud_points), "cloud_points", split, k_neighbors, batch_size,
                                                                          shuffle, False, seed, device, drop_last))
        self.surface_points, self.pointing_size, self.num_patches = int(surface_points), int(pointing_size), int(num_patches)
        self.geometry, self.names, self._round, self._made = geometry, names, 0, {}
        self.tables = surface.build_surface_tables(pairs, device=self.device, names=names)

    def resample(self):
        """Forget every mesh's surface cloud and pointing samples: the next use makes them from new draws."""
        self._round += 1
        self._made = {}
        return self

    def mesh_samples(self, m):
        """``pointing.sample_fn_pointing``'s dict for mesh m of the split, made on first use."""
        m = int(m)
        if m not in self._made:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(((self.seed * 1000003 + self._round) * 1000003 + m + 500000003) & (2 ** 63 - 1))
            made = pointing_mod.sample_fn_pointing(self.tables, m, self.surface_points, gen, self.pointing_size, **self.geometry)
            if made["points"].shape[0] == 0:
                raise ValueError("%s: no pointing sample (no candidate in the band)" % self.names[m])
            self._made[m] = made
        return self._made[m]

    def _batch(self, idx, gen):
        dev, n, P = self.device, self._n, self.num_patches
        clouds, inputs, normals, cloud_idx, sample_idx, queries = [], [], [], [], [], []
        for m in idx.tolist():
            made = self.mesh_samples(m)
            rows = torch.randint(made["surface"].shape[0], (n,), generator=gen, device=dev)
            pick = torch.randint(made["points"].shape[0], (P,), generator=gen, device=dev)
            cloud = made["surface"][rows]
            q = made["points"][pick].float().double()
            clouds.append(cloud)
            inputs.append(seed_patches(cloud, q, self.k_neighbors))
            normals.append(made["pointing"][pick].float())
            cloud_idx.append(rows)
            sample_idx.append(pick)
            queries.append(q)
        self.last_draws = {"cloud_idx": torch.stack(cloud_idx), "sample_idx": torch.stack(sample_idx), "queries": torch.stack(queries)}
        return {"input": torch.stack(inputs), "normal": torch.stack(normals), "cloud": torch.stack(clouds), "index": idx}


class FdSeedPatches(_DeviceLoader):
    """fd's batches of the reference's folder route, from the meshes themselves: ``fd/transform.py:Subsamplerfd`` over
    ``FdRayPatches.sample``.  A batch entry is a fresh run of the ray sampler on its mesh (``num_rays`` rays), a fresh surface sampling
    of ``cloud_points`` points of the same mesh (``surface.sample_surface``) and ``num_patches`` of the kept rays, drawn with
    replacement; the patches are centred on the rays' origins and turned so that the cast direction lies on +x
    (``seed_patches(..., normals=directions)``): ``input`` f32 [B,P,k,3], ``len`` f32 [B,P], ``cloud`` f32 [B,cloud_points,3],
    ``index``.  Every draw comes from the (seed, epoch, batch) generator, per entry the ray sampler's (``FdRayPatches``), then ``u``,
    ``r1``, ``r2`` of the cloud, then the rays; ``last_draws`` holds ``ray_idx`` with the ``queries`` f64 [B,P,3] and ``directions``
    f32 [B,P,3].  A mesh that is not watertight (unless ``allow_open``) or keeps no ray: ValueError."""

    def __init__(self, meshes, num_rays=4096, cloud_points=2048, num_patches=16, k_neighbors=100, split="train", batch_size=4, shuffle=True,
                 seed=0, device=None, drop_last=False, allow_open=False):
        _seed_loader_checks(cloud_points, num_patches, k_neighbors)
        if int(num_rays) < 1:
            raise ValueError("num_rays must be >= 1")
        # the shared checks first, on a stand-in count: the ray sampler's constructor below already builds tables on the device
        self._configure(10, int(cloud_points), "cloud_points", split, k_neighbors, batch_size, shuffle, False, seed, device, drop_last)
        self.rays = FdRayPatches(meshes, num_rays=num_rays, split=split, shuffle=False, seed=seed, device=device, allow_open=allow_open)
        self._configure(len(self.rays), int(cloud_points), "cloud_points", "all", k_neighbors, batch_size, shuffle, False, seed, self.rays.device,
                        drop_last)
        self.split, self.num_patches, self.tables = split, int(num_patches), self.rays.tables

    def _batch(self, idx, gen):
        dev, n, P = self.device, self._n, self.num_patches
        clouds, inputs, lens, ray_idx, queries, directions = [], [], [], [], [], []
        for m in idx.tolist():
            item = self.rays.sample(m, gen=gen)
            if item["input"].shape[0] == 0:
                raise ValueError("%s: the ray sampler kept no ray" % self.tables.names[m])
            u = torch.rand((1, n), generator=gen, device=dev, dtype=torch.float64)
            r1 = torch.rand((1, n), generator=gen, device=dev, dtype=torch.float64).float()
            r2 = torch.rand((1, n), generator=gen, device=dev, dtype=torch.float64).float()
            entry = torch.full((1,), m, dtype=torch.int64, device=dev)
            cloud = surface.sample_surface(self.tables, entry, n, u, r1, r2, validate=False)[0][0]
            pick = torch.randint(item["input"].shape[0], (P,), generator=gen, device=dev)
            q, d = item["input"][pick].double(), item["normal"][pick].contiguous()
            clouds.append(cloud)
            inputs.append(seed_patches(cloud, q, self.k_neighbors, normals=d))
            lens.append(item["len"][pick, 0])
            ray_idx.append(pick)
            queries.append(q)
            directions.append(d)
        self.last_draws = {"ray_idx": torch.stack(ray_idx), "queries": torch.stack(queries), "directions": torch.stack(directions)}
        return {"input": torch.stack(inputs), "len": torch.stack(lens), "cloud": torch.stack(clouds), "index": idx}
