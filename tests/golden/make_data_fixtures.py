#!/usr/bin/env python3
"""tests/golden/train_data.npz: what the reference's own dataset classes return for a handful of samples.

Run where the reference tree is present (it never travels; set SAPCU_REFERENCE if it is not at its usual place):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_data_fixtures.py

``fd.datacore.PU1KDataset.__getitem__`` (256 / 1024 points, k = 32; two val samples, two train samples under ``np.random.seed``)
and ``fn.datacore.PU1KMeshDataset.__getitem__`` (512 points, 64 patches, k = 12; one val and one train sample, over three small .off
files written to a temporary directory) are CALLED, not restated.  Stored per sample: the raw inputs, every returned array (patches
as neighbour indices: the maker asserts patches == cloud[idx]), the augmentation draws recovered by replaying the same ``np.random``
calls after re-seeding, the reference's rotation products on their own (an f32 BLAS call: the one step whose rounding order is
not fixed) and the augmented-but-not-normalised arrays, so that the later stages can be checked on exactly the reference's
intermediate.  A seed is redrawn when two of the first k + 1 neighbour distances of any centre are equal (a tree's order
among ties is unspecified; the fixture must not depend on it).  The maker refuses to write unless tests/data_ref.py reproduces every
stored output bit for bit from the recorded intermediate.  Only arrays are stored; the file is written with fixed zip time stamps,
so a second run reproduces it byte for byte."""
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SAPCU_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)
sys.modules.setdefault("h5py", types.ModuleType("h5py"))          # imported by fd/datacore.py, used only by its __init__

import data_ref as R  # noqa: E402
from fd import datacore as fd_data  # noqa: E402
from fn import datacore as fn_data  # noqa: E402

F32 = np.float32
FD_N, FD_G, FD_K = 256, 1024, 32
FN_N, FN_PATCHES, FN_K = 512, 64, 12


def shape_points(rng, count, kind):
    """Points near an analytic surface (a bumpy sphere or a torus), f32 — stand-ins for a Poisson-disc pair."""
    u, v = rng.uniform(0, 2 * np.pi, count), rng.uniform(-1, 1, count)
    if kind == 0:
        r = 0.6 + 0.1 * np.sin(3 * u) * v
        s = np.sqrt(1 - v * v)
        p = np.stack([r * s * np.cos(u), r * s * np.sin(u), r * v], 1)
    else:
        w = rng.uniform(0, 2 * np.pi, count)
        p = np.stack([(0.5 + 0.2 * np.cos(w)) * np.cos(u), (0.5 + 0.2 * np.cos(w)) * np.sin(u), 0.2 * np.sin(w)], 1)
    return (p + np.array([0.3, -0.2, 0.1])).astype(F32)


def tie_free(cloud, centres, k):
    """No two of the first k + 1 neighbour distances of any centre are equal."""
    d, _ = cKDTree(cloud).query(cloud[centres], k=min(k + 1, len(cloud)))
    return bool((np.diff(d, axis=1) > 0).all())


def rotation_of(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=F32)


def indices_of(cloud, centres, patches, k):
    _, idx = cKDTree(cloud).query(cloud[centres], k=k)
    assert np.array_equal(cloud[idx], patches), "patches are not cloud[idx]"
    return idx.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ fd
def fd_dataset(inputs, dense, split):
    ds = fd_data.PU1KDataset.__new__(fd_data.PU1KDataset)            # __init__ only reads h5 files and splits
    ds.inputs, ds.gt, ds.split, ds.k_neighbors, ds.transform = inputs, dense, split, FD_K, None
    return ds


def fd_case(out, name, inputs, dense, i, split, seed):
    ds = fd_dataset(inputs, dense, split)
    while True:
        np.random.seed(seed)
        item = {k: v.numpy() for k, v in ds[i].items()}
        if tie_free(item["cloud"], np.arange(FD_N), FD_K):
            break
        seed += 1000
    rec = {"input_raw": inputs[i], "dense_raw": dense[i], "cloud": item["cloud"], "points": item["points"], "len": item["len"],
           "idx": indices_of(item["cloud"], np.arange(FD_N), item["input"], FD_K)}
    aug_cloud, aug_dense = inputs[i].copy(), dense[i].copy()
    if split == "train":
        np.random.seed(seed)                                          # the same calls in the same order
        theta = np.random.uniform(0, 2 * np.pi)
        scale = np.random.uniform(0.8, 1.2)
        jitter = np.random.normal(0, 0.002, inputs[i].shape).astype(F32)
        rot = rotation_of(theta)
        aug_cloud, aug_dense = aug_cloud @ rot.T, aug_dense @ rot.T   # the reference's own statements
        rec.update(rot_cloud=aug_cloud.copy(), rot_dense=aug_dense.copy())    # its BLAS products on their own
        aug_cloud *= scale
        aug_dense *= scale
        aug_cloud += jitter
        rec.update(theta=np.float64(theta), scale=np.float64(scale), jitter=jitter, rot=rot, aug_cloud=aug_cloud, aug_dense=aug_dense,
                   seed=np.int64(seed))
    want = R.sample(aug_cloud, FD_K, dense=aug_dense)
    for key, ref in (("cloud", "cloud"), ("points", "dense"), ("len", "len"), ("idx", "idx")):
        assert rec[key].dtype == want[ref].dtype and np.array_equal(rec[key], want[ref]), (name, key)
    for k, v in rec.items():
        out["%s/%s" % (name, k)] = v
    print("%-10s seed %-5d len %.4f..%.4f" % (name, seed, rec["len"].min(), rec["len"].max()))


# ------------------------------------------------------------------------------------------------------------------ fn
def icosphere(level=2):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * 0.7, [list(t) for t in f]


def box(sx, sy, sz):
    v = np.array([(x, y, z) for x in (0, sx) for y in (0, sy) for z in (0, sz)], float)
    f = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]       # quads: the loader fans them
    return v, f


def write_off(path, v, f):
    with open(path, "w") as fh:
        fh.write("OFF\n%d %d 0\n" % (len(v), len(f)))
        for p in v:
            fh.write("%.6f %.6f %.6f\n" % tuple(p))
        for face in f:
            fh.write("%d %s\n" % (len(face), " ".join(str(i) for i in face)))


def fn_case(out, name, folder, split, seed):
    ds = fn_data.PU1KMeshDataset(folder, split=split, num_points=FN_N, num_patches=FN_PATCHES, k_neighbors=FN_K)
    vertices, faces = ds._load_off(ds.mesh_files[0])
    while True:
        np.random.seed(seed)
        item = {k: v.numpy() for k, v in ds[0].items()}
        np.random.seed(seed)                                          # the same calls in the same order
        points, normals = ds._sample_points_from_mesh(vertices, faces, FN_N)
        rec = {"points_raw": points.copy(), "normals_raw": normals.copy()}
        aug_cloud, aug_normals = points, normals
        if split == "train":
            theta = np.random.uniform(0, 2 * np.pi)
            scale = np.random.uniform(0.8, 1.2)
            jitter = np.random.normal(0, 0.002, points.shape).astype(F32)
            rot = rotation_of(theta)
            aug_cloud, aug_normals = points @ rot.T, normals @ rot.T
            rec.update(rot_cloud=aug_cloud.copy())                    # its BLAS product on its own (aug_normals is the other)
            aug_cloud *= scale
            aug_cloud += jitter
            rec.update(theta=np.float64(theta), scale=np.float64(scale), jitter=jitter, rot=rot, aug_cloud=aug_cloud,
                       aug_normals=aug_normals)
        centres = np.random.choice(FN_N, FN_PATCHES, replace=False)
        if tie_free(item["cloud"], centres, FN_K):
            break
        seed += 1000
    rec.update(cloud=item["cloud"], all_normals=item["all_normals"], normal=item["normal"], centres=centres.astype(np.int32),
               idx=indices_of(item["cloud"], centres, item["input"], FN_K), seed=np.int64(seed))
    assert np.array_equal(item["all_normals"][centres], item["normal"]), "the replayed centres are not the reference's"
    want = R.sample(aug_cloud, FN_K, normals=aug_normals, centres=centres)
    for key, ref in (("cloud", "cloud"), ("all_normals", "normals"), ("normal", "patch_normals"), ("idx", "idx")):
        assert rec[key].dtype == want[ref].dtype and np.array_equal(rec[key], want[ref]), (name, key)
    for k, v in rec.items():
        out["%s/%s" % (name, k)] = v
    print("%-10s seed %-5d mesh %s" % (name, seed, os.path.basename(ds.mesh_files[0])))


def save_reproducibly(path, arrays):
    """An .npz (np.load reads it) whose bytes depend on the arrays alone: sorted names, one fixed time stamp."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    out = {}
    rng = np.random.default_rng(2024)
    S = 20                                                            # 18 train, 2 val: the reference's 0.9 split
    inputs = np.stack([shape_points(rng, FD_N, s % 2) for s in range(S)])
    dense = np.stack([shape_points(rng, FD_G, s % 2) for s in range(S)])
    split = int(S * 0.9)
    fd_case(out, "fd_val0", inputs[split:], dense[split:], 0, "val", 0)
    fd_case(out, "fd_val1", inputs[split:], dense[split:], 1, "val", 0)
    fd_case(out, "fd_train0", inputs[:split], dense[:split], 0, "train", 11)
    fd_case(out, "fd_train1", inputs[:split], dense[:split], 5, "train", 12)
    with tempfile.TemporaryDirectory() as folder:
        write_off(os.path.join(folder, "a_icosphere.off"), *icosphere())
        write_off(os.path.join(folder, "b_box.off"), *box(1.0, 0.6, 0.4))
        write_off(os.path.join(folder, "c_box.off"), *box(0.5, 0.9, 0.7))        # sorted: two train meshes, one val mesh
        fn_case(out, "fn_train", folder, "train", 21)
        fn_case(out, "fn_val", folder, "val", 22)
    out["cases"] = np.array(sorted({k.split("/")[0] for k in out}))
    path = os.path.join(HERE, "train_data.npz")
    save_reproducibly(path, out)
    print("wrote %s %.1f KiB" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
