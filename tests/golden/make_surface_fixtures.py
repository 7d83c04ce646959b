#!/usr/bin/env python3
"""tests/golden/surface_sample.npz: what the reference's own mesh sampler returns for four small meshes.

Run where the reference tree is present (it never travels; set SAPCU_REFERENCE if it is not at its usual place):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_surface_fixtures.py

``fn.datacore.PU1KMeshDataset._load_off``, ``_sample_points_from_mesh`` (512 points per mesh under ``np.random.seed``) and
``__getitem__`` (512 points, 64 patches, k = 12; one train and one val sample) are CALLED, not restated, on four ``.off`` files
written to a temporary directory: an icosphere (320 faces), a torus of 5000 faces whose areas spread over eleven orders of magnitude, a
mesh with zero-area faces at the first, a middle and the last position, and a box of quads, a pentagon, triangles and one two-corner
face (the loader fans the polygons and drops the last).  Stored per mesh: the loaded vertices and faces, the draws ``u`` (f64), ``r1``, ``r2`` (f32) recovered by replaying the
same ``np.random`` calls after re-seeding, the selected faces, the points and the normals.  Stored per ``__getitem__`` case: the
same, the augmentation draws, the reference's rotation products and augmented arrays (the rotation is an f32 BLAS call, the one step
whose rounding order is not fixed: the later stages are checked from the reference's own intermediate, as in train_data.npz), the
centres and every returned array.  The text of the polygon file is stored as bytes, for ``read_off(triangulate=True)``.

The maker refuses to write unless tests/surface_ref.py, followed by tests/data_ref.py, reproduces every stored array bit for bit,
and unless the torus shows what the host tests assert about it (a two-block scan and a sequential f32 sum both differ from numpy's
order).  Only arrays are stored; the file is written with fixed zip time stamps, so a second run reproduces it byte for byte."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SAPCU_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, REF)
sys.modules.setdefault("h5py", types.ModuleType("h5py"))

import data_ref as R  # noqa: E402
import surface_ref as SR  # noqa: E402
from fn import datacore as fn_data  # noqa: E402
from make_data_fixtures import icosphere, indices_of, rotation_of, save_reproducibly, tie_free  # noqa: E402

F32 = np.float32
N, PATCHES, K = 512, 64, 12


def torus(nu=50, nv=50, spread=1e6):
    """A torus whose grid lines are spaced geometrically in both directions — face areas over eleven orders of magnitude, so that
    the f64 running sum of the f32 probabilities rounds (it needs more than 53 bits) — with its faces in a shuffled order."""
    def angles(count):
        w = np.exp(np.linspace(0.0, np.log(spread), count))
        return 2 * np.pi * np.concatenate([[0.0], np.cumsum(w)[:-1]]) / w.sum()
    a, b = angles(nu), angles(nv)
    v = np.array([[(0.6 + 0.25 * np.cos(q)) * np.cos(p), (0.6 + 0.25 * np.cos(q)) * np.sin(p), 0.25 * np.sin(q)] for p in a for q in b])
    f = []
    for i in range(nu):
        for j in range(nv):
            p00, p01 = i * nv + j, i * nv + (j + 1) % nv
            p10, p11 = ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv
            f += [[p00, p10, p11], [p00, p11, p01]]
    return v, [f[i] for i in np.random.default_rng(7).permutation(len(f))]


def degenerate():
    """An 80-face icosphere with a face of zero area (a repeated corner) put first, in the middle and last."""
    v, f = icosphere(1)
    f = [[0, 0, 1]] + f[:40] + [[5, 7, 5]] + f[40:] + [[3, 3, 3]]
    return v * 1.3 + np.array([0.2, 0.1, -0.4]), f


def polygons():
    """A box with an extra vertex on one top edge: three sides as quads, the fourth as a pentagon, the bottom as two triangles, the
    top as a quad and a triangle, and a two-corner "face" that the loader drops."""
    v = np.array([(x, y, z) for x in (0, 1.0) for y in (0, 0.6) for z in (0, 0.4)] + [(0.5, 0, 0.4)], float)
    f = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 8, 1], [2, 3, 7, 6], [0, 2, 6], [0, 6, 4], [1, 8], [8, 5, 7, 3], [1, 8, 3]]
    return v, f


def write_off(path, v, f):
    with open(path, "w") as fh:
        fh.write("OFF\n%d %d 0\n" % (len(v), len(f)))
        for p in v:
            fh.write("%.9g %.9g %.9g\n" % tuple(p))
        for face in f:
            fh.write("%d %s\n" % (len(face), " ".join(str(i) for i in face)))


def replay_sampler_draws(seed):
    np.random.seed(seed)                                          # the same calls in the same order as _sample_points_from_mesh
    u = np.random.random_sample(N)                                # RandomState.choice(p=...): uniform_samples = random_sample(size)
    r1 = np.random.random(N).astype(F32)
    r2 = np.random.random(N).astype(F32)
    return u, r1, r2


def check_sampling(name, vertices, faces, u, r1, r2, points, normals):
    """surface_ref on the recorded draws must give the reference's arrays; -> the selected faces."""
    tab = SR.tables(vertices, faces)
    assert tab["area_sum"] == SR.face_tables(vertices, faces)[1].sum(), (name, "area sum")
    p, nr, face = SR.sample(vertices, faces, tab, u, r1, r2)
    for got, want, what in ((p, points, "points"), (nr, normals, "normals")):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (name, what)
    assert (tab["areas"][face] > 0).all(), (name, "a zero-area face was selected")
    return face, tab


def sampler_case(out, ds, name, path, seed):
    vertices, faces = ds._load_off(path)
    np.random.seed(seed)
    points, normals = ds._sample_points_from_mesh(vertices, faces, N)
    u, r1, r2 = replay_sampler_draws(seed)
    face, tab = check_sampling(name, vertices, faces, u, r1, r2, points, normals)
    rec = {"vertices": vertices, "faces": faces, "u": u, "r1": r1, "r2": r2, "face": face, "points": points, "normals": normals,
           "seed": np.int64(seed)}
    for k, v in rec.items():
        out["%s/%s" % (name, k)] = v
    print("%-12s %5d faces, area sum %.6g, prob sum %.17g, %d distinct faces drawn" % (name, len(faces), tab["area_sum"], tab["prob_sum"],
                                                                                      len(set(face.tolist()))))
    return vertices, faces, tab


def item_case(out, name, folder, split, index, seed):
    ds = fn_data.PU1KMeshDataset(folder, split=split, num_points=N, num_patches=PATCHES, k_neighbors=K)
    vertices, faces = ds._load_off(ds.mesh_files[index])
    while True:
        np.random.seed(seed)
        item = {k: v.numpy() for k, v in ds[index].items()}
        u, r1, r2 = replay_sampler_draws(seed)                    # (re-seeds) ... and the rest of __getitem__'s calls, in order
        rec = {"u": u, "r1": r1, "r2": r2}
        tab = SR.tables(vertices, faces)
        points, normals, face = SR.sample(vertices, faces, tab, u, r1, r2)
        aug_cloud, aug_normals = points, normals
        if split == "train":
            theta = np.random.uniform(0, 2 * np.pi)
            scale = np.random.uniform(0.8, 1.2)
            jitter = np.random.normal(0, 0.002, points.shape).astype(F32)
            rot = rotation_of(theta)
            aug_cloud, aug_normals = points @ rot.T, normals @ rot.T          # the reference's own statements
            rec.update(rot_cloud=aug_cloud.copy())
            aug_cloud *= scale
            aug_cloud += jitter
            rec.update(theta=np.float64(theta), scale=np.float64(scale), jitter=jitter, rot=rot, aug_cloud=aug_cloud, aug_normals=aug_normals)
        centres = np.random.choice(N, PATCHES, replace=False)
        if tie_free(item["cloud"], centres, K):
            break
        seed += 1000
    rec.update(mesh=np.array(os.path.basename(ds.mesh_files[index])[2:-4]), face=face, points=points, normals=normals, cloud=item["cloud"],
               all_normals=item["all_normals"], normal=item["normal"], centres=centres.astype(np.int32),
               idx=indices_of(item["cloud"], centres, item["input"], K), seed=np.int64(seed))
    assert np.array_equal(item["all_normals"][centres], item["normal"]), "the replayed centres are not the reference's"
    want = R.sample(aug_cloud, K, normals=aug_normals, centres=centres)
    for key, ref in (("cloud", "cloud"), ("all_normals", "normals"), ("normal", "patch_normals"), ("idx", "idx")):
        assert rec[key].dtype == want[ref].dtype and np.array_equal(rec[key], want[ref]), (name, key)
    if split != "train":                                          # no BLAS product in between: the whole chain from the draws
        assert np.array_equal(aug_cloud, points) and np.array_equal(aug_normals, normals)
    for k, v in rec.items():
        out["%s/%s" % (name, k)] = v
    print("%-12s seed %-5d mesh %s" % (name, seed, rec["mesh"]))


def torus_shows_the_orders(vertices, faces, tab):
    areas = tab["areas"]
    p = (areas / F32(tab["area_sum"] + F32(1e-8))).astype(F32).astype(np.float64)
    seq = np.add.accumulate(p, dtype=np.float64)
    assert (SR.two_block_scan(p, len(p) // 2) != seq).any(), "a two-block scan equals the sequential cdf on the torus: change the mesh"
    assert np.add.accumulate(areas, dtype=F32)[-1] != tab["area_sum"], "a sequential f32 sum equals numpy's on the torus: change the mesh"
    assert areas.max() / areas[areas > 0].min() > 1e4


def main():
    out = {}
    with tempfile.TemporaryDirectory() as folder:
        meshes = (("icosphere", icosphere(2)), ("torus", torus()), ("degenerate", degenerate()), ("polygons", polygons()))
        paths = {}
        for i, (name, (v, f)) in enumerate(meshes):               # sorted: three train meshes, one val mesh (the polygons)
            paths[name] = os.path.join(folder, "%s_%s.off" % ("abcd"[i], name))
            write_off(paths[name], v, f)
        with open(paths["polygons"], "rb") as fh:
            out["polygons/off_text"] = np.frombuffer(fh.read(), dtype=np.uint8)
        ds = fn_data.PU1KMeshDataset(folder, split="all", num_points=N, num_patches=PATCHES, k_neighbors=K)
        for i, (name, _) in enumerate(meshes):
            got = sampler_case(out, ds, name, paths[name], 31 + i)
            if name == "torus":
                torus_shows_the_orders(*got)
        assert len(out["icosphere/faces"]) == 320 and len(out["torus/faces"]) == 5000
        zero = np.flatnonzero(SR.face_tables(out["degenerate/vertices"], out["degenerate/faces"])[1] == 0)
        assert zero.tolist() == [0, 41, len(out["degenerate/faces"]) - 1], zero
        item_case(out, "item_train", folder, "train", 1, 41)      # the torus
        item_case(out, "item_val", folder, "val", 0, 42)          # the polygons
        assert str(out["item_train/mesh"]) == "torus" and str(out["item_val/mesh"]) == "polygons"
    out["cases"] = np.array(sorted({k.split("/")[0] for k in out}))
    path = os.path.join(HERE, "surface_sample.npz")
    save_reproducibly(path, out)
    print("wrote %s %.1f KiB" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
