"""Area-weighted sampling of triangle meshes on the device: fn's training clouds straight from the meshes.

The reference's ``PU1KMeshDataset.__getitem__`` (fn/datacore.py:186-199) draws a NEW sampling of its mesh on every call:
``_sample_points_from_mesh`` (:122-184, numpy) picks ``num_points`` faces with probability proportional to their area and a uniform
point on each, and returns the points with their face normals.  Here the part that depends on the mesh alone — face normals, face
areas, the cumulative distribution ``RandomState.choice`` searches — is computed once per data set by ``build_surface_tables``
(``sapcu_surface_tables_f32``), and a batch of samplings is one launch of ``sapcu_surface_sample_f32`` (csrc/surface_sample.hip,
include/sapcu_surface.h: the definition, operation by operation).  Given the same draws every output equals the reference's bit for
bit (tests/golden/surface_sample.npz).

No CPU path: the HIP library and a device are required.
"""
import functools

import numpy as np
import torch

from . import _inputs, _lib

MAX_N = 4096


class SurfaceTables(object):
    """The ragged device arrays of S meshes and their sampling tables (``build_surface_tables`` makes them): ``vertices`` f32
    [total_vertices,3], ``vert_off`` int64 [S+1], ``faces`` int32 [total_faces,3] (indices local to the mesh), ``face_off`` int64 [S+1],
    ``face_normals`` f32 [total_faces,3], ``cdf`` f64 [total_faces], ``area_sum`` f32 [S], ``prob_sum`` f64 [S]; ``face_counts`` and
    ``vertex_counts`` are host lists, ``names`` what the error messages call the meshes."""

    def __init__(self, vertices, vert_off, faces, face_off, face_normals, cdf, area_sum, prob_sum, vertex_counts, face_counts, names):
        self.vertices, self.vert_off, self.faces, self.face_off = vertices, vert_off, faces, face_off
        self.face_normals, self.cdf, self.area_sum, self.prob_sum = face_normals, cdf, area_sum, prob_sum
        self.vertex_counts, self.face_counts, self.names = list(vertex_counts), list(face_counts), list(names)

    def __len__(self):
        return len(self.face_counts)

    @property
    def device(self):
        return self.vertices.device

    def mesh(self, m):
        """(vertices, faces, face_normals, cdf) of mesh m: views of the ragged arrays."""
        v0, f0 = sum(self.vertex_counts[:m]), sum(self.face_counts[:m])
        v1, f1 = v0 + self.vertex_counts[m], f0 + self.face_counts[m]
        return self.vertices[v0:v1], self.faces[f0:f1], self.face_normals[f0:f1], self.cdf[f0:f1]


def _host(x, name, what):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError("%s: %s: expected [count, 3], got shape %s" % (name, what, tuple(x.shape)))
    return x


def build_surface_tables(meshes, device=None, names=None):
    """The sampling tables of ``meshes``, a list of (vertices [nv,3] floating, faces [nf,3] integer) as numpy arrays or tensors ->
    ``SurfaceTables`` on ``device`` (None = the current one).  Vertices are taken as f32 (the reference's loader stores them so).

    Validated here, on the host, with ``ValueError`` naming the mesh (``names``; default "mesh <i>"): an empty mesh (no vertex or no
    face), a face index outside the mesh's vertices, and a mesh whose probabilities do not sum to 1 — ``|prob_sum - 1| >
    sqrt(finfo(float32).eps)`` or a non-finite ``prob_sum`` — which is the reference's "probabilities do not sum to 1" and covers a
    mesh of zero total area and one so small that the ``+ 1e-8`` of its normalisation matters.  numpy tests this on a Kahan sum of
    the probabilities; ``prob_sum`` is their sequential f64 sum (the last cdf entry before the division), which differs from it
    only in rounding, some 1e-16 relative per face against a bound of 3.5e-4.  One synchronisation (the read-back of ``prob_sum``)."""
    meshes = list(meshes)
    if not meshes:
        raise ValueError("build_surface_tables: no mesh")
    names = ["mesh %d" % i for i in range(len(meshes))] if names is None else [str(s) for s in names]
    if len(names) != len(meshes):
        raise ValueError("build_surface_tables: %d names for %d meshes" % (len(names), len(meshes)))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("device %s: there is no CPU path" % dev)
    verts, faces = [], []
    for name, pair in zip(names, meshes):
        v, f = _host(pair[0], name, "vertices"), _host(pair[1], name, "faces")
        if v.dtype.kind != "f":
            raise ValueError("%s: vertices: expected a floating dtype" % name)
        if f.dtype.kind not in "iu":
            raise ValueError("%s: faces: expected an integer dtype" % name)
        if v.shape[0] < 1 or f.shape[0] < 1:
            raise ValueError("%s: an empty mesh (%d vertices, %d faces)" % (name, v.shape[0], f.shape[0]))
        lo, hi = int(f.min()), int(f.max())
        if lo < 0 or hi >= v.shape[0]:
            raise ValueError("%s: a face index outside [0, %d) (smallest %d, largest %d)" % (name, v.shape[0], lo, hi))
        verts.append(np.ascontiguousarray(v, dtype=np.float32))
        faces.append(np.ascontiguousarray(f).astype(np.int32))
    vcount, fcount = [len(v) for v in verts], [len(f) for f in faces]
    S, tv, tf = len(meshes), sum(vcount), sum(fcount)
    refusal = "build_surface_tables: %d meshes with %d vertices and %d faces are outside the range of the call" % (S, tv, tf)
    if tv >= 2 ** 31:
        raise ValueError(refusal)
    ws, nbytes = _lib.workspace("sapcu_surface_tables_workspace_bytes", (S, tf), dev, refusal)
    up = lambda a: torch.from_numpy(a).to(dev)
    vertices, tri = up(np.concatenate(verts)), up(np.concatenate(faces))
    vert_off = up(np.concatenate([[0], np.cumsum(vcount)]).astype(np.int64))
    face_off = up(np.concatenate([[0], np.cumsum(fcount)]).astype(np.int64))
    face_normals = torch.zeros((tf, 3), dtype=torch.float32, device=dev)
    cdf = torch.zeros((tf,), dtype=torch.float64, device=dev)
    area_sum = torch.zeros((S,), dtype=torch.float32, device=dev)
    prob_sum = torch.zeros((S,), dtype=torch.float64, device=dev)
    _lib.call("sapcu_surface_tables_f32", dev, vertices, vert_off, tv, tri, face_off, tf, S, face_normals, cdf, area_sum, prob_sum, ws,
              nbytes)
    atol = float(np.sqrt(np.finfo(np.float32).eps))
    for name, ps, area in zip(names, prob_sum.tolist(), area_sum.tolist()):
        if not np.isfinite(ps) or abs(ps - 1.0) > atol:
            raise ValueError("%s: probabilities do not sum to 1 (the face areas sum to %g, the probabilities to %r): a mesh of zero or "
                             "vanishing area cannot be sampled" % (name, area, ps))
    return SurfaceTables(vertices, vert_off, tri, face_off, face_normals, cdf, area_sum, prob_sum, vcount, fcount, names)


def sample_surface(tables, mesh_idx, n, u, r1, r2, validate=True):
    """``n`` surface points of each of b batch entries: ``mesh_idx`` int64 [b] (the mesh of every entry, repeats allowed), the draws
    ``u`` f64 [b,n] in [0,1) (the face: the number of cdf entries <= u) and ``r1``, ``r2`` f32 [b,n] in [0,1] (the position inside
    it), device tensors -> (points f32 [b,n,3], normals f32 [b,n,3], faces int32 [b,n], local to the mesh).  One launch, no
    read-back.  The VALUES of ``mesh_idx`` are checked here (one synchronisation; ``validate=False`` skips it, for stream capture —
    the kernel then leaves the rows of a bad index unwritten, NaN / -1): ValueError.  CPU tensors: RuntimeError."""
    if not isinstance(tables, SurfaceTables):
        raise ValueError("tables: expected the result of build_surface_tables")
    n = int(n)
    if not 1 <= n <= MAX_N:
        raise ValueError("n: need 1 <= n <= %d points, got %d" % (MAX_N, n))
    dev = tables.device

    dev_tensor = functools.partial(_inputs.device_tensor, dev, "the tables")
    mesh_idx = dev_tensor(mesh_idx, "mesh_idx", torch.int64, (None,))
    b, S = mesh_idx.shape[0], len(tables)
    u = dev_tensor(u, "u", torch.float64, (b, n))
    r1 = dev_tensor(r1, "r1", torch.float32, (b, n))
    r2 = dev_tensor(r2, "r2", torch.float32, (b, n))
    if b > 2 ** 20:
        raise ValueError("mesh_idx: a batch of %d entries is outside the range of the call" % b)
    if validate and b:
        bad = int(((mesh_idx < 0) | (mesh_idx >= S)).sum())
        if bad:
            raise ValueError("mesh_idx: %d indices outside [0, %d)" % (bad, S))
    points = torch.full((b, n, 3), float("nan"), dtype=torch.float32, device=dev)
    normals = torch.full((b, n, 3), float("nan"), dtype=torch.float32, device=dev)
    faces = torch.full((b, n), -1, dtype=torch.int32, device=dev)
    if b == 0:
        return points, normals, faces
    t = tables
    _lib.call("sapcu_surface_sample_f32", dev, t.vertices, t.vert_off, t.vertices.shape[0], t.faces, t.face_off, t.faces.shape[0],
              t.face_normals, t.cdf, S, mesh_idx, b, n, u, r1, r2, points, normals, faces)
    return points, normals, faces
