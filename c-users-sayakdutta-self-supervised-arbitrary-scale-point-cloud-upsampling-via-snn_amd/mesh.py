"""P2F, the point-to-surface distance of a predicted cloud to the ground-truth triangle mesh, on the device.

The third figure an upsampler is judged on, beside Chamfer and Hausdorff distance (``metrics``).  The reference computes it on the
host with a CGAL program, ``external/Meta-PU_evaluation/evaluation_code/evaluation.cpp`` (``evaluation mesh.off pred.xyz``), which
writes one distance per point and prints their mean, sample standard deviation, minimum and maximum.  Here the distances are one
call of ``sapcu_point_mesh_f64`` (csrc/mesh_dist.hip, include/sapcu_mesh.h: the definition, the skipped faces, the caveat about
slivers), and every float equals numpy's (``==``) on the same distance vector, through the fixed summation order of ``metrics``.

Distances stay f64.  The tool stores each distance as ``float`` and prints six digits; that rounding is NOT reproduced, so a value
agrees with the tool's to about 5e-6 relative, not bit for bit.  The tool's uniformity figures (geodesic disks on the mesh) are
``uniformity``'s, which maps the points with ``point_to_mesh``.

No CPU path: the HIP library and a device are required (``read_off`` alone runs on the host).
"""
import ctypes

import numpy as np
import torch

from . import _inputs, _lib
from . import metrics


def point_to_mesh(points, vertices, faces, cell_size=0.0, info=None):
    """Distance from every point f64 [nq,3] to the mesh (``vertices`` f64 [nv,3], ``faces`` integer [nf,3]):
    (dist f64 [nq], face int64 [nq], closest f64 [nq,3]) on the device — the distance, the nearest face (the lowest index among faces
    at a bit-equal distance) and the closest point on it.  Inputs are numpy arrays or device tensors.  A face index outside [0, nv)
    raises ``ValueError`` here (the C entry point would skip that face); zero-area faces are skipped by the kernel and counted.
    A point that no face gives a distance for (a NaN point, every face skipped) gets NaN, -1, NaN.  ``cell_size`` 0 = automatic
    (any value gives the same result, bit for bit).  ``info``, a list, receives [route (0 brute force, 1 grid), gx, gy, gz, faces
    on the oversize list, faces skipped].  Synchronises the current stream once."""
    points, vertices, faces = on_device(points, vertices, faces)
    nq, nv, nf = points.shape[0], vertices.shape[0], faces.shape[0]
    dev = vertices.device
    dist = torch.full((nq,), float("nan"), dtype=torch.float64, device=dev)
    face = torch.full((nq,), -1, dtype=torch.int64, device=dev)
    closest = torch.full((nq, 3), float("nan"), dtype=torch.float64, device=dev)
    out = (ctypes.c_int64 * 6)()
    if nq:
        ws, nbytes = _lib.workspace("sapcu_point_mesh_workspace_bytes", (nv, nf, nq), dev,
                                    "point_to_mesh: %d vertices, %d faces and %d points are outside the search's range" % (nv, nf, nq))
        _lib.call("sapcu_point_mesh_f64", dev, vertices, nv, faces, nf, points, nq, float(cell_size), dist, face, closest, ws, nbytes, out)
    if info is not None:
        info[:] = list(out)
    return dist, face, closest


def mesh_metrics(pred, vertices, faces):
    """The P2F figures of one predicted cloud against its mesh, a dict: ``p2f_mean``, ``p2f_std`` (the SAMPLE standard deviation,
    n - 1, as the reference's tool prints; NaN for a single point), ``p2f_min``, ``p2f_max``, ``n_pre``, ``n_faces``, ``n_skipped``
    (zero-area faces, which take no part).  Floats are ``np.float64`` and equal numpy's on the same distance vector d:
    ``np.mean(d)``, ``np.sqrt(np.sum((d - mean) ** 2) / (n - 1))``, ``d.min()``, ``d.max()``.  Distances stay f64: the tool's
    rounding of each distance to ``float`` is not reproduced.  Non-finite input and a mesh whose every face is skipped raise
    ``ValueError``."""
    d, nf, ns = _distances(pred, vertices, faces)
    return _figures(d, nf, ns)


def mesh_dataset_metrics(triples):
    """The pooled figures over ``triples``, an iterable of (pred, vertices, faces): the distance vectors of all clouds concatenated
    in the order given, then the statistics of ``mesh_metrics`` (``n_pre`` / ``n_faces`` / ``n_skipped``: the pooled counts)."""
    parts = [_distances(pred, vertices, faces) for pred, vertices, faces in triples]
    if not parts:
        raise ValueError("mesh_dataset_metrics: no (pred, vertices, faces) triple")
    return _figures(torch.cat([d for d, _, _ in parts]), sum(nf for _, nf, _ in parts), sum(ns for _, _, ns in parts))


def read_off(path, triangulate=False):
    """A triangle mesh from an ``.off`` text file, on the host: (vertices f64 [nv,3], faces int64 [nf,3]).  Accepted: ``OFF`` with
    the counts on the same or on the next line, ``#`` comments, blank lines, trailing per-face colour fields.  ``ValueError`` on a
    face that is not a triangle, on a truncated file and on counts that do not match the file's content.  With ``triangulate`` a
    polygon of m vertices becomes the fan (0, j, j+1), j = 1..m-2, and a face of fewer than three vertices is dropped, as the
    reference's training loader does (fn/datacore.py:111-117); nf is then the number of triangles, not the file's face count."""
    with open(path) as f:
        lines = [ln.split("#", 1)[0].split() for ln in f]
    lines = [t for t in lines if t]
    if not lines or not lines[0][0].startswith("OFF"):
        raise ValueError("%s: not an OFF file" % path)
    head = lines[0][1:] if lines[0][0] == "OFF" else [lines[0][0][3:]] + lines[0][1:]
    pos = 1
    if not head:
        if len(lines) < 2:
            raise ValueError("%s: truncated before the counts" % path)
        head, pos = lines[1], 2
    try:
        nv, nf = int(head[0]), int(head[1])
    except (ValueError, IndexError):
        raise ValueError("%s: bad counts line %r" % (path, " ".join(head))) from None
    if nv < 0 or nf < 0:
        raise ValueError("%s: negative counts" % path)
    if len(lines) < pos + nv + nf:
        raise ValueError("%s: truncated: %d vertices and %d faces announced, %d lines follow" % (path, nv, nf, len(lines) - pos))
    if len(lines) > pos + nv + nf:
        raise ValueError("%s: %d lines beyond the %d vertices and %d faces announced" % (path, len(lines) - pos - nv - nf, nv, nf))
    vertices = np.zeros((nv, 3), dtype=np.float64)
    faces = np.zeros((nf, 3), dtype=np.int64)
    try:
        for i in range(nv):
            t = lines[pos + i]
            if len(t) < 3:
                raise ValueError("vertex %d has %d coordinates" % (i, len(t)))
            vertices[i] = [float(t[0]), float(t[1]), float(t[2])]
        fans = []
        for i in range(nf):
            t = lines[pos + nv + i]
            if triangulate:
                m = int(t[0])
                if m < 0 or len(t) < 1 + m:
                    raise ValueError("face %d is truncated" % i)
                corners = [int(c) for c in t[1:1 + m]]
                fans += [[corners[0], corners[j], corners[j + 1]] for j in range(1, m - 1)]
                continue
            if int(t[0]) != 3:
                raise ValueError("face %d has %s vertices, not 3" % (i, t[0]))
            if len(t) < 4:
                raise ValueError("face %d is truncated" % i)
            faces[i] = [int(t[1]), int(t[2]), int(t[3])]
        if triangulate:
            faces = np.array(fans, dtype=np.int64).reshape(-1, 3)
    except ValueError as e:
        raise ValueError("%s: %s" % (path, e)) from None
    return vertices, faces


def evaluate_mesh_file(pred_path, mesh_path, device="cuda"):
    """``mesh_metrics`` of a text cloud, loaded the way ``pipeline.evaluate_file`` loads its clouds, against an ``.off`` mesh: what
    the reference's ``evaluation mesh.off pred.xyz`` prints as Mean / std / min / max (in f64, see the module docstring)."""
    pred = np.loadtxt(pred_path, ndmin=2)[:, :3]
    vertices, faces = read_off(mesh_path)
    dev = torch.device(device)
    return mesh_metrics(torch.from_numpy(np.ascontiguousarray(pred)).to(dev), torch.from_numpy(vertices).to(dev),
                        torch.from_numpy(faces).to(dev))


def checked_faces(faces):
    """The faces of a mesh after their host checks: shape, integer dtype, placement, at least one face."""
    if torch.is_tensor(faces):
        shape, on_host = tuple(faces.shape), not faces.is_cuda
        integer = not (faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == torch.bool)
    else:
        faces = np.asarray(faces)
        shape, on_host, integer = faces.shape, False, faces.dtype.kind in "iu"
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("faces: expected triangles [nf, 3], got shape %s" % (tuple(shape),))
    if not integer:
        raise ValueError("faces: expected an integer dtype")
    if on_host:
        raise RuntimeError("faces: a CPU tensor (there is no CPU path; pass a device tensor or a numpy array)")
    if shape[0] < 1:
        raise ValueError("faces: an empty mesh")
    return faces


def on_device(points, vertices, faces, name="points", min_rows=0, finite=False):
    """points (called ``name`` in messages) and vertices as contiguous f64 [n,3], faces as contiguous int32 [nf,3] with every index
    in [0, nv), on one device.  ``min_rows`` and ``finite`` are the points' and, ``finite``, the vertices' checks of
    ``_inputs.on_device``; the range check of the faces (one read-back) comes before the device tensors' values are tested."""
    _inputs.checked(points, name), _inputs.checked(vertices, "vertices")      # shape, dtype, placement of both before the rest
    xs = [_inputs.checked(points, name, min_rows, finite), _inputs.checked(vertices, "vertices", 0, finite)]
    faces = checked_faces(faces)
    nv = xs[1].shape[0]
    if nv < 1:
        raise ValueError("vertices: an empty mesh")
    out = _inputs.upload(xs, others=(faces,))
    if not torch.is_tensor(faces):
        if faces.dtype.kind == "u":
            if int(faces.max()) >= nv:
                raise ValueError("faces: an index outside [0, %d)" % nv)
        faces = torch.from_numpy(np.ascontiguousarray(faces).astype(np.int64))
    faces = faces.to(device=out[0].device)
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0 or hi >= nv:
        raise ValueError("faces: an index outside [0, %d) (smallest %d, largest %d)" % (nv, lo, hi))
    if finite:
        _inputs.finite_on_device(xs, out, (name, "vertices"))
    return out + [faces.to(torch.int32).contiguous()]


# ------------------------------------------------------------------------------------------------------------ internals
def _distances(pred, vertices, faces):
    """(dist f64 [n_pre] on the device, faces, skipped faces); the input checks of mesh_metrics."""
    pred, vertices, faces = on_device(pred, vertices, faces, "pred", min_rows=1, finite=True)
    info = []
    d = point_to_mesh(pred, vertices, faces, info=info)[0]
    nf = int(faces.shape[0])
    if info[5] >= nf:
        raise ValueError("mesh: every one of the %d faces has zero area" % nf)
    return d, nf, int(info[5])


def _figures(d, n_faces, n_skipped):
    mean, std, lo, hi = metrics.moments(d, 1)
    return {"p2f_mean": mean, "p2f_std": std, "p2f_min": lo, "p2f_max": hi,
            "n_pre": int(d.numel()), "n_faces": int(n_faces), "n_skipped": int(n_skipped)}
