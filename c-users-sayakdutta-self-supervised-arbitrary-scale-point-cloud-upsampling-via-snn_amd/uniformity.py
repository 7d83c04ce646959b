"""Uniformity: how evenly a predicted cloud covers the ground-truth surface — the NUC figures, on the device.

The fourth figure an upsampler is judged on in the PU-GAN / Meta-PU protocol, beside Chamfer and Hausdorff distance (``metrics``) and
P2F (``mesh``).  The reference computes it in the second half of ``external/Meta-PU_evaluation/evaluation_code/evaluation.cpp``: every
predicted point is mapped to its closest surface point; for every seed on the mesh and each of seven disk areas (0.2 % .. 1.5 % of
the surface) it counts the mapped points within the disk's GEODESIC radius, CGAL's exact ``Surface_mesh_shortest_path`` once per
seed; density = count / (n * fraction); ``external/3D_Processing/calc_NUC.py`` pools the disks of all clouds and takes the
population standard deviation per disk size.  Here the mapping is ``mesh.point_to_mesh`` and the counts are one call of
``sapcu_geodesic_disks_f64`` (csrc/geodesic.hip; include/sapcu_mesh.h has the definition, tests/geodesic_ref.py states it in Python):
the tool's integer counts are reproduced exactly (tests/golden/uniformity.npz).

Radii carry the tool's two float32 roundings (``disk_radii``).  Densities stay f64: the tool stores them as ``float`` and prints six
digits; that rounding is NOT reproduced (5e-8 relative).  The tool's random seeds come from ``CGAL::Random``: its distribution is
rebuilt (``uniformity_seeds``), its stream is not; ``read_seeds`` takes the tool's own seed files.

No CPU path: the HIP library and a device are required (``disk_radii``, the seed functions and the file readers run on the host).
"""
import ctypes
import math

import numpy as np
import torch

from . import _inputs, _lib
from . import mesh as _mesh

TOOL_FRACTIONS = np.array([0.002, 0.004, 0.006, 0.008, 0.010, 0.012, 0.015], dtype=np.float32)   # evaluation.cpp's `precentage`
MAX_RADII = 16                                                                                     # SAPCU_GEODESIC_MAX_RADII
ERR_MESH = -5                                                                                      # SAPCU_ERR_MESH


def _host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _face_areas(vertices, faces):
    v, f = _host(vertices).astype(np.float64), _host(faces).astype(np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return 0.5 * np.sqrt(np.sum(n * n, -1))


def _fractions(fractions):
    fr = np.asarray(fractions, dtype=np.float32).reshape(-1)
    if not 1 <= fr.size <= MAX_RADII:
        raise ValueError("fractions: between 1 and %d disk sizes, got %d" % (MAX_RADII, fr.size))
    if not (np.isfinite(fr).all() and (fr > 0).all() and (np.diff(fr) >= 0).all()):
        raise ValueError("fractions: expected finite, positive, ascending shares of the surface area")
    return fr.astype(np.float64)


def disk_radii(vertices, faces, fractions=TOOL_FRACTIONS):
    """The geodesic radius of a disk covering each share ``fractions`` of the mesh's area, f64 [nr], with the tool's two float32
    roundings: ``float32(sqrt(A * float32(fraction) / pi))``, A the total area in f64 (on the host)."""
    area = float(np.sum(_face_areas(vertices, faces)))
    return np.sqrt(area * _fractions(fractions) / math.pi).astype(np.float32).astype(np.float64)


def _seeds_on(dev, seed_faces, seed_bary):
    sf, sb = _host(seed_faces), _host(seed_bary)
    if sf.ndim != 1 or sf.dtype.kind not in "iu":
        raise ValueError("seed_faces: expected integers [ns], got shape %s, dtype %s" % (sf.shape, sf.dtype))
    if sb.shape != (sf.shape[0], 3) or sb.dtype.kind != "f":
        raise ValueError("seed_bary: expected floating weights [%d, 3], got shape %s, dtype %s" % (sf.shape[0], sb.shape, sb.dtype))
    return (torch.from_numpy(np.ascontiguousarray(sf, dtype=np.int64)).to(dev),
            torch.from_numpy(np.ascontiguousarray(sb, dtype=np.float64)).to(dev))


def geodesic_disks(points, vertices, faces, seed_faces, seed_bary, fractions=TOOL_FRACTIONS, return_dist=False, radii=None,
                   queue_slots=0, info=None):
    """counts int64 [ns, nr] on the device: for every seed (face ``seed_faces[s]``, weights ``seed_bary[s]`` in the face's own vertex
    order, strictly inside the face) the number of ``points`` f64 [n,3], each mapped to its closest point of the mesh
    (``point_to_mesh``), within the geodesic radius of each disk size.  ``radii`` f64 [nr], ascending, replaces
    ``disk_radii(vertices, faces, fractions)``.  With ``return_dist`` also dist f64 [ns, n]: the geodesic distance from the seed to
    the mapped point, +inf beyond the largest radius.  A mesh that is no oriented 2-manifold (an edge with more than two faces, two
    faces crossing an edge in the same direction, a zero-area face) and a seed on an edge or a vertex raise ``ValueError``.
    ``queue_slots`` caps the LDS capacities of the kernel (0 = automatic; any value gives the same counts); ``info``, a list,
    receives [windows processed, largest queue, seeds that left LDS, boundary edges, pseudo-source vertices, seeds at the window
    cap, seeds past the workspace queue, work groups].  Synchronises the current stream."""
    points, vertices, faces = _mesh.on_device(points, vertices, faces, finite=True)
    dev = vertices.device
    radii = disk_radii(vertices, faces, fractions) if radii is None else np.ascontiguousarray(_host(radii), dtype=np.float64).reshape(-1)
    if not 1 <= radii.size <= MAX_RADII or not (np.isfinite(radii).all() and (radii > 0).all() and (np.diff(radii) >= 0).all()):
        raise ValueError("radii: expected 1 to %d finite, positive, ascending radii" % MAX_RADII)
    seed_faces, seed_bary = _seeds_on(dev, seed_faces, seed_bary)
    nq, nv, nf, ns, nr = points.shape[0], vertices.shape[0], faces.shape[0], seed_faces.shape[0], int(radii.size)
    counts = torch.zeros((ns, nr), dtype=torch.int64, device=dev)
    dist = torch.full((ns, nq), float("inf"), dtype=torch.float64, device=dev) if return_dist else None
    out = (ctypes.c_int64 * 8)()
    if ns:
        tpoint, tface = None, None
        if nq:
            _, tface, tpoint = _mesh.point_to_mesh(points, vertices, faces)
        ws, nbytes = _lib.workspace("sapcu_geodesic_disks_workspace_bytes", (nv, nf, nq, ns, nr), dev,
                                    "geodesic_disks: %d vertices, %d faces, %d points, %d seeds and %d radii are outside the call's range"
                                    % (nv, nf, nq, ns, nr))
        try:
            _lib.call("sapcu_geodesic_disks_f64", dev, vertices, nv, faces, nf, tpoint, tface, nq, seed_faces, seed_bary, ns,
                      radii.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nr, counts, dist, int(queue_slots), ws, nbytes, out)
        except _lib.SapcuError as e:
            if e.args[0] in (ERR_MESH, -1):
                raise ValueError(e.args[1]) from None
            raise
    if info is not None:
        info[:] = list(out)
    return (counts, dist) if return_dist else counts


def uniformity_seeds(vertices, faces, n, generator=None):
    """``n`` seeds of the tool's random mode, (faces int64 [n], bary f64 [n,3]) as numpy arrays: a face drawn with probability
    proportional to its area, three weights U(0.01, 1) normalised to sum 1.  ``generator``: a ``numpy.random.Generator``, a seed
    for one, or None.  The distribution is the tool's, the stream is not (``CGAL::Random``)."""
    rng = generator if isinstance(generator, np.random.Generator) else np.random.default_rng(generator)
    cdf = np.cumsum(_face_areas(vertices, faces))
    if not cdf.size or not cdf[-1] > 0:
        raise ValueError("uniformity_seeds: a mesh without area")
    face = np.minimum(np.searchsorted(cdf / cdf[-1], rng.uniform(0.0, 1.0, int(n)), side="right"), cdf.size - 1).astype(np.int64)
    w = rng.uniform(0.01, 1.0, (int(n), 3))
    return face, w / w.sum(-1, keepdims=True)


def read_seeds(path):
    """(faces int64 [n], bary f64 [n,3]) from a seed file of the tool, rows ``id x1 x2 x3``.  The tool's x1 is the weight of the
    face's THIRD vertex as the .off lists it, x2 of the first, x3 of the second (CGAL's ``halfedge(f)`` order); the weights returned
    are in the face's own vertex order."""
    rows = np.loadtxt(path, ndmin=2, dtype=np.float64)
    if rows.shape[1] != 4:
        raise ValueError("%s: expected rows `id x1 x2 x3`, got %d columns" % (path, rows.shape[1]))
    return rows[:, 0].astype(np.int64), np.ascontiguousarray(rows[:, [2, 3, 1]])


def write_seeds(path, faces, bary):
    """The inverse of ``read_seeds``: every weight with 17 significant digits."""
    faces, bary = _host(faces), _host(bary)
    with open(path, "w") as f:
        for i, w in zip(faces, bary):
            f.write("%d %.17g %.17g %.17g\n" % (int(i), w[2], w[0], w[1]))


def _figures(counts, n_pre, fractions, radii):
    counts = np.asarray(counts, dtype=np.int64)
    density = counts / (np.float64(n_pre) * fractions)[None, :]
    mean = density.mean(0)
    nuc = np.sqrt(np.mean((density - mean) ** 2, 0))
    return {"density": density, "counts": counts, "radii": radii, "nuc": nuc, "mean_density": mean, "n_pre": int(n_pre),
            "n_seeds": int(counts.shape[0])}


def uniformity_metrics(pred, vertices, faces, seeds=None, n_seeds=1000, generator=None, fractions=TOOL_FRACTIONS):
    """The uniformity figures of one predicted cloud on its mesh, a dict: ``density`` f64 [ns, nr] = counts / (n_pre * fraction),
    ``counts`` int64 [ns, nr], ``radii`` [nr], ``nuc`` [nr] (the population standard deviation of a column of ``density``, as
    calc_NUC.py pools it), ``mean_density`` [nr], ``n_pre``, ``n_seeds``; numpy arrays, every float numpy's own on the same counts.
    ``seeds`` = (faces, bary), e.g. ``read_seeds``'s; else ``n_seeds`` are drawn with ``uniformity_seeds``."""
    fr = _fractions(fractions)
    radii = disk_radii(vertices, faces, fr)
    if seeds is None:
        seeds = uniformity_seeds(vertices, faces, n_seeds, generator)
    n_pre = int(pred.shape[0])
    if n_pre < 1:
        raise ValueError("pred: an empty cloud")
    counts = geodesic_disks(pred, vertices, faces, seeds[0], seeds[1], radii=radii)
    if counts.shape[0] < 1:
        raise ValueError("uniformity_metrics: no seed")
    return _figures(counts.cpu().numpy(), n_pre, fr, radii)


def dataset_uniformity(items):
    """The pooled figures over ``items``, an iterable of dicts as ``uniformity_metrics`` returns them: the density rows of all clouds
    concatenated in the order given, then ``nuc`` and ``mean_density`` over all disks, as calc_NUC.py does; ``n_seeds`` and
    ``n_pre`` are the pooled counts.  Every item has to have the same number of disk sizes."""
    items = list(items)
    if not items:
        raise ValueError("dataset_uniformity: no item")
    density = np.concatenate([it["density"] for it in items], 0)
    mean = density.mean(0)
    return {"density": density, "nuc": np.sqrt(np.mean((density - mean) ** 2, 0)), "mean_density": mean,
            "n_pre": int(sum(it["n_pre"] for it in items)), "n_seeds": int(density.shape[0])}


def evaluate_uniformity_file(pred_path, mesh_path, seeds_path, device="cuda"):
    """``uniformity_metrics`` from the tool's own files: what ``evaluation mesh.off pred.xyz F seeds.txt`` writes to
    ``pred_density.xyz`` is ``density`` (in f64, see the module docstring)."""
    pred = np.loadtxt(pred_path, ndmin=2)[:, :3]
    vertices, faces = _mesh.read_off(mesh_path)
    dev = torch.device(device)
    return uniformity_metrics(torch.from_numpy(np.ascontiguousarray(pred)).to(dev), torch.from_numpy(vertices).to(dev),
                              torch.from_numpy(faces).to(dev), seeds=read_seeds(seeds_path))
