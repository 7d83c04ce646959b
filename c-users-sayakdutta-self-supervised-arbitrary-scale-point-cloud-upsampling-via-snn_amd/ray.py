"""Ray casting against triangle meshes on the device, and fd's training samples from meshes.

fd predicts a distance ALONG a direction: ``Generator3D6`` moves a seed to ``p + n*d``.  The ground truth of that quantity against a
mesh is a ray-mesh intersection, and the reference makes fd's mesh training data that way: ``scripts/sample_mesh-rd.py`` samples
surface points, throws each one out along a random unit direction by a length in [0.003, 0.03), casts the ray back with trimesh's
embree intersector, keeps a sample when the first face hit is the sampled face and the ray meets it at less than 1 rad, and writes
``points / normals / lens`` — the ``fd.npz`` that ``fd/field.py:fdField`` reads.  Here a cast is one call of ``sapcu_ray_mesh_f64``
and the sampler's step one call of ``sapcu_ray_fd_samples_f64`` (csrc/ray_cast.hip, include/sapcu_ray.h: the definition, the skipped
faces, the caveat about rays through shared edges); tests/ray_ref.py states both in numpy, and the device equals it bit for bit.

P2F (``mesh``) measures the closest distance, a lower bound of the directed one that says nothing about the direction fn chose;
``signed_ray_distance`` / ``ray_metrics`` score fd's distances and a generator's displacement step along that direction.

No CPU path: the HIP library and a device are required (``is_watertight`` and ``as_fd_npz`` alone run on the host).
"""
import ctypes

import numpy as np
import torch

from . import _inputs, _lib
from . import mesh as mesh_mod
from . import metrics
from . import surface

COS_1RAD = 0.5403023058681398
LEN_MIN, LEN_SPAN = 0.003, 0.027


def _rays_on_device(origins, directions, vertices, faces, t_max):
    origins, vertices, faces = mesh_mod.on_device(origins, vertices, faces)
    directions = _inputs.checked(directions, "directions")
    if tuple(directions.shape) != tuple(origins.shape):
        raise ValueError("directions: shape %s, the origins have %s" % (tuple(directions.shape), tuple(origins.shape)))
    dev = vertices.device
    directions = _inputs.upload([directions], dev)[0]
    if t_max is not None:
        nq = origins.shape[0]
        if torch.is_tensor(t_max):
            if t_max.dim() and not t_max.is_cuda:
                raise RuntimeError("t_max: a CPU tensor (there is no CPU path; pass a device tensor, a numpy array or a number)")
            if not t_max.dtype.is_floating_point:
                raise ValueError("t_max: expected a floating dtype")
            t_max = t_max.to(device=dev, dtype=torch.float64)
        else:
            t_max = torch.from_numpy(np.asarray(t_max, dtype=np.float64)).to(dev)
        if t_max.dim() == 0:
            t_max = t_max.expand(nq)
        if tuple(t_max.shape) != (nq,):
            raise ValueError("t_max: expected a number or [%d], got shape %s" % (nq, tuple(t_max.shape)))
        t_max = t_max.contiguous()
    return origins, directions, vertices, faces, t_max


def ray_to_mesh(origins, directions, vertices, faces, t_max=None, cell_size=0.0, info=None):
    """Where every ray ``origins[i] + t * directions[i]`` (f64 [nq,3] each; a direction need not be unit, t is in units of its
    length) first meets the mesh (``vertices`` f64 [nv,3], ``faces`` integer [nf,3]) at 0 <= t <= ``t_max`` (None = no limit, a
    number, or f64 [nq]): (t f64 [nq], face int64 [nq], hit f64 [nq,3]) on the device — the smallest t, the face hit (the lowest
    index among faces at an equal t) and the point ``o + t*d``.  Two-sided.  A ray that hits nothing gets +inf, -1, NaN.  Inputs
    are numpy arrays or device tensors.  A face index outside [0, nv) raises ``ValueError`` here (the C entry point would skip that
    face); zero-area faces are skipped by the kernel and counted.  ``cell_size`` 0 = automatic (any value gives the same result,
    bit for bit).  ``info``, a list, receives [route (0 brute force, 1 grid), gx, gy, gz, faces on the oversize list, faces
    skipped].  Synchronises the current stream once."""
    origins, directions, vertices, faces, t_max = _rays_on_device(origins, directions, vertices, faces, t_max)
    nq, nv, nf = origins.shape[0], vertices.shape[0], faces.shape[0]
    dev = vertices.device
    t = torch.full((nq,), float("inf"), dtype=torch.float64, device=dev)
    face = torch.full((nq,), -1, dtype=torch.int64, device=dev)
    hit = torch.full((nq, 3), float("nan"), dtype=torch.float64, device=dev)
    out = (ctypes.c_int64 * 6)()
    if nq:
        ws, nbytes = _lib.workspace("sapcu_ray_mesh_workspace_bytes", (nv, nf, nq), dev,
                                    "ray_to_mesh: %d vertices, %d faces and %d rays are outside the cast's range" % (nv, nf, nq))
        _lib.call("sapcu_ray_mesh_f64", dev, vertices, nv, faces, nf, origins, directions, t_max, nq, float(cell_size), t, face, hit, ws,
                  nbytes, out)
    if info is not None:
        info[:] = list(out)
    return t, face, hit


def signed_ray_distance(points, normals, vertices, faces, t_max=None, info=None):
    """The distance from every point to the mesh ALONG its normal: the rays ``p + t*n`` and ``p - t*n`` are cast and the nearer hit
    is returned as a signed d (f64 [n]; +t of the first ray when it is nearer or as near, else -t of the second), so that
    ``p + n*d`` is the hit; the second value is the face (int64 [n]).  A point with no hit within ``t_max`` on either side gets NaN
    and -1.  d is in units of |n|: a distance for unit normals.  The ground truth of fd's output and of ``Generator3D6``'s
    displacement step.  ``info`` as in ``ray_to_mesh`` (of the cast along +n)."""
    points, normals, vertices, faces, t_max = _rays_on_device(points, normals, vertices, faces, t_max)
    tp, fp, _ = ray_to_mesh(points, normals, vertices, faces, t_max=t_max, info=info)
    tn, fn, _ = ray_to_mesh(points, -normals, vertices, faces, t_max=t_max)
    fwd = tp <= tn
    d = torch.where(fwd, tp, -tn)
    face = torch.where(fwd, fp, fn)
    return torch.where(face >= 0, d, torch.full_like(d, float("nan"))), face


def ray_metrics(points, normals, pred_d, vertices, faces, t_max=None, bufsize=None):
    """The error of predicted directed distances ``pred_d`` [n] against ``signed_ray_distance``, a dict: ``ray_mean``, ``ray_std``
    (the SAMPLE standard deviation, n - 1; NaN for a single point), ``ray_min``, ``ray_max`` of |pred_d - d| over the points with a
    hit, ``n`` (those points), ``n_missed``, ``n_faces``, ``n_skipped``.  Floats are ``np.float64`` and equal numpy's on the same
    vector e: ``np.mean(e)``, ``np.sqrt(np.sum((e - mean) ** 2) / (n - 1))``, ``e.min()``, ``e.max()`` (the fixed-order sums of
    ``metrics``, as ``mesh_metrics``).  No point with a hit: ``ValueError``."""
    info = []
    d, face = signed_ray_distance(points, normals, vertices, faces, t_max=t_max, info=info)
    n_all = d.shape[0]
    if torch.is_tensor(pred_d):
        if not pred_d.is_cuda:
            raise RuntimeError("pred_d: a CPU tensor (there is no CPU path; pass a device tensor or a numpy array)")
        pred = pred_d.to(device=d.device, dtype=torch.float64).reshape(-1)
    else:
        pred = torch.from_numpy(np.ascontiguousarray(np.asarray(pred_d, dtype=np.float64)).reshape(-1)).to(d.device)
    if pred.shape[0] != n_all:
        raise ValueError("pred_d: %d values for %d points" % (pred.shape[0], n_all))
    got = face >= 0
    e = (pred[got] - d[got]).abs().contiguous()
    n = int(e.numel())
    if n < 1:
        raise ValueError("ray_metrics: no point meets the mesh along its normal")
    mean, std, lo, hi = metrics.moments(e, 1, bufsize)
    return {"ray_mean": mean, "ray_std": std, "ray_min": lo, "ray_max": hi, "n": n,
            "n_missed": int(n_all - n), "n_faces": int(np.shape(faces)[0]), "n_skipped": int(info[5])}


def is_watertight(faces):
    """True when every undirected edge of ``faces`` (integer [nf,3], numpy or tensor) occurs in exactly two faces: the reference's
    ``mesh.is_watertight`` refusal.  On the host."""
    if torch.is_tensor(faces):
        faces = faces.detach().cpu().numpy()
    faces = np.asarray(faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in "iu":
        raise ValueError("faces: expected integer triangles [nf, 3]")
    if faces.shape[0] == 0:
        return False
    f = faces.astype(np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return bool((counts == 2).all())


def sample_fd_rays(tables, mesh_idx, u, r1, r2, g, w, allow_open=False, cell_size=0.0):
    """fd's ray samples of one mesh, the sampler of the reference's ``scripts/sample_mesh-rd.py`` with the draws as inputs (the
    reference's come from trimesh's and Python's generators and cannot be reproduced).  ``tables``: ``build_surface_tables``'
    result, ``mesh_idx`` the mesh in it; the draws are device tensors of n entries: ``u`` f64, ``r1``, ``r2`` f32 (the surface
    point: ``sample_surface``), ``g`` f64 [n,3] Gaussian (the direction) and ``w`` f64 [n] uniform in [0,1) (the length).  In f64:
    the surface point ``out`` and its face come from ``sample_surface`` (f32, widened); ``dir = g * (1/sqrt(dot(g,g)))``;
    ``len = w*0.027 + 0.003``; ``p = out + len*dir``; the ray from p along -dir with ``t_max = len*(1 + 2^-20)`` is cast against the
    mesh (its f32 vertices widened).  A sample is KEPT iff the first face hit is the sampled face and ``dot(n_face, dir) >
    cos(1.0)`` (0.5403023058681398), n_face = cross(e1, e2) normalised in f64.  The reference tests ``arccos(dot) < 1``; the cosine
    is compared instead because no device acos would reproduce numpy's bit for bit, so a sample whose angle is within an ulp of 1 rad
    may be decided differently.
    -> (keep bool [n], points f32 [K,3], normals f32 [K,3] = -dir, lens f32 [K]) with K kept samples, on the device.  A mesh that is
    not watertight raises ``ValueError`` unless ``allow_open`` (the reference refuses such meshes)."""
    if not isinstance(tables, surface.SurfaceTables):
        raise ValueError("tables: expected the result of build_surface_tables")
    m = int(mesh_idx)
    if not 0 <= m < len(tables):
        raise ValueError("mesh_idx: %d outside [0, %d)" % (m, len(tables)))
    v32, faces, _, _ = tables.mesh(m)
    if not allow_open and not _watertight_cached(tables, m, faces):
        raise ValueError("%s: not watertight (an edge that does not belong to exactly two faces); pass allow_open=True to sample it "
                         "anyway" % tables.names[m])
    dev = tables.device
    for t, name in ((u, "u"), (r1, "r1"), (r2, "r2"), (g, "g"), (w, "w")):
        if not torch.is_tensor(t):
            raise ValueError("%s: expected a device tensor" % name)
        if not t.is_cuda:
            raise RuntimeError("%s: a CPU tensor (there is no CPU path)" % name)
        if not t.dtype.is_floating_point:
            raise ValueError("%s: expected a floating dtype" % name)
    n = int(u.numel())
    if tuple(g.shape) != (n, 3) or any(int(t.numel()) != n or t.dim() != 1 for t in (u, r1, r2, w)):
        raise ValueError("draws: expected u, r1, r2, w [n] and g [n, 3] for one n")
    keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    points = torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev)
    normals = torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev)
    lens = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    if n:
        idx = torch.full((1,), m, dtype=torch.int64, device=dev)
        outs, sfaces = [], []
        for a in range(0, n, surface.MAX_N):                                  # sample_surface takes at most MAX_N points per entry
            b = min(n, a + surface.MAX_N)
            o, _, sf = surface.sample_surface(tables, idx, b - a, u[a:b].reshape(1, -1), r1[a:b].reshape(1, -1), r2[a:b].reshape(1, -1),
                                              validate=False)
            outs.append(o[0])
            sfaces.append(sf[0])
        surf = torch.cat(outs).to(torch.float64).contiguous()
        sface = torch.cat(sfaces).to(torch.int64).contiguous()
        vertices = v32.to(torch.float64).contiguous()
        faces = faces.contiguous()
        g = g.to(device=dev, dtype=torch.float64).contiguous()
        w = w.to(device=dev, dtype=torch.float64).contiguous()
        nv, nf = vertices.shape[0], faces.shape[0]
        ws, nbytes = _lib.workspace("sapcu_ray_fd_samples_workspace_bytes", (nv, nf, n), dev,
                                    "sample_fd_rays: %d vertices, %d faces and %d samples are outside the sampler's range" % (nv, nf, n))
        _lib.call("sapcu_ray_fd_samples_f64", dev, vertices, nv, faces, nf, surf, sface, g, w, n, float(cell_size), points, normals, lens,
                  keep, ws, nbytes, None)
    keep = keep.bool()
    return keep, points[keep].float(), normals[keep].float(), lens[keep].float()


def _watertight_cached(tables, m, faces):
    cache = tables.__dict__.setdefault("_watertight", {})
    if m not in cache:
        cache[m] = is_watertight(faces)
    return cache[m]


def as_fd_npz(points, normals, lens):
    """The dict the reference's script saves as ``fd.npz`` (``np.savez(path, **as_fd_npz(...))``): ``points`` [K,3], ``normals``
    [K,3] and ``lens`` repeated to [K,3], as the script writes it; numpy f32 on the host."""
    host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    points, normals, lens = (host(t).astype(np.float32) for t in (points, normals, lens))
    return {"points": points.reshape(-1, 3), "normals": normals.reshape(-1, 3), "lens": np.repeat(lens.reshape(-1, 1), 3, axis=1)}
