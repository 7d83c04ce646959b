"""Seed-centred training samples of fn from a surface cloud, on the device: query points in a band off the surface, each with
the unit vector from the query towards the mean of its k nearest surface points.

This is the reference's ``scripts/sample_mesh-fn.py`` (``export_pointing``), which writes ``fn.npz`` for the folder route of fn's
training (``fn/field.py:fnField``, ``fn/transform.py:Subsamplefn``): the voxels of a coarse lattice whose centre lies near the
surface cloud (``near_voxels``), their fine cells jittered into candidates, one kNN query per candidate, the band test on the
first distance and the pointing direction (``pointing_samples``, one kernel: csrc/pointing.hip).  csrc/sapcu_pointing.h has the
definition, operation by operation; tests/pointing_ref.py states it in numpy; every output equals it bit for bit.  The script's
random streams (trimesh's even sampler, numpy's ``rand`` and ``shuffle``) are not reproduced: ``sample_fn_pointing`` draws from a
device generator.

No CPU path: the HIP library and a device are required.
"""
import ctypes
import functools
import math

import numpy as np
import torch

from . import _inputs, _lib, metrics, surface as surface_mod

MAX_K = 16                     # SAPCU_POINTING_MAX_K
MAX_SUB, MAX_COUNT = 1024, 1024
SURFACE_CHUNK = 4096           # points per entry of the surface sampling in sample_fn_pointing
GEOMETRY = ("origin", "step", "count", "near", "sub", "k", "band", "cell_size", "voxels_per_call")


def _geometry(origin, step, count):
    origin, step, count = float(origin), float(step), int(count)
    if not (math.isfinite(origin) and math.isfinite(step) and step > 0):
        raise ValueError("origin and step: need finite numbers and step > 0, got %r, %r" % (origin, step))
    if not 1 <= count <= MAX_COUNT:
        raise ValueError("count: need 1 <= count <= %d, got %d" % (MAX_COUNT, count))
    return origin, step, count


def _surface(surface):
    """The surface cloud as a contiguous f32 [n,3] device tensor (the script's ``points.astype(float32)``)."""
    if not torch.is_tensor(surface):
        raise ValueError("surface: expected a device tensor")
    if not surface.is_cuda:
        raise RuntimeError("surface: a CPU tensor (there is no CPU path)")
    s = _inputs.device_tensor(surface.device, "the surface", surface, "surface", torch.float32, (None, 3))
    if not 1 <= s.shape[0] <= 2 ** 29:
        raise ValueError("surface: need 1 <= n <= 2^29 points, got %d" % s.shape[0])
    return s


def near_voxels(surface, origin=-1.0, step=0.05, count=50, near=None):
    """The voxels of the ``count``^3 lattice (corner ``i * step + origin`` per axis, centre ``corner + step / 2``) whose centre is
    closer than ``near`` (default ``step + 0.01``; strict) to the nearest point of ``surface`` f32 [n,3] (device): their ids
    ``(ix * count + iy) * count + iz`` ascending, int64 on the device.  The distances are ``metrics.nearest``'s; a centre farther
    than ``near`` from the cloud's bounding box is left out before the search, which changes no result."""
    origin, step, count = _geometry(origin, step, count)
    near = step + 0.01 if near is None else float(near)
    if math.isnan(near):
        raise ValueError("near: NaN")
    s = _surface(surface)
    axis = (torch.arange(count, dtype=torch.float64, device=s.device) * step + origin) + step / 2
    centres = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1).reshape(-1, 3)
    cloud = s.double()
    if not (near > 0 and math.isfinite(near)):
        rows = torch.arange(centres.shape[0], device=s.device)
    else:
        # a centre farther than `near` from the cloud's bounding box is farther from every point: only the others are searched
        # (most of a lattice lies far outside the box, where a search walks the whole grid).  1e-6 relative on the square is far
        # above the rounding of the three products and two sums; a NaN coordinate makes the box NaN and drops nothing
        gap = torch.clamp_min(torch.maximum(cloud.amin(0) - centres, centres - cloud.amax(0)), 0.0)
        rows = torch.nonzero(~((gap * gap).sum(1) > near * near * (1 + 1e-6))).reshape(-1)
    dist, _ = metrics.nearest(centres[rows], cloud)
    return rows[dist < near]


def pointing_samples(surface, voxels, jitter=None, sub=10, k=10, band=(0.003, 0.03), origin=-1.0, step=0.05, count=50, cell_size=0.0,
                     voxels_per_call=1024, return_all=False, info=None):
    """The pointing samples of the voxels ``voxels`` int64 [nv] (``near_voxels``) of ``surface`` f32 [n,3], device tensors.
    Candidate ``t * sub^3 + (jx * sub + jy) * sub + jz`` lies at ``((corner + jc * (step / sub)) + (step / sub) / 2) + jitter`` per axis
    (``jitter`` f64 [nv * sub^3, 3], None: nothing is added); it is kept when it has ``k`` neighbours and the distance to the
    nearest lies in ``band`` (both ends inclusive) -> a dict of device tensors, kept candidates in ascending order: ``points`` f64
    [K,3], ``pointing`` f64 [K,3] (unit; NaN where the neighbours' mean is the point itself), ``candidate`` int64 [K].  With
    ``return_all`` also ``keep`` bool [m], ``d1`` f64 [m] and ``idx`` int32 [m,k] of every candidate (-1 / +inf: no neighbour).
    The voxels are taken ``voxels_per_call`` at a time (the result does not depend on it), one read-back of the count per call;
    ``cell_size`` 0 = automatic (any value gives the same result); ``info``, a list, receives [1 if the grid ran else 0 (brute
    force), gx, gy, gz] of the last call."""
    origin, step, count = _geometry(origin, step, count)
    sub, k, per = int(sub), int(k), int(voxels_per_call)
    if not 1 <= sub <= MAX_SUB:
        raise ValueError("sub: need 1 <= sub <= %d, got %d" % (MAX_SUB, sub))
    if not 1 <= k <= MAX_K:
        raise ValueError("k: need 1 <= k <= %d, got %d" % (MAX_K, k))
    if per < 1:
        raise ValueError("voxels_per_call must be >= 1")
    lo, hi = (float(b) for b in band)
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError("band: NaN")
    cell_size = float(cell_size)
    if not (math.isfinite(cell_size) and cell_size >= 0):
        raise ValueError("cell_size: need a finite number >= 0, got %r" % cell_size)
    s = _surface(surface)
    n, dev, sub3 = s.shape[0], s.device, sub ** 3
    if k > n:
        raise ValueError("k must be less than or equal to the number of surface points (k=%d, n=%d)" % (k, n))
    dev_tensor = functools.partial(_inputs.device_tensor, dev, "the surface")
    voxels = dev_tensor(voxels, "voxels", torch.int64, (None,))
    nv = voxels.shape[0]
    jitter = dev_tensor(jitter, "jitter", torch.float64, (nv * sub3, 3), optional=True)
    step2 = step / sub
    half2 = step2 / 2
    parts, every = [], []
    out = (ctypes.c_int64 * 4)()
    for t0 in range(0, nv, per):
        t1 = min(t0 + per, nv)
        m = (t1 - t0) * sub3
        ws, nbytes = _lib.workspace("sapcu_pointing_workspace_bytes", (n, t1 - t0, sub, k), dev,
                                    "pointing_samples: %d voxels of %d candidates each are outside the range of one call" % (t1 - t0, sub3))
        keep = torch.zeros((m,), dtype=torch.uint8, device=dev)
        d1 = torch.full((m,), float("nan"), dtype=torch.float64, device=dev) if return_all else None
        idx = torch.full((m, k), -1, dtype=torch.int32, device=dev) if return_all else None
        points = torch.zeros((m, 3), dtype=torch.float64, device=dev)
        pointing = torch.zeros((m, 3), dtype=torch.float64, device=dev)
        candidate = torch.zeros((m,), dtype=torch.int64, device=dev)
        kept = torch.zeros((1,), dtype=torch.int64, device=dev)
        _lib.call("sapcu_pointing_samples_f32", dev, s, n, voxels[t0:t1], t1 - t0, origin, step, count, sub, step2, half2,
                  None if jitter is None else jitter[t0 * sub3:t1 * sub3], k, lo, hi, cell_size, t0 * sub3, keep, d1, idx, points, pointing,
                  candidate, kept, ws, nbytes, out)
        c = int(kept.item())
        parts.append((points[:c], pointing[:c], candidate[:c]))
        every.append((keep, d1, idx))
    if info is not None:
        info[:] = list(out)
    if parts:
        res = {name: torch.cat([p[j] for p in parts]) for j, name in enumerate(("points", "pointing", "candidate"))}
    else:
        res = {"points": torch.zeros((0, 3), dtype=torch.float64, device=dev), "pointing": torch.zeros((0, 3), dtype=torch.float64, device=dev),
               "candidate": torch.zeros((0,), dtype=torch.int64, device=dev)}
    if return_all:
        if every:
            res.update(keep=torch.cat([e[0] for e in every]).bool(), d1=torch.cat([e[1] for e in every]), idx=torch.cat([e[2] for e in every]))
        else:
            res.update(keep=torch.zeros((0,), dtype=torch.bool, device=dev), d1=torch.zeros((0,), dtype=torch.float64, device=dev),
                       idx=torch.zeros((0, k), dtype=torch.int32, device=dev))
    return res


def sample_fn_pointing(tables, mesh_idx, surface_points, gen, pointing_size=50000, **geometry):
    """One run of ``export_pointing`` for mesh ``mesh_idx`` of ``tables`` (``surface.build_surface_tables``): a surface cloud of
    ``surface_points`` area-weighted points (``surface.sample_surface`` on repeated entries of the one mesh, 4096 points each),
    ``near_voxels``, a jitter of ``torch.rand * 0.001`` per candidate, ``pointing_samples``, then a ``torch.randperm`` of the kept
    candidates cut to ``pointing_size`` -> a dict: ``points`` f64 [K,3], ``pointing`` f64 [K,3], ``candidate`` int64 [K] and
    ``surface`` f32 [surface_points,3].  Every draw comes from the device generator ``gen`` in this order: ``u`` (f64), ``r1``, ``r2``
    (f64 rounded to f32), the jitter, the permutation.  ``geometry``: ``origin``, ``step``, ``count``, ``near``, ``sub``, ``k``, ``band``,
    ``cell_size``, ``voxels_per_call`` as the two functions take them."""
    unknown = sorted(set(geometry) - set(GEOMETRY))
    if unknown:
        raise ValueError("sample_fn_pointing: unknown arguments %s" % ", ".join(unknown))
    if not isinstance(tables, surface_mod.SurfaceTables):
        raise ValueError("tables: expected the result of build_surface_tables")
    surface_points, pointing_size, mesh_idx = int(surface_points), int(pointing_size), int(mesh_idx)
    if surface_points < 1 or pointing_size < 1:
        raise ValueError("surface_points and pointing_size must be >= 1")
    if not 0 <= mesh_idx < len(tables):
        raise ValueError("mesh_idx: %d outside [0, %d)" % (mesh_idx, len(tables)))
    dev = tables.device
    b = -(-surface_points // SURFACE_CHUNK)
    u = torch.rand((b, SURFACE_CHUNK), generator=gen, device=dev, dtype=torch.float64)
    r1 = torch.rand((b, SURFACE_CHUNK), generator=gen, device=dev, dtype=torch.float64).float()
    r2 = torch.rand((b, SURFACE_CHUNK), generator=gen, device=dev, dtype=torch.float64).float()
    entries = torch.full((b,), mesh_idx, dtype=torch.int64, device=dev)
    cloud = surface_mod.sample_surface(tables, entries, SURFACE_CHUNK, u, r1, r2, validate=False)[0].reshape(-1, 3)[:surface_points].contiguous()
    lattice = {name: geometry[name] for name in ("origin", "step", "count") if name in geometry}
    voxels = near_voxels(cloud, near=geometry.get("near"), **lattice)
    sub = int(geometry.get("sub", 10))
    jitter = torch.rand((voxels.shape[0] * sub ** 3, 3), generator=gen, device=dev, dtype=torch.float64) * 0.001
    out = pointing_samples(cloud, voxels, jitter, **{name: v for name, v in geometry.items() if name != "near"})
    order = torch.randperm(out["points"].shape[0], generator=gen, device=dev)[:pointing_size]
    return {"points": out["points"][order], "pointing": out["pointing"][order], "candidate": out["candidate"][order], "surface": cloud}


def as_fn_npz(points, pointing):
    """The arrays of one ``fn.npz`` as a dict for ``np.savez``: ``points`` and ``pointing`` f64 as the script writes them, and
    ``normals``, the same array as ``pointing``, the key ``fn/field.py:fnField`` reads."""
    p = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    d = pointing.detach().cpu().numpy() if torch.is_tensor(pointing) else np.asarray(pointing)
    p, d = np.ascontiguousarray(p, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3 or p.shape != d.shape:
        raise ValueError("as_fn_npz: expected points and pointing [K, 3], got %s and %s" % (list(p.shape), list(d.shape)))
    return {"points": p, "pointing": d, "normals": d}
