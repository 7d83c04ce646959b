"""Poisson-disk sampling of clouds and meshes on the device: blue-noise subsets of exactly n points.

The clouds the reference trains fd on and the PU-GAN / PU1K protocol evaluates on are "poisson disk sampled" (the h5 keys
``poisson_256`` / ``poisson_1024`` of fd/datacore.py, README.md of the reference); the reference holds no sampler for them, its
files came from outside.  Here a cloud is thinned by dart throwing with a priority order: ``poisson_select`` keeps a row iff no
kept lower row lies within the radius, ``poisson_subsample`` bisects the radius until the selection holds at least ``n`` rows and
returns the first ``n`` of them, and ``poisson_disk_sample`` does that to an area-weighted sampling of a mesh
(``surface.sample_surface``), the candidates in draw order.  csrc/sapcu_poisson.h has the definition, operation by operation;
tests/poisson_ref.py states it in numpy; every output equals it bit for bit, whatever the scheduling.

Clouds of at most ``PD_RESIDENT_MAX`` points run in one launch per call (one work group per batch entry, no read-back:
capturable into a graph); larger ones, up to 2^24 points, on a device cell grid with one launch per round and host read-backs.

No CPU path: the HIP library and a device are required.
"""
import math

import torch

from . import _lib, surface

PD_RESIDENT_MAX = 8192         # SAPCU_PD_RESIDENT_MAX
MAX_C, MAX_B, MAX_STEPS = 2 ** 24, 65535, 64


def _cloud(points):
    """(points f32 [b,C,3] contiguous, whether a batch dimension was given)."""
    if not torch.is_tensor(points):
        raise ValueError("points: expected a device tensor")
    if not points.is_cuda:
        raise RuntimeError("points: a CPU tensor (there is no CPU path)")
    batched = points.dim() == 3
    if points.dim() not in (2, 3) or points.shape[-1] != 3:
        raise ValueError("points: expected [C, 3] or [b, C, 3], got %s" % list(points.shape))
    if not points.dtype.is_floating_point:
        raise ValueError("points: expected a floating dtype")
    p = points.to(torch.float32).contiguous()
    p = p if batched else p[None]
    b, C = p.shape[0], p.shape[1]
    if not 1 <= C <= MAX_C or b > MAX_B:
        raise ValueError("points: need 1 <= C <= 2^24 points and at most %d entries, got %s" % (MAX_B, list(points.shape)))
    return p, batched


def _finite(points, validate):
    if validate and not bool(torch.isfinite(points).all()):
        raise ValueError("points contains NaN or infinity")


def _workspace(b, C, dev):
    return _lib.workspace("sapcu_poisson_workspace_bytes", (b, C), dev,
                          "points: %d entries of %d points are outside the range of the call" % (b, C))


def poisson_select(points, radius, validate=True, path=None):
    """The rows of ``points`` f32 [C,3] or [b,C,3] (device) that dart throwing in row order keeps at ``radius`` (a number, or one per
    entry [b]): row i is kept iff no kept row j < i has squared distance ``(dx*dx + dy*dy) + dz*dz < radius * radius`` in f32 —
    strict, so radius 0 keeps everything -> (keep bool [b,C], count int32 [b], rounds int32 [b]: the synchronous rounds the
    selection took); without the batch dimension when ``points`` has none.  A radius that is negative or not finite, and (one
    synchronisation; ``validate=False`` skips it, the kernel then keeps nothing of such an entry) a coordinate that is not finite:
    ValueError.  ``path="grid"`` forces the cell-grid path at any C, one round per read-back (tests)."""
    if not torch.is_tensor(radius) and not (math.isfinite(float(radius)) and float(radius) >= 0):
        raise ValueError("radius: negative or not finite (%r)" % (radius,))
    if path not in (None, "grid"):
        raise ValueError("path: None or 'grid'")
    p, batched = _cloud(points)
    b, C, dev = p.shape[0], p.shape[1], p.device
    if torch.is_tensor(radius):
        if radius.dim() > 1 or (radius.dim() == 1 and radius.shape[0] != b) or not radius.dtype.is_floating_point:
            raise ValueError("radius: expected a number or a floating tensor [%d], got %s" % (b, list(radius.shape)))
        r = radius.to(device=dev, dtype=torch.float32).reshape(-1).expand(b).contiguous()
        if validate and b and not bool((torch.isfinite(r) & (r >= 0)).all()):
            raise ValueError("radius: negative or not finite")
    else:
        r = torch.full((b,), float(radius), dtype=torch.float32, device=dev)
    _finite(p, validate)
    keep = torch.zeros((b, C), dtype=torch.uint8, device=dev)
    count = torch.zeros((b,), dtype=torch.int32, device=dev)
    rounds = torch.zeros((b,), dtype=torch.int32, device=dev)
    if b:
        ws, nbytes = _workspace(b, C, dev)
        _lib.call("sapcu_poisson_select_f32" if path is None else "sapcu_internal_poisson_select_grid", dev, p, b, C, r, keep, count,
                  rounds, ws, nbytes)
    keep = keep.bool()
    return (keep, count, rounds) if batched else (keep[0], count[0], rounds[0])


def poisson_subsample(points, n, steps=20, validate=True):
    """Exactly ``n`` rows of ``points`` f32 [C,3] or [b,C,3] (device) with blue-noise spacing: ``steps`` bisection steps on the radius
    between 0 and the bounding box's diagonal, keeping the largest radius tried whose ``poisson_select`` holds at least n rows, then
    the first n rows of that selection -> (idx int32 [b,n] ascending, radius f32 [b], count int32 [b] >= n: the rows that
    selection holds, rounds int32 [b]: summed over the steps + 1 selections); without the batch dimension when ``points`` has none.
    ``n`` outside [1, C], ``steps`` outside [0, 64] and (``validate``, one synchronisation) coordinates that are not finite:
    ValueError; with ``validate=False`` such an entry comes back as idx -1, count 0."""
    p, batched = _cloud(points)
    b, C, dev = p.shape[0], p.shape[1], p.device
    n, steps = int(n), int(steps)
    if not 1 <= n <= C:
        raise ValueError("n: need 1 <= n <= %d points, got %d" % (C, n))
    if not 0 <= steps <= MAX_STEPS:
        raise ValueError("steps: need 0 <= steps <= %d, got %d" % (MAX_STEPS, steps))
    _finite(p, validate)
    idx = torch.full((b, n), -1, dtype=torch.int32, device=dev)
    radius = torch.zeros((b,), dtype=torch.float32, device=dev)
    count = torch.zeros((b,), dtype=torch.int32, device=dev)
    rounds = torch.zeros((b,), dtype=torch.int32, device=dev)
    if b:
        ws, nbytes = _workspace(b, C, dev)
        _lib.call("sapcu_poisson_subsample_f32", dev, p, b, C, n, steps, idx, radius, count, rounds, ws, nbytes)
    return (idx, radius, count, rounds) if batched else (idx[0], radius[0], count[0], rounds[0])


def poisson_disk_sample(tables, mesh_idx, n, u, r1, r2, steps=20, validate=True):
    """``n`` Poisson-disk points on each of b meshes: the draws ``u`` f64, ``r1``, ``r2`` f32 [b,C] give C area-weighted candidates
    per entry as ``surface.sample_surface`` takes them (C may exceed ``surface.MAX_N``: the draws are then sampled in slices of one
    entry's columns, which changes no value), and ``poisson_subsample`` keeps n of them, the candidates in draw order -> (points
    f32 [b,n,3], normals f32 [b,n,3], faces int32 [b,n], radius f32 [b], count int32 [b], idx int32 [b,n]: the draws kept).
    ``validate=False`` skips the value checks of both steps (for stream capture when C <= PD_RESIDENT_MAX)."""
    if not torch.is_tensor(u) or u.dim() != 2:
        raise ValueError("u: expected a device tensor [b, C]")
    C = u.shape[1]
    if not 1 <= int(n) <= C:
        raise ValueError("n: need 1 <= n <= %d candidates, got %d" % (C, int(n)))
    parts = [surface.sample_surface(tables, mesh_idx, min(surface.MAX_N, C - c0), u[:, c0:c0 + surface.MAX_N], r1[:, c0:c0 + surface.MAX_N],
                                    r2[:, c0:c0 + surface.MAX_N], validate=validate) for c0 in range(0, C, surface.MAX_N)]
    points, normals, faces = (parts[0] if len(parts) == 1 else tuple(torch.cat([p[j] for p in parts], 1) for j in range(3)))
    idx, radius, count, _ = poisson_subsample(points, n, steps, validate=validate)
    rows = idx.clamp(min=0).long()
    pick = rows[..., None].expand(-1, -1, 3)
    return (torch.gather(points, 1, pick), torch.gather(normals, 1, pick), torch.gather(faces, 1, rows), radius, count, idx)
