"""Sinkhorn / EMD figures of two clouds on the device, without the n x m cost matrix.

The transport distance of the upsampling literature: the reference's README ("Metrics & Evaluation") lists Sinkhorn figures as the
approximation "to true EMD", names a ``scripts/compute_sinkhorn.py`` that is not in its tree, and has to "downsample GT to save
memory" because its recipe materialises the cost matrix.  Here a half-step recomputes the cost per pair (csrc/sinkhorn.hip,
include/sapcu_sinkhorn.h), so memory is O(n + m).  The iteration counts, the schedule and the names of the figures are this
package's own; tests/sinkhorn_ref.py states the definition in numpy:

* uniform weights; cost ``|x - y|^2 / 2`` for ``p = 2`` (the geomloss convention) and ``|x - y|`` for ``p = 1`` (the EMD of the
  upsampling papers: the mean matched distance); ``eps = blur ** p``;
* ``iters`` alternating iterations (f, then g from the new f) at the final eps from f = g = 0; with ``scaling`` = s in (0, 1) one
  iteration first at each ``eps_k = max(D^p s^(p k), blur^p)``, k = 0, 1, .. up to, not including, the first that equals ``blur^p``
  (D: the diagonal of the common bounding box);
* ``ot`` = <a, f> + <b, g>; ``primal_cost`` = sum_ij P_ij C_ij, the figure that tends to the EMD as blur -> 0; ``marginal_error`` =
  sum_i |sum_j P_ij - a_i| (the column marginals are exact after an iteration); ``divergence`` = ot(a,b) - ot(a,a)/2 - ot(b,b)/2.

Every sum over points is ``metrics.np_sum`` (numpy's order), so the floats equal numpy's on the same device vectors.  The loop
only enqueues launches: nothing is read back inside it.  No CPU path: the HIP library and a device are required.
"""
import ctypes

import numpy as np
import torch

from . import _inputs, _lib
from . import metrics


def split_plan(rows, cols):
    """(tile, shortest planned chunk, chunks, columns per chunk) of a half-step of ``rows`` rows against ``cols`` columns, as
    csrc/sinkhorn.hip plans it: a function of the two counts only.  Host only, no device."""
    out = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().sapcu_internal_sinkhorn_split(int(rows), int(cols), out))
    return tuple(int(v) for v in out)


def eps_schedule(diameter, p, blur, scaling):
    """The eps of the iterations that precede the ``iters`` at ``blur ** p``: [] without ``scaling``."""
    final = float(blur) ** p
    if scaling is None:
        return []
    out, k = [], 0
    while True:
        e = max(float(diameter) ** p * float(scaling) ** (p * k), final)
        if e == final:
            return out
        out.append(e)
        k += 1


def softmin(x, y, pot_y, p, eps):
    """One half-step: f64 [n] = ``-eps log sum_j exp(log(1/m) + pot_y[j]/eps - C(x_i, y_j)/eps)`` for device clouds x [n,3], y [m,3]
    and a device potential pot_y [m]."""
    _check_p(p)
    eps = _positive(eps, "eps")
    x, y = _clouds(x, y)
    if not torch.is_tensor(pot_y) or not pot_y.is_cuda:
        raise RuntimeError("pot_y: expected a device tensor")
    if pot_y.shape != (y.shape[0],):
        raise ValueError("pot_y: expected shape (%d,), got %s" % (y.shape[0], tuple(pot_y.shape)))
    pot_y = pot_y.to(dtype=torch.float64).contiguous()
    n, m = x.shape[0], y.shape[0]
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=x.device)
    ws, nbytes = _workspace(n, m, x.device)
    _lib.call("sapcu_softmin_f64", x.device, x, n, y, m, pot_y, int(p), eps, out, ws, nbytes)
    return out


def sinkhorn_potentials(x, y=None, p=2, blur=0.05, iters=100, scaling=None, *, diameter=None):
    """(f [n], g [m]) after the schedule and ``iters`` iterations; with ``y`` None the potential of the symmetric problem OT(a, a),
    returned twice.  ``diameter`` (for ``scaling``) defaults to the diagonal of the bounding box of both clouds, read back before
    the loop starts."""
    _check_settings(p, blur, iters, scaling)
    given = [_inputs.checked(x, "x", 1, True)] + ([] if y is None else [_inputs.checked(y, "y", 1, True)])
    x, y = (_on_device(given, ("x", "y")) + [None])[:2]
    if scaling is not None and diameter is None:
        diameter = _diameter(x, y)
    return _potentials(x, y, p, blur, iters, eps_schedule(diameter, p, blur, scaling))


def sinkhorn_metrics(pred, gt, p=2, blur=0.05, iters=100, scaling=None, debias=True, downsample_gt=None):
    """The transport figures of one cloud pair, a dict: ``ot``, ``primal_cost``, ``marginal_error``, ``divergence`` (None without
    ``debias``), ``eps``, ``n_pre``, ``n_gt``; floats are ``np.float64``.  ``downsample_gt`` = k keeps k ground-truth points chosen by
    the package's device farthest-point sampling (deterministic; the first point is index n_gt // 2), for comparison with recipes
    that have to shrink the ground truth; nothing here needs it.  ``pred``, ``gt``: [n,3] numpy arrays or device tensors."""
    _check_settings(p, blur, iters, scaling)
    if downsample_gt is not None and (isinstance(downsample_gt, bool) or int(downsample_gt) != downsample_gt or downsample_gt < 1):
        raise ValueError("downsample_gt: expected a positive integer or None")
    pred, gt = _inputs.checked(pred, "pred", 1, True), _inputs.checked(gt, "gt", 1, True)
    if downsample_gt is not None and downsample_gt > gt.shape[0]:
        raise ValueError("downsample_gt = %d exceeds the %d ground-truth points" % (downsample_gt, gt.shape[0]))
    pred, gt = _on_device((pred, gt), ("pred", "gt"))
    if downsample_gt is not None:
        gt = gt[downsampled_indices(gt, downsample_gt)].contiguous()
    n, m = pred.shape[0], gt.shape[0]
    eps = float(blur) ** p
    sched = eps_schedule(_diameter(pred, gt), p, blur, scaling) if scaling is not None else []
    f, g = _potentials(pred, gt, p, blur, iters, sched)
    r, c = plan_stats(pred, gt, f, g, p, eps)
    ot = _ot(f, g)
    out = {"ot": ot, "primal_cost": np.float64(metrics.np_sum(c)), "marginal_error": np.float64(metrics.np_sum((r - 1.0 / n).abs())),
           "divergence": None, "eps": np.float64(eps), "n_pre": n, "n_gt": m}
    if debias:
        fa = _potentials(pred, None, p, blur, iters, sched)[0]
        fb = _potentials(gt, None, p, blur, iters, sched)[0]
        out["divergence"] = ot - 0.5 * _ot(fa, fa) - 0.5 * _ot(fb, fb)
    return out


def dataset_sinkhorn(pairs, **settings):
    """``sinkhorn_metrics`` of every (pred, gt) of ``pairs`` and the means over pairs: {"pairs": [dict, ..], "mean": dict} — the
    mean of each float figure in the order given (``divergence`` None without debias), ``n_pairs``."""
    each = [sinkhorn_metrics(pred, gt, **settings) for pred, gt in pairs]
    if not each:
        raise ValueError("dataset_sinkhorn: no cloud pair")
    mean = {"n_pairs": len(each)}
    for k in ("ot", "primal_cost", "marginal_error", "divergence"):
        vals = [d[k] for d in each]
        mean[k] = None if vals[0] is None else np.float64(np.sum(np.array(vals, dtype=np.float64)) / len(vals))
    return {"pairs": each, "mean": mean}


def plan_stats(x, y, f, g, p, eps):
    """(r [n], c [n]) on the device: the row sums of the plan P_ij = a_i b_j exp((f_i + g_j - C_ij)/eps) and of P_ij C_ij."""
    _check_p(p)
    eps = _positive(eps, "eps")
    x, y = _clouds(x, y)
    n, m = x.shape[0], y.shape[0]
    if tuple(f.shape) != (n,) or tuple(g.shape) != (m,):
        raise ValueError("plan_stats: expected potentials of shapes (%d,) and (%d,)" % (n, m))
    f, g = f.to(dtype=torch.float64).contiguous(), g.to(dtype=torch.float64).contiguous()
    r = torch.full((n,), float("nan"), dtype=torch.float64, device=x.device)
    c = torch.full((n,), float("nan"), dtype=torch.float64, device=x.device)
    ws, nbytes = _workspace(n, m, x.device)
    _lib.call("sapcu_plan_stats_f64", x.device, x, n, y, m, f, g, int(p), eps, r, c, ws, nbytes)
    return r, c


def downsampled_indices(gt, k):
    """The int64 device indices of the ``k`` points ``sinkhorn_metrics(downsample_gt=k)`` keeps of the device cloud ``gt`` f64 [m,3]."""
    from . import pipeline
    return pipeline.farthest_point_sample_device(gt.to(torch.float32).contiguous(), int(k))


# ------------------------------------------------------------------------------------------------------------ internals
def _check_p(p):
    if isinstance(p, bool) or p not in (1, 2):
        raise ValueError("p: expected 1 or 2, got %r" % (p,))


def _positive(v, name):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s: expected a positive finite number, got %r" % (name, v))
    if not (v > 0.0 and np.isfinite(v)):
        raise ValueError("%s: expected a positive finite number, got %r" % (name, v))
    return v


def _check_settings(p, blur, iters, scaling):
    _check_p(p)
    blur = _positive(blur, "blur")
    if not float(blur) ** p > 0.0:
        raise ValueError("blur: %r ** %d underflows" % (blur, p))
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0 or iters > 1 << 20:
        raise ValueError("iters: expected an integer in [0, 2^20], got %r" % (iters,))
    if scaling is not None:
        s = _positive(scaling, "scaling")
        if not s < 1.0:
            raise ValueError("scaling: expected a number in (0, 1) or None, got %r" % (scaling,))


def _clouds(x, y):
    """The clouds of one half-step on one device; y must hold a point, then x."""
    x, y = _inputs.on_device(((x, "x"), (y, "y")), min_rows=(0, 1))
    if x.shape[0] < 1:
        raise ValueError("x: an empty cloud")
    return x, y


def _on_device(given, names):
    """Inputs that passed ``_inputs.checked`` one after the other, uploaded, the device tensors among them tested for NaN."""
    out = _inputs.upload(given)
    _inputs.finite_on_device(given, out, names)
    return out


def _diameter(x, y):
    """The diagonal of the bounding box of both device clouds, in np.float64 (one read-back, before the loop)."""
    both = x if y is None else torch.cat([x, y])
    e = (both.max(dim=0).values - both.min(dim=0).values).cpu().numpy()
    return float(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


def _workspace(n, m, dev):
    return _lib.workspace("sapcu_sinkhorn_workspace_bytes", (n, m), dev,
                          "sinkhorn: clouds of %d and %d points are outside the supported range" % (n, m))


def _potentials(x, y, p, blur, iters, sched):
    """The loop on checked, contiguous f64 device clouds (y None: the symmetric problem); only enqueues."""
    n = x.shape[0]
    m = n if y is None else y.shape[0]
    dev = x.device
    f = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    g = None if y is None else torch.full((m,), float("nan"), dtype=torch.float64, device=dev)
    ws, nbytes = _workspace(n, m, dev)
    arr = (ctypes.c_double * max(len(sched), 1))(*sched)
    _lib.call("sapcu_sinkhorn_f64", dev, x, n, y, m, int(p), arr, len(sched), float(blur) ** p, int(iters), f, g, ws, nbytes)
    return (f, f) if y is None else (f, g)


def _ot(f, g):
    """<a, f> + <b, g> for uniform weights, sums in numpy's order."""
    return np.float64(metrics.np_sum(f)) / f.numel() + np.float64(metrics.np_sum(g)) / g.numel()
