"""PCA normals of a cloud and the angular error of normals on the device.

What the reference computes on the host with ``scripts/generate_gt_normals.py`` (``estimate_normals_pca``: sklearn
``NearestNeighbors(k=16)``, then ``np.cov`` + ``np.linalg.eigh`` per point in a Python loop) and ``scripts/old_metrics/eval_normals.py``
(``angular_error_deg``: mean and median unoriented angle in degrees), with the oriented variant of ``fn/trainer.py:eval_step``.  Here
the neighbours are ``generation.knn_self_grid`` (exact, on the device cell grid), the normals one call of ``sapcu_pca_normals_f64``
per row chunk and the angles one call of ``sapcu_normal_angles_f64`` (csrc/normals.hip; include/sapcu_normals.h states the definition
op for op, tests/normals_ref.py restates it in numpy).  Three uses: score fn's normals against ground truth (``normal_metrics``), make
ground-truth normals for a cloud (``pca_normals``), and score the SURFACE of an upsampled cloud by its own PCA normals against the
ground truth's (``cloud_normal_metrics``).

A PCA normal has no orientation.  ``pca_normals`` fixes the sign by a rule instead of leaving it to the eigen-solver: without a
viewpoint the component of largest magnitude is positive, with one the normal points to the viewpoint's side.

Every float of ``normal_metrics`` equals numpy's on the device's own angle vector (``==``): mean and rms go through numpy's chunked
pairwise sum (``metrics.np_sum``), the median is the average of the two middle values of the sorted vector, the rates are integer
counts.

No CPU path: the HIP library and a device are required.
"""
import ctypes

import numpy as np
import torch

from . import _inputs, _lib
from . import generation
from . import metrics

MAX_K = 64                                       # SAPCU_PCA_NORMALS_MAX_K
THRESHOLDS = (5.0, 10.0, 20.0, 30.0)             # degrees: the shares of angles at or below each ("PGP")
GT_NORMAL_KEYS = ("normals", "fn", "gt_normals")  # the first present is the ground truth of evaluate_normals_file


def normals_from_neighbours(points, idx, viewpoint=None, return_evals=False):
    """The PCA normals of the rows whose neighbour table is ``idx`` int64 [rows,k] (3 <= k <= 64, every entry in [0, n), the row's
    own point first, as ``generation.knn_self_grid`` returns it), ``points`` f64 [n,3], both contiguous on one device: normals f64
    [rows,3], and the eigenvalues f64 [rows,3] ascending with ``return_evals``.  An index outside [0, n) raises ``ValueError`` (no
    out-of-range read happens; the rows concerned come back as NaN from the kernel)."""
    out = _normals_into(points, idx, _viewpoint(viewpoint), return_evals)
    return out if return_evals else out[0]


def pca_normals(points, k=16, viewpoint=None, chunk_rows=1 << 20, return_evals=False):
    """Normals f64 [n,3] on the device of ``points`` ([n,3] numpy or device tensor of any float dtype): for every point the
    eigenvector of the smallest eigenvalue of the covariance of its min(k, n) nearest points, itself included
    (``estimate_normals_pca``).  ``viewpoint`` (three numbers) turns every normal to that side; None makes the component of largest
    magnitude positive.  ``return_evals``: additionally the eigenvalues f64 [n,3], ascending.  The rows are processed ``chunk_rows``
    at a time (the neighbour table of a chunk is chunk_rows x k x 16 bytes); the result does not depend on it.  Raises ``ValueError``
    for n < 3, k < 3, min(k, n) > 64 or a non-finite coordinate."""
    points = _inputs.checked(points, "points")
    n = int(points.shape[0])
    k = int(k)
    if n < 3:
        raise ValueError("pca_normals: a cloud of %d points (at least 3 are needed)" % n)
    if k < 3:
        raise ValueError("pca_normals: k = %d (at least 3 neighbours are needed)" % k)
    k_eff = min(k, n)
    if k_eff > MAX_K:
        raise ValueError("pca_normals: min(k, n) = %d is above %d" % (k_eff, MAX_K))
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("pca_normals: chunk_rows = %d" % chunk_rows)
    view = _viewpoint(viewpoint)
    pts = _inputs.on_device(((points, "points"),), finite=True)[0]
    normals = torch.full((n, 3), float("nan"), dtype=torch.float64, device=pts.device)
    evals = torch.full((n, 3), float("nan"), dtype=torch.float64, device=pts.device) if return_evals else None
    for r0 in range(0, n, chunk_rows):
        r1 = min(n, r0 + chunk_rows)
        idx, _ = generation.knn_self_grid(pts, k_eff, rows=(r0, r1))
        _normals_into(pts, idx, view, return_evals, normals[r0:r1], None if evals is None else evals[r0:r1])
    return (normals, evals) if return_evals else normals


def normal_angles(a, b, oriented=False, clamp_eps=0.0, return_cos=False):
    """The angle in degrees, f64 [n] on the device, between the rows of two normal tables ([n,3] numpy or device tensors of any float
    dtype, any length): ``angular_error_deg`` of the reference's script (unoriented: 0 .. 90) or, with ``oriented=True,
    clamp_eps=1e-6``, the angle of fn's trainer (0 .. 180, the cosine clamped to +-(1 - 1e-6)).  A zero normal gives 90 degrees, a NaN
    stays a NaN.  ``return_cos``: additionally the clamped cosine."""
    a, b = _inputs.on_device(((a, "a"), (b, "b")))
    if a.shape[0] != b.shape[0]:
        raise ValueError("normal_angles: %d and %d rows" % (a.shape[0], b.shape[0]))
    clamp_eps = float(clamp_eps)
    if not 0.0 <= clamp_eps <= 1.0:
        raise ValueError("normal_angles: clamp_eps = %r is outside [0, 1]" % clamp_eps)
    rows = a.shape[0]
    deg = torch.full((rows,), float("nan"), dtype=torch.float64, device=a.device)
    cos = torch.full((rows,), float("nan"), dtype=torch.float64, device=a.device) if return_cos else None
    if rows:
        _lib.call("sapcu_normal_angles_f64", a.device, a, b, rows, 1 if oriented else 0, clamp_eps, cos, deg)
    return (deg, cos) if return_cos else deg


def normal_metrics(pred_normals, gt_normals, pred_points=None, gt_points=None, oriented=False, clamp_eps=0.0, thresholds=THRESHOLDS):
    """The figures of predicted against ground-truth normals, a dict: ``mean_deg``, ``median_deg``, ``rms_deg`` of the angles of
    ``normal_angles``, ``pgp`` (a tuple: the share of angles <= each of ``thresholds``, in degrees) and ``count``.  Floats are
    ``np.float64`` and equal numpy's on the same angles.

    With ``pred_points`` and ``gt_points`` ([n,3] and [m,3], one row per normal) every predicted point is scored against the normal
    of its nearest ground-truth point (``metrics.nearest``); without them the two tables must have the same number of rows.  (The
    reference's script, given tables of different lengths, matches each normal to the most similar NORMAL, which scores nothing;
    here the match is by position.)"""
    if (pred_points is None) != (gt_points is None):
        raise ValueError("normal_metrics: pred_points and gt_points go together")
    a, b = _inputs.on_device(((pred_normals, "pred_normals"), (gt_normals, "gt_normals")))
    if pred_points is None:
        if a.shape[0] != b.shape[0]:
            raise ValueError("normal_metrics: %d predicted and %d ground-truth normals, and no points to match them by"
                             % (a.shape[0], b.shape[0]))
    else:
        pp, gp = _inputs.on_device(((pred_points, "pred_points"), (gt_points, "gt_points")), device=a.device)
        if pp.shape[0] != a.shape[0] or gp.shape[0] != b.shape[0]:
            raise ValueError("normal_metrics: %d / %d predicted points / normals, %d / %d ground-truth points / normals"
                             % (pp.shape[0], a.shape[0], gp.shape[0], b.shape[0]))
        _inputs.finite_on_device((pp, gp), (pp, gp), ("pred_points", "gt_points"))       # after the row counts, so both on the device
        b = b[metrics.nearest(pp, gp)[1]] if pp.shape[0] else b[:0]
    if a.shape[0] < 1:
        raise ValueError("normal_metrics: no normal to score")
    return _figures(normal_angles(a, b, oriented, clamp_eps), thresholds)


def cloud_normal_metrics(pred_points, gt_points, gt_normals, k=16, **kw):
    """``normal_metrics`` of the PCA normals of ``pred_points`` (``pca_normals(pred_points, k)``) against the ground truth, matched
    by position: how well the surface of an upsampled cloud follows the ground truth's, whatever the two point counts.  Unoriented
    unless ``oriented=True`` is passed (a PCA normal has no side)."""
    return normal_metrics(pca_normals(pred_points, k), gt_normals, pred_points, gt_points, **kw)


def evaluate_normals_file(pred_npz, gt_npz, device="cuda", **kw):
    """``normal_metrics`` of two ``.npz`` files with the keys ``points`` and ``normals`` that the reference's
    ``generate_gt_normals.py`` writes.  The ground truth's normals are the first present of ``normals``, ``fn``, ``gt_normals``.
    With ``points`` in both files the match is by position, otherwise the row counts must agree."""
    with np.load(pred_npz) as pred, np.load(gt_npz) as gt:
        if "normals" not in pred.files:
            raise ValueError("%s: no array 'normals'" % pred_npz)
        key = next((name for name in GT_NORMAL_KEYS if name in gt.files), None)
        if key is None:
            raise ValueError("%s: none of the arrays %s" % (gt_npz, ", ".join(GT_NORMAL_KEYS)))
        pn, gn = pred["normals"], gt[key]
        both = "points" in pred.files and "points" in gt.files
        pp, gp = (pred["points"], gt["points"]) if both else (None, None)
    dev = torch.device(device)
    put = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return normal_metrics(put(pn), put(gn), put(pp), put(gp), **kw)


# ------------------------------------------------------------------------------------------------------------ internals
def _viewpoint(viewpoint):
    """None, or the viewpoint as a host double[3]."""
    if viewpoint is None:
        return None
    if torch.is_tensor(viewpoint):
        viewpoint = viewpoint.detach().cpu().numpy()
    v = np.asarray(viewpoint, dtype=np.float64).reshape(-1)
    if v.shape != (3,) or not np.isfinite(v).all():
        raise ValueError("viewpoint: expected three finite numbers, got %r" % (viewpoint,))
    return (ctypes.c_double * 3)(*v.tolist())


def _normals_into(pts, idx, view, want_evals, normals=None, evals=None):
    """One call of sapcu_pca_normals_f64 on a table; the outputs are written in place when given (contiguous row slices)."""
    if not (torch.is_tensor(pts) and pts.is_cuda and pts.dtype == torch.float64 and pts.dim() == 2 and pts.shape[1] == 3 and
            pts.is_contiguous()):
        raise ValueError("points: expected a contiguous f64 [n,3] device tensor")
    if not (torch.is_tensor(idx) and idx.device == pts.device and idx.dtype == torch.int64 and idx.dim() == 2 and idx.is_contiguous()):
        raise ValueError("idx: expected a contiguous int64 [rows,k] tensor on the points' device")
    rows, k = idx.shape
    if not 3 <= k <= MAX_K:
        raise ValueError("idx: k = %d is outside 3 .. %d" % (k, MAX_K))
    if pts.shape[0] < 1:
        raise ValueError("points: an empty cloud")
    dev = pts.device
    if normals is None:
        normals = torch.full((rows, 3), float("nan"), dtype=torch.float64, device=dev)
    if want_evals and evals is None:
        evals = torch.full((rows, 3), float("nan"), dtype=torch.float64, device=dev)
    assert normals.is_contiguous() and (evals is None or evals.is_contiguous())
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.call("sapcu_pca_normals_f64", dev, pts, pts.shape[0], idx, rows, k, view, normals, evals if want_evals else None, bad)
    nbad = int(bad.item())
    if nbad:
        raise ValueError("idx: %d entries outside [0, %d)" % (nbad, pts.shape[0]))
    return normals, evals


def _host_figures(n, total, total_sq, mid_lo, mid_hi, counts):
    """The host arithmetic of normal_metrics in np.float64: np.mean, np.median, sqrt(np.mean(x * x)) and np.mean(x <= t) from the
    sum, the sum of squares, the two middle values of the sorted vector (equal for an odd n) and the integer counts."""
    n = int(n)
    return {"mean_deg": np.float64(total) / n, "median_deg": (np.float64(mid_lo) + np.float64(mid_hi)) / 2.0,
            "rms_deg": np.sqrt(np.float64(total_sq) / n), "pgp": tuple(np.float64(int(c)) / n for c in counts), "count": n}


def _figures(deg, thresholds):
    n = deg.numel()
    if bool(torch.isnan(deg).any()):
        mid_lo = mid_hi = float("nan")                                     # np.median of a vector with a NaN
    else:
        ordered = torch.sort(deg).values
        mid_lo, mid_hi = ordered[(n - 1) // 2].item(), ordered[n // 2].item()
    counts = [int((deg <= float(t)).sum()) for t in thresholds]
    return _host_figures(n, metrics.np_sum(deg), metrics.np_sum(deg * deg), mid_lo, mid_hi, counts)
