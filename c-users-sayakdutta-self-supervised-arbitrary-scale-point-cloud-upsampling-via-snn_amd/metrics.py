"""Chamfer distance, Hausdorff distance, precision / recall and F-score of two clouds on the device.

The quantities the reference's ``external/Meta-PU_evaluation/evaluation_code/evaluation_cd.py`` prints (without EMD), plus the
Hausdorff distance its README lists.  That script runs two ``sklearn.neighbors.NearestNeighbors(n_neighbors=1)`` queries per cloud
pair on the host; here both are one call of ``sapcu_nn_cross_grid_f64`` (csrc/metrics.hip, include/sapcu_metrics.h), whose distances
equal sklearn's bit for bit, and every float below equals numpy's (``==``), because the order of every operation is fixed:

* mean: ``generation.outlier_stats_device`` on the [n, 1] distance table (numpy's pairwise sums of ``np.getbufsize()``-element
  chunks), the chunk sums added in sequence by ``generation.outlier_global_mean``;
* std: numpy's ``_var`` — ``x = d - mean`` and ``x * x`` as two f64 operations on the device, the same chunked sum, then ``/ n``
  and ``sqrt`` on the host in ``np.float64``;
* rates: an integer count on the device over ``n`` (a 0/1 sum is exact in any order);
* cd, fscore: host ``np.float64`` arithmetic in the script's order.

No CPU path: the HIP library and a device are required.
"""
import ctypes

import numpy as np
import torch

from . import _inputs, _lib
from . import generation

THRESHOLDS = (1e-2, 2e-2)


def nearest(queries, cloud, cell_size=0.0, info=None):
    """Exact nearest neighbour of every query f64 [nq,3] in ``cloud`` f64 [n,3], both on the device: (dist f64 [nq], idx int64 [nq]),
    bit for bit ``knn_gather(cloud, queries, 1, want_dist=True)``.  ``cell_size`` 0 = automatic (any value gives the same result).
    ``info``, a list, receives [1 if the grid ran else 0 (brute force), gx, gy, gz].  Synchronises the current stream once."""
    queries, cloud = _inputs.on_device(((queries, "queries"), (cloud, "cloud")), min_rows=(0, 1))
    n, nq = cloud.shape[0], queries.shape[0]
    dev = cloud.device
    dist = torch.full((nq,), float("nan"), dtype=torch.float64, device=dev)
    idx = torch.full((nq,), -1, dtype=torch.int64, device=dev)
    out = (ctypes.c_int64 * 4)()
    if nq:
        ws, nbytes = _lib.workspace("sapcu_nn_cross_workspace_bytes", (n, nq), dev,
                                    "nearest: a cloud of %d points and %d queries are outside the search's range" % (n, nq))
        _lib.call("sapcu_nn_cross_grid_f64", dev, cloud, n, queries, nq, float(cell_size), dist, idx, ws, nbytes, out)
    if info is not None:
        info[:] = list(out)
    return dist, idx


def cloud_metrics(pred, gt, thresholds=THRESHOLDS):
    """The figures of one cloud pair, a dict: ``gt2pre_mean / _std / _max`` and ``recall`` (a tuple, one rate per threshold) of the
    distances from every ground-truth point to its nearest predicted point; ``pre2gt_mean / _std / _max`` and ``precision`` the other
    way; ``cd`` = 0.5 (gt2pre_mean + pre2gt_mean); ``fscore`` = 2 / (1 / recall + 1 / precision) per threshold (0.0 where either
    rate is 0); ``hausdorff`` = max(gt2pre_max, pre2gt_max); ``n_gt``, ``n_pre``.  Floats are ``np.float64`` and equal numpy's on
    the same distances.  ``pred``, ``gt``: [n,3] numpy arrays or device tensors of any float dtype, contiguous or not."""
    gt2pre, pre2gt = _pair_distances(pred, gt)
    return _figures(gt2pre, pre2gt, thresholds)


def dataset_metrics(pairs, thresholds=THRESHOLDS):
    """The pooled figures of ``evaluation_cd.py`` over ``pairs``, an iterable of (pred, gt): the distance vectors of all pairs
    concatenated in the order given, then the statistics of ``cloud_metrics`` (``n_gt`` / ``n_pre``: the pooled counts)."""
    both = [_pair_distances(pred, gt) for pred, gt in pairs]
    if not both:
        raise ValueError("dataset_metrics: no cloud pair")
    return _figures(torch.cat([a for a, _ in both]), torch.cat([b for _, b in both]), thresholds)


def np_sum(v, bufsize=None):
    """np.sum of a device f64 vector in numpy's order (pairwise within chunks of ``bufsize`` elements, None = ``np.getbufsize()``,
    the chunk sums added in sequence), as a Python float."""
    _, sums = generation.outlier_stats_device(v.view(-1, 1), bufsize)
    return generation.outlier_global_mean(sums.cpu(), 1)


def moments(d, ddof, bufsize=None):
    """(mean, std, min, max) of a device f64 vector as ``np.float64``, equal to numpy's: ``np.mean``, numpy's ``_var`` (the
    deviations and their squares as two f64 operations on the device, the same chunked sum) and ``sqrt`` on the host.  ``ddof`` 0
    divides by n, as ``np.std``; ``ddof`` 1 by ``np.float64(n - 1)``, the sample deviation, NaN for a single value."""
    n = d.numel()
    mean = np.float64(np_sum(d, bufsize)) / n
    x = d - float(mean)
    squares = np.float64(np_sum(x * x, bufsize))
    if ddof == 0:
        std = np.sqrt(squares / n)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            std = np.sqrt(squares / np.float64(n - ddof))
    lo, hi = torch.stack(torch.aminmax(d)).tolist()
    return mean, std, np.float64(lo), np.float64(hi)


# ------------------------------------------------------------------------------------------------------------ internals
def _pair_distances(pred, gt):
    """(gt2pre f64 [n_gt], pre2gt f64 [n_pre]) on the device; the input checks of cloud_metrics."""
    pred, gt = _inputs.on_device(((pred, "pred"), (gt, "gt")), min_rows=1, finite=True)
    return nearest(gt, pred)[0], nearest(pred, gt)[0]


def _direction(d, thresholds):
    """np.mean, np.std, max and the rates np.mean(d <= t) of one device distance vector."""
    mean, std, _, top = moments(d, 0)
    rates = tuple(np.float64(int((d <= float(t)).sum())) / d.numel() for t in thresholds)
    return mean, std, top, rates


def _figures(gt2pre, pre2gt, thresholds):
    thresholds = tuple(thresholds)
    gm, gs, gmax, recall = _direction(gt2pre, thresholds)
    pm, ps, pmax, precision = _direction(pre2gt, thresholds)
    fscore = tuple(np.float64(0.0) if r == 0 or p == 0 else 2 / (1 / r + 1 / p) for r, p in zip(recall, precision))
    return {"gt2pre_mean": gm, "gt2pre_std": gs, "gt2pre_max": gmax, "recall": recall,
            "pre2gt_mean": pm, "pre2gt_std": ps, "pre2gt_max": pmax, "precision": precision,
            "cd": 0.5 * (gm + pm), "fscore": fscore, "hausdorff": max(gmax, pmax),
            "n_gt": int(gt2pre.numel()), "n_pre": int(pre2gt.numel())}
