"""Cloud metrics without a GPU: the binding's sixth table against include/sapcu_metrics.h, the fixture of the reference's evaluation
script (tests/golden/cloud_metrics.npz) against a numpy restatement of the statistics in the order sapcu_amd/metrics.py fixes,
the argument errors that need no device, and the refusals of the C entry point that come before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_tables
from conftest import ROOT, golden

THRESHOLDS = (1e-2, 2e-2)


def header_entry_points():
    """{name: argument list} of include/sapcu_metrics.h."""
    return abi_tables.header_entry_points("sapcu_metrics.h")


def test_the_header_declares_exactly_the_sixth_table():
    from sapcu_amd import _lib
    decl = header_entry_points()
    assert set(decl) == set(_lib.METRICS_EXPORTS) == {"sapcu_nn_cross_workspace_bytes", "sapcu_nn_cross_grid_f64"}
    for other in (_lib.EXPORTS, _lib.SEEDS_EXPORTS, _lib.FD_TRAIN_EXPORTS, _lib.FD_EDGECONV_EXPORTS, _lib.TRAIN_STEP_EXPORTS):
        assert not set(other) & set(_lib.METRICS_EXPORTS)
    lib = _lib.load()
    for name in _lib.METRICS_EXPORTS:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len([a for a in decl[name].split(",") if a.strip()]), name
    with open(os.path.join(ROOT, "include", "sapcu.h")) as f:
        assert "sapcu_nn_cross" not in f.read() and _lib.ABI_VERSION == 2


def test_the_sizer_and_the_refusals_before_any_launch():
    """Everything include/sapcu_metrics.h promises to refuse is refused with SAPCU_ERR_ARG (-1) on a machine without a GPU too:
    the checks come before the first HIP call, and no pointer is dereferenced."""
    from sapcu_amd import _lib
    lib = _lib.load()
    size = lib.sapcu_nn_cross_workspace_bytes
    assert size(0, 5) == -1 and size(5, -1) == -1 and size((1 << 29) + 1, 5) == -1 and size(5, (1 << 31) - 63) == -1
    assert size(1, 0) > 0 and size(5000, 4097) > size(5000, 100) > 0 and size(5000, 100) % 8 == 0
    n, nq = 5000, 100
    need = size(n, nq)
    P = ctypes.c_void_p
    cloud, qs, dist, idx, ws = P(0x10000), P(0x20000), P(0x30000), P(0x40000), P(0x50000)       # never dereferenced
    info = (ctypes.c_int64 * 4)(7, 7, 7, 7)

    def call(cloud=cloud, n=n, qs=qs, nq=nq, cell=0.0, dist=dist, idx=idx, ws=ws, nbytes=need):
        return lib.sapcu_nn_cross_grid_f64(cloud, n, qs, nq, cell, dist, idx, ws, nbytes, info, None)

    for kw in (dict(cloud=None), dict(qs=None), dict(dist=None), dict(n=0), dict(nq=-1), dict(n=(1 << 29) + 1),
               dict(nq=(1 << 31) - 63), dict(nbytes=need - 1), dict(ws=None), dict(ws=P(0x50004)), dict(cell=-1.0),
               dict(cell=float("nan")), dict(cell=float("inf"))):
        assert call(**kw) == -1, kw
        assert lib.sapcu_last_error()
    assert list(info) == [7, 7, 7, 7]
    assert call(nq=0, qs=None, dist=None, idx=None) == 0 and list(info) == [0, 0, 0, 0]           # no query: nothing is launched


# ------------------------------------------------------------------------------------------------ numpy restatement
def np_leaf(a):
    """numpy's pairwise leaf (n <= 128): eight accumulators, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the rest in order."""
    n = len(a)
    if n < 8:
        res = np.float64(0.0)
        for v in a:
            res = res + v
        return res
    r = a[:8].copy()
    i = 8
    while i < n - n % 8:
        r = r + a[i:i + 8]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[i:]:
        res = res + v
    return res


def np_pairwise(a):
    if len(a) <= 128:
        return np_leaf(a)
    n2 = len(a) // 2
    n2 -= n2 % 8
    return np_pairwise(a[:n2]) + np_pairwise(a[n2:])


def chunked_sum(a, bufsize):
    """The order csrc/knn_grid.hip and generation.outlier_global_mean fix: pairwise sums of bufsize-element chunks, added in sequence."""
    total = 0.0
    for c0 in range(0, len(a), bufsize):
        total += float(np_pairwise(a[c0:c0 + bufsize]))
    return total


def restated_values(gt2pre, pre2gt, bufsize):
    """The eleven values of the fixture in the operation order of sapcu_amd/metrics.py, on host f64."""
    out = []
    rates = []
    for d in (gt2pre, pre2gt):
        n = len(d)
        mean = np.float64(chunked_sum(d, bufsize)) / n
        x = d - mean
        std = np.sqrt(np.float64(chunked_sum(x * x, bufsize)) / n)
        r = [np.float64(int((d <= t).sum())) / n for t in THRESHOLDS]
        rates.append(r)
        out += [mean, std] + r
    out.append(0.5 * (out[0] + out[4]))
    out += [2 / (1 / r + 1 / p) for r, p in zip(*rates)]
    return np.array(out, dtype=np.float64)


def plain_nearest(cloud, queries):
    """sqrt(((dx*dx + dy*dy) + dz*dz).min()) in f64: what sklearn returns bit for bit (tests/golden/make_metrics_fixtures.py)."""
    out = np.empty(len(queries))
    for i, q in enumerate(queries):
        d = q - cloud
        out[i] = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).min())
    return out


_DIST = {}


def pair_distances(g, name):
    if name not in _DIST:
        pred, gt = g[name + "/pred"], g[name + "/gt"]
        _DIST[name] = (plain_nearest(pred, gt), plain_nearest(gt, pred))
    return _DIST[name]


def test_a_numpy_restatement_reproduces_every_value_the_reference_script_printed():
    g = golden("cloud_metrics.npz")
    bufsize = np.getbufsize()
    assert list(g["pairs"]) == ["a", "b", "c"] and sorted(g["pooled/order"]) == ["a", "b", "c"]
    assert g["a/gt"].shape[0] >= 4096 and g["a/pred"].shape[0] >= 4096 and g["b/gt"].shape[0] >= 4096     # the grid route
    assert g["c/pred"].shape == (300, 3) and g["c/gt"].shape == (200, 3)                                     # the brute-force route
    for name in g["pairs"]:
        g2p, p2g = pair_distances(g, name)
        assert np.array_equal(restated_values(g2p, p2g, bufsize), g[name + "/values"]), name
        # and numpy's own functions say the same: the restated order IS np.mean / np.std
        assert np.mean(g2p) == g[name + "/values"][0] and np.std(p2g) == g[name + "/values"][5]
    assert np.array_equal(pair_distances(g, "b")[0], g["b/gt2pre"]) and np.array_equal(pair_distances(g, "b")[1], g["b/pre2gt"])
    order = list(g["pooled/order"])
    pooled = restated_values(np.hstack([pair_distances(g, n)[0] for n in order]), np.hstack([pair_distances(g, n)[1] for n in order]),
                             bufsize)
    assert np.array_equal(pooled, g["pooled/values"])
    v = g["b/values"]
    assert 0 < v[2] < v[3] < 1 and 0 < v[6] < v[7] < 1 and np.isfinite(g["pooled/values"]).all()


# ------------------------------------------------------------------------------------------------ argument errors
def test_cloud_metrics_argument_errors_that_need_no_device():
    from sapcu_amd import metrics
    import sapcu_amd
    assert sapcu_amd.cloud_metrics is metrics.cloud_metrics and callable(sapcu_amd.dataset_metrics) and callable(sapcu_amd.evaluate_file)
    ok = np.zeros((5, 3))
    for bad in (np.zeros((5, 2)), np.zeros((5,)), np.zeros((2, 5, 3)), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            metrics.cloud_metrics(bad, ok)
        with pytest.raises(ValueError):
            metrics.cloud_metrics(ok, bad)
    for v in (np.nan, np.inf, -np.inf):
        bad = np.zeros((5, 3))
        bad[3, 1] = v
        with pytest.raises(ValueError):
            metrics.cloud_metrics(bad, ok)
        with pytest.raises(ValueError):
            metrics.cloud_metrics(ok, bad.astype(np.float32))
    with pytest.raises(RuntimeError):
        metrics.cloud_metrics(torch.zeros(5, 3), ok)
    with pytest.raises(RuntimeError):
        metrics.cloud_metrics(ok, torch.zeros(5, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        metrics.nearest(torch.zeros(5, 3), torch.zeros(5, 3))
    with pytest.raises(ValueError):
        metrics.dataset_metrics([])
    with pytest.raises(ValueError):
        metrics.cloud_metrics(np.zeros((5, 3), dtype=np.int64), ok)
