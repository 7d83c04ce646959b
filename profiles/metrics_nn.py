#!/usr/bin/env python3
"""Nearest neighbour of every query in another cloud: the grid search of csrc/metrics.hip against the brute force of
csrc/knn_outer.hip (``knn_gather`` at k = 1, the only way before it), on the 385 582 seeds of the whole-cloud workload (sphere
5000, spacing 0.004) against themselves and against an 8192-point ground-truth sphere in both directions.

After one warm-up of each path the two are ALTERNATED in one session, several runs each, every run timed by device events around
the whole call (grid build, query sort and search included) and ended by a synchronise.  Bit equality of distances and indices is
asserted at every size timed.  Then the sweep of the cell population parameter c (cell edge = longest extent * sqrt(2 c / n)), and,
for context only, sklearn's NearestNeighbors(n_neighbors=1) on the host for the same pairs, as the reference's evaluation_cd.py
runs it.  Needs a GPU; writes the report (default profiles/metrics_nn.txt).

Usage: metrics_nn.py [report path] [runs]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sapcu_amd  # noqa: E402,F401
from sapcu_amd import generation as gen, metrics, testing as T  # noqa: E402

POPS = (8, 16, 32, 64)
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def pair(name, cloud, q, runs, brute_runs):
    n, nq = cloud.shape[0], q.shape[0]
    grid = lambda: metrics.nearest(q, cloud)                                                    # noqa: E731
    brute = lambda: gen.knn_gather(cloud, q, 1, want_dist=True, want_patch=False)               # noqa: E731
    info = []
    d, i = metrics.nearest(q, cloud, 0.0, info)                                                 # warm-up of both paths
    bi, bd, _ = brute()
    assert torch.equal(d.view(torch.int64), bd[:, 0].contiguous().view(torch.int64)) and torch.equal(i, bi[:, 0]), name
    tg, tb = [], []
    for r in range(max(runs, brute_runs)):                                                      # alternated
        if r < runs:
            tg.append(timed(grid)[0])
        if r < brute_runs:
            tb.append(timed(brute)[0])
    say("%s: cloud n = %d, queries nq = %d, grid %d x %d x %d, bit-equal to brute force (distances and indices)" %
        (name, n, nq, info[1], info[2], info[3]))
    say("  grid  ms: %s   (min %.3f, max %.3f)" % (" ".join("%.3f" % t for t in tg), min(tg), max(tg)))
    say("  brute ms: %s   (min %.3f, max %.3f)" % (" ".join("%.3f" % t for t in tb), min(tb), max(tb)))
    say("  slowest grid run against fastest brute run: %.1f x faster; median against median: %.1f x; every grid run faster: %s" %
        (min(tb) / max(tg), float(np.median(tb)) / float(np.median(tg)), max(tg) < min(tb)))
    # the cell population sweep
    ext = float((cloud.max(0)[0] - cloud.min(0)[0]).max())
    row = []
    for c in POPS:
        cell = ext * (2.0 * c / n) ** 0.5
        info = []
        dd, ii = metrics.nearest(q, cloud, cell, info)
        assert torch.equal(dd.view(torch.int64), d.view(torch.int64)) and torch.equal(ii, i), (name, c)
        ts = [timed(lambda: metrics.nearest(q, cloud, cell))[0] for _ in range(runs)]
        row.append("c=%d (%dx%dx%d): min %.3f med %.3f" % (c, info[1], info[2], info[3], min(ts), float(np.median(ts))))
    say("  sweep ms: " + " | ".join(row))
    return min(tb) / max(tg), max(tg) < min(tb)


def host_sklearn(name, cloud, q):
    from sklearn.neighbors import NearestNeighbors
    c, x = cloud.cpu().numpy(), q.cpu().numpy()
    t0 = time.perf_counter()
    d, _ = NearestNeighbors(n_neighbors=1, algorithm="auto").fit(c).kneighbors(x)
    t1 = time.perf_counter()
    say("  %s: sklearn NearestNeighbors(n_neighbors=1) fit + kneighbors on the host: %.1f ms" % (name, (t1 - t0) * 1e3))
    return np.squeeze(d)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics_nn.txt")
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    assert torch.cuda.is_available(), "metrics_nn.py measures on a GPU"
    dev = torch.device("cuda:0")
    big = torch.as_tensor(gen.dense_seeds(T.sphere_cloud(5000, 0), 0.004), device=dev)
    gt = torch.as_tensor(T.sphere_cloud(8192, 1), device=dev, dtype=torch.float64)
    say("# nearest neighbour in another cloud: grid (csrc/metrics.hip) against brute force (knn_gather, k = 1)")
    say("# %s, torch %s; times are device-event ms of the whole call, paths alternated, %d runs each (brute 385k x 385k: 3)" %
        (torch.cuda.get_device_name(0), torch.__version__, runs))
    results = [pair("seeds -> seeds", big, big, runs, 3),
               pair("seeds -> gt (queries 385 582, cloud 8192)", gt, big, runs, runs),
               pair("gt -> seeds (queries 8192, cloud 385 582)", big, gt, runs, runs)]
    say("whole metric: cloud_metrics(seeds, gt) = both directions + statistics")
    metrics.cloud_metrics(big, gt)
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = metrics.cloud_metrics(big, gt)
        ts.append((time.perf_counter() - t0) * 1e3)
    say("  host wall ms (ends with the figures on the host): %s" % " ".join("%.2f" % t for t in ts))
    say("  cd %r hausdorff %r fscore %r" % (float(m["cd"]), float(m["hausdorff"]), tuple(float(f) for f in m["fscore"])))
    say("host, for context only (what evaluation_cd.py runs per pair, in one process):")
    g2p = host_sklearn("gt -> seeds", big, gt)
    p2g = host_sklearn("seeds -> gt", gt, big)
    assert np.array_equal(g2p, metrics.nearest(gt, big)[0].cpu().numpy()) and np.array_equal(p2g, metrics.nearest(big, gt)[0].cpu().numpy())
    say("  sklearn's distances equal the device's bit for bit at this size")
    say("bar (every grid run faster than every brute-force run at 385 582 x 385 582): %s, %.1f x" %
        ("met" if results[0][1] else "MISSED", results[0][0]))
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    assert results[0][1]


if __name__ == "__main__":
    main()
