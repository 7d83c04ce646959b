#!/usr/bin/env python3
"""pca_normals at n = 100 000, k = 16 on a noisy sphere shell: wall time per call with a synchronise, for a run under
``rocprofv3 --kernel-trace --stats`` that separates the kNN kernels (csrc/knn_grid.hip) from pca_normals_kernel (csrc/normals.hip).
Needs a GPU.  Usage: pca_normals.py [n] [k] [calls]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sapcu_amd  # noqa: E402


def main():
    n, k, calls = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 100000), (2, 16), (3, 5)))
    assert torch.cuda.is_available(), "pca_normals.py measures on a GPU"
    rng = np.random.default_rng(5)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    pts = torch.from_numpy(0.5 * v + rng.normal(size=(n, 3)) * 0.002).cuda()
    sapcu_amd.pca_normals(pts, k)                                  # warm-up: code objects, the allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        normals = sapcu_amd.pca_normals(pts, k)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    radial = torch.from_numpy(v).cuda()
    fig = sapcu_amd.normal_metrics(normals, radial)
    print("pca_normals n = %d k = %d: %.3f ms per call (median of %d, synchronised), mean angle to the radial normals %.4f degrees"
          % (n, k, 1e3 * float(np.median(times)), calls, fig["mean_deg"]))


if __name__ == "__main__":
    main()
