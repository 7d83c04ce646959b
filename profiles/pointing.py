#!/usr/bin/env python3
"""fn's pointing samples on the device (csrc/pointing.hip) at the size of the reference's scripts/sample_mesh-fn.py:
an 800 000-point surface cloud of one mesh (a sphere of 2048 faces, radius 0.35), the 50^3 lattice of step 0.05, 10^3 fine cells
per voxel, k = 10, band 0.003 .. 0.03.

  near_voxels, pointing_samples   host clock round a call that ends in a device synchronise, best and median of `runs` after a
                                  warm-up; the candidate and kept counts; pointing_samples with and without the per-candidate
                                  outputs (without them a hopeless candidate leaves its walk early), and over forced cell sizes
  the same two KDTree.query calls on this host's CPU, ONCE: what the feature replaces (no threshold); the first distances and
                                  the neighbour tables of the two are compared on the way
Needs a GPU.  Usage: pointing.py [runs] [--no-host]   (the output is profiles/pointing.txt)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sapcu_amd  # noqa: E402, F401
from sapcu_amd import pointing, surface  # noqa: E402
import pointing_cases  # noqa: E402

SURFACE, SUB, K, BAND = 800000, 10, 10, (0.003, 0.03)


def timed(fn, runs):
    """(best, median) seconds of fn() on the host clock, each run synchronised, after one warm-up."""
    fn()
    torch.cuda.synchronize()
    s = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t)
    return min(s), float(np.median(s))


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
    dev = torch.device("cuda:0")
    print("device: %s; %d runs after a warm-up, best (median) by the host clock round synchronised calls" % (torch.cuda.get_device_name(0), runs), flush=True)
    tables = surface.build_surface_tables([pointing_cases.octasphere(4)], device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    b = -(-SURFACE // pointing.SURFACE_CHUNK)
    u = torch.rand((b, 4096), generator=gen, device=dev, dtype=torch.float64)
    r1, r2 = (torch.rand((b, 4096), generator=gen, device=dev, dtype=torch.float64).float() for _ in range(2))
    cloud = surface.sample_surface(tables, torch.zeros((b,), dtype=torch.int64, device=dev), 4096, u, r1, r2)[0].reshape(-1, 3)[:SURFACE].contiguous()
    voxels = pointing.near_voxels(cloud)
    jitter = torch.rand((voxels.shape[0] * SUB ** 3, 3), generator=gen, device=dev, dtype=torch.float64) * 0.001
    m = voxels.shape[0] * SUB ** 3
    print("surface cloud %d points, lattice 50^3 step 0.05: %d voxels near, %d candidates" % (SURFACE, voxels.shape[0], m), flush=True)
    best, med = timed(lambda: pointing.near_voxels(cloud), runs)
    print("  near_voxels (125000 centres, metrics.nearest):        %8.2f (%8.2f) ms" % (best * 1e3, med * 1e3), flush=True)
    info = []
    out = pointing.pointing_samples(cloud, voxels, jitter, info=info)
    kept = out["points"].shape[0]
    print("  kept %d of %d candidates (%.1f %%); grid %s" % (kept, m, 100.0 * kept / m, info), flush=True)
    best, med = timed(lambda: pointing.pointing_samples(cloud, voxels, jitter), runs)
    print("  pointing_samples, compacted outputs only:              %8.2f (%8.2f) ms, %.1f M candidates / s" % (best * 1e3, med * 1e3, m / best / 1e6),
          flush=True)
    best, med = timed(lambda: pointing.pointing_samples(cloud, voxels, jitter, return_all=True), runs)
    print("  pointing_samples, with keep, d1 and idx of every one:  %8.2f (%8.2f) ms" % (best * 1e3, med * 1e3), flush=True)
    for per in (256, 4096):
        best, med = timed(lambda: pointing.pointing_samples(cloud, voxels, jitter, voxels_per_call=per), runs)
        print("  compacted outputs only, %4d voxels per call:           %8.2f (%8.2f) ms" % (per, best * 1e3, med * 1e3), flush=True)
    print("  forced cell sizes (automatic: the edge that puts about 32 points of a surface into an occupied cell), compacted / all outputs:")
    for cell in (0.006, 0.008, 0.011, 0.015, 0.02, 0.03):
        gi = []
        pointing.pointing_samples(cloud, voxels, jitter, cell_size=cell, info=gi)
        a, _ = timed(lambda: pointing.pointing_samples(cloud, voxels, jitter, cell_size=cell), 2)
        c, _ = timed(lambda: pointing.pointing_samples(cloud, voxels, jitter, cell_size=cell, return_all=True), 2)
        print("    cell %.4f (grid %d x %d x %d): %8.2f / %8.2f ms" % (cell, gi[1], gi[2], gi[3], a * 1e3, c * 1e3), flush=True)
    if "--no-host" in sys.argv:
        return
    from sklearn.neighbors import KDTree
    import pointing_ref as R
    P = cloud.cpu().numpy()
    t = time.perf_counter()
    tree = KDTree(P)
    build = time.perf_counter() - t
    t = time.perf_counter()
    d0, _ = tree.query(R.centres(-1.0, 0.05, 50), 1)
    first = time.perf_counter() - t
    host_voxels = np.flatnonzero(d0[:, 0] < 0.05 + 0.01)
    print("host, once: KDTree build %.2f s; query of the 125000 centres %.2f s; its voxels equal the device's: %s"
          % (build, first, np.array_equal(host_voxels, voxels.cpu().numpy())), flush=True)
    q = R.candidates(host_voxels, -1.0, 0.05, 50, SUB, jitter.cpu().numpy())
    t = time.perf_counter()
    dist, idx = tree.query(q, K)
    second = time.perf_counter() - t
    print("host, once: KDTree.query(%d candidates, %d) %.2f s" % (len(q), K, second), flush=True)
    every = pointing.pointing_samples(cloud, voxels, jitter, return_all=True)
    same_d = np.array_equal(dist[:, 0], every["d1"].cpu().numpy())
    differ = int((idx != every["idx"].cpu().numpy()).any(1).sum())
    print("  first distances equal the device's bit for bit: %s; rows whose neighbour table differs (ties in sklearn's traversal order): %d"
          % (same_d, differ), flush=True)


if __name__ == "__main__":
    main()
