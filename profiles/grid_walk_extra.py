#!/usr/bin/env python3
"""What profiles/grid_walk_ab.txt times beside metrics_nn.py, mesh_dist.py and ray_cast.py, for the library SAPCU_LIB_PATH selects:

  * device seed generation (seeds_eval_kernel) on the cloud of bench.py's strong leg: sphere 5000, spacing 0.004, 385 582 seeds;
  * the self-kNN of those seeds on the cell grid (knn_self_grid_kernel) at k = 1, 30 and 64;
  * the brute-force routes of point_mesh and ray_mesh at 8192 queries on icospheres of 20 480 and 81 920 faces (mesh_brute_kernel,
    ray_brute_kernel: 32 workgroups, where a change of their prologue shows).

Device-event ms of whole calls after one warm-up, with a checksum of each result so that two libraries can be compared.  Needs a
GPU.  Usage: SAPCU_LIB_PATH=profiles/ab/libA.so python profiles/grid_walk_extra.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sapcu_amd  # noqa: E402,F401
from sapcu_amd import generation as gen, testing as T  # noqa: E402
import mesh_dist as MD  # noqa: E402
import ray_cast as RC  # noqa: E402


def times(fn, n):
    return " ".join("%.3f" % t for t in sorted(MD.timed(fn)[0] for _ in range(n)))


def main():
    assert torch.cuda.is_available(), "grid_walk_extra.py measures on a GPU"
    dev = torch.device("cuda:0")
    print("library %s" % os.environ.get("SAPCU_LIB_PATH", "csrc/libsapcu_hip.so"), flush=True)
    cloud = T.sphere_cloud(5000, 0)
    seeds = gen.dense_seeds_device(cloud, 0.004, dev)                       # warm-up: grows its buffers
    print("dense_seeds_device sphere 5000 spacing 0.004 (%d seeds, sum %r) ms: %s" %
          (seeds.shape[0], float(seeds.sum()), times(lambda: gen.dense_seeds_device(cloud, 0.004, dev), 5)), flush=True)
    for k in (1, 30, 64):
        info = []
        idx, dist = gen.knn_self_grid(seeds, k, info=info)
        print("knn_self_grid %d points k=%d grid %s (sums %d %r) ms: %s" %
              (seeds.shape[0], k, info[1:], int(idx.sum()), float(dist.sum()), times(lambda: gen.knn_self_grid(seeds, k), 7)), flush=True)
    pts = torch.as_tensor(T.sphere_cloud(8192, 1), device=dev)
    o = np.random.default_rng(3).normal(size=(8192, 3))
    o = 1.5 * o / np.linalg.norm(o, axis=1, keepdims=True)                 # rays from three radii away towards the centre
    for level in (5, 6):
        v, f = MD.icosphere(level, 0.5)
        c = MD.Call(v, f, pts, dev)
        c.run(brute=True)
        print("mesh brute %6d faces x 8192 points (sum %r) ms: %s" % (len(f), float(c.dist.sum()), times(lambda: c.run(brute=True), 7)), flush=True)
        r = RC.Call(v, f, (o, -o / 1.5, None), dev)
        r.run(brute=True)
        print("ray  brute %6d faces x 8192 rays (sum %r) ms: %s" % (len(f), float(r.t.sum()), times(lambda: r.run(brute=True), 7)), flush=True)


if __name__ == "__main__":
    main()
