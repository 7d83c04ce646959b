#!/usr/bin/env python3
"""Whole-cloud run of generate.py's per-cloud body (seeds in process -> hot path -> outlier filter -> FPS to 4N), stage-timed.

A second line times the outlier filter's two forms on the same refined cloud (host: brute-force kNN + numpy means; device:
grid kNN + numpy-order means on the device, generation.outlier_filter_device) and the two kNN-30 kernels alone (grid vs
knn_outer brute force), best of five after a warm-up, and checks that the keep masks and the kNN tables are equal."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import sapcu_amd  # noqa: E402
from sapcu_amd import testing as T, generation as gen  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
    bs = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    dev = torch.device("cuda:0")
    fn, fd, _, _ = bench.build_models(dev)
    g = sapcu_amd.Generator3D6(fn, fd, dev, k_neighbors=48, dense_spacing=0.004, batch_size=bs)
    cloud = T.sphere_cloud(n, 0)
    t0 = time.perf_counter()
    seeds = gen.dense_seeds(cloud, 0.004)
    t1 = time.perf_counter()
    c_dev, s_dev = torch.as_tensor(cloud, device=dev), torch.as_tensor(seeds, device=dev)
    with torch.no_grad():
        g.refine(c_dev, s_dev[: 4 * bs])                  # warm-up (workspace, module handles)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        refined, _, _ = g.refine(c_dev, s_dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        keep = g.outlier_filter(refined)
        t4 = time.perf_counter()
    out = refined.cpu().numpy()[keep]
    t5 = time.perf_counter()
    from sapcu_amd import pipeline
    target = min(4 * n, out.shape[0])                      # generate.py: FPS to 4x the input size
    pipeline.farthest_point_sample(out[:1000], 8)         # (library warm-up)
    t6 = time.perf_counter()
    picked = pipeline.farthest_point_sample(out, target)
    t7 = time.perf_counter()
    print("cloud N=%d: %d seeds | seeds %.2f s | hot path %.2f s (%.0f query-points/s) | outlier filter %.2f s | copy-out %.2f s | "
          "FPS to %d: %.3f s | kept %d | radius mean %.4f std %.4f" % (
              n, seeds.shape[0], t1 - t0, t3 - t2, seeds.shape[0] / (t3 - t2), t4 - t3, t5 - t4, target, t7 - t6, out.shape[0],
              np.linalg.norm(out, axis=1).mean(), np.linalg.norm(out, axis=1).std()))
    assert np.unique(picked).shape[0] == target

    def best(f, reps=5):
        f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return min(ts), r

    with torch.no_grad():
        m = refined.shape[0]
        t_host, keep_h = best(lambda: g.outlier_filter(refined))
        t_dev, keep_d = best(lambda: gen.outlier_filter_device(refined, g.outlier_threshold).cpu().numpy())
        t_grid, (gi, gd) = best(lambda: gen.knn_self_grid(refined, 30))
        t_brute, (bi, bd, _) = best(lambda: gen.knn_gather(refined, refined, 30, want_dist=True, want_patch=False))
        info = []
        gen.knn_self_grid(refined, 30, info=info)
    assert np.array_equal(keep_h, keep_d) and torch.equal(gi, bi) and torch.equal(gd, bd)
    print("outlier filter on %d refined points: host %.1f ms | device %.1f ms (keep masks equal) | kNN-30 alone: grid %.2f ms "
          "(%d x %d x %d cells) vs knn_outer brute force %.2f ms (tables equal)" % (
              m, 1e3 * t_host, 1e3 * t_dev, 1e3 * t_grid, info[1], info[2], info[3], 1e3 * t_brute))

    st = []
    t_sh, s_host = best(lambda: gen.dense_seeds(cloud, 0.004))
    t_sd, s_dev2 = best(lambda: gen.dense_seeds_device(c_dev, 0.004, dev, stats=st))
    assert np.array_equal(s_host, s_dev2.cpu().numpy())
    print("seeds of the N=%d cloud (%d): host %.1f ms (%s threads) | device %.1f ms (arrays equal; %d levels, %d voxels, %d recomputed "
          "on the host)" % (n, s_host.shape[0], 1e3 * t_sh, os.environ.get("SAPCU_SEED_THREADS", "default"), 1e3 * t_sd, st[0], st[1], st[2]))


if __name__ == "__main__":
    main()
