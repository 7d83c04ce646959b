#!/usr/bin/env python3
"""Poisson-disk subsampling on the device (csrc/poisson.hip): device events around synchronised calls after a warm-up.

  resident path   poisson_subsample, b = 4 and 64, (C, n) = (2048, 256) and (8192, 1024), 20 steps; rounds per selection and
                  per bisection (the kernel's own count)
  grid path       poisson_select at C = 2^17 and 2^20, a fixed radius
  loader          one whole data.PoissonPU1KPatches batch (host clock, synchronised)
beside two comparisons without a threshold: tests/poisson_ref.py's subsample on this host's CPU for the same input, and
farthest_point_sample from the same C to the same n on the device (one cloud per call, the project's present way to thin a cloud).
Needs a GPU.  Usage: poisson.py [runs]   (the output is profiles/poisson.txt)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sapcu_amd  # noqa: E402
from sapcu_amd import pipeline, poisson  # noqa: E402
import poisson_ref  # noqa: E402


def sphere(b, C, seed):
    g = np.random.default_rng(seed).standard_normal((b, C, 3))
    return (g / np.linalg.norm(g, axis=-1, keepdims=True)).astype(np.float32)


def timed(fn, runs, warm=3):
    """(median, min, max) ms of fn() by device events, each run synchronised."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def icosphere(level):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, g = {}, []
        for a, b, c in f:
            m = []
            for p, q in ((a, b), (b, c), (c, a)):
                key = (min(p, q), max(p, q))
                if key not in mid:
                    w = v[p] + v[q]
                    v.append(w / np.linalg.norm(w))
                    mid[key] = len(v) - 1
                m.append(mid[key])
            g += [(a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2])]
        f = g
    return (0.5 * np.array(v)).astype(np.float32), np.array(f, np.int32)


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    assert torch.cuda.is_available(), "poisson.py measures on a GPU"
    dev = torch.device("cuda:0")
    print("device: %s; %d runs after 3 warm-ups, median (min - max) ms by device events" % (torch.cuda.get_device_name(0), runs))
    print("\nresident path: poisson_subsample, 20 steps, points on a unit sphere")
    for C, n in ((2048, 256), (8192, 1024)):
        for b in (4, 64):
            P = torch.from_numpy(sphere(b, C, 7)).to(dev)
            med, lo, hi = timed(lambda: poisson.poisson_subsample(P, n, 20, validate=False), runs)
            idx, radius, count, rounds = poisson.poisson_subsample(P, n, 20)
            r = rounds.float()
            print("  b = %2d C = %4d n = %4d: %8.3f (%.3f - %.3f) ms; rounds per bisection %.0f (%d - %d), per selection %.1f; count - n at most %d; "
                  "r / sqrt(area / n) = %.3f" % (b, C, n, med, lo, hi, float(r.mean()), int(rounds.min()), int(rounds.max()), float(r.mean()) / 21,
                                                 int((count - n).max()), float(radius.mean()) / np.sqrt(4 * np.pi / n)))
        one = P[0].contiguous()
        med, lo, hi = timed(lambda: pipeline.farthest_point_sample_device(one, n), runs)
        print("  farthest_point_sample_device, ONE cloud C = %d -> %d: %8.3f (%.3f - %.3f) ms" % (C, n, med, lo, hi))
        t0 = time.perf_counter()
        ref = poisson_ref.subsample(P[0].cpu().numpy(), n, 20)
        cpu = time.perf_counter() - t0
        same = np.array_equal(ref[0], idx[0].cpu().numpy()) and ref[1].tobytes() == radius[0].cpu().numpy().tobytes()
        print("  tests/poisson_ref.py subsample on this host's CPU, ONE cloud C = %d -> %d: %.0f ms; the device's entry 0 equals it: %s"
              % (C, n, 1e3 * cpu, same))

    print("\ngrid path: poisson_select at a fixed radius, one entry, points on a unit sphere")
    for C in (1 << 17, 1 << 20):
        P = torch.from_numpy(sphere(1, C, 9)[0]).to(dev)
        radius = float(0.7 * np.sqrt(4 * np.pi / (C / 8)))
        med, lo, hi = timed(lambda: poisson.poisson_select(P, radius, validate=False), max(3, runs // 2), warm=1)
        keep, count, rounds = poisson.poisson_select(P, radius)
        print("  C = %7d r = %.5f: %8.2f (%.2f - %.2f) ms; kept %d, %d rounds" % (C, radius, med, lo, hi, int(count), int(rounds)))
        if C == 1 << 17:
            med, lo, hi = timed(lambda: pipeline.farthest_point_sample_device(P, int(count)), 3, warm=1)
            print("  farthest_point_sample_device C = %d -> %d: %8.2f (%.2f - %.2f) ms" % (C, int(count), med, lo, hi))

    print("\nloader: one data.PoissonPU1KPatches batch (defaults: 256 / 1024 points, oversample 8, k 32), host clock, synchronised")
    meshes = [icosphere(4)] * 64
    for bs in (4, 32):
        loader = sapcu_amd.PoissonPU1KPatches(meshes, split="all", batch_size=bs, seed=1, device=dev)
        it = iter(loader)
        next(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch = next(it)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        d = loader.last_draws
        print("  batch of %2d: %.2f ms; count - n at most %d (input), %d (dense)" % (bs, ms, int((d["count_input"] - 256).max()),
                                                                                    int((d["count_dense"] - 1024).max())))
        assert batch["input"].shape == (bs, 256, 32, 3)


if __name__ == "__main__":
    main()
