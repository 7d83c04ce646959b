#!/usr/bin/env python3
"""The rows of profiles/wave_ops_ab.txt for the library SAPCU_LIB_PATH selects: the calls whose kernels use csrc/wave_ops.h, at the
workloads of knn_microbench.py, grid_walk_extra.py, train_patches.py, surface_sample.py, poisson.py, uniformity.py, metrics_nn.py,
mesh_dist.py and ray_cast.py (their builders are imported), without those scripts' host comparisons and sweeps.  Every row is
`runs` device-event times in ms after a warm-up, one line `ROW <name> | t t t ...`; a row of short calls times windows of
back-to-back calls and prints ms per call.  Needs a GPU.  Usage: SAPCU_LIB_PATH=profiles/ab/libA.so wave_ops_rows.py [runs [knn_outer]]
(the word knn_outer: the three rows of the outer kNN alone, profiles/klist_tests_ab.txt)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sapcu_amd  # noqa: E402
from sapcu_amd import data, generation as gen, metrics, poisson, testing as T, uniformity  # noqa: E402
import mesh_dist as MD  # noqa: E402
import poisson as PP  # noqa: E402  (profiles/poisson.py: this directory comes first on the path)
import ray_cast as RC  # noqa: E402
import surface_sample as SS  # noqa: E402
import train_patches as TP  # noqa: E402


def row(name, fn, runs, calls=1):
    fn()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / calls)
    print("ROW %-58s | %s" % (name, " ".join("%.4f" % t for t in ts)), flush=True)


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    assert torch.cuda.is_available(), "wave_ops_rows.py measures on a GPU"
    dev = torch.device("cuda:0")
    print("library %s, %s, %d runs a row" % (os.environ.get("SAPCU_LIB_PATH", "csrc/libsapcu_hip.so"), torch.cuda.get_device_name(0), runs),
          flush=True)
    rng = np.random.default_rng(0)

    # knn_microbench.py: the outer kNN (k = 100: the two-slot list)
    cloud = torch.as_tensor(rng.standard_normal((5000, 3)), device=dev)
    many = torch.as_tensor(rng.standard_normal((65536, 3)), device=dev)
    for b, k, calls in ((4096, 48, 20), (65536, 48, 5), (4096, 100, 20)):
        q = cloud[:b].contiguous() if b <= 5000 else many
        row("knn_outer N=5000 B=%d k=%d" % (b, k), lambda: gen.knn_gather(cloud, q, k), runs, calls)
    if len(sys.argv) > 2 and sys.argv[2] == "knn_outer":
        return

    # grid_walk_extra.py: seed generation, the self-kNN on the grid; the outlier statistics of its k = 30 table
    sphere = T.sphere_cloud(5000, 0)
    seeds = gen.dense_seeds_device(sphere, 0.004, dev)
    row("dense_seeds_device sphere 5000 spacing 0.004", lambda: gen.dense_seeds_device(sphere, 0.004, dev), runs)
    for k in (1, 30, 64):
        row("knn_self_grid %d points k=%d" % (seeds.shape[0], k), lambda: gen.knn_self_grid(seeds, k), runs)
    dist30 = gen.knn_self_grid(seeds, 30)[1]
    row("outlier_stats_device %d x 30" % seeds.shape[0], lambda: gen.outlier_stats_device(dist30), runs)

    # train_patches.py: the fd and fn batches
    S = 64
    fd_in, fd_dense = TP.sphere(rng, S, 256) * np.float32(0.5), TP.sphere(rng, S, 1024) * np.float32(0.5)
    fn_nrm = TP.sphere(rng, S, 512)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                            # noqa: E731
    d_in, d_dense, d_pts, d_nrm = up(fd_in), up(fd_dense), up(fn_nrm * np.float32(0.5)), up(fn_nrm)
    for b in (4, 64):
        idx = torch.arange(b, device=dev) % S
        rot, scale, jitter = TP.draws(dev, b, 256, b)
        row("train_patches fd B=%d (256 / 1024 points, k=32)" % b, lambda: data.build_patches(
            d_in, idx, 32, dense=d_dense, rotation=rot, scale=scale, jitter=jitter, validate=False), runs, TP.CALLS)
    idx = torch.arange(4, device=dev)
    rot, scale, jitter = TP.draws(dev, 4, 512, 7)
    centres = torch.stack([torch.randperm(512, device=dev)[:64] for _ in range(4)]).to(torch.int32)
    row("train_patches fn B=4 (512 points, 64 centres, k=12)", lambda: data.build_patches(
        d_pts, idx, 12, normals=d_nrm, rotation=rot, scale=scale, jitter=jitter, centres=centres, validate=False), runs, TP.CALLS)
    rot, scale, jitter = TP.draws(dev, 4, 256, 9)
    row("train_patches fd B=4 k=128 (the two-slot list)", lambda: data.build_patches(
        d_in, idx, 128, rotation=rot, scale=scale, jitter=jitter, validate=False), runs, TP.CALLS)

    # surface_sample.py: the tables call (faces + area sum + cdf)
    g = np.load(os.path.join(ROOT, "tests", "golden", "surface_sample.npz"))
    big = SS.torus(224, 224)
    for name, mesh, n in (("fixture torus, 1 mesh", (g["torus/vertices"], g["torus/faces"]), 1), ("torus 100 352 faces, 1 mesh", big, 1),
                          ("torus 100 352 faces, 64 meshes", big, 64)):
        call = SS.TablesCall(mesh, n, dev)
        row("surface tables " + name, call.run, runs)
        del call

    # poisson.py: both paths
    for C, n in ((2048, 256), (8192, 1024)):
        for b in (4, 64):
            P = torch.from_numpy(PP.sphere(b, C, 7)).to(dev)
            row("poisson_subsample resident b=%d C=%d n=%d" % (b, C, n), lambda: poisson.poisson_subsample(P, n, 20, validate=False), runs)
    for C in (1 << 17, 1 << 20):
        P = torch.from_numpy(PP.sphere(1, C, 9)[0]).to(dev)
        radius = float(0.7 * np.sqrt(4 * np.pi / (C / 8)))
        row("poisson_select grid C=%d" % C, lambda: poisson.poisson_select(P, radius, validate=False), max(3, runs // 2))

    # uniformity.py: the geodesic disks call (with its point_to_mesh)
    gold = os.path.join(ROOT, "tests", "golden")
    p2f, fx = np.load(os.path.join(gold, "mesh_p2f.npz")), np.load(os.path.join(gold, "uniformity.npz"))
    v, f, p = (torch.from_numpy(p2f["ico/" + key]).to(dev) for key in ("vertices", "faces", "points"))
    rows = fx["ico/seeds"]
    tool = (rows[:, 0].astype(np.int64), np.ascontiguousarray(rows[:, [2, 3, 1]]))
    more = uniformity.uniformity_seeds(p2f["ico/vertices"], p2f["ico/faces"], 9000, generator=1)
    for name, sd in (("48 seeds", tool), ("9000 seeds", more)):
        radii = uniformity.uniformity_metrics(p, v, f, seeds=sd)["radii"]
        row("geodesic_disks " + name, lambda: uniformity.geodesic_disks(p, v, f, sd[0], sd[1], radii=radii), runs)

    # metrics_nn.py: the grid route of nearest
    gt = torch.as_tensor(T.sphere_cloud(8192, 1), device=dev, dtype=torch.float64)
    for name, c, q in (("seeds -> seeds", seeds, seeds), ("seeds -> gt", gt, seeds), ("gt -> seeds", seeds, gt)):
        row("nearest grid " + name, lambda: metrics.nearest(q, c), runs)

    # mesh_dist.py and ray_cast.py: the grid routes (the setup and classify kernels fold through wave_ops.h)
    radius = float(seeds.norm(dim=1).mean())
    for level in (4, 6):
        mv, mf = MD.icosphere(level, radius)
        for pts, pname in ((gt, "8192 points"), (seeds, "385 582 seeds")):
            c = MD.Call(mv, mf, pts, dev)
            row("point_mesh grid %d faces x %s" % (len(mf), pname), lambda: c.run(cell=c.auto_cell(MD.POP)), runs)
            del c
        rv, rf = MD.icosphere(level, 0.5)
        for n in (8192, 385582):
            c = RC.Call(rv, rf, RC.make_rays("sampler", rv, rf, n, 100 * level + (n & 1)), dev)
            row("ray_mesh grid %d faces x %d sampler rays" % (len(rf), n), lambda: c.run(cell=c.auto_cell(RC.POP)), runs)
            del c


if __name__ == "__main__":
    main()
