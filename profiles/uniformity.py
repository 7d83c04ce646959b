#!/usr/bin/env python3
"""Uniformity on the reference's icosphere (5120 faces) with its 8192 points, at 48 and at 9000 seeds (calc_NUC.py pools D = 9000
disks per cloud): ``uniformity_metrics`` as a whole (point_to_mesh, the geodesic disks, the read-back and the numpy figures) and the
``sapcu_geodesic_disks_f64`` call alone, by device events around calls that end in a synchronise, 5 warm-ups, then the median, the
smallest and the largest of the runs.  The mesh and the points come from tests/golden/mesh_p2f.npz, the 48 seeds from
tests/golden/uniformity.npz (the counts are checked against the tool's), the 9000 from ``uniformity_seeds``.  Needs a GPU.
Usage: uniformity.py [report] [runs >= 20]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sapcu_amd  # noqa: E402
from sapcu_amd import uniformity  # noqa: E402


def timed(fn, runs, warm=5):
    for _ in range(warm):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return out, float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    report = sys.argv[1] if len(sys.argv) > 1 else None
    runs = max(20, int(sys.argv[2])) if len(sys.argv) > 2 else 20
    assert torch.cuda.is_available(), "uniformity.py measures on a GPU"
    gold = os.path.join(ROOT, "tests", "golden")
    p2f, fx = np.load(os.path.join(gold, "mesh_p2f.npz")), np.load(os.path.join(gold, "uniformity.npz"))
    dev = torch.device("cuda")
    v = torch.from_numpy(p2f["ico/vertices"]).to(dev)
    f = torch.from_numpy(p2f["ico/faces"]).to(dev)
    p = torch.from_numpy(p2f["ico/points"]).to(dev)
    rows = fx["ico/seeds"]
    tool = (rows[:, 0].astype(np.int64), np.ascontiguousarray(rows[:, [2, 3, 1]]))
    many = uniformity.uniformity_seeds(p2f["ico/vertices"], p2f["ico/faces"], 9000, generator=1)
    lines = ["uniformity on the icosphere: %d faces, %d points; device events around synchronised calls, 5 warm-ups, %d runs"
             % (f.shape[0], p.shape[0], runs)]
    for name, seeds in (("48 seeds (the fixture's)", tool), ("9000 seeds", many)):
        m, med, lo, hi = timed(lambda: uniformity.uniformity_metrics(p, v, f, seeds=seeds), runs)
        if len(seeds[0]) == 48:
            assert np.array_equal(m["counts"], fx["ico/counts"]), "the counts are not the tool's"
        info = []
        _, kmed, klo, khi = timed(lambda: uniformity.geodesic_disks(p, v, f, seeds[0], seeds[1], radii=m["radii"], info=info), runs)
        _, pmed, _, _ = timed(lambda: sapcu_amd.point_to_mesh(p, v, f), runs)
        lines.append("%-26s uniformity_metrics %8.3f ms (min %.3f, max %.3f)   geodesic_disks with its point_to_mesh %8.3f ms (min %.3f, "
                     "max %.3f)   point_to_mesh alone %.3f ms" % (name, med, lo, hi, kmed, klo, khi, pmed))
        lines.append("%-26s windows and vertex events %d (%.0f a seed), largest queue %d, seeds that left LDS %d, work groups %d, NUC %s"
                     % ("", info[0], info[0] / len(seeds[0]), info[1], info[2], info[7], np.array2string(m["nuc"], precision=4)))
    lines.append("the reference tool on the same 48 seeds, its own 'elapsed time' on the CPU with its 16 threads: %.2f s "
                 "(tests/golden/uniformity.npz, tool_seconds)" % float(fx["tool_seconds"][0]))
    text = "\n".join(lines)
    print(text)
    if report:
        with open(report, "w") as out:
            out.write(text + "\n")


if __name__ == "__main__":
    main()
