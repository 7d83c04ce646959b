#!/usr/bin/env python3
"""Distance from every point to a triangle mesh (csrc/mesh_dist.hip): the grid route against the brute-force route, the sweeps of
the cell population and of the oversize cap, and the sizes the automatic threshold was set from.

Meshes: icospheres subdivided in this script (20 * 4^level faces: 320, 1280, 5120, 20 480, 81 920), scaled to the radius of the
point sets.  Points: an 8192-point sphere cloud and the 385 582 refined seeds of the whole-cloud workload (sphere 5000, spacing
0.004).  After one warm-up of each path the two are ALTERNATED in one session, several runs each, every run timed by device events
around the whole call (bounding boxes, centroids, sorts, the read-back and the search included) on buffers allocated once.  Bit
equality of distance, face and closest point is asserted at every size timed.  Needs a GPU; writes the report (default
profiles/mesh_dist.txt).

Usage: mesh_dist.py [report path] [runs]
       mesh_dist.py --one grid|brute     (one route, 81 920 faces x 385 582 points, three calls: for a profiler)"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sapcu_amd  # noqa: E402,F401
from sapcu_amd import _lib, generation as gen, mesh, testing as T  # noqa: E402

POPS = (2, 4, 8, 16, 32, 64)
CAPS = (0.5, 1.0, 2.0, 4.0)
POP, CAP = 4, 2.0                 # MESH_CELL_POP and MESH_OVERSIZE_MULT of csrc/mesh_dist.hip: the settings the routes are compared at
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def icosphere(level, radius):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius, np.array(f, dtype=np.int32)


def torus(nu, nw, R, r):
    u, w = np.arange(nu) * (2 * np.pi / nu), np.arange(nw) * (2 * np.pi / nw)
    gu, gw = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(gw)) * np.cos(gu), (R + r * np.cos(gw)) * np.sin(gu), r * np.sin(gw)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nw), indexing="ij")
    idx = lambda a, b: (a % nu) * nw + (b % nw)                                                 # noqa: E731
    f = np.concatenate([np.stack([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], -1).reshape(-1, 3),
                        np.stack([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)], -1).reshape(-1, 3)])
    return v, f.astype(np.int32)


class Call:
    """One (mesh, points) pair on buffers allocated once; run(...) is one whole call of the tuned entry point."""

    def __init__(self, v, f, p, dev):
        self.lib = _lib.load()
        self.v = torch.as_tensor(v, device=dev)
        self.f = torch.as_tensor(f, device=dev)
        self.p = p
        self.nv, self.nf, self.nq = len(v), len(f), p.shape[0]
        self.dist = torch.zeros((self.nq,), dtype=torch.float64, device=dev)
        self.face = torch.zeros((self.nq,), dtype=torch.int64, device=dev)
        self.clo = torch.zeros((self.nq, 3), dtype=torch.float64, device=dev)
        self.nbytes = int(self.lib.sapcu_point_mesh_workspace_bytes(self.nv, self.nf, self.nq))
        self.ws = torch.zeros((self.nbytes,), dtype=torch.uint8, device=dev)
        self.info = (ctypes.c_int64 * 6)()
        self.ext = float((self.v.max(0)[0] - self.v.min(0)[0]).max())

    def run(self, cell=0.0, brute=False, mult=CAP, pop=POP):
        _lib.check(self.lib.sapcu_internal_point_mesh_tuned(_lib.ptr(self.v), self.nv, _lib.ptr(self.f), self.nf, _lib.ptr(self.p), self.nq,
                                                            float(cell), float(mult), int(pop), int(brute), _lib.ptr(self.dist),
                                                            _lib.ptr(self.face), _lib.ptr(self.clo), _lib.ptr(self.ws), self.nbytes, self.info,
                                                            _lib.current_stream()))
        return list(self.info)

    def bits(self):
        return self.dist.clone().view(torch.int64), self.face.clone(), self.clo.clone().view(torch.int64)

    def auto_cell(self, pop):
        return self.ext * (2.0 * pop / self.nf) ** 0.5         # what cell_size 0 computes from the centroids' extent (about the vertices')


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def pair(name, c, runs, brute_runs, sweeps=True):
    grid = lambda: c.run(cell=c.auto_cell(POP))                                                  # noqa: E731
    brute = lambda: c.run(brute=True)                                                           # noqa: E731
    info = grid()                                                                               # warm-up of both paths
    g = c.bits()
    brute()
    assert same(g, c.bits()), (name, info)
    tg, tb = [], []
    for r in range(max(runs, brute_runs)):                                                      # alternated
        if r < runs:
            tg.append(timed(grid)[0])
        if r < brute_runs:
            tb.append(timed(brute)[0])
    say("%s: %d faces, %d points, grid %d x %d x %d, %d oversize%s, bit-equal to brute force (distance, face, closest point)" %
        (name, c.nf, c.nq, info[1], info[2], info[3], info[4], "" if info[0] else " (FELL BACK to brute force)"))
    say("  grid  ms: %s   (min %.3f, med %.3f, max %.3f)" % (" ".join("%.3f" % t for t in tg), min(tg), float(np.median(tg)), max(tg)))
    say("  brute ms: %s   (min %.3f, med %.3f, max %.3f)" % (" ".join("%.3f" % t for t in tb), min(tb), float(np.median(tb)), max(tb)))
    say("  median against median: grid %.2f x faster; every grid run faster than every brute run: %s" %
        (float(np.median(tb)) / float(np.median(tg)), max(tg) < min(tb)))
    if not sweeps:
        return
    row = []
    for pop in POPS:
        info = c.run(cell=c.auto_cell(pop))
        assert same(g, c.bits()), (name, pop)
        ts = [timed(lambda: c.run(cell=c.auto_cell(pop)))[0] for _ in range(runs)]
        row.append("c=%d (%dx%dx%d, %d oversize%s): min %.3f med %.3f" % (pop, info[1], info[2], info[3], info[4],
                                                                          "" if info[0] else ", FELL BACK", min(ts), float(np.median(ts))))
    say("  population sweep ms: " + " | ".join(row))
    row = []
    for mult in CAPS:
        info = c.run(cell=c.auto_cell(POP), mult=mult)
        assert same(g, c.bits()), (name, mult)
        ts = [timed(lambda: c.run(cell=c.auto_cell(POP), mult=mult))[0] for _ in range(runs)]
        row.append("cap=%.1f h (%d oversize%s): min %.3f med %.3f" % (mult, info[4], "" if info[0] else ", FELL BACK", min(ts),
                                                                      float(np.median(ts))))
    say("  oversize cap sweep ms (c=%d): " % POP + " | ".join(row))


def one(route):
    dev = torch.device("cuda:0")
    seeds = torch.as_tensor(gen.dense_seeds(T.sphere_cloud(5000, 0), 0.004), device=dev)
    v, f = icosphere(6, float(seeds.norm(dim=1).mean()))
    c = Call(v, f, seeds, dev)
    for _ in range(3):
        print(route, c.run(brute=(route == "brute")), flush=True)
    torch.cuda.synchronize()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        return one(sys.argv[2])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesh_dist.txt")
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    assert torch.cuda.is_available(), "mesh_dist.py measures on a GPU"
    dev = torch.device("cuda:0")
    seeds = torch.as_tensor(gen.dense_seeds(T.sphere_cloud(5000, 0), 0.004), device=dev)
    small = torch.as_tensor(T.sphere_cloud(8192, 1), device=dev, dtype=torch.float64)
    radius = float(seeds.norm(dim=1).mean())
    say("# point-to-mesh distance: grid route against brute-force route (csrc/mesh_dist.hip)")
    say("# %s, torch %s; times are device-event ms of the whole call, paths alternated, %d runs each (brute on 385 582 points: 3)" %
        (torch.cuda.get_device_name(0), torch.__version__, runs))
    say("# icospheres of radius %.4f (the seeds' mean radius); points: %d seeds, %d-point sphere cloud" % (radius, seeds.shape[0], small.shape[0]))
    meshes = {level: icosphere(level, radius) for level in (2, 3, 4, 5, 6)}
    for level in (4, 6):
        for pts, pname, br in ((small, "8192 points", runs), (seeds, "385 582 seeds", 3)):
            v, f = meshes[level]
            pair("%d faces x %s" % (len(f), pname), Call(v, f, pts, dev), runs, br)
    say("meshes with faces of very different sizes (an oversize list) and with long thin faces:")
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "mesh_p2f.npz"))
    pair("the fixture: the reference's Icosahedron.off x Icosahedron.xyz", Call(g["ico/vertices"], g["ico/faces"],
                                                                               torch.as_tensor(g["ico/points"], device=dev), dev), runs, runs)
    tv, tf = torus(100, 100, radius * 0.7, radius * 0.25)
    pair("torus 100 x 100 (faces four times as long as wide) x 8192 points", Call(tv, tf, small, dev), runs, runs)
    pair("torus 100 x 100 x 385 582 seeds", Call(tv, tf, seeds, dev), runs, 3)
    say("the automatic threshold (grid forced with the automatic cell edge below it):")
    for level in (2, 3, 5):
        for pts, pname, br in ((small, "8192 points", runs), (seeds, "385 582 seeds", 3)):
            v, f = meshes[level]
            pair("%d faces x %s" % (len(f), pname), Call(v, f, pts, dev), runs, br, sweeps=False)
    say("whole metric: mesh_metrics(seeds, 81 920-face icosphere)")
    v, f = meshes[6]
    tv, tf = torch.as_tensor(v, device=dev), torch.as_tensor(f, device=dev)
    m = mesh.mesh_metrics(seeds, tv, tf)
    ts = [timed(lambda: mesh.mesh_metrics(seeds, tv, tf))[0] for _ in range(runs)]
    say("  device-event ms (ends with the figures on the host): %s" % " ".join("%.2f" % t for t in ts))
    say("  p2f mean %r std %r min %r max %r" % (float(m["p2f_mean"]), float(m["p2f_std"]), float(m["p2f_min"]), float(m["p2f_max"])))
    with open(out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
