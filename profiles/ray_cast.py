#!/usr/bin/env python3
"""Ray casting against a triangle mesh (csrc/ray_cast.hip): the grid route against the brute-force route, the sweeps of the cell
population and of the piece length, and the sizes the automatic threshold is set from.

Meshes: icospheres subdivided in this script (20 * 4^level faces: 320, 1280, 5120, 20 480, 81 920) of radius 0.5.  Rays: 8192 and
385 582 of them, of two kinds: the sampler's (a surface point thrown out by 0.003 .. 0.03 along a random unit direction and cast
back, t_max = len * (1 + 2^-20)) and unbounded ones from three extents away towards the mesh's box.  After one warm-up of each path
the two are ALTERNATED in one session, several runs each, every run timed by device events around the whole call (bounding boxes,
centroids, clipping, sorts, the read-back and the search included) on buffers allocated once.  Bit equality of t, face and hit point
is asserted at every size timed.  Needs a GPU; writes the report (default profiles/ray_cast.txt) line by line.

The grid is forced for the comparison (the automatic choice would take brute force for the unbounded rays); what the automatic
choice takes and costs is timed as well.

Usage: ray_cast.py [report path] [runs]"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sapcu_amd  # noqa: E402,F401
from sapcu_amd import _lib  # noqa: E402
from mesh_dist import icosphere, timed, same  # noqa: E402

POPS = (2, 4, 8, 16, 32)
PIECES = (0.5, 1.0, 2.0, 4.0, 8.0)
POP, CAP, PIECE = 4, 2.0, 2.0     # RAY_CELL_POP, RAY_OVERSIZE_MULT and RAY_PIECE_CELLS of csrc/ray_cast.hip: the settings the routes are compared at
OUT = [None]


def say(text=""):
    print(text, flush=True)
    with open(OUT[0], "a") as fh:
        fh.write(text + "\n")


def make_rays(kind, v, f, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "sampler":
        fi = rng.integers(0, len(f), n)
        r1, r2 = np.sqrt(rng.uniform(size=n)), rng.uniform(size=n)
        a, b, c = (v[f[fi, k]] for k in range(3))
        surf = (1 - r1)[:, None] * a + (r1 * (1 - r2))[:, None] * b + (r1 * r2)[:, None] * c
        g = rng.normal(size=(n, 3))
        d = g / np.linalg.norm(g, axis=1)[:, None]
        lens = rng.uniform(size=n) * 0.027 + 0.003
        return surf + lens[:, None] * d, -d, lens * (1.0 + 2.0 ** -20)
    lo, hi = v.min(0), v.max(0)
    ext = float((hi - lo).max())
    u = rng.normal(size=(n, 3))
    o = (lo + hi) / 2 + 3 * ext * u / np.linalg.norm(u, axis=1)[:, None]
    target = rng.uniform(lo, hi, size=(n, 3))
    return o, target - o, None


class Call:
    """One (mesh, rays) pair on buffers allocated once; run(...) is one whole call of the tuned entry point."""

    def __init__(self, v, f, rays, dev):
        self.lib = _lib.load()
        self.v = torch.as_tensor(v, device=dev)
        self.f = torch.as_tensor(f, device=dev)
        self.o, self.d = torch.as_tensor(rays[0], device=dev), torch.as_tensor(rays[1], device=dev)
        self.tm = None if rays[2] is None else torch.as_tensor(rays[2], device=dev)
        self.nv, self.nf, self.nq = len(v), len(f), len(rays[0])
        self.t = torch.zeros((self.nq,), dtype=torch.float64, device=dev)
        self.face = torch.zeros((self.nq,), dtype=torch.int64, device=dev)
        self.hit = torch.zeros((self.nq, 3), dtype=torch.float64, device=dev)
        self.nbytes = int(self.lib.sapcu_ray_mesh_workspace_bytes(self.nv, self.nf, self.nq))
        self.ws = torch.zeros((self.nbytes,), dtype=torch.uint8, device=dev)
        self.info = (ctypes.c_int64 * 6)()
        self.ext = float((self.v.max(0)[0] - self.v.min(0)[0]).max())

    def run(self, cell=0.0, brute=False, mult=CAP, pop=POP, piece=PIECE, auto=False):
        p = _lib.ptr
        _lib.check(self.lib.sapcu_internal_ray_mesh_tuned(p(self.v), self.nv, p(self.f), self.nf, p(self.o), p(self.d), p(self.tm), self.nq,
                                                          float(cell), float(mult), int(pop), float(piece), 1 if brute else (0 if auto else 2), p(self.t),
                                                          p(self.face), p(self.hit), p(self.ws), self.nbytes, self.info,
                                                          _lib.current_stream()))
        return list(self.info)

    def bits(self):
        return self.t.clone().view(torch.int64), self.face.clone(), self.hit.clone().view(torch.int64)

    def auto_cell(self, pop):
        return self.ext * (2.0 * pop / self.nf) ** 0.5         # what cell_size 0 computes from the centroids' extent (about the vertices')


def pair(name, c, runs, brute_runs, sweeps=False):
    grid = lambda: c.run(cell=c.auto_cell(POP))                                                  # noqa: E731
    brute = lambda: c.run(brute=True)                                                           # noqa: E731
    w_g, info = timed(grid)                                                                     # warm-up of both paths
    g = c.bits()
    w_b, _ = timed(brute)
    assert same(g, c.bits()), (name, info)
    hits = int((c.face >= 0).sum())
    if w_g > 20 * w_b or w_g > 5000.0:                                                          # a route this far behind is timed once
        runs = 1
    tg, tb = [], []
    for r in range(max(runs, brute_runs)):                                                      # alternated
        if r < runs:
            tg.append(timed(grid)[0])
        if r < brute_runs:
            tb.append(timed(brute)[0])
    say("%s: %d faces, %d rays (%d hit), grid %d x %d x %d, %d oversize%s, bit-equal to brute force (t, face, hit point)" %
        (name, c.nf, c.nq, hits, info[1], info[2], info[3], info[4], "" if info[0] else " (FELL BACK to brute force)"))
    say("  grid  ms: %s   (min %.3f, med %.3f, max %.3f)" % (" ".join("%.3f" % t for t in tg), min(tg), float(np.median(tg)), max(tg)))
    say("  brute ms: %s   (min %.3f, med %.3f, max %.3f)" % (" ".join("%.3f" % t for t in tb), min(tb), float(np.median(tb)), max(tb)))
    say("  median against median: grid %.2f x faster; every grid run faster than every brute run: %s" %
        (float(np.median(tb)) / float(np.median(tg)), max(tg) < min(tb)))
    info = c.run(auto=True)
    assert same(g, c.bits()), (name, "automatic")
    ta = [timed(lambda: c.run(auto=True))[0] for _ in range(brute_runs)]
    say("  automatic (cell_size 0) takes the %s route: ms %s   (med %.3f)" % ("grid" if info[0] else "brute-force", " ".join("%.3f" % t for t in ta),
                                                                              float(np.median(ta))))
    if not sweeps:
        return
    row = []
    for pop in POPS:
        info = c.run(cell=c.auto_cell(pop))
        assert same(g, c.bits()), (name, pop)
        ts = [timed(lambda: c.run(cell=c.auto_cell(pop)))[0] for _ in range(runs)]
        row.append("c=%d (%dx%dx%d%s): min %.3f med %.3f" % (pop, info[1], info[2], info[3], "" if info[0] else ", FELL BACK", min(ts),
                                                             float(np.median(ts))))
    say("  population sweep ms: " + " | ".join(row))
    row = []
    for piece in PIECES:
        info = c.run(cell=c.auto_cell(POP), piece=piece)
        assert same(g, c.bits()), (name, piece)
        ts = [timed(lambda: c.run(cell=c.auto_cell(POP), piece=piece))[0] for _ in range(runs)]
        row.append("piece=%.1f h: min %.3f med %.3f" % (piece, min(ts), float(np.median(ts))))
    say("  piece length sweep ms (c=%d): " % POP + " | ".join(row))


def main():
    OUT[0] = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "ray_cast.txt")
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    assert torch.cuda.is_available(), "ray_cast.py measures on a GPU"
    open(OUT[0], "w").close()
    dev = torch.device("cuda:0")
    say("# ray casting: grid route against brute-force route (csrc/ray_cast.hip)")
    say("# %s, torch %s; times are device-event ms of the whole call, paths alternated, %d runs each (brute on 385 582 rays: 3)" %
        (torch.cuda.get_device_name(0), torch.__version__, runs))
    say("# icospheres of radius 0.5; rays: the sampler's (0.003 .. 0.03 off the surface, cast back) and unbounded ones from three extents away")
    meshes = {level: icosphere(level, 0.5) for level in (2, 3, 4, 5, 6)}
    for level in (2, 3, 4, 5, 6):
        v, f = meshes[level]
        for n, br in ((8192, runs), (385582, 3)):
            for kind in ("sampler", "unbounded"):
                c = Call(v, f, make_rays(kind, v, f, n, 100 * level + (n & 1)), dev)
                pair("%d faces x %d %s rays" % (len(f), n, kind), c, runs, br, sweeps=(level in (4, 6) and n == 8192))
                del c


if __name__ == "__main__":
    main()
