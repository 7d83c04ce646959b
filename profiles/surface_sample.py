#!/usr/bin/env python3
"""What sampling fn's training clouds from the meshes costs on the device (csrc/surface_sample.hip through sapcu_amd.surface and
sapcu_amd.data.MeshSurfacePatches), next to what it replaces.

In one session, after a warm-up of every shape: (1) the tables call (``sapcu_surface_tables_f32`` on buffers allocated once: faces,
area sum, cdf) for the fixture's 5000-face torus and for a torus of 100 352 faces, whole calls by device events; (2) the sampler
(``sample_surface`` with its output fills, ``validate=False``) at b = 4 and b = 64 meshes of 100 352 faces, n = 512 — 50 back-to-back
calls in one timed window, several windows; (3) a whole ``MeshSurfacePatches`` batch (draws + sampler + ``build_patches``) by the host
clock; (4) the same samplings the reference's way on the same box: numpy, per sample, from the mesh (cross products, norms, sum,
``RandomState.choice``, barycentric points).  There is no bar: none of these numbers existed.  Needs a GPU; writes the report
(default profiles/surface_sample.txt).

Usage: surface_sample.py [report path] [windows]
       surface_sample.py --one     (twenty tables calls and two hundred sampler calls at the large shapes: for a profiler)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sapcu_amd  # noqa: E402,F401
from sapcu_amd import _lib, data, surface  # noqa: E402

CALLS = 50
N = 512
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def torus(nu, nw, R=0.6, r=0.25):
    u, w = np.arange(nu) * (2 * np.pi / nu), np.arange(nw) * (2 * np.pi / nw)
    gu, gw = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(gw)) * np.cos(gu), (R + r * np.cos(gw)) * np.sin(gu), r * np.sin(gw)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nw), indexing="ij")
    idx = lambda a, b: (a % nu) * nw + (b % nw)                                                 # noqa: E731
    f = np.concatenate([np.stack([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], -1).reshape(-1, 3),
                        np.stack([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)], -1).reshape(-1, 3)])
    return v.astype(np.float32), f.astype(np.int32)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def window(fn, calls=CALLS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


class TablesCall:
    """sapcu_surface_tables_f32 for S copies of one mesh on buffers allocated once."""

    def __init__(self, mesh, S, dev):
        v, f = mesh
        self.lib, self.S, self.tv, self.tf = _lib.load(), S, S * len(v), S * len(f)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                         # noqa: E731
        self.v, self.f = up(np.tile(v, (S, 1))), up(np.tile(f, (S, 1)))
        self.vo, self.fo = up(np.arange(S + 1, dtype=np.int64) * len(v)), up(np.arange(S + 1, dtype=np.int64) * len(f))
        self.nrm = torch.zeros((self.tf, 3), device=dev)
        self.cdf = torch.zeros((self.tf,), dtype=torch.float64, device=dev)
        self.area, self.prob = torch.zeros((S,), device=dev), torch.zeros((S,), dtype=torch.float64, device=dev)
        self.nbytes = int(self.lib.sapcu_surface_tables_workspace_bytes(S, self.tf))
        self.ws = torch.zeros((self.nbytes,), dtype=torch.uint8, device=dev)

    def run(self):
        p = _lib.ptr
        _lib.check(self.lib.sapcu_surface_tables_f32(p(self.v), p(self.vo), self.tv, p(self.f), p(self.fo), self.tf, self.S, p(self.nrm),
                                                     p(self.cdf), p(self.area), p(self.prob), p(self.ws), self.nbytes, _lib.current_stream()))


def host_sampling(v, f, n, rng_state):
    """One sampling the reference's way: everything from the mesh, per sample, in numpy (fn/datacore.py:122-184 in outline)."""
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cross = np.cross(v1 - v0, v2 - v0)
    norms = np.linalg.norm(cross, axis=1, keepdims=True)
    normals = cross / np.maximum(norms, 1e-8)
    areas = 0.5 * norms[:, 0]
    face = rng_state.choice(len(f), size=n, p=areas / (areas.sum() + 1e-8))
    r1, r2 = rng_state.random_sample(n).astype(np.float32), rng_state.random_sample(n).astype(np.float32)
    s = np.sqrt(r1)
    points = (1 - s)[:, None] * v[f[face, 0]] + (s * (1 - r2))[:, None] * v[f[face, 1]] + (s * r2)[:, None] * v[f[face, 2]]
    return points.astype(np.float32), normals[face].astype(np.float32)


def draws(dev, b, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand((b, N), generator=gen, device=dev, dtype=torch.float64)
    return u, torch.rand((b, N), generator=gen, device=dev), torch.rand((b, N), generator=gen, device=dev)


def one(dev):
    big = torus(224, 224)
    call = TablesCall(big, 1, dev)
    for _ in range(20):
        call.run()
    t = surface.build_surface_tables([big] * 64, device=dev)
    idx = torch.arange(64, device=dev)
    u, r1, r2 = draws(dev, 64, 1)
    for _ in range(200):
        surface.sample_surface(t, idx, N, u, r1, r2, validate=False)
    torch.cuda.synchronize()


def main():
    assert torch.cuda.is_available(), "surface_sample.py measures on a GPU"
    dev = torch.device("cuda:0")
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        return one(dev)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "surface_sample.txt")
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    g = np.load(os.path.join(ROOT, "tests", "golden", "surface_sample.npz"))
    small = (g["torus/vertices"], g["torus/faces"])
    big = torus(224, 224)
    say("# sampling triangle meshes on the device: sapcu_surface_tables_f32 / sapcu_surface_sample_f32 (csrc/surface_sample.hip)")
    say("# %s, torch %s; device-event ms after a warm-up; windows of %d back-to-back calls" % (torch.cuda.get_device_name(0), torch.__version__,
                                                                                                CALLS))
    say("the tables call (faces + area sum + cdf: three launches), whole call, ms:")
    for name, mesh, S in (("fixture torus, %d faces, 1 mesh" % len(small[1]), small, 1), ("torus, %d faces, 1 mesh" % len(big[1]), big, 1),
                          ("torus, %d faces, 64 meshes in one call" % len(big[1]), big, 64)):
        call = TablesCall(mesh, S, dev)
        call.run()
        ts = [timed(call.run) for _ in range(2 * windows)]
        say("  %-52s %s   (min %.4f, median %.4f)" % (name, " ".join("%.4f" % t for t in ts), min(ts), float(np.median(ts))))
    device_ms = {}
    say("the sampler (one launch; with the fills of its three outputs), n = %d, meshes of %d faces, ms per call:" % (N, len(big[1])))
    tables = surface.build_surface_tables([big] * 64, device=dev)
    for b in (4, 64):
        idx = torch.arange(b, device=dev)
        u, r1, r2 = draws(dev, b, b)
        fn = lambda: surface.sample_surface(tables, idx, N, u, r1, r2, validate=False)          # noqa: E731
        fn()
        ts = [window(fn) for _ in range(windows)]
        device_ms[b] = float(np.median(ts))
        say("  b = %-49d %s   (min %.4f, median %.4f)" % (b, " ".join("%.4f" % t for t in ts), min(ts), device_ms[b]))
    say("the same on the fixture torus (%d faces):" % len(small[1]))
    tables_small = surface.build_surface_tables([small] * 64, device=dev)
    for b in (4, 64):
        idx = torch.arange(b, device=dev)
        u, r1, r2 = draws(dev, b, b)
        fn = lambda: surface.sample_surface(tables_small, idx, N, u, r1, r2, validate=False)    # noqa: E731
        fn()
        ts = [window(fn) for _ in range(windows)]
        say("  b = %-49d %s   (min %.4f, median %.4f)" % (b, " ".join("%.4f" % t for t in ts), min(ts), float(np.median(ts))))

    say("a MeshSurfacePatches batch by the host clock (draws + sampler + build_patches, ended by a synchronise), 64 meshes, ms:")
    for name, mesh in (("%d faces" % len(small[1]), small), ("%d faces" % len(big[1]), big)):
        for bs in (4, 64):
            loader = data.MeshSurfacePatches([mesh] * 64, num_points=N, split="all", batch_size=bs, augment=True, device=dev)
            ts = []
            for epoch in range(3):
                loader.set_epoch(epoch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                count = 0
                for _ in loader:
                    count += 1
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3 / count)
            say("  %-52s %s   (per batch, %d batches per epoch; the first epoch warms up)" % ("%s, batch %d" % (name, bs),
                                                                                              " ".join("%.3f" % t for t in ts), count))

    say("the reference's way on this box: numpy per sample, everything from the mesh (one thread), ms per SAMPLE:")
    state = np.random.RandomState(0)
    for name, mesh in (("%d faces" % len(small[1]), small), ("%d faces" % len(big[1]), big)):
        host_sampling(mesh[0], mesh[1], N, state)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            host_sampling(mesh[0], mesh[1], N, state)
            ts.append((time.perf_counter() - t0) * 1e3)
        say("  %-52s %s   (median %.3f)" % (name, " ".join("%.3f" % t for t in ts), float(np.median(ts))))
        if mesh is big:
            for b in (4, 64):
                say("    a batch of %d such samples: %.2f ms against %.4f ms of the sampler: %.0f x" % (
                    b, b * float(np.median(ts)), device_ms[b], b * float(np.median(ts)) / device_ms[b]))
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
