#!/usr/bin/env python3
"""What building a training batch on the device costs (csrc/train_patches.hip through sapcu_amd.data), next to what it replaces
and next to the step it feeds.

In one session, after a warm-up of every shape: (1) device-event time of ``build_patches`` per batch — 50 back-to-back calls in one
timed window, several windows — for the fd shape (256 input / 1024 dense points, k = 32, rotation + scale + jitter) at B = 4 and
B = 64 and the fn shape (512 points, normals, 64 centres, k = 12) at B = 4, each also with one part left out (no dense = no
nearest-dense kernel) so that the phases can be told apart; (2) a whole loader batch (draws + call) by the host clock; (3) the same
batch the reference's way on the host — numpy + two scipy cKDTree builds per sample (tests/data_ref.py's arithmetic), the samples of
a batch spread over 16 threads; (4) the eager ``fd_trainer.AmpTrainer`` step at B = 4 on a loader batch.  There is no bar: none of
these numbers existed.  Needs a GPU; writes the report (default profiles/train_patches.txt).

Usage: train_patches.py [report path] [windows]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sapcu_amd  # noqa: E402,F401
from sapcu_amd import data, fd_trainer  # noqa: E402
import data_ref as R  # noqa: E402

CALLS = 50
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def window(fn, calls=CALLS):
    """ms per call over `calls` back-to-back calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def report(name, fn, windows):
    fn()
    ts = [window(fn) for _ in range(windows)]
    say("  %-58s %s   (min %.4f, median %.4f)" % (name, " ".join("%.4f" % t for t in ts), min(ts), float(np.median(ts))))
    return float(np.median(ts))


def sphere(rng, S, count):
    u, v = rng.uniform(0, 2 * np.pi, (S, count)), rng.uniform(-1, 1, (S, count))
    return np.stack([np.sqrt(1 - v * v) * np.cos(u), np.sqrt(1 - v * v) * np.sin(u), v], -1).astype(np.float32)


def draws(dev, b, n, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    theta = torch.rand((b,), generator=gen, device=dev, dtype=torch.float64) * (2 * np.pi)
    rot = torch.zeros((b, 3, 3), device=dev)
    c, s = torch.cos(theta).float(), torch.sin(theta).float()
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = c, -s, s, c, 1.0
    scale = (0.8 + 0.4 * torch.rand((b,), generator=gen, device=dev)).float()
    jitter = torch.randn((b, n, 3), generator=gen, device=dev) * 0.002
    return rot, scale, jitter


def host_batch(inputs, dense, normals, idx, rot, scale, jitter, centres, k, pool):
    """The reference's construction of the same batch on the host: numpy in data_ref's order, neighbours by scipy's cKDTree."""
    from scipy.spatial import cKDTree

    def one(i):
        s = idx[i]
        cloud, dn, nr = R.augment(inputs[s], None if dense is None else dense[s], None if normals is None else normals[s], rot[i], scale[i],
                                  jitter[i])
        cloud, dn, _, _ = R.normalise(cloud, dn)
        out = {}
        if dn is not None:
            out["len"] = cKDTree(dn).query(cloud, k=1)[0].astype(np.float32)
        if nr is not None:
            out["normals"] = R.renormalise(nr)
        q = cloud if centres is None else cloud[centres[i]]
        out["idx"] = cKDTree(cloud).query(q, k=k)[1]
        out["input"] = cloud[out["idx"]]
        return out
    return list(pool.map(one, range(len(idx))))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_patches.txt")
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    assert torch.cuda.is_available(), "train_patches.py measures on a GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    S = 64
    fd_in, fd_dense = sphere(rng, S, 256) * np.float32(0.5), sphere(rng, S, 1024) * np.float32(0.5)
    fn_nrm = sphere(rng, S, 512)                                     # a sphere's normal is its point
    fn_pts = fn_nrm * np.float32(0.5)
    d_in, d_dense, d_pts, d_nrm = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (fd_in, fd_dense, fn_pts, fn_nrm))
    say("# training batches on the device: sapcu_train_patches_f32 through sapcu_amd.data.build_patches (validate=False)")
    say("# %s, torch %s; ms per batch: %d back-to-back calls between two device events, %d windows each, after a warm-up" %
        (torch.cuda.get_device_name(0), torch.__version__, CALLS, windows))
    results = {}
    host_rows = []
    for name, b in (("fd B=4", 4), ("fd B=64", 64)):
        idx = torch.arange(b, device=dev) % S
        rot, scale, jitter = draws(dev, b, 256, b)
        full = lambda: data.build_patches(d_in, idx, 32, dense=d_dense, rotation=rot, scale=scale, jitter=jitter, validate=False)   # noqa: E731
        nolen = lambda: data.build_patches(d_in, idx, 32, rotation=rot, scale=scale, jitter=jitter, validate=False)                 # noqa: E731
        say("%s (256 / 1024 points, all 256 centres, k = 32):" % name)
        results[name] = report("whole call (prepare + nearest-dense + neighbours)", full, windows)
        report("without dense (prepare + neighbours)", nolen, windows)
        host_rows.append((name, fd_in, fd_dense, None, idx.cpu().numpy(), rot.cpu().numpy(), scale.cpu().numpy(), jitter.cpu().numpy(), None, 32))
    b = 4
    idx = torch.arange(b, device=dev)
    rot, scale, jitter = draws(dev, b, 512, 7)
    centres = torch.stack([torch.randperm(512, device=dev)[:64] for _ in range(b)]).to(torch.int32)
    say("fn B=4 (512 points with normals, 64 centres, k = 12):")
    results["fn B=4"] = report("whole call (prepare + neighbours)", lambda: data.build_patches(
        d_pts, idx, 12, normals=d_nrm, rotation=rot, scale=scale, jitter=jitter, centres=centres, validate=False), windows)
    host_rows.append(("fn B=4", fn_pts, None, fn_nrm, idx.cpu().numpy(), rot.cpu().numpy(), scale.cpu().numpy(), jitter.cpu().numpy(),
                      centres.cpu().numpy(), 12))

    say("a loader batch by the host clock (draws from the device generator + the call, ended by a synchronise), ms:")
    for name, loader in (("PU1KPatches B=4", data.PU1KPatches(fd_in, fd_dense, split="all", batch_size=4, augment=True, device=dev)),
                         ("PU1KPatches B=64", data.PU1KPatches(fd_in, fd_dense, split="all", batch_size=64, augment=True, device=dev)),
                         ("MeshPatches B=4", data.MeshPatches(fn_pts, fn_nrm, split="all", batch_size=4, augment=True, device=dev))):
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
        say("  %-58s %s   (per batch, %d batches per epoch; the first epoch warms up)" % (name, " ".join("%.3f" % t for t in ts), count))

    say("the same batches on the host, the reference's way (numpy + two cKDTree builds per sample, 16 threads), ms per batch:")
    try:
        with ThreadPoolExecutor(16) as pool:
            for row in host_rows:
                host_batch(*row[1:], pool)
                ts = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    host_batch(*row[1:], pool)
                    ts.append((time.perf_counter() - t0) * 1e3)
                say("  %-58s %s   (median %.2f; device %.4f: %.0f x)" % (row[0], " ".join("%.2f" % t for t in ts), float(np.median(ts)),
                                                                        results[row[0]], float(np.median(ts)) / results[row[0]]))
    except ImportError:
        say("  not measured: scipy is not installed here")

    say("the step a batch feeds: eager fd_trainer.AmpTrainer (bf16, factored EdgeConv) at B = 4 on a PU1KPatches batch [4,256,32,3], ms:")
    torch.manual_seed(0)
    kw = dict(k=32, emb_dims=768, time_steps_enc=7, time_steps_dec=10, num_heads=8, dropout=0.1, k_scales=[8, 16, 32, 48])
    model = sapcu_amd.TrainableSNNDistanceEstimation(**kw).to(dev)
    model.dropout_generator = torch.Generator(device=dev).manual_seed(1)
    trainer = fd_trainer.AmpTrainer(model, torch.optim.AdamW(model.parameters(), lr=1e-4), device=dev, grad_clip=0.1)
    loader = data.PU1KPatches(fd_in, fd_dense, split="all", batch_size=4, augment=True, device=dev)
    batches = [b for _, b in zip(range(8), loader)]
    ts, losses = [], []
    for i, batch in enumerate(batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses.append(trainer.train_step(batch)[0])
        torch.cuda.synchronize()
        if i >= 3:
            ts.append((time.perf_counter() - t0) * 1e3)
    step = float(np.median(ts))
    say("  %s   (median %.2f after 3 warm-up steps; losses %s)" % (" ".join("%.2f" % t for t in ts), step,
                                                                 " ".join("%.4f" % float(v) for v in losses if v is not None)))
    say("building the fd B = 4 batch takes %.2f %% of the step it feeds (a tenth would be %.2f ms)" % (100 * results["fd B=4"] / step, step / 10))
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
