"""Times of the streamed Sinkhorn half-step (csrc/sinkhorn.hip) against the dense form: writes the text of profiles/sinkhorn.txt.

    python profiles/sinkhorn.py [OUT]        (needs the GPU; OUT defaults to stdout)

Per size n = m in 2048, 8192, 32768 and p in 1, 2: the half-step (sapcu_softmin_f64: h kernel + softmin kernel + merge) on
preallocated buffers, device events around REPS calls, several rounds after a warm-up -> best and median ms per half-step and
pairs/s; the plan statistics the same way; one default sinkhorn_metrics call at 8192 x 8192 (host wall, ends with the figures on the
host); and at 8192 x 8192 the dense form the reference's README describes, in torch on the same device: the f64 cost matrix
materialised once (as that recipe keeps it), then a half-step = torch.logsumexp(h[None, :] - C / eps, dim=1)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS = 7


def _events(fn, reps):
    """ms per call: `reps` calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _rounds(fn, reps):
    for _ in range(2):
        _events(fn, max(1, reps // 2))                      # warm-up
    t = sorted(_events(fn, reps) for _ in range(ROUNDS))
    return t[0], t[len(t) // 2]


def main():
    from sapcu_amd import _lib, sinkhorn
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout

    def say(text):
        print(text, file=out, flush=True)
        if out is not sys.stdout:
            print(text, flush=True)

    dev = torch.device("cuda:0")
    lib = _lib.load()
    eps_of = {1: 0.05, 2: 0.05 ** 2}
    say("# streamed Sinkhorn half-step (csrc/sinkhorn.hip) on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("# device-event ms per call over back-to-back calls on preallocated buffers, %d rounds after a warm-up: best / median" % ROUNDS)
    rng = np.random.default_rng(0)
    for n in (2048, 8192, 32768):
        x = torch.from_numpy(rng.uniform(size=(n, 3))).to(dev)
        y = torch.from_numpy(rng.uniform(size=(n, 3)) + 0.05).to(dev)
        pot = torch.from_numpy(rng.normal(size=n) * 0.05).to(dev)
        f = torch.from_numpy(rng.normal(size=n) * 0.05).to(dev)
        res, res2 = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
        nbytes = int(lib.sapcu_sinkhorn_workspace_bytes(n, n))
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        st = _lib.current_stream()
        tile, min_cols, split, chunk = sinkhorn.split_plan(n, n)
        reps = {2048: 200, 8192: 40, 32768: 5}[n]
        say("n = m = %d: %d chunks of %d columns, %d wavefronts, workspace %.2f MB (the dense f64 matrix: %.1f MB)" % (
            n, split, chunk, (n + 63) // 64 * split, nbytes / 1e6, n * n * 8 / 1e6))
        for p in (1, 2):
            eps = eps_of[p]

            def half():
                _lib.check(lib.sapcu_softmin_f64(_lib.ptr(x), n, _lib.ptr(y), n, _lib.ptr(pot), p, eps, _lib.ptr(res), _lib.ptr(ws), nbytes, st))

            def stats():
                _lib.check(lib.sapcu_plan_stats_f64(_lib.ptr(x), n, _lib.ptr(y), n, _lib.ptr(f), _lib.ptr(pot), p, eps, _lib.ptr(res),
                                                    _lib.ptr(res2), _lib.ptr(ws), nbytes, st))

            best, med = _rounds(half, reps)
            sbest, smed = _rounds(stats, reps)
            say("  p = %d  half-step %.4f / %.4f ms  = %.1f / %.1f G pairs/s    plan statistics %.4f / %.4f ms" % (
                p, best, med, n * n / best / 1e6, n * n / med / 1e6, sbest, smed))
        if n == 8192:
            for p in (1, 2):
                eps = eps_of[p]
                d = x[:, None, :] - y[None, :, :]
                s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                del d
                C = 0.5 * s if p == 2 else torch.sqrt(s)
                del s
                h = np.log(1.0 / n) + pot / eps

                def dense():
                    return -eps * torch.logsumexp(h[None, :] - C / eps, dim=1)

                best, med = _rounds(dense, 10)
                half()
                torch.cuda.synchronize()
                diff = float((dense() - res).abs().max())
                say("  p = %d  dense torch half-step (cost matrix kept, logsumexp over h - C / eps): %.4f / %.4f ms; max |dense - streamed| = %.2e"
                    % (p, best, med, diff))
                del C
            torch.cuda.synchronize()
            for p in (1, 2):
                times = []
                for _ in range(4):
                    t0 = time.perf_counter()
                    m = sinkhorn.sinkhorn_metrics(x, y, p=p)
                    times.append((time.perf_counter() - t0) * 1e3)
                say("  p = %d  sinkhorn_metrics(x, y) at its defaults (blur 0.05, 100 iterations, debias: 400 half-steps and the statistics), "
                    "host wall ms: %s" % (p, " ".join("%.1f" % t for t in times)))
                say("         ot %.9f primal_cost %.9f marginal_error %.3e divergence %.9f" % (m["ot"], m["primal_cost"], m["marginal_error"],
                                                                                                m["divergence"]))
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
