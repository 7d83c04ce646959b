"""Step time, clouds/s and launch count of one fd training step (row f-5) at the reference's shape — config/fd.yaml: 4 clouds x 16
patches x 100 points, k = 32, k_scales = [8, 16, 32, 48], T = 7, emb_dims = 768, num_heads = 8, dropout 0.1; AdamW, grad_clip 0.1.

    python profiles/fd_train_step.py [--steps 10] [--warmup 3] [--precision f32|bf16] [--edgeconv feature|factored] [--graph]
                                     [--round N] [--out FILE]

The default (f32, feature) is fd_trainer.Trainer's step; anything else runs fd_trainer.AmpTrainer.  --out appends.
--graph times fd_trainer.GraphedTrainStep over the same trainer (AdamW capturable=True; its warm-up steps are the eager ones) and
adds "shadow_select_ms": the shadow copies plus the sapcu_multi_select launch it adds to a step, timed on their own.  An A/B is
this script alternated, eager and --graph, configuration by configuration, two rounds in one session (--round tags the line).

Prints (and writes to --out) one JSON line.  The launch count is the number of device kernels torch's profiler sees in one step
(HIP ops of the library and torch's own element-wise / optimiser kernels alike)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shadow_select_ms(step, reps=50):
    """What GraphedTrainStep adds to a step (its run_added_work: the shadow copies and one sapcu_multi_select launch with the flag
    clear), timed on its own with events."""
    step.run_added_work()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        step.run_added_work()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--edgeconv", choices=("feature", "factored"), default="feature")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--round", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sapcu_amd
    from sapcu_amd import fd_trainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    kw = dict(k=32, emb_dims=768, time_steps_enc=7, time_steps_dec=10, num_heads=8, dropout=0.1, k_scales=[8, 16, 32, 48])
    model = sapcu_amd.TrainableSNNDistanceEstimation(**kw).to(dev)
    model.dropout_generator = torch.Generator(device=dev).manual_seed(1)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, capturable=True) if a.graph else torch.optim.AdamW(model.parameters(), lr=1e-4)
    if a.precision == "f32" and a.edgeconv == "feature":
        trainer = fd_trainer.Trainer(model, opt, device=dev, grad_clip=0.1)
    else:
        trainer = fd_trainer.AmpTrainer(model, opt, device=dev, grad_clip=0.1, use_amp=a.precision == "bf16", edgeconv=a.edgeconv)
    batches = list(fd_trainer.SyntheticFdPatches(batches=a.warmup + a.steps + 1, batch_size=4, patches=16, points=100, seed=0))
    losses = []
    for b in batches[:a.warmup]:
        losses.append(trainer.train_step(b)[0])
    extra = {}
    if a.graph:
        trainer = fd_trainer.GraphedTrainStep(trainer, batches[0], warmup=0)
        extra["shadow_select_ms"] = round(shadow_select_ms(trainer), 4)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for b in batches[a.warmup:a.warmup + a.steps]:
        losses.append(trainer.train_step(b)[0])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            trainer.train_step(batches[-1])
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    except Exception as e:                                   # the profiler is optional: the timing stands without it
        print("profiler unavailable: %r" % (e,), file=sys.stderr)
    if a.round is not None:
        extra["round"] = a.round
    res = {"what": "fd training step, %s, %s EdgeConv%s" % (a.precision, a.edgeconv, ", HIP graph" if a.graph else ""), "shape": "4 clouds x 16 patches x 100 points", "model": kw, "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": round(dt * 1e3, 2), "clouds_per_s": round(4 / dt, 2), "device_kernels_per_step": launches,
           "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "first_loss": losses[0], "last_loss": losses[-1],
           "device": torch.cuda.get_device_name(0)}
    res.update(extra)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
