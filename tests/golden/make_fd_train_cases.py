"""Writes tests/fd_train_cases.py: the inputs of the fd training-step sweep (tests/test_gpu_fd_train_shapes.py), chosen on the CPU
from the oracle alone.  A case is a batch gpu_utils.sphere_patches(P, M, skip=...) with ground-truth distances from a generator
seeded by the case, taken through oracle.train_path.fd_train_forward + distance_loss + backward.

Weights: testing.training_state_dict(shell, WEIGHT_SEED = 12) with encoder.snn_fc.threshold_base shifted by FC_THRESHOLD_SHIFT, as
make_fd_train_fixtures.py shifts it (without the shift every snn_fc neuron fires for every patch and the decoder's BatchNorms see
P identical rows).  Families:

  "M"   the base configuration (BASE_KW: k = 20, k_scales = (10, 20, 40), emb_dims = 96, T = 4, heads = 4 — configuration B of the
        reference runs), P = 4 (P = 3 from M = 100) and M = M_SIZES: through the clamps min(k, M) at 10, 20 and 40, P M through 16, 64
        and 256 rows, the edge rows P M kk through 1024, up to the largest patch sapcu_patch_knn takes.
  "P"   the base configuration at M = 12: every neighbour count clamps to 12, P 12 point rows and P 144 edge rows.  P_SIZES is
        derived below from the constants of the kernels.
  "hp"  P = 4, M = 48 (fd-kclamp, fd-sclamp: M = 12), one case per fd row of the hyper-parameter matrix of make_fixtures.py; the
        row's constructor arguments are read from tests/golden/hparams.npz (conftest.FD_KW with the row's override), dropout 0.

Rule per case: try skip = 300, 303, 306, ... for at most CANDIDATES and take the first candidate at which

  (a) the oracle's FREE f32 run (its own tables under the library's neighbour rule, its own spikes) and its f64 run FORCED on that
      run's tables and spikes agree on
        the prediction   max |f32 - f64| <= COND = 3e-5,
        the loss         |f32 - f64| <= COND,
        the gradients    max over the compared tensors of max|f32 - f64| / (max|f64| + 5e-5 peak) <= GRAD_COND = 2e-3 (the scale of
                         test_oracle_golden.check_fn_train_grads; a tenth of the 2e-2 the GPU tests allow the device);
        the buffers      max |f32 - f64| over the BatchNorm running statistics after the step (momentum 0.1) <= BUF_COND = 1e-6, a
                         tenth of the 1e-5 the GPU tests allow the device.  (A BatchNorm over very few rows — the decoder's at
                         P = 2 — turns a rounding of its input into a relative error of its batch variance that is many times
                         larger: at P = 2, skip 300 the oracle's own f32 run is 4.1e-6 off on a decoder running_var of 0.4.)
  (b) the f32 prediction is spread out over the patches: max - min >= SPREAD = 2e-2;
  (c) the snn_fc spikes hold a 0 and a 1 and no two patches have the same spike row (two equal rows of the decoder's input make
      two equal rows in each of its BatchNorms).

The biases in front of a BatchNorm (make_fn_train_cases.cancelled: the decoder's fc_in.0, fc.0, fc.4, fc_hidden.0) are not compared:
they cancel in the normalisation and their gradient is rounding noise in the oracle itself.  A gradient that is None counts as zero.

A case with no qualifying candidate goes to UNSCREENED with its best candidate (smallest prediction and buffer gaps relative to their conditions
among those that pass (b) and (c), if any) and a one-line structural reason from UNSCREENED_REASONS; more than CAP = 4 such keys IN TOTAL is an error here and
in tests/test_fd_train_cases_host.py.  MOVED lists cases whose first qualifying candidates the GPU sweep set aside for a cause
outside the device and outside the oracle's restatement; the generator passes over that many qualifying candidates.

Needs nothing but oracle/, sapcu_amd.testing, gpu_utils.sphere_patches and tests/golden/hparams.npz; no GPU, no reference checkout.
Measured with one torch thread per worker, so that the numbers do not depend on the machine's core count:

    python tests/golden/make_fd_train_cases.py            # about 2 minutes on 8 cores
"""
import argparse
import multiprocessing
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_fn_train_cases import cancelled, grad_ratio  # noqa: E402  (the same rule for the same kind of tensor)

COND = 3e-5             # prediction and loss (the fn sweep's value)
GRAD_COND = 2e-3        # a tenth of the 2e-2 of test_training_step_of_whole_fd_model_teacher_forced_on_the_reference_run
BUF_COND = 1e-6         # a tenth of the 1e-5 of the same test's BatchNorm buffers
SPREAD = 2e-2
SKIP0, SKIP_STEP, CANDIDATES = 300, 3, 32
CAP = 4                 # unscreened keys in total
WEIGHT_SEED = 12
FC_THRESHOLD_SHIFT = 2.0                  # make_fd_train_fixtures.py FC_THRESHOLD_SHIFT
GT_RANGE = (0.05, 0.6)                    # inside what Softplus(beta = 5) of the head gives with these weights (0.01 .. 1.5)

BASE_KW = dict(k=20, emb_dims=96, time_steps_enc=4, num_heads=4, k_scales=[10, 20, 40], dropout=0.0)
M_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 15, 16, 17, 19, 20, 21, 31, 32, 33, 39, 40, 41, 47, 48, 49, 63, 64, 65, 100, 127, 128)

# "P" family.  At M = 12 every neighbour count is 12: P patches have 12 P point rows and 144 P edge rows per EdgeConv.
#   EC_STAT_PTS = 16, EC_GZ_PTS = 64   points per workgroup, csrc/fd_edgeconv_ops.hip       P_MIN = 2 (24 rows) is above 16; 5 (60) | 6 (72)
#   NS_ROWS_PER_WG = 64                rows per neuron-step workgroup, csrc/fd_train_ops.hip  5 (60) | 6 (72)
#   CR_ROWS = 256                      rows per f64 column-sum workgroup, csrc/train_ops.hip  21 (252) | 22 (264)
#   1024                               rows per weight-gradient slab (wgrad_slabs)            edge rows: 7 (1008) | 8 (1152)
#   64 x 1024 = 65 536                 wgrad_slabs' cap of 64 slabs                           edge rows: 456 (65 664): SLAB_CAP_P, outside the table
# The 16-point boundary is crossed by the "M" family (P M = 15 | 16 | 20 at M = 5, 4 | 5 ...).  P_MIN = 2 is the smallest batch a
# BatchNorm over the P decoder rows takes.  At SLAB_CAP_P one oracle step takes minutes: that batch runs without an oracle.
P_M = 12
P_MIN = 2
P_POINT_BOUNDS = (64, 256)
P_EDGE_BOUNDS = (1024,)
P_SLAB_CAP = 64 * 1024


def _p_sizes():
    out = {P_MIN}
    for bound in P_POINT_BOUNDS:
        out |= {bound // P_M, bound // P_M + 1}
    for bound in P_EDGE_BOUNDS:
        out |= {bound // (P_M * P_M), bound // (P_M * P_M) + 1}
    return tuple(sorted(out))


P_SIZES = _p_sizes()
assert P_SIZES == (2, 5, 6, 7, 8, 21, 22)
SLAB_CAP_P = P_SLAB_CAP // (P_M * P_M) + 1           # 456 patches: 65 664 edge rows, the first batch of whole patches past 64 slabs
SLAB_CAP_SKIP = SKIP0

HP_ROWS = ("fd-ctor", "fd-h1", "fd-h2", "fd-h16", "fd-h64", "fd-s1", "fd-s2u", "fd-s3", "fd-s5", "fd-s8", "fd-k1", "fd-k20", "fd-kfull",
           "fd-kclamp", "fd-sclamp", "fd-e32", "fd-e64", "fd-e96", "fd-e160", "fd-T1")
HP_P, HP_M, HP_M_CLAMP = 4, 48, 12
HP_CLAMP_ROWS = ("fd-kclamp", "fd-sclamp")

FAMILIES = {"M": M_SIZES, "P": P_SIZES, "hp": HP_ROWS}

# (family, key) -> the structural reason, for the shapes expected to have no qualifying candidate.  With these weights both do
# qualify (the f64 run is forced on the f32 run's spikes, so a degenerate BatchNorm cannot spread a flipped spike): the table has
# no unscreened key, and the reasons are kept for a regeneration with other weights.
UNSCREENED_REASONS = {
    ("M", 1): "one point per patch: every neighbour is the point itself, x_n - x_i = 0, and each BatchNorm sees P = 4 rows",
    ("hp", "fd-k1"): "k = 1: in blocks 1-3 every neighbour is the point itself, the x_n - x_i half of the feature is identically zero",
}

# family -> {key: (qualifying candidates to pass over, "diagnosis of the device's miss at the candidates left")}
MOVED = {"M": {}, "P": {}, "hp": {}}

_STATE = {}


def model_kw(family, key):
    """The constructor arguments of the case's model: BASE_KW, for "hp" the row of hparams.npz with dropout 0."""
    if family != "hp":
        return dict(BASE_KW)
    if "hparams" not in _STATE:
        import gpu_utils as U
        g = np.load(os.path.join(HERE, "hparams.npz"))
        _STATE["hparams"] = {rid: dict(U.hparam_row(g, rid)["kw"], dropout=0.0) for rid in HP_ROWS}
    return dict(_STATE["hparams"][key])


def shape(family, key):
    """(P, M) of the case."""
    if family == "M":
        return (3 if key >= 100 else 4), key
    if family == "P":                               # key SLAB_CAP_P included: same shape rule, no entry in the table
        return key, P_M
    return HP_P, (HP_M_CLAMP if key in HP_CLAMP_ROWS else HP_M)


def state_dict(family, key):
    """(state dict with the shifted snn_fc thresholds, parameter names) of the case's model."""
    kw = model_kw(family, key)
    tag = repr(sorted(kw.items()))
    if tag not in _STATE:
        import sapcu_amd
        from sapcu_amd import testing as T
        shell = sapcu_amd.TrainableSNNDistanceEstimation(**kw)
        sd = T.training_state_dict(shell.state_dict(), WEIGHT_SEED)
        sd["encoder.snn_fc.threshold_base"] = sd["encoder.snn_fc.threshold_base"] + FC_THRESHOLD_SHIFT
        _STATE[tag] = (sd, [n for n, _ in shell.named_parameters()])
    return _STATE[tag]


def gt_distances(family, key, p):
    """Ground-truth distances [p] (f32) of the case, uniform in GT_RANGE from a generator seeded by the case."""
    rng = np.random.default_rng([23, zlib.crc32(("%s/%s" % (family, key)).encode())])
    return torch.from_numpy(rng.uniform(GT_RANGE[0], GT_RANGE[1], p).astype(np.float32))


def inputs(family, key, skip):
    """(patches [P, M, 3] f32, gt [P] f32) of the case at candidate `skip`."""
    import gpu_utils as U
    p, m = shape(family, key)
    return U.sphere_patches(p, m, skip=skip), gt_distances(family, key, p)


def xyz_tables(family, key, pts):
    """The oracle's xyz tables of k_scales, each [P, M, min(k_scale, M)] (int64)."""
    from oracle import train_path as TP
    return [TP.xyz_knn(pts, min(int(ks), pts.shape[1])) for ks in model_kw(family, key)["k_scales"]]


def forcing(taps, steps):
    """(knn [T, 3, P, M, kk], force_spikes) that force a run on the tables and spikes `taps` recorded."""
    force = {"fc": taps["enc"][0].float()}
    for t in range(steps):
        for b in range(4):
            force[(t, b)] = taps["spikes"][4 * t + b].float()
    return torch.stack(taps["knn"]).long(), force


def oracle_step(family, key, pts, gt, dtype=torch.float32, knn=None, force=None, knn_xyz=None, grads=True, momentum=None):
    """One training step of the oracle in `dtype`, free (knn, force None) or forced: -> (prediction, loss, {name: gradient or
    None}, taps, p) as CPU tensors of that dtype; without `grads` the forward alone.  With momentum, p also carries the buffers."""
    from oracle import train_path as TP
    kw = model_kw(family, key)
    sd, names = state_dict(family, key)
    p = {n: sd[n].to(dtype).clone().requires_grad_(grads) for n in names}
    if momentum is not None:
        p.update({n: (v.clone() if v.dtype == torch.int64 else v.to(dtype).clone()) for n, v in sd.items() if n not in p})
    if force is not None:
        force = {k: v.to(dtype) for k, v in force.items()}
    taps = {}
    with torch.set_grad_enabled(grads):
        pred = TP.fd_train_forward(p, pts.to(dtype), kw["k"], tuple(kw["k_scales"]), kw["time_steps_enc"], kw["num_heads"], knn=knn,
                                   momentum=momentum, taps=taps, force_spikes=force, knn_xyz=knn_xyz)
        loss = TP.distance_loss(pred, gt.to(dtype))
        if grads:
            loss.backward()
    g = {n: p[n].grad for n in names} if grads else None
    return pred.detach(), loss.detach(), g, taps, p


def _zeros_for_none(g, sd):
    return {n: (v if v is not None else torch.zeros_like(sd[n], dtype=torch.float64)).detach() for n, v in g.items()}


def fc_ok(enc):
    """Condition (c) on the snn_fc spikes [P, emb]."""
    rows = {tuple(r.tolist()) for r in enc}
    return bool(enc.min() == 0) and bool(enc.max() == 1) and len(rows) == enc.shape[0]


def measure(family, key, skip, grads=True):
    """(prediction gap, loss gap, gradient gap, buffer gap, spread, condition (c)) at a candidate: the f32 free run and the f64 run forced on
    it; without `grads` the forwards alone and a gradient gap of 0."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        pts, gt = inputs(family, key, skip)
        kw = model_kw(family, key)
        xyz = xyz_tables(family, key, pts)
        p32, l32, g32, taps, b32 = oracle_step(family, key, pts, gt, torch.float32, knn_xyz=xyz, grads=grads, momentum=0.1)
        knn, force = forcing(taps, kw["time_steps_enc"])
        p64, l64, g64, _, b64 = oracle_step(family, key, pts, gt, torch.float64, knn=knn, force=force, knn_xyz=xyz, grads=grads, momentum=0.1)
        ratio = 0.0
        sd, names = state_dict(family, key)
        gb = max(float((b32[n].double() - b64[n]).abs().max()) for n in sd if n not in names and not n.endswith("num_batches_tracked"))
        if grads:
            ratio = grad_ratio(_zeros_for_none(g32, sd), _zeros_for_none(g64, sd), cancelled(sd))[0]
        spread = float(p32.max() - p32.min())
        return float((p64 - p32.double()).abs().max()), abs(float(l64) - float(l32)), ratio, gb, spread, fc_ok(taps["enc"][0])
    finally:
        torch.set_num_threads(threads)


def qualifies(gp, gl, gg, gb, spread, fc):
    return gp <= COND and gl <= COND and gg <= GRAD_COND and gb <= BUF_COND and spread >= SPREAD and fc


def choose(job):
    """(family, key) -> (family, key, skip, prediction gap, loss gap, gradient gap, buffer gap, spread, (c), screened)."""
    family, key = job
    pass_over = MOVED[family].get(key, (0,))[0]
    best = None
    for c in range(CANDIDATES):
        skip = SKIP0 + SKIP_STEP * c
        gp, gl, _, gb, spread, fc = measure(family, key, skip, grads=False)
        if gp <= COND and gl <= COND and gb <= BUF_COND and spread >= SPREAD and fc:
            full = measure(family, key, skip)
            if qualifies(*full):
                if pass_over == 0:
                    return (family, key, skip) + full + (True,)
                pass_over -= 1
                continue
        rank = (not (spread >= SPREAD and fc), max(gp / COND, gb / BUF_COND) if gp == gp and gb == gb else float("inf"))
        if best is None or rank < best[0]:
            best = (rank, skip)
    if best is None:
        raise SystemExit("%s %s: all %d candidates qualified and MOVED passes over every one of them" % (family, key, CANDIDATES))
    return (family, key, best[1]) + measure(family, key, best[1]) + (False,)


def render(rows):
    out = ['"""fd training-step sweep of tests/test_gpu_fd_train_shapes.py: the screened inputs.  WRITTEN BY',
           "tests/golden/make_fd_train_cases.py (the rule is in its docstring) — edit the generator, not this file.",
           "",
           "CASES[family][key] = (skip, prediction gap, loss gap, gradient gap, buffer gap, spread): at gpu_utils.sphere_patches(P, M,",
           "skip=skip) the CPU oracle's free f32 training step and its f64 step forced on that run's tables and spikes agree to COND on",
           "prediction and loss, to GRAD_COND on the gradients and to BUF_COND on the BatchNorm buffers, the prediction is spread out and",
           "no two rows of the snn_fc spikes are equal.",
           "UNSCREENED[family] = keys with no such candidate among those tried; their entry holds the best one.",
           '"""',
           "COND = %r" % COND, "GRAD_COND = %r" % GRAD_COND, "BUF_COND = %r" % BUF_COND, "SPREAD = %r" % SPREAD, "CAP = %d" % CAP,
           "WEIGHT_SEED = %d" % WEIGHT_SEED, "FC_THRESHOLD_SHIFT = %r" % FC_THRESHOLD_SHIFT, "",
           "CASES = {"]
    unscreened = {f: [] for f in FAMILIES}
    for family in FAMILIES:
        out.append('    "%s": {' % family)
        for f, key, skip, gp, gl, gg, gb, spread, fc, ok in rows:
            if f != family:
                continue
            note = ""
            if not ok:
                unscreened[family].append(key)
                note = "    # unscreened%s: %s" % ("" if fc else " (snn_fc rows repeat)", UNSCREENED_REASONS.get((family, key), "no candidate qualifies"))
            if key in MOVED[family]:
                note += "    # moved past %d qualifying candidate(s): %s" % MOVED[family][key]
            out.append("        %r: (%d, %r, %r, %r, %r, %r),%s" % (key, skip, gp, gl, gg, gb, spread, note))
        out.append("    },")
    out.append("}")
    out.append("UNSCREENED = {%s}" % ", ".join('"%s": %r' % (f, tuple(v)) for f, v in unscreened.items()))
    out.append("")
    return "\n".join(out), unscreened


def main():
    global CANDIDATES
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--candidates", type=int, default=CANDIDATES)
    ap.add_argument("--out", default=os.path.join(TESTS, "fd_train_cases.py"))
    args = ap.parse_args()
    CANDIDATES = args.candidates
    order = {j: i for i, j in enumerate((f, k) for f in FAMILIES for k in FAMILIES[f])}
    jobs = sorted(order, key=lambda j: -shape(*j)[0] * shape(*j)[1] ** 2)          # the long ones first
    rows = []
    with multiprocessing.get_context("spawn").Pool(args.jobs, initializer=_set_candidates, initargs=(CANDIDATES,)) as pool:
        for r in pool.imap_unordered(choose, jobs):
            print("%-2s %-9s skip %d  prediction %.2e  loss %.2e  grads %.2e  buffers %.2e  spread %.3f  fc %s%s" % (r[:9] + ("" if r[9] else "  UNSCREENED",)),
                  flush=True)
            rows.append(r)
    rows.sort(key=lambda r: order[(r[0], r[1])])
    text, unscreened = render(rows)
    with open(args.out, "w") as f:
        f.write(text)
    total = sum(len(v) for v in unscreened.values())
    print("unscreened: %d %s" % (total, unscreened))
    if total > CAP:
        raise SystemExit("%d cases have no qualifying candidate (cap %d in total): a finding about the oracle or the weights" % (total, CAP))


def _set_candidates(n):
    global CANDIDATES
    CANDIDATES = n


if __name__ == "__main__":
    main()
