"""Writes tests/fn_train_cases.py: the inputs of the fn training-step sweep (tests/test_gpu_fn_train_shapes.py), chosen on the CPU
from the oracle alone.  A case is a batch gpu_utils.sphere_patches(B, M, skip=...) with ground-truth normals from a generator
seeded by the case, taken through oracle.train_path.fn_train_forward + angular_loss + backward.

Families (all weights testing.training_state_dict(shell, WEIGHT_SEED = 3)):

  "M"   B = 4 and M = 1..16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65; B = 3 and M = 100, 127, 128 — through the clamps
        k = min(k, M) at 12, 18 and 24, P = B M through 64 and 256, the edge rows P k through 1024.
  "B"   M = 12 (the reference's training patch; every block then has k = 12, so B 12 point rows and B 144 edge rows).  B_SIZES
        is derived below from the constants of csrc/train_ops.hip.
  "hp"  B = 4, M = 24 (fn-kclamp: M = 12), one case per fn row of the hyper-parameter matrix of make_fixtures.py that changes what
        training runs; the overrides are read from tests/golden/hparams.npz.

Rule per case, the one make_patch_size_cases.py applies: try skip = 300, 303, 306, ... for at most CANDIDATES and take the first
candidate at which the oracle in f32 and in f64 (the f64 run on the f32 run's kNN tables) agree on

  the normals    max |f32 - f64| <= COND = 3e-5 (make_fixtures.py HP_COND),
  the loss       |f32 - f64| <= COND,
  the gradients  max over the compared tensors of max|f32 - f64| / (max|f64| + 5e-5 peak) <= GRAD_COND = 2e-3, peak = the largest
                 |f64| gradient entry of the compared tensors (the rule of test_oracle_golden.check_fn_train_grads; a tenth of
                 the 2e-2 the GPU tests allow the device),

and at which the f32 normals are spread out: std(0).max() >= SPREAD = 2e-2.  The biases in front of a BatchNorm (cancelled())
are not compared: they cancel in the normalisation, their gradient is rounding noise several times the tensor's own scale in the
oracle itself; the op-level bounds cases of tests/test_gpu_bounds.py own grad_bias.

The normals are measured first, without autograd (for every candidate, spread over the worker pool); a candidate that fails
there cannot qualify and is not taken through the backward.  A case with no qualifying candidate goes to UNSCREENED with the
candidate whose normals agree best (among those that are spread out, if any) and that candidate's three gaps; more than CAP = 4
such cases in a family is an error here and in tests/test_fn_train_cases_host.py.  MOVED lists the cases whose first qualifying
candidates the GPU sweep set aside, with the layer-level diagnosis (a spike within rounding of its threshold); the generator
passes over that many qualifying candidates.

The neuron loops of the oracle run under torch.utils.checkpoint here (same operations, recomputed in the backward), which
keeps the largest case's f64 backward within memory.  Needs nothing but oracle/, sapcu_amd.testing, gpu_utils.sphere_patches
and tests/golden/hparams.npz; no GPU, no reference checkout.  Measured with one torch thread, so that the numbers do not depend
on the machine's core count:

    python tests/golden/make_fn_train_cases.py            # about 40 minutes on 8 cores
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
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

COND = 3e-5             # make_fixtures.py HP_COND: normals and loss
GRAD_COND = 2e-3        # a tenth of the 2e-2 of test_training_step_of_whole_fn_model_against_reference_run
FLOOR_REL = 5e-5        # check_fn_train_grads' noise floor relative to the largest gradient entry
SPREAD = 2e-2
SKIP0, SKIP_STEP, CANDIDATES = 300, 3, 32
CAP = 4
WEIGHT_SEED = 3

M_SIZES = tuple(range(1, 17)) + (17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 127, 128)

# "B" family.  At M = 12 every block has k = min(k, 12) = 12: a batch of B patches has P = 12 B point rows (conv1, fc1, q/k/v,
# out_proj, fc2, conv_final) and E = 144 B edge rows (fc_delta.., fc_gamma..).  The row boundaries of csrc/train_ops.hip:
#   LT_ROWS_PER_WG = 64     one LIF-backward workgroup, 16-row slabs          P: B = 5 (60) | 6 (72)
#   CR_ROWS = 256           one column-sum workgroup, 32-row stride           P: B = 21 (252) | 22 (264)
#   1024                    rows per weight-gradient slab (wgrad_slabs)       P: B = 85 (1020) | 86 (1032);  E: B = 7 (1008) | 8 (1152)
#   16 x 64 = 1024          lif_train_param_reduce_kernel walks the per-workgroup partials 16 at a time: the 17th workgroup
#                           starts at row 1025 — the same pairs as the slab boundary, B = 85 | 86 and 7 | 8
#   64 x 1024 = 65 536      wgrad_slabs' cap of 64 slabs                      E: B = 456 (65 664): SLAB_CAP_B, outside the table
# E = 144 B >= 432 at B >= 3, so E has no case below 64 or 256; those two are crossed by P.
# The slab cap: at B = 456 one oracle step keeps more than 35 GB in float64 (with the neuron loops checkpointed) and takes minutes
# on one thread, 32 candidates of it most of an hour, and the f32 oracle step every run of the GPU test would pay is tens of
# seconds.  So that batch is not screened and has no entry in CASES: tests/test_gpu_fn_train_shapes.py runs the whole step at
# SLAB_CAP_B under the protocol of an unscreened case without its printed oracle figures (tables, shapes, finiteness, unit normals,
# two runs bit for bit), and the weight gradient alone against exact integer sums at and above the cap.
B_POINT_BOUNDS = (64, 256, 1024, 16 * 64)
B_EDGE_BOUNDS = (1024, 16 * 64)
B_SLAB_CAP = 64 * 1024
B_M = 12


def _b_sizes():
    out = set()
    for bound in B_POINT_BOUNDS:
        out |= {bound // B_M, bound // B_M + 1}
    for bound in B_EDGE_BOUNDS:
        out |= {bound // (B_M * B_M), bound // (B_M * B_M) + 1}
    return tuple(sorted(out))


B_SIZES = _b_sizes()
assert B_SIZES == (5, 6, 7, 8, 21, 22, 85, 86)
SLAB_CAP_B = B_SLAB_CAP // (B_M * B_M) + 1          # 456 patches: 65 664 edge rows, the first batch of whole patches past 64 slabs
SLAB_CAP_SKIP = SKIP0

HP_ROWS = ("fn-ctor", "fn-h1", "fn-h128", "fn-mixed2", "fn-k1", "fn-kfull", "fn-kclamp", "fn-e32", "fn-e96", "fn-e160", "fn-T1")
HP_B, HP_M, HP_M_KCLAMP = 4, 24, 12

FAMILIES = {"M": M_SIZES, "B": B_SIZES, "hp": HP_ROWS}

# family -> {key: (qualifying candidates to pass over, "layer-level diagnosis of the device's miss at the candidate left")}
# Method (tests/fn_train_flips.py FAMILY KEY SKIP prints these figures; it extends test_training_hard_spike_flips_sit_on_their_
# thresholds to every layer): each conv + BatchNorm + neuron layer on the device against the oracle's, fed the oracle's input and in
# the free run; margin = min over the neuron steps of |m_t - theta_t| in float64.  Where no OUTPUT spike differs, the neuron loop's
# backward (upstream gradient 1) on each side's own BatchNorm output: an inner step's spike can flip and leave the last step's spike,
# hence the forward, as it was.
MOVED = {
    "M": {
        24: (1, "skip 303: normals 9.9e-06 and loss 3.6e-07 inside their bars, gradients 2.24 x their bar (encoder.snn_init.membrane_decay); no "
                "output spike differs in any layer; trans2.snn_gamma: 1 of 442 368 elements has an inner-step spike on its threshold (margin "
                "7.5e-07, input gradient off by 1.99), trans3.snn_delta2: 1 (margin 1.5e-07); the gradients downstream of trans2.fc_gamma2 agree to 1e-4"),
        100: (1, "skip 300: normals 3.0e-05, loss 3.2e-06, gradients 9.5 x their bar (encoder.trans1.w_ks.0.weight); trans3.snn_delta on the oracle's "
                 "input: 1 of 1 843 200 output spikes differs, margin 2.6e-07; in the free run it spreads to 15 / 87 spikes of snn_delta2 / snn_gamma"),
        127: (2, "skip 300: normals 5.6e-05, loss 2.1e-05, gradients 1.62 x their bar (encoder.conv1.1.bias); no output spike differs in any layer; "
                 "inner-step spikes on their thresholds in trans1.snn_delta (1 element, margin 3.4e-08, input gradient off by 25.5), trans1.snn_gamma "
                 "(2, 2.4e-07), trans2.snn1 (2, 1.4e-06, off by 10.6), trans3.snn_gamma (1, 7.1e-08, off by 6.35) and three more below 1.7e-06; "
                 "the gradients of block 3 and the decoder agree to 6e-4.  skip 303: normals 7.1e-05, loss 2.2e-05, gradients 1.16 x their bar "
                 "(encoder.trans1.w_vs.0.weight); no output spike differs; inner-step spikes in trans2.snn1 (1, margin 3.6e-06, off by 2.13), "
                 "trans3.snn_delta (1, 1.8e-07) and trans3.snn_delta2 (2, 3.6e-07, off by 2.61)"),
    },
    "B": {
        86: (2, "skip 306: normals 0.946, loss 0.009, gradients 177 x their bar; trans1.snn_gamma on the oracle's input: 1 of 1 585 152 output spikes "
                "differs, margin 1.5e-07; in the free run it reaches block 2 through fc1 (2 spikes) and spreads from there.  skip 378: normals "
                "4.7e-06, loss 0, gradients 2.16 x their bar (encoder.trans1.fc_delta.0.weight); trans3.snn_gamma on the oracle's input: 1 of "
                "6 340 608 output spikes differs, margin 2.0e-07 (2 spikes of snn_final follow); inner-step spikes on their thresholds in "
                "trans1.snn_delta (1 element, margin 4.1e-08, input gradient off by 2.07), trans2.snn_gamma (1, 1.1e-06, off by 21.6), "
                "trans3.snn_delta (1, 2.0e-07, off by 21.2) and three more below 1.5e-06"),
    },
    "hp": {
        "fn-mixed2": (1, "skip 300: normals 0.807, loss 0.334, gradients 148 x their bar; trans2.snn_k on the oracle's input: 1 of 24 576 output "
                         "spikes differs, margin 1.2e-07; in the free run it spreads through trans2.snn_gamma (215 spikes) into block 3 (23 593)"),
    },
}

_STATE = {}


def model_kw(family, key):
    """The constructor arguments of the case's model: FN_KW, for "hp" with the row's override from hparams.npz."""
    from conftest import FN_KW
    if family != "hp":
        return dict(FN_KW)
    if "hparams" not in _STATE:
        import gpu_utils as U
        g = np.load(os.path.join(HERE, "hparams.npz"))
        _STATE["hparams"] = {rid: U.hparam_row(g, rid)["kw"] for rid in HP_ROWS}
    return dict(_STATE["hparams"][key])


def shape(family, key):
    """(B, M) of the case."""
    if family == "M":
        return (3 if key >= 100 else 4), key
    if family == "B":                               # key SLAB_CAP_B included: same shape rule, no entry in the table
        return key, B_M
    return HP_B, (HP_M_KCLAMP if key == "fn-kclamp" else HP_M)


def state_dict(family, key):
    """(state dict, parameter names) of the case's model: training_state_dict(shell, WEIGHT_SEED)."""
    kw = model_kw(family, key)
    tag = repr(sorted(kw.items()))
    if tag not in _STATE:
        import sapcu_amd
        from sapcu_amd import testing as T
        shell = sapcu_amd.ImprovedSNNNormalEstimation(**kw)
        _STATE[tag] = (T.training_state_dict(shell.state_dict(), WEIGHT_SEED), [n for n, _ in shell.named_parameters()])
    return _STATE[tag]


def cancelled(sd):
    """The biases whose gradient is mathematically zero: every `X.0.bias` whose `X.1` is a BatchNorm, and the bias of every
    decoder Linear `mlp.i` followed by the BatchNorm `mlp.(i+1)`."""
    out = set()
    for n in sd:
        if not n.endswith(".bias"):
            continue
        stem = n[:-len(".bias")]
        head, _, last = stem.rpartition(".")
        if last.isdigit() and ("%s.%d.running_mean" % (head, int(last) + 1)) in sd and sd[stem + ".weight"].dim() >= 2:
            out.add(n)
    return out


def gt_normals(family, key, b):
    """Ground-truth unit normals [b, 3] (f32) of the case, from a generator seeded by the case."""
    rng = np.random.default_rng([17, zlib.crc32(("%s/%s" % (family, key)).encode())])
    v = rng.normal(size=(b, 3))
    return torch.from_numpy((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))


def knn_tables(pts, k_values):
    """The three in-patch neighbour tables [B, M, min(k, M)] (int64) of f32 points, as the oracle tests build them."""
    d = ((pts[:, :, None, :] - pts[:, None, :, :]) ** 2).sum(-1)
    return [d.topk(min(k, pts.shape[1]), dim=-1, largest=False)[1] for k in k_values]


def inputs(family, key, skip):
    """(points [B, M, 3] f32, gt [B, 3] f32) of the case at candidate `skip`."""
    import gpu_utils as U
    b, m = shape(family, key)
    return U.sphere_patches(b, m, skip=skip), gt_normals(family, key, b)


class _checkpointed_neurons(object):
    """The oracle's neuron loop under torch.utils.checkpoint while grad is on: same operations, its activations recomputed in
    the backward instead of kept (50 tensors of [rows, C] per layer otherwise)."""

    def __enter__(self):
        from torch.utils.checkpoint import checkpoint
        from oracle import train_path as TP
        self.TP, self.orig = TP, TP.lif_selfloop_train

        def lif(*a):
            if not torch.is_grad_enabled():
                return self.orig(*a)
            return checkpoint(self.orig, *a, use_reentrant=False)
        TP.lif_selfloop_train = lif
        return self

    def __exit__(self, *exc):
        self.TP.lif_selfloop_train = self.orig
        return False


def oracle_step(family, key, pts, gt, knn, dtype=torch.float32, grads=True):
    """One training step of the oracle in `dtype` on the given tables: (normals, loss, {name: gradient}) as CPU tensors of
    that dtype; without `grads` the forward alone, (normals, loss, None)."""
    from oracle import train_path as TP
    kw = model_kw(family, key)
    sd, names = state_dict(family, key)
    p = {n: sd[n].to(dtype).clone().requires_grad_(grads) for n in names}
    with torch.set_grad_enabled(grads), _checkpointed_neurons():
        normals = TP.fn_train_forward(p, pts.to(dtype), knn, kw["time_steps_enc"], kw["num_heads"])
        loss = TP.angular_loss(normals, gt.to(dtype))
        if grads:
            loss.backward()
    g = {n: (p[n].grad if p[n].grad is not None else torch.zeros_like(p[n])).detach() for n in names} if grads else None
    return normals.detach(), loss.detach(), g


def grad_ratio(got, ref, skip_names):
    """check_fn_train_grads' figure over whole tensors: max over the compared tensors of max|got - ref| / (max|ref| + FLOOR_REL
    peak).  Returns (worst ratio, its tensor's name, peak)."""
    names = [n for n in ref if n not in skip_names]
    peak = max(float(ref[n].abs().max()) for n in names)
    worst, where = 0.0, ""
    for n in names:
        r = float((got[n].double().cpu() - ref[n].double()).abs().max()) / (float(ref[n].abs().max()) + FLOOR_REL * peak)
        if not r <= worst:                      # a NaN lands here too
            worst, where = r, n
    return worst, where, peak


def measure_normals(family, key, skip):
    """(gap of the normals, spread) at a candidate: the forward alone, f32 and f64."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        pts, gt = inputs(family, key, skip)
        knn = knn_tables(pts, model_kw(family, key)["k_values"])
        n32, _, _ = oracle_step(family, key, pts, gt, knn, torch.float32, grads=False)
        n64, _, _ = oracle_step(family, key, pts, gt, knn, torch.float64, grads=False)
        return float((n64 - n32.double()).abs().max()), float(n32.std(0).max())
    finally:
        torch.set_num_threads(threads)


def measure(family, key, skip):
    """(gap of the normals, gap of the loss, gap of the gradients, spread) at a candidate: the whole step, f32 and f64."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        pts, gt = inputs(family, key, skip)
        knn = knn_tables(pts, model_kw(family, key)["k_values"])
        n32, l32, g32 = oracle_step(family, key, pts, gt, knn, torch.float32)
        n64, l64, g64 = oracle_step(family, key, pts, gt, knn, torch.float64)
        ratio = grad_ratio(g32, g64, cancelled(state_dict(family, key)[0]))[0]
        return float((n64 - n32.double()).abs().max()), abs(float(l64) - float(l32)), ratio, float(n32.std(0).max())
    finally:
        torch.set_num_threads(threads)


def qualifies(gn, gl, gg, spread):
    return gn <= COND and gl <= COND and gg <= GRAD_COND and spread >= SPREAD


def _normals_job(job):
    family, key, skip = job
    return job, measure_normals(family, key, skip)


def choose(job, normals=None):
    """(family, key) -> (family, key, skip, normals gap, loss gap, gradient gap, spread, screened).  normals: {(family, key,
    skip): measure_normals(...)} measured ahead (main() spreads them over the pool); what is missing is measured here."""
    family, key = job
    pass_over = MOVED[family].get(key, (0,))[0]
    best = None
    for c in range(CANDIDATES):
        skip = SKIP0 + SKIP_STEP * c
        gn, spread = (normals or {}).get((family, key, skip)) or measure_normals(family, key, skip)
        if gn <= COND and spread >= SPREAD:
            full = measure(family, key, skip)
            if qualifies(*full):
                if pass_over == 0:
                    return (family, key, skip) + full + (True,)
                pass_over -= 1
                continue
        rank = (spread < SPREAD, gn)
        if best is None or rank < best[0]:
            best = (rank, skip)
    if best is None:
        raise SystemExit("%s %s: all %d candidates qualified and MOVED passes over every one of them" % (family, key, CANDIDATES))
    return (family, key, best[1]) + measure(family, key, best[1]) + (False,)


def _choose_job(args):
    return choose(*args)


def render(rows):
    out = ['"""fn training-step sweep of tests/test_gpu_fn_train_shapes.py: the screened inputs.  WRITTEN BY',
           "tests/golden/make_fn_train_cases.py (the rule is in its docstring) — edit the generator, not this file.",
           "",
           "CASES[family][key] = (skip, normals gap, loss gap, gradient gap, spread): at gpu_utils.sphere_patches(B, M, skip=skip) the CPU",
           "oracle's training step in f32 and in f64 agree to COND on normals and loss and to GRAD_COND on the gradients, and the normals",
           "are spread out.  UNSCREENED[family] = keys with no such candidate among those tried; their entry holds the best one.",
           '"""',
           "COND = %r" % COND, "GRAD_COND = %r" % GRAD_COND, "SPREAD = %r" % SPREAD, "CAP = %d" % CAP, "",
           "CASES = {"]
    unscreened = {f: [] for f in FAMILIES}
    for family in FAMILIES:
        out.append('    "%s": {' % family)
        for f, key, skip, gn, gl, gg, spread, ok in rows:
            if f != family:
                continue
            note = ""
            if not ok:
                unscreened[family].append(key)
                note = "    # unscreened: no candidate qualifies"
            if key in MOVED[family]:
                note += "    # moved past %d qualifying candidate(s): %s" % MOVED[family][key]
            out.append("        %r: (%d, %r, %r, %r, %r),%s" % (key, skip, gn, gl, gg, spread, note))
        out.append("    },")
    out.append("}")
    out.append("UNSCREENED = {%s}" % ", ".join('"%s": %r' % (f, tuple(v)) for f, v in unscreened.items()))
    out.append("")
    return "\n".join(out), unscreened


def main():
    global CANDIDATES
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--candidates", type=int, default=CANDIDATES, help="64 is the one thing to try when a family passes its cap")
    ap.add_argument("--out", default=os.path.join(TESTS, "fn_train_cases.py"))
    args = ap.parse_args()
    CANDIDATES = args.candidates
    order = {j: i for i, j in enumerate((f, k) for f in FAMILIES for k in FAMILIES[f])}
    jobs = sorted(order, key=lambda j: -shape(*j)[0] * shape(*j)[1] ** 2)          # the long ones first
    with multiprocessing.get_context("spawn").Pool(args.jobs, initializer=_set_candidates, initargs=(CANDIDATES,)) as pool:
        # every candidate's forward pair first, one candidate per task: a batch with no qualifying candidate (the largest ones)
        # would otherwise hold one worker for all of its candidates
        pairs = [(f, k, SKIP0 + SKIP_STEP * c) for f, k in jobs for c in range(CANDIDATES)]
        normals = {}
        for job, r in pool.imap_unordered(_normals_job, pairs):
            normals[job] = r
            if len(normals) % 100 == 0:
                print("forward pairs: %d of %d" % (len(normals), len(pairs)), flush=True)
        rows = []
        for r in pool.imap_unordered(_choose_job, [(j, {k: v for k, v in normals.items() if k[:2] == j}) for j in jobs]):
            print("%-2s %-9s skip %d  normals %.2e  loss %.2e  grads %.2e  spread %.3f%s" % (r[:7] + ("" if r[7] else "  UNSCREENED",)), flush=True)
            rows.append(r)
    rows.sort(key=lambda r: order[(r[0], r[1])])
    text, unscreened = render(rows)
    with open(args.out, "w") as f:
        f.write(text)
    for family, v in unscreened.items():
        print("%s: %d unscreened %s" % (family, len(v), v))
    for family, v in unscreened.items():
        if len(v) > CAP:
            raise SystemExit("%s: %d cases have no qualifying candidate (cap %d): a finding about the oracle or the weights" % (family, len(v), CAP))


def _set_candidates(n):
    global CANDIDATES
    CANDIDATES = n


if __name__ == "__main__":
    main()
