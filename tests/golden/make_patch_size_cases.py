"""Writes tests/patch_size_cases.py: for fn and fd at the default configuration and every patch size m = 1..128, the `skip` handed to
gpu_utils.sphere_patches(3, m, skip=...) by tests/test_gpu_patch_sizes.py, chosen on the CPU from the oracle alone.

Rule per (kind, m), the one make_fixtures.py applies to the hyper-parameter rows (HP_COND and the spread floor of _hp_row): try
skip = 300, 303, 306, ... for at most 32 candidates and take the first one that is

  well conditioned:  |oracle f32 - oracle f64| <= COND = 3e-5 (the f64 run on the f32 run's neighbour tables: fn `knn_idx`, fd
                     `encoder.knn1..3` through force_idx) — rounding noise a third of the GPU tests' 1e-4, a property of the
                     function at these inputs measured on the reference arithmetic alone;
  spread out:        fn ref.std(0).max() >= SPREAD = 2e-2, fd d.std() >= 2e-2 — twice the floor the GPU tests assert.

A size with no qualifying candidate goes to UNSCREENED with the best gap found (among the candidates that are spread out, if any);
more than CAP = 4 such sizes per net is an error here and in tests/test_patch_sizes_host.py.  MOVED below lists the sizes whose
first qualifying candidates the GPU sweep set aside (a spike within rounding of its threshold under the split-f16 arithmetic,
settled with a SAPCU_GEMM=f32 handle); the generator skips that many qualifying candidates there and writes the note.

Needs nothing but oracle/, sapcu_amd.testing and the committed BatchNorm calibration; no GPU, no reference checkout.  The numbers
are measured with one torch thread so that they do not depend on the machine's core count:

    python tests/golden/make_patch_size_cases.py            # all 256 entries, a few minutes on 8 cores
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

COND = 3e-5             # make_fixtures.py HP_COND
SPREAD = 2e-2           # make_fixtures.py _hp_row: twice the 1e-2 the GPU tests assert
SKIP0, SKIP_STEP, CANDIDATES = 300, 3, 32
CAP = 4
PATCHES = 3
SIZES = range(1, 129)

# kind -> {m: (qualifying candidates to pass over, |default handle - oracle|, |SAPCU_GEMM=f32 handle - oracle|) at the skip left}
MOVED = {"fn": {}, "fd": {}}

_STATE = {}


def state_dicts(kind):
    """(f32, f64) conditioned state dicts of the default configuration: seed 0 + the committed BatchNorm calibration, what the
    `weights` fixture of tests/conftest.py builds."""
    if kind not in _STATE:
        import sapcu_amd
        from conftest import FD_KW, FN_KW
        from sapcu_amd import testing as T
        cls, kw = (sapcu_amd.ImprovedSNNNormalEstimation, FN_KW) if kind == "fn" else (sapcu_amd.EnhancedSNNDistanceEstimation, FD_KW)
        bn = dict(np.load(os.path.join(HERE, "bn_calib_%s.npz" % kind)))
        sd = T.conditioned_state_dict(cls(**kw).state_dict(), 0, bn_stats=bn)
        _STATE[kind] = (sd, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})
    return _STATE[kind]


def measure(kind, m, skip):
    """(gap, spread) of the oracle on sphere_patches(3, m, skip=skip): max |f32 - f64| with the f32 run's neighbours, and the spread
    of the f32 outputs over the three patches."""
    import gpu_utils as U
    from oracle import snn_path as O
    sd, sd64 = state_dicts(kind)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        p = U.sphere_patches(PATCHES, m, skip=skip)
        taps = {}
        with torch.no_grad():
            if kind == "fn":
                ref = O.fn_forward(sd, p, U.FN_HP, taps=taps)
                ref64 = O.fn_forward(sd64, p.double(), U.FN_HP, knn_idx=taps["knn_idx"])
                spread = float(ref.std(0).max())
            else:
                ref = O.fd_forward(sd, p, U.FD_HP, taps=taps)
                ref64 = O.fd_forward(sd64, p.double(), U.FD_HP, force_idx=[taps["encoder.knn%d" % i] for i in (1, 2, 3)])
                spread = float(ref.std())
        return float((ref64 - ref.double()).abs().max()), spread
    finally:
        torch.set_num_threads(threads)


def qualifies(gap, spread):
    return gap <= COND and spread >= SPREAD


def choose(job):
    """(kind, m) -> (kind, m, skip, gap, spread, screened)."""
    kind, m = job
    pass_over = MOVED[kind].get(m, (0,))[0]
    best = None
    for c in range(CANDIDATES):
        skip = SKIP0 + SKIP_STEP * c
        gap, spread = measure(kind, m, skip)
        if qualifies(gap, spread):
            if pass_over == 0:
                return kind, m, skip, gap, spread, True
            pass_over -= 1
            continue
        key = (spread < SPREAD, gap)
        if best is None or key < best[0]:
            best = (key, skip, gap, spread)
    return kind, m, best[1], best[2], best[3], False


def render(rows):
    out = ['"""Patch-size sweep of tests/test_gpu_patch_sizes.py: the screened inputs.  WRITTEN BY tests/golden/make_patch_size_cases.py',
           "(the rule is in its docstring) — edit the generator, not this file.",
           "",
           "CASES[kind][m] = (skip, gap, spread): sphere_patches(3, m, skip=skip) is the first candidate at which the CPU oracle is well",
           "conditioned (gap = |oracle f32 - oracle f64| <= COND) and spread out (spread >= SPREAD) at the default configuration.",
           "UNSCREENED[kind] = ((m, best gap), ...): sizes with no such candidate among the 32 tried; their entry holds the best one.",
           '"""',
           "COND = %r" % COND, "SPREAD = %r" % SPREAD, "CAP = %d" % CAP, "",
           "CASES = {"]
    unscreened = {"fn": [], "fd": []}
    for kind in ("fn", "fd"):
        out.append('    "%s": {' % kind)
        for k, m, skip, gap, spread, ok in rows:
            if k != kind:
                continue
            note = ""
            if not ok:
                unscreened[kind].append((m, gap))
                note = "    # unscreened: no candidate qualifies"
            if m in MOVED[kind]:
                n, e_def, e_f32 = MOVED[kind][m]
                note += "    # moved past %d qualifying candidate(s): there |default - oracle| %.3g, |SAPCU_GEMM=f32 - oracle| %.3g" % (n, e_def, e_f32)
            out.append("        %d: (%d, %r, %r),%s" % (m, skip, gap, spread, note))
        out.append("    },")
    out.append("}")
    out.append("UNSCREENED = {%s}" % ", ".join('"%s": %r' % (k, tuple(v)) for k, v in unscreened.items()))
    out += ["", "",
            "def patches(kind, m, b=3):",
            '    """The case\'s patches [b, m, 3] (CPU, f32): the first three are the screened ones."""',
            "    import gpu_utils as U",
            "    return U.sphere_patches(b, m, skip=CASES[kind][m][0])",
            ""]
    return "\n".join(out), unscreened


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(TESTS, "patch_size_cases.py"))
    args = ap.parse_args()
    jobs = [(kind, m) for kind in ("fn", "fd") for m in sorted(SIZES, reverse=True)]
    with multiprocessing.get_context("spawn").Pool(args.jobs) as pool:
        rows = []
        for r in pool.imap_unordered(choose, jobs):
            print("%s m=%-3d skip %d  gap %.2e  spread %.3f%s" % (r[0], r[1], r[2], r[3], r[4], "" if r[5] else "  UNSCREENED"), flush=True)
            rows.append(r)
    rows.sort(key=lambda r: (r[0] != "fn", r[1]))
    text, unscreened = render(rows)
    with open(args.out, "w") as f:
        f.write(text)
    for kind, v in unscreened.items():
        print("%s: %d unscreened %s" % (kind, len(v), v))
        if len(v) > CAP:
            raise SystemExit("%s: %d sizes have no qualifying candidate (cap %d): a finding about the oracle or the weights" % (kind, len(v), CAP))


if __name__ == "__main__":
    main()
