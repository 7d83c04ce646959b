"""CPU checks of tests/patch_size_cases.py, the screened inputs of the patch-size sweep (tests/test_gpu_patch_sizes.py).

The table is written by tests/golden/make_patch_size_cases.py from the CPU oracle alone.  Here a fixed subset of its entries is
measured again — the sizes at which the kernels change path — and must give the recorded numbers and meet the screening rule; the
FULL table is reproduced by re-running the generator (a few minutes; `git diff` must then be empty), not by this test.
"""
import os
import sys

import pytest

import patch_size_cases as P

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_patch_size_cases as G  # noqa: E402

SUBSET = (1, 2, 3, 4, 11, 12, 17, 18, 23, 24, 48, 49, 64, 65, 128)


def _fn_mask(m):
    """include/sapcu.h sapcu_model_fused_blocks at the default k_values: bit l set iff min(k_l, m) is exactly 24 / 18 / 12."""
    return sum(1 << l for l, k in enumerate((24, 18, 12)) if min(k, m) == k)


@pytest.mark.parametrize("kind", ["fn", "fd"])
@pytest.mark.parametrize("m", SUBSET)
def test_recorded_numbers_are_reproduced_and_meet_the_rule(kind, m):
    skip, gap, spread = P.CASES[kind][m]
    assert (skip - G.SKIP0) % G.SKIP_STEP == 0 and 0 <= (skip - G.SKIP0) // G.SKIP_STEP < G.CANDIDATES
    got_gap, got_spread = G.measure(kind, m, skip)
    assert (got_gap, got_spread) == (gap, spread), (kind, m, got_gap, got_spread)
    if m not in [u[0] for u in P.UNSCREENED[kind]]:
        assert gap <= P.COND and spread >= P.SPREAD, (kind, m)
    p = P.patches(kind, m)
    assert tuple(p.shape) == (3, m, 3)
    assert P.patches(kind, m, 5)[:3].equal(p)                   # larger batches of a case start with the screened patches


def test_table_covers_every_patch_size():
    assert (P.COND, P.SPREAD, P.CAP) == (G.COND, G.SPREAD, G.CAP) == (3e-5, 2e-2, 4)
    for kind in ("fn", "fd"):
        assert sorted(P.CASES[kind]) == list(range(1, 129)), kind
        unscreened = dict(P.UNSCREENED[kind])
        for m, (skip, gap, spread) in P.CASES[kind].items():
            if m in unscreened:
                assert unscreened[m] == gap and not (gap <= P.COND and spread >= P.SPREAD), (kind, m)
            else:
                assert gap <= P.COND and spread >= P.SPREAD, (kind, m)


def test_unscreened_sizes_are_within_the_cap():
    for kind in ("fn", "fd"):
        assert len(P.UNSCREENED[kind]) <= P.CAP, (kind, P.UNSCREENED[kind])
        assert len(G.MOVED[kind]) <= 4, (kind, G.MOVED[kind])


def test_sweep_reaches_every_kernel_selection():
    """The fused-blocks masks the sweep expects take every value the rule of include/sapcu.h can give at the default configuration:
    fn 0b111 (m >= 24), 0b110 (18..23), 0b100 (12..17) and 0 (the five-kernel chain with kk = m); fd 1 (m <= 48) and 2."""
    fn = {}
    for m in P.CASES["fn"]:
        fn.setdefault(_fn_mask(m), []).append(m)
    assert fn == {0: list(range(1, 12)), 0b100: list(range(12, 18)), 0b110: list(range(18, 24)), 0b111: list(range(24, 129))}
    fd = {1 if m <= 48 else 2 for m in P.CASES["fd"]}
    assert fd == {1, 2}
