"""CPU checks of tests/fn_train_cases.py, the screened inputs of the fn training-step sweep (tests/test_gpu_fn_train_shapes.py).

The table is written by tests/golden/make_fn_train_cases.py from the CPU oracle alone.  Here a handful of its entries — small
ones, one per family and the k clamps — are measured again and must give the recorded numbers; every family must be complete,
within its cap of unscreened cases, and every screened entry's recorded gaps within the rule.  The FULL table is reproduced by
re-running the generator (`git diff` must then be empty), not by this test.
"""
import os
import sys

import pytest

import fn_train_cases as C

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_fn_train_cases as G  # noqa: E402

SUBSET = (("M", 1), ("M", 2), ("M", 12), ("B", 5), ("hp", "fn-k1"), ("hp", "fn-T1"))


def _within_rule(entry):
    skip, gn, gl, gg, spread = entry
    return gn <= C.COND and gl <= C.COND and gg <= C.GRAD_COND and spread >= C.SPREAD


@pytest.mark.parametrize("family,key", SUBSET)
def test_recorded_numbers_are_reproduced(family, key):
    entry = C.CASES[family][key]
    skip = entry[0]
    assert (skip - G.SKIP0) % G.SKIP_STEP == 0 and 0 <= (skip - G.SKIP0) // G.SKIP_STEP < 64
    assert G.measure(family, key, skip) == tuple(entry[1:]), (family, key)
    pts, gt = G.inputs(family, key, skip)
    assert tuple(pts.shape) == G.shape(family, key) + (3,) and tuple(gt.shape) == (pts.shape[0], 3)
    assert float((gt.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    assert G.inputs(family, key, skip)[1].equal(gt)                      # the ground truth is seeded by the case alone


def test_every_family_is_complete_and_every_screened_entry_is_within_the_rule():
    assert (C.COND, C.GRAD_COND, C.SPREAD, C.CAP) == (G.COND, G.GRAD_COND, G.SPREAD, G.CAP) == (3e-5, 2e-3, 2e-2, 4)
    assert set(C.CASES) == set(C.UNSCREENED) == set(G.FAMILIES) == {"M", "B", "hp"}
    assert list(C.CASES["M"]) == list(range(1, 17)) + [17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 127, 128]
    assert list(C.CASES["B"]) == list(G.B_SIZES)
    assert list(C.CASES["hp"]) == ["fn-ctor", "fn-h1", "fn-h128", "fn-mixed2", "fn-k1", "fn-kfull", "fn-kclamp", "fn-e32", "fn-e96", "fn-e160",
                                   "fn-T1"]
    for family, cases in C.CASES.items():
        assert set(C.UNSCREENED[family]) <= set(cases), family
        for key, entry in cases.items():
            assert _within_rule(entry) == (key not in C.UNSCREENED[family]), (family, key, entry)
            assert G.shape(family, key)[0] >= 3, (family, key)          # a BatchNorm over two rows gives +-1 whatever its input


def test_unscreened_and_moved_cases_are_within_the_cap():
    for family in C.CASES:
        assert len(C.UNSCREENED[family]) <= C.CAP, (family, C.UNSCREENED[family])
        assert len(G.MOVED[family]) <= 4 and set(G.MOVED[family]) <= set(C.CASES[family]), (family, G.MOVED[family])
        for key, (passed_over, diagnosis) in G.MOVED[family].items():
            assert passed_over >= 1 and diagnosis, (family, key)


def test_batch_sizes_sit_on_both_sides_of_every_row_boundary():
    """The "B" family against the derivation in the generator: 12 B point rows and 144 B edge rows one below and one above each
    boundary of csrc/train_ops.hip; the weight-gradient slab cap (65 536 edge rows) is crossed by SLAB_CAP_B = 456 patches, a whole
    step the GPU sweep runs without an oracle, outside the table (the generator says why)."""
    m = G.B_M
    for bound in G.B_POINT_BOUNDS:
        rows = sorted(b * m for b in G.B_SIZES)
        assert max(r for r in rows if r <= bound) > bound - m and min(r for r in rows if r > bound) <= bound + m, bound
    for bound in G.B_EDGE_BOUNDS:
        rows = sorted(b * m * m for b in G.B_SIZES)
        assert max(r for r in rows if r <= bound) > bound - m * m and min(r for r in rows if r > bound) <= bound + m * m, bound
    assert max(G.B_SIZES) * m * m < G.B_SLAB_CAP
    assert G.SLAB_CAP_B == 456 and (G.SLAB_CAP_B - 1) * m * m <= G.B_SLAB_CAP < G.SLAB_CAP_B * m * m and G.shape("B", G.SLAB_CAP_B) == (456, 12)


def test_hyper_parameter_rows_change_what_training_runs():
    """Each "hp" case differs from the default configuration in an argument of fn_train_forward or in a weight's shape, and the
    sweep's M reaches every clamp k = min(k, M) of the default k_values."""
    from conftest import FN_KW
    seen = set()
    for rid in C.CASES["hp"]:
        kw = G.model_kw("hp", rid)
        diff = {k for k in ("k_values", "emb_dims", "time_steps_enc", "num_heads") if kw[k] != FN_KW[k]}
        assert diff, rid
        seen |= diff
        b, mm = G.shape("hp", rid)
        assert b % 2 == 0                                                # the [B/2, 2, M, 3] form of the module check
    assert seen == {"k_values", "emb_dims", "time_steps_enc", "num_heads"}
    assert G.model_kw("hp", "fn-ctor")["time_steps_enc"] == 8 and all(k > G.HP_M_KCLAMP for k in G.model_kw("hp", "fn-kclamp")["k_values"][:2])
    assert all(k >= G.HP_M for k in G.model_kw("hp", "fn-kfull")["k_values"])
    clamps = {tuple(min(k, m) for k in FN_KW["k_values"]) for m in C.CASES["M"]}
    assert {(24, 18, 12), (23, 18, 12), (17, 17, 12), (11, 11, 11)} <= clamps
