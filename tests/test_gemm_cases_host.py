"""The conditions the GEMM epilogue sweep rests on, checked from the operands alone (no GPU): the two operand families are exact in
f32 in any summation order, family S really separates the split-f16 kernels' three-term sum from the true product, the scaled
pre-activations are not saturated — and the pair table of tests/gemm_cases.py is what the launchers' sources serve."""
import os
import re

import numpy as np
import pytest

import gemm_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c-users-sayakdutta-self-supervised-arbitrary-scale-point-cloud-upsampling-via-snn_amd", "csrc")


def _exact_f32(x):
    return np.array_equal(x.astype(np.float32).astype(np.float64), x)


@pytest.mark.parametrize("k", GC.ALL_KS)
@pytest.mark.parametrize("family", ["I", "S"])
def test_family_is_exact_in_any_order(family, k):
    a, w, acc = GC.operands(family, k)
    s = GC.w_scale(k)
    ah, al = (p.astype(np.float64) for p in GC.split16(a))
    wh, wl = (p.astype(np.float64) for p in GC.split16(w * np.float32(16.0)))
    # the split is exact: two halves carry the operand
    assert np.array_equal(ah + al, a.astype(np.float64)) and np.array_equal(wh + wl, 16.0 * w.astype(np.float64))
    assert np.abs(ah).max() <= 2 and np.abs(al).max() <= 2.0 ** -12 and np.abs(wh).max() <= 32 * s
    # condition 1, the term quantum: every term of the three passes is a multiple of q (on the accumulator's x16 scale) ...
    qa, qw = (1.0, 16.0 * s) if family == "I" else (2.0 ** -12, 16.0 * s * 2.0 ** -12)
    q = (1.0 if family == "I" else 2.0 ** -12) * 16.0 * s
    for plane, quantum in ((ah, 1.0), (al, qa), (wh, 16.0 * s), (wl, qw)):
        assert np.array_equal(np.round(plane / quantum) * quantum, plane)
    # ... condition 2: and the absolute values of the terms add up to less than 2^24 quanta, so every partial sum in every order is
    # an integer number of quanta below 2^24: exact in f32
    total = np.abs(ah) @ np.abs(wh).T + np.abs(ah) @ np.abs(wl).T + np.abs(al) @ np.abs(wh).T
    assert total.max() / q < 2 ** 24, total.max() / q
    # the exact-f32 kernel's own sum (family I): products a w are multiples of s
    if family == "I":
        assert (np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)).T).max() / s < 2 ** 24
        assert np.array_equal(a.astype(np.float64) @ w.astype(np.float64).T, acc)
    # the epilogue's additions stay exact: acc / 16 (+ bias) (+ residual) are f32 values
    assert _exact_f32(acc) and _exact_f32(GC.argument(family, k, False)) and _exact_f32(GC.argument(family, k, True))


@pytest.mark.parametrize("k", GC.ALL_KS)
def test_family_s_separates_the_three_term_sum_from_the_product(k):
    a, w, acc = GC.operands("S", k)
    lo_share = np.mean([np.mean(GC.split16(a)[1] != 0), np.mean(GC.split16(w * np.float32(16.0))[1] != 0)])
    assert lo_share >= 0.5, lo_share                       # 4/5 of the m are non-zero, 2/3 of their j
    true = a.astype(np.float64) @ w.astype(np.float64).T
    differs = np.mean(true != acc)
    assert differs >= 0.8, differs
    # and family I does not: its lo planes are empty
    a, w, _ = GC.operands("I", k)
    assert not GC.split16(a)[1].any() and not GC.split16(w * np.float32(16.0))[1].any()


@pytest.mark.parametrize("k", GC.ALL_KS)
@pytest.mark.parametrize("family", ["I", "S"])
def test_scaled_pre_activations_are_not_saturated(family, k):
    for resid in (False, True):
        x = GC.argument(family, k, resid)
        assert np.mean(np.abs(x) < 4.0) >= 0.5, (resid, np.mean(np.abs(x) < 4.0))
        assert np.std(x) >= 1.0, np.std(x)                 # ... and not collapsed onto the bias either


def test_shapes_and_counts():
    assert len(GC.TABLE) == 29 == len(set(GC.TABLE)) and len(GC.REFUSED) == 5 * 9 - 29
    for launcher, epi in GC.TABLE:
        shapes = GC.star(launcher, epi)
        for s in shapes:
            assert s.r <= GC.R_MAX and s.n <= GC.N_MAX and s.k in GC.KS[launcher], s
            assert GC.accepts(launcher, epi, s), (launcher, epi, s)
            for f in GC.families(launcher):
                p = GC.partner(launcher, epi, f, s)
                assert p is None or (p != launcher and GC.accepts(p, epi, s))
            for lay in GC.layouts(launcher, epi, s):
                assert lay.lda >= s.k and lay.lda % 8 == 0 and lay.ldc >= s.n and lay.ldr >= s.n, lay
                assert lay.name in ("compact", "split32") or lay.ldr != lay.ldc, lay
                if launcher == "bt":
                    assert lay.ldc % 4 == 0 and not lay.misalign
        own, others = GC.expected_runs(launcher, epi)
        assert own >= 2 * len(shapes) and others <= own
        if epi in GC.MAXES and launcher != "shortk":
            for m in GC.MAX_MS:
                rs = [s.r for s in shapes if s.max_m == m]
                assert any(r % m == 0 for r in rs) and (m == 1 or any(r % m for r in rs)), m
    # every launcher is compared with another one on every epilogue it shares, from one side at least
    for epi in GC.EPI:
        serving = [l for l in GC.LAUNCHERS if (l, epi) in GC.TABLE]
        linked = {frozenset((l, GC.partner(l, epi, f, s))) for l in serving for s in GC.star(l, epi) for f in GC.families(l)
                  if GC.partner(l, epi, f, s)}
        reach = {serving[0]}
        for _ in serving:
            reach |= {x for pair in linked if pair & reach for x in pair}
        assert reach == set(serving), (epi, reach)
    tab = GC.edge_rows()
    assert tab[:, 0].max() < GC.Q_ROWS and tab[:, 1].max() < GC.Q_ROWS and tab.min() >= 0


# ------------------------------------------------------------------------------------------------ the coverage gate
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(text, head):
    """The text of the function whose definition starts with `head`, up to the closing brace in column 0."""
    start = text.index(head)
    return text[start:text.index("\n}\n", start)]


def _switch_arms(text, head):
    return set(re.findall(r"case EPI_(\w+):", _body(text, head)))


def _predicate_epilogues(text, head):
    return set(re.findall(r"EPI_(\w+)", _body(text, head)))


def served_pairs():
    """(launcher, epilogue) pairs as the sources state them: the `case EPI_...` arms of the three dispatch switches that take every
    epilogue value (exact-f32, f32-A split-f16, ring — whose default arm is the one epilogue its predicate leaves) and the epilogue
    lines of gemm_sf16_bt_ok, gemm_shortk_ok and gemm_sf16_ring_accepts."""
    f32 = _switch_arms(_source(GC.SOURCES["f32"]), "int launch_gemm(const GemmArgs& g")
    sf16 = _switch_arms(_source(GC.SOURCES["sf16"]), "int launch_gemm_sf16(const GemmArgs& g")
    ring_text = _source(GC.SOURCES["ring"])
    ring = _predicate_epilogues(ring_text, "bool gemm_sf16_ring_accepts(const GemmArgs& g")
    ring_arms = _switch_arms(ring_text, "int launch_gemm_sf16_ring(const GemmArgs& g")
    assert ring_arms <= ring and len(ring - ring_arms) == 1, (ring, ring_arms)          # the default arm
    bt_text = _source(GC.SOURCES["bt"])
    bt = _predicate_epilogues(bt_text, "bool gemm_sf16_bt_ok(const GemmArgs& g")
    bt_arms = _switch_arms(bt_text, "int launch_gemm_sf16_bt(const GemmArgs& g")
    assert bt_arms <= bt and len(bt - bt_arms) == 1, (bt, bt_arms)
    shortk = _predicate_epilogues(_source(GC.SOURCES["shortk"]), "bool gemm_shortk_ok(const GemmArgs& g")
    found = {"f32": f32, "sf16": sf16, "ring": ring, "bt": bt, "shortk": shortk}
    return {(l, e) for l, es in found.items() for e in es}


def gate(table):
    served = served_pairs()
    missing, unserved = sorted(served - set(table)), sorted(set(table) - served)
    assert not missing, "served by a launcher but not in the case table: %s" % missing
    assert not unserved, "in the case table but served nowhere: %s" % unserved


def test_every_served_pair_has_a_row_in_the_table():
    assert {e for _, e in served_pairs()} == set(GC.EPI)
    gate(GC.TABLE)


def test_the_gate_notices_a_missing_and_a_spare_row():
    for i in range(len(GC.TABLE)):
        with pytest.raises(AssertionError, match="not in the case table"):
            gate(GC.TABLE[:i] + GC.TABLE[i + 1:])
    with pytest.raises(AssertionError, match="served nowhere"):
        gate(GC.TABLE + [("shortk", "GELU")])
