"""CPU checks of tests/fd_train_cases.py, the screened inputs of the fd training-step sweep (tests/test_gpu_fd_train_shapes.py).

The table is written by tests/golden/make_fd_train_cases.py from the CPU oracle alone.  Here a handful of its entries — small
ones, one per family and the clamps — are measured again and must still qualify with gaps like the recorded ones (the digits of
rounding noise depend on the CPU); every family must be complete, the
unscreened keys within their cap IN TOTAL, and every screened entry's recorded gaps within the rule.  The FULL table is reproduced
by re-running the generator (`git diff` must then be empty), not by this test.
"""
import os
import sys

import pytest
import torch

import fd_train_cases as C

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_fd_train_cases as G  # noqa: E402

SUBSET = (("M", 1), ("M", 2), ("M", 11), ("P", 5), ("P", 6), ("hp", "fd-k1"), ("hp", "fd-kclamp"), ("hp", "fd-T1"))


def _within_rule(entry):
    skip, gp, gl, gg, gb, spread = entry
    return gp <= C.COND and gl <= C.COND and gg <= C.GRAD_COND and gb <= C.BUF_COND and spread >= C.SPREAD


@pytest.mark.parametrize("family,key", SUBSET)
def test_recorded_candidates_qualify_again(family, key):
    entry = C.CASES[family][key]
    skip = entry[0]
    assert (skip - G.SKIP0) % G.SKIP_STEP == 0 and 0 <= (skip - G.SKIP0) // G.SKIP_STEP < G.CANDIDATES
    got = G.measure(family, key, skip)
    # the gaps are rounding noise: another CPU's torch kernels give other digits (the recorded ones are reproduced exactly only by
    # re-running the generator on the machine that wrote the table).  What must hold anywhere: the candidate still qualifies, its
    # gaps are those of the same well-conditioned step (within a factor 16 and COND / 16 of the recorded ones) and the spread, a
    # forward value, is the recorded one to COND.
    assert G.qualifies(*got), (family, key, got)
    for new, old, cond in zip(got[:4], entry[1:5], (C.COND, C.COND, C.GRAD_COND, C.BUF_COND)):
        assert new <= 16 * old + cond / 16, (family, key, got, entry)
    assert abs(got[4] - entry[5]) <= C.COND and got[5] is True, (family, key, got)
    pts, gt = G.inputs(family, key, skip)
    assert tuple(pts.shape) == G.shape(family, key) + (3,) and tuple(gt.shape) == (pts.shape[0],)
    assert G.GT_RANGE[0] <= float(gt.min()) and float(gt.max()) <= G.GT_RANGE[1]
    assert G.inputs(family, key, skip)[1].equal(gt)                      # the ground truth is seeded by the case alone


def test_every_family_is_complete_and_every_screened_entry_is_within_the_rule():
    assert (C.COND, C.GRAD_COND, C.BUF_COND, C.SPREAD, C.CAP) == (G.COND, G.GRAD_COND, G.BUF_COND, G.SPREAD, G.CAP) == (3e-5, 2e-3, 1e-6, 2e-2, 4)
    assert (C.WEIGHT_SEED, C.FC_THRESHOLD_SHIFT) == (G.WEIGHT_SEED, G.FC_THRESHOLD_SHIFT)
    assert set(C.CASES) == set(C.UNSCREENED) == set(G.FAMILIES) == {"M", "P", "hp"}
    assert list(C.CASES["M"]) == [1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 15, 16, 17, 19, 20, 21, 31, 32, 33, 39, 40, 41, 47, 48, 49, 63, 64, 65,
                                  100, 127, 128]
    assert list(C.CASES["P"]) == list(G.P_SIZES) == [2, 5, 6, 7, 8, 21, 22]
    assert list(C.CASES["hp"]) == ["fd-ctor", "fd-h1", "fd-h2", "fd-h16", "fd-h64", "fd-s1", "fd-s2u", "fd-s3", "fd-s5", "fd-s8", "fd-k1",
                                   "fd-k20", "fd-kfull", "fd-kclamp", "fd-sclamp", "fd-e32", "fd-e64", "fd-e96", "fd-e160", "fd-T1"]
    for family, cases in C.CASES.items():
        assert set(C.UNSCREENED[family]) <= set(cases), family
        for key, entry in cases.items():
            assert _within_rule(entry) == (key not in C.UNSCREENED[family]), (family, key, entry)
            assert G.shape(family, key)[0] >= 2, (family, key)           # a BatchNorm over the P decoder rows needs two


def test_unscreened_and_moved_cases_are_within_the_cap():
    """At most CAP = 4 keys in total have no qualifying candidate, each with a structural reason; as many may have been moved."""
    unscreened = [(f, k) for f in C.CASES for k in C.UNSCREENED[f]]
    print("unscreened: %d %s" % (len(unscreened), unscreened))
    assert len(unscreened) <= C.CAP, unscreened
    assert all(G.UNSCREENED_REASONS.get(fk) for fk in unscreened), unscreened
    moved = [(f, k) for f in G.MOVED for k in G.MOVED[f]]
    assert len(moved) <= 4 and all(k in C.CASES[f] for f, k in moved), moved
    for f, k in moved:
        passed_over, diagnosis = G.MOVED[f][k]
        assert passed_over >= 1 and diagnosis, (f, k)


def test_batch_sizes_sit_on_both_sides_of_every_row_boundary():
    """The "P" family against the derivation in the generator: 12 P point rows and 144 P edge rows one below and one above each
    boundary; the "M" family crosses the 16-point boundary and the clamps; the weight-gradient slab cap (65 536 edge rows) is crossed
    by SLAB_CAP_P = 456 patches, a whole step the GPU sweep runs without an oracle, outside the table."""
    m = G.P_M
    for bound in G.P_POINT_BOUNDS:
        rows = sorted(p * m for p in G.P_SIZES)
        assert max(r for r in rows if r <= bound) > bound - m and min(r for r in rows if r > bound) <= bound + m, bound
    for bound in G.P_EDGE_BOUNDS:
        rows = sorted(p * m * m for p in G.P_SIZES)
        assert max(r for r in rows if r <= bound) > bound - m * m and min(r for r in rows if r > bound) <= bound + m * m, bound
    assert max(G.P_SIZES) * m * m < G.P_SLAB_CAP
    assert G.SLAB_CAP_P == 456 and (G.SLAB_CAP_P - 1) * m * m <= G.P_SLAB_CAP < G.SLAB_CAP_P * m * m and G.shape("P", G.SLAB_CAP_P) == (456, 12)
    points = sorted(G.shape("M", k)[0] * k for k in C.CASES["M"])
    for bound in (16, 64, 256):
        assert any(r < bound for r in points) and bound in points and any(r > bound for r in points), bound
    kw = G.BASE_KW
    edges = sorted(G.shape("M", k)[0] * k * min(kw["k"], k) for k in C.CASES["M"])
    assert any(r < 1024 for r in edges) and any(1024 < r < 2048 for r in edges)
    clamps = {tuple(min(k, mm) for k in list(kw["k_scales"]) + [kw["k"]]) for mm in C.CASES["M"]}
    assert {(9, 9, 9, 9), (10, 10, 10, 10), (10, 11, 11, 11), (10, 19, 19, 19), (10, 20, 20, 20), (10, 20, 21, 20), (10, 20, 39, 20),
            (10, 20, 40, 20)} <= clamps
    assert max(C.CASES["M"]) == 128                                      # the largest patch sapcu_patch_knn takes


def test_every_hyper_parameter_row_is_accepted_by_the_trainable_class():
    """Each fd row inference accepts is a case (none is dropped), the trainable class constructs with it and keeps its settings, and
    no row needs more LDS in the EdgeConv backward than the forward check allows: there is no refusal among the rows."""
    import sapcu_amd
    from sapcu_amd import fd_train
    seen = set()
    for rid in G.HP_ROWS:
        kw = G.model_kw("hp", rid)
        assert kw["dropout"] == 0.0
        model = sapcu_amd.TrainableSNNDistanceEstimation(**kw)
        assert (model.k, model.emb_dims, model.time_steps_enc, model.num_heads, list(model.k_scales)) == \
            (kw["k"], kw["emb_dims"], kw["time_steps_enc"], kw["num_heads"], list(kw["k_scales"])), rid
        assert model.dropout == 0.0 and model.emb_dims % 32 == 0
        p, m = G.shape("hp", rid)
        for kq in list(kw["k_scales"]) + [kw["k"]]:
            fd_train._check_patch_shape(m, min(int(kq), m))
        sd, names = G.state_dict("hp", rid)
        assert set(names) <= set(sd) and float(sd["encoder.snn_fc.threshold_base"].mean()) > 1.5
        from conftest import FD_KW
        seen |= {k for k in ("k", "k_scales", "emb_dims", "time_steps_enc", "num_heads") if kw[k] != FD_KW[k]}
    assert seen == {"k", "k_scales", "emb_dims", "time_steps_enc", "num_heads"}
    assert G.shape("hp", "fd-kclamp") == (4, 12) == G.shape("hp", "fd-sclamp") and G.model_kw("hp", "fd-kclamp")["k"] > 12
    assert G.model_kw("hp", "fd-k1")["k"] == 1 and G.model_kw("hp", "fd-kfull")["k"] == G.HP_M


def test_oracle_free_run_obeys_the_library_rule_and_forcing_on_itself_changes_nothing():
    """The oracle's own tables are the stable descending sort of exact integer scores, the same in f32 and f64; a run forced on its
    own tables and spikes returns the bits of the free run."""
    from oracle import train_path as TP
    family, key = "M", 11
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # torch's CPU gather backward sums in a thread-dependent order
    try:
        _free_and_forced(TP, family, key)
    finally:
        torch.set_num_threads(threads)


def _free_and_forced(TP, family, key):
    pts, gt = G.inputs(family, key, C.CASES[family][key][0])
    xyz = G.xyz_tables(family, key, pts)
    pred, loss, g, taps, _ = G.oracle_step(family, key, pts, gt, knn_xyz=xyz)
    knn, force = G.forcing(taps, G.BASE_KW["time_steps_enc"])
    for t in range(G.BASE_KW["time_steps_enc"]):
        for b in range(1, 4):
            sp = taps["spikes"][4 * t + b - 1]
            assert set(sp.unique().tolist()) <= {0.0, 1.0}
            assert torch.equal(TP.library_knn(sp.double(), 4, 11, 11), knn[t, b - 1]) and torch.equal(TP.library_knn(sp, 4, 11, 11), knn[t, b - 1])
            # score 0 comes first: the point itself, or a point of lower index with the same spike row
            first = knn[t, b - 1][..., 0]
            assert bool((first <= torch.arange(11)).all())
            assert torch.equal(torch.gather(sp.view(4, 11, -1), 1, first.unsqueeze(-1).expand(4, 11, sp.shape[1])), sp.view(4, 11, -1))
    pred2, loss2, g2, _, _ = G.oracle_step(family, key, pts, gt, knn=knn, force=force, knn_xyz=xyz)
    assert torch.equal(pred, pred2) and torch.equal(loss, loss2)
    assert all((g[n] is None and g2[n] is None) or torch.equal(g[n], g2[n]) for n in g)
    assert {n for n in g if g[n] is None} == {n for n in g if "threshold_adapt" in n or "refractory_decay" in n}
