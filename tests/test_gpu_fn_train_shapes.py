"""fn's training step (sapcu_amd/train.py over csrc/train_ops.hip) across patch sizes, batch shapes and hyper-parameter settings.

The single training ops are compared with f64 references at edge shapes in tests/test_gpu_bounds.py; here the COMPOSITION runs —
train.fn_train_forward + the loss + backward — at the inputs tests/fn_train_cases.py holds (chosen on the CPU by
tests/golden/make_fn_train_cases.py; its docstring has the families and the screening rule).  Per case:

  * the device's in-patch kNN tables equal the oracle's as sets per row;
  * normals <= 2e-4, loss <= 2e-4 and every compared gradient within 2e-2 max|ref| + 5e-5 peak of the f32 oracle run on the
    device's tables (the bars of test_training_step_of_whole_fn_model_against_reference_run); the biases that cancel in a
    BatchNorm (make_fn_train_cases.cancelled) must only be finite;
  * the step run a second time from fresh tensors gives the same bits: normals, loss and every gradient.

The screening ran the oracle with one torch thread on its own topk tables; here the f32 oracle runs with the machine's threads on
the device's tables (the same neighbour sets, possibly in another order within a row).  Another summation order in the ORACLE can
itself move a spike that sits on its threshold, as in test_training_step_of_whole_fn_model_against_reference_run: when a screened
case misses a bar, tests/fn_train_flips.py FAMILY KEY [SKIP] prints, layer by layer, which spikes differ and how far from their
thresholds they sit (output spikes and inner-step spikes); that is how the MOVED entries of the generator were made.

An UNSCREENED case (the oracle's own precisions disagree at every candidate) runs everything, asserts shapes, finiteness, unit
normals, the tables and the bit-equality, and prints the rest.  fn-k1 is the one such case: every neighbour is the point itself,
the position-encoding chain of block 1 sees identical rows, its gradients are mathematically zero and come out of the f32 oracle as
rounding noise (0.4 against a peak of 2.2e6, twice GRAD_COND).

Measured on an MI355X over the 50 screened cases: normals at most 1.2e-4 and loss 1.9e-5 (3 x 100), gradients at most 0.15 of their
bar (fn-e160), typically 0.003 .. 0.05.  Seven candidates were set aside on the way (make_fn_train_cases.MOVED has each one's figures
and layer): in all of them a neuron's membrane passes within 4e-6 of its threshold at some step, four times at the last step (the
flipped output spike spreads through the batch statistics), three times at an inner step only — the forward stays within its bars
and the gradients leave theirs, because the surrogate's path through that element changes.

The "B" family's table stops below the weight gradient's cap of 64 row slabs (65 536 edge rows = 456 patches: the CPU oracle of
such a step does not fit the time of a test).  test_training_step_above_the_weight_gradient_slab_cap runs the whole step there
without an oracle, test_weight_gradient_at_and_above_its_cap_... checks the op alone against exact sums.
"""
import os
import sys

import numpy as np
import pytest
import torch

import fn_train_cases as C
import gpu_utils as U

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_fn_train_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu

NORMALS_BAR, LOSS_BAR, GRAD_TOL, GRAD_FLOOR = 2e-4, 2e-4, 2e-2, 5e-5


def _device_step(family, key, pts, gt):
    """One training step on the device from fresh tensors: (normals, loss, {name: gradient}), all on the device."""
    from sapcu_amd import train
    kw = G.model_kw(family, key)
    sd, names = G.state_dict(family, key)
    p = {n: sd[n].to(U.dev()).clone().requires_grad_(True) for n in names}
    normals = train.fn_train_forward(p, pts.to(U.dev()), tuple(kw["k_values"]), kw["time_steps_enc"], kw["num_heads"])
    loss, _ = train.angular_loss_with_consistency(normals, gt.to(U.dev()), None)
    loss.backward()
    return normals.detach(), loss.detach(), {n: p[n].grad for n in names}


def _tables(family, key, pts):
    """The device's three kNN tables (CPU, int64), asserted equal to the oracle's as sets per row."""
    from sapcu_amd import train
    k_values = G.model_kw(family, key)["k_values"]
    ref = G.knn_tables(pts, k_values)
    out = []
    for k, r in zip(k_values, ref):
        idx = train.inpatch_knn(pts.to(U.dev()), min(k, pts.shape[1])).cpu().long()
        assert tuple(idx.shape) == tuple(r.shape)
        assert torch.equal(idx.sort(-1)[0], r.sort(-1)[0]), (family, key, k)
        out.append(idx)
    return out


def _device_case(family, key, skip):
    """The part of a case that needs no oracle step: the device's tables equal the oracle's as sets, the step runs twice from fresh
    tensors, shapes, finiteness, unit normals, and the second run's bits.  -> (pts, gt, tables, normals, loss, gradients)."""
    b, m = G.shape(family, key)
    pts, gt = G.inputs(family, key, skip)
    knn = _tables(family, key, pts)
    sd, names = G.state_dict(family, key)
    normals, loss, grads = _device_step(family, key, pts, gt)
    normals2, loss2, grads2 = _device_step(family, key, pts, gt)
    assert tuple(normals.shape) == (b, 3) and bool(torch.isfinite(normals).all()) and bool(torch.isfinite(loss))
    assert float((normals.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    for n in names:
        assert grads[n] is not None and grads[n].shape == sd[n].shape and bool(torch.isfinite(grads[n]).all()), n
    assert torch.equal(normals.view(torch.int32), normals2.view(torch.int32)) and torch.equal(loss, loss2), "the second run differs"
    differing = [n for n in names if not torch.equal(grads[n].view(torch.int32), grads2[n].view(torch.int32))]
    assert not differing, "gradients differ between two runs of the same step: %s" % differing[:8]
    return pts, gt, knn, normals, loss, grads


def _check_case(family, key):
    skip = C.CASES[family][key][0]
    screened = key not in C.UNSCREENED[family]
    b, m = G.shape(family, key)
    pts, gt, knn, normals, loss, grads = _device_case(family, key, skip)
    sd, names = G.state_dict(family, key)
    skip_names = G.cancelled(sd)

    ref_n, ref_l, ref_g = G.oracle_step(family, key, pts, gt, knn, torch.float32)
    e_n = float((normals.cpu() - ref_n).abs().max())
    e_l = abs(float(loss) - float(ref_l))
    compared = [n for n in names if n not in skip_names]
    peak = max(float(ref_g[n].abs().max()) for n in compared)
    worst, where = 0.0, ""
    for n in compared:
        err = float((grads[n].cpu() - ref_g[n]).abs().max())
        r = err / (GRAD_TOL * float(ref_g[n].abs().max()) + GRAD_FLOOR * peak)
        if not r <= worst:
            worst, where = r, n
    print("%s %s [%d x %d, skip %d]%s: normals %.3g (bar %g), loss %.3g (bar %g), gradients %.3g of their bar at %s (peak %.3g)"
          % (family, key, b, m, skip, "" if screened else " UNSCREENED", e_n, NORMALS_BAR, e_l, LOSS_BAR, worst, where, peak))
    if screened:
        assert e_n <= NORMALS_BAR and e_l <= LOSS_BAR, (family, key, e_n, e_l)
        assert worst <= 1.0, (family, key, where, worst)
    return normals, (pts, gt)


@pytest.mark.parametrize("m", sorted(C.CASES["M"]))
def test_training_step_at_patch_size(m):
    """B = 4 (3 from M = 100): through the clamps k = min(k, M) at 12, 18 and 24, B M through 64 and 256 rows, the edge rows
    through 1024."""
    _check_case("M", m)


@pytest.mark.parametrize("b", sorted(C.CASES["B"]))
def test_training_step_at_batch_size(b):
    """M = 12: the point rows 12 B and the edge rows 144 B one below and one above the row boundaries of csrc/train_ops.hip
    (make_fn_train_cases.B_SIZES has the derivation)."""
    _check_case("B", b)


def test_training_step_above_the_weight_gradient_slab_cap():
    """M = 12, B = SLAB_CAP_B = 456: 65 664 edge rows in every block, so the weight gradients of the fc_delta / fc_gamma layers run
    with more than 64 slabs' worth of rows (wgrad_slabs' cap: the slabs grow), through train.py's own workspace sizing and autograd,
    and the neuron backward and the column sums at that row count.  The CPU oracle of such a step does not fit the time of a test
    (make_fn_train_cases.py, at SLAB_CAP_B), so this is the protocol of an unscreened case without the printed oracle figures: the
    tables, shapes, finiteness, unit normals, and two runs bit for bit; additionally every compared gradient tensor is non-zero."""
    assert G.SLAB_CAP_B * G.B_M * G.B_M > G.B_SLAB_CAP >= (G.SLAB_CAP_B - 1) * G.B_M * G.B_M and G.SLAB_CAP_B not in C.CASES["B"]
    pts, gt, knn, normals, loss, grads = _device_case("B", G.SLAB_CAP_B, G.SLAB_CAP_SKIP)
    assert all(tuple(t.shape) == (G.SLAB_CAP_B, G.B_M, G.B_M) for t in knn)
    assert float(normals.std(0).max()) >= C.SPREAD
    dead = [n for n, g in grads.items() if n.endswith(".weight") and not bool(g.any())]
    assert not dead, dead
    print("B %d [%d x %d, skip %d]: loss %.6f, largest gradient entry %.3g" % (G.SLAB_CAP_B, G.SLAB_CAP_B, G.B_M, G.SLAB_CAP_SKIP, float(loss),
                                                                            max(float(g.abs().max()) for g in grads.values())))


@pytest.mark.parametrize("rid", list(C.CASES["hp"]))
def test_training_step_at_hyper_parameter_setting(rid):
    """One case per fn row of the hyper-parameter matrix; then the module itself in train() mode (dropouts 0) must return the
    bits of the direct fn_train_forward call with the row's settings — the constructor's arguments reach the ops — and a
    [B/2, 2, M, 3] input the bits of its [B, M, 3] flattening."""
    import sapcu_amd
    normals, (pts, _) = _check_case("hp", rid)
    model = sapcu_amd.ImprovedSNNNormalEstimation(**G.model_kw("hp", rid))
    model.load_state_dict(G.state_dict("hp", rid)[0], strict=True)
    model.attn_dropout = model.decoder_dropout = 0.0
    model = model.to(U.dev()).train()
    b, m, _ = pts.shape
    out = model(pts.to(U.dev())).detach()
    assert tuple(out.shape) == (b, 3) and torch.equal(out.view(torch.int32), normals.view(torch.int32)), rid
    out4 = model(pts.view(b // 2, 2, m, 3).to(U.dev())).detach()
    assert tuple(out4.shape) == (b // 2, 2, 3) and torch.equal(out4.reshape(b, 3).view(torch.int32), normals.view(torch.int32)), rid


# ---- the limits -----------------------------------------------------------------------------------------------------------------

def _small_params(requires_grad=True):
    sd, names = G.state_dict("M", 12)
    return {n: sd[n].to(U.dev()).clone().requires_grad_(requires_grad) for n in names}


def test_group_beyond_the_backward_lds_limit_is_refused_in_the_forward():
    """M = 700, k = 12 through knn= tables: (2 M k + M + 1) 4 B = 70 004 B of LDS in the grouped sum of the backward.  With
    gradients asked for, the forward raises ValueError and no gradient tensor is touched; under no_grad the same call runs."""
    from sapcu_amd import train
    b, m, k = 3, 700, 12
    assert not train.group_fits_backward(m, m * k) and train.group_fits_backward(128, 128 * 24)
    rng = np.random.default_rng(5)
    pts = torch.from_numpy(rng.normal(size=(b, m, 3)).astype(np.float32) * 0.05).to(U.dev())
    knn = [torch.from_numpy(np.stack([rng.permutation(m)[:k] for _ in range(b * m)]).reshape(b, m, k).astype(np.int32)).to(U.dev())
           for _ in range(3)]
    p = _small_params()
    with pytest.raises(ValueError, match="LDS"):
        train.fn_train_forward(p, pts, (k, k, k), 4, 8, knn=knn)
    assert all(t.grad is None for t in p.values())
    with torch.no_grad():
        out = train.fn_train_forward(p, pts, (k, k, k), 4, 8, knn=knn)
    assert tuple(out.shape) == (b, 3) and bool(torch.isfinite(out).all())
    # the ops themselves: refused only where a gradient is needed
    src = torch.zeros((b * m, 32), device=U.dev())
    index = (knn[0].to(torch.int64) + (torch.arange(b, device=U.dev()) * m).view(b, 1, 1)).reshape(-1)
    assert tuple(train.gather_rows(src, index, (m, m * k)).shape) == (b * m * k, 32)
    with pytest.raises(ValueError, match="gather_rows"):
        train.gather_rows(src.clone().requires_grad_(True), index, (m, m * k))
    a = torch.zeros((b * m * k, 32), device=U.dev())
    assert tuple(train.softmax_agg(a, a, src, knn[0].reshape(-1), m, 2.0).shape) == (b * m, 32)
    with pytest.raises(ValueError, match="softmax_agg"):
        train.softmax_agg(a, a, src.clone().requires_grad_(True), knn[0].reshape(-1), m, 2.0)


@pytest.mark.parametrize("gs,gr,fits", [(1, 8191, True), (2, 8191, False), (127, 8128, True), (128, 8128, False)])
def test_forward_refusal_and_the_grouped_sum_agree_on_the_limit(gs, gr, fits):
    """train.group_fits_backward against sapcu_scatter_add_rows_grouped itself on both sides of the 64 KiB limit: the largest
    groups the library takes (whose sums are checked) and the smallest it refuses (SAPCU_ERR_ARG before any launch)."""
    from sapcu_amd import _lib, train
    lib = _lib.load()
    assert train.group_fits_backward(gs, gr) == fits and ((2 * gr + gs + 1) * 4 <= 64 * 1024) == fits
    rng = np.random.default_rng(gs)
    d = 3
    gout = torch.from_numpy(rng.normal(size=(gr, d)).astype(np.float32))
    index = torch.from_numpy(rng.integers(0, gs, gr).astype(np.int64))
    out = torch.full((gs, d), float("nan"), device=U.dev())
    gout_d, index_d = gout.to(U.dev()), index.to(U.dev())
    rc = lib.sapcu_scatter_add_rows_grouped(_lib.ptr(gout_d), _lib.ptr(index_d), gr, d, _lib.ptr(out), d, gs, gs, gr, None, _lib.current_stream())
    torch.cuda.synchronize()
    if not fits:
        assert rc == -1 and bool(torch.isnan(out).all())                    # SAPCU_ERR_ARG, nothing written
        return
    assert rc == 0
    ref = torch.zeros((gs, d), dtype=torch.float64).index_add_(0, index, gout.double())
    # gr f32 additions one after the other: at most gr half-ulps of the sum of the magnitudes
    assert float((out.cpu().double() - ref).abs().max()) <= gr * 2.0 ** -24 * float(gout.abs().sum(0).max())


@pytest.mark.parametrize("rows", [64 * 1024, 64 * 1024 + 129])
def test_weight_gradient_at_and_above_its_cap_of_64_row_slabs_is_exact_on_integer_operands(rows):
    """sapcu_conv1x1_wgrad_f32 takes ~1024 rows per slab and at most 64 slabs: from 65 536 rows on a slab grows instead (no whole
    step of the sweep is that large: the "B" family stops below it).  Operands are integers in -2..2, so every product and every
    partial sum is an integer below 2^24 and the f32 result is exact in any summation order: grad_w and grad_bias must EQUAL the
    integer sums, whatever the slabs do with the rows past the 64th full slab."""
    from sapcu_amd import _lib
    lib = _lib.load()
    n, k = 64, 96
    rng = np.random.default_rng(rows)
    gy = rng.integers(-2, 3, (rows, n)).astype(np.float32)
    x = rng.integers(-2, 3, (rows, k)).astype(np.float32)
    gy_d, x_d = torch.from_numpy(gy).to(U.dev()), torch.from_numpy(x).to(U.dev())
    dw = torch.full((n, k), float("nan"), device=U.dev())
    db = torch.full((n,), float("nan"), device=U.dev())
    need = int(lib.sapcu_train_workspace_bytes(rows, n, k))
    ws = torch.empty((need,), dtype=torch.uint8, device=U.dev())
    _lib.check(lib.sapcu_conv1x1_wgrad_f32(_lib.ptr(gy_d), n, _lib.ptr(x_d), k, rows, n, k, _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), need,
                                           _lib.current_stream()))
    torch.cuda.synchronize()
    want_w = gy.astype(np.int64).T @ x.astype(np.int64)
    want_b = gy.astype(np.int64).sum(0)
    assert int(np.abs(want_w).max()) < 2 ** 24
    assert np.array_equal(dw.cpu().numpy().astype(np.int64), want_w) and np.array_equal(db.cpu().numpy(), want_b.astype(np.float32))


def test_more_than_eight_encoder_time_steps_are_refused_by_the_training_ops():
    """time_steps_enc = 9 in train() mode: the neuron ops take 1..8 steps — SapcuError(SAPCU_ERR_ARG) from the forward."""
    import sapcu_amd
    from conftest import FN_KW
    from sapcu_amd import _lib
    model = sapcu_amd.ImprovedSNNNormalEstimation(**dict(FN_KW, time_steps_enc=9)).to(U.dev()).train()
    with pytest.raises(_lib.SapcuError) as e:
        model(U.sphere_patches(3, 12).to(U.dev()))
    assert e.value.args[0] == -1                                            # SAPCU_ERR_ARG
    assert all(q.grad is None for q in model.parameters())


def test_patches_beyond_128_points_are_refused_by_the_neighbour_search():
    """M = 129 without knn=: sapcu_patch_knn refuses it (SAPCU_ERR_ARG) in the forward."""
    from sapcu_amd import _lib, train
    p = _small_params()
    pts = torch.from_numpy(np.random.default_rng(1).normal(size=(3, 129, 3)).astype(np.float32) * 0.05).to(U.dev())
    with pytest.raises(_lib.SapcuError) as e:
        train.fn_train_forward(p, pts)
    assert e.value.args[0] == -1 and "patch_knn" in e.value.args[1]
    assert all(t.grad is None for t in p.values())


def test_single_patch_batch_is_refused_like_batchnorm_refuses_it():
    """B = 1 through the module in train() mode: the decoder's BatchNorm has one value per channel — ValueError, as torch's
    BatchNorm gives in the reference."""
    import sapcu_amd
    from conftest import FN_KW
    model = sapcu_amd.ImprovedSNNNormalEstimation(**FN_KW)
    model.load_state_dict(G.state_dict("M", 12)[0], strict=True)
    model = model.to(U.dev()).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        model(U.sphere_patches(1, 12).to(U.dev()))
