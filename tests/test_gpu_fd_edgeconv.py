"""The factored EdgeConv training op of fd's blocks 1-3 and the AMP trainer on the GPU (row f-5; include/sapcu_fd_edgeconv.h,
csrc/fd_edgeconv_ops.hip, fd_train.edgeconv_factored / edgeconv_form, fd_trainer.AmpTrainer).

  * exact on dyadic inputs against the feature path (conv_bn_lrelu_max with idx), f32 and bf16, bit for bit;
  * against the reference's autograd on fd_edgeconv_train.npz at the feature path's bars; bf16 against a float64 restatement with
    bf16-rounded weights, the factored form's gradient error bounded by the feature path's;
  * the whole model teacher-forced (fd_train.npz, fd_train_b.npz) under edgeconv_form("factored"), f32 at the bars of the feature
    path's test, bf16 factored against bf16 feature;
  * AmpTrainer through fn_trainer.run_epoch, and the memory contract of the new header under guard bands.
"""
import math

import numpy as np
import pytest
import torch

from conftest import golden
import gpu_utils as U
from test_gpu_fd_train import CONFIGS, EIF_NAMES, _config, _dev, _feature_ref, _forced_run

F32, I32 = torch.float32, torch.int32


# ================================================================================================ exact on dyadic inputs
def _dyadic(P, M, kk, C, cout):
    rng = np.random.default_rng(P * 1000 + M * 10 + kk)
    x = (rng.uniform(size=(P * M, C)) > 0.5).astype(np.float32)
    w = (rng.integers(-16, 17, (cout, 2 * C)) / 8.0).astype(np.float32)             # multiples of 1/8 in [-2, 2]
    gamma, beta = rng.uniform(-1.5, 1.5, cout).astype(np.float32), rng.normal(0.0, 0.5, cout).astype(np.float32)
    idx = rng.integers(0, M, (P, M, kk)).astype(np.int32)                           # duplicates and self-neighbours occur
    go = rng.integers(-3, 4, (P * M, cout)).astype(np.float32)
    return x, w, gamma, beta, idx, go


def _run_op(form, mode, data, kk):
    """-> forward quantities (out, arg, mean, var * R / (R - 1), invstd) and gradients (x, w, gamma, beta), all on the CPU."""
    from sapcu_amd import fd_train, train as T
    x, w, gamma, beta, idx, go = data
    leaves = [_dev(a).requires_grad_(True) for a in (x, w, gamma, beta)]
    cout = w.shape[0]
    rm, rv = torch.zeros(cout, device=U.dev()), torch.zeros(cout, device=U.dev())
    with T.gemm_precision(mode):
        if form == "factored":
            out = fd_train.edgeconv_factored(*leaves, _dev(idx), running=(rm, rv, None, 1.0))
        else:
            out = fd_train.conv_bn_lrelu_max(*leaves, group=kk, idx=_dev(idx), running=(rm, rv, None, 1.0))
        mean, invstd, arg = out.grad_fn.saved_tensors[5:8]
        fwd = [t.detach().cpu().clone() for t in (out, arg, mean, rv, invstd)]
        assert torch.equal(fwd[2], rm.cpu())                                        # momentum 1: the running mean IS the batch mean
        out.backward(_dev(go))
    assert fd_train.take_bad_index_count() == 0
    return fwd, [t.grad.cpu().clone() for t in leaves]


@pytest.mark.gpu
@pytest.mark.parametrize("P,M,kk,C,cout", [(3, 7, 5, 96, 64), (2, 48, 20, 128, 256), (2, 100, 32, 256, 512), (1, 33, 33, 64, 96)])
def test_factored_equals_the_feature_path_bit_for_bit_on_dyadic_inputs(P, M, kk, C, cout):
    """x in {0,1}, weights multiples of 1/8 in [-2, 2] (exact in bf16), integer upstream gradients: every product and every sum up
    to y and its f64 statistics is exact, so out, arg, mean, var and invstd of the factored form equal the feature path's in f32
    mode, bf16 mode equals f32 mode, and two runs of either form are bit-identical in every gradient.  (2, 100, 32, 256, 512) is the
    reference's block 3: 6 400 edge rows, eight column tiles."""
    data = _dyadic(P, M, kk, C, cout)
    runs = {(form, mode): [_run_op(form, mode, data, kk) for _ in range(2)] for form in ("feature", "factored") for mode in ("f32", "bf16")}
    base = runs[("feature", "f32")][0][0]
    for key, (r0, r1) in runs.items():
        for name, a, b in zip(("out", "arg", "mean", "var", "invstd"), base, r0[0]):
            assert torch.equal(a, b), (key, name)
        for name, a, b in zip(("out", "arg", "mean", "var", "invstd"), r0[0], r1[0]):
            assert torch.equal(a, b), (key, name, "second run")
        for name, a, b in zip(("gx", "gw", "ggamma", "gbeta"), r0[1], r1[1]):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (key, name)
    x, w, _, _, idx, _ = data
    y = (_feature_ref(torch.from_numpy(x).double(), torch.from_numpy(idx), P, M, kk) @ torch.from_numpy(w).double().t()).view(P * M, kk, cout)
    at_max = torch.gather(y, 1, base[1].long().unsqueeze(1))
    assert int(((y == at_max).sum(1) > 1).sum()) > 0                                # arg-max ties did occur


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_smallest_case_one_edge_row_equals_the_feature_ops(mode):
    """P = M = kk = 1, C = 64, cout = 32: ONE edge row.  Both Python ops refuse it (BatchNorm in training mode needs more than one
    value per channel), so the comparison runs one level down: the feature path composed of its own entry points
    (sapcu_fd_edge_feature_forward, the GEMM, sapcu_fd_bn_stats, sapcu_fd_bn_lrelu_max_forward) against the factored forward,
    torch.equal in out, arg, mean, var, invstd; the factored backward twice, bit-identical."""
    from sapcu_amd import _lib, fd_train, train as T
    lib = _lib.load()
    P, M, kk, C, cout = 1, 1, 1, 64, 32
    x, w, gamma, beta, idx, go = (_dev(a) for a in _dyadic(P, M, kk, C, cout))
    for op in (lambda: fd_train.edgeconv_factored(x, w, gamma, beta, idx), lambda: fd_train.conv_bn_lrelu_max(x, w, gamma, beta, group=kk, idx=idx)):
        with pytest.raises(ValueError):
            op()
    wst = torch.cat([w[:, :C], w[:, C:]], dim=0).contiguous()
    with T.gemm_precision(mode):
        ab, mean, var, invstd, out, arg = fd_train._edgeconv_factored_forward(x, wst, idx, gamma, beta, 1e-5)
        y = torch.empty(1, cout, device=U.dev())
        T._gemm(fd_train.edge_feature_forward(x, idx), w, None, y)
        st = [torch.empty(cout, device=U.dev()) for _ in range(3)]
        need = int(lib.sapcu_fd_bn_stats_workspace_bytes(1, cout))
        ws = torch.empty(need, dtype=torch.uint8, device=U.dev())
        _lib.check(lib.sapcu_fd_bn_stats(_lib.ptr(y), 1, cout, 1e-5, *[_lib.ptr(t) for t in st], _lib.ptr(ws), need, _lib.current_stream()))
        o2, a2 = torch.empty(1, cout, device=U.dev()), torch.empty(1, cout, dtype=I32, device=U.dev())
        _lib.check(lib.sapcu_fd_bn_lrelu_max_forward(_lib.ptr(y), 1, 1, cout, _lib.ptr(st[0]), _lib.ptr(st[2]), _lib.ptr(gamma), _lib.ptr(beta),
                                                     _lib.ptr(o2), _lib.ptr(a2), _lib.current_stream()))
        for name, a, b in zip(("out", "arg", "mean", "var", "invstd"), (out, arg, mean, var, invstd), (o2, a2, st[0], st[1], st[2])):
            assert torch.equal(a, b), name
        assert not bool(var.any()) and not bool(arg.any())
        g = [fd_train._edgeconv_factored_backward(x, wst, idx, gamma, beta, ab, mean, invstd, arg, go) for _ in range(2)]
    assert fd_train.take_bad_index_count() == 0
    for a, b in zip(*g):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


# ================================================================================================ against the reference's autograd
@pytest.mark.gpu
def test_factored_edgeconv_block_against_reference_run():
    """The body of test_edgeconv_block_against_reference_run with edgeconv_factored in f32 mode, at that test's bars: block output
    <= 2e-4, spikes equal, running statistics <= 1e-5, gradients |d| <= 5e-3 max|ref| + 5e-5 max over all tensors."""
    from sapcu_amd import fd_train
    g = golden("fd_edgeconv_train.npz")
    assert int(g["argmax_ties"]) > 0
    x = _dev(g["x"]).requires_grad_(True)
    w, gamma, beta = (_dev(g[n]).requires_grad_(True) for n in ("w", "gamma", "beta"))
    raw = {n: _dev(g["raw:" + n]).requires_grad_(True) for n in EIF_NAMES}
    rm, rv, nt = torch.zeros(128, device=U.dev()), torch.ones(128, device=U.dev()), torch.zeros((), dtype=torch.int64, device=U.dev())
    z = fd_train.edgeconv_factored(x, w, gamma, beta, _dev(g["idx"]), running=(rm, rv, nt, 0.1))
    sp, _, pre = fd_train.neuron_step_train(z, raw)
    print("block output max err %.3g" % float((z.detach().cpu() - torch.from_numpy(g["z"])).abs().max()))
    assert float((z.detach().cpu() - torch.from_numpy(g["z"])).abs().max()) <= 2e-4
    assert torch.equal(sp.detach().cpu(), torch.from_numpy(g["spikes"]))
    np.testing.assert_allclose(rm.cpu().numpy(), g["running_mean"], atol=1e-5)
    np.testing.assert_allclose(rv.cpu().numpy(), g["running_var"], atol=1e-5)
    assert int(nt) == 1
    (sp * _dev(g["g"])).sum().backward()
    assert fd_train.take_bad_index_count() == 0
    pairs = [("gx", x), ("gw", w), ("ggamma", gamma), ("gbeta", beta)] + [("g:" + n, raw[n]) for n in EIF_NAMES if ("g:" + n) in g]
    floor = 5e-5 * max(float(np.abs(g[k]).max()) for k, _ in pairs)
    for key, tns in pairs:
        err = float((tns.grad.cpu() - torch.from_numpy(g[key])).abs().max())
        print("%s: max err %.3g of %.3g" % (key, err, float(np.abs(g[key]).max())))
        assert err <= 5e-3 * float(np.abs(g[key]).max()) + floor, (key, err)


@pytest.mark.gpu
def test_bf16_factored_against_a_float64_restatement_with_bf16_rounded_weights():
    """fd_edgeconv_train.npz with w replaced by its bf16 rounding ({0,1} inputs are exact in bf16, so the forward multiplies exact
    products and only the f32 summation order differs: forward <= 2e-4, the f32 bar).  Gradients: the feature path under
    gemm_precision("bf16") (the arithmetic before the factored form existed) and the factored op, each against float64 autograd of
    a torch restatement (feature, conv, train-mode BatchNorm, LeakyReLU, first arg-max).  The two forms round different
    intermediates to bf16 at 2^-9 relative each — the feature path dy [R, cout], the factored form the scattered sums — and neither
    is the more exact, so the bar is: factored error <= 2 x the feature path's + 5e-5 max|ref| over all tensors.
    Measured on MI355X (max abs error, feature / factored): see DESIGN.md 4.5."""
    from sapcu_amd import fd_train, train as T
    g = golden("fd_edgeconv_train.npz")
    P, M, kk = (int(v) for v in g["idx"].shape)
    wb = torch.from_numpy(g["w"]).reshape(128, -1).to(torch.bfloat16).to(F32)
    up = torch.from_numpy(np.random.default_rng(5).normal(size=(P * M, 128)).astype(np.float32))
    ref = [torch.from_numpy(g["x"]).double().requires_grad_(True), wb.double().requires_grad_(True),
           torch.from_numpy(g["gamma"]).double().requires_grad_(True), torch.from_numpy(g["beta"]).double().requires_grad_(True)]
    y = _feature_ref(ref[0], torch.from_numpy(g["idx"]), P, M, kk) @ ref[1].t()
    zn = (y - y.mean(0)) / torch.sqrt(y.var(0, unbiased=False) + 1e-5) * ref[2] + ref[3]
    act = torch.nn.functional.leaky_relu(zn, 0.2).view(P * M, kk, 128)
    first = (act == act.max(dim=1)[0].unsqueeze(1)).float().argmax(dim=1)
    want = torch.gather(act, 1, first.unsqueeze(1)).squeeze(1)
    (want * up.double()).sum().backward()
    floor = 5e-5 * max(float(t.grad.abs().max()) for t in ref)
    errs = {}
    for form in ("feature", "factored"):
        leaves = [_dev(g["x"]).requires_grad_(True), wb.to(U.dev()).requires_grad_(True), _dev(g["gamma"]).requires_grad_(True),
                  _dev(g["beta"]).requires_grad_(True)]
        with T.gemm_precision("bf16"):
            if form == "factored":
                out = fd_train.edgeconv_factored(*leaves, _dev(g["idx"]))
            else:
                out = fd_train.conv_bn_lrelu_max(*leaves, group=kk, idx=_dev(g["idx"]))
            (out * up.to(U.dev())).sum().backward()
        e_fwd = float((out.detach().cpu().double() - want.detach()).abs().max())
        print("%s bf16: forward max err %.3g" % (form, e_fwd))
        assert e_fwd <= 2e-4, (form, e_fwd)
        errs[form] = [float((t.grad.cpu().double() - r.grad).abs().max()) for t, r in zip(leaves, ref)]
    assert fd_train.take_bad_index_count() == 0
    for i, name in enumerate(("gx", "gw", "ggamma", "gbeta")):
        print("%s: bf16 max err feature %.3g, factored %.3g, of %.3g" % (name, errs["feature"][i], errs["factored"][i], float(ref[i].grad.abs().max())))
    for i, name in enumerate(("gx", "gw", "ggamma", "gbeta")):
        assert errs["factored"][i] <= 2 * errs["feature"][i] + floor, (name, errs["factored"][i], errs["feature"][i], floor)


# ================================================================================================ the whole model, teacher-forced
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_whole_fd_model_teacher_forced_in_factored_form_f32(cfg):
    """_forced_run of test_gpu_fd_train.py under edgeconv_form("factored"), f32: every bar of
    test_training_step_of_whole_fd_model_teacher_forced_on_the_reference_run."""
    from sapcu_amd import fd_train
    from test_oracle_golden import check_fn_train_grads
    kw, g, sd, names = _config(cfg)
    with fd_train.edgeconv_form("factored"):
        p, pred, loss, taps, flip, mar = _forced_run(kw, g, sd, names, True)
    assert fd_train._EDGECONV_FORM[0] == "feature"
    print("config %s factored: %d of %d spikes differ (largest |u| among them %.3g)"
          % (cfg, int(flip.sum()), flip.numel(), float(mar[flip].max()) if flip.any() else 0.0))
    assert float(flip.float().mean()) <= 0.01
    assert not bool(flip[mar > 1e-4].any())
    e_pool = float((torch.stack(taps["pooled"]).cpu() - torch.from_numpy(g["pooled"])).abs().max())
    e_int = float((taps["integrated"][0].cpu() - torch.from_numpy(g["integrated"])).abs().max())
    e_pred = float((pred - torch.from_numpy(g["pred"])).abs().max())
    print("config %s factored: pooled %.3g, integrated %.3g, prediction %.3g, loss %.3g" % (cfg, e_pool, e_int, e_pred, abs(loss - float(g["loss"]))))
    assert e_pool <= 2e-4 and e_int <= 2e-4 and e_pred <= 2e-4 and abs(loss - float(g["loss"])) <= 2e-4
    assert {n for n in names if p[n].grad is None} == {str(n) for n in g["grad_none"]}
    assert {n for n in names if p[n].grad is not None and not bool(p[n].grad.any())} == {str(n) for n in g["grad_zero"]}
    graded = [n for n in names if p[n].grad is not None]
    worst = check_fn_train_grads(g, p, graded, 2e-2, 5e-5)
    print("config %s factored: worst gradient error relative to its bar's scale %.3g" % (cfg, worst))
    for n, v in sd.items():
        if n in names:
            continue
        if n.endswith("num_batches_tracked"):
            assert int(p[n]) == int(g["buf:" + n]), n
        else:
            np.testing.assert_allclose(p[n].cpu().numpy(), g["buf:" + n], rtol=0, atol=1e-5, err_msg=n)


def _worst_grad_error(g, p, names, floor_rel):
    """The value test_oracle_golden.check_fn_train_grads(g, p, names, tol, floor_rel) returns — max over the tensors of
    max|got - ref| / (max|ref| + floor_rel * peak), sampled rows for the large ones — by the same formula, without that helper's
    own assertions: at tol = 1.0 the bf16 FEATURE path (the arithmetic that existed before the factored form) already trips them
    on MI355X for distance_decoder.attention.norm.bias, a tensor whose reference gradient is 7.5e-9 (error 4.14e-5 against
    1.0 * 7.5e-9 + floor 3.94e-5), and no value would be returned to compare."""
    peak = max(float(np.abs(g[("g:" if ("g:" + n) in g else "gs:") + n]).max()) for n in names)
    floor = floor_rel * peak
    worst = 0.0
    for n in names:
        got = p[n].grad.detach().cpu().numpy().ravel()
        ref = g["g:" + n].ravel() if ("g:" + n) in g else g["gs:" + n]
        if ("g:" + n) not in g:
            got = got[g["gi:" + n]]
        worst = max(worst, float(np.abs(got - ref).max()) / (float(np.abs(ref).max()) + floor))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_whole_fd_model_teacher_forced_bf16_factored_against_bf16_feature(cfg):
    """Both forms under gemm_precision("bf16"), teacher-forced: pooled, integrated, prediction and loss within 2e-4 of each other,
    the grad-None and grad-zero sets the fixture's, and the worst gradient error (the value check_fn_train_grads(.., 1.0, 5e-5)
    returns, relative to max|ref| + floor; see _worst_grad_error) of the factored form <= 2 x the feature form's — the two round different intermediates to bf16 at 2^-9
    each, neither is the more exact.  Measured values: DESIGN.md 4.5."""
    from sapcu_amd import fd_train, train as T
    kw, g, sd, names = _config(cfg)
    res = {}
    for form in ("feature", "factored"):
        with T.gemm_precision("bf16"), fd_train.edgeconv_form(form):
            p, pred, loss, taps, _, _ = _forced_run(kw, g, sd, names, True)
        assert {n for n in names if p[n].grad is None} == {str(n) for n in g["grad_none"]}, form
        assert {n for n in names if p[n].grad is not None and not bool(p[n].grad.any())} == {str(n) for n in g["grad_zero"]}, form
        graded = [n for n in names if p[n].grad is not None]
        worst = _worst_grad_error(g, p, graded, 5e-5)
        print("config %s bf16 %s: worst gradient error relative to its scale %.3g" % (cfg, form, worst))
        res[form] = (torch.stack(taps["pooled"]).cpu(), taps["integrated"][0].cpu(), pred, torch.tensor(loss), worst)
    for i, name in enumerate(("pooled", "integrated", "prediction", "loss")):
        d = float((res["feature"][i] - res["factored"][i]).abs().max())
        print("config %s bf16: %s differs by %.3g between the forms" % (cfg, name, d))
        assert d <= 2e-4, (name, d)
    assert res["factored"][4] <= 2 * res["feature"][4], (res["factored"][4], res["feature"][4])


# ================================================================================================ trainer
EPOCH_KW = dict(k=8, emb_dims=64, time_steps_enc=3, num_heads=4, k_scales=[4, 8, 16], dropout=0.1)


def _fresh(seed=0):
    import sapcu_amd
    torch.manual_seed(seed)
    model = sapcu_amd.TrainableSNNDistanceEstimation(**EPOCH_KW).to(U.dev())
    model.dropout_generator = torch.Generator(device=U.dev()).manual_seed(7)
    return model, torch.optim.AdamW(model.parameters(), lr=3e-3)


@pytest.mark.gpu
def test_amp_epoch_is_reproducible_accumulates_learns_and_leaves_an_inference_model():
    """fn_trainer.run_epoch over 12 SyntheticFdPatches batches with AmpTrainer(use_amp=True, gradient_accumulation=2,
    grad_clip=0.1) in its default EdgeConv form, twice: bit-identical; six optimiser steps."""
    import sapcu_amd
    from sapcu_amd import fd_trainer, fn_trainer
    runs = []
    for _ in range(2):
        model, opt = _fresh()
        trainer = fd_trainer.AmpTrainer(model, opt, device=U.dev(), use_amp=True, gradient_accumulation=2, grad_clip=0.1)
        loader = fd_trainer.SyntheticFdPatches(batches=12, batch_size=2, patches=8, points=24, seed=3)
        it, losses, st = fn_trainer.run_epoch(trainer, loader, clamp_parameters=True)
        assert it == 12 and st["skipped"] == 0 and len(losses) == 12 and all(np.isfinite(losses))
        assert trainer.accumulation_step == 0
        runs.append((losses, {n: q.detach().cpu().clone() for n, q in model.named_parameters()},
                     {n: b.detach().cpu().clone() for n, b in model.named_buffers()}, model))
    print("losses: " + " ".join("%.5f" % v for v in runs[0][0]))
    assert runs[0][0] == runs[1][0]
    for k in (1, 2):
        for n in runs[0][k]:
            assert torch.equal(runs[0][k][n], runs[1][k][n]), n
    assert int(runs[0][2]["encoder.scale_fusion.1.num_batches_tracked"]) == 36
    # accumulation really defers the step: an odd first call leaves the parameters, the second moves them
    model, opt = _fresh()
    init = {n: q.detach().clone() for n, q in model.named_parameters()}
    trainer = fd_trainer.AmpTrainer(model, opt, device=U.dev(), use_amp=True, gradient_accumulation=2, grad_clip=0.1)
    two = list(fd_trainer.SyntheticFdPatches(batches=2, batch_size=2, patches=8, points=24, seed=3))
    assert trainer.train_step(two[0])[0] is not None and trainer.accumulation_step == 1
    assert all(torch.equal(q.detach(), init[n]) for n, q in model.named_parameters())
    assert trainer.train_step(two[1])[0] is not None and trainer.accumulation_step == 0
    assert any(not torch.equal(q.detach(), init[n]) for n, q in model.named_parameters())
    assert any(not torch.equal(q, init[n].cpu()) for n, q in runs[0][1].items())
    assert np.mean(runs[0][0][-4:]) < np.mean(runs[0][0][:4]), runs[0][0]
    model = runs[0][3].eval()
    base = sapcu_amd.EnhancedSNNDistanceEstimation(**EPOCH_KW)
    base.load_state_dict(model.state_dict(), strict=True)
    base = base.to(U.dev())
    x = next(iter(fd_trainer.SyntheticFdPatches(batches=1, batch_size=2, patches=8, points=24, seed=9)))["input"].to(U.dev())
    with torch.no_grad():
        a, b = model(x), base(x)
    assert a.shape == (2, 8) and torch.equal(a, b)


@pytest.mark.gpu
def test_amp_trainer_in_f32_feature_form_is_the_f32_trainer_and_a_grad_scaler_is_driven():
    from sapcu_amd import fd_trainer
    batches = list(fd_trainer.SyntheticFdPatches(batches=3, batch_size=2, patches=8, points=24, seed=3))
    losses = []
    for make in (lambda m, o: fd_trainer.Trainer(m, o, device=U.dev(), grad_clip=0.1),
                 lambda m, o: fd_trainer.AmpTrainer(m, o, device=U.dev(), grad_clip=0.1, use_amp=False, edgeconv="feature")):
        model, opt = _fresh()
        tr = make(model, opt)
        losses.append([tr.train_step(b)[0] for b in batches])
    print(losses)
    assert losses[0] == losses[1] and all(v is not None and math.isfinite(v) for v in losses[0])
    model, opt = _fresh()
    init = {n: q.detach().clone() for n, q in model.named_parameters()}
    scaler = torch.amp.GradScaler('cuda')
    tr = fd_trainer.AmpTrainer(model, opt, device=U.dev(), grad_clip=0.1, use_amp=True, scaler=scaler)
    assert tr.train_step(batches[0])[0] is not None
    assert int(scaler.state_dict()["_growth_tracker"]) == 1                         # update() ran after a step that was not skipped
    assert any(not torch.equal(q.detach(), init[n]) for n, q in model.named_parameters())
    assert tr.train_step(batches[1])[0] is not None and int(scaler.state_dict()["_growth_tracker"]) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["feature", "factored"])
def test_an_index_outside_its_patch_fails_the_amp_step_and_leaves_the_gradients_zeroed(form, monkeypatch):
    """fd_train_forward refuses a forced table with such an index up front (ValueError, as before), so the index is planted where
    no check stands: in the table the free-running feature kNN hands to blocks 1-3."""
    from sapcu_amd import fd_train, fd_trainer
    real = fd_train.feature_knn

    def planted(x, P, M, k):
        idx = real(x, P, M, k)
        idx[0, 0, 0] = M
        return idx
    monkeypatch.setattr(fd_train, "feature_knn", planted)
    model, opt = _fresh()
    tr = fd_trainer.AmpTrainer(model, opt, device=U.dev(), grad_clip=0.1, use_amp=True, gradient_accumulation=2, edgeconv=form)
    batch = next(iter(fd_trainer.SyntheticFdPatches(batches=1, batch_size=2, patches=8, points=24, seed=3)))
    with pytest.raises(RuntimeError):
        tr.train_step(batch)
    assert tr.accumulation_step == 0 and fd_train.take_bad_index_count() == 0
    assert all(q.grad is None or not bool(q.grad.any()) for q in model.parameters())


# ================================================================================================ small behaviours
@pytest.mark.gpu
def test_factored_max_propagates_nan_like_the_feature_path():
    """A NaN in s of one point reaches exactly the edges whose neighbour it is; a NaN in a of a point all of its own.  Out, the NaN
    mask and the arg-max (the first NaN) equal sapcu_fd_bn_lrelu_max_forward's on the same y."""
    from sapcu_amd import _lib
    lib = _lib.load()
    P, M, kk, ch = 2, 6, 4, 32
    rng = np.random.default_rng(2)
    ab = torch.from_numpy(rng.integers(-8, 9, (P * M, 2 * ch)).astype(np.float32))
    idx = torch.from_numpy(rng.integers(0, M, (P, M, kk)).astype(np.int32))
    ab[3, ch + 5] = float("nan")                                                    # b of point 3, channel 5 -> s[3]
    ab[M + 2, 7] = float("nan")                                                     # a of point 2 of patch 1, channel 7
    a, s = ab[:, :ch].view(P, M, ch), (ab[:, :ch] + ab[:, ch:]).view(P, M, ch)
    y = (torch.gather(s.unsqueeze(1).expand(P, M, M, ch), 2, idx.long().unsqueeze(-1).expand(P, M, kk, ch)) - a.unsqueeze(2)).reshape(P * M * kk, ch)
    dev = U.dev()
    mean, one = torch.full((ch,), 0.5, device=dev), torch.ones(ch, device=dev)
    gamma, beta = _dev(rng.uniform(-1.5, 1.5, ch).astype(np.float32)), _dev(rng.normal(0, 0.5, ch).astype(np.float32))
    o1, a1, o2, a2 = (torch.empty(P * M, ch, dtype=dt, device=dev) for dt in (F32, I32, F32, I32))
    abd, idxd, yd = ab.to(dev), idx.to(dev), y.to(dev)
    _lib.check(lib.sapcu_fd_edgeconv_max_forward(_lib.ptr(abd), _lib.ptr(idxd), P, M, kk, ch, _lib.ptr(mean), _lib.ptr(one), _lib.ptr(gamma),
                                                 _lib.ptr(beta), _lib.ptr(o1), _lib.ptr(a1), _lib.current_stream()))
    _lib.check(lib.sapcu_fd_bn_lrelu_max_forward(_lib.ptr(yd), P * M, kk, ch, _lib.ptr(mean), _lib.ptr(one), _lib.ptr(gamma), _lib.ptr(beta),
                                                 _lib.ptr(o2), _lib.ptr(a2), _lib.current_stream()))
    nan = torch.isnan(o2.cpu())
    assert int(nan.sum()) >= 2 and int(nan.sum()) < nan.numel() and torch.equal(torch.isnan(o1.cpu()), nan)
    assert torch.equal(o1.cpu()[~nan], o2.cpu()[~nan]) and torch.equal(a1.cpu(), a2.cpu())


@pytest.mark.gpu
def test_factored_op_refuses_a_patch_beyond_the_lds_limit_in_the_forward():
    from sapcu_amd import fd_train
    x = torch.zeros(128, 32, device=U.dev())
    with pytest.raises(ValueError):
        fd_train.edgeconv_factored(x, torch.zeros(32, 64, device=U.dev()), torch.ones(32, device=U.dev()), torch.zeros(32, device=U.dev()),
                                   torch.zeros(1, 128, 64, dtype=I32, device=U.dev()))


# ================================================================================================ the memory contract
EC_CASES, EC_REFUSALS = [], []


def _B():
    import test_gpu_bounds as B
    return B


def _edgeconv_case(P, M, kk, ch, ws_off):
    def build(A):
        B = _B()
        _lib, lib = B._lib_()
        rng = np.random.default_rng(P + M + kk + ch)
        pts = P * M
        ab = rng.normal(0.2, 1.0, (pts, 2 * ch)).astype(np.float32)
        idx = rng.integers(0, M, (P, M, kk)).astype(np.int32)
        gamma, beta = rng.uniform(-1.5, 1.5, ch).astype(np.float32), rng.normal(0.2, 0.5, ch).astype(np.float32)
        go = rng.normal(size=(pts, ch)).astype(np.float32)
        AB, I, Ga, Be, GO = (A.inp(v, offset=4, name=n) for v, n in ((ab, "ab"), (idx, "idx"), (gamma, "gamma"), (beta, "beta"), (go, "grad_out")))
        s_need = int(lib.sapcu_fd_edgeconv_stats_workspace_bytes(P, M, kk, ch))
        b_need = int(lib.sapcu_fd_edgeconv_backward_workspace_bytes(P, M, kk, ch))
        assert s_need > 0 and b_need > 0
        ws_s = A.ws(s_need, offset=ws_off, tile_row_bytes=8 * ch, name="edgeconv stats workspace")
        ws_b = A.ws(b_need, offset=ws_off, tile_row_bytes=8 * ch, name="edgeconv backward workspace")
        o = {n: A.out((ch,), F32, offset=4, name=n) for n in ("mean", "var", "invstd", "ggamma", "gbeta")}
        o["out"], o["arg"] = A.out((pts, ch), F32, offset=4, name="out"), A.out((pts, ch), I32, offset=4, name="argmax")
        o["gab"] = A.out((pts, 2 * ch), F32, offset=4, name="grad_ab")
        o["bad_f"], o["bad_b"] = A.out((1,), I32, offset=4, name="bad_count stats"), A.out((1,), I32, offset=4, name="bad_count backward")
        Pp = B.P

        def call():
            B.ok(lib.sapcu_fd_edgeconv_stats(Pp(AB), Pp(I), P, M, kk, ch, 1e-5, Pp(o["mean"]), Pp(o["var"]), Pp(o["invstd"]), Pp(o["bad_f"]),
                                             Pp(ws_s), s_need, B.S()))
            B.ok(lib.sapcu_fd_edgeconv_max_forward(Pp(AB), Pp(I), P, M, kk, ch, Pp(o["mean"]), Pp(o["invstd"]), Pp(Ga), Pp(Be), Pp(o["out"]),
                                                   Pp(o["arg"]), B.S()))
            B.ok(lib.sapcu_fd_edgeconv_backward(Pp(AB), Pp(I), Pp(GO), Pp(o["arg"]), P, M, kk, ch, Pp(o["mean"]), Pp(o["invstd"]), Pp(Ga), Pp(Be),
                                                Pp(o["gab"]), Pp(o["ggamma"]), Pp(o["gbeta"]), Pp(o["bad_b"]), Pp(ws_b), b_need, B.S()))

        def ref(r):
            abr = torch.from_numpy(ab).double().requires_grad_(True)
            ga, be = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
            a, s = abr[:, :ch].view(P, M, ch), (abr[:, :ch] + abr[:, ch:]).view(P, M, ch)
            nb = torch.gather(s.unsqueeze(1).expand(P, M, M, ch), 2, torch.from_numpy(idx).long().unsqueeze(-1).expand(P, M, kk, ch))
            y = (nb - a.unsqueeze(2)).reshape(pts * kk, ch)
            mean, var = y.mean(0), y.var(0, unbiased=False)
            z = (y - mean) / torch.sqrt(var + 1e-5) * ga + be
            act = torch.nn.functional.leaky_relu(z, 0.2).view(pts, kk, ch)
            first = (act == act.max(dim=1)[0].unsqueeze(1)).float().argmax(dim=1)       # duplicates tie exactly: the first
            val = torch.gather(act, 1, first.unsqueeze(1)).squeeze(1)
            val.backward(torch.from_numpy(go).double())
            tol = lambda want: 5e-5 * max(1.0, float(want.abs().max()))
            for n, want in (("mean", mean), ("var", var), ("invstd", 1 / torch.sqrt(var + 1e-5)), ("out", val), ("gab", abr.grad),
                            ("ggamma", ga.grad), ("gbeta", be.grad)):
                assert float((r[n].double() - want.detach()).abs().max()) <= tol(want.detach()), n
            assert torch.equal(r["arg"].long(), first)
            assert int(r["bad_f"]) == 0 and int(r["bad_b"]) == 0
        return B.built(call, o, ref)
    EC_CASES.append(_B().Case("fd_edgeconv-P%d-M%d-k%d-c%d" % (P, M, kk, ch),
                              ("sapcu_fd_edgeconv_stats", "sapcu_fd_edgeconv_max_forward", "sapcu_fd_edgeconv_backward"),
                              ("sapcu_fd_edgeconv_stats_workspace_bytes", "sapcu_fd_edgeconv_backward_workspace_bytes"), build))


_edgeconv_case(3, 7, 5, 96, 0)
_edgeconv_case(2, 48, 20, 64, 8)
_edgeconv_case(1, 1, 1, 32, 0)
_edgeconv_case(5, 33, 33, 160, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("c", EC_CASES, ids=[c.id for c in EC_CASES])
def test_fd_edgeconv_bounds(c):
    """0xFF bands, 0x00 bands, dirty workspace, compact call (tests/test_gpu_bounds.py): bands intact, the four results bit-identical,
    and the values against float64 autograd of a torch restatement."""
    _B().run_protocol(c)


def _ec_refusal(id_, want, what, short=0, ws_off=0, m=7, kk=5, null=None):
    def run(A):
        B = _B()
        _lib, lib = B._lib_()
        P, ch = 2, 32
        mm, kq = (m, kk) if kk > 0 and (2 * m * kk + m + 1) * 4 <= 64 * 1024 else (7, 5)      # buffers of a legal size for an illegal shape
        ab, idx = A.inp(np.ones((P * mm, 2 * ch), np.float32), name="ab"), A.inp(np.zeros((P, mm, kq), np.int32), name="idx")
        v = [A.inp(np.ones(ch, np.float32), name="v%d" % i) for i in range(4)]
        go, arg = A.inp(np.ones((P * mm, ch), np.float32), name="grad_out"), A.inp(np.zeros((P * mm, ch), np.int32), name="argmax")
        st = [A.out((ch,), F32, name="stat%d" % i) for i in range(3)]
        out, argo, gab = A.out((P * mm, ch), F32, name="out"), A.out((P * mm, ch), I32, name="argmax_out"), A.out((P * mm, 2 * ch), F32, name="grad_ab")
        gg, gb, bad = A.out((ch,), F32, name="grad_gamma"), A.out((ch,), F32, name="grad_beta"), A.out((1,), I32, name="bad_count")
        sizer = lib.sapcu_fd_edgeconv_stats_workspace_bytes if what == "stats" else lib.sapcu_fd_edgeconv_backward_workspace_bytes
        need = int(sizer(P, mm, kq, ch))
        ws = A.ws(need - short, offset=ws_off, name="workspace")
        if what == "stats":
            return lib.sapcu_fd_edgeconv_stats(B.P(ab), None if null == "idx" else B.P(idx), P, m, kk, ch, 1e-5, *[B.P(q) for q in st], B.P(bad),
                                               B.P(ws), need - short, B.S())
        if what == "max":
            return lib.sapcu_fd_edgeconv_max_forward(B.P(ab), B.P(idx), P, m, kk, ch, *[B.P(q) for q in v], B.P(out),
                                                     None if null == "arg" else B.P(argo), B.S())
        return lib.sapcu_fd_edgeconv_backward(B.P(ab), B.P(idx), B.P(go), B.P(arg), P, m, kk, ch, *[B.P(q) for q in v], B.P(gab), B.P(gg), B.P(gb),
                                              None if null == "bad" else B.P(bad), B.P(ws), need - short, B.S())
    EC_REFUSALS.append((id_, want, run))


_ec_refusal("stats-workspace-one-byte-short", -2, "stats", short=1)
_ec_refusal("stats-workspace-4-byte-aligned", -1, "stats", ws_off=4)
_ec_refusal("stats-null-idx", -1, "stats", null="idx")
_ec_refusal("stats-inverse-table-beyond-lds", -1, "stats", m=128, kk=64)
_ec_refusal("max-forward-null-argmax", -1, "max", null="arg")
_ec_refusal("max-forward-zero-neighbours", -1, "max", kk=0)
_ec_refusal("max-forward-inverse-table-beyond-lds", -1, "max", m=128, kk=64)
_ec_refusal("backward-workspace-one-byte-short", -2, "backward", short=1)
_ec_refusal("backward-workspace-4-byte-aligned", -1, "backward", ws_off=4)
_ec_refusal("backward-null-bad_count", -1, "backward", null="bad")
_ec_refusal("backward-inverse-table-beyond-lds", -1, "backward", m=128, kk=64)


@pytest.mark.gpu
@pytest.mark.parametrize("r", EC_REFUSALS, ids=[r[0] for r in EC_REFUSALS])
def test_fd_edgeconv_refusal_launches_nothing(r):
    from guarded import Arena
    id_, want, run = r
    A = Arena("guard", 0xFF, U.dev())
    rc = run(A)
    torch.cuda.synchronize()
    assert rc == want, "%s returned %d, expected %d" % (id_, rc, want)
    A.check()
    for gd in A.outs + A.wss:
        assert bool((gd.payload_bits() == 0xFF).all()), "%s: %s was written by a refused call" % (id_, gd.name)


@pytest.mark.gpu
def test_edgeconv_entry_points_count_indices_outside_their_patch_and_give_them_no_gradient():
    """An index outside [0, m): y of that edge is 0 (it counts in the statistics as a zero row), both counters count it, the
    gradient is that of the same table with the edge removed from the scatter, and nothing outside the buffers is touched."""
    from guarded import Arena
    B = _B()
    _lib, lib = B._lib_()
    P, M, kk, ch = 2, 7, 5, 32
    rng = np.random.default_rng(0)
    idx = rng.integers(0, M, (P, M, kk)).astype(np.int32)
    idx[0, 3, 2], idx[1, 6, 4], idx[1, 0, 0] = M, -1, 1 << 30
    ab = rng.integers(-8, 9, (P * M, 2 * ch)).astype(np.float32)
    A = Arena("guard", 0xFF, U.dev())
    AB, I = A.inp(ab, name="ab"), A.inp(idx, name="idx")
    st = [A.out((ch,), F32, name="stat%d" % i) for i in range(3)]
    bf, bb = A.out((1,), I32, name="bad stats"), A.out((1,), I32, name="bad backward")
    out, arg, gab = A.out((P * M, ch), F32, name="out"), A.out((P * M, ch), I32, name="argmax"), A.out((P * M, 2 * ch), F32, name="grad_ab")
    gg, gb = A.out((ch,), F32, name="grad_gamma"), A.out((ch,), F32, name="grad_beta")
    one, zero, go = A.inp(np.ones(ch, np.float32), name="gamma"), A.inp(np.zeros(ch, np.float32), name="beta"), A.inp(np.ones((P * M, ch), np.float32), name="grad_out")
    s_need, b_need = int(lib.sapcu_fd_edgeconv_stats_workspace_bytes(P, M, kk, ch)), int(lib.sapcu_fd_edgeconv_backward_workspace_bytes(P, M, kk, ch))
    ws_s, ws_b = A.ws(s_need, name="stats workspace"), A.ws(b_need, name="backward workspace")
    B.ok(lib.sapcu_fd_edgeconv_stats(B.P(AB), B.P(I), P, M, kk, ch, 1e-5, *[B.P(q) for q in st], B.P(bf), B.P(ws_s), s_need, B.S()))
    B.ok(lib.sapcu_fd_edgeconv_max_forward(B.P(AB), B.P(I), P, M, kk, ch, B.P(st[0]), B.P(st[2]), B.P(one), B.P(zero), B.P(out), B.P(arg), B.S()))
    B.ok(lib.sapcu_fd_edgeconv_backward(B.P(AB), B.P(I), B.P(go), B.P(arg), P, M, kk, ch, B.P(st[0]), B.P(st[2]), B.P(one), B.P(zero), B.P(gab),
                                        B.P(gg), B.P(gb), B.P(bb), B.P(ws_b), b_need, B.S()))
    torch.cuda.synchronize()
    A.check()
    assert int(bf) == 3 and int(bb) == 3
    a, s = torch.from_numpy(ab[:, :ch]).view(P, M, ch), torch.from_numpy(ab[:, :ch] + ab[:, ch:]).view(P, M, ch)
    ok = torch.from_numpy((idx >= 0) & (idx < M))
    nb = torch.gather(s.unsqueeze(1).expand(P, M, M, ch), 2, torch.from_numpy(idx).long().clamp(0, M - 1).unsqueeze(-1).expand(P, M, kk, ch))
    y = ((nb - a.unsqueeze(2)) * ok.unsqueeze(-1)).reshape(P * M * kk, ch).double()
    np.testing.assert_allclose(st[0].cpu().numpy(), y.mean(0).numpy(), atol=1e-6)               # the zero rows count
    np.testing.assert_allclose(st[1].cpu().numpy(), y.var(0, unbiased=False).numpy(), rtol=1e-6, atol=1e-6)
    assert bool(torch.isfinite(gab).all()) and bool(torch.isfinite(out).all())


def test_every_entry_point_of_the_fd_edgeconv_header_has_a_bounds_case():
    """The gate of test_every_entry_point_of_the_fd_train_header_has_a_bounds_case over include/sapcu_fd_edgeconv.h."""
    from sapcu_amd import _lib
    from test_fd_edgeconv_host import fd_edgeconv_header_entry_points
    decl = fd_edgeconv_header_entry_points()
    assert set(decl) == set(_lib.FD_EDGECONV_EXPORTS)
    covered, used = set(), set()
    for c in EC_CASES:
        assert c.entry_points, c.id
        covered.update(c.entry_points)
        used.update(c.sizers)

    def uncovered(cov):
        return sorted(n for n, args in decl.items() if "*" in args and n not in cov)
    assert covered <= set(decl) and not uncovered(covered), uncovered(covered)
    assert uncovered(covered - {"sapcu_fd_edgeconv_stats"}) == ["sapcu_fd_edgeconv_stats"]      # the gate itself
    assert {n for n in decl if n.endswith("workspace_bytes")} == used
    assert {r[0] for r in EC_REFUSALS} >= {"stats-workspace-one-byte-short", "backward-workspace-one-byte-short", "backward-null-bad_count",
                                           "backward-workspace-4-byte-aligned", "max-forward-null-argmax", "backward-inverse-table-beyond-lds"}
