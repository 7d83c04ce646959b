"""fd training on the GPU (row f-5; include/sapcu_fd_train.h, csrc/fd_train_ops.hip, sapcu_amd/fd_train.py, fd_trainer.py).

  * the single-step neuron and one EdgeConv block against runs of the reference (tests/golden/fd_neuron_step_train.npz,
    fd_edgeconv_train.npz), the feature op and the fused BatchNorm + LeakyReLU + max against torch on {0,1} inputs, bit for bit;
  * one training step of the whole model, two configurations, teacher-forced on the reference's own kNN tables and spikes
    (fd_train.npz, fd_train_b.npz): taps, prediction, loss, every gradient, the None / zero gradient sets, the BatchNorm buffers;
  * a free-running step, an epoch through fn_trainer.run_epoch, and the memory contract of the new header under guard bands.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import golden
import gpu_utils as U

F32, I32 = torch.float32, torch.int32
LIF_NAMES = ("membrane_decay", "threshold_adapt", "refractory_decay", "threshold_base")
EIF_NAMES = LIF_NAMES + ("delta_T", "theta_rh")
CONFIGS = {
    "A": (dict(k=8, emb_dims=64, time_steps_enc=3, num_heads=4, k_scales=[4, 8, 24], dropout=0.0), "fd_train.npz"),
    "B": (dict(k=20, emb_dims=96, time_steps_enc=4, num_heads=4, k_scales=[10, 20, 40], dropout=0.0), "fd_train_b.npz"),
}


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(U.dev())


def _step_ref(x, raw, state, eif):
    """One neuron step of train() mode restated in torch ops (hard spike forward, soft surrogate backward) for the cases that have
    no reference run: -> spikes, (membrane, threshold, refractory), u.  The arithmetic lives in oracle/train_path.py, where the
    whole-model oracle uses it (and tests/test_oracle_golden.py pins it on the reference's runs)."""
    from oracle import train_path as TP
    assert eif == ("delta_T" in raw)
    return TP.neuron_step_train(x, raw, state)


# ================================================================================================ ops against reference runs
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lif", "eif"])
def test_neuron_step_three_chained_steps_against_reference_run(kind):
    """Bars of test_training_neuron_loop_forward_backward_against_reference_run: spikes (and the carried state's spike-driven parts)
    equal, grad_x rtol 2e-5 / atol 1e-6, parameter gradients rtol 1e-4 / atol 2e-5; raw parameters outside a clamp get exactly 0;
    threshold_adapt / refractory_decay get no gradient at all, threshold_base only on the step without a carried state."""
    from sapcu_amd import fd_train
    g = golden("fd_neuron_step_train.npz")
    names = EIF_NAMES if kind == "eif" else LIF_NAMES
    raw_h = {n: g["%s/raw:%s" % (kind, n)] for n in names}
    clamps = {"membrane_decay": (0.1, 0.99), "delta_T": (0.1, 5.0), "theta_rh": (0.1, 2.0)}
    for n, (lo, hi) in clamps.items():
        if n in raw_h:
            assert (raw_h[n] < lo).any() and (raw_h[n] > hi).any(), n          # the fixture does reach beyond every clamp
    state = None
    for t in range(3):
        tag = "%s/t%d:" % (kind, t)
        raw = {n: _dev(v).requires_grad_(True) for n, v in raw_h.items()}
        x = _dev(g[tag + "x"]).requires_grad_(True)
        sp, state, pre = fd_train.neuron_step_train(x, raw, state)
        assert torch.equal(sp.detach().cpu(), torch.from_numpy(g[tag + "spikes"])), tag
        assert set(np.unique(g[tag + "spikes"])) == {0.0, 1.0}
        # (an EIF membrane reaches delta_T e^5 ~ 700: one ulp of the exponential is 6e-5 there, hence the relative part)
        np.testing.assert_allclose(pre.cpu().numpy(), g[tag + "preact"], rtol=2e-6, atol=2e-6, err_msg=tag)
        for s, key in zip(state, ("membrane", "threshold", "refractory")):
            np.testing.assert_allclose(s.cpu().numpy(), g[tag + key], rtol=2e-6, atol=2e-6, err_msg=tag + key)
        assert torch.equal(state[2].cpu() > 0, torch.from_numpy(g[tag + "refractory"]) > 0)
        (sp * _dev(g[tag + "g"])).sum().backward()
        print("%s grad_x max err %.3g" % (tag, float(np.abs(x.grad.cpu().numpy() - g[tag + "gx"]).max())))
        np.testing.assert_allclose(x.grad.cpu().numpy(), g[tag + "gx"], rtol=2e-5, atol=1e-6, err_msg=tag)
        none = {str(n) for n in g[tag + "none"]}
        assert none == ({"threshold_adapt", "refractory_decay"} | ({"threshold_base"} if t > 0 else set())), (tag, none)
        for n in names:
            if n in none and n != "threshold_base":
                assert raw[n].grad is None, (tag, n)
            elif n in none:                                                 # a carried threshold: the op reports exact zeros
                assert raw[n].grad is not None and not bool(raw[n].grad.any()), (tag, n)
            else:
                got, want = raw[n].grad.cpu().numpy(), g[tag + "g:" + n]
                np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5, err_msg=tag + n)
                if n in clamps:
                    out = (raw_h[n] < clamps[n][0]) | (raw_h[n] > clamps[n][1])
                    assert not got[out].any() and not want[out].any(), (tag, n)
        if t == 0:
            assert not raw["membrane_decay"].grad.any()                    # the zero state: exactly zero, as for snn_fc


@pytest.mark.gpu
def test_edgeconv_block_against_reference_run():
    """feature -> Conv2d(128, 128) -> BatchNorm (train) -> LeakyReLU -> max over 8 neighbours -> EIF step, P = 4, M = 16, on {0,1}
    inputs (arg-max ties occur: the fixture counts them).  Block output <= 2e-4, spikes equal, gradients
    |d| <= 5e-3 max|ref| + 5e-5 max over all tensors (test_training_transformer_block_forward_backward_against_reference_run)."""
    from sapcu_amd import fd_train
    g = golden("fd_edgeconv_train.npz")
    assert int(g["argmax_ties"]) > 0
    x = _dev(g["x"]).requires_grad_(True)
    w, gamma, beta = (_dev(g[n]).requires_grad_(True) for n in ("w", "gamma", "beta"))
    raw = {n: _dev(g["raw:" + n]).requires_grad_(True) for n in EIF_NAMES}
    rm, rv, nt = torch.zeros(128, device=U.dev()), torch.ones(128, device=U.dev()), torch.zeros((), dtype=torch.int64, device=U.dev())
    z = fd_train.conv_bn_lrelu_max(x, w, gamma, beta, group=8, idx=_dev(g["idx"]), running=(rm, rv, nt, 0.1))
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


# ================================================================================================ ops against torch, bit for bit
def _feature_ref(x, idx, P, M, kk):
    xv = x.view(P, M, -1)
    nb = torch.gather(xv.unsqueeze(1).expand(P, M, M, xv.shape[-1]), 2, idx.long().unsqueeze(-1).expand(P, M, kk, xv.shape[-1]))
    return torch.cat([nb - xv.unsqueeze(2), nb], dim=-1).reshape(P * M * kk, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("P,M,kk,C", [(3, 7, 5, 96), (2, 48, 20, 128), (1, 1, 1, 64)])
def test_edge_feature_and_fused_max_equal_torch_on_binary_inputs(P, M, kk, C):
    """{0,1} inputs and integer-valued upstream gradients: every sum is exact, so values and gradients are torch.equal whatever the
    summation order; arg-max ties (constant with binary features) go to the first neighbour; two runs are bit-identical."""
    from sapcu_amd import _lib, fd_train
    lib = _lib.load()
    rng = np.random.default_rng(P * 1000 + M)
    xh = torch.from_numpy((rng.uniform(size=(P * M, C)) > 0.5).astype(np.float32))
    idx = torch.from_numpy(rng.integers(0, M, (P, M, kk)).astype(np.int32))
    go = torch.from_numpy(rng.integers(-3, 4, (P * M * kk, 2 * C)).astype(np.float32))
    xr = xh.clone().requires_grad_(True)
    fr = _feature_ref(xr, idx, P, M, kk)
    fr.backward(go)
    runs = []
    for _ in range(2):
        xd = xh.to(U.dev()).requires_grad_(True)
        fdv = fd_train.edge_feature(xd, idx.to(U.dev()))
        fdv.backward(go.to(U.dev()))
        runs.append((fdv.detach().cpu(), xd.grad.cpu()))
    assert fd_train.take_bad_index_count() == 0
    assert torch.equal(runs[0][0], fr.detach()) and torch.equal(runs[0][1], xr.grad)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0][:, C:], fr.detach()[:, C:])                      # second half: the neighbour, not the centre
    padded = fd_train.edge_feature_forward(xh.to(U.dev()), idx.to(U.dev()), 2 * C + 32).cpu()
    assert torch.equal(padded[:, :2 * C], fr.detach()) and not bool(padded[:, 2 * C:].any())

    # fused BatchNorm-apply + LeakyReLU + max over kk on the binary feature rows (statistics from sapcu_fd_bn_stats)
    y = runs[0][0][:, :C].abs().contiguous()                                       # {0,1}
    rows = y.shape[0]
    yd = y.to(U.dev())
    gamma, beta = _dev(rng.uniform(-1.5, 1.5, C).astype(np.float32)), _dev(rng.normal(0.0, 0.5, C).astype(np.float32))
    mean, var, invstd = (torch.empty(C, device=U.dev()) for _ in range(3))
    need = int(lib.sapcu_fd_bn_stats_workspace_bytes(rows, C))
    ws = torch.empty(need, dtype=torch.uint8, device=U.dev())
    _lib.check(lib.sapcu_fd_bn_stats(_lib.ptr(yd), rows, C, 1e-5, _lib.ptr(mean), _lib.ptr(var), _lib.ptr(invstd), _lib.ptr(ws), need, _lib.current_stream()))
    y64 = y.double()
    np.testing.assert_allclose(mean.cpu().numpy(), y64.mean(0).numpy(), atol=1e-6)
    np.testing.assert_allclose(var.cpu().numpy(), y64.var(0, unbiased=False).numpy(), atol=1e-6)
    np.testing.assert_allclose(invstd.cpu().numpy(), (1 / torch.sqrt(y64.var(0, unbiased=False) + 1e-5)).numpy(), rtol=2e-6)
    groups = P * M
    gout = torch.from_numpy(rng.integers(-3, 4, (groups, C)).astype(np.float32))
    zr = (((y - mean.cpu()) * invstd.cpu()) * gamma.cpu() + beta.cpu()).requires_grad_(True)      # the kernel's own operation order
    act = torch.nn.functional.leaky_relu(zr, 0.2).view(groups, kk, C)
    val = act.max(dim=1)[0]
    first = (act == val.unsqueeze(1)).float().argmax(dim=1)                       # first index of the maximum
    torch.gather(act, 1, first.unsqueeze(1)).squeeze(1).backward(gout)
    outs = []
    for _ in range(2):
        out, arg = torch.empty(groups, C, device=U.dev()), torch.empty(groups, C, dtype=I32, device=U.dev())
        gz = torch.empty(rows, C, device=U.dev())
        _lib.check(lib.sapcu_fd_bn_lrelu_max_forward(_lib.ptr(yd), groups, kk, C, _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(gamma), _lib.ptr(beta),
                                                     _lib.ptr(out), _lib.ptr(arg), _lib.current_stream()))
        _lib.check(lib.sapcu_fd_bn_lrelu_max_backward(_lib.ptr(yd), _lib.ptr(gout.to(U.dev())), _lib.ptr(arg), groups, kk, C, _lib.ptr(mean),
                                                      _lib.ptr(invstd), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(gz), _lib.current_stream()))
        outs.append((out.cpu(), arg.cpu(), gz.cpu()))
    assert torch.equal(outs[0][0], val.detach()) and torch.equal(outs[0][1].long(), first) and torch.equal(outs[0][2], zr.grad)
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    if kk > 1:
        assert int(((act == val.unsqueeze(1)).sum(1) > 1).sum()) > 0                # ties did occur


# ================================================================================================ the whole model, teacher-forced
def _config(cfg):
    import sapcu_amd
    from sapcu_amd import testing as T
    kw, fname = CONFIGS[cfg]
    g = golden(fname)
    g = {k[len(cfg) + 1:]: g[k] for k in g.files}
    shell = sapcu_amd.TrainableSNNDistanceEstimation(**kw)
    sd = T.training_state_dict(shell.state_dict(), int(g["weight_seed"]))
    # the fixture's one departure from training_state_dict (make_fd_train_fixtures.py: with thresholds ~ N(0, 0.4^2) every neuron
    # of snn_fc fires for every patch and the decoder sees P identical rows)
    sd["encoder.snn_fc.threshold_base"] = sd["encoder.snn_fc.threshold_base"] + float(g["fc_threshold_shift"])
    names = [str(n) for n in g["names"]]
    return kw, g, sd, names


def _forced_run(kw, g, sd, names, with_spikes):
    from sapcu_amd import fd_train
    P, M, Tn, emb = int(g["P"]), int(g["M"]), kw["time_steps_enc"], kw["emb_dims"]
    p = {n: sd[n].to(U.dev()).clone().requires_grad_(True) for n in names}
    p.update({n: v.to(U.dev()).clone() for n, v in sd.items() if n not in p})
    spikes = torch.from_numpy(np.unpackbits(g["spikes"], axis=-1)[..., :960].astype(np.float32))          # [T, P*M, 960]
    fc = torch.from_numpy(np.unpackbits(g["fc_spikes"], axis=-1)[..., :emb].astype(np.float32))
    force = None
    if with_spikes:
        force = {"fc": fc.to(U.dev())}
        for t in range(Tn):
            for b, (lo, hi) in enumerate(((0, 64), (64, 192), (192, 448), (448, 960))):
                force[(t, b)] = spikes[t, :, lo:hi].contiguous().to(U.dev())
    taps = {}
    pred = fd_train.fd_train_forward(p, _dev(g["input"]), kw["k"], tuple(kw["k_scales"]), Tn, kw["num_heads"], knn=_dev(g["knn"].astype(np.int32)),
                                     momentum=0.1, dropout=0.0, taps=taps, force_spikes=force)
    loss = fd_train.distance_loss(pred, _dev(g["gt"]))
    loss.backward()
    assert fd_train.take_bad_index_count() == 0
    own = torch.stack([torch.cat([(u > 0).float() for u in taps["preact"][4 * t:4 * t + 4]], dim=1) for t in range(Tn)]).cpu()
    margin = torch.stack([torch.cat([u.abs() for u in taps["preact"][4 * t:4 * t + 4]], dim=1) for t in range(Tn)]).cpu()
    own_fc, margin_fc = (taps["fc_preact"][0] > 0).float().cpu(), taps["fc_preact"][0].abs().cpu()
    flip = torch.cat([(own != spikes).flatten(), (own_fc != fc).flatten()])
    mar = torch.cat([margin.flatten(), margin_fc.flatten()])
    return p, pred.detach().cpu(), float(loss.detach()), taps, flip, mar


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_training_step_of_whole_fd_model_teacher_forced_on_the_reference_run(cfg):
    """One training step (train() mode, dropout 0) forced on the reference's kNN tables and hard spikes: forward values come from
    the reference's spikes, derivatives from the device's own pre-activations.  Bars of the fn whole-model test: taps, prediction,
    loss <= 2e-4; gradients by check_fn_train_grads at 2e-2 / 5e-5 (sampled rows, total and per-row norms for the three large
    tensors); grad-is-None and exactly-zero sets equal to the reference's; BatchNorm buffers within 1e-5, num_batches_tracked equal.
    The device's own spikes (u > 0) against the reference's: share of differing ones <= 0.01 and none with |u| > 1e-4
    (test_training_hard_spike_flips_sit_on_their_thresholds).  A second run forced on the tables only equals the first bit for
    bit when no spike differs."""
    from test_oracle_golden import check_fn_train_grads
    kw, g, sd, names = _config(cfg)
    p, pred, loss, taps, flip, mar = _forced_run(kw, g, sd, names, True)
    print("config %s: %d of %d spikes differ from the reference's (largest |u| among them %.3g; the fixture's smallest margin %.3g)"
          % (cfg, int(flip.sum()), flip.numel(), float(mar[flip].max()) if flip.any() else 0.0, float(g["margin"])))
    assert float(flip.float().mean()) <= 0.01
    assert not bool(flip[mar > 1e-4].any()), "a spike away from its threshold differs: an arithmetic defect, not a rounding flip"
    e_pool = float((torch.stack(taps["pooled"]).cpu() - torch.from_numpy(g["pooled"])).abs().max())
    e_int = float((taps["integrated"][0].cpu() - torch.from_numpy(g["integrated"])).abs().max())
    e_pred = float((pred - torch.from_numpy(g["pred"])).abs().max())
    print("config %s: pooled %.3g, integrated %.3g, prediction %.3g, loss %.3g" % (cfg, e_pool, e_int, e_pred, abs(loss - float(g["loss"]))))
    assert e_pool <= 2e-4 and e_int <= 2e-4 and e_pred <= 2e-4 and abs(loss - float(g["loss"])) <= 2e-4
    emb = kw["emb_dims"]
    assert torch.equal(taps["enc"][0].cpu(), torch.from_numpy(np.unpackbits(g["fc_spikes"], axis=-1)[..., :emb].astype(np.float32)))
    assert {n for n in names if p[n].grad is None} == {str(n) for n in g["grad_none"]}
    assert {n for n in names if p[n].grad is not None and not bool(p[n].grad.any())} == {str(n) for n in g["grad_zero"]}
    graded = [n for n in names if p[n].grad is not None]
    worst = check_fn_train_grads(g, p, graded, 2e-2, 5e-5)
    print("config %s: worst gradient error relative to its bar's scale %.3g" % (cfg, worst))
    big = [n for n in names if ("grn:" + n) in g]
    assert sorted(big) == ["encoder.conv_blocks.1.0.weight", "encoder.conv_blocks.2.0.weight", "encoder.multi_scale_conv.0.weight"]
    peak = max(float(np.abs(g[("g:" if ("g:" + n) in g else "gs:") + n]).max()) for n in graded)
    for n in big:
        got = np.linalg.norm(p[n].grad.detach().cpu().numpy().reshape(p[n].shape[0], -1).astype(np.float64), axis=1)
        assert np.abs(got - g["grn:" + n]).max() <= 2e-2 * g["grn:" + n].max() + 5e-5 * peak * math.sqrt(p[n][0].numel()), n
    for n, v in sd.items():
        if n in names:
            continue
        if n.endswith("num_batches_tracked"):
            assert int(p[n]) == int(g["buf:" + n]), n
        else:
            np.testing.assert_allclose(p[n].cpu().numpy(), g["buf:" + n], rtol=0, atol=1e-5, err_msg=n)
    assert int(p["encoder.scale_fusion.1.num_batches_tracked"]) == kw["time_steps_enc"]
    p2, pred2, loss2, _, flip2, _ = _forced_run(kw, g, sd, names, False)
    assert torch.equal(flip, flip2)
    if not flip.any():
        assert torch.equal(pred, pred2) and loss == loss2
        for n in names:
            assert (p[n].grad is None and p2[n].grad is None) or torch.equal(p[n].grad, p2[n].grad), n


# ================================================================================================ free running, epoch
@pytest.mark.gpu
def test_free_running_step_obeys_the_library_tie_rule_and_gives_finite_gradients():
    """Own kNN tables: not compared with the reference.  With hard spikes the squared distances between spike vectors are small
    integers, and in a reference run with these weights (B = 8, M = 16, k = 8) between 60 % and 98 % of the rows of blocks 1-3 have
    an exact tie at rank k, where torch.topk's choice is unspecified.  What is checked: the tables are sapcu_patch_knn's — scores
    descending, equal scores by ascending index — the step runs, and every gradient is finite."""
    import sapcu_amd
    from sapcu_amd import fd_train, testing as T
    kw = dict(CONFIGS["A"][0])
    model = sapcu_amd.TrainableSNNDistanceEstimation(**kw)
    model.load_state_dict(T.training_state_dict(model.state_dict(), 11))
    model = model.to(U.dev()).train()
    g = golden("fd_train.npz")
    x, gt = _dev(g["A/input"]), _dev(g["A/gt"])
    taps = {}
    pred = model(x, taps=taps)
    loss, d = model.compute_loss(pred, gt)
    loss.backward()
    assert fd_train.take_bad_index_count() == 0
    assert pred.shape == (8,) and bool(torch.isfinite(pred).all()) and math.isfinite(d["total_loss"])
    P, M, kk = 8, 16, 8
    ties = 0
    for t in range(3):
        tab = taps["knn"][t].cpu().long()
        assert tab.shape == (3, P, M, kk) and int(tab.min()) >= 0 and int(tab.max()) < M
        for b in range(3):
            f = taps["spikes"][4 * t + b].cpu().view(P, M, -1).double()                # the block's input: spikes of block b
            score = -((f.unsqueeze(2) - f.unsqueeze(1)) ** 2).sum(-1)                  # small integers: exact
            s = torch.gather(score, 2, tab[b])
            assert bool((s[..., :-1] >= s[..., 1:]).all())
            same = s[..., :-1] == s[..., 1:]
            assert bool((tab[b][..., :-1][same] < tab[b][..., 1:][same]).all())
            srt = score.sort(dim=-1, descending=True)[0]
            assert torch.equal(s, srt[..., :kk])                                       # the k best scores
            ties += int((srt[..., kk - 1] == srt[..., kk]).sum())
    print("free run: %d of %d rows tie at rank k" % (ties, 9 * P * M))
    for n, prm in model.named_parameters():
        if "threshold_adapt" in n or "refractory_decay" in n:
            assert prm.grad is None, n
        else:
            assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), n
    model.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(model(x)).all())                                    # the inherited engine, on the same weights


@pytest.mark.gpu
def test_fd_epoch_is_reproducible_learns_and_leaves_an_inference_model():
    """fn_trainer.run_epoch over 12 SyntheticFdPatches batches (B = 2, N = 8, M = 24; k = 8, emb_dims = 64, T = 3; AdamW,
    grad_clip = 0.1, clamp_parameters, dropout 0.1 from a seeded generator), twice."""
    import sapcu_amd
    from sapcu_amd import fd_trainer, fn_trainer
    kw = dict(k=8, emb_dims=64, time_steps_enc=3, num_heads=4, k_scales=[4, 8, 16], dropout=0.1)
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        model = sapcu_amd.TrainableSNNDistanceEstimation(**kw).to(U.dev())
        model.dropout_generator = torch.Generator(device=U.dev()).manual_seed(7)
        opt = torch.optim.AdamW(model.parameters(), lr=3e-3)
        trainer = fd_trainer.Trainer(model, opt, device=U.dev(), grad_clip=0.1)
        loader = fd_trainer.SyntheticFdPatches(batches=12, batch_size=2, patches=8, points=24, seed=3)
        it, losses, st = fn_trainer.run_epoch(trainer, loader, clamp_parameters=True)
        assert it == 12 and st["skipped"] == 0 and len(losses) == 12 and all(np.isfinite(losses))
        runs.append((losses, {n: q.detach().cpu().clone() for n, q in model.named_parameters()},
                     {n: b.detach().cpu().clone() for n, b in model.named_buffers()}, model))
    print("losses: " + " ".join("%.5f" % v for v in runs[0][0]))
    assert runs[0][0] == runs[1][0]
    for k in (1, 2):
        for n in runs[0][k]:
            assert torch.equal(runs[0][k][n], runs[1][k][n]), n
    for n, q in runs[0][1].items():
        for key, (lo, hi) in (("membrane_decay", (0.1, 0.99)), ("threshold_adapt", (0.001, 0.1)), ("refractory_decay", (0.1, 0.95))):
            if key in n:
                assert float(q.min()) >= lo and float(q.max()) <= hi, n
    assert int(runs[0][2]["encoder.scale_fusion.1.num_batches_tracked"]) == 12 * 3
    assert np.mean(runs[0][0][-4:]) < np.mean(runs[0][0][:4]), runs[0][0]
    model = runs[0][3].eval()
    base = sapcu_amd.EnhancedSNNDistanceEstimation(**kw)
    base.load_state_dict(model.state_dict(), strict=True)
    base = base.to(U.dev())
    x = next(iter(fd_trainer.SyntheticFdPatches(batches=1, batch_size=2, patches=8, points=24, seed=9)))["input"].to(U.dev())
    with torch.no_grad():
        a, b = model(x), base(x)
    assert a.shape == (2, 8) and torch.equal(a, b)
    m = trainer.evaluate(fd_trainer.SyntheticFdPatches(batches=2, batch_size=2, patches=8, points=24, seed=10), return_metrics=True)
    assert math.isfinite(m[0]) and {"mae", "mse", "relative_error", "total_loss", "distance_loss"} <= set(m[1])


# ================================================================================================ the memory contract
FD_CASES, FD_REFUSALS = [], []


def _B():
    import test_gpu_bounds as B
    return B


def _fd_case(id_, entry_points, sizers, build):
    FD_CASES.append(_B().Case(id_, tuple(entry_points), tuple(sizers), build))


def _neuron_case(rows, ch, eif, carried, forced, ws_off):
    def build(A):
        B = _B()
        _lib, lib = B._lib_()
        rng = np.random.default_rng(rows * 7 + ch)
        names = EIF_NAMES if eif else LIF_NAMES
        draw = {"membrane_decay": (0.0, 1.1), "threshold_adapt": (-0.02, 0.15), "refractory_decay": (0.05, 1.0), "threshold_base": (0.2, 1.2),
                "delta_T": (0.05, 5.5), "theta_rh": (0.0, 2.3)}
        raw = {n: rng.uniform(*draw[n], ch).astype(np.float32) for n in names}
        x, g = rng.normal(0.6, 1.0, (rows, ch)).astype(np.float32), rng.normal(0, 1, (rows, ch)).astype(np.float32)
        st = None
        if carried:
            spk = (rng.uniform(size=(rows, ch)) > 0.7).astype(np.float32)
            st = [rng.uniform(0, 1.5, (rows, ch)).astype(np.float32) * (1 - spk), rng.normal(0.8, 0.3, (rows, ch)).astype(np.float32), spk * 0.7]
        frc = (rng.uniform(size=(rows, ch)) > 0.5).astype(np.float32) if forced else None
        X, G = A.inp(x, offset=4, name="x"), A.inp(g, offset=4, name="grad_spikes")
        R = {n: A.inp(raw[n], offset=4, name=n) for n in names}
        ST = [A.inp(s, offset=4, name="state%d" % i) for i, s in enumerate(st)] if carried else [None] * 3
        FR = A.inp(frc, offset=4, name="force_spikes") if forced else None
        need = int(lib.sapcu_fd_neuron_step_workspace_bytes(rows, ch))
        assert need > 0
        ws = A.ws(need, offset=ws_off, tile_row_bytes=4 * ch, name="neuron step workspace")
        outs = {n: A.out((rows, ch), F32, offset=4, name=n) for n in ("spikes", "membrane", "threshold", "refractory", "preact", "gx")}
        gnames = ("membrane_decay", "threshold_base") + (("delta_T", "theta_rh") if eif else ())
        for n in gnames:
            outs["g:" + n] = A.out((ch,), F32, offset=4, name="grad_" + n)
        Pp = B.P

        def call():
            B.ok(lib.sapcu_fd_neuron_step_forward(Pp(X), rows, ch, int(eif), *[Pp(R.get(n)) for n in EIF_NAMES], *[Pp(s) for s in ST], Pp(FR),
                                                  *[Pp(outs[n]) for n in ("spikes", "membrane", "threshold", "refractory", "preact")], B.S()))
            B.ok(lib.sapcu_fd_neuron_step_backward(Pp(X), Pp(G), rows, ch, int(eif), Pp(R["membrane_decay"]), Pp(R["threshold_base"]),
                                                   Pp(R.get("delta_T")), Pp(R.get("theta_rh")), *[Pp(s) for s in ST], Pp(outs["gx"]),
                                                   Pp(outs["g:membrane_decay"]), Pp(outs["g:threshold_base"]), Pp(outs.get("g:delta_T")),
                                                   Pp(outs.get("g:theta_rh")), Pp(ws), need, B.S()))

        def ref(o):
            xo = torch.from_numpy(x).requires_grad_(True)
            ro = {n: torch.from_numpy(raw[n]).requires_grad_(True) for n in names}
            sp, state, u = _step_ref(xo, ro, [torch.from_numpy(s) for s in st] if carried else None, eif)
            (sp * torch.from_numpy(g)).sum().backward()
            np.testing.assert_allclose(o["preact"].numpy(), u.numpy(), rtol=1e-5, atol=1e-5)
            if forced:
                assert torch.equal(o["spikes"], torch.from_numpy(frc))
            else:
                away = u.abs() > 1e-4
                assert torch.equal(o["spikes"][away], sp.detach()[away])
                for key, s in zip(("membrane", "threshold", "refractory"), state):
                    np.testing.assert_allclose(o[key][away].numpy(), s[away].numpy(), rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(o["gx"].numpy(), xo.grad.numpy(), rtol=1e-4, atol=1e-5)
            for n in gnames:
                want = ro[n].grad if ro[n].grad is not None else torch.zeros(ch)
                assert float((o["g:" + n] - want).abs().max()) <= 2e-4 * (float(want.abs().max()) + 1e-6) + 1e-4, n
        return B.built(call, outs, ref)
    _fd_case("fd_neuron_step-r%d-c%d-%s%s%s" % (rows, ch, "eif" if eif else "lif", "-carried" if carried else "", "-forced" if forced else ""),
             ["sapcu_fd_neuron_step_forward", "sapcu_fd_neuron_step_backward"], ["sapcu_fd_neuron_step_workspace_bytes"], build)


def _edge_case(P, M, kk, C, oc_x, ld_x):
    def build(A):
        B = _B()
        _lib, lib = B._lib_()
        rng = np.random.default_rng(P + M + kk + C)
        oc = 2 * C + oc_x
        ld = C + (0 if A.compact else ld_x)
        x = rng.normal(size=(P * M, C)).astype(np.float32)
        idx = rng.integers(0, M, (P, M, kk)).astype(np.int32)
        g = rng.normal(size=(P * M * kk, oc)).astype(np.float32)
        X, I, G = A.inp(x, pitch=ld, offset=4, name="x"), A.inp(idx, offset=4, name="idx"), A.inp(g, offset=4, name="grad_out")
        outs = {"feat": A.out((P * M * kk, oc), F32, offset=4, name="feature"), "gx": A.out((P * M, C), F32, pitch=ld, offset=4, name="grad_x"),
                "bad_f": A.out((1,), I32, offset=4, name="bad_count forward"), "bad_b": A.out((1,), I32, offset=4, name="bad_count backward")}

        def call():
            B.ok(lib.sapcu_fd_edge_feature_forward(B.P(X), ld, B.P(I), P, M, kk, C, oc, B.P(outs["feat"]), B.P(outs["bad_f"]), B.S()))
            B.ok(lib.sapcu_fd_edge_feature_backward(B.P(G), B.P(I), P, M, kk, C, oc, B.P(outs["gx"]), ld, B.P(outs["bad_b"]), B.S()))

        def ref(o):
            xo = torch.from_numpy(x).double().requires_grad_(True)
            f = _feature_ref(xo, torch.from_numpy(idx), P, M, kk)
            f.backward(torch.from_numpy(g[:, :2 * C]).double())
            assert torch.equal(o["feat"][:, :2 * C], f.detach().float()) and not bool(o["feat"][:, 2 * C:].any())
            np.testing.assert_allclose(o["gx"].numpy(), xo.grad.numpy(), rtol=1e-5, atol=1e-5)
            assert int(o["bad_f"]) == 0 and int(o["bad_b"]) == 0
        return B.built(call, outs, ref)
    _fd_case("fd_edge_feature-P%d-M%d-k%d-C%d-oc+%d-ld+%d" % (P, M, kk, C, oc_x, ld_x),
             ["sapcu_fd_edge_feature_forward", "sapcu_fd_edge_feature_backward"], [], build)


def _bn_max_case(groups, kk, ch, ws_off):
    def build(A):
        B = _B()
        _lib, lib = B._lib_()
        rng = np.random.default_rng(groups + kk + ch)
        rows = groups * kk
        y = rng.normal(0.3, 1.2, (rows, ch)).astype(np.float32)
        gamma, beta = rng.uniform(-1.5, 1.5, ch).astype(np.float32), rng.normal(0.2, 0.5, ch).astype(np.float32)
        go = rng.normal(size=(groups, ch)).astype(np.float32)
        Y, Ga, Be, GO = A.inp(y, offset=4, name="y"), A.inp(gamma, offset=4, name="gamma"), A.inp(beta, offset=4, name="beta"), A.inp(go, offset=4, name="grad_out")
        need = int(lib.sapcu_fd_bn_stats_workspace_bytes(rows, ch))
        assert need > 0
        ws = A.ws(need, offset=ws_off, tile_row_bytes=8 * ch, name="bn stats workspace")
        o = {n: A.out((ch,), F32, offset=4, name=n) for n in ("mean", "var", "invstd")}
        o["out"], o["arg"], o["gz"] = A.out((groups, ch), F32, offset=4, name="out"), A.out((groups, ch), I32, offset=4, name="argmax"), \
            A.out((rows, ch), F32, offset=4, name="grad_z")

        def call():
            B.ok(lib.sapcu_fd_bn_stats(B.P(Y), rows, ch, 1e-5, B.P(o["mean"]), B.P(o["var"]), B.P(o["invstd"]), B.P(ws), need, B.S()))
            B.ok(lib.sapcu_fd_bn_lrelu_max_forward(B.P(Y), groups, kk, ch, B.P(o["mean"]), B.P(o["invstd"]), B.P(Ga), B.P(Be), B.P(o["out"]), B.P(o["arg"]), B.S()))
            B.ok(lib.sapcu_fd_bn_lrelu_max_backward(B.P(Y), B.P(GO), B.P(o["arg"]), groups, kk, ch, B.P(o["mean"]), B.P(o["invstd"]), B.P(Ga), B.P(Be),
                                                    B.P(o["gz"]), B.S()))

        def ref(r):
            y64 = torch.from_numpy(y).double()
            mean, var = y64.mean(0), y64.var(0, unbiased=False)
            z = ((y64 - mean) / torch.sqrt(var + 1e-5) * torch.from_numpy(gamma).double() + torch.from_numpy(beta).double()).requires_grad_(True)
            val, arg = torch.nn.functional.leaky_relu(z, 0.2).view(groups, kk, ch).max(dim=1)
            val.backward(torch.from_numpy(go).double())
            tol = lambda want: 2e-5 * max(1.0, float(want.abs().max()))
            for n, want in (("mean", mean), ("var", var), ("invstd", 1 / torch.sqrt(var + 1e-5)), ("out", val.detach())):
                assert float((r[n].double() - want).abs().max()) <= tol(want), n
            assert torch.equal(r["arg"].long(), arg)                                     # continuous values: no ties
            assert float((r["gz"].double() - z.grad).abs().max()) <= tol(z.grad)
        return B.built(call, o, ref)
    _fd_case("fd_bn_max-g%d-k%d-c%d" % (groups, kk, ch), ["sapcu_fd_bn_stats", "sapcu_fd_bn_lrelu_max_forward", "sapcu_fd_bn_lrelu_max_backward"],
             ["sapcu_fd_bn_stats_workspace_bytes"], build)


def _make_cases():
    _neuron_case(257, 33, False, False, False, 0)
    _neuron_case(70, 96, True, True, True, 4)
    _neuron_case(1, 3, True, False, False, 0)
    _neuron_case(130, 64, False, True, False, 4)
    _edge_case(3, 7, 5, 96, 0, 3)
    _edge_case(2, 48, 20, 3, 26, 1)
    _edge_case(1, 1, 1, 64, 0, 0)
    _bn_max_case(21, 5, 96, 0)
    _bn_max_case(300, 3, 33, 8)
    _bn_max_case(2, 1, 64, 0)


_make_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("c", FD_CASES, ids=[c.id for c in FD_CASES])
def test_fd_train_bounds(c):
    """0xFF bands, 0x00 bands, dirty workspace, compact call (tests/test_gpu_bounds.py): bands intact, the four results bit-identical."""
    _B().run_protocol(c)


def _refusal(id_):
    def deco(fn):
        FD_REFUSALS.append((id_, fn))
        return fn
    return deco


def _neuron_refusal_args(A, rows=70, ch=96, short=0, ws_off=0):
    B = _B()
    _lib, lib = B._lib_()
    need = int(lib.sapcu_fd_neuron_step_workspace_bytes(rows, ch))
    t = lambda name: A.inp(np.ones((rows, ch), np.float32), name=name)
    prm = [A.inp(np.full(ch, 0.5, np.float32), name="param%d" % i) for i in range(6)]
    outs = [A.out((rows, ch), F32, name="out%d" % i) for i in range(6)] + [A.out((ch,), F32, name="gparam%d" % i) for i in range(4)]
    ws = A.ws(need - short, offset=ws_off, name="neuron step workspace")
    return B, lib, t, prm, outs, ws, need - short


@_refusal("neuron-backward-workspace-one-byte-short")
def _r_nws(A):
    B, lib, t, prm, o, ws, nb = _neuron_refusal_args(A, short=1)
    return lib.sapcu_fd_neuron_step_backward(B.P(t("x")), B.P(t("g")), 70, 96, 1, B.P(prm[0]), B.P(prm[3]), B.P(prm[4]), B.P(prm[5]), None, None, None,
                                             B.P(o[5]), *[B.P(q) for q in o[6:]], B.P(ws), nb, B.S())


@_refusal("neuron-backward-workspace-2-byte-aligned")
def _r_nal(A):
    B, lib, t, prm, o, ws, nb = _neuron_refusal_args(A, ws_off=2)
    return lib.sapcu_fd_neuron_step_backward(B.P(t("x")), B.P(t("g")), 70, 96, 1, B.P(prm[0]), B.P(prm[3]), B.P(prm[4]), B.P(prm[5]), None, None, None,
                                             B.P(o[5]), *[B.P(q) for q in o[6:]], B.P(ws), nb, B.S())


@_refusal("neuron-forward-state-given-in-part")
def _r_nstate(A):
    B, lib, t, prm, o, ws, nb = _neuron_refusal_args(A)
    return lib.sapcu_fd_neuron_step_forward(B.P(t("x")), 70, 96, 0, *[B.P(q) for q in prm], B.P(t("membrane")), None, B.P(t("refractory")), None,
                                            *[B.P(q) for q in o[:5]], B.S())


@_refusal("neuron-forward-eif-without-theta_rh")
def _r_neif(A):
    B, lib, t, prm, o, ws, nb = _neuron_refusal_args(A)
    return lib.sapcu_fd_neuron_step_forward(B.P(t("x")), 70, 96, 1, *[B.P(q) for q in prm[:5]], None, None, None, None, None,
                                            *[B.P(q) for q in o[:5]], B.S())


def _edge_refusal(oc, ld, m=7, kk=5, with_bad=True):
    def run(A):
        B = _B()
        _lib, lib = B._lib_()
        P, C = 2, 8
        g = A.inp(np.ones((P * m * kk, max(oc, 1)), np.float32), name="grad_out")
        idx = A.inp(np.zeros((P, m, kk), np.int32), name="idx")
        gx, bad = A.out((P * m, C), F32, name="grad_x"), A.out((1,), I32, name="bad_count")
        return lib.sapcu_fd_edge_feature_backward(B.P(g), B.P(idx), P, m, kk, C, oc, B.P(gx), ld, B.P(bad) if with_bad else None, B.S())
    return run


_refusal("edge-backward-out_channels-below-2c")(_edge_refusal(15, 8))
_refusal("edge-backward-ld_grad-below-c")(_edge_refusal(16, 7))
_refusal("edge-backward-null-bad_count")(_edge_refusal(16, 8, with_bad=False))
_refusal("edge-backward-inverse-table-beyond-lds")(_edge_refusal(16, 8, m=128, kk=70))


@_refusal("edge-forward-ldx-below-c")
def _r_eldx(A):
    B = _B()
    _lib, lib = B._lib_()
    x, idx = A.inp(np.ones((14, 8), np.float32), name="x"), A.inp(np.zeros((2, 7, 5), np.int32), name="idx")
    out = A.out((70, 16), F32, name="feature")
    return lib.sapcu_fd_edge_feature_forward(B.P(x), 7, B.P(idx), 2, 7, 5, 8, 16, B.P(out), None, B.S())


def _bn_refusal(short, ws_off):
    def run(A):
        B = _B()
        _lib, lib = B._lib_()
        rows, ch = 300, 33
        need = int(lib.sapcu_fd_bn_stats_workspace_bytes(rows, ch))
        y = A.inp(np.ones((rows, ch), np.float32), name="y")
        o = [A.out((ch,), F32, name="stat%d" % i) for i in range(3)]
        ws = A.ws(need - short, offset=ws_off, name="bn stats workspace")
        return lib.sapcu_fd_bn_stats(B.P(y), rows, ch, 1e-5, *[B.P(q) for q in o], B.P(ws), need - short, B.S())
    return run


_refusal("bn_stats-workspace-one-byte-short")(_bn_refusal(1, 0))
_refusal("bn_stats-workspace-4-byte-aligned")(_bn_refusal(0, 4))


@_refusal("bn_lrelu_max-zero-group-size")
def _r_kk0(A):
    B = _B()
    _lib, lib = B._lib_()
    y, v = A.inp(np.ones((8, 4), np.float32), name="y"), [A.inp(np.ones(4, np.float32), name="v%d" % i) for i in range(4)]
    out, arg = A.out((4, 4), F32, name="out"), A.out((4, 4), I32, name="argmax")
    return lib.sapcu_fd_bn_lrelu_max_forward(B.P(y), 4, 0, 4, *[B.P(q) for q in v], B.P(out), B.P(arg), B.S())


def _bn_max_bwd_refusal(kk, with_arg):
    def run(A):
        B = _B()
        _lib, lib = B._lib_()
        y, go = A.inp(np.ones((8, 4), np.float32), name="y"), A.inp(np.ones((4, 4), np.float32), name="grad_out")
        v = [A.inp(np.ones(4, np.float32), name="v%d" % i) for i in range(4)]
        arg = A.inp(np.zeros((4, 4), np.int32), name="argmax")
        gz = A.out((8, 4), F32, name="grad_z")
        return lib.sapcu_fd_bn_lrelu_max_backward(B.P(y), B.P(go), B.P(arg) if with_arg else None, 4, kk, 4, *[B.P(q) for q in v], B.P(gz), B.S())
    return run


_refusal("bn_lrelu_max-backward-null-argmax")(_bn_max_bwd_refusal(2, False))
_refusal("bn_lrelu_max-backward-zero-group-size")(_bn_max_bwd_refusal(0, True))


@pytest.mark.gpu
@pytest.mark.parametrize("r", FD_REFUSALS, ids=[r[0] for r in FD_REFUSALS])
def test_fd_train_refusal_launches_nothing(r):
    from guarded import Arena
    id_, run = r
    A = Arena("guard", 0xFF, U.dev())
    rc = run(A)
    torch.cuda.synchronize()
    assert rc == -1, "%s returned %d, expected SAPCU_ERR_ARG" % (id_, rc)
    A.check()
    for gd in A.outs + A.wss:
        assert bool((gd.payload_bits() == 0xFF).all()), "%s: %s was written by a refused call" % (id_, gd.name)


@pytest.mark.gpu
def test_edge_feature_counts_indices_outside_their_patch_and_the_trainer_fails_the_step():
    """An index outside [0, m): the forward writes zeros for that edge, the backward gives it no gradient, both count it, and
    nothing outside the buffers is touched (guard bands)."""
    from guarded import Arena
    from sapcu_amd import fd_train
    B = _B()
    _lib, lib = B._lib_()
    P, M, kk, C = 2, 7, 5, 8
    rng = np.random.default_rng(0)
    idx = rng.integers(0, M, (P, M, kk)).astype(np.int32)
    idx[0, 3, 2], idx[1, 6, 4], idx[1, 0, 0] = M, -1, 1 << 30
    A = Arena("guard", 0xFF, U.dev())
    x, I = A.inp(rng.normal(size=(P * M, C)).astype(np.float32), name="x"), A.inp(idx, name="idx")
    g = A.inp(np.ones((P * M * kk, 2 * C), np.float32), name="grad_out")
    feat, gx = A.out((P * M * kk, 2 * C), F32, name="feature"), A.out((P * M, C), F32, name="grad_x")
    bf, bb = A.out((1,), I32, name="bad forward"), A.out((1,), I32, name="bad backward")
    B.ok(lib.sapcu_fd_edge_feature_forward(B.P(x), C, B.P(I), P, M, kk, C, 2 * C, B.P(feat), B.P(bf), B.S()))
    B.ok(lib.sapcu_fd_edge_feature_backward(B.P(g), B.P(I), P, M, kk, C, 2 * C, B.P(gx), C, B.P(bb), B.S()))
    torch.cuda.synchronize()
    A.check()
    assert int(bf) == 3 and int(bb) == 3
    f = feat.cpu().view(P, M, kk, 2 * C)
    assert not bool(f[0, 3, 2].any()) and not bool(f[1, 6, 4].any()) and not bool(f[1, 0, 0].any()) and bool(f[0, 3, 1].any())
    assert bool(torch.isfinite(gx).all())
    xd = x.clone().contiguous().requires_grad_(True)
    fd_train.take_bad_index_count()
    fd_train.edge_feature(xd, I.contiguous()).sum().backward()
    assert fd_train.take_bad_index_count() == 3 and fd_train.take_bad_index_count() == 0


@pytest.mark.gpu
def test_fused_max_propagates_nan_like_torch_max():
    """A NaN among the kk rows is the result, as torch.max(dim) gives it (the trainer's finite check on the loss then sees it), and
    the arg-max is the first NaN row."""
    from sapcu_amd import _lib
    lib = _lib.load()
    groups, kk, C = 3, 4, 5
    y = torch.arange(groups * kk * C, dtype=F32).view(groups * kk, C) * 0.01
    y[1 * kk + 2, 3] = float("nan")                                                  # group 1, row 2
    y[1 * kk + 3, 3] = float("nan")
    y[2 * kk + 0, 0] = float("nan")                                                  # group 2, its first row
    yd = y.to(U.dev())
    one, zero = torch.ones(C, device=U.dev()), torch.zeros(C, device=U.dev())
    out, arg = torch.empty(groups, C, device=U.dev()), torch.empty(groups, C, dtype=I32, device=U.dev())
    _lib.check(lib.sapcu_fd_bn_lrelu_max_forward(_lib.ptr(yd), groups, kk, C, _lib.ptr(zero), _lib.ptr(one), _lib.ptr(one), _lib.ptr(zero),
                                                 _lib.ptr(out), _lib.ptr(arg), _lib.current_stream()))
    want, warg = torch.nn.functional.leaky_relu(y, 0.2).view(groups, kk, C).max(dim=1)
    assert torch.equal(torch.isnan(out.cpu()), torch.isnan(want)) and int(torch.isnan(want).sum()) == 2
    ok = ~torch.isnan(want)
    assert torch.equal(out.cpu()[ok], want[ok]) and torch.equal(arg.cpu().long()[ok], warg[ok])
    assert int(arg[1, 3]) == 2 and int(arg[2, 0]) == 0


@pytest.mark.gpu
def test_eval_train_step_eval_repacks_the_engine_and_a_checkpoint_round_trips(tmp_path):
    """eval() forward, one optimisation step, eval() forward on ONE model: the second inference uses the updated parameters (the
    packed blob follows them) and equals a fresh base-class model loaded from the state_dict bit for bit; Trainer.save_model /
    load_model / predict round-trip that state into another model."""
    import sapcu_amd
    from sapcu_amd import fd_trainer
    kw = dict(k=8, emb_dims=64, time_steps_enc=2, num_heads=4, k_scales=[4, 8], dropout=0.0)
    torch.manual_seed(1)
    model = sapcu_amd.TrainableSNNDistanceEstimation(**kw).to(U.dev())
    trainer = fd_trainer.Trainer(model, torch.optim.AdamW(model.parameters(), lr=1e-2), device=U.dev(), grad_clip=0.1)
    batches = list(fd_trainer.SyntheticFdPatches(batches=2, batch_size=2, patches=8, points=24, seed=21))
    before = trainer.predict(batches[1]).clone()
    assert not model.training and before.shape == (2, 8)
    loss, d = trainer.train_step(batches[0])
    assert model.training and math.isfinite(loss) and d["total_loss"] == d["distance_loss"]
    after = trainer.predict(batches[1])
    assert not model.training and not torch.equal(before, after)
    base = sapcu_amd.EnhancedSNNDistanceEstimation(**kw)
    base.load_state_dict(model.state_dict(), strict=True)
    with torch.no_grad():
        assert torch.equal(base.to(U.dev())(batches[1]["input"].to(U.dev())), after)
    assert float(trainer.eval_step(batches[1])) == pytest.approx(float(trainer.evaluate([batches[1]])), rel=1e-6)
    path = str(tmp_path / "fd.pt")
    trainer.save_model(path)
    torch.manual_seed(2)
    other = sapcu_amd.TrainableSNNDistanceEstimation(**kw).to(U.dev())
    tr2 = fd_trainer.Trainer(other, torch.optim.AdamW(other.parameters(), lr=1e-2), device=U.dev())
    assert not torch.equal(tr2.predict(batches[1]), after)
    tr2.load_model(path)
    assert torch.equal(tr2.predict(batches[1]), after)
    assert tr2.optimizer.state_dict()["state"].keys() == trainer.optimizer.state_dict()["state"].keys()
    with pytest.raises(NotImplementedError):
        trainer.predict(batches[1], return_uncertainty=True)


def test_patch_shapes_beyond_the_backward_lds_limit_are_refused_in_the_forward():
    """128 points x 64 neighbours: the EdgeConv backward's inverse table would pass 64 KiB of LDS; the Python ops refuse the shape
    before any launch instead of failing inside loss.backward()."""
    from sapcu_amd import fd_train
    fd_train._check_patch_shape(128, 63)
    fd_train._check_patch_shape(100, 48)                                             # the reference's shape
    with pytest.raises(ValueError):
        fd_train._check_patch_shape(128, 64)


def test_every_entry_point_of_the_fd_train_header_has_a_bounds_case():
    """The gate of tests/test_guarded.py over include/sapcu_fd_train.h: the binding's third table equals the header, every
    pointer-taking entry point has a case above, every sizer is used at exactly its size — and sapcu.h's table is untouched."""
    import test_guarded as TG
    from sapcu_amd import _lib
    from test_fd_train_host import fd_train_header_entry_points
    decl = fd_train_header_entry_points()
    assert set(decl) == set(_lib.FD_TRAIN_EXPORTS)
    assert set(TG.header_entry_points()) == set(_lib.EXPORTS) and not set(_lib.EXPORTS) & set(_lib.FD_TRAIN_EXPORTS)
    covered, used = set(), set()
    for c in FD_CASES:
        assert c.entry_points, c.id
        covered.update(c.entry_points)
        used.update(c.sizers)

    def uncovered(cov):
        return sorted(n for n, args in decl.items() if "*" in args and n not in cov)
    assert covered <= set(decl) and not uncovered(covered), uncovered(covered)
    assert uncovered(covered - {"sapcu_fd_bn_stats"}) == ["sapcu_fd_bn_stats"]                  # the gate itself
    assert {n for n in decl if n.endswith("workspace_bytes")} == used == {"sapcu_fd_neuron_step_workspace_bytes", "sapcu_fd_bn_stats_workspace_bytes"}
    assert {r[0] for r in FD_REFUSALS} >= {"neuron-backward-workspace-one-byte-short", "bn_stats-workspace-one-byte-short",
                                           "edge-backward-null-bad_count", "neuron-forward-state-given-in-part",
                                           "bn_lrelu_max-backward-null-argmax", "edge-forward-ldx-below-c", "bn_lrelu_max-zero-group-size"}
