"""fn's training step replayed as one HIP graph (train_step.GraphedTrainStep under the name fn_trainer.GraphedTrainStep, -m gpu):
the cases of tests/test_gpu_fd_graph.py that fn's trainer takes another way through — a batch skipped at the loss, a batch refused
on the host before the forward, run_epoch's learning-rate warm-up, a batch of another shape.  As there, a replay leaves parameters,
buffers and optimiser state bit for bit as the eager step does: every comparison is torch.equal or ==.  (The plain four-step
comparison is test_gpu_parity.py::test_graph_captured_training_step_equals_the_eager_step.)  Shapes: 2 clouds x 16 patches x 12
points, the model of that test, dropout off."""
import copy

import pytest
import torch

import gpu_utils as U
from test_gpu_fd_graph import _assert_equal_states, _state

KW = dict(k_values=[24, 18, 12], emb_dims=640, time_steps_enc=4, time_steps_dec=12, num_heads=8, use_snn_decoder=False, decoder_dropout=0.1)
_SHARED = {}


def _batches(n=4, batch_size=2, seed=0):
    from sapcu_amd import fn_trainer
    key = (n, batch_size, seed)
    if key not in _SHARED:
        _SHARED[key] = list(fn_trainer.SyntheticPU1K(batches=n, batch_size=batch_size, patches=16, points=12, seed=seed))
    return [dict(b) for b in _SHARED[key]]


def _fresh(lr=1e-4):
    import sapcu_amd
    from sapcu_amd import fn_trainer, testing as T
    if "sd" not in _SHARED:
        _SHARED["sd"] = T.training_state_dict(sapcu_amd.ImprovedSNNNormalEstimation(**KW).state_dict(), 0)
    model = sapcu_amd.ImprovedSNNNormalEstimation(**KW)
    model.load_state_dict(copy.deepcopy(_SHARED["sd"]), strict=True)
    model.attn_dropout = model.decoder_dropout = 0.0
    model.to(U.dev())
    opt = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=1e-4, capturable=True)
    return model, opt, fn_trainer.Trainer(model, opt, device=U.dev(), grad_clip=0.15, grad_clip_type="norm")


def _run(batches, graphed, before=None):
    """-> (results, [state after every batch], step): the eager Trainer or the graphed step (warmup=0) from the same start."""
    from sapcu_amd import fn_trainer
    model, opt, tr = _fresh()
    step = fn_trainer.GraphedTrainStep(tr, batches[0], warmup=0) if graphed else tr
    results, states = [], []
    for i, b in enumerate(batches):
        if before is not None:
            before(i)
        results.append(step.train_step(b))
        states.append(_state(model, opt))
    return results, states, step


@pytest.mark.gpu
def test_a_batch_skipped_at_the_loss_is_skipped_exactly(monkeypatch, capsys):
    """The loss of batch 2 is NaN on finite inputs: angular_loss_with_consistency is wrapped, before the capture and for the eager
    run alike, to multiply its loss by a one-element device tensor that lives outside the graph — 1.0 (exact) on the other batches.
    Both steps return (None, None) and print the eager warning once; the graph has run its backward and optimizer.step() on NaNs and
    put everything back."""
    from sapcu_amd import train
    real = train.angular_loss_with_consistency
    gate = torch.ones((1,), device=U.dev())

    def gated(*args, **kw):
        loss, conf = real(*args, **kw)
        return loss * gate[0], conf
    monkeypatch.setattr(train, "angular_loss_with_consistency", gated)

    def before(i):
        gate.fill_(float("nan") if i == 1 else 1.0)
    re, se, _ = _run(_batches(), False, before)
    assert capsys.readouterr().out.count("WARNING: NaN/Inf in loss value") == 1
    rg, sg, step = _run(_batches(), True, before)
    assert capsys.readouterr().out.count("WARNING: NaN/Inf in loss value") == 1
    assert re == rg and re[1] == (None, None) and all(r[0] is not None for r in (re[0], re[2], re[3]))
    assert (step.replays, step.eager_fallbacks) == (4, 0)
    for i in range(4):
        _assert_equal_states(se[i], sg[i], "after batch %d" % (i + 1))
    # skipped: parameters and optimiser state are those after batch 1, the BatchNorm buffers have moved
    _assert_equal_states(sg[0], sg[1], "across the skipped batch", skip_prefix=("buffer/",))
    assert any(not torch.equal(sg[0][n], sg[1][n]) for n in sg[0] if n.startswith("buffer/"))
    assert all(float(v) == 3 for n, v in sg[3].items() if n.endswith("/step"))


@pytest.mark.gpu
def test_a_non_finite_input_is_refused_before_the_replay(capsys):
    """A NaN in batch 2's `normal`: the eager step returns before its forward, so nothing moves, BatchNorm buffers included; the
    graphed step makes the same test on the host and does not replay."""
    batches = _batches()
    batches[1]["normal"] = batches[1]["normal"].clone()
    batches[1]["normal"][0, 3, 0] = float("nan")
    warning = "WARNING: NaN/Inf detected in the batch at step 1"
    re, se, _ = _run(batches, False)
    assert capsys.readouterr().out.count(warning) == 1
    rg, sg, step = _run(batches, True)
    assert capsys.readouterr().out.count(warning) == 1
    assert re == rg and re[1] == (None, None) and all(r[0] is not None for r in (re[0], re[2], re[3]))
    assert (step.replays, step.eager_fallbacks, step.captures) == (3, 0, 1)
    for i in range(4):
        _assert_equal_states(se[i], sg[i], "after batch %d" % (i + 1))
    _assert_equal_states(sg[0], sg[1], "across the refused batch")


@pytest.mark.gpu
def test_the_learning_rate_follows_the_groups_through_run_epoch():
    """warmup_steps=3 over four batches writes two new float rates into the groups (iterations 1 and 2) and then leaves the second:
    batches 1 and 2 run eager, batch 3 finds the rate of batch 2 again and is captured anew, batch 4 replays."""
    from sapcu_amd import fn_trainer
    out = []
    for graphed in (False, True):
        model, opt, tr = _fresh()
        step = fn_trainer.GraphedTrainStep(tr, _batches()[0], warmup=0) if graphed else tr
        it, losses, st = fn_trainer.run_epoch(step, _batches(), warmup_steps=3)
        assert it == 4 and st["skipped"] == 0 and len(losses) == 4
        assert not graphed or (step.captures, step.eager_fallbacks, step.replays) == (2, 2, 2)
        out.append((losses, _state(model, opt), opt.param_groups[0]["lr"]))
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2] and out[0][2] != 1e-4
    _assert_equal_states(out[0][1], out[1][1], "after run_epoch with warm-up")


@pytest.mark.gpu
def test_a_batch_of_another_shape_runs_the_eager_step():
    batches = _batches()
    batches[2] = _batches(1, batch_size=1, seed=4)[0]
    assert [b["input"].shape[0] for b in batches] == [2, 2, 1, 2]
    re, se, _ = _run(batches, False)
    rg, sg, step = _run(batches, True)
    assert re == rg and all(r[0] is not None for r in re)
    assert (step.captures, step.eager_fallbacks, step.replays) == (1, 1, 3)
    for i in range(4):
        _assert_equal_states(se[i], sg[i], "after batch %d" % (i + 1))
