"""fd's training step replayed as one HIP graph (fd_trainer.GraphedTrainStep, -m gpu) and the kernel that makes its skip decision
on the device (sapcu_multi_select, include/sapcu_train_step.h).

The contract is exactness: a replay leaves parameters, buffers and the optimiser's state bit for bit as the eager step on the same
batch leaves them — step applied, batch skipped, bad index raised.  fd's step has no atomics and is reproducible bit for bit
(DESIGN 4.5), so every comparison here is torch.equal or ==; there is no tolerance.  Shapes are the smallest the fd trainer tests
use (2 clouds x 8 patches x 24 points, T = 3)."""
import math

import numpy as np
import pytest
import torch

import gpu_utils as U

KW = dict(k=8, emb_dims=64, time_steps_enc=3, num_heads=4, k_scales=[4, 8, 16])
MODES = [("f32", "feature"), ("bf16", "factored")]
F32, I32, I64 = torch.float32, torch.int32, torch.int64


def _fresh(dropout=0.0, lr=3e-3, generator=True, **opt_kw):
    import sapcu_amd
    torch.manual_seed(0)
    model = sapcu_amd.TrainableSNNDistanceEstimation(dropout=dropout, **KW).to(U.dev())
    model.dropout_generator = torch.Generator(device=U.dev()).manual_seed(7) if generator else None
    return model, torch.optim.AdamW(model.parameters(), lr=lr, capturable=True, **opt_kw)


def _trainer(model, opt, mode="bf16", form="factored"):
    from sapcu_amd import fd_trainer
    return fd_trainer.AmpTrainer(model, opt, device=U.dev(), grad_clip=0.1, use_amp=(mode == "bf16"), edgeconv=form)


_BATCHES = {}


def _batches(n=4, batch_size=2, seed=3):
    from sapcu_amd import fd_trainer
    key = (n, batch_size, seed)
    if key not in _BATCHES:
        _BATCHES[key] = list(fd_trainer.SyntheticFdPatches(batches=n, batch_size=batch_size, patches=8, points=24, seed=seed))
    return [dict(b) for b in _BATCHES[key]]


def _state(model, opt):
    """Clones of everything the contract covers: parameters, buffers, optimiser state keyed by the parameter's name."""
    names = {q: n for n, q in model.named_parameters()}
    out = {"param/" + n: q.detach().clone() for n, q in model.named_parameters()}
    out.update({"buffer/" + n: b.detach().clone() for n, b in model.named_buffers()})
    for q, st in opt.state.items():
        for key, v in st.items():
            if torch.is_tensor(v):
                out["opt/%s/%s" % (names[q], key)] = v.detach().clone()
    return out


def _assert_equal_states(a, b, what, skip_prefix=()):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    for n in a:
        if not n.startswith(tuple(skip_prefix)):
            assert a[n].dtype == b[n].dtype and torch.equal(a[n], b[n]), "%s: %s differs" % (what, n)


def _grads_are_zero(model):
    return all(q.grad is None or not bool(q.grad.any()) for q in model.parameters())


def _run(mode, form, batches, graphed, after=None, **fresh_kw):
    """-> (losses, [state after every batch], model, opt, step): the eager AmpTrainer or the graphed step (warmup=0) from the same start."""
    from sapcu_amd import fd_trainer
    model, opt = _fresh(**fresh_kw)
    tr = _trainer(model, opt, mode, form)
    step = fd_trainer.GraphedTrainStep(tr, batches[0], warmup=0) if graphed else tr
    losses, states = [], []
    for i, b in enumerate(batches):
        losses.append(step.train_step(b)[0])
        states.append(_state(model, opt))
        if after is not None:
            after(i, model, opt)
    return losses, states, model, opt, step


# ================================================================================================ the contract
@pytest.mark.gpu
@pytest.mark.parametrize("mode,form", MODES)
def test_graphed_step_equals_the_eager_step_bit_for_bit(mode, form):
    import sapcu_amd
    from sapcu_amd import fd_trainer
    batches = _batches()
    le, se, _, opt_e, _ = _run(mode, form, batches, False)
    lg, sg, model, opt_g, _ = _run(mode, form, batches, True)
    print("eager  ", le, "\ngraphed", lg)
    assert le == lg and all(v is not None and math.isfinite(v) for v in le)
    for i in range(len(batches)):
        _assert_equal_states(se[i], sg[i], "after batch %d" % (i + 1))
    assert any(n.endswith("num_batches_tracked") for n in se[-1]) and any(n.endswith("/step") for n in se[-1])
    assert any(n.endswith("/exp_avg") for n in se[-1]) and any(n.endswith("/exp_avg_sq") for n in se[-1])
    assert float(sg[-1]["opt/distance_decoder.fc_distance.weight/step"]) == len(batches)
    assert isinstance(opt_g.param_groups[0]["lr"], float) and opt_g.param_groups[0]["lr"] == opt_e.param_groups[0]["lr"]
    # the packed inference blob was dropped by the replays: eval() sees the trained parameters and buffers
    assert model._packed_key is None
    model.eval()
    base = sapcu_amd.EnhancedSNNDistanceEstimation(**KW)
    base.load_state_dict(model.state_dict(), strict=True)
    base = base.to(U.dev())
    x = next(iter(fd_trainer.SyntheticFdPatches(batches=1, batch_size=2, patches=8, points=24, seed=9)))["input"].to(U.dev())
    with torch.no_grad():
        a, b = model(x), base(x)
    assert a.shape == (2, 8) and torch.equal(a, b)


@pytest.mark.gpu
def test_a_skipped_batch_is_skipped_exactly(capsys):
    """One entry of batch 2's `len` is NaN (the input stays finite): the loss is NaN, both steps return (None, None) and print the
    eager warning; the graph has run its backward and optimizer.step() on NaNs and put everything back."""
    batches = _batches()
    batches[1]["len"] = batches[1]["len"].clone()
    batches[1]["len"][0, 3] = float("nan")
    seen = {}

    def after(i, model, opt):
        if i == 1:
            seen["zero"] = _grads_are_zero(model)
    le, se, _, _, _ = _run("bf16", "factored", batches, False)
    assert capsys.readouterr().out.count("WARNING: NaN/Inf in loss value") == 1
    lg, sg, _, _, step = _run("bf16", "factored", batches, True, after=after)
    assert capsys.readouterr().out.count("WARNING: NaN/Inf in loss value") == 1
    assert le == lg and le[1] is None and all(v is not None for v in (le[0], le[2], le[3]))
    for i in (1, 2, 3):
        _assert_equal_states(se[i], sg[i], "after batch %d" % (i + 1))
    # skipped: parameters and optimiser state are those after batch 1, the BatchNorm buffers have moved
    _assert_equal_states(sg[0], sg[1], "across the skipped batch", skip_prefix=("buffer/",))
    assert any(not torch.equal(sg[0][n], sg[1][n]) for n in sg[0] if n.startswith("buffer/"))
    assert seen["zero"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["feature", "factored"])
def test_a_bad_index_raises_from_the_replay_and_changes_nothing(form, monkeypatch):
    """The index is planted where no check stands, in the table the free-running feature kNN hands to blocks 1-3 (the method of
    test_an_index_outside_its_patch_fails_the_amp_step...), before the capture: the library counts it and gives it no gradient."""
    from sapcu_amd import fd_train, fd_trainer
    real = fd_train.feature_knn

    def planted(x, P, M, k):
        idx = real(x, P, M, k)
        idx[0, 0, :1].fill_(M)                                                   # a fill kernel: `idx[0, 0, 0] = M` copies from the host
        return idx
    monkeypatch.setattr(fd_train, "feature_knn", planted)
    batch = _batches()[0]
    model, opt = _fresh()
    tr = _trainer(model, opt, "bf16", form)
    step = fd_trainer.GraphedTrainStep(tr, batch, warmup=0)
    before = _state(model, opt)
    with pytest.raises(RuntimeError, match="neighbour indices outside their patch reached the EdgeConv backward"):
        step(batch)
    _assert_equal_states(before, _state(model, opt), "after the refused replay", skip_prefix=("buffer/",))
    assert fd_train.take_bad_index_count() == 0 and _grads_are_zero(model)
    assert all(float(v) == 0 for n, v in before.items() if n.endswith("/step"))
    # and the eager step on the same model says the same
    with pytest.raises(RuntimeError, match="neighbour indices outside their patch"):
        tr.train_step(batch)
    assert fd_train.take_bad_index_count() == 0


@pytest.mark.gpu
def test_the_learning_rate_follows_the_groups():
    from sapcu_amd import fd_trainer, fn_trainer
    batches = _batches(6)
    rate = {}

    def after(i, model, opt):
        if i == 0:
            opt.param_groups[0]["lr"] = 1e-3                                    # batch 2 runs eager, batch 3 is captured anew
        if i == 2:
            rate["t"] = opt.param_groups[0]["lr"] = torch.tensor(2e-3, device=U.dev())      # batch 4 eager, batch 5 captured anew
        if i == 4:
            rate["t"].fill_(5e-4)                                               # in place: batch 6 is a replay of the same graph
    le, se, _, _, _ = _run("bf16", "factored", batches, False, after=after)
    lg, sg, _, _, step = _run("bf16", "factored", batches, True, after=after)
    assert le == lg and step.captures == 3 and step.eager_fallbacks == 2
    for i in range(6):
        _assert_equal_states(se[i], sg[i], "after batch %d" % (i + 1))
    l3, s3, _, _, _ = _run("bf16", "factored", batches, True)                   # the schedule matters: a constant rate ends elsewhere
    assert l3[:2] == lg[:2] and not torch.equal(s3[5]["param/distance_decoder.fc_distance.weight"], sg[5]["param/distance_decoder.fc_distance.weight"])
    # run_epoch's warm-up writes floats into the groups
    out = []
    for graphed in (False, True):
        model, opt = _fresh()
        tr = _trainer(model, opt)
        step = fd_trainer.GraphedTrainStep(tr, batches[0], warmup=0) if graphed else tr
        it, losses, st = fn_trainer.run_epoch(step, _batches(), warmup_steps=3)
        assert it == 4 and st["skipped"] == 0 and (not graphed or (step.captures, step.eager_fallbacks) == (2, 2))
        out.append((losses, _state(model, opt), opt.param_groups[0]["lr"]))
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2] and out[0][2] != 3e-3
    _assert_equal_states(out[0][1], out[1][1], "after run_epoch with warm-up")


@pytest.mark.gpu
def test_a_float_rate_and_a_tensor_rate_do_not_give_the_same_bits_in_eager_adamw():
    """Why a float learning rate is captured as a float and not turned into a device tensor (fd_trainer.GraphedTrainStep): ONE eager
    AdamW(capturable=True) step from the same start with lr = 3e-3 and with lr = tensor(3e-3) leaves different parameters (moments and
    step counts equal; some parameters one ulp apart).  A graph that read the rate from a tensor would equal the second and could not
    equal the first.  Should a later torch make the two equal, this test fails and the rate can become a tensor as first planned.
    The graphed step over a tensor rate equals the eager step over the same tensor."""
    from sapcu_amd import fd_trainer
    batch = _batches()[0]
    states = []
    for rate, graphed in (("float", False), ("tensor", False), ("tensor", True)):
        model, opt = _fresh()
        if rate == "tensor":
            opt.param_groups[0]["lr"] = torch.tensor(3e-3, device=U.dev())
        tr = _trainer(model, opt, "f32", "feature")
        step = fd_trainer.GraphedTrainStep(tr, batch, warmup=0) if graphed else tr
        assert step.train_step(batch)[0] is not None
        states.append(_state(model, opt))
    differing = [n for n in states[0] if not torch.equal(states[0][n], states[1][n])]
    worst = max(float((states[0][n].double() - states[1][n].double()).abs().max() / states[0][n].double().abs().max()) for n in differing) if differing else 0.0
    print("tensors that differ between a float and a tensor rate: %d of %d, worst relative difference %.3g" % (len(differing), len(states[0]), worst))
    assert differing and all(n.startswith("param/") for n in differing) and worst < 1e-6
    _assert_equal_states(states[1], states[2], "graphed against eager, both over the same rate tensor")


@pytest.mark.gpu
def test_a_batch_of_another_shape_runs_the_eager_step():
    batches = _batches()
    batches[2] = _batches(1, batch_size=1, seed=4)[0]
    assert [b["input"].shape[0] for b in batches] == [2, 2, 1, 2]
    le, se, _, _, _ = _run("bf16", "factored", batches, False)
    lg, sg, _, _, step = _run("bf16", "factored", batches, True)
    assert le == lg and all(v is not None for v in le) and (step.captures, step.eager_fallbacks) == (1, 1)
    for i in range(4):
        _assert_equal_states(se[i], sg[i], "after batch %d" % (i + 1))


@pytest.mark.gpu
def test_dropout_masks_move_from_replay_to_replay():
    """dropout = 0.1 with a seeded generator: two graphed runs are bit-identical; with a zero rate the same batch replayed twice
    gives two different losses (the masks moved), with dropout = 0.0 the same loss.

    This is also the test that needs the library's capture-aware zeroing of the bad_count slots (zero_count, csrc/common.h): with
    hipMemsetAsync captured as a memset node, the first graphed run here raised "16843009 neighbour indices outside their patch"
    (0x01010101 in one EdgeConv backward's slot, in the feature and the factored form alike; the eager step counts 0)."""
    from sapcu_amd import fd_trainer
    batches = _batches()
    runs = [_run("bf16", "factored", batches, True, dropout=0.1) for _ in range(2)]
    assert runs[0][0] == runs[1][0] and all(v is not None for v in runs[0][0])
    _assert_equal_states(runs[0][1][3], runs[1][1][3], "two graphed runs with a seeded generator")
    eager = _run("bf16", "factored", batches, False, dropout=0.1)
    print("graphed masks equal the eager ones (a property of torch's generator, not asserted):", eager[0] == runs[0][0])
    for dropout, generator in ((0.1, True), (0.1, False), (0.0, True)):
        model, opt = _fresh(dropout=dropout, lr=0.0, generator=generator, weight_decay=0.0)
        step = fd_trainer.GraphedTrainStep(_trainer(model, opt), batches[0], warmup=0)
        a, b = step(batches[0])[0], step(batches[0])[0]
        print("dropout %.1f, %s generator: %.9g %.9g" % (dropout, "the model's" if generator else "the default", a, b))
        assert (a != b) if dropout > 0 else (a == b)


@pytest.mark.gpu
def test_clamp_parameters_runs_inside_the_graph_after_the_step():
    from sapcu_amd import fd_trainer, fn_trainer
    batch = _batches()[0]
    out = []
    for graphed in (False, True):
        model, opt = _fresh()
        with torch.no_grad():
            for n, q in model.named_parameters():
                if "membrane_decay" in n:
                    q.fill_(1.5)
        tr = _trainer(model, opt)
        if graphed:
            step = fd_trainer.GraphedTrainStep(tr, batch, warmup=0, clamp_parameters=True)
            it, losses, _ = fn_trainer.run_epoch(step, [batch], clamp_parameters=False)
        else:
            it, losses, _ = fn_trainer.run_epoch(tr, [batch], clamp_parameters=True)
        assert it == 1 and len(losses) == 1
        out.append((losses, _state(model, opt)))
    assert out[0][0] == out[1][0]
    _assert_equal_states(out[0][1], out[1][1], "after one clamped step")
    decays = [v for n, v in out[1][1].items() if n.startswith("param/") and "membrane_decay" in n]
    assert decays and all(bool((v <= 0.99).all()) for v in decays)                # (in f32, as the clamp compares)


# ================================================================================================ sapcu_multi_select: the memory contract
SIZES = (4, 12, 20, 4096 + 4, 1 << 20)
OFFSETS = (4, 8, 16)
MS_CASES = [(1, 1, 0), (1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 1, 4), (1, 8, 4), (1, 8, 2), (37, 1, 0), (37, 8, 0)]
MS_ENTRY_POINTS = ("sapcu_multi_select",)
DIRTY = 0xAB


def _select_tables(count, first_size, band_fill):
    """count guarded (dst, src) pairs: sizes walk SIZES from `first_size`, dst bases sit at offsets 4, 8, 16 (mod 512), src bases
    at another walk of the same offsets, so a pair is aligned alike or not; with count > 1 entry 3 (and every 5th after) has a NULL
    source and entry 5 is zero bytes long (its 16-byte buffers stay as they are)."""
    from guarded import guarded
    rng = np.random.default_rng(count + first_size)
    entries = []
    for i in range(count):
        n = SIZES[(first_size + i) % len(SIZES)]
        zero_len = count > 1 and i == 5
        null_src = count > 1 and i % 5 == 3
        alloc = 16 if zero_len else n
        d = guarded((alloc // 4,), I32, offset=OFFSETS[i % 3], band_fill=band_fill, device=U.dev(), name="dst %d" % i)
        s = guarded((alloc // 4,), I32, offset=OFFSETS[(i // 3 + i) % 3], band_fill=band_fill, device=U.dev(), name="src %d" % i)
        s.set(torch.from_numpy(rng.integers(1, 1 << 30, alloc // 4).astype(np.int32)).to(U.dev()))
        d.fill_payload_bytes(DIRTY)
        entries.append((d, s, 0 if zero_len else n, null_src))
    dev = U.dev()
    dst = torch.tensor([d.t.data_ptr() for d, _, _, _ in entries], dtype=I64, device=dev)
    src = torch.tensor([0 if null else s.t.data_ptr() for _, s, _, null in entries], dtype=I64, device=dev)
    nbytes = torch.tensor([n for _, _, n, _ in entries], dtype=I64, device=dev)
    return entries, dst, src, nbytes


def _select(flag, dst, src, nbytes, count, blocks):
    from sapcu_amd import _lib
    lib = _lib.load()
    fl = torch.tensor([flag], dtype=I32, device=U.dev())
    rc = lib.sapcu_multi_select(_lib.ptr(fl), _lib.ptr(dst), _lib.ptr(src), _lib.ptr(nbytes), count, blocks, _lib.current_stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("count,blocks,first_size", MS_CASES, ids=["n%d-b%d-s%d" % c for c in MS_CASES])
def test_multi_select_bounds(count, blocks, first_size):
    """Twice, with 0xFF and with 0x00 bands.  Flag 0: every dst and every band is what it was.  Flag 1: every dst equals its source,
    or zero for a NULL source, a zero-length entry is untouched, sources and bands intact."""
    for band_fill in (0xFF, 0x00):
        entries, dst, src, nbytes = _select_tables(count, first_size, band_fill)
        sources = [s.payload_bits() for _, s, _, _ in entries]
        assert _select(0, dst, src, nbytes, count, blocks) == 0
        for d, s, n, null in entries:
            d.check()
            s.check()
            assert bool((d.payload_bits() == DIRTY).all()), "%s was written with the flag clear" % d.name
        assert _select(1, dst, src, nbytes, count, blocks) == 0
        for (d, s, n, null), was in zip(entries, sources):
            d.check()
            s.check()
            assert torch.equal(s.payload_bits(), was), "%s was written" % s.name
            got = d.payload_bits()
            if n == 0:
                assert bool((got == DIRTY).all()), "%s: a zero-length entry was written" % d.name
            elif null:
                assert not bool(got.any()), "%s: not zero-filled" % d.name
            else:
                assert torch.equal(got, was), "%s differs from its source" % d.name
    if count > 1:
        assert any(null for _, _, _, null in entries) and any(n == 0 for _, _, n, _ in entries)
        assert {n for _, _, n, _ in entries} >= set(SIZES)


MS_REFUSALS = [("count-0", dict(count=0)), ("count-negative", dict(count=-3)), ("blocks-0", dict(blocks=0)), ("blocks-65536", dict(blocks=65536)),
               ("null-flag", dict(null="flag")), ("null-dst", dict(null="dst")), ("null-nbytes", dict(null="nbytes"))]


@pytest.mark.gpu
@pytest.mark.parametrize("r", MS_REFUSALS, ids=[r[0] for r in MS_REFUSALS])
def test_multi_select_refusal_launches_nothing(r):
    from sapcu_amd import _lib
    lib = _lib.load()
    kw = dict(count=3, blocks=4, null=None)
    kw.update(r[1])
    entries, dst, src, nbytes = _select_tables(3, 1, 0xFF)
    fl = torch.ones((1,), dtype=I32, device=U.dev())                            # set: a launch would show
    p = {"flag": _lib.ptr(fl), "dst": _lib.ptr(dst), "src": _lib.ptr(src), "nbytes": _lib.ptr(nbytes)}
    if kw["null"]:
        p[kw["null"]] = None
    rc = lib.sapcu_multi_select(p["flag"], p["dst"], p["src"], p["nbytes"], kw["count"], kw["blocks"], _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == -1, "%s returned %d" % (r[0], rc)
    for d, s, _, _ in entries:
        d.check()
        assert bool((d.payload_bits() == DIRTY).all()), "%s: %s was written by a refused call" % (r[0], d.name)


def test_every_entry_point_of_the_train_step_header_has_a_bounds_case():
    """The gate of test_every_entry_point_of_the_fd_edgeconv_header_has_a_bounds_case over include/sapcu_train_step.h; sapcu.h's own
    table (the gate of tests/test_guarded.py) is what it was."""
    import test_guarded as TG
    from sapcu_amd import _lib
    from test_fd_graph_host import train_step_header_entry_points
    decl = train_step_header_entry_points()
    assert set(decl) == set(_lib.TRAIN_STEP_EXPORTS)
    assert sorted(n for n, args in decl.items() if "*" in args and n not in MS_ENTRY_POINTS) == []
    assert sorted(n for n, args in decl.items() if "*" in args) == ["sapcu_multi_select"]      # the gate itself: it sees the entry point
    for other in (_lib.EXPORTS, _lib.SEEDS_EXPORTS, _lib.FD_TRAIN_EXPORTS, _lib.FD_EDGECONV_EXPORTS):
        assert not set(other) & set(_lib.TRAIN_STEP_EXPORTS)
    assert set(TG.header_entry_points()) == set(_lib.EXPORTS) and len(_lib.EXPORTS) == 46
    assert {c[0] for c in MS_CASES} == {1, 37} and {c[1] for c in MS_CASES} == {1, 8}
    assert {r[0] for r in MS_REFUSALS} >= {"count-0", "blocks-0", "blocks-65536", "null-flag", "null-dst", "null-nbytes"}
