"""fd training (row f-5), the part that needs no GPU: the trainable subclass's interface, the third export table against its header,
argument refusals before any launch, the synthetic loader and the trainer's metric arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

import sapcu_amd
import abi_tables
from conftest import FD_KW, golden



def fd_train_header_entry_points():
    """{name: argument list} of include/sapcu_fd_train.h."""
    return abi_tables.header_entry_points("sapcu_fd_train.h")


def test_trainable_subclass_keeps_the_state_dict_layout_of_the_reference():
    g = golden("state_dict_layout.npz")
    model = sapcu_amd.TrainableSNNDistanceEstimation(**FD_KW)
    sd = model.state_dict()
    assert list(sd) == list(g["fd_keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(g["fd_shapes"])
    base = sapcu_amd.EnhancedSNNDistanceEstimation(**FD_KW)
    assert list(base.state_dict()) == list(sd)
    base.load_state_dict(sd, strict=True)                                  # checkpoints move between the two classes


def test_train_mode_works_on_the_subclass_and_still_raises_on_the_base_class():
    model = sapcu_amd.TrainableSNNDistanceEstimation(**FD_KW)
    assert isinstance(model, sapcu_amd.EnhancedSNNDistanceEstimation) and not model.training
    assert model.train() is model and model.training
    assert model.eval() is model and not model.training
    with pytest.raises(NotImplementedError):
        sapcu_amd.EnhancedSNNDistanceEstimation(**FD_KW).train()
    with pytest.raises(NotImplementedError):
        sapcu_amd.TrainableSNNDistanceEstimation(use_snn_decoder=True)


def test_cpu_tensors_raise_runtime_error_in_both_modes():
    model = sapcu_amd.TrainableSNNDistanceEstimation(k=8, emb_dims=64, time_steps_enc=2, num_heads=4, k_scales=[4, 8])
    x = torch.zeros(4, 16, 3)
    for mode in (True, False):
        model.train(mode)
        with pytest.raises(RuntimeError):
            model(x)
    from sapcu_amd import fd_train
    prm = {n: torch.ones(4) for n in ("membrane_decay", "threshold_adapt", "refractory_decay", "threshold_base")}
    with pytest.raises(RuntimeError):
        fd_train.neuron_step_train(torch.zeros(3, 4), prm)
    with pytest.raises(RuntimeError):
        fd_train.edge_feature(torch.zeros(8, 4), torch.zeros(2, 4, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        fd_train.conv_bn_lrelu_max(torch.zeros(8, 32), torch.zeros(32, 32), torch.ones(32), torch.zeros(32))


def test_fd_train_exports_equal_the_header_and_the_other_tables_are_untouched():
    import test_guarded as TG
    from sapcu_amd import _lib
    decl = fd_train_header_entry_points()
    assert set(decl) == set(_lib.FD_TRAIN_EXPORTS) and len(decl) == 9
    assert set(TG.header_entry_points()) == set(_lib.EXPORTS)
    assert not set(_lib.EXPORTS) & set(_lib.FD_TRAIN_EXPORTS) and not set(_lib.SEEDS_EXPORTS) & set(_lib.FD_TRAIN_EXPORTS)
    lib = _lib.load()
    assert lib.sapcu_abi_version() == _lib.ABI_VERSION == 2
    for name in _lib.FD_TRAIN_EXPORTS:
        assert getattr(lib, name).argtypes is not None, name
        nargs = len([a for a in decl[name].split(",") if a.strip()])
        assert len(getattr(lib, name).argtypes) == nargs, (name, nargs)


def test_fd_train_argument_refusals_need_no_gpu():
    """Everything include/sapcu_fd_train.h promises to refuse is refused with SAPCU_ERR_ARG (-1) before any launch — on a machine
    without a GPU, with pointers that are never dereferenced — and the sizers answer -1 for what the calls would refuse."""
    from sapcu_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(4096)                                             # aligned, never touched by a refused call
    nsz, bsz = lib.sapcu_fd_neuron_step_workspace_bytes, lib.sapcu_fd_bn_stats_workspace_bytes
    assert nsz(-1, 4) == -1 and nsz(4, 0) == -1 and bsz(0, 4) == -1 and bsz(4, 0) == -1
    assert 0 < nsz(64, 96) < nsz(65, 96) and nsz(64, 96) < nsz(64, 97) and 0 < bsz(256, 8) < bsz(257, 8)
    n_need, b_need = nsz(64, 96), bsz(64, 96)

    def fwd(x=f, rows=64, ch=96, eif=0, md=f, dT=None, rh=None, state=(None, None, None), sp=f):
        return lib.sapcu_fd_neuron_step_forward(x, rows, ch, eif, md, f, f, f, dT, rh, *state, None, sp, f, f, f, None, None)

    def bwd(x=f, rows=64, ch=96, eif=0, dT=None, rh=None, gdT=None, state=(None, None, None), ws=f, nbytes=n_need):
        return lib.sapcu_fd_neuron_step_backward(x, f, rows, ch, eif, f, f, dT, rh, *state, f, f, f, gdT, None, ws, nbytes, None)

    refused = [fwd(x=None), fwd(md=None), fwd(sp=None), fwd(rows=-1), fwd(ch=0), fwd(eif=1), fwd(eif=1, dT=f), fwd(state=(f, None, None)),
               fwd(state=(f, f, None)), bwd(x=None), bwd(ws=None), bwd(nbytes=n_need - 1), bwd(nbytes=0), bwd(ws=ctypes.c_void_p(4098)),
               bwd(eif=1, dT=f, rh=f), bwd(state=(None, f, f)), bwd(ch=0),
               lib.sapcu_fd_edge_feature_forward(None, 4, f, 2, 4, 2, 4, 8, f, None, None),
               lib.sapcu_fd_edge_feature_forward(f, 3, f, 2, 4, 2, 4, 8, f, None, None),            # ldx < channels
               lib.sapcu_fd_edge_feature_forward(f, 4, f, 2, 4, 2, 4, 7, f, None, None),            # out_channels < 2 channels
               lib.sapcu_fd_edge_feature_forward(f, 4, f, 2, 0, 2, 4, 8, f, None, None),
               lib.sapcu_fd_edge_feature_backward(f, f, 2, 4, 2, 4, 8, f, 4, None, None),           # bad_count is required
               lib.sapcu_fd_edge_feature_backward(f, f, 2, 4, 2, 4, 8, f, 3, f, None),              # ld_grad < channels
               lib.sapcu_fd_edge_feature_backward(f, f, 2, 128, 100, 4, 8, f, 4, f, None),          # inverse table beyond 64 KiB of LDS
               lib.sapcu_fd_bn_stats(f, 64, 96, 1e-5, f, f, f, f, b_need - 1, None),
               lib.sapcu_fd_bn_stats(f, 64, 96, 1e-5, f, f, f, None, b_need, None),
               lib.sapcu_fd_bn_stats(f, 64, 96, 1e-5, f, f, f, ctypes.c_void_p(4100), b_need, None),
               lib.sapcu_fd_bn_stats(f, 0, 96, 1e-5, f, f, f, f, b_need, None),
               lib.sapcu_fd_bn_lrelu_max_forward(f, 4, 0, 8, f, f, f, f, f, f, None),
               lib.sapcu_fd_bn_lrelu_max_forward(f, 4, 2, 8, f, f, f, f, f, None, None),
               lib.sapcu_fd_bn_lrelu_max_backward(f, f, None, 4, 2, 8, f, f, f, f, f, None),
               lib.sapcu_fd_bn_lrelu_max_backward(f, f, f, 4, 2, 0, f, f, f, f, f, None)]
    assert refused == [-1] * len(refused), refused
    assert lib.sapcu_last_error()


def test_synthetic_fd_patches_are_deterministic_and_len_is_the_analytic_distance():
    from sapcu_amd import fd_trainer
    mk = lambda seed: list(fd_trainer.SyntheticFdPatches(batches=3, batch_size=2, patches=8, points=24, seed=seed))
    a, b, c = mk(4), mk(4), mk(5)
    assert len(a) == 3 and len(fd_trainer.SyntheticFdPatches(batches=3)) == 3
    shapes = set()
    for x, y in zip(a, b):
        assert x["input"].shape == (2, 8, 24, 3) and x["input"].dtype == torch.float32
        assert x["len"].shape == (2, 8) and x["len"].dtype == torch.float32
        assert torch.equal(x["input"], y["input"]) and torch.equal(x["len"], y["len"])
        for i in range(2):
            want = fd_trainer.SyntheticFdPatches.surface_distance(x["shape"][i], x["pose"][i].numpy(), x["seed"][i].numpy())
            np.testing.assert_allclose(x["len"][i].numpy(), want, rtol=0, atol=1e-6)
            shapes.add(x["shape"][i])
        assert float(x["len"].min()) >= 0.005 and float(x["len"].max()) <= 0.03
        # rotated normal -> x: the surface lies below the seed along x, at about the seed's distance for the nearest point
        nearest = x["input"].norm(dim=-1).min(dim=-1)[0]
        assert bool((nearest >= x["len"] - 1e-6).all()) and bool((x["input"][..., 0].mean(dim=-1) < 0).all())
    assert not torch.equal(a[0]["input"], c[0]["input"]) and not torch.equal(a[0]["input"], a[1]["input"])
    assert shapes == {"sphere", "torus"}
    n = np.array([0.3, -0.5, 0.8])
    R = fd_trainer.rotation_to_x(n)
    np.testing.assert_allclose(R @ (n / np.linalg.norm(n)), [1, 0, 0], atol=1e-12)
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
    assert np.array_equal(fd_trainer.rotation_to_x([2.0, 0, 0]), np.eye(3))


def test_trainer_metric_arithmetic_and_refused_options():
    from sapcu_amd import fd_trainer
    rng = np.random.default_rng(0)
    pred, gt = torch.from_numpy(rng.uniform(0, 0.05, (4, 16)).astype(np.float32)), torch.from_numpy(rng.uniform(0.005, 0.03, (4, 16)).astype(np.float32))
    m = fd_trainer.Trainer.calculate_metrics(pred, gt, {"total_loss": 1.5})
    assert m["total_loss"] == 1.5
    assert m["mae"] == pytest.approx(float((pred - gt).abs().mean()), rel=1e-6)
    assert m["mse"] == pytest.approx(float(((pred - gt) ** 2).mean()), rel=1e-6)
    assert m["relative_error"] == pytest.approx(float(((pred - gt).abs() / (gt + 1e-8)).mean()), rel=1e-6)
    model = sapcu_amd.TrainableSNNDistanceEstimation(k=8, emb_dims=64, time_steps_enc=2, num_heads=4, k_scales=[4, 8])
    loss, d = model.compute_loss(pred, gt)
    want = torch.nn.functional.smooth_l1_loss(pred, gt, beta=0.1)
    assert torch.equal(loss, want) and d == {"total_loss": want.item(), "distance_loss": want.item()}
    assert model.compute_loss(pred, gt, reduction="none")[0].shape == pred.shape
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    tr = fd_trainer.Trainer(model, opt, grad_clip=0.1)
    assert tr.get_learning_rate() == 1e-3
    tr.set_learning_rate(5e-4)
    assert tr.get_learning_rate() == 5e-4 and tr.reset_model_states() is None
    for kw in (dict(use_amp=True), dict(scaler=object()), dict(gradient_accumulation=2)):
        with pytest.raises(NotImplementedError):
            fd_trainer.Trainer(model, opt, **kw)
    with pytest.raises(NotImplementedError):
        fd_trainer.Trainer(torch.nn.DataParallel(torch.nn.Linear(2, 2)), opt)
    with pytest.raises(ValueError):
        fd_trainer.Trainer(model, opt, grad_clip_type="max")
