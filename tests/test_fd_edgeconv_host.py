"""The factored EdgeConv training op and the AMP trainer of fd (row f-5), the part that needs no GPU: the fourth export table
against include/sapcu_fd_edgeconv.h, argument refusals before any launch, the sizers, the form context and AmpTrainer's options."""
import ctypes

import pytest
import torch

import sapcu_amd
import abi_tables


def fd_edgeconv_header_entry_points():
    """{name: argument list} of include/sapcu_fd_edgeconv.h."""
    return abi_tables.header_entry_points("sapcu_fd_edgeconv.h")


def test_fd_edgeconv_exports_equal_the_header_and_the_other_tables_are_untouched():
    import test_guarded as TG
    from sapcu_amd import _lib
    from test_fd_train_host import fd_train_header_entry_points
    decl = fd_edgeconv_header_entry_points()
    assert set(decl) == set(_lib.FD_EDGECONV_EXPORTS) and len(decl) == 5
    assert set(TG.header_entry_points()) == set(_lib.EXPORTS)
    assert set(fd_train_header_entry_points()) == set(_lib.FD_TRAIN_EXPORTS) and len(_lib.FD_TRAIN_EXPORTS) == 9
    for other in (_lib.EXPORTS, _lib.SEEDS_EXPORTS, _lib.FD_TRAIN_EXPORTS):
        assert not set(other) & set(_lib.FD_EDGECONV_EXPORTS)
    lib = _lib.load()
    assert lib.sapcu_abi_version() == _lib.ABI_VERSION == 2
    for name in _lib.FD_EDGECONV_EXPORTS:
        nargs = len([a for a in decl[name].split(",") if a.strip()])
        assert len(getattr(lib, name).argtypes) == nargs, (name, nargs)


def test_fd_edgeconv_argument_refusals_need_no_gpu():
    """Everything include/sapcu_fd_edgeconv.h promises to refuse with SAPCU_ERR_ARG (-1) is refused before any launch, with pointers
    that are never dereferenced; a workspace one byte short is SAPCU_ERR_WORKSPACE (-2); the sizers answer -1 for the shapes the
    calls refuse and grow with rows and channels."""
    from sapcu_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(4096)
    ssz, bsz = lib.sapcu_fd_edgeconv_stats_workspace_bytes, lib.sapcu_fd_edgeconv_backward_workspace_bytes
    for sz in (ssz, bsz):
        assert sz(0, 7, 5, 64) == -1 and sz(-1, 7, 5, 64) == -1 and sz(2, 0, 5, 64) == -1 and sz(2, 7, 0, 64) == -1 and sz(2, 7, 5, 0) == -1
        assert sz(2, 128, 64, 64) == -1                                     # the inverse table passes 64 KiB of LDS
        assert 0 < sz(2, 100, 32, 64) < sz(3, 100, 32, 64) and sz(2, 100, 32, 64) < sz(2, 100, 32, 65) and sz(2, 99, 32, 64) <= sz(2, 100, 32, 64)
    s_need, b_need = ssz(2, 7, 5, 64), bsz(2, 7, 5, 64)

    def stats(ab=f, idx=f, P=2, m=7, kk=5, ch=64, mean=f, ws=f, nbytes=s_need):
        return lib.sapcu_fd_edgeconv_stats(ab, idx, P, m, kk, ch, 1e-5, mean, f, f, None, ws, nbytes, None)

    def fmax(ab=f, P=2, m=7, kk=5, ch=64, out=f, arg=f):
        return lib.sapcu_fd_edgeconv_max_forward(ab, f, P, m, kk, ch, f, f, f, f, out, arg, None)

    def bwd(ab=f, arg=f, P=2, m=7, kk=5, ch=64, gab=f, bad=f, ws=f, nbytes=b_need):
        return lib.sapcu_fd_edgeconv_backward(ab, f, f, arg, P, m, kk, ch, f, f, f, f, gab, f, f, bad, ws, nbytes, None)

    refused = [stats(ab=None), stats(idx=None), stats(mean=None), stats(ws=None), stats(P=0), stats(m=0), stats(kk=0), stats(ch=0),
               stats(m=128, kk=64), stats(ws=ctypes.c_void_p(4100)),
               fmax(ab=None), fmax(out=None), fmax(arg=None), fmax(P=-1), fmax(kk=0), fmax(ch=0), fmax(m=128, kk=64),
               bwd(ab=None), bwd(arg=None), bwd(gab=None), bwd(bad=None), bwd(ws=None), bwd(P=0), bwd(m=0), bwd(kk=0), bwd(ch=0),
               bwd(m=128, kk=64), bwd(ws=ctypes.c_void_p(4100))]
    assert refused == [-1] * len(refused), refused
    assert lib.sapcu_last_error()
    short = [stats(nbytes=s_need - 1), stats(nbytes=0), bwd(nbytes=b_need - 1), bwd(nbytes=0)]
    assert short == [-2] * len(short), short


def test_edgeconv_form_context_and_cpu_tensors():
    from sapcu_amd import fd_train
    assert fd_train._EDGECONV_FORM[0] == "feature"
    with pytest.raises(ValueError):
        fd_train.edgeconv_form("x")
    with fd_train.edgeconv_form("factored"):
        assert fd_train._EDGECONV_FORM[0] == "factored"
        with fd_train.edgeconv_form("feature"):
            assert fd_train._EDGECONV_FORM[0] == "feature"
        assert fd_train._EDGECONV_FORM[0] == "factored"
    assert fd_train._EDGECONV_FORM[0] == "feature"
    with pytest.raises(KeyError):
        with fd_train.edgeconv_form("factored"):
            raise KeyError("left by an exception")
    assert fd_train._EDGECONV_FORM[0] == "feature"
    with pytest.raises(RuntimeError):
        fd_train.edgeconv_factored(torch.zeros(8, 32), torch.zeros(32, 64), torch.ones(32), torch.zeros(32), torch.zeros(2, 4, 2, dtype=torch.int32))


def test_amp_trainer_options_and_the_f32_trainer_still_refuses_them():
    from sapcu_amd import fd_trainer
    model = sapcu_amd.TrainableSNNDistanceEstimation(k=8, emb_dims=64, time_steps_enc=2, num_heads=4, k_scales=[4, 8])
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    tr = fd_trainer.AmpTrainer(model, opt, use_amp=True, scaler=None, gradient_accumulation=2, edgeconv="factored", grad_clip=0.1)
    assert isinstance(tr, fd_trainer.Trainer) and tr.use_amp and tr.gradient_accumulation == 2 and tr.edgeconv == "factored"
    assert tr.accumulation_step == 0 and tr.get_learning_rate() == 1e-3
    scaler = object()
    assert fd_trainer.AmpTrainer(model, opt, use_amp=False, scaler=scaler, edgeconv="feature").scaler is scaler
    assert fd_trainer.AmpTrainer(model, opt).edgeconv in ("feature", "factored")
    with pytest.raises(ValueError):
        fd_trainer.AmpTrainer(model, opt, edgeconv="x")
    with pytest.raises(ValueError):
        fd_trainer.AmpTrainer(model, opt, grad_clip_type="max")
    with pytest.raises(ValueError):
        fd_trainer.AmpTrainer(model, opt, gradient_accumulation=0)
    with pytest.raises(NotImplementedError):
        fd_trainer.AmpTrainer(torch.nn.DataParallel(torch.nn.Linear(2, 2)), opt)
    for kw in (dict(use_amp=True), dict(scaler=object()), dict(gradient_accumulation=2)):
        with pytest.raises(NotImplementedError):
            fd_trainer.Trainer(model, opt, **kw)
