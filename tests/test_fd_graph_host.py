"""The graphed training step (rows f-4 and f-5), the part that needs no GPU: the fifth export table against
include/sapcu_train_step.h, sapcu_multi_select's refusals before any launch, what train_step.GraphedTrainStep — one class under the
names fn_trainer.GraphedTrainStep and fd_trainer.GraphedTrainStep — refuses before it captures anything, and that it knows no network."""
import ctypes
import subprocess
import sys

import pytest
import torch

import abi_tables
from conftest import ROOT



def train_step_header_entry_points():
    """{name: argument list} of include/sapcu_train_step.h."""
    return abi_tables.header_entry_points("sapcu_train_step.h")


def test_train_step_exports_equal_the_header_and_the_other_tables_are_untouched():
    import test_guarded as TG
    from sapcu_amd import _lib
    from test_fd_edgeconv_host import fd_edgeconv_header_entry_points
    from test_fd_train_host import fd_train_header_entry_points
    decl = train_step_header_entry_points()
    assert set(decl) == set(_lib.TRAIN_STEP_EXPORTS) == {"sapcu_multi_select"}
    assert set(TG.header_entry_points()) == set(_lib.EXPORTS) and len(_lib.EXPORTS) == 46      # sapcu.h's table is what it was
    assert set(fd_train_header_entry_points()) == set(_lib.FD_TRAIN_EXPORTS) and len(_lib.FD_TRAIN_EXPORTS) == 9
    assert set(fd_edgeconv_header_entry_points()) == set(_lib.FD_EDGECONV_EXPORTS) and len(_lib.FD_EDGECONV_EXPORTS) == 5
    for other in (_lib.EXPORTS, _lib.SEEDS_EXPORTS, _lib.FD_TRAIN_EXPORTS, _lib.FD_EDGECONV_EXPORTS):
        assert not set(other) & set(_lib.TRAIN_STEP_EXPORTS)
    lib = _lib.load()
    assert lib.sapcu_abi_version() == _lib.ABI_VERSION == 2
    for name in _lib.TRAIN_STEP_EXPORTS:
        nargs = len([a for a in decl[name].split(",") if a.strip()])
        assert len(getattr(lib, name).argtypes) == nargs == 7, (name, nargs)


def test_multi_select_argument_refusals_need_no_gpu():
    """What include/sapcu_train_step.h promises to refuse is refused before any HIP call, with pointers never dereferenced."""
    from sapcu_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(4096)

    def call(flag=f, dst=f, src=f, nbytes=f, count=3, blocks=4):
        return lib.sapcu_multi_select(flag, dst, src, nbytes, count, blocks, None)

    refused = [call(flag=None), call(dst=None), call(nbytes=None), call(count=0), call(count=-1), call(count=65536),
               call(blocks=0), call(blocks=-1), call(blocks=65536), call(flag=None, dst=None, src=None, nbytes=None)]
    assert refused == [-1] * len(refused), refused
    assert lib.sapcu_last_error()


class _StubOptimizer:
    def __init__(self, capturable=True):
        self.param_groups = [{"lr": 1e-3, "capturable": capturable, "params": []}]
        self.state = {}


class _StubTrainer:
    """What GraphedTrainStep looks at before it touches a device."""

    def __init__(self, model, scaler=None, gradient_accumulation=1, capturable=True):
        self.model, self.optimizer = model, _StubOptimizer(capturable)
        self.scaler, self.gradient_accumulation = scaler, gradient_accumulation
        self.batched = 0

    def _batch(self, data):
        self.batched += 1
        raise AssertionError("nothing may be staged before the refusals")


def test_graphed_train_step_refuses_before_anything_is_captured():
    from sapcu_amd import fd_trainer
    cpu_model = torch.nn.Linear(3, 1)
    cases = [(dict(scaler=object()), "GradScaler"), (dict(gradient_accumulation=2), "accumulation"), (dict(capturable=False), "capturable"),
             (dict(), "ROCm")]
    for kw, word in cases:
        tr = _StubTrainer(cpu_model, **kw)
        with pytest.raises(ValueError, match=word):
            fd_trainer.GraphedTrainStep(tr, {"input": torch.zeros(1, 2, 4, 3), "len": torch.zeros(1, 2)}, warmup=0)
        assert tr.batched == 0
    # the order: the three checks of the trainer's settings come before the device check, so each is reported on a CPU model
    tr = _StubTrainer(cpu_model, scaler=object(), gradient_accumulation=2, capturable=False)
    with pytest.raises(ValueError, match="GradScaler"):
        fd_trainer.GraphedTrainStep(tr, {}, warmup=0)
    # a real AmpTrainer with accumulation or a scaler, and a real optimiser without capturable=True
    import sapcu_amd
    model = sapcu_amd.TrainableSNNDistanceEstimation(k=8, emb_dims=64, time_steps_enc=2, num_heads=4, k_scales=[4, 8])
    for opt_kw, tr_kw, word in ((dict(capturable=True), dict(gradient_accumulation=2), "accumulation"),
                                (dict(capturable=True), dict(scaler=object()), "GradScaler"), (dict(), dict(), "capturable"),
                                (dict(capturable=True), dict(), "ROCm")):
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, **opt_kw)
        with pytest.raises(ValueError, match=word):
            fd_trainer.GraphedTrainStep(fd_trainer.AmpTrainer(model, opt, **tr_kw), {}, warmup=0)


def test_the_graphed_step_is_one_method_under_two_names_and_no_counter_exists_before_a_device_is_used():
    from sapcu_amd import fd_train, fd_trainer
    assert fd_trainer.GraphedTrainStep.__call__ is fd_trainer.GraphedTrainStep.train_step
    if not torch.cuda.is_available():
        assert fd_train._BAD == {} and fd_train.take_bad_index_count() == 0
        with pytest.raises((RuntimeError, AssertionError)):                       # the counter is a device tensor: no device, no counter
            fd_train.bad_index_counter("cuda:0")
        assert fd_train._BAD == {}


def test_the_two_public_names_are_one_class_and_it_refuses_for_an_fn_trainer_too():
    from sapcu_amd import fd_trainer, fn_trainer, train_step
    assert fn_trainer.GraphedTrainStep is fd_trainer.GraphedTrainStep is train_step.GraphedTrainStep
    assert fn_trainer.run_epoch is train_step.run_epoch and fn_trainer.clamp_neuron_parameters is train_step.clamp_neuron_parameters
    cpu_model = torch.nn.Linear(3, 1)
    batch = {"input": torch.zeros(1, 2, 4, 3), "normal": torch.zeros(1, 2, 3)}
    for opt_kw, tr_kw, word in ((dict(capturable=True), dict(use_amp=True, scaler=object()), "GradScaler"),
                                (dict(capturable=True), dict(gradient_accumulation=2), "accumulation"), (dict(), dict(), "capturable"),
                                (dict(capturable=True), dict(), "ROCm")):
        opt = torch.optim.AdamW(cpu_model.parameters(), lr=1e-3, **opt_kw)
        with pytest.raises(ValueError, match=word):
            fn_trainer.GraphedTrainStep(fn_trainer.Trainer(cpu_model, opt, **tr_kw), batch, warmup=0)
    # the order, on a stub that has fn's attributes and would fail at the first use of a hook
    tr = _StubTrainer(cpu_model, scaler=object(), gradient_accumulation=2, capturable=False)
    tr.use_amp = True
    with pytest.raises(ValueError, match="GradScaler"):
        fn_trainer.GraphedTrainStep(tr, batch, warmup=0)
    assert tr.batched == 0


def test_train_step_does_not_import_fd_train():
    """The shared module knows no network: importing it in a fresh interpreter loads neither fd_train nor a trainer."""
    code = ("import sys, sapcu_amd.train_step\n"
            "print(sorted(m for m in ('sapcu_amd.fd_train', 'sapcu_amd.fd_trainer', 'sapcu_amd.fn_trainer') if m in sys.modules))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "[]", (r.stdout, r.stderr[-2000:])
