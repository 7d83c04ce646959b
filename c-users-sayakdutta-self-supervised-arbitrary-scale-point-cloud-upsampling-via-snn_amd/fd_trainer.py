"""Training driver for fd — the reference's ``fd/trainer.py`` ``Trainer`` (methods and return values) over
``TrainableSNNDistanceEstimation`` (sapcu_amd/fd_train.py).  With the optional ``grad_clip`` / ``grad_clip_type``, applied between
backward and step, ``fn_trainer.run_epoch(trainer, loader, clamp_parameters=True)`` is the batch loop of the reference's
trainfd.py:264-313 in f32.  ``SyntheticFdPatches`` stands in for the reference's h5 distance-field data, absent here.

``Trainer`` is the f32 step and refuses ``use_amp`` / ``scaler`` / ``gradient_accumulation``; ``AmpTrainer`` is the reference's
default configuration (config/fd.yaml ``use_amp: true``, trainfd.py:194-291): bf16 GEMMs, an optional GradScaler, gradient
accumulation, and the EdgeConv form of blocks 1-3.

``GraphedTrainStep`` replays one whole step of either trainer as a HIP graph and leaves exactly the state the eager step leaves.

Not built, and the constructors say so: DataParallel (``model.module``), ``use_snn_decoder=True`` (refused by the model)."""
import contextlib
import math

import numpy as np
import torch


class Trainer:
    def __init__(self, model, optimizer, device=None, input_type='pointcloud', vis_dir=None, threshold=0.5, eval_sample=False,
                 grad_clip=None, grad_clip_type='norm', use_amp=False, scaler=None, gradient_accumulation=1):
        if use_amp or scaler is not None:
            raise NotImplementedError("fd_trainer.Trainer runs in f32: bf16 / GradScaler are AmpTrainer's")
        if gradient_accumulation != 1:
            raise NotImplementedError("fd_trainer.Trainer: gradient accumulation is AmpTrainer's")
        if hasattr(model, 'module'):
            raise NotImplementedError("fd training: DataParallel is not built (one process per GPU)")
        if grad_clip_type not in ('norm', 'value'):
            raise ValueError("grad_clip_type must be 'norm' or 'value'")
        self.model, self.optimizer, self.device = model, optimizer, device
        self.input_type, self.vis_dir, self.threshold, self.eval_sample = input_type, vis_dir, threshold, eval_sample
        self.grad_clip, self.grad_clip_type = grad_clip, grad_clip_type
        if device is not None:
            self.model.to(device)

    def _batch(self, data):
        x = data.get('input').to(self.device).float()
        gt = data.get('len').to(self.device).float()
        if gt.dim() in (2, 3) and gt.shape[-1] == 1 and gt.dim() == x.dim() - 1:        # [B, 1] / [B, N, 1] (fd/trainer.py:75-78)
            gt = gt.squeeze(-1)
        return x, gt

    def train_step(self, data):
        """fd/trainer.py:24-36 (+ the clipping of trainfd.py:301-302): -> (loss value, loss dict), or (None, None) when the loss or
        a gradient is not finite (the batch is skipped, as trainfd.py's except branch does)."""
        from . import fd_train
        self.model.train()
        self.optimizer.zero_grad()
        self.reset_model_states()
        fd_train.take_bad_index_count()
        loss, loss_dict = self.compute_loss_with_dict(data)
        if not bool(torch.isfinite(loss)):
            print("WARNING: NaN/Inf in loss value")
            return None, None
        loss.backward()
        bad = fd_train.take_bad_index_count()
        if bad:
            self.optimizer.zero_grad()
            raise RuntimeError("fd training step: %d neighbour indices outside their patch reached the EdgeConv backward" % bad)
        if self.grad_clip is not None and self.grad_clip > 0:
            if self.grad_clip_type == 'norm':
                total = torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.grad_clip)
            else:
                torch.nn.utils.clip_grad_value_(self.model.parameters(), self.grad_clip)
                total = None
        else:
            total = None
        if total is None:
            grads = [prm.grad for prm in self.model.parameters() if prm.grad is not None]
            total = torch.stack(torch._foreach_norm(grads)).sum()
        if not bool(torch.isfinite(total)):
            print("WARNING: NaN/Inf in gradients")
            self.optimizer.zero_grad()
            return None, None
        self.optimizer.step()
        return loss.item(), loss_dict

    def evaluate(self, val_loader, return_metrics=False):
        """Mean loss over the loader's batches (0.0 for an empty loader); with return_metrics also the per-key batch means of
        ``calculate_metrics``."""
        self.model.eval()
        self.reset_model_states()
        per_batch = [self.eval_step_with_metrics(batch) for batch in val_loader]
        n = len(per_batch)
        mean_loss = sum(float(loss) for loss, _ in per_batch) / n if n else 0.0
        if not return_metrics:
            return mean_loss
        keys = sorted({key for _, m in per_batch for key in m})
        return mean_loss, {key: sum(m.get(key, 0.0) for _, m in per_batch) / n for key in keys}

    def eval_step(self, data):
        self.model.eval()
        return self.eval_step_with_metrics(data, metrics=False)[0]

    def eval_step_with_metrics(self, data, metrics=True):
        """-> (loss tensor, metrics dict) of one batch in whatever mode the model is in (the reference's method does not switch it)."""
        x, gt = self._batch(data)
        with torch.no_grad():
            pred = self.model(x)
            loss, loss_dict = self.model.compute_loss(pred, gt)
            return loss, (self.calculate_metrics(pred, gt, loss_dict) if metrics else loss_dict)

    def compute_loss(self, data):
        return self.compute_loss_with_dict(data)[0]

    def compute_loss_with_dict(self, data):
        x, gt = self._batch(data)
        return self.model.compute_loss(self.model(x), gt)

    @staticmethod
    def calculate_metrics(pred_distances, gt_distances, loss_dict):
        """The loss dict plus 'mae', 'mse' and 'relative_error' = mean(|pred - gt| / (gt + 1e-8)); one device-to-host copy."""
        err = (pred_distances - gt_distances).abs()
        mae, mse, rel = torch.stack([err.mean(), (err * err).mean(), (err / (gt_distances + 1e-8)).mean()]).tolist()
        return dict(loss_dict, mae=mae, mse=mse, relative_error=rel)

    def predict(self, data, return_uncertainty=False):
        if return_uncertainty:
            raise NotImplementedError("the distance decoder has no uncertainty output (the reference's branch expects a model "
                                      "that returns a pair)")
        self.model.eval()
        self.reset_model_states()
        with torch.no_grad():
            return self.model(data.get('input').to(self.device).float())

    def save_model(self, path):
        """One file with the model's and the optimiser's state under the reference's two keys."""
        state = {'model_state_dict': self.model.state_dict(), 'optimizer_state_dict': self.optimizer.state_dict()}
        torch.save(state, path)

    def load_model(self, path):
        state = torch.load(path, map_location=self.device)
        self.model.load_state_dict(state['model_state_dict'], strict=True)
        self.optimizer.load_state_dict(state['optimizer_state_dict'])

    def get_learning_rate(self):
        return self.optimizer.param_groups[0]['lr']

    def set_learning_rate(self, lr):
        for group in self.optimizer.param_groups:
            group['lr'] = lr

    def reset_model_states(self):
        reset = getattr(self.model, 'reset_states', None)
        if reset is not None:
            reset()


class AmpTrainer(Trainer):
    """``Trainer`` with the options of the reference's default fd configuration (trainfd.py:194-291); the step mirrors
    ``fn_trainer.Trainer.train_step``.  ``use_amp``: the GEMMs, data and weight gradients of the step on bf16 operands with f32
    accumulation (``train.gemm_precision``; BatchNorm statistics, neurons, softmax, loss and optimiser stay f32, as under autocast;
    block 0's xyz EdgeConvs form x_n - x_i in f32 first).  ``scaler``: a GradScaler, driven through scale / unscale_ / step / update
    when ``use_amp`` (bf16 needs no loss scaling; a reference script runs unchanged).  ``gradient_accumulation``: loss / n, clip and
    step on every n-th call.  ``edgeconv``: how blocks 1-3 run (``fd_train.edgeconv_form``); "factored" is the measured faster of
    the two in bf16."""

    def __init__(self, model, optimizer, device=None, input_type='pointcloud', vis_dir=None, threshold=0.5, eval_sample=False,
                 grad_clip=None, grad_clip_type='norm', use_amp=True, scaler=None, gradient_accumulation=1, edgeconv="factored"):
        super().__init__(model, optimizer, device=device, input_type=input_type, vis_dir=vis_dir, threshold=threshold,
                         eval_sample=eval_sample, grad_clip=grad_clip, grad_clip_type=grad_clip_type)
        if edgeconv not in ("feature", "factored"):
            raise ValueError("edgeconv must be 'feature' or 'factored'")
        if int(gradient_accumulation) < 1:
            raise ValueError("gradient_accumulation must be >= 1")
        self.use_amp, self.scaler, self.gradient_accumulation, self.edgeconv = bool(use_amp), scaler, int(gradient_accumulation), edgeconv
        self.accumulation_step = 0

    def _abort(self):
        self.optimizer.zero_grad()
        self.accumulation_step = 0
        return None, None

    def train_step(self, data):
        """-> (loss value, loss dict); (None, None) when the loss or a gradient is not finite (gradients zeroed, the accumulation
        counter reset); RuntimeError when a neighbour index outside its patch reached an EdgeConv backward."""
        from . import fd_train
        from . import train as T
        self.model.train()
        if self.accumulation_step == 0:
            self.optimizer.zero_grad()
        self.accumulation_step += 1
        self.reset_model_states()
        fd_train.take_bad_index_count()
        amp = self.use_amp and self.scaler is not None
        with T.gemm_precision("bf16" if self.use_amp else "f32"), fd_train.edgeconv_form(self.edgeconv):     # forward AND backward
            loss, loss_dict = self.compute_loss_with_dict(data)
            if not bool(torch.isfinite(loss)):
                print("WARNING: NaN/Inf in loss value")
                return self._abort()
            scaled = loss / self.gradient_accumulation if self.gradient_accumulation != 1 else loss
            (self.scaler.scale(scaled) if amp else scaled).backward()
        bad = fd_train.take_bad_index_count()
        if bad:
            self._abort()
            raise RuntimeError("fd training step: %d neighbour indices outside their patch reached the EdgeConv backward" % bad)
        if self.accumulation_step % self.gradient_accumulation == 0:
            total = None
            if amp:
                self.scaler.unscale_(self.optimizer)
            if self.grad_clip is not None and self.grad_clip > 0:
                if self.grad_clip_type == 'norm':
                    total = torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.grad_clip)
                else:
                    torch.nn.utils.clip_grad_value_(self.model.parameters(), self.grad_clip)
            if total is None:
                grads = [prm.grad for prm in self.model.parameters() if prm.grad is not None]
                total = torch.stack(torch._foreach_norm(grads)).sum()
            if not bool(torch.isfinite(total)):
                print("WARNING: NaN/Inf in gradients")
                return self._abort()
            if amp:
                self.scaler.step(self.optimizer)
                self.scaler.update()
            else:
                self.optimizer.step()
            self.optimizer.zero_grad()
            self.accumulation_step = 0
        return loss.item(), loss_dict


class GraphedTrainStep:
    """One optimisation step of ``Trainer`` / ``AmpTrainer`` for the batch shape of `example`, captured as a HIP graph and replayed
    (ours; the reference has no counterpart).  fd's step is some 1 400 launches with the host between them; a replay is one.

    The contract: a replay leaves the model's parameters and buffers and the optimiser's state bit for bit as
    ``trainer.train_step`` on the same batch would — step applied, batch skipped (non-finite loss or gradient: (None, None) and
    the eager warning) or an index outside its patch (RuntimeError, the eager message, counter taken).  So it is a drop-in for
    ``fn_trainer.run_epoch`` (``model`` and ``optimizer`` are exposed), and a batch of another shape simply runs the eager step.

    The three host decisions of the eager step are one device flag: skip = !isfinite(loss) | !isfinite(total) | (bad-index counter
    != 0).  Before ``optimizer.step()`` every parameter and every tensor of ``optimizer.state`` is copied to a shadow
    (``_foreach_copy_``); after it ONE launch of ``sapcu_multi_select`` (include/sapcu_train_step.h) puts the shadows back and
    zero-fills every gradient when the flag is set, and writes nothing when it is not.  No protocol of a particular optimiser is
    used: any ``capturable=True`` one works.  BatchNorm buffers are not put back — the eager step's forward has moved them too
    before it skips.  With ``clamp_parameters`` the graph ends with ``fn_trainer.clamp_neuron_parameters`` (after the restore, as
    ``run_epoch`` clamps after a skipped step too; call ``run_epoch`` with its own ``clamp_parameters=False`` then).

    Learning rate: a float ``param_groups[i]["lr"]`` is part of the captured launches, exactly as the eager step passes it (torch's
    optimisers do not compute the same bits from a float and from a device tensor of the same value: after ONE AdamW step 31 of
    this model's parameter tensors differ by an ulp, so a graph that read the rate from a tensor could not equal the eager step).
    (tests/test_gpu_fd_graph.py shows that difference.)  A call that finds another rate in the groups than the captured one —
    ``run_epoch``'s warm-up, a scheduler, ``set_learning_rate`` — runs the eager step; when the next call finds that rate again
    the step is captured anew with it (every launch recorded again, a new pool, new shadows) and replayed from then on.  So a float
    rate that changes at EVERY step never replays: each call is the eager step, counted in ``eager_fallbacks`` (``captures``
    counts the captures).  A rate that is a device tensor is read by the graph where it is: a per-step schedule that updates that
    tensor in place keeps the graph, and costs nothing.

    `warmup` eager steps on `example` run before the capture and are real optimisation steps; 0 is legal and changes nothing (one
    eager forward and backward runs so that libraries are set up, and what it moved is put back; the capture runs no kernel): the
    optimiser's state must then exist already or be that of Adam / AdamW, whose lazily created tensors start at zero (a first
    capture that is thrown away finds their names and shapes; creating them inside the kept graph would zero them at every replay).
    Dropout masks move from replay to replay: the model's ``dropout_generator`` (or the default one) is registered with the graph.

    Refused with ValueError before anything is captured: a GradScaler, gradient accumulation, an optimiser that is not
    ``capturable=True``, a model that is not on a ROCm device."""

    BLOCKS_PER_TENSOR = 8

    def __init__(self, trainer, example, warmup=3, clamp_parameters=False):
        self.trainer = tr = trainer
        if getattr(tr, "scaler", None) is not None:
            raise ValueError("fd_trainer.GraphedTrainStep: a GradScaler's skip logic lives on the host and is not captured")
        if int(getattr(tr, "gradient_accumulation", 1)) != 1:
            raise ValueError("fd_trainer.GraphedTrainStep: gradient accumulation is not supported (one step per replay)")
        if not all(g.get("capturable", False) for g in tr.optimizer.param_groups):
            raise ValueError("fd_trainer.GraphedTrainStep: build the optimiser with capturable=True")
        params = list(tr.model.parameters())
        if not params or not all(q.is_cuda for q in params):
            raise ValueError("fd_trainer.GraphedTrainStep: the model must be on a ROCm device (there is no CPU path)")
        from . import fd_train
        self.model, self.optimizer = tr.model, tr.optimizer
        self.clamp_parameters = bool(clamp_parameters)
        dev = params[0].device
        x, gt = tr._batch(example)
        self._x, self._gt = x.to(dev, copy=True), gt.to(dev, copy=True)
        for _ in range(int(warmup)):
            tr.train_step(example)
        self._counter = fd_train.bad_index_counter(dev)                  # must exist before the capture
        self._flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._captured_lr = self._pending_lr = None
        self.captures = 0                                                 # how often the step was captured (1 + the rates it met twice)
        self.eager_fallbacks = 0                                          # calls that ran trainer.train_step: another shape, or a new rate
        if int(warmup) == 0:
            self._first_use()
        torch.cuda.synchronize(dev)
        if not self.optimizer.state:
            self._create_optimizer_state()
        self._capture()

    def _first_use(self):
        """warmup = 0: nothing of the step has run in this process, and what libraries set up at their first use (torch's BLAS
        backend creates its handle and workspace at its first product) is not permitted inside a capture.  One eager forward and
        backward on `example`, whatever the model calls in them, with everything they move put back: BatchNorm buffers, the dropout
        generator's state, the bad-index counter, the gradients."""
        model, dev = self.model, self._flag.device
        buffers = list(model.buffers())
        kept = [b.clone() for b in buffers]
        gen = getattr(model, "dropout_generator", None)
        rng = gen.get_state() if gen is not None else torch.cuda.get_rng_state(dev)
        model.train()
        with self._contexts():
            from . import fd_train
            fd_train.distance_loss(model(self._x), self._gt).backward()
        self._counter.zero_()
        self.optimizer.zero_grad(set_to_none=True)
        with torch.no_grad():
            torch._foreach_copy_(buffers, kept)
        if gen is not None:
            gen.set_state(rng)
        else:
            torch.cuda.set_rng_state(rng, dev)

    def _learning_rates(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    @staticmethod
    def _same_rates(a, b):
        return a is not None and b is not None and len(a) == len(b) and all(
            (x is y) if (torch.is_tensor(x) or torch.is_tensor(y)) else (x == y) for x, y in zip(a, b))

    def _capture(self):
        """(Re)capture the step with the learning rates the groups hold now.  Everything that is written from outside the graph
        — inputs, flag, counter, the select tables — is allocated outside its memory pool: inside, the graph reuses memory between
        its own launches, and a replay would overwrite what was put there after the capture."""
        opt, dev = self.optimizer, self._flag.device
        self.graph = self._out = self._live = self._shadow = self._grads = None
        opt.zero_grad(set_to_none=True)
        owned = [prm for g in opt.param_groups for prm in g["params"]]
        capacity = 2 * len(owned) + sum(1 for prm in owned for v in opt.state.get(prm, {}).values() if torch.is_tensor(v))
        self._device_tables = [torch.zeros((capacity,), dtype=torch.int64, device=dev) for _ in range(3)]
        self._captured_lr, self._pending_lr = self._learning_rates(), None
        graph = self._new_graph()
        with torch.cuda.graph(graph):
            self._out = self._step(select=True)
        for tab, host in zip(self._device_tables, self._tables):         # the launch is recorded, nothing has run: fill them now
            tab[:len(host)].copy_(torch.tensor(host, dtype=torch.int64))
        torch.cuda.synchronize(dev)
        self.graph = graph
        self.captures += 1

    def _new_graph(self):
        graph = torch.cuda.CUDAGraph()
        gen = getattr(self.model, "dropout_generator", None)
        if gen is not None:                                               # the default generator is registered by the capture itself
            graph.register_generator_state(gen)
        return graph

    def _contexts(self):
        from . import fd_train
        from . import train as T
        tr, stack = self.trainer, contextlib.ExitStack()
        if hasattr(tr, "use_amp"):                                        # AmpTrainer's settings; Trainer runs in whatever is set
            stack.enter_context(T.gemm_precision("bf16" if tr.use_amp else "f32"))
            stack.enter_context(fd_train.edgeconv_form(tr.edgeconv))
        return stack

    def _create_optimizer_state(self):
        """warmup = 0 on a fresh optimiser: capture the step once and throw the graph away — no kernel runs, but ``optimizer.step()``
        has created its state, so the tensors' owners, names, shapes and dtypes are known; each is replaced by a zero tensor
        allocated outside any graph."""
        opt = self.optimizer
        if not isinstance(opt, (torch.optim.Adam, torch.optim.AdamW)):
            raise ValueError("fd_trainer.GraphedTrainStep: warmup=0 needs the state of %s to exist (run a step, or warmup >= 1); only "
                             "Adam / AdamW are known to start from zero" % type(opt).__name__)
        graph = self._new_graph()
        with torch.cuda.graph(graph):
            self._step(select=False)
        for st in opt.state.values():
            for key, v in list(st.items()):
                if torch.is_tensor(v):
                    st[key] = torch.zeros(v.shape, dtype=v.dtype, device=v.device)
        opt.zero_grad(set_to_none=True)
        del graph

    def _step(self, select):
        """The body of the graph: ``train_step`` with the host decisions as device values."""
        from . import _lib, fd_train, fn_trainer
        tr, model, opt = self.trainer, self.model, self.optimizer
        model.train()
        self._counter.zero_()
        opt.zero_grad(set_to_none=True)
        tr.reset_model_states()
        with self._contexts():
            loss = fd_train.distance_loss(model(self._x), self._gt)
            loss.backward()
        total = None
        if tr.grad_clip is not None and tr.grad_clip > 0:
            if tr.grad_clip_type == 'norm':
                total = torch.nn.utils.clip_grad_norm_(model.parameters(), tr.grad_clip)
            else:
                torch.nn.utils.clip_grad_value_(model.parameters(), tr.grad_clip)
        grads = [prm.grad for prm in model.parameters() if prm.grad is not None]
        if total is None:
            total = torch.stack(torch._foreach_norm(grads)).sum()
        if not select:
            opt.step()
            return None
        skip = ~torch.isfinite(loss.detach()) | ~torch.isfinite(total) | (self._counter[0] != 0)
        self._flag.copy_(skip.to(torch.int32).reshape(1))
        owned = [prm for g in opt.param_groups for prm in g["params"]]
        if any(prm.grad is not None and not opt.state.get(prm) for prm in owned):
            raise RuntimeError("fd_trainer.GraphedTrainStep: the optimiser has no state for a parameter that receives a gradient")
        live = owned + [v for prm in owned for v in opt.state.get(prm, {}).values() if torch.is_tensor(v)]
        shadow = [torch.empty_like(t) for t in live]
        torch._foreach_copy_(shadow, live)
        opt.step()
        for t in live + shadow + grads:
            if not t.is_contiguous() or (t.numel() * t.element_size()) % 4 or t.data_ptr() % 4:
                raise ValueError("fd_trainer.GraphedTrainStep: parameters, optimiser state and gradients must be contiguous 4-byte data")
        self._live, self._shadow, self._grads = live, shadow, [(prm, prm.grad) for prm in model.parameters() if prm.grad is not None]
        size = lambda t: t.numel() * t.element_size()
        self._tables = ([t.data_ptr() for t in live + grads], [t.data_ptr() for t in shadow] + [0] * len(grads),
                        [size(t) for t in live + grads])
        self.entries = count = len(live) + len(grads)
        d, s, n = self._device_tables
        if count > d.numel():
            raise RuntimeError("fd_trainer.GraphedTrainStep: the optimiser created state inside the capture")
        with torch.cuda.device(self._flag.device):
            _lib.check(_lib.load().sapcu_multi_select(_lib.ptr(self._flag), _lib.ptr(d), _lib.ptr(s), _lib.ptr(n), count,
                                                      self.BLOCKS_PER_TENSOR, _lib.current_stream()))
        if self.clamp_parameters:
            fn_trainer.clamp_neuron_parameters(model)
        return torch.stack([loss.detach().double(), total.double(), self._counter[0].double()])

    def run_added_work(self):
        """What a replay adds to the eager step's launches, run on its own (profiles/fd_train_step.py times it): the shadow copies and
        the select launch over this step's tables with a clear flag, the case of every batch that is not skipped."""
        from . import _lib
        clear = torch.zeros_like(self._flag)
        d, s, n = self._device_tables
        torch._foreach_copy_(self._shadow, self._live)
        with torch.cuda.device(clear.device):
            _lib.check(_lib.load().sapcu_multi_select(_lib.ptr(clear), _lib.ptr(d), _lib.ptr(s), _lib.ptr(n), self.entries,
                                                      self.BLOCKS_PER_TENSOR, _lib.current_stream()))

    def train_step(self, data):
        """-> what ``trainer.train_step(data)`` returns or raises, and the state it leaves in parameters, buffers and optimiser; one
        device-to-host copy.  (Gradients are outside the contract: a replay leaves them attached — zeros after a skip — where
        ``AmpTrainer.train_step`` leaves None.)"""
        tr = self.trainer
        x, gt = tr._batch(data)
        if x.shape != self._x.shape or gt.shape != self._gt.shape:       # e.g. a loader's last batch: the contract makes this legal
            self.eager_fallbacks += 1
            return tr.train_step(data)
        rates = self._learning_rates()
        if not self._same_rates(rates, self._captured_lr):               # a new rate: eager once, captured when it is seen again
            if not self._same_rates(rates, self._pending_lr):
                self._pending_lr = rates
                self.eager_fallbacks += 1
                return tr.train_step(data)
            self._capture()
        self._pending_lr = None
        self.model.train()
        self._x.copy_(x)
        self._gt.copy_(gt)
        self.graph.replay()
        # a replay moves parameters and BatchNorm statistics without any Python in-place op: the version counters the packed
        # inference blob follows do not move, so drop it; the gradients live where the graph wrote them
        self.model._packed_key = None
        for prm, grad in self._grads:
            prm.grad = grad
        loss, total, bad = self._out.tolist()
        if bad:
            self._counter.zero_()                                         # taken, as take_bad_index_count() leaves it
        if not math.isfinite(loss):                                       # the eager step stops here, before its backward
            print("WARNING: NaN/Inf in loss value")
            return None, None
        if bad:
            raise RuntimeError("fd training step: %d neighbour indices outside their patch reached the EdgeConv backward" % bad)
        if not math.isfinite(total):
            print("WARNING: NaN/Inf in gradients")
            return None, None
        return loss, {'total_loss': loss, 'distance_loss': loss}

    __call__ = train_step


def rotation_to_x(normal):
    """The rotation that takes unit vector `normal` to (1, 0, 0) (Rodrigues; identity when they already agree), the alignment the
    reference's Subsamplerfd applies to every patch (fd/transform.py:55-57)."""
    a = np.asarray(normal, np.float64)
    a = a / np.linalg.norm(a)
    b = np.array([1.0, 0.0, 0.0])
    v = np.cross(a, b)
    s2 = float(v @ v)
    if s2 == 0.0:
        return np.eye(3)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + K + K @ K * ((1.0 - float(a @ b)) / s2)


class SyntheticFdPatches(object):
    """Stand-in for the reference's fd training loader (fd/datacore.py + Subsamplerfd; config/fd.yaml: 16 patches of 100 points per
    cloud): batches {'input': [B, N, M, 3] f32, 'len': [B, N] f32, 'seed': [B, N, 3] f64, 'shape': B names}.  Each cloud is 2048
    points on an analytic sphere (radius 0.5) or torus (R = 0.35, r = 0.15) shell in a random pose; a seed sits at a known
    distance `len` outside the surface along the normal of its foot point; its patch is the M nearest cloud points minus the
    seed, rotated normal -> x.  Deterministic in (seed, batch index)."""

    SPHERE_R, TORUS_R, TORUS_r = 0.5, 0.35, 0.15

    def __init__(self, batches, batch_size=4, patches=16, points=100, seed=0, cloud_points=2048, band=(0.005, 0.03)):
        self.batches, self.batch_size, self.patches, self.points = batches, batch_size, patches, points
        self.seed, self.cloud_points, self.band = seed, cloud_points, band

    def __len__(self):
        return self.batches

    @classmethod
    def surface_distance(cls, shape, pose, points):
        """Analytic distance of world-space `points` [.., 3] to the surface of `shape` posed by the orthogonal matrix `pose`."""
        q = np.asarray(points, np.float64) @ pose                 # back to the shape's frame (pose^-1 = pose^T; row vectors)
        if shape == "sphere":
            return np.abs(np.linalg.norm(q, axis=-1) - cls.SPHERE_R)
        ring = np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - cls.TORUS_R
        return np.abs(np.sqrt(ring ** 2 + q[..., 2] ** 2) - cls.TORUS_r)

    def _surface(self, rng, shape, n):
        if shape == "sphere":
            nrm = rng.normal(size=(n, 3))
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            return nrm * self.SPHERE_R, nrm
        u, v = rng.uniform(0, 2 * np.pi, (2, n))
        R, r = self.TORUS_R, self.TORUS_r
        pts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], 1)
        nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
        return pts, nrm

    def _cloud(self, rng):
        shape = "sphere" if rng.random() < 0.5 else "torus"
        pose, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        cloud, _ = self._surface(rng, shape, self.cloud_points)
        foot, nrm = self._surface(rng, shape, self.patches)
        d = rng.uniform(self.band[0], self.band[1], self.patches)
        seeds = foot + d[:, None] * nrm                           # outside, closer to its foot point than any curvature radius
        cloud, seeds, nrm = cloud @ pose.T, seeds @ pose.T, nrm @ pose.T
        dist = ((seeds[:, None, :] - cloud[None, :, :]) ** 2).sum(-1)
        idx = np.argsort(dist, axis=1, kind="stable")[:, :self.points]
        patches = cloud[idx] - seeds[:, None, :]
        for i in range(self.patches):
            patches[i] = patches[i] @ rotation_to_x(nrm[i]).T
        return patches.astype(np.float32), d.astype(np.float32), seeds, shape, pose

    def __iter__(self):
        for b in range(self.batches):
            rng = np.random.default_rng([self.seed, b])
            clouds = [self._cloud(rng) for _ in range(self.batch_size)]
            yield {"input": torch.from_numpy(np.stack([c[0] for c in clouds])), "len": torch.from_numpy(np.stack([c[1] for c in clouds])),
                   "seed": torch.from_numpy(np.stack([c[2] for c in clouds])), "shape": [c[3] for c in clouds],
                   "pose": torch.from_numpy(np.stack([c[4] for c in clouds]))}
