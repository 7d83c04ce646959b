"""What fn's and fd's training drivers share (ours; the reference states each of them per network): the hooks a trainer gives
(``TrainerHooks``), the step after its backward (``finish_step``), the whole step replayed as one HIP graph (``GraphedTrainStep``),
and the batch loop with its parameter clamp (``run_epoch``, ``clamp_neuron_parameters``).  Nothing here knows a network or a loss:
``fn_trainer`` and ``fd_trainer`` build on it and keep these names importable."""
import contextlib
import math
import time

import numpy as np
import torch


class TrainerHooks:
    """The pieces of one optimisation step that differ between the networks.  ``Trainer.train_step`` is written over them, and
    ``GraphedTrainStep`` records the same pieces into a graph, so the two cannot drift apart.  A trainer also has ``model``,
    ``optimizer``, ``use_amp``, ``scaler``, ``gradient_accumulation``, ``accumulation_step``, ``grad_clip``, ``grad_clip_type`` and
    ``_batch(data) -> (input, target)`` on the device."""

    def _begin(self, x, gt):
        """Host work before the forward -> the warning of a batch that is refused here (nothing has run), or None."""
        return None

    def _prepare(self):
        """Device work before the forward; no synchronisation (it is captured)."""

    def _arithmetic(self):
        """The context the forward AND the backward run in."""
        return contextlib.nullcontext()

    def _loss(self, x, gt):
        """No synchronisation -> (loss tensor, {name: device scalar} of the returned loss dict, [(warning, device bool: finite)] —
        what the eager step tests, in this order, before its backward)."""
        raise NotImplementedError

    def _bad_index_counter(self, device):
        """The device counter that must read 0 after the backward (else RuntimeError(BAD_INDEX_ERROR % count)), or None."""
        return None

    def _finish(self, update=None):
        """``finish_step`` with this network's clipping rule."""
        raise NotImplementedError

    def _skip(self):
        """A batch refused at one of ``_loss``'s tests."""
        self.accumulation_step = 0
        return None, None

    def _abort(self):
        self.optimizer.zero_grad()
        self.accumulation_step = 0
        return None, None


def finish_step(tr, unscale, clip, update=None):
    """An optimisation step from the end of its backward on: ``scaler.unscale_`` (when `unscale` and a scaler is driven), clipping
    by norm or value (when `clip`), the global gradient norm when clipping gave none, the finite decision, the update, ``zero_grad``
    and the accumulation reset.  -> False for a skipped batch (warning printed, ``tr._abort()`` called), else True.  `update`: the
    graph body's stand-in for everything from the decision on, called with the norm (the decision is a device flag there)."""
    model, opt = tr.model, tr.optimizer
    amp = tr.use_amp and tr.scaler is not None
    if unscale and amp:
        tr.scaler.unscale_(opt)
    total = None
    if clip:
        if tr.grad_clip_type == 'norm':
            total = torch.nn.utils.clip_grad_norm_(model.parameters(), tr.grad_clip)
        else:
            torch.nn.utils.clip_grad_value_(model.parameters(), tr.grad_clip)
    if total is None:
        grads = [prm.grad for prm in model.parameters() if prm.grad is not None]
        total = torch.stack(torch._foreach_norm(grads)).sum() if grads else torch.zeros(())
    if update is not None:
        return update(total)
    # the reference tests every gradient tensor for NaN/Inf (one host sync each); the global norm is finite exactly when all of
    # them are, so one sync decides
    if not bool(torch.isfinite(total)):
        print("WARNING: NaN/Inf in gradients")
        tr._abort()
        return False
    if amp:
        tr.scaler.step(opt)
        tr.scaler.update()
    else:
        opt.step()
    opt.zero_grad()
    tr.accumulation_step = 0
    return True


def clamp_neuron_parameters(model):
    """The post-step clamp of the neuron parameters the reference's fd training loop applies (trainfd.py:305-313); trainfn.py has
    none — the forward clamps the values it uses either way (fn/snn_coder.py:87-110), this keeps the stored parameters in range."""
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if 'membrane_decay' in name:
                prm.data.clamp_(0.1, 0.99)
            elif 'threshold_adapt' in name:
                prm.data.clamp_(0.001, 0.1)
            elif 'refractory_decay' in name:
                prm.data.clamp_(0.1, 0.95)


def run_epoch(trainer, train_loader, it=0, epoch_it=0, lr=None, warmup_steps=0, warmup_factor=0.01, state_reset_freq=0, print_every=0,
              log=print, clamp_parameters=False):
    """One pass over ``train_loader`` — the batch loop of the reference's trainfn.py:253-330 without its logging / checkpoint
    side effects: iteration counter, SNN state reset every ``state_reset_freq`` iterations, linear learning-rate warm-up, skipped
    invalid or non-finite batches, per-iteration losses, samples per second; optionally the neuron-parameter clamp of the fd loop.
    -> (it, losses, stats)."""
    model, optimizer = trainer.model, trainer.optimizer
    lr = optimizer.param_groups[0]["lr"] if lr is None else lr
    losses, skipped, start, seen = [], 0, time.time(), 0
    for batch in train_loader:
        it += 1
        if "input" not in batch:                                         # trainfn.py:259-260
            continue
        if state_reset_freq > 0 and it % state_reset_freq == 0 and hasattr(model, "reset_states"):
            model.reset_states()
        if warmup_steps > 0 and it < warmup_steps:                       # trainfn.py:266-269
            f = warmup_factor + (1 - warmup_factor) * (it / warmup_steps)
            for g in optimizer.param_groups:
                g["lr"] = lr * f
        loss, _ = trainer.train_step(batch)
        if clamp_parameters:                                             # (trainfd.py:305-313; off = trainfn.py's behaviour)
            clamp_neuron_parameters(model)
        if loss is None:
            skipped += 1
            continue
        losses.append(float(loss))
        seen += int(batch["input"].shape[0])
        if print_every > 0 and it % print_every == 0:
            log("[Epoch %03d] it=%06d, loss=%.6f, avg_loss=%.6f, lr=%.6f, samples/s=%.1f" % (
                epoch_it, it, losses[-1], float(np.mean(losses[-print_every:])), optimizer.param_groups[0]["lr"],
                seen / max(time.time() - start, 1e-9)))
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    dt = time.time() - start
    return it, losses, {"clouds": seen, "seconds": dt, "clouds_per_s": seen / max(dt, 1e-9), "skipped": skipped}


class GraphedTrainStep:
    """One optimisation step of an fn or fd trainer for the batch shape of `example`, captured as a HIP graph and replayed (ours;
    the reference has no counterpart).  A step is some 1 300 - 1 400 launches with the host between them; a replay is one.

    The contract: a replay leaves the model's parameters and buffers and the optimiser's state bit for bit as
    ``trainer.train_step`` on the same batch would — step applied, batch skipped (non-finite prediction, loss or gradient:
    (None, None) and the eager warning) or an index outside its patch (RuntimeError, the eager message, counter taken).  So it is a
    drop-in for ``run_epoch`` (``model`` and ``optimizer`` are exposed), and a batch of another shape simply runs the eager step.

    The graph body is the trainer's own hooks (``TrainerHooks``): ``_prepare``, ``_loss`` and the backward inside ``_arithmetic``,
    then ``_finish``.  A batch that ``_begin`` refuses on the host (fn: a non-finite input) is not replayed at all, as the eager step
    runs nothing for it.  The other host decisions of the eager step are one device flag: skip = any test of ``_loss`` failed |
    !isfinite(total) | (bad-index counter != 0).  Before ``optimizer.step()`` every parameter and every tensor of
    ``optimizer.state`` is copied to a shadow (``_foreach_copy_``); after it ONE launch of ``sapcu_multi_select``
    (include/sapcu_train_step.h) puts the shadows back and zero-fills every gradient when the flag is set, and writes nothing when
    it is not.  No protocol of a particular optimiser is used: any ``capturable=True`` one works.  BatchNorm buffers are not put
    back — the eager step's forward has moved them too before it skips.  With ``clamp_parameters`` the graph ends with
    ``clamp_neuron_parameters`` (after the restore, as ``run_epoch`` clamps after a skipped step too; call ``run_epoch`` with its
    own ``clamp_parameters=False`` then).

    Learning rate: a float ``param_groups[i]["lr"]`` is part of the captured launches, exactly as the eager step passes it (torch's
    optimisers do not compute the same bits from a float and from a device tensor of the same value: after ONE AdamW step 31 of
    fd's parameter tensors differ by an ulp, so a graph that read the rate from a tensor could not equal the eager step).
    (tests/test_gpu_fd_graph.py shows that difference.)  A call that finds another rate in the groups than the captured one —
    ``run_epoch``'s warm-up, a scheduler, ``set_learning_rate`` — runs the eager step; when the next call finds that rate again
    the step is captured anew with it (every launch recorded again, a new pool, new shadows) and replayed from then on.  So a float
    rate that changes at EVERY step never replays: each call is the eager step, counted in ``eager_fallbacks`` (``captures``
    counts the captures, ``replays`` the replays).  A rate that is a device tensor is read by the graph where it is: a per-step
    schedule that updates that tensor in place keeps the graph, and costs nothing.

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
        if tr.scaler is not None:
            raise ValueError("GraphedTrainStep: a GradScaler's skip logic lives on the host and is not captured")
        if int(tr.gradient_accumulation) != 1:
            raise ValueError("GraphedTrainStep: gradient accumulation is not supported (one step per replay)")
        if not all(g.get("capturable", False) for g in tr.optimizer.param_groups):
            raise ValueError("GraphedTrainStep: build the optimiser with capturable=True")
        params = list(tr.model.parameters())
        if not params or not all(q.is_cuda for q in params):
            raise ValueError("GraphedTrainStep: the model must be on a ROCm device (there is no CPU path)")
        self.model, self.optimizer = tr.model, tr.optimizer
        self.clamp_parameters = bool(clamp_parameters)
        dev = params[0].device
        x, gt = tr._batch(example)
        self._x, self._gt = x.to(dev, copy=True), gt.to(dev, copy=True)
        for _ in range(int(warmup)):
            tr.train_step(example)
        self._counter = tr._bad_index_counter(dev)                       # must exist before the capture
        self._flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._captured_lr = self._pending_lr = None
        self.captures = 0                                                 # how often the step was captured (1 + the rates it met twice)
        self.eager_fallbacks = 0                                          # calls that ran trainer.train_step: another shape, or a new rate
        self.replays = 0
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
        tr, model, dev = self.trainer, self.model, self._flag.device
        buffers = list(model.buffers())
        kept = [b.clone() for b in buffers]
        gen = getattr(model, "dropout_generator", None)
        rng = gen.get_state() if gen is not None else torch.cuda.get_rng_state(dev)
        model.train()
        with tr._arithmetic():
            tr._loss(self._x, self._gt)[0].backward()
        if self._counter is not None:
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

    def _create_optimizer_state(self):
        """warmup = 0 on a fresh optimiser: capture the step once and throw the graph away — no kernel runs, but ``optimizer.step()``
        has created its state, so the tensors' owners, names, shapes and dtypes are known; each is replaced by a zero tensor
        allocated outside any graph."""
        opt = self.optimizer
        if not isinstance(opt, (torch.optim.Adam, torch.optim.AdamW)):
            raise ValueError("GraphedTrainStep: warmup=0 needs the state of %s to exist (run a step, or warmup >= 1); only "
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
        tr, model, opt = self.trainer, self.model, self.optimizer
        model.train()
        if self._counter is not None:
            self._counter.zero_()
        opt.zero_grad(set_to_none=True)
        tr._prepare()
        with tr._arithmetic():
            loss, scalars, tests = tr._loss(self._x, self._gt)
            loss.backward()
        if not select:
            return tr._finish(update=lambda total: opt.step())
        self._names, self._warnings = list(scalars), [text for text, _ in tests]
        failed = [~ok.reshape(()) for _, ok in tests]
        return tr._finish(update=lambda total: self._guarded_update(total, list(scalars.values()), failed))

    def _guarded_update(self, total, scalars, failed):
        """``optimizer.step()`` between the shadow copies and the select launch -> what the host reads after a replay: the loss
        dict's scalars, the gradient norm, the bad-index count, the failed tests."""
        model, opt = self.model, self.optimizer
        skip = ~torch.isfinite(total)
        for term in failed + ([self._counter[0] != 0] if self._counter is not None else []):
            skip = skip | term
        self._flag.copy_(skip.to(torch.int32).reshape(1))
        grads = [prm.grad for prm in model.parameters() if prm.grad is not None]
        owned = [prm for g in opt.param_groups for prm in g["params"]]
        if any(prm.grad is not None and not opt.state.get(prm) for prm in owned):
            raise RuntimeError("GraphedTrainStep: the optimiser has no state for a parameter that receives a gradient")
        live = owned + [v for prm in owned for v in opt.state.get(prm, {}).values() if torch.is_tensor(v)]
        shadow = [torch.empty_like(t) for t in live]
        torch._foreach_copy_(shadow, live)
        opt.step()
        for t in live + shadow + grads:
            if not t.is_contiguous() or (t.numel() * t.element_size()) % 4 or t.data_ptr() % 4:
                raise ValueError("GraphedTrainStep: parameters, optimiser state and gradients must be contiguous 4-byte data")
        self._live, self._shadow, self._grads = live, shadow, [(prm, prm.grad) for prm in model.parameters() if prm.grad is not None]
        size = lambda t: t.numel() * t.element_size()
        self._tables = ([t.data_ptr() for t in live + grads], [t.data_ptr() for t in shadow] + [0] * len(grads),
                        [size(t) for t in live + grads])
        self.entries = len(live) + len(grads)
        if self.entries > self._device_tables[0].numel():
            raise RuntimeError("GraphedTrainStep: the optimiser created state inside the capture")
        self._select(self._flag)
        if self.clamp_parameters:
            clamp_neuron_parameters(model)
        counter = [self._counter[0]] if self._counter is not None else []
        return torch.stack([v.detach().double().reshape(()) for v in scalars + [total] + counter + failed])

    def _select(self, flag):
        from . import _lib
        d, s, n = self._device_tables
        with torch.cuda.device(flag.device):
            _lib.check(_lib.load().sapcu_multi_select(_lib.ptr(flag), _lib.ptr(d), _lib.ptr(s), _lib.ptr(n), self.entries,
                                                      self.BLOCKS_PER_TENSOR, _lib.current_stream()))

    def run_added_work(self):
        """What a replay adds to the eager step's launches, run on its own (profiles/fd_train_step.py times it): the shadow copies and
        the select launch over this step's tables with a clear flag, the case of every batch that is not skipped."""
        torch._foreach_copy_(self._shadow, self._live)
        self._select(torch.zeros_like(self._flag))

    def _eager(self, data):
        self.eager_fallbacks += 1
        self.optimizer.zero_grad(set_to_none=True)                        # a replay leaves its gradients attached; fn's eager step adds to what it finds
        return self.trainer.train_step(data)

    def train_step(self, data):
        """-> what ``trainer.train_step(data)`` returns or raises, and the state it leaves in parameters, buffers and optimiser; one
        device-to-host copy (and the one of ``_begin``, where the trainer has such a test).  (Gradients are outside the contract: a
        replay leaves them attached — zeros after a skip — where the eager step leaves None.)"""
        tr = self.trainer
        x, gt = tr._batch(data)
        if x.shape != self._x.shape or gt.shape != self._gt.shape:       # e.g. a loader's last batch: the contract makes this legal
            return self._eager(data)
        rates = self._learning_rates()
        if not self._same_rates(rates, self._captured_lr):               # a new rate: eager once, captured when it is seen again
            if not self._same_rates(rates, self._pending_lr):
                self._pending_lr = rates
                return self._eager(data)
            self._capture()
        self._pending_lr = None
        self.model.train()
        warning = tr._begin(x, gt)
        if warning is not None:                                           # the eager step stops here, before its forward
            print(warning)
            return None, None
        self._x.copy_(x)
        self._gt.copy_(gt)
        self.graph.replay()
        self.replays += 1
        # a replay moves parameters and BatchNorm statistics without any Python in-place op: the version counters the packed
        # inference blob follows do not move, so drop it; the gradients live where the graph wrote them
        self.model._packed_key = None
        for prm, grad in self._grads:
            prm.grad = grad
        out = self._out.tolist()
        k = len(self._names)
        values, total = dict(zip(self._names, out[:k])), out[k]
        bad = int(out[k + 1]) if self._counter is not None else 0
        if bad:
            self._counter.zero_()                                         # taken, as take_bad_index_count() leaves it
        for text, failed in zip(self._warnings, out[len(out) - len(self._warnings):]):
            if failed:                                                    # the eager step stops here, before its backward
                print(text)
                return tr._skip()
        tr.accumulation_step = 0
        if bad:
            raise RuntimeError(tr.BAD_INDEX_ERROR % bad)
        if not math.isfinite(total):
            print("WARNING: NaN/Inf in gradients")
            return None, None
        return values["total_loss"], values

    __call__ = train_step
