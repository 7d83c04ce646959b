"""Training forward of fd (row f-5): ``EnhancedSNNDistanceEstimation.forward`` in train() mode (/root/reference/fd/snn_coder.py:392-492,
711-725) as ``torch.autograd.Function``s over the HIP ops of include/sapcu_fd_train.h (csrc/fd_train_ops.hip) and the GEMM,
weight-gradient, BatchNorm-backward and kNN entry points fn's training already uses (sapcu_amd/train.py).

Two facts of the reference shape this module:

* The encoder DETACHES its neuron state between time steps (fd/snn_coder.py:438-442, 467-471): every step is one single-step neuron
  with the carried state as constants (``neuron_step_train``), not fn's T-step self-loop.  ``threshold_adapt`` and
  ``refractory_decay`` therefore get no gradient at all (``grad is None``), ``snn_fc.membrane_decay`` gets exactly zero, and
  ``threshold_base`` only through the step that starts from it.
* In train() mode the spikes are {0, 1}, squared distances between spike vectors are small integers, and most rows of the
  feature-space kNN of blocks 1-3 have an exact tie at rank k.  Which neighbour ``torch.topk`` keeps there is unspecified; when this
  module runs free it applies ``sapcu_patch_knn``'s rule — descending score, equal scores by ascending index.  A free run can
  therefore not be compared with a reference run: parity is teacher-forced on the reference's own tables (``knn=``) and spikes
  (``force_spikes=``).

bf16: every GEMM / weight gradient here goes through ``train._gemm`` / ``_wgrad`` and so follows ``train.gemm_precision``;
``edgeconv_form("factored")`` runs blocks 1-3 through ``edgeconv_factored`` (include/sapcu_fd_edgeconv.h, csrc/fd_edgeconv_ops.hip),
which never builds the [P M kk, 2C] edge tensors.  ``fd_trainer.AmpTrainer`` drives both, a GradScaler and gradient accumulation.

``fd_trainer.GraphedTrainStep`` replays the whole step as one HIP graph: nothing here synchronises or reads the device (the
bad-index counter is a device tensor, ``bad_index_counter``), and a replay leaves exactly the state the eager step leaves.

Not built, and refused where a caller could ask for it: ``use_snn_decoder=True``, DataParallel.
The decoder works on [P, <= 256] tensors: its Linear / BatchNorm layers are the HIP ops of
train.py, GELU, LayerNorm, the softmax over heads, Softplus, the loss and the dropout masks are torch ops, as in fn's training.
"""
import torch

from . import _lib
from . import train as T

F = torch.nn.functional
_BAD = {}            # device -> one int32 counter: indices outside their patch met by the EdgeConv backwards on that device
EDGE_LDS_LIMIT = 64 * 1024      # bytes of LDS the EdgeConv backward may use for a patch's inverse table (csrc/fd_train_ops.hip)


def _need_cuda(x, what):
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError("%s: expected a float32 tensor on a ROCm device (there is no CPU path)" % what)


def _check_patch_shape(M, kk):
    """The EdgeConv backward keeps a patch's inverse neighbour table (2 M kk + M + 1 ints) in LDS: a shape beyond its limit is
    refused here, in the forward, not later inside loss.backward()."""
    need = T.group_lds_bytes(M, M * kk)
    if need > EDGE_LDS_LIMIT:
        raise ValueError("EdgeConv training op: %d points x %d neighbours per patch need %d bytes of LDS in the backward, the limit is %d"
                         % (M, kk, need, EDGE_LDS_LIMIT))


def bad_index_counter(device):
    """The int32 [1] counter of `device`, created (zero) on first use.  A HIP-graph capture of the step needs it to exist before
    the capture begins — a tensor created inside one would be zeroed again by every replay."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    acc = _BAD.get(device)
    if acc is None:
        acc = _BAD[device] = torch.zeros((1,), dtype=torch.int32, device=device)
    return acc


def take_bad_index_count():
    """Neighbour indices outside their patch met by the EdgeConv backwards since the last call, summed over devices (one host
    sync per device), and reset.  Anything but 0 means the gradients of that step are wrong: ``fd_trainer.Trainer`` calls this
    after every backward and fails the step; a caller that drives ``loss.backward()`` itself must do the same.  The state is one
    4-byte counter per device, however many steps run between two calls."""
    n = 0
    for acc in _BAD.values():
        n += int(acc.item())
        acc.zero_()
    return n


class _NeuronStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, md, ta, rd, tb, dT, rh, m_in, th_in, r_in, force):
        _need_cuda(x, "neuron_step_train")
        eif = dT is not None
        x = x.contiguous()
        rows, ch = x.shape
        prm = [None if p is None else p.detach().contiguous() for p in (md, ta, rd, tb, dT, rh)]
        state = [None if s is None else s.contiguous() for s in (m_in, th_in, r_in)]
        force = None if force is None else force.contiguous()
        sp, m, th, r, pre = (torch.empty_like(x) for _ in range(5))
        _lib.call("sapcu_fd_neuron_step_forward", x.device, x, rows, ch, int(eif), *prm, *state, force, sp, m, th, r, pre)
        ctx.eif, ctx.prm, ctx.state = eif, prm, state
        ctx.save_for_backward(x)
        ctx.mark_non_differentiable(m, th, r, pre)
        return sp, m, th, r, pre

    @staticmethod
    def backward(ctx, g_sp, *_unused):
        (x,) = ctx.saved_tensors
        rows, ch = x.shape
        md, _, _, tb, dT, rh = ctx.prm
        gx = torch.empty_like(x)
        gmd, gtb = torch.empty_like(md), torch.empty_like(tb)
        gdT, grh = (torch.empty_like(dT), torch.empty_like(rh)) if ctx.eif else (None, None)
        ws, nbytes = T._empty_ws("sapcu_fd_neuron_step_workspace_bytes", (rows, ch), x.device)
        _lib.call("sapcu_fd_neuron_step_backward", x.device, x, g_sp.contiguous(), rows, ch, int(ctx.eif), md, tb, dT, rh, *ctx.state,
                  gx, gmd, gtb, gdT, grh, ws, nbytes)
        return gx, gmd, None, None, gtb, gdT, grh, None, None, None, None


def neuron_step_train(x, prm, state=None, force_spikes=None):
    """One neuron step in training mode on x [rows, C].  prm: dict with the raw ``membrane_decay``, ``threshold_adapt``,
    ``refractory_decay``, ``threshold_base`` (LIF) plus ``delta_T``, ``theta_rh`` (EIF).  state: None (first step) or the detached
    (membrane, threshold, refractory) of the previous step.  -> (hard spikes, (membrane, threshold, refractory), u = m - theta);
    differentiable w.r.t. x, membrane_decay, threshold_base (first step only), delta_T and theta_rh."""
    m_in, th_in, r_in = state if state is not None else (None, None, None)
    sp, m, th, r, pre = _NeuronStep.apply(x, prm["membrane_decay"], prm["threshold_adapt"], prm["refractory_decay"], prm["threshold_base"],
                                          prm.get("delta_T"), prm.get("theta_rh"), m_in, th_in, r_in, force_spikes)
    return sp, (m, th, r), pre


def _pad32(n):
    return (n + 31) // 32 * 32


def edge_feature_forward(x, idx, out_channels=None):
    """The EdgeConv graph feature as a plain op: x [P*M, C], idx int32 [P, M, kk] -> [P*M*kk, out_channels] = [x[nbr] - x[i] | x[nbr] | 0]."""
    _need_cuda(x, "edge_feature")
    P, M, kk = idx.shape
    _check_patch_shape(M, kk)
    c = x.shape[1]
    oc = 2 * c if out_channels is None else int(out_channels)
    x, idx = x.contiguous(), idx.contiguous()
    out = torch.empty((P * M * kk, oc), dtype=torch.float32, device=x.device)
    _lib.call("sapcu_fd_edge_feature_forward", x.device, x, c, idx, P, M, kk, c, oc, out, None)
    return out


def _edge_feature_backward(g, idx, c):
    P, M, kk = idx.shape
    gx = torch.empty((P * M, c), dtype=torch.float32, device=g.device)
    bad = torch.empty((1,), dtype=torch.int32, device=g.device)
    _lib.call("sapcu_fd_edge_feature_backward", g.device, g, idx, P, M, kk, c, g.shape[1], gx, c, bad)
    bad_index_counter(g.device).add_(bad)
    return gx


class _EdgeFeature(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, out_channels):
        ctx.idx, ctx.c = idx.contiguous(), x.shape[1]
        return edge_feature_forward(x, ctx.idx, out_channels)

    @staticmethod
    def backward(ctx, g):
        return _edge_feature_backward(g.contiguous(), ctx.idx, ctx.c), None, None


def edge_feature(x, idx, out_channels=None):
    """Differentiable ``get_graph_feature`` (fd/snn_coder.py:52-68) on channels-last rows; see edge_feature_forward."""
    return _EdgeFeature.apply(x, idx, out_channels)


def _bn_stats(y, eps):
    rows, ch = y.shape
    if rows < 2:
        raise ValueError("BatchNorm in training mode needs more than 1 value per channel (got %d rows)" % rows)
    mean, var, invstd = (torch.empty((ch,), dtype=torch.float32, device=y.device) for _ in range(3))
    ws, nbytes = T._empty_ws("sapcu_fd_bn_stats_workspace_bytes", (rows, ch), y.device)
    _lib.call("sapcu_fd_bn_stats", y.device, y, rows, ch, float(eps), mean, var, invstd, ws, nbytes)
    return mean, var, invstd


def _update_running(running, mean, var, rows, reps):
    """nn.BatchNorm's train()-mode bookkeeping, `reps` times over (a layer whose value is the same at every time step is
    computed once, its buffers still move as if it had run `reps` times)."""
    if running is None:
        return
    r_mean, r_var, n_tracked, momentum = running
    with torch.no_grad():
        for _ in range(reps):
            r_mean.mul_(1.0 - momentum).add_(mean, alpha=momentum)
            r_var.mul_(1.0 - momentum).add_(var, alpha=momentum * rows / (rows - 1.0))
        if n_tracked is not None:
            n_tracked.add_(reps)


class _ConvBnLreluMax(torch.autograd.Function):
    """[EdgeConv feature ->] 1x1 convolution (no bias) -> BatchNorm (batch statistics) -> LeakyReLU(0.2) -> max over each group of
    `group` rows.  With idx the input is x [P*M, C] and the feature is built here and again in the backward (it is 2 kk times
    the size of x and never kept)."""

    @staticmethod
    def forward(ctx, x, idx, weight, gamma, beta, group, eps, running, reps):
        _need_cuda(x, "conv_bn_lrelu_max")
        dev = x.device
        x = x.contiguous()
        w = weight.detach().reshape(weight.shape[0], -1)
        cin, cout = w.shape[1], w.shape[0]
        if cout % 32:
            raise ValueError("conv_bn_lrelu_max: output channels must be a multiple of 32 (got %d)" % cout)
        w = F.pad(w, (0, _pad32(cin) - cin)).contiguous()
        ga, be = gamma.detach().contiguous(), beta.detach().contiguous()
        if idx is not None:
            idx = idx.contiguous()
            a = edge_feature_forward(x, idx, w.shape[1])
        else:
            a = x if cin == w.shape[1] else F.pad(x, (0, w.shape[1] - cin))
        rows = a.shape[0]
        if rows % group:
            raise ValueError("conv_bn_lrelu_max: %d rows are not whole groups of %d" % (rows, group))
        y = torch.empty((rows, cout), dtype=torch.float32, device=dev)
        T._gemm(a, w, None, y)
        mean, var, invstd = _bn_stats(y, eps)
        out = torch.empty((rows // group, cout), dtype=torch.float32, device=dev)
        arg = torch.empty((rows // group, cout), dtype=torch.int32, device=dev)
        _lib.call("sapcu_fd_bn_lrelu_max_forward", dev, y, rows // group, int(group), cout, mean, invstd, ga, be, out, arg)
        _update_running(running, mean, var, rows, int(reps))
        ctx.save_for_backward(x, w, ga, be, y, mean, invstd, arg)
        ctx.idx, ctx.group, ctx.cin, ctx.wshape = idx, int(group), cin, weight.shape
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, ga, be, y, mean, invstd, arg = ctx.saved_tensors
        dev = x.device
        rows, cout = y.shape
        kpad = w.shape[1]
        gz, dy = torch.empty_like(y), torch.empty_like(y)
        dgamma, dbeta = torch.empty_like(ga), torch.empty_like(be)
        dw = torch.empty_like(w)
        ws, nbytes = T._empty_ws("sapcu_train_workspace_bytes", (rows, cout, kpad), dev)
        dx = None
        _lib.call("sapcu_fd_bn_lrelu_max_backward", dev, y, g.contiguous(), arg, rows // ctx.group, ctx.group, cout, mean, invstd, ga, be, gz)
        _lib.call("sapcu_bn_train_backward", dev, y, gz, rows, cout, ga, mean, invstd, dy, dgamma, dbeta, ws, nbytes)
        del gz
        if ctx.idx is not None:
            a = edge_feature_forward(x, ctx.idx, kpad)
        else:
            a = x if ctx.cin == kpad else F.pad(x, (0, kpad - ctx.cin))
        T._wgrad(dy, a, rows, cout, kpad, dw, None, ws, nbytes)
        del a
        if ctx.needs_input_grad[0]:
            da = torch.empty((rows, kpad), dtype=torch.float32, device=dev)
            T._gemm(dy, w.t().contiguous(), None, da)                # da[r, k] = dy[r, n] . (W^T)[k, n]^T
            dx = _edge_feature_backward(da, ctx.idx, x.shape[1]) if ctx.idx is not None else da[:, :ctx.cin]
        return dx, None, dw[:, :ctx.cin].reshape(ctx.wshape), dgamma, dbeta, None, None, None, None


def conv_bn_lrelu_max(x, weight, gamma, beta, group=1, idx=None, eps=1e-5, running=None, reps=1):
    """x [rows, c_in] (idx None) or x [P*M, C] with idx int32 [P, M, kk] (the EdgeConv feature of x is the convolution's input)
    -> [rows / group, c_out]: max over each `group` consecutive rows of LeakyReLU_0.2(BatchNorm_train(conv1x1(.))); the arg-max
    tie goes to the first row.  group = 1 is Conv + BatchNorm + LeakyReLU.  running: as train.conv_bn_train, updated `reps` times."""
    return _ConvBnLreluMax.apply(x, idx, weight, gamma, beta, group, eps, running, reps)


# How blocks 1-3 of fd_train_forward evaluate their EdgeConv: "feature" = conv_bn_lrelu_max(idx=...) — the [P M kk, 2C] graph
# feature is built, forward and backward; "factored" = edgeconv_factored — one point-level GEMM and gathers (the parity reference
# stays "feature"; fd_trainer.AmpTrainer selects the form).  Block 0's xyz EdgeConvs (C = 3) are on the feature path in both:
# x_n - x_i cancels and must be formed in f32 before any rounding.
_EDGECONV_FORM = ["feature"]


class edgeconv_form(object):
    """``with edgeconv_form("factored"): loss = ...; loss.backward()`` — in the style of ``train.gemm_precision``.  The form is read
    in the forward; the backward of an op is the backward of the form its forward ran in."""

    def __init__(self, form):
        if form not in ("feature", "factored"):
            raise ValueError("edgeconv_form: 'feature' or 'factored'")
        self.form = form

    def __enter__(self):
        self.prev = _EDGECONV_FORM[0]
        _EDGECONV_FORM[0] = self.form
        return self

    def __exit__(self, *exc):
        _EDGECONV_FORM[0] = self.prev
        return False


def _edgeconv_factored_forward(x, wst, idx, ga, be, eps):
    """x [P*M, C], wst = [W1 ; W2] [2 cout, C], idx int32 [P, M, kk] -> ab = [x W1^T | x W2^T], mean, var, invstd, out, arg."""
    P, M, kk = idx.shape
    cout, dev = wst.shape[0] // 2, x.device
    ab = torch.empty((P * M, 2 * cout), dtype=torch.float32, device=dev)
    T._gemm(x, wst, None, ab)
    mean, var, invstd = (torch.empty((cout,), dtype=torch.float32, device=dev) for _ in range(3))
    ws, nbytes = T._empty_ws("sapcu_fd_edgeconv_stats_workspace_bytes", (P, M, kk, cout), dev)
    _lib.call("sapcu_fd_edgeconv_stats", dev, ab, idx, P, M, kk, cout, float(eps), mean, var, invstd, None, ws, nbytes)
    out = torch.empty((P * M, cout), dtype=torch.float32, device=dev)
    arg = torch.empty((P * M, cout), dtype=torch.int32, device=dev)
    _lib.call("sapcu_fd_edgeconv_max_forward", dev, ab, idx, P, M, kk, cout, mean, invstd, ga, be, out, arg)
    return ab, mean, var, invstd, out, arg


def _edgeconv_factored_backward(x, wst, idx, ga, be, ab, mean, invstd, arg, g, need_dx=True):
    """-> dx [P*M, C] | None, dwst [2 cout, C], dgamma, dbeta: the three HIP passes of sapcu_fd_edgeconv_backward, then ONE
    point-level weight gradient and ONE point-level GEMM."""
    P, M, kk = idx.shape
    rows, cin = x.shape
    cout, dev = wst.shape[0] // 2, x.device
    gab = torch.empty_like(ab)
    dgamma, dbeta = torch.empty_like(ga), torch.empty_like(be)
    bad = torch.empty((1,), dtype=torch.int32, device=dev)
    ws, nbytes = T._empty_ws("sapcu_fd_edgeconv_backward_workspace_bytes", (P, M, kk, cout), dev)
    _lib.call("sapcu_fd_edgeconv_backward", dev, ab, idx, g, arg, P, M, kk, cout, mean, invstd, ga, be, gab, dgamma, dbeta, bad, ws, nbytes)
    bad_index_counter(dev).add_(bad)
    dwst = torch.empty_like(wst)
    tws, tbytes = T._empty_ws("sapcu_train_workspace_bytes", (rows, 2 * cout, cin), dev)
    T._wgrad(gab, x, rows, 2 * cout, cin, dwst, None, tws, tbytes)
    dx = None
    if need_dx:
        dx = torch.empty_like(x)
        T._gemm(gab, wst.t().contiguous(), None, dx)                 # dx[r, c] = gab[r, n] . (Wst^T)[c, n]^T
    return dx, dwst, dgamma, dbeta


class _EdgeConvFactored(torch.autograd.Function):
    """The job of _ConvBnLreluMax with idx, without the edge tensors: y[i, j] = s[n(i, j)] - a[i] with [a | b] = x [W1 ; W2]^T and
    s = a + b (include/sapcu_fd_edgeconv.h).  Saved for the backward: x, the stacked weight and ab [P*M, 2 cout]."""

    @staticmethod
    def forward(ctx, x, idx, weight, gamma, beta, eps, running, reps):
        _need_cuda(x, "edgeconv_factored")
        P, M, kk = idx.shape
        _check_patch_shape(M, kk)
        x = x.contiguous()
        rows, C = x.shape
        w = weight.detach().reshape(weight.shape[0], -1)
        cout = w.shape[0]
        if rows != P * M or w.shape[1] != 2 * C:
            raise ValueError("edgeconv_factored: x [%d, %d], idx %s and weight %s do not fit" % (rows, C, tuple(idx.shape), tuple(weight.shape)))
        if C % 32 or cout % 32:
            raise ValueError("edgeconv_factored: channel counts must be multiples of 32 (got %d -> %d)" % (C, cout))
        if rows * kk < 2:
            raise ValueError("BatchNorm in training mode needs more than 1 value per channel (got %d rows)" % (rows * kk))
        wst = torch.cat([w[:, :C], w[:, C:]], dim=0).contiguous()         # W1 and W2 are rounded (bf16 mode) separately
        idx = idx.to(torch.int32).contiguous()
        ga, be = gamma.detach().contiguous(), beta.detach().contiguous()
        ab, mean, var, invstd, out, arg = _edgeconv_factored_forward(x, wst, idx, ga, be, eps)
        _update_running(running, mean, var, rows * kk, int(reps))
        ctx.save_for_backward(x, wst, ga, be, ab, mean, invstd, arg)
        ctx.idx, ctx.wshape = idx, weight.shape
        return out

    @staticmethod
    def backward(ctx, g):
        x, wst, ga, be, ab, mean, invstd, arg = ctx.saved_tensors
        cout = wst.shape[0] // 2
        dx, dwst, dgamma, dbeta = _edgeconv_factored_backward(x, wst, ctx.idx, ga, be, ab, mean, invstd, arg, g.contiguous(),
                                                              ctx.needs_input_grad[0])
        dw = torch.cat([dwst[:cout], dwst[cout:]], dim=1).reshape(ctx.wshape)
        return dx, None, dw, dgamma, dbeta, None, None, None


def edgeconv_factored(x, weight, gamma, beta, idx, eps=1e-5, running=None, reps=1):
    """``conv_bn_lrelu_max(x, weight, gamma, beta, group=kk, idx=idx)`` in factored form: x [P*M, C] (C % 32 == 0), idx int32
    [P, M, kk], weight [c_out, 2C(, 1, 1)] -> [P*M, c_out], with one GEMM on the P*M point rows (it follows train.gemm_precision)
    and gathers over the neighbours instead of any [P*M*kk, .] tensor, forward or backward.  An index outside [0, M) gives that edge
    y = 0 and no gradient and is counted for take_bad_index_count()."""
    return _EdgeConvFactored.apply(x, idx, weight, gamma, beta, eps, running, reps)


def feature_knn(x, P, M, k):
    """The library's free-running neighbour rule on features x [P*M, C]: ``sapcu_patch_knn`` — the k highest scores
    -|x_i - x_j|^2 in descending order, equal scores by ascending index -> int32 [P, M, k]."""
    _need_cuda(x, "feature_knn")
    x = x.contiguous()
    c = x.shape[1]
    idx = torch.empty((P, M, k), dtype=torch.int32, device=x.device)
    _lib.call("sapcu_patch_knn", x.device, x, P, M, c, c, k, idx)
    return idx


def _sub(p, prefix):
    return {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)}


def _tap(taps, key, value):
    if taps is not None:
        taps.setdefault(key, []).append(value.detach())


def fd_train_forward(p, patches, k=20, k_scales=(10, 20, 40), time_steps_enc=5, num_heads=4, eps=1e-5, knn=None, momentum=None,
                     dropout=0.0, generator=None, taps=None, force_spikes=None):
    """``EnhancedSNNDistanceEstimation.forward`` in TRAINING mode: patches [P, M, 3] -> distances [P], differentiable w.r.t. every
    tensor of p (the model's parameters — and, for the running statistics, buffers — under the reference's state_dict names).

    knn: None (free running: sapcu_patch_knn on the spikes, see feature_knn) or integer tables [T, 3, P, M, min(k, M)] for blocks
    1-3 of every step.  The xyz tables of `k_scales` are exact and always computed here, each clamped to min(k_scale, M).
    force_spikes: None or a dict {(t, block): [P*M, C_block] spikes, "fc": [P, emb]} — teacher forcing: forward values come from
    the given spikes, derivatives from this run's own pre-activations.  taps: None or a dict that receives lists of detached
    tensors: "spikes", "preact", "threshold" (blocks 0-3 of step 0, then of step 1, ...; the threshold each step compared with),
    "knn" (per step, [3, P, M, kk]), "pooled" (per step), "integrated", "fc_preact", "enc".
    momentum: when set and p carries the BatchNorm buffers they are updated as train() mode does (0.1 in the reference).
    dropout: the decoder's dropout probability, masks drawn from `generator` on the device.

    The block-0 path (the k_scales EdgeConvs, concatenation, scale_fusion) has the same value at every time step — its input is the
    patch — so it is computed once and feeds T neuron steps; its BatchNorm buffers still receive T momentum updates and
    num_batches_tracked += T, and autograd sums the T steps' gradients into it."""
    _need_cuda(patches, "fd_train_forward")
    P, M, _ = patches.shape
    Tn = int(time_steps_enc)
    for kq in list(k_scales) + [k]:                               # refused before any launch, not inside loss.backward()
        _check_patch_shape(M, min(int(kq), M))
    dev = patches.device
    enc = _sub(p, "encoder.")
    xyz = patches.reshape(P * M, 3).contiguous()

    def bn(prefix, group, x, idx=None, reps=1, src=enc):
        return conv_bn_lrelu_max(x, src[prefix + ".0.weight"], src[prefix + ".1.weight"], src[prefix + ".1.bias"], group=group, idx=idx,
                                 eps=eps, running=T._running(src, prefix + ".1", momentum), reps=reps)

    def neuron(name, x, state, key):
        prm = _sub(enc, name + ".")
        force = None if force_spikes is None else force_spikes.get(key)
        return neuron_step_train(x, prm, state, force)

    scales = []
    for s, ks in enumerate(k_scales):
        kk = min(int(ks), M)
        scales.append(bn("multi_scale_first_conv.%d" % s, kk, xyz, T.inpatch_knn(patches, kk), reps=Tn))
    fused = bn("scale_fusion", 1, torch.cat(scales, dim=1), reps=Tn)                      # [P*M, 64], the same at every step
    kk = min(int(k), M)
    if knn is not None:
        if tuple(knn.shape) != (Tn, 3, P, M, kk):
            raise ValueError("knn must be [%d, 3, %d, %d, %d]" % (Tn, P, M, kk))
        knn = knn.to(device=dev, dtype=torch.int32)
        if int(knn.min()) < 0 or int(knn.max()) >= M:
            raise ValueError("knn holds indices outside [0, %d)" % M)
    factored = _EDGECONV_FORM[0] == "factored"                     # blocks 1-3 only; block 0 (xyz, C = 3) stays on the feature path
    states = [None] * 4
    pooled = []
    for t in range(Tn):
        feats = []
        cur = fused
        tabs = []
        for b in range(4):
            if b > 0:
                idx = knn[t, b - 1] if knn is not None else feature_knn(cur.detach(), P, M, kk)
                tabs.append(idx)
                if factored:
                    pre = "conv_blocks.%d" % (b - 1)
                    cur = edgeconv_factored(cur, enc[pre + ".0.weight"], enc[pre + ".1.weight"], enc[pre + ".1.bias"], idx, eps=eps,
                                            running=T._running(enc, pre + ".1", momentum))
                else:
                    cur = bn("conv_blocks.%d" % (b - 1), kk, cur, idx)
            if taps is not None:
                th_used = states[b][1] if states[b] is not None else enc["snn_blocks.%d.threshold_base" % b].detach().expand_as(cur)
                _tap(taps, "threshold", th_used)
            cur, states[b], pre = neuron("snn_blocks.%d" % b, cur, states[b], (t, b))
            _tap(taps, "spikes", cur)
            _tap(taps, "preact", pre)
            feats.append(cur)
        if taps is not None:
            _tap(taps, "knn", torch.stack(tabs))
        pooled.append(bn("multi_scale_conv", M, torch.cat(feats, dim=1)))                  # [P, emb]: conv + BN + LeakyReLU + max over M
        _tap(taps, "pooled", pooled[-1])
    w = torch.softmax(enc["temporal_integration.weights"], dim=0)
    x = torch.einsum("t,tbf->bf", w, torch.stack(pooled, dim=0))
    _tap(taps, "integrated", x)
    x, _, pre = neuron("snn_fc", x, None, "fc")                                             # one step from the zero state
    _tap(taps, "fc_preact", pre)
    _tap(taps, "enc", x)
    return _decoder_train(_sub(p, "distance_decoder."), x, num_heads, eps, momentum, dropout, generator)


def _decoder_train(dec, x, num_heads, eps, momentum, dropout, generator):
    """StandardDistanceDecoder.forward in train() mode (fd/snn_coder.py:711-725, 751-758, 777-798) on [P, <= 256] tensors."""
    def lin_bn(x, lin, bnm):
        return T.conv_bn_train(T._pad_channels(x), T._pad_channels(dec[lin + ".weight"]), dec[lin + ".bias"], dec[bnm + ".weight"],
                               dec[bnm + ".bias"], eps=eps, running=T._running(dec, bnm, momentum))

    def drop(x):
        return x * T.dropout_keep(x.shape, dropout, x.device, generator) if dropout > 0 else x

    x = F.gelu(lin_bn(x, "fc_in.0", "fc_in.1"))
    i = 0
    while ("residual_blocks.%d.fc.0.weight" % i) in dec:
        pre = "residual_blocks.%d." % i
        h = drop(F.gelu(lin_bn(x, pre + "fc.0", pre + "fc.1")))
        h = lin_bn(h, pre + "fc.4", pre + "fc.5")
        res = T.linear_train(x, dec[pre + "res_proj.weight"], dec[pre + "res_proj.bias"]) if (pre + "res_proj.weight") in dec else x
        x = F.gelu(h + res)
        i += 1
    B, dim = x.shape
    hd = dim // num_heads
    q, kq, v = T.linear_train(x, dec["attention.to_qkv.weight"], dec["attention.to_qkv.bias"]).chunk(3, dim=-1)
    attn = torch.softmax((q.reshape(B, num_heads, hd) * kq.reshape(B, num_heads, hd)).sum(-1) * hd ** -0.5, dim=-1)
    out = (attn.unsqueeze(-1) * v.reshape(B, num_heads, hd)).reshape(B, dim)
    out = drop(T.linear_train(out, dec["attention.to_out.0.weight"], dec["attention.to_out.0.bias"]))
    x = F.layer_norm(out + x, (dim,), dec["attention.norm.weight"], dec["attention.norm.bias"], 1e-5)
    x = drop(F.gelu(lin_bn(x, "fc_hidden.0", "fc_hidden.1")))
    d = T.linear_train(x, dec["fc_distance.weight"], dec["fc_distance.bias"])
    return F.softplus(d, beta=5.0).squeeze(-1)


def distance_loss(pred, gt, reduction="mean", beta=0.1):
    """enhanced_distance_loss (fd/snn_coder.py:800-803): smooth-L1."""
    return F.smooth_l1_loss(pred, gt, reduction=reduction, beta=beta)
