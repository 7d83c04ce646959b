"""CPU ORACLE (test infrastructure, NOT product code) — training mode: fn's neuron loop and whole step
and, below them, fd's single-step neurons, EdgeConv blocks and whole step (row f-5, ``fd_train_forward``).

torch restatement of /root/reference/fn/snn_coder.py:87-151 with ``self.training`` (hard spikes forward, soft-surrogate
derivative backward through autograd's straight-through construction, constant gate mask), driven as at :318-320.
Gradients come from torch autograd on this restatement.  Only ``tests/`` may import it.  Pinned by
tests/golden/neuron_train.npz (the reference's own module in train mode, forward and backward).
"""
import math

import torch


def _expand(p, x):
    return p.view([1, -1] + [1] * (x.dim() - 2)).expand_as(x)


def spike_train(u, grad_width=10.0):
    uc = torch.clamp(u, -10.0, 10.0)
    soft = 0.5 * torch.exp(-(uc ** 2) / 2) / math.sqrt(2 * math.pi) + 0.5 * torch.sigmoid(grad_width * uc)
    hard = (u > 0).float()
    return soft + (hard - soft).detach()


def lif_selfloop_train(x, membrane_decay, threshold_adapt, refractory_decay, threshold_base, steps=4):
    decay = _expand(torch.clamp(membrane_decay, 0.1, 0.99), x)
    adapt = _expand(torch.clamp(threshold_adapt, 0.001, 0.1), x)
    rdecay = _expand(torch.clamp(refractory_decay, 0.1, 0.95), x)
    theta0 = _expand(threshold_base, x)
    m, th, r = torch.zeros_like(x), theta0, torch.zeros_like(x)
    for _ in range(steps):
        x = x * (r <= 0).float()
        m = m * decay * (1 - r) + x
        sp = spike_train(m - th)
        m = m * (1 - sp)
        r = r * rdecay + sp
        th = th + adapt * sp
        th = theta0 + (th - theta0) * 0.95
        x = sp
    return x


def conv_bn_lif_train(x, weight, bias, gamma, beta, membrane_decay, threshold_adapt, refractory_decay, threshold_base,
                      steps=4, eps=1e-5):
    """fn/snn_coder.py:225-229 + 317-320 in training mode on channels-last rows: x [rows, c_in] -> spikes [rows, c_out]."""
    y = x @ weight.reshape(weight.shape[0], -1).t() + bias
    mean = y.mean(0)
    var = y.var(0, unbiased=False)
    z = (y - mean) / torch.sqrt(var + eps) * gamma + beta
    return lif_selfloop_train(z, membrane_decay, threshold_adapt, refractory_decay, threshold_base, steps)


def softmax_agg(a, pe, v, idx, m, sqrt_hd):
    """fn/snn_coder.py:379-389 on edge rows (the stage oracle/snn_path.py:158-159 evaluates channels-first): a, pe
    [P*k, d], v [P, d], idx [P*k] in-patch neighbour indices, m points per patch -> [P, d]."""
    pts, d = v.shape
    kk = a.shape[0] // pts
    nbr = (torch.arange(pts).div(m, rounding_mode="floor") * m).repeat_interleave(kk) + idx.long()
    w = torch.softmax(a.view(pts, kk, d) / sqrt_hd, dim=1)
    u = v[nbr].view(pts, kk, d) + pe.view(pts, kk, d)
    return (w * u).sum(1)


def conv_bn_train(x, weight, bias, gamma, beta, eps=1e-5):
    y = x @ weight.reshape(weight.shape[0], -1).t() + bias
    return (y - y.mean(0)) / torch.sqrt(y.var(0, unbiased=False) + eps) * gamma + beta


def transformer_block_train(p, xyz, features, knn_idx, time_steps=4, num_heads=8, eps=1e-5):
    """MultiHeadSNNTransformerBlock.forward in training mode (fn/snn_coder.py:294-396, dropout 0), restated on
    channels-last rows with plain torch ops; p = the block's parameters under the reference's names."""
    B, N, _ = xyz.shape
    k = knn_idx.shape[-1]
    P = B * N
    nbr = (knn_idx.long() + (torch.arange(B) * N).view(B, 1, 1)).reshape(P * k)
    ptr = torch.arange(P).repeat_interleave(k)
    feat, xyzr = features.reshape(P, -1), xyz.reshape(P, 3)

    def layer(x, conv, bn, snn=None):
        z = conv_bn_train(x, p[conv + ".weight"], p[conv + ".bias"], p[bn + ".weight"], p[bn + ".bias"], eps)
        if snn is None:
            return z
        return lif_selfloop_train(z, p[snn + ".membrane_decay"], p[snn + ".threshold_adapt"], p[snn + ".refractory_decay"],
                                  p[snn + ".threshold_base"], time_steps)

    x = layer(feat, "fc1.0", "fc1.1", "snn1")
    q, kf, v = (layer(x, "w_%ss.0" % c, "w_%ss.1" % c, "snn_" + c) for c in "qkv")
    pe = layer(xyzr[ptr] - xyzr[nbr], "fc_delta.0", "fc_delta.1", "snn_delta")
    pe = layer(pe, "fc_delta2.0", "fc_delta2.1", "snn_delta2")
    a = layer(q[ptr] - kf[nbr] + pe, "fc_gamma.0", "fc_gamma.1", "snn_gamma")
    a = layer(a, "fc_gamma2.0", "fc_gamma2.1")
    d_model = a.shape[1]
    res = softmax_agg(a, pe, v, knn_idx.reshape(P * k), N, float((d_model // num_heads) ** 0.5))
    res = layer(res, "out_proj.0", "out_proj.1")
    return (layer(res, "fc2.0", "fc2.1") + feat).view(B, N, -1)


def fn_train_forward(p, points, knn, time_steps_enc=4, num_heads=8, eps=1e-5):
    """ImprovedSNNNormalEstimation.forward in training mode, dropout off (fn/snn_coder.py:430-476, 542-549), restated with
    plain torch ops on channels-last rows; knn = the three blocks' in-patch neighbour tables [B, N, k]."""
    import torch.nn.functional as F
    B, N, _ = points.shape
    P = B * N

    def sub(prefix):
        return {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)}

    def lif(z, e, name):
        return lif_selfloop_train(z, e[name + ".membrane_decay"], e[name + ".threshold_adapt"], e[name + ".refractory_decay"],
                                  e[name + ".threshold_base"], time_steps_enc)

    enc = sub("encoder.")
    cur = lif(conv_bn_train(points.reshape(P, 3), enc["conv1.0.weight"], enc["conv1.0.bias"], enc["conv1.1.weight"], enc["conv1.1.bias"], eps),
              enc, "snn_init").view(B, N, 64)
    feats = []
    for i in range(3):
        cur = transformer_block_train(sub("encoder.trans%d." % (i + 1)), points, cur, knn[i], 4, num_heads, eps)
        feats.append(cur)
    g = lif(conv_bn_train(torch.cat(feats, 2).reshape(P, 192), enc["conv_final.0.weight"], enc["conv_final.0.bias"],
                          enc["conv_final.1.weight"], enc["conv_final.1.bias"], eps), enc, "snn_final")
    x = g.view(B, N, -1).max(dim=1)[0] @ enc["fc_out.weight"].t() + enc["fc_out.bias"]
    dec = sub("decoder.")
    for li in sorted({int(k.split(".")[1]) for k in dec if k.startswith("mlp.") and k.endswith(".weight") and dec[k].dim() == 2}):
        x = F.gelu(conv_bn_train(x, dec["mlp.%d.weight" % li], dec["mlp.%d.bias" % li], dec["mlp.%d.weight" % (li + 1)],
                                 dec["mlp.%d.bias" % (li + 1)], eps))
    x = x @ dec["fc_out.weight"].t() + dec["fc_out.bias"]
    return F.normalize(F.layer_norm(x, (3,), dec["norm_out.weight"], dec["norm_out.bias"], 1e-5), dim=1)


def angular_loss(pred, gt, temperature=0.1, alpha=0.1):
    """enhanced_angular_loss_with_consistency without the consistency term (fn/snn_coder.py:603-612): for [B, 3] predictions
    that term compares each normal with copies of itself — its value is 0.15 * mean(1 - 1) and its gradient is zero."""
    cos = torch.nn.functional.cosine_similarity(pred, gt, dim=1)
    err = torch.acos(torch.clamp(cos, -1 + 1e-6, 1 - 1e-6))
    conf = torch.sigmoid(err.detach() / temperature)
    return (err * conf + alpha * (conf - 0.5) ** 2).mean()


def angular_loss_with_consistency(pred, gt, xyz, temperature=0.1, alpha=0.1, consistency_weight=0.15, k_neighbors=8):
    """enhanced_angular_loss_with_consistency with its consistency term (fn/snn_coder.py:557-625): pred/gt [B, N, 3] or [B, 3],
    xyz [B, N, 3] -> (loss, mean confidence)."""
    F = torch.nn.functional
    base = angular_loss(pred.reshape(-1, 3), gt.reshape(-1, 3), temperature, alpha)
    cos = F.cosine_similarity(pred.reshape(-1, 3), gt.reshape(-1, 3), dim=1)
    conf = torch.sigmoid(torch.acos(torch.clamp(cos, -1 + 1e-6, 1 - 1e-6)).detach() / temperature).mean()
    B, N, _ = xyz.shape
    d = ((xyz[:, :, None, :] - xyz[:, None, :, :]) ** 2).sum(-1)
    nbr = d.argsort()[:, :, 1:k_neighbors + 1]
    full = pred.unsqueeze(1).expand(B, N, 3) if pred.dim() == 2 else pred.view(B, N, 3)
    nb = torch.gather(full.unsqueeze(1).expand(B, N, N, 3), 2, nbr.unsqueeze(-1).expand(B, N, nbr.shape[2], 3))
    return base + consistency_weight * (1 - F.cosine_similarity(full.unsqueeze(2), nb, dim=-1)).mean(), conf


# ------------------------------------------------------------------------------------------------ fd (row f-5)
# EnhancedSNNDistanceEstimation.forward in train() mode (fd/snn_coder.py:392-492, 711-725) and its loss (:800-803), restated on
# channels-last rows.  f32 or f64 by the dtype of the inputs; every gradient is autograd's.  Pinned by tests/golden/fd_train.npz and
# fd_train_b.npz (tests/test_oracle_golden.py).

def neuron_step_train(x, raw, state=None, force=None):
    """One step of MultiTimeConstantLIFNeuron / ...EIFNeuron (EIF when raw has ``delta_T``) in train() mode on x [rows, C]
    (fd/snn_coder.py:117-155, 223-275): hard spike forward, soft-surrogate derivative backward.  state: None (zero membrane and
    refractory, threshold_base) or the carried (membrane, threshold, refractory); what is returned for the next step is detached, as
    the encoder detaches it (:438-442).  force: None or {0, 1} spikes that replace this step's own ``u > 0`` in every forward value,
    the derivative staying that of this run's u.  -> spikes, (membrane, threshold, refractory), u = membrane - threshold."""
    md, ta, rd = raw["membrane_decay"].clamp(0.1, 0.99), raw["threshold_adapt"].clamp(0.001, 0.1), raw["refractory_decay"].clamp(0.1, 0.95)
    tb = raw["threshold_base"]
    m0, th0, r0 = state if state is not None else (torch.zeros_like(x), tb.expand_as(x), torch.zeros_like(x))
    mm = m0 * md * (1 - r0) + x * (r0 <= 0).to(x.dtype)
    if "delta_T" in raw:
        dT, rh = raw["delta_T"].clamp(0.1, 5.0), raw["theta_rh"].clamp(0.1, 2.0)
        mm = mm + dT * torch.exp(((m0 - rh) / (dT + 1e-6)).clamp(-5.0, 5.0))
    u = mm - th0
    uc = u.clamp(-10.0, 10.0)
    soft = 0.5 * torch.exp(-(uc ** 2) / 2) / math.sqrt(2 * math.pi) + 0.5 * torch.sigmoid(10.0 * uc)
    hard = (u > 0).to(x.dtype) if force is None else force.to(x.dtype)
    sp = soft + (hard - soft).detach()
    m1 = mm * (1 - sp)
    r1 = r0 * rd + sp
    th1 = tb + ((th0 + ta * sp) - tb) * 0.95
    return sp, (m1.detach(), th1.detach(), r1.detach()), u.detach()


def first_max(act, dim):
    """max over `dim` whose gradient goes to the FIRST position of the maximum (what torch's CPU max(dim) does and what the
    library's arg-max does: with {0, 1} spikes equal maxima are the rule, not the exception)."""
    n = act.shape[dim]
    val = act.max(dim)[0]
    pos = torch.arange(n).view([n if d == dim else 1 for d in range(act.dim())])
    first = torch.where(act == val.unsqueeze(dim), pos, n).min(dim)[0]
    return torch.gather(act, dim, first.unsqueeze(dim)).squeeze(dim)


def edge_feature(x, idx):
    """get_graph_feature (fd/snn_coder.py:52-68) on rows: x [P*M, C], idx [P, M, kk] in-patch -> [P*M*kk, 2C] = [x_n - x_i | x_n]."""
    P, M, kk = idx.shape
    nbr = (idx.long() + (torch.arange(P) * M).view(P, 1, 1)).reshape(-1)
    nb = x[nbr]
    return torch.cat([nb - x[torch.arange(P * M).repeat_interleave(kk)], nb], dim=1)


def _bn_running(p, bn, mean, var, rows, momentum, reps):
    if momentum is None or (bn + ".running_mean") not in p:
        return
    with torch.no_grad():
        for _ in range(reps):
            p[bn + ".running_mean"].mul_(1 - momentum).add_(mean.detach(), alpha=momentum)
            p[bn + ".running_var"].mul_(1 - momentum).add_(var.detach() * (rows / (rows - 1.0)), alpha=momentum)
        if (bn + ".num_batches_tracked") in p:
            p[bn + ".num_batches_tracked"].add_(reps)


def batchnorm_train(y, p, bn, eps=1e-5, momentum=None, reps=1):
    """nn.BatchNorm in train() mode on rows y [rows, C] with p[bn + ".weight" / ".bias"]; the buffers of p, when present and
    momentum is set, move as train() moves them, `reps` times."""
    rows = y.shape[0]
    if rows < 2:
        raise ValueError("BatchNorm in training mode needs more than 1 value per channel (got %d rows)" % rows)
    mean, var = y.mean(0), y.var(0, unbiased=False)
    _bn_running(p, bn, mean, var, rows, momentum, reps)
    return (y - mean) / torch.sqrt(var + eps) * p[bn + ".weight"] + p[bn + ".bias"]


def conv_bn_lrelu_max_train(a, p, prefix, group=1, eps=1e-5, momentum=None, reps=1):
    """Conv (1x1, no bias) `prefix.0` -> BatchNorm `prefix.1` on batch statistics -> LeakyReLU(0.2) -> max over each `group`
    consecutive rows: a [rows, c_in] -> [rows / group, c_out]."""
    w = p[prefix + ".0.weight"]
    act = torch.nn.functional.leaky_relu(batchnorm_train(a @ w.reshape(w.shape[0], -1).t(), p, prefix + ".1", eps, momentum, reps), 0.2)
    return act if group == 1 else first_max(act.view(a.shape[0] // group, group, -1), 1)


def library_knn(x, P, M, k):
    """The library's neighbour rule on rows x [P*M, C]: scores -|x_i - x_j|^2 descending, equal scores by ascending index (a
    stable sort) -> int64 [P, M, k].  On {0, 1} spikes the scores are integers below 2^24: the table is the same in any precision."""
    f = x.detach().view(P, M, -1)
    n = (f * f).sum(-1)
    score = -(n.unsqueeze(2) + n.unsqueeze(1) - 2 * (f @ f.transpose(1, 2)))
    return torch.sort(score, dim=-1, descending=True, stable=True)[1][..., :k]


def xyz_knn(patches, k):
    """The xyz tables of `k_scales`: the reference's scores (oracle/snn_path.inpatch_knn_scores) and topk -> int64 [P, M, k]."""
    from . import snn_path
    return snn_path.inpatch_knn_scores(patches.detach().transpose(1, 2)).topk(k=k, dim=-1)[1]


def _sub(p, prefix):
    return {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)}


def _tap(taps, key, value):
    if taps is not None:
        taps.setdefault(key, []).append(value.detach())


def fd_decoder_train(dec, x, num_heads=4, eps=1e-5, momentum=None):
    """StandardDistanceDecoder.forward in train() mode, dropout 0 (fd/snn_coder.py:711-725, 751-758, 777-798): x [P, emb] -> [P]."""
    F = torch.nn.functional

    def lin(x, name):
        return x @ dec[name + ".weight"].t() + dec[name + ".bias"]

    def lin_bn(x, l, b):
        return batchnorm_train(lin(x, l), dec, b, eps, momentum)

    x = F.gelu(lin_bn(x, "fc_in.0", "fc_in.1"))
    i = 0
    while ("residual_blocks.%d.fc.0.weight" % i) in dec:
        pre = "residual_blocks.%d." % i
        h = lin_bn(F.gelu(lin_bn(x, pre + "fc.0", pre + "fc.1")), pre + "fc.4", pre + "fc.5")
        x = F.gelu(h + (lin(x, pre + "res_proj") if (pre + "res_proj.weight") in dec else x))
        i += 1
    B, dim = x.shape
    hd = dim // num_heads
    q, k, v = lin(x, "attention.to_qkv").chunk(3, dim=-1)
    attn = torch.softmax((q.reshape(B, num_heads, hd) * k.reshape(B, num_heads, hd)).sum(-1) * hd ** -0.5, dim=-1)
    out = lin((attn.unsqueeze(-1) * v.reshape(B, num_heads, hd)).reshape(B, dim), "attention.to_out.0")
    x = F.layer_norm(out + x, (dim,), dec["attention.norm.weight"], dec["attention.norm.bias"], 1e-5)
    x = F.gelu(lin_bn(x, "fc_hidden.0", "fc_hidden.1"))
    return F.softplus(lin(x, "fc_distance"), beta=5.0).squeeze(-1)


def fd_train_forward(p, patches, k=20, k_scales=(10, 20, 40), time_steps_enc=5, num_heads=4, eps=1e-5, knn=None, momentum=None,
                     taps=None, force_spikes=None, knn_xyz=None):
    """EnhancedSNNDistanceEstimation.forward in train() mode, dropout 0, with the arguments and taps of
    sapcu_amd.fd_train.fd_train_forward: p = parameters (and, for the running statistics, buffers) under the reference's names,
    patches [P, M, 3] -> distances [P].  knn: None (free running under the library's rule, library_knn) or tables
    [T, 3, P, M, min(k, M)] for blocks 1-3; knn_xyz: None (xyz_knn) or one table [P, M, min(k_scale, M)] per entry of k_scales;
    force_spikes: None or {(t, block): [P*M, C] spikes, "fc": [P, emb]}.  The block-0 path has the same value at every step: it is
    evaluated once, its BatchNorm buffers move T times."""
    P, M, _ = patches.shape
    Tn = int(time_steps_enc)
    enc = _sub(p, "encoder.")
    xyz = patches.reshape(P * M, 3)

    def neuron(name, x, state, key):
        return neuron_step_train(x, _sub(enc, name + "."), state, None if force_spikes is None else force_spikes.get(key))

    scales = []
    for s, ks in enumerate(k_scales):
        kk = min(int(ks), M)
        idx = knn_xyz[s] if knn_xyz is not None else xyz_knn(patches, kk)
        scales.append(conv_bn_lrelu_max_train(edge_feature(xyz, idx), enc, "multi_scale_first_conv.%d" % s, kk, eps, momentum, Tn))
    fused = conv_bn_lrelu_max_train(torch.cat(scales, dim=1), enc, "scale_fusion", 1, eps, momentum, Tn)
    kk = min(int(k), M)
    if knn is not None and tuple(knn.shape) != (Tn, 3, P, M, kk):
        raise ValueError("knn must be [%d, 3, %d, %d, %d]" % (Tn, P, M, kk))
    states = [None] * 4
    pooled = []
    for t in range(Tn):
        feats, tabs = [], []
        cur = fused
        for b in range(4):
            if b > 0:
                idx = knn[t, b - 1].long() if knn is not None else library_knn(cur, P, M, kk)
                tabs.append(idx)
                cur = conv_bn_lrelu_max_train(edge_feature(cur, idx), enc, "conv_blocks.%d" % (b - 1), kk, eps, momentum)
            if taps is not None:
                _tap(taps, "threshold", states[b][1] if states[b] is not None else enc["snn_blocks.%d.threshold_base" % b].expand_as(cur))
            cur, states[b], pre = neuron("snn_blocks.%d" % b, cur, states[b], (t, b))
            _tap(taps, "spikes", cur)
            _tap(taps, "preact", pre)
            feats.append(cur)
        if taps is not None:
            _tap(taps, "knn", torch.stack(tabs))
        pooled.append(conv_bn_lrelu_max_train(torch.cat(feats, dim=1), enc, "multi_scale_conv", M, eps, momentum))
        _tap(taps, "pooled", pooled[-1])
    w = torch.softmax(enc["temporal_integration.weights"], dim=0)
    x = torch.einsum("t,tbf->bf", w, torch.stack(pooled, dim=0))
    _tap(taps, "integrated", x)
    x, _, pre = neuron("snn_fc", x, None, "fc")
    _tap(taps, "fc_preact", pre)
    _tap(taps, "enc", x)
    return fd_decoder_train(_sub(p, "distance_decoder."), x, num_heads, eps, momentum)


def distance_loss(pred, gt, reduction="mean", beta=0.1):
    """enhanced_distance_loss (fd/snn_coder.py:800-803): smooth-L1."""
    return torch.nn.functional.smooth_l1_loss(pred, gt, reduction=reduction, beta=beta)
