"""Where a screened case of tests/fn_train_cases.py misses a bar on the device: is it a spike on its threshold?  (Needs a GPU.)

    python tests/fn_train_flips.py FAMILY KEY [SKIP]        # e.g.  M 127 303   — the figures of make_fn_train_cases.MOVED

The method of test_training_hard_spike_flips_sit_on_their_thresholds (tests/test_gpu_parity.py), over EVERY conv + BatchNorm
(+ neuron) layer of the case's training forward, the oracle run on the device's kNN tables:

  forced   the device layer on the ORACLE's input against the oracle's output: differing output spikes and their float64 margin
           min over the neuron steps of |m_t - theta_t|; for a layer without neuron the largest difference;
  free     the device's own forward, layer by layer against the oracle's: where a flipped spike spreads;
  inner    the neuron loop forward AND backward (upstream gradient 1) on each side's own BatchNorm output of the free run: the
           elements whose input gradient differs, and their margin over ALL steps.  oracle.train_path.lif_selfloop_train returns
           the last step's spike only; an inner step's spike steers the membrane, the refractory gate and the surrogate's path, so
           it can flip and leave the output spike — the forward — as it was while the gradient through that element changes.

A miss is a spike flip when every differing element of the forced comparison, and every differing element of the FIRST layer at
which the free run departs (later layers see changed inputs), has a margin below 1e-4; a differing element away from its threshold
there, or a miss with no differing element in any of the three, is an arithmetic defect.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MARGIN = 1e-4


def margins(z, md, ta, rd, tb, steps):
    """float64 min over the `steps` neuron steps of |m_t - theta_t| per element of z (fn/snn_coder.py:125-151)."""
    z = z.double()
    decay, adapt, rdecay, th0 = md.double().clamp(0.1, 0.99), ta.double().clamp(0.001, 0.1), rd.double().clamp(0.1, 0.95), tb.double()
    m, th, r, inp = torch.zeros_like(z), th0.expand_as(z).clone(), torch.zeros_like(z), z
    out = torch.full_like(z, float("inf"))
    for _ in range(steps):
        inp = inp * (r <= 0).double()
        m = m * decay * (1 - r) + inp
        out = torch.minimum(out, (m - th).abs())
        sp = (m - th > 0).double()
        m = m * (1 - sp)
        r = r * rdecay + sp
        th = th0 + ((th + adapt * sp) - th0) * 0.95
        inp = sp
    return out


def oracle_layers(family, key, pts, knn):
    """The oracle's f32 forward with every conv + BatchNorm call recorded in order: [{x, w, b, gamma, beta, z, lif}], lif = None or
    (md, ta, rd, tb, steps, spikes); and the normals."""
    import make_fn_train_cases as G
    from oracle import train_path as TP
    kw = G.model_kw(family, key)
    sd, names = G.state_dict(family, key)
    calls = []
    orig_cb, orig_lif = TP.conv_bn_train, TP.lif_selfloop_train

    def cb(x, w, b, gamma, beta, eps=1e-5):
        z = orig_cb(x, w, b, gamma, beta, eps)
        calls.append(dict(x=x, w=w, b=b, gamma=gamma, beta=beta, z=z, lif=None))
        return z

    def lif(z, md, ta, rd, tb, steps=4):
        out = orig_lif(z, md, ta, rd, tb, steps)
        if calls and calls[-1]["z"] is z:
            calls[-1]["lif"] = (md, ta, rd, tb, steps, out)
        return out

    TP.conv_bn_train, TP.lif_selfloop_train = cb, lif
    try:
        with torch.no_grad():
            normals = TP.fn_train_forward({n: sd[n] for n in names}, pts, knn, kw["time_steps_enc"], kw["num_heads"])
    finally:
        TP.conv_bn_train, TP.lif_selfloop_train = orig_cb, orig_lif
    by_id = {id(v): n for n, v in sd.items()}
    for c in calls:
        c["name"] = by_id.get(id(c["w"]), "?")
    return calls, normals


def device_layers(family, key, pts, knn):
    """The device's free forward with every conv + BatchNorm(+ neuron) layer's output recorded in order, the padded inputs of the
    neuron layers too: (outputs, {index: (x, w, bias, gamma, beta)}, normals)."""
    import gpu_utils as U
    import make_fn_train_cases as G
    from sapcu_amd import train as TR
    kw = G.model_kw(family, key)
    sd, names = G.state_dict(family, key)
    outs, ins = [], {}
    o1, o2 = TR.conv_bn_lif_train, TR.conv_bn_train

    def with_neuron(*a, **k):
        ins[len(outs)] = a[:5]
        outs.append(o1(*a, **k))
        return outs[-1]

    def without(*a, **k):
        outs.append(o2(*a, **k))
        return outs[-1]

    TR.conv_bn_lif_train, TR.conv_bn_train = with_neuron, without
    try:
        with torch.no_grad():
            normals = TR.fn_train_forward({n: sd[n].to(U.dev()) for n in names}, pts.to(U.dev()), tuple(kw["k_values"]), kw["time_steps_enc"],
                                          kw["num_heads"], knn=[t.to(torch.int32).to(U.dev()) for t in knn])
    finally:
        TR.conv_bn_lif_train, TR.conv_bn_train = o1, o2
    return outs, ins, normals


def report(family, key, skip=None, out=print):
    """Print the three comparisons for the case at candidate `skip` (default: the one in the table); returns (differing elements
    up to and including the first layer whose free output departs plus the forced ones after it, the largest margin among them)."""
    import fn_train_cases as C
    import gpu_utils as U
    import make_fn_train_cases as G
    from oracle import train_path as TP
    from sapcu_amd import train as TR
    skip = C.CASES[family][key][0] if skip is None else skip
    pts, _ = G.inputs(family, key, skip)
    kw = G.model_kw(family, key)
    knn = [TR.inpatch_knn(pts.to(U.dev()), min(k, pts.shape[1])).cpu().long() for k in kw["k_values"]]
    calls, ref_n = oracle_layers(family, key, pts, knn)
    free, free_in, dev_n = device_layers(family, key, pts, knn)
    assert len(free) == len(calls)
    out("%s %s skip %d: normals max |device - oracle| %.3g, %d layers" % (family, key, skip, float((dev_n.cpu() - ref_n).abs().max()), len(calls)))
    d = lambda t: t.to(U.dev())
    differing, worst, spread = 0, 0.0, False
    for i, c in enumerate(calls):
        W = c["w"].reshape(c["w"].shape[0], -1)
        ref = c["lif"][5] if c["lif"] is not None else c["z"]
        got_free = free[i].cpu()[:, :ref.shape[1]]
        with torch.no_grad():
            if c["lif"] is None:
                got = TR.conv_bn_train(TR._pad_channels(d(c["x"])), TR._pad_channels(d(W)), d(c["b"]), d(c["gamma"]), d(c["beta"])).cpu()
                out("%2d %-34s rows %7d  no neuron: max |device - oracle| forced %.3g, free %.3g (oracle max %.3g)"
                    % (i, c["name"], ref.shape[0], float((got - ref).abs().max()), float((got_free - ref).abs().max()), float(ref.abs().max())))
                continue
            md, ta, rd, tb, steps, _ = c["lif"]
            got = TR.conv_bn_lif_train(TR._pad_channels(d(c["x"])), TR._pad_channels(d(W)), d(c["b"]), d(c["gamma"]), d(c["beta"]), d(md), d(ta),
                                       d(rd), d(tb), steps=steps).cpu()
            zdev = TR.conv_bn_train(*free_in[i])[:, :ref.shape[1]].contiguous()
        margin = margins(c["z"], md, ta, rd, tb, steps)
        flip = got != ref
        zo = c["z"].detach().clone().requires_grad_(True)
        TP.lif_selfloop_train(zo, md, ta, rd, tb, steps).sum().backward()
        zd = zdev.clone().requires_grad_(True)
        TR.lif_selfloop_train(zd, d(md), d(ta), d(rd), d(tb), steps).sum().backward()
        bad = (zd.grad.cpu() - zo.grad).abs() > 1e-3 * (1.0 + zo.grad.abs())
        n_free = int((got_free != ref).sum())
        if flip.any() or bad.any() or n_free:
            both = flip if spread else (flip | bad)        # after a flipped OUTPUT spike the free run's inputs differ downstream
            spread = spread or n_free > 0
            differing += int(both.sum())
            worst = max(worst, float(margin[both].max()) if both.any() else 0.0)
            out("%2d %-34s rows %7d  forced: %d of %d output spikes differ (margin max %.3g); free: %d output spikes differ; inner: %d input "
                "gradients differ (by at most %.3g, margin over all steps max %.3g)"
                % (i, c["name"], ref.shape[0], int(flip.sum()), flip.numel(), float(margin[flip].max()) if flip.any() else 0.0, n_free,
                   int(bad.sum()), float((zd.grad.cpu() - zo.grad).abs()[bad].max()) if bad.any() else 0.0,
                   float(margin[bad].max()) if bad.any() else 0.0))
    out("elements that differ on the oracle's input or in the neuron loops' backward: %d, their largest margin %.3g (%s)"
        % (differing, worst, "spike flips" if differing and worst < MARGIN else "NOT explained by spikes on their thresholds"))
    return differing, worst


if __name__ == "__main__":
    fam, k = sys.argv[1], sys.argv[2]
    report(fam, k if fam == "hp" else int(k), int(sys.argv[3]) if len(sys.argv) > 3 else None)
