"""fd's training step (sapcu_amd/fd_train.py over csrc/fd_train_ops.hip, fd_edgeconv_ops.hip and the GEMM / weight-gradient /
BatchNorm-backward ops of csrc/train_ops.hip) across patch sizes, batch shapes and hyper-parameter settings.

The single ops are compared with references at a few shapes in tests/test_gpu_fd_train.py / test_gpu_fd_edgeconv.py, and the whole
step with two recorded runs of the reference.  Here the COMPOSITION runs — fd_train.fd_train_forward + distance_loss + backward — at
the inputs tests/fd_train_cases.py holds (chosen on the CPU by tests/golden/make_fd_train_cases.py; its docstring has the families
and the screening rule), against oracle.train_path.fd_train_forward (pinned on the reference's two runs by
tests/test_oracle_golden.py).  The forcing goes the opposite way to the fixture test, so no case depends on where a spike falls.
Per case, in BOTH EdgeConv forms (fd_train.edgeconv_form "feature" and "factored", f32):

  1. the device runs FREE from fresh tensors (momentum 0.1, buffers included); take_bad_index_count() is 0;
  2. its tables of blocks 1-3 equal the library rule (scores -|x_i - x_j|^2 descending, ties by ascending index) recomputed on
     the CPU from the device's own spikes — integer scores, exact; its xyz tables equal the oracle's as sets per row;
  3. the oracle runs in f32 FORCED on the device's tables and spikes; wherever the device's spike differs from the oracle's own
     u > 0: the share of such spikes is <= 0.01 and none has an oracle |u| above 1e-4;
  4. pooled, integrated, prediction and loss <= 2e-4; every gradient within 2e-2 max|ref| + 5e-5 peak; the grad-is-None set equals
     the oracle's, the exactly-zero set too except the biases that cancel in a BatchNorm (finite only); BatchNorm buffers within
     1e-5, num_batches_tracked equal (the block-0 path counts T updates);
  5. a second run from fresh tensors gives the same bits: prediction, loss, every gradient;
  6. the two forms' tables and spikes are equal, or every differing spike is within the 1e-4 margin of item 3.

An UNSCREENED case asserts items 1, 2, 5, shapes and finiteness and prints the rest.

All 58 keys of the table are screened.  Measured on an MI355X over the 116 runs (58 cases, two forms): at most 1 spike differs from
the oracle's (|u| 3.6e-7); pooled at most 3.3e-5 (fd-kfull), integrated 2.0e-5 (fd-T1), prediction 6.7e-5 (M = 100), loss 4.9e-6
(M = 100), gradients 0.045 of their bar (M = 128; typically 0.002 .. 0.02), buffers 2.6e-6 (M = 128); the two forms never differ in a
spike or a table.  One input was moved on the way, by the rule and not by hand: at P = 2, skip 300 the device's buffers were 1.5e-5
off, on a running_var of the decoder's two-row BatchNorm where the oracle's own f32 and f64 runs are 4.1e-6 apart; the screening
rule now holds the buffers to a tenth of their bar and chose skip 321 (device: 6.7e-7; M = 3 and M = 100, which had passed, moved
to their next candidates under the same rule).  The sweep found no defect.

The "P" family's table stops below the weight gradient's cap of 64 row slabs (65 536 edge rows = 456 patches at M = 12: the CPU
oracle of such a step does not fit the time of a test).  test_training_step_above_the_weight_gradient_slab_cap runs the whole step
there without an oracle; test_edgeconv_ops_and_bn_stats_above_the_slab_cap_are_exact_on_dyadic_operands checks the factored ops
and the statistics alone against exact integer sums at that row count.
"""
import os
import sys

import numpy as np
import pytest
import torch

import fd_train_cases as C
import gpu_utils as U

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_fd_train_cases as G  # noqa: E402

VALUE_BAR, GRAD_TOL, GRAD_FLOOR, BUFFER_BAR = 2e-4, 2e-2, 5e-5, 1e-5
FLIP_SHARE, FLIP_MARGIN = 0.01, 1e-4
FORMS = ("feature", "factored")
I32 = torch.int32


def _bits(t):
    return t.contiguous().view(I32)


def _device_step(family, key, pts, gt, form, taps=None):
    """One free-running training step on the device from fresh tensors in `form`: (prediction, loss, {name: gradient or None},
    p with the updated buffers), on the device."""
    from sapcu_amd import fd_train
    kw = G.model_kw(family, key)
    sd, names = G.state_dict(family, key)
    p = {n: sd[n].to(U.dev()).clone().requires_grad_(True) for n in names}
    p.update({n: v.to(U.dev()).clone() for n, v in sd.items() if n not in p})
    with fd_train.edgeconv_form(form):
        pred = fd_train.fd_train_forward(p, pts.to(U.dev()), kw["k"], tuple(kw["k_scales"]), kw["time_steps_enc"], kw["num_heads"],
                                         momentum=0.1, taps=taps)
        loss = fd_train.distance_loss(pred, gt.to(U.dev()))
        loss.backward()
    assert fd_train.take_bad_index_count() == 0
    return pred.detach(), loss.detach(), {n: p[n].grad for n in names}, p


def _check_tables(family, key, pts, taps):
    """Item 2.  -> (knn [T, 3, P, M, kk] int64, the device's xyz tables) on the CPU."""
    from oracle import train_path as TP
    from sapcu_amd import train
    kw = G.model_kw(family, key)
    P, M = G.shape(family, key)
    kk, Tn = min(kw["k"], M), kw["time_steps_enc"]
    knn = torch.stack(taps["knn"]).cpu().long()
    assert tuple(knn.shape) == (Tn, 3, P, M, kk)
    for t in range(Tn):
        for b in range(1, 4):
            want = TP.library_knn(taps["spikes"][4 * t + b - 1].cpu(), P, M, kk)
            assert torch.equal(knn[t, b - 1], want), (family, key, "step %d block %d: not the library's neighbour rule" % (t, b))
    xyz = []
    for ks, ref in zip(kw["k_scales"], G.xyz_tables(family, key, pts)):
        idx = train.inpatch_knn(pts.to(U.dev()), min(int(ks), M)).cpu().long()
        assert tuple(idx.shape) == tuple(ref.shape) and torch.equal(idx.sort(-1)[0], ref.sort(-1)[0]), (family, key, ks)
        xyz.append(idx)
    return knn, xyz


def _device_case(family, key, skip, form):
    """Items 1, 2 and 5, shapes and finiteness: -> (pts, gt, knn, xyz, taps, prediction, loss, gradients, p)."""
    P, M = G.shape(family, key)
    pts, gt = G.inputs(family, key, skip)
    sd, names = G.state_dict(family, key)
    taps = {}
    pred, loss, grads, p = _device_step(family, key, pts, gt, form, taps)
    knn, xyz = _check_tables(family, key, pts, taps)
    pred2, loss2, grads2, _ = _device_step(family, key, pts, gt, form)
    assert tuple(pred.shape) == (P,) and bool(torch.isfinite(pred).all()) and bool(torch.isfinite(loss))
    for n in names:
        assert grads[n] is None or (grads[n].shape == sd[n].shape and bool(torch.isfinite(grads[n]).all())), n
    assert torch.equal(_bits(pred), _bits(pred2)) and torch.equal(loss, loss2), "the second run differs"
    differing = [n for n in names if (grads[n] is None) != (grads2[n] is None) or (grads[n] is not None and not torch.equal(_bits(grads[n]), _bits(grads2[n])))]
    assert not differing, "gradients differ between two runs of the same step: %s" % differing[:8]
    return pts, gt, knn, xyz, taps, pred, loss, grads, p


def _spike_state(taps):
    return torch.cat([s.flatten() for s in taps["spikes"]] + [taps["enc"][0].flatten()]).cpu()


def _check_form(family, key, skip, form, screened):
    P, M = G.shape(family, key)
    kw = G.model_kw(family, key)
    Tn = kw["time_steps_enc"]
    pts, gt, knn, xyz, taps, pred, loss, grads, p = _device_case(family, key, skip, form)
    sd, names = G.state_dict(family, key)
    cancelled = G.cancelled(sd)
    dev_taps = {k: [v.cpu() for v in vs] for k, vs in taps.items() if k in ("spikes", "enc", "knn")}
    _, force = G.forcing(dev_taps, Tn)
    ref_pred, ref_loss, ref_g, ref_taps, ref_p = G.oracle_step(family, key, pts, gt, torch.float32, knn=knn, force=force, knn_xyz=xyz, momentum=0.1)

    # item 3: the device's spikes against the oracle's own u > 0
    u = torch.cat([v.flatten() for v in ref_taps["preact"]] + [ref_taps["fc_preact"][0].flatten()])
    flip = (u > 0).float() != _spike_state(taps)
    share = float(flip.float().mean())
    far = float(u[flip].abs().max()) if bool(flip.any()) else 0.0
    # item 4
    e = {"pooled": float((torch.stack(taps["pooled"]).cpu() - torch.stack(ref_taps["pooled"])).abs().max()),
         "integrated": float((taps["integrated"][0].cpu() - ref_taps["integrated"][0]).abs().max()),
         "prediction": float((pred.cpu() - ref_pred).abs().max()), "loss": abs(float(loss) - float(ref_loss))}
    none_dev, none_ref = {n for n in names if grads[n] is None}, {n for n in names if ref_g[n] is None}
    zero_dev = {n for n in names if grads[n] is not None and not bool(grads[n].any()) and n not in cancelled}
    zero_ref = {n for n in names if ref_g[n] is not None and not bool(ref_g[n].any()) and n not in cancelled}
    compared = [n for n in names if n not in cancelled and ref_g[n] is not None and grads[n] is not None]
    peak = max(float(ref_g[n].abs().max()) for n in compared)
    worst, where = 0.0, ""
    for n in compared:
        r = float((grads[n].cpu() - ref_g[n]).abs().max()) / (GRAD_TOL * float(ref_g[n].abs().max()) + GRAD_FLOOR * peak)
        if not r <= worst:
            worst, where = r, n
    e_buf, where_buf, tracked = 0.0, "", []
    for n in sd:
        if n in names:
            continue
        if n.endswith("num_batches_tracked"):
            tracked.append((n, int(p[n]), int(ref_p[n])))
        else:
            d = float((p[n].cpu() - ref_p[n]).abs().max())
            if not d <= e_buf:
                e_buf, where_buf = d, n
    print("%s %s %s [%d x %d, skip %d]%s: %d of %d spikes differ from the oracle's (largest |u| %.3g, bar %g); pooled %.3g, integrated %.3g, "
          "prediction %.3g, loss %.3g (bar %g); gradients %.3g of their bar at %s (peak %.3g); buffers %.3g (bar %g) at %s"
          % (family, key, form, P, M, skip, "" if screened else " UNSCREENED", int(flip.sum()), flip.numel(), far, FLIP_MARGIN, e["pooled"],
             e["integrated"], e["prediction"], e["loss"], VALUE_BAR, worst, where, peak, e_buf, BUFFER_BAR, where_buf))
    assert int(p["encoder.scale_fusion.1.num_batches_tracked"]) == Tn == int(p["encoder.multi_scale_first_conv.0.1.num_batches_tracked"])
    if screened:
        assert share <= FLIP_SHARE, (family, key, form, share)
        assert far <= FLIP_MARGIN, "a spike away from its threshold differs: an arithmetic defect, not a rounding flip (|u| %g)" % far
        assert max(e.values()) <= VALUE_BAR, (family, key, form, e)
        assert none_dev == none_ref, (none_dev ^ none_ref)
        assert zero_dev == zero_ref, (zero_dev ^ zero_ref)
        assert worst <= 1.0, (family, key, form, where, worst)
        assert e_buf <= BUFFER_BAR, (family, key, form, e_buf)
        assert all(a == b for _, a, b in tracked), [t for t in tracked if t[1] != t[2]]
    return pts, pred, knn, _spike_state(taps), u


def _check_case(family, key):
    skip = C.CASES[family][key][0]
    screened = key not in C.UNSCREENED[family]
    runs = {form: _check_form(family, key, skip, form, screened) for form in FORMS}
    # item 6: the two forms against each other
    (_, _, knn_a, sp_a, u_a), (_, _, knn_b, sp_b, u_b) = runs["feature"], runs["factored"]
    diff = sp_a != sp_b
    if bool(diff.any()) or not torch.equal(knn_a, knn_b):
        margin = float(torch.minimum(u_a.abs(), u_b.abs())[diff].max()) if bool(diff.any()) else 0.0
        print("%s %s: the forms differ in %d spikes, largest |u| among them %.3g" % (family, key, int(diff.sum()), margin))
        assert bool(diff.any()), "the forms' tables differ while their spikes agree"
        assert margin <= FLIP_MARGIN, (family, key, margin)
    return runs["feature"][0], runs["feature"][1]


@pytest.mark.gpu
@pytest.mark.parametrize("m", sorted(C.CASES["M"]))
def test_training_step_at_patch_size(m):
    """P = 4 (3 from M = 100): through the clamps min(k, M) at 10, 20 and 40, P M through 16, 64 and 256 rows, the edge rows
    through 1024, up to the largest patch sapcu_patch_knn takes."""
    _check_case("M", m)


@pytest.mark.gpu
@pytest.mark.parametrize("p", sorted(C.CASES["P"]))
def test_training_step_at_batch_size(p):
    """M = 12: the point rows 12 P and the edge rows 144 P one below and one above the row boundaries of the kernels
    (make_fd_train_cases.P_SIZES has the derivation)."""
    _check_case("P", p)


@pytest.mark.gpu
@pytest.mark.parametrize("rid", list(C.CASES["hp"]))
def test_training_step_at_hyper_parameter_setting(rid):
    """One case per fd row of the hyper-parameter matrix (the trainable class accepts every row inference accepts:
    tests/test_fd_train_cases_host.py); then the module itself in train() mode with dropout 0 must return the bits of the direct
    fd_train_forward call with the row's settings — the constructor's arguments reach the ops."""
    import sapcu_amd
    pts, pred = _check_case("hp", rid)
    model = sapcu_amd.TrainableSNNDistanceEstimation(**G.model_kw("hp", rid))
    model.load_state_dict(G.state_dict("hp", rid)[0], strict=True)
    assert model.dropout == 0.0
    model = model.to(U.dev()).train()
    out = model(pts.to(U.dev())).detach()
    assert tuple(out.shape) == tuple(pred.shape) and torch.equal(_bits(out), _bits(pred)), rid


# ---- above the weight gradient's slab cap ----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_training_step_above_the_weight_gradient_slab_cap():
    """M = 12, P = SLAB_CAP_P = 456: 65 664 edge rows in every EdgeConv, so the feature form's weight gradients run with more than 64
    slabs' worth of [P M kk, 2C] rows (wgrad_slabs' cap: the slabs grow), through fd_train.py's own workspace sizing and autograd.
    No oracle (make_fd_train_cases.py, at SLAB_CAP_P): the tables by the library rule, shapes, finiteness, two runs bit for bit, and
    no weight gradient all zero."""
    assert G.SLAB_CAP_P * G.P_M * G.P_M > G.P_SLAB_CAP >= (G.SLAB_CAP_P - 1) * G.P_M * G.P_M and G.SLAB_CAP_P not in C.CASES["P"]
    pts, gt, knn, xyz, taps, pred, loss, grads, p = _device_case("P", G.SLAB_CAP_P, G.SLAB_CAP_SKIP, "feature")
    assert tuple(knn.shape) == (G.BASE_KW["time_steps_enc"], 3, G.SLAB_CAP_P, G.P_M, G.P_M)
    dead = [n for n, g in grads.items() if n.endswith(".weight") and (g is None or not bool(g.any()))]
    assert not dead, dead
    print("P %d [%d x %d, skip %d]: loss %.6f, prediction %.3g .. %.3g, largest gradient entry %.3g"
          % (G.SLAB_CAP_P, G.SLAB_CAP_P, G.P_M, G.SLAB_CAP_SKIP, float(loss), float(pred.min()), float(pred.max()),
             max(float(g.abs().max()) for g in grads.values() if g is not None)))


@pytest.mark.gpu
def test_edgeconv_ops_and_bn_stats_above_the_slab_cap_are_exact_on_dyadic_operands():
    """sapcu_fd_edgeconv_stats / _max_forward / _backward and sapcu_fd_bn_stats at P = 456, M = 12, kk = 12 (65 664 edge rows).
    Operands are small integers chosen so that every sum is an exact integer in f32 and in f64 and the statistics are dyadic:

      ab = [a | b] integers in -2..2, s = a + b; the edge value y[i, j] = s[n(i, j)] - a[i] is an integer in -6..6.  The sum of y and
      of y^2 over the 65 664 edges are integers below 2^24, so the mean and the variance must EQUAL the f64 values rounded to f32 once
      (mean = sum / rows, var = sumsq / rows - mean^2 evaluated in f64).

    With gamma = 1, beta = 0 and the statistics passed in as mean = 0, invstd = 1 (powers of two) the forward's BatchNorm is the
    identity: out must EQUAL max_j LeakyReLU(y) (0.2 y rounds once, the same on both sides) and arg the FIRST such j.  The backward
    runs on the measured statistics (the same arg-max: BatchNorm with a positive scale is monotone) and is compared on its exact
    part: grad_beta, the f64 column sums of the routed gradient (g or 0.2f g), must EQUAL those sums formed on the host.
    sapcu_fd_bn_stats on the [rows, C] integer matrix y itself gives the same mean, variance and invstd."""
    from sapcu_amd import _lib
    lib = _lib.load()
    P, M, kk, cout = G.SLAB_CAP_P, G.P_M, G.P_M, 64
    rows = P * M * kk
    assert rows > G.P_SLAB_CAP
    rng = np.random.default_rng(rows)
    ab = rng.integers(-2, 3, (P * M, 2 * cout)).astype(np.float32)
    idx = rng.integers(0, M, (P, M, kk)).astype(np.int32)
    a, s = ab[:, :cout].astype(np.int64), (ab[:, :cout] + ab[:, cout:]).astype(np.int64)
    nbr = (idx.astype(np.int64) + (np.arange(P) * M)[:, None, None]).reshape(P * M, kk)
    y = s[nbr] - a[:, None, :]                                                       # [P M, kk, cout] integers
    total, totsq = y.sum((0, 1)), (y * y).sum((0, 1))
    assert int(np.abs(total).max()) < 2 ** 24 and int(totsq.max()) < 2 ** 24
    mean64 = total / float(rows)
    var64 = totsq / float(rows) - mean64 ** 2
    dev = U.dev()
    ab_d, idx_d = torch.from_numpy(ab).to(dev), torch.from_numpy(idx).to(dev)
    mean, var, invstd = (torch.full((cout,), float("nan"), device=dev) for _ in range(3))
    need = int(lib.sapcu_fd_edgeconv_stats_workspace_bytes(P, M, kk, cout))
    ws = torch.empty((max(need, 0),), dtype=torch.uint8, device=dev)
    st = _lib.current_stream()
    _lib.check(lib.sapcu_fd_edgeconv_stats(_lib.ptr(ab_d), _lib.ptr(idx_d), P, M, kk, cout, 1e-5, _lib.ptr(mean), _lib.ptr(var), _lib.ptr(invstd),
                                           None, _lib.ptr(ws), need, st))
    eps = float(np.float32(1e-5))
    assert np.array_equal(mean.cpu().numpy(), mean64.astype(np.float32)), "edgeconv_stats: mean"
    assert np.array_equal(var.cpu().numpy(), var64.astype(np.float32)), "edgeconv_stats: variance"
    np.testing.assert_allclose(invstd.cpu().numpy().astype(np.float64), 1 / np.sqrt(var64 + eps), rtol=2.0 ** -23, atol=0)   # one f32 ulp

    yd = torch.from_numpy(y.reshape(rows, cout).astype(np.float32)).to(dev)
    mean2, var2, invstd2 = (torch.full((cout,), float("nan"), device=dev) for _ in range(3))
    need2 = int(lib.sapcu_fd_bn_stats_workspace_bytes(rows, cout))
    ws2 = torch.empty((need2,), dtype=torch.uint8, device=dev)
    _lib.check(lib.sapcu_fd_bn_stats(_lib.ptr(yd), rows, cout, 1e-5, _lib.ptr(mean2), _lib.ptr(var2), _lib.ptr(invstd2), _lib.ptr(ws2), need2, st))
    assert np.array_equal(mean2.cpu().numpy(), mean64.astype(np.float32)), "bn_stats: mean"
    assert np.array_equal(var2.cpu().numpy(), var64.astype(np.float32)), "bn_stats: variance"
    assert torch.equal(invstd2, invstd), "bn_stats and edgeconv_stats: invstd"

    zero, one = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
    out = torch.full((P * M, cout), float("nan"), device=dev)
    arg = torch.full((P * M, cout), -1, dtype=I32, device=dev)
    _lib.check(lib.sapcu_fd_edgeconv_max_forward(_lib.ptr(ab_d), _lib.ptr(idx_d), P, M, kk, cout, _lib.ptr(zero), _lib.ptr(one), _lib.ptr(one),
                                                 _lib.ptr(zero), _lib.ptr(out), _lib.ptr(arg), st))
    yf = y.astype(np.float32)
    act = np.where(yf >= 0, yf, np.float32(0.2) * yf)
    want = act.max(1)
    first = (act == want[:, None, :]).argmax(1)                                      # numpy: the first True
    assert np.array_equal(out.cpu().numpy(), want), "edgeconv_max_forward: values"
    assert np.array_equal(arg.cpu().numpy().astype(np.int64), first), "edgeconv_max_forward: not the first of equal maxima"
    assert int(((act == want[:, None, :]).sum(1) > 1).sum()) > 0                     # ties did occur

    g = rng.integers(-3, 4, (P * M, cout)).astype(np.float32)
    g_d = torch.from_numpy(g).to(dev)
    gab = torch.full((P * M, 2 * cout), float("nan"), device=dev)
    dgamma, dbeta = (torch.full((cout,), float("nan"), device=dev) for _ in range(2))
    bad = torch.full((1,), -1, dtype=I32, device=dev)
    need3 = int(lib.sapcu_fd_edgeconv_backward_workspace_bytes(P, M, kk, cout))
    ws3 = torch.empty((max(need3, 0),), dtype=torch.uint8, device=dev)
    _lib.check(lib.sapcu_fd_edgeconv_backward(_lib.ptr(ab_d), _lib.ptr(idx_d), _lib.ptr(g_d), _lib.ptr(arg), P, M, kk, cout, _lib.ptr(mean),
                                              _lib.ptr(invstd), _lib.ptr(one), _lib.ptr(zero), _lib.ptr(gab), _lib.ptr(dgamma), _lib.ptr(dbeta),
                                              _lib.ptr(bad), _lib.ptr(ws3), need3, st))
    torch.cuda.synchronize()
    assert int(bad) == 0 and bool(torch.isfinite(gab).all()) and bool(torch.isfinite(dgamma).all())
    # the gradient routed to the arg-max edge: g where z = (y - mean) invstd > 0, else g * 0.2f (one f32 rounding); the sign of z is
    # that of y - mean, exact in f32.  The column sums run in f64 over <= 5472 f32 values: exact in any order.
    sel = np.take_along_axis(y, first[:, None, :], 1)[:, 0, :].astype(np.float64) - mean.cpu().numpy().astype(np.float64)
    routed = np.where(sel > 0, g, g * np.float32(0.2)).astype(np.float32)
    assert np.array_equal(dbeta.cpu().numpy(), routed.astype(np.float64).sum(0).astype(np.float32)), "edgeconv_backward: grad_beta"


# ---- the limits -----------------------------------------------------------------------------------------------------------------

def _small_params():
    sd, names = G.state_dict("P", 2)
    p = {n: sd[n].to(U.dev()).clone().requires_grad_(True) for n in names}
    p.update({n: v.to(U.dev()).clone() for n, v in sd.items() if n not in p})
    return p, names


@pytest.mark.gpu
def test_patches_beyond_128_points_are_refused_by_the_neighbour_search():
    """M = 129 without knn=: sapcu_patch_knn refuses it (SAPCU_ERR_ARG) in the forward, before any gradient tensor is touched."""
    from sapcu_amd import _lib, fd_train
    p, names = _small_params()
    kw = G.BASE_KW
    pts = torch.from_numpy(np.random.default_rng(1).normal(size=(3, 129, 3)).astype(np.float32) * 0.05).to(U.dev())
    with pytest.raises(_lib.SapcuError) as e:
        fd_train.fd_train_forward(p, pts, kw["k"], tuple(kw["k_scales"]), kw["time_steps_enc"], kw["num_heads"])
    assert e.value.args[0] == -1 and "patch_knn" in e.value.args[1]
    assert all(p[n].grad is None for n in names)


@pytest.mark.gpu
def test_single_patch_batch_is_refused_like_batchnorm_refuses_it():
    """P = 1 through the module in train() mode: the decoder's BatchNorm has one value per channel — ValueError, as torch's
    BatchNorm gives in the reference."""
    import sapcu_amd
    model = sapcu_amd.TrainableSNNDistanceEstimation(**G.BASE_KW)
    model.load_state_dict(G.state_dict("P", 2)[0], strict=True)
    model = model.to(U.dev()).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        model(U.sphere_patches(1, 12).to(U.dev()))
    assert all(q.grad is None for q in model.parameters())


def test_time_steps_beyond_the_constructors_range_are_refused_on_the_host():
    """fd's training ops run one neuron step per call, so the encoder's step count has no bound of their own (fn's T-step loop
    kernel takes 1..8): the bound is the constructor's, 1..64, a ValueError before any tensor exists."""
    import sapcu_amd
    for steps in (0, 65):
        with pytest.raises(ValueError, match="time_steps_enc"):
            sapcu_amd.TrainableSNNDistanceEstimation(**dict(G.BASE_KW, time_steps_enc=steps))
    assert sapcu_amd.TrainableSNNDistanceEstimation(**dict(G.BASE_KW, time_steps_enc=64)).time_steps_enc == 64


@pytest.mark.gpu
def test_nine_encoder_time_steps_train():
    """time_steps_enc = 9, one more than fn's training ops take: fd trains, the block-0 path counts 9 BatchNorm updates."""
    import sapcu_amd
    from sapcu_amd import fd_train
    kw = dict(G.BASE_KW, time_steps_enc=9)
    torch.manual_seed(0)
    model = sapcu_amd.TrainableSNNDistanceEstimation(**kw).to(U.dev()).train()
    pred = model(U.sphere_patches(3, 12).to(U.dev()))
    loss, _ = model.compute_loss(pred, torch.full((3,), 0.2, device=U.dev()))
    loss.backward()
    assert fd_train.take_bad_index_count() == 0
    assert tuple(pred.shape) == (3,) and bool(torch.isfinite(pred).all())
    assert int(model.encoder.scale_fusion[1].num_batches_tracked) == 9 and int(model.encoder.conv_blocks[0][1].num_batches_tracked) == 9
    assert tuple(model.encoder.temporal_integration.weights.grad.shape) == (9,)
