"""CPU suite, part 1: the oracle (our restatement) against golden vectors produced by the real
reference (tests/golden/make_fixtures.py).  This is what pins the oracle."""
import numpy as np
import pytest
import torch

from conftest import FD_KW, FN_KW, golden
import gpu_utils as U
from oracle import geom_path as G
from oracle import snn_path as O

FN_HP = {"k_values": FN_KW["k_values"], "emb_dims": 640, "time_steps_enc": 4, "num_heads": 8}
FD_HP = {"k": 32, "k_scales": FD_KW["k_scales"], "emb_dims": 768, "time_steps_enc": 4, "num_heads": 8}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_neuron_unit_lif_eif():
    g = golden("neuron_unit.npz")
    x, raw = t(g["x"]), g["raw_params"]
    names = ["membrane_decay", "threshold_adapt", "refractory_decay", "threshold_base", "delta_T", "theta_rh"]
    for kind, n in (("lif", 4), ("eif", 6)):
        sd = {"n." + names[i]: t(raw[i]) for i in range(n)}
        p = O.neuron_params(sd, "n")
        for T in (1, 4, 7):
            v, st = x, None
            for _ in range(T):
                v, st = O.neuron_step(v, st, p)
            for key, val in (("spikes", v), ("membrane", st[0]), ("threshold", st[1]), ("refractory", st[2])):
                ref = g["%s_T%d_%s" % (kind, T, key)]
                np.testing.assert_allclose(val.numpy(), ref, rtol=0, atol=1e-7, err_msg="%s T=%d %s" % (kind, T, key))


def test_neuron_far_outside_the_spike_clamp():
    """neuron_wide.npz: the reference's fd neurons out to |x| = 1e4, driven fd's way (same input every step, the gate decides).
    The oracle reproduces every step's spikes and the final state; the reference's gate is closed for t >= 1 on ALL of these
    inputs — its clamped spike surrogate bottoms out at 3.85e-23 > 0, so r > 0 (the invariant the HIP kernels' dead-stage
    elimination and gate counter rest on)."""
    g = golden("neuron_wide.npz")
    x, raw = t(g["x"]), g["raw_params"]
    names = ["membrane_decay", "threshold_adapt", "refractory_decay", "threshold_base", "delta_T", "theta_rh"]
    assert float(np.abs(g["x"]).max()) == 1e4 and int(g["lif_gate_open"]) == 0 and int(g["eif_gate_open"]) == 0
    for kind, n in (("lif", 4), ("eif", 6)):
        sd = {"n." + names[i]: t(raw[i]) for i in range(n)}
        p = O.neuron_params(sd, "n")
        st = None
        for step in range(g[kind + "_spikes"].shape[0]):
            if step:
                assert bool((st[2] > 0).all())
            v, st = O.neuron_step(x, st, p)
            np.testing.assert_allclose(v.numpy(), g[kind + "_spikes"][step], rtol=1e-6, atol=1e-7, err_msg="%s step %d" % (kind, step))
        for key, val in (("membrane", st[0]), ("threshold", st[1]), ("refractory", st[2])):
            np.testing.assert_allclose(val.numpy(), g["%s_%s" % (kind, key)], rtol=1e-6, atol=1e-7, err_msg=kind + " " + key)
        assert g[kind + "_spikes"].min() >= 3.8e-23 and g[kind + "_refractory"].min() > 0


def test_closed_gate_identity():
    """eval-mode spikes are > 0, so the input gate is closed for t >= 1."""
    g = golden("neuron_unit.npz")
    assert g["lif_T1_spikes"].min() > 0 and g["eif_T1_spikes"].min() > 0
    assert g["lif_T1_refractory"].min() > 0


def test_inpatch_knn_indices_exact():
    g = golden("patch_knn.npz")
    for c in (3, 64, 128, 256):
        f = t(g["feat_c%d" % c])
        for k in (8, 12, 16, 18, 24, 32, 48):
            idx = O.inpatch_knn(f, k).numpy()
            assert np.array_equal(idx, g["idx_c%d_k%d" % (c, k)].astype(np.int64)), (c, k)
        # the score matrix the reference itself ranked (captured inside its knn() call): same formula, same torch ops
        sc = O.inpatch_knn_scores(f).numpy()
        ref = g["score_c%d" % c]
        assert sc.shape == ref.shape and np.abs(sc - ref).max() <= 16 * np.spacing(np.float32(np.abs(ref).max())), c


def test_fn_stage_taps(weights):
    g = golden("fn_taps.npz")
    sd = weights("fn")
    taps = {}
    with torch.no_grad():
        n = O.fn_forward(sd, t(g["patch"]), FN_HP, taps=taps)
    pairs = [("stem", taps["encoder.snn_init"]), ("block1", taps["encoder.trans1"]), ("block2", taps["encoder.trans2"]),
             ("block3", taps["encoder.trans3"]), ("enc", taps["encoder.out"]), ("logits", taps["decoder.logits"]),
             ("normals", n)]
    for name, val in pairs:
        np.testing.assert_allclose(val.numpy(), g[name], rtol=0, atol=1e-6, err_msg=name)
    for i in range(3):
        assert np.array_equal(taps["knn_idx"][i].numpy(), g["knn%d" % i].astype(np.int64))
    # the conditioned weights make the net input-sensitive: outputs differ across patches
    assert g["normals"].std(axis=0).max() > 1e-2


def test_fn_stale_cache_pair(weights):
    g = golden("fn_cache_pair.npz")
    sd = weights("fn")
    with torch.no_grad():
        ta = {}
        na = O.fn_forward(sd, t(g["patch_a"]), FN_HP, taps=ta)
        nb_stale = O.fn_forward(sd, t(g["patch_b"]), FN_HP, knn_idx=ta["knn_idx"])
        nb_fresh = O.fn_forward(sd, t(g["patch_b"]), FN_HP)
    np.testing.assert_allclose(na.numpy(), g["normals_a"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(nb_stale.numpy(), g["normals_b_stale"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(nb_fresh.numpy(), g["normals_b_fresh"], rtol=0, atol=1e-6)
    assert np.abs(g["normals_b_stale"] - g["normals_b_fresh"]).max() > 1e-4   # the quirk is observable


def test_fd_stage_taps(weights):
    g = golden("fd_taps.npz")
    sd = weights("fd")
    taps = {}
    with torch.no_grad():
        d = O.fd_forward(sd, t(g["patch"]), FD_HP, taps=taps)
    np.testing.assert_allclose(taps["encoder.fused0"].numpy().transpose(0, 2, 1), g["fused0"], rtol=0, atol=1e-6)
    for tag, tt in (("spikes_t0", 0), ("spikes_tlast", 3)):
        cat = torch.cat([taps["encoder.spk%d.t%d" % (i, tt)] for i in range(4)], 1).numpy().transpose(0, 2, 1)
        np.testing.assert_allclose(cat, g[tag], rtol=0, atol=1e-6, err_msg=tag)
    for i in (1, 2, 3):
        assert np.array_equal(taps["encoder.knn%d" % i].numpy(), g["knn%d" % i].astype(np.int64))
    np.testing.assert_allclose(taps["encoder.pooled_t"].numpy(), g["pooled"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(taps["encoder.out"].numpy(), g["enc"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(d.numpy(), g["dist"], rtol=0, atol=1e-6)
    assert g["dist"].std() > 1e-2


def test_fd_dead_stages_are_dead(weights):
    """The t >= 1 EdgeConv stages feed only gated (zeroed) inputs: the spikes at t = T-1 depend on the t = 0
    pre-activations alone.  Evolving the t = 0 state with zero input reproduces the oracle's last-step spikes."""
    g = golden("fd_taps.npz")
    sd = weights("fd")
    taps = {}
    with torch.no_grad():
        O.fd_forward(sd, t(g["patch"]), FD_HP, taps=taps)
        for bi in range(4):
            p = O.neuron_params(sd, "encoder.snn_blocks.%d" % bi)
            # recover the t=0 pre-activation is not needed: replay from the oracle's own t=0 input tap for block 0
        p0 = O.neuron_params(sd, "encoder.snn_blocks.0")
        x0 = taps["encoder.fused0"]
        s, st = O.neuron_step(x0, None, p0)
        for _ in range(3):
            s, st = O.neuron_step(torch.zeros_like(x0), st, p0)
    assert torch.equal(s, taps["encoder.spk0.t3"])


def test_shape_and_T_variants(weights):
    g = golden("variants.npz")
    with torch.no_grad():
        for M in (12, 100):
            p = t(g["patch_M%d" % M])
            np.testing.assert_allclose(O.fn_forward(weights("fn"), p, FN_HP).numpy(), g["normals_M%d" % M], rtol=0, atol=1e-6)
            np.testing.assert_allclose(O.fd_forward(weights("fd"), p, FD_HP).numpy(), g["dist_M%d" % M], rtol=0, atol=1e-6)
        p = t(g["patch_T"])
        for Tv in (6, 7):
            np.testing.assert_allclose(O.fn_forward(weights("fn", time_steps_enc=Tv), p, dict(FN_HP, time_steps_enc=Tv)).numpy(),
                                       g["normals_T%d" % Tv], rtol=0, atol=1e-6)
            np.testing.assert_allclose(O.fd_forward(weights("fd", time_steps_enc=Tv), p, dict(FD_HP, time_steps_enc=Tv)).numpy(),
                                       g["dist_T%d" % Tv], rtol=0, atol=1e-6)


@pytest.mark.parametrize("rid", [str(r) for r in golden("hparams.npz")["rows"]])
def test_hyper_parameter_rows(rid):
    """hparams.npz: the reference at every hyper-parameter setting of the matrix in make_fixtures.py (constructor defaults, head counts,
    neighbour counts, scale lists, widths, T = 1), 3 patches per patch size.  The oracle reproduces the normals / distances at the
    tolerance of variants.npz, picks the reference's xyz neighbour sets (fn) and, under the reference's own feature-space
    neighbours, its distances (fd).  Well conditioned: f32 and f64 evaluations of the oracle agree to 3e-5.  Not vacuous: outputs differ between the patches, and each of fd's four blocks fires on a
    fraction of its elements strictly between 0 and 1."""
    g = golden("hparams.npz")
    row = U.hparam_row(g, rid)
    _, sd = U.hparam_model(row)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    for m in row["sizes"]:
        p = t(g["%s/m%d:patch" % (rid, m)])
        assert p.shape == (3, m, 3)
        taps = {}
        with torch.no_grad():
            if row["kind"] == "fn":
                ref = g["%s/m%d:normals" % (rid, m)]
                out = O.fn_forward(sd, p, row["hp"], taps=taps)
                out64 = O.fn_forward(sd64, p.double(), row["hp"])
                for i in range(3):
                    want = g["%s/m%d:knn%d" % (rid, m, i)].astype(np.int64)
                    assert want.shape == (3, m, min(row["hp"]["k_values"][i], m))
                    assert np.array_equal(np.sort(taps["knn_idx"][i].numpy(), -1), want), (m, i)
                assert ref.std(axis=0).max() > 1e-2, m
            else:
                ref = g["%s/m%d:dist" % (rid, m)]
                force = [t(g["%s/m%d:knn%d" % (rid, m, i)].astype(np.int64)) for i in (1, 2, 3)]
                assert all(f.shape == (3, m, min(row["hp"]["k"], m)) for f in force)
                out = O.fd_forward(sd, p, row["hp"], taps=taps, force_idx=force)
                out64 = O.fd_forward(sd64, p.double(), row["hp"], force_idx=force)
                assert ref.std() > 1e-2, m
                for bi in range(4):
                    fire = float((taps["encoder.spk%d.t0" % bi] > 0.5).float().mean())
                    assert 0.0 < fire < 1.0, (m, bi, fire)
        np.testing.assert_allclose(out.numpy(), ref, rtol=0, atol=1e-6, err_msg="%s m=%d" % (rid, m))
        # well conditioned: the same arithmetic in f64 lands within a third of the GPU tests' 1e-4, so that bar can be asked of an f32
        # implementation that sums in another order (BatchNorm statistics calibrated on a handful of patches fail this by 100x)
        assert float((out64 - out.double()).abs().max()) <= 3e-5, (m, float((out64 - out.double()).abs().max()))


def test_outer_knn_matches_kdtree_bit_exact():
    from sapcu_amd import testing as T
    g = golden("outer_knn.npz")
    idx = G.knn_bruteforce(T.sphere_cloud(5000, 0), T.grid_queries(4096, 0), 48)
    assert np.array_equal(idx, g["idx_n5000_k48"].astype(np.int64))
    idx2 = G.knn_bruteforce(T.sphere_cloud(2048, 0), T.grid_queries(256, 3), 100)
    assert np.array_equal(idx2, g["idx_n2048_k100"].astype(np.int64))


def test_rotation_matrices_and_quirks():
    g = golden("rotation.npz")
    for n, m in zip(g["normals"], g["matrices"]):
        assert np.array_equal(G.rotation_to_x(n), m)
    assert np.array_equal(G.rotation_to_x(np.array([-1, 0, 0], np.float32)), np.eye(3))   # antiparallel -> identity


def test_batch_split_equals_array_split():
    for n in (1, 63, 64, 65, 901, 4096, 385123):
        for bs in (64, 256, 400):
            ref = np.array_split(np.arange(n), max(1, n // bs))
            assert [(int(c[0]), int(c[-1]) + 1) for c in ref] == G.split_batches(n, bs)


def test_end_to_end_upsample_against_reference_run(weights):
    """Generator3D6.upsample of the real reference (sphere N=2048, 901 seeds, batch 64 -> two batch
    shapes, so the stale-cache path is exercised) vs the oracle's two hot loops + outlier filter."""
    from sapcu_amd import testing as T
    g = golden("e2e_upsample.npz")
    sdn, sdd = weights("fn"), weights("fd")
    seeds = g["seeds"]
    assert len({e - s for s, e in G.split_batches(seeds.shape[0], 64)}) == 2

    def fn_fwd(patch, pre):
        taps = {}
        with torch.no_grad():
            n = O.fn_forward(sdn, patch, FN_HP, knn_idx=pre, taps=taps)
        return n, taps["knn_idx"]

    def fd_fwd(patch):
        with torch.no_grad():
            return O.fd_forward(sdd, patch, FD_HP)

    torch.set_num_threads(8)
    refined, _, _, _ = G.upsample_core(T.sphere_cloud(2048, 0), seeds, fn_fwd, fd_fwd, 48, 64, "reference")
    np.testing.assert_allclose(refined, g["unfiltered"], rtol=0, atol=1e-6)
    keep = G.outlier_filter(g["unfiltered"], 1.5)
    assert np.array_equal(g["unfiltered"][keep], g["filtered"])


def test_fps_and_normalisation_against_reference_run():
    """generate.py:43-74 — the restatement reproduces the reference's own sampled indices (ties included)."""
    from oracle import fps_path as F
    from sapcu_amd import testing as T
    g = golden("fps.npz")
    for name in g["names"]:
        if name == "big400k":
            continue                                   # 400 k x 512 numpy steps: GPU-suite case
        cloud, npoint = T.fps_case(str(name))
        assert npoint == int(g[name + "_npoint"])
        np.testing.assert_array_equal(F.farthest_point_sample(cloud, npoint), g[name + "_idx"], err_msg=str(name))
    c, loc, scale = F.normalize_pointcloud(g["norm_in"])
    np.testing.assert_array_equal(c, g["norm_cloud"])
    np.testing.assert_array_equal(loc, g["norm_loc"])
    assert scale == float(g["norm_scale"])
    c, loc, scale = F.normalize_pointcloud(g["flat_in"])
    np.testing.assert_array_equal(c, g["flat_cloud"])
    assert scale == 0.0 == float(g["flat_scale"])


def test_training_mode_neuron_loop_against_reference_run():
    """Row f-4, first piece: the oracle's training-mode neuron loop (hard spikes, surrogate gradient) reproduces the
    reference module's forward AND its autograd gradients (input + four raw parameters, clamp masks included)."""
    from oracle import train_path as TP
    g = golden("neuron_train.npz")
    for tag in g["tags"]:
        tag = str(tag)
        x = t(g[tag + "_x"]).requires_grad_(True)
        raw = [t(g[tag + "_raw"][i]).requires_grad_(True) for i in range(4)]
        out = TP.lif_selfloop_train(x, *raw, steps=int(g[tag + "_T"]))
        np.testing.assert_array_equal(out.detach().numpy(), g[tag + "_spikes"], err_msg=tag)
        (out * t(g[tag + "_g"])).sum().backward()
        np.testing.assert_allclose(x.grad.numpy(), g[tag + "_gx"], rtol=1e-5, atol=1e-7, err_msg=tag)
        for p, key in zip(raw, ("_gmd", "_gta", "_grd", "_gtb")):
            got = p.grad.numpy() if p.grad is not None else np.zeros_like(g[tag + key])
            np.testing.assert_allclose(got, g[tag + key], rtol=1e-5, atol=1e-6, err_msg=tag + key)


def test_training_layer_conv_bn_neuron_against_reference_run():
    """Row f-4: the oracle's layer restatement (1x1 conv + BatchNorm batch statistics + neuron loop, channels-last rows)
    reproduces the reference modules in train mode: spikes exact, all ten gradients."""
    from oracle import train_path as TP
    g = golden("neuron_train.npz")
    B, cin, N = g["layer_x"].shape
    cout = g["layer_w"].shape[0]
    x = t(g["layer_x"]).permute(0, 2, 1).reshape(B * N, cin).clone().requires_grad_(True)
    prm = [t(g[k]).clone().requires_grad_(True) for k in ("layer_w", "layer_b", "layer_gamma", "layer_beta")]
    raw = [t(g["layer_raw"][i]).clone().requires_grad_(True) for i in range(4)]
    out = TP.conv_bn_lif_train(x, *prm, *raw, steps=4)
    want = t(g["layer_spikes"]).permute(0, 2, 1).reshape(B * N, cout)
    assert (out.detach() != want).float().mean() <= 1e-4          # a pre-activation within 1e-6 of the threshold may flip
    (out * t(g["layer_g"]).permute(0, 2, 1).reshape(B * N, cout)).sum().backward()
    if torch.equal(out.detach(), want):
        gx = t(g["layer_gx"]).permute(0, 2, 1).reshape(B * N, cin)
        np.testing.assert_allclose(x.grad.numpy(), gx.numpy(), rtol=1e-3, atol=2e-5)
        for p, key in zip(prm, ("layer_gw", "layer_gb", "layer_ggamma", "layer_gbeta")):
            np.testing.assert_allclose(p.grad.numpy(), g[key].reshape(p.shape), rtol=1e-3, atol=5e-4, err_msg=key)
        for i, p in enumerate(raw):
            np.testing.assert_allclose(p.grad.numpy(), g["layer_graw"][i], rtol=1e-3, atol=5e-4)


def _block_params(g, device=None):
    p = {}
    for n in g["names"]:
        tt = t(g["p:" + str(n)]).clone()
        if device is not None:
            tt = tt.to(device)
        p[str(n)] = tt.requires_grad_(True)
    return p


def test_training_transformer_block_against_reference_run():
    """Row f-4: one whole MultiHeadSNNTransformerBlock in training mode — the oracle's rows-layout restatement against the
    reference block's forward and autograd gradients (input features + all 60 parameter tensors)."""
    from oracle import train_path as TP
    g = golden("block_train.npz")
    p = _block_params(g)
    feats = t(g["features"]).clone().requires_grad_(True)
    out = TP.transformer_block_train(p, t(g["xyz"]), feats, t(g["knn_idx"]))
    np.testing.assert_allclose(out.detach().numpy(), g["out"], rtol=0, atol=2e-4)
    (out * t(g["g"])).sum().backward()
    ref = t(g["g_features"])
    assert float((feats.grad - ref).norm() / ref.norm()) <= 1e-3
    # the gradients reach 1e4 (surrogate slope 10 through seven neuron layers); convolution biases in front of a BatchNorm
    # have a mathematically zero gradient that comes out as cancellation noise: noise floor relative to the largest gradient
    floor = 2e-5 * max(float(np.abs(g["g:" + str(n)]).max()) for n in g["names"])
    for n in g["names"]:
        n = str(n)
        ref = t(g["g:" + n])
        got = p[n].grad if p[n].grad is not None else torch.zeros_like(ref)
        scale = float(ref.abs().max())
        assert float((got - ref).abs().max()) <= 2e-3 * scale + floor, (n, float((got - ref).abs().max()), scale, floor)


def _fn_train_params(g, device="cpu"):
    import sapcu_amd
    from sapcu_amd import testing as T
    shell = sapcu_amd.ImprovedSNNNormalEstimation(k_values=[24, 18, 12], emb_dims=640, time_steps_enc=4, time_steps_dec=12, num_heads=8,
                                                  use_snn_decoder=False, decoder_dropout=0.1)
    sd = T.training_state_dict(shell.state_dict(), int(g["seed"]))
    names = [str(n) for n in g["names"]]
    return {n: sd[n].to(device).clone().requires_grad_(True) for n in names}, names


def check_fn_train_grads(g, p, names, tol, floor_rel):
    """Compare p[n].grad with the fixture: full tensors, or the stored sample + L2 norm of the large ones."""
    peak = max(float(np.abs(g[("g:" if ("g:" + n) in g else "gs:") + n]).max()) for n in names)
    floor = floor_rel * peak
    worst = 0.0
    for n in names:
        got = p[n].grad.detach().cpu().numpy().ravel() if p[n].grad is not None else np.zeros(p[n].numel(), np.float32)
        if ("g:" + n) in g:
            ref = g["g:" + n].ravel()
        else:
            ref = g["gs:" + n]
            norm = float(np.linalg.norm(got.astype(np.float64)))
            assert abs(norm - float(g["gn:" + n])) <= tol * float(g["gn:" + n]) + floor, (n, norm, float(g["gn:" + n]))
            got = got[g["gi:" + n]]
        scale = float(np.abs(ref).max())
        err = float(np.abs(got - ref).max())
        worst = max(worst, err / (scale + floor))
        assert err <= tol * scale + floor, (n, err, scale, floor)
    return worst


def test_fn_training_step_matches_reference():
    """Row f-4: one training step of the WHOLE fn model (train() mode, dropout off) — the oracle's restatement against the
    reference's normals, loss and parameter gradients (tests/golden/fn_train.npz)."""
    from oracle import train_path as TP
    g = golden("fn_train.npz")
    p, names = _fn_train_params(g)
    knn = [t(g["knn%d" % i]) for i in range(3)]
    normals = TP.fn_train_forward(p, t(g["points"]), knn)
    np.testing.assert_allclose(normals.detach().numpy(), g["normals"], rtol=0, atol=2e-4)
    loss = TP.angular_loss(normals, t(g["gt"]))
    assert abs(float(loss.detach()) - float(g["loss"])) <= 2e-4
    loss.backward()
    check_fn_train_grads(g, p, names, 1e-2, 2e-5)


def check_fn_trainer_updates(g, new, old, names, tol, floor_rel):
    """Parameter updates (new - old) against the fixture's: full tensors, or the stored sample + L2 norm."""
    peak = max(float(np.abs(g[("d:" if ("d:" + n) in g else "ds:") + n]).max()) for n in names)
    floor = floor_rel * peak
    for n in names:
        got = (new[n].detach().cpu().double() - old[n].detach().cpu().double()).numpy().ravel()
        if ("d:" + n) in g:
            ref = g["d:" + n].ravel()
        else:
            ref = g["ds:" + n]
            assert abs(float(np.linalg.norm(got)) - float(g["dn:" + n])) <= tol * float(g["dn:" + n]) + floor, n
            got = got[g["di:" + n]]
        # f32 parameters: an update far below the parameter's own ulp is rounded away on both sides
        ulp = float(np.abs(old[n].detach().cpu().numpy()).max()) * 1.2e-7
        assert float(np.abs(got - ref).max()) <= tol * float(np.abs(ref).max()) + floor + ulp, (n, float(np.abs(got - ref).max()))


def test_fn_trainer_step_matches_reference():
    """Row f-4: the reference Trainer's train_step (4-D batch, consistency loss, global-norm clipping, SGD) restated with the
    oracle's forward: loss, confidence and every parameter update (tests/golden/fn_trainer.npz)."""
    import sapcu_amd
    from sapcu_amd import testing as T
    from oracle import train_path as TP
    g = golden("fn_trainer.npz")
    shell = sapcu_amd.ImprovedSNNNormalEstimation(k_values=[24, 18, 12], emb_dims=640, time_steps_enc=4, time_steps_dec=12, num_heads=8,
                                                  use_snn_decoder=False, decoder_dropout=0.1)
    sd = T.training_state_dict(shell.state_dict(), int(g["seed"]))
    names = [str(n) for n in g["names"]]
    p = {n: sd[n].clone().requires_grad_(True) for n in names}
    pts = t(g["points"])
    B, NP, M, _ = pts.shape
    flat = pts.reshape(B * NP, M, 3)
    d = ((flat[:, :, None, :] - flat[:, None, :, :]) ** 2).sum(-1)
    knn = [d.topk(min(k, M), dim=-1, largest=False)[1] for k in (24, 18, 12)]
    pred = torch.nn.functional.normalize(TP.fn_train_forward(p, flat, knn).view(B, NP, 3), dim=-1)
    gt = torch.nn.functional.normalize(t(g["gt"]), dim=-1)
    loss, conf = TP.angular_loss_with_consistency(pred, gt, pts.mean(dim=2))
    assert abs(float(loss.detach()) - float(g["loss"])) <= 2e-4 and abs(float(conf) - float(g["confidence"])) <= 2e-4
    loss.backward()
    grads = [p[n].grad if p[n].grad is not None else torch.zeros_like(p[n]) for n in names]
    total = torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads))
    coef = min(1.0, float(g["grad_clip"]) / (float(total) + 1e-6))
    new = {n: (p[n].detach() - float(g["lr"]) * coef * gr) for n, gr in zip(names, grads)}
    check_fn_trainer_updates(g, new, {n: p[n] for n in names}, names, 2e-2, 5e-5)


@pytest.mark.parametrize("cfg", ["A", "B"])
def test_fd_training_step_matches_reference(cfg):
    """Row f-5: one training step of the WHOLE fd model (train() mode, dropout 0) — oracle.train_path.fd_train_forward in f32,
    forced on the reference's own kNN tables and hard spikes, against what tests/golden/fd_train.npz (A) and fd_train_b.npz (B)
    store of the reference's run: pooled / integrated taps, prediction, loss, every gradient (check_fn_train_grads, and the row
    norms of the three large tensors), the grad-is-None and exactly-zero sets, the BatchNorm buffers and num_batches_tracked, and
    the oracle's own spikes (u > 0) against the reference's.

    Both sides are CPU torch in f32: only the summation order differs.  Measured on two hosts with different CPUs (on each, 1 and 8
    threads give the same figures to the digits shown; the digits depend on the CPU's torch kernels):

        A: pooled 6.2e-06, integrated 2.6e-06, prediction 6.0e-07, loss 1.3e-07; gradients 0.00176 of the device's bar; buffers 7.8e-08
        B: pooled 6.7e-06, integrated 2.9e-06, prediction 8.6e-07, loss 6.0e-08; gradients 0.00138 of the device's bar; buffers 1.2e-07
        A: pooled 5.0e-06, integrated 2.4e-06, prediction 4.8e-07, loss 3.0e-08; gradients 0.00183 of the device's bar; buffers 6.7e-08
        B: pooled 8.6e-06, integrated 2.9e-06, prediction 3.0e-07, loss 6.0e-08; gradients 0.00694 of the device's bar; buffers 1.2e-07

    The bars are the largest figure of each kind times 4 (thread-count-dependent summation order): 3.4e-5 for the values,
    4 x 0.00694 = 0.0278 of the device's gradient bar, 4.8e-7 for the buffers (FD_PIN_BARS below) — a sixth of the device's value
    bar, a thirty-sixth of its gradient bar and a twentieth of its buffer bar (2e-4; 2e-2 / 5e-5; 1e-5).  No spike of either run
    differs from the reference's."""
    from oracle import train_path as TP
    from test_gpu_fd_train import _config
    kw, g, sd, names = _config(cfg)
    P, M, Tn, emb = int(g["P"]), int(g["M"]), kw["time_steps_enc"], kw["emb_dims"]
    p = {n: sd[n].clone().requires_grad_(True) for n in names}
    p.update({n: v.clone() for n, v in sd.items() if n not in p})
    spikes = t(np.unpackbits(g["spikes"], axis=-1)[..., :960].astype(np.float32))
    fc = t(np.unpackbits(g["fc_spikes"], axis=-1)[..., :emb].astype(np.float32))
    force = {"fc": fc}
    for s in range(Tn):
        for b, (lo, hi) in enumerate(((0, 64), (64, 192), (192, 448), (448, 960))):
            force[(s, b)] = spikes[s, :, lo:hi].contiguous()
    taps = {}
    pred = TP.fd_train_forward(p, t(g["input"]), kw["k"], tuple(kw["k_scales"]), Tn, kw["num_heads"], knn=t(g["knn"].astype(np.int64)),
                               momentum=0.1, taps=taps, force_spikes=force)
    loss = TP.distance_loss(pred, t(g["gt"]))
    loss.backward()
    own = torch.stack([torch.cat([(u > 0).float() for u in taps["preact"][4 * s:4 * s + 4]], dim=1) for s in range(Tn)])
    assert torch.equal(own, spikes) and torch.equal((taps["fc_preact"][0] > 0).float(), fc)
    assert torch.equal(torch.stack(taps["knn"]), t(g["knn"].astype(np.int64)))
    e = {"pooled": float((torch.stack(taps["pooled"]) - t(g["pooled"])).abs().max()),
         "integrated": float((taps["integrated"][0] - t(g["integrated"])).abs().max()),
         "prediction": float((pred.detach() - t(g["pred"])).abs().max()), "loss": abs(float(loss.detach()) - float(g["loss"]))}
    assert {n for n in names if p[n].grad is None} == {str(n) for n in g["grad_none"]}
    assert {n for n in names if p[n].grad is not None and not bool(p[n].grad.any())} == {str(n) for n in g["grad_zero"]}
    graded = [n for n in names if p[n].grad is not None]
    tol, floor_rel = FD_PIN_BARS["grads"]
    worst = check_fn_train_grads(g, p, graded, tol, floor_rel)
    # the same comparison as a share of the device's bar 2e-2 max|ref| + 5e-5 peak, the figure the docstring quotes
    peak = max(float(np.abs(g[("g:" if ("g:" + n) in g else "gs:") + n]).max()) for n in graded)
    share = 0.0
    for n in graded:
        got = p[n].grad.numpy().ravel()
        ref, got = (g["g:" + n].ravel(), got) if ("g:" + n) in g else (g["gs:" + n], got[g["gi:" + n]])
        share = max(share, float(np.abs(got - ref).max()) / (2e-2 * float(np.abs(ref).max()) + 5e-5 * peak))
    big = [n for n in names if ("grn:" + n) in g]
    assert sorted(big) == ["encoder.conv_blocks.1.0.weight", "encoder.conv_blocks.2.0.weight", "encoder.multi_scale_conv.0.weight"]
    for n in big:
        got = np.linalg.norm(p[n].grad.numpy().reshape(p[n].shape[0], -1).astype(np.float64), axis=1)
        bar = tol * g["grn:" + n].max() + floor_rel * peak * np.sqrt(p[n][0].numel())
        share = max(share, float(np.abs(got - g["grn:" + n]).max()) / (2e-2 * g["grn:" + n].max() + 5e-5 * peak * np.sqrt(p[n][0].numel())))
        assert np.abs(got - g["grn:" + n]).max() <= bar, n
    e_buf = 0.0
    for n in sd:
        if n in names:
            continue
        if n.endswith("num_batches_tracked"):
            assert int(p[n]) == int(g["buf:" + n]), n
        else:
            e_buf = max(e_buf, float(np.abs(p[n].numpy() - g["buf:" + n]).max()))
    assert int(p["encoder.scale_fusion.1.num_batches_tracked"]) == Tn and int(p["encoder.conv_blocks.0.1.num_batches_tracked"]) == Tn
    print("config %s: pooled %.3g, integrated %.3g, prediction %.3g, loss %.3g; gradients %.3g of the device's bar (worst error / scale "
          "%.3g); buffers %.3g" % (cfg, e["pooled"], e["integrated"], e["prediction"], e["loss"], share, worst, e_buf))
    assert max(e.values()) <= FD_PIN_BARS["values"], e
    assert e_buf <= FD_PIN_BARS["buffers"], e_buf


# (values: taps, prediction and loss; grads: (tol, floor_rel) of check_fn_train_grads; buffers) — see the docstring above
FD_PIN_BARS = {"values": 3.4e-5, "grads": (0.0278 * 2e-2, 0.0278 * 5e-5), "buffers": 4.8e-7}


def test_reference_against_itself_fixture():
    """tests/golden/ref_vs_ref.npz (make_fixtures.py --only-ref-vs-ref): the REAL reference run with 1 thread and with 8 threads —
    the floor under every free-running fd parity figure quoted in DESIGN.md section 2 and profiles/r03_flip_sources.md.  fd alone is
    bit-stable across thread counts on the build host (0 flipped neighbour sets on 256 patches); end to end, fn's thread-dependent
    sums (~6e-6 on the normals) rotate the patches by enough to flip fd neighbours: 96.8 % of the refined points within 2e-4."""
    g = golden("ref_vs_ref.npz")
    assert list(g["threads"]) == [1, 8]
    assert int(g["fd256_flip_patches"]) == 0 and float(g["fd256_max_abs_diff"]) == 0.0
    assert int(g["e2e_points"]) == 901 and 0.9 <= float(g["e2e_within_2e4"]) < 1.0 and float(g["e2e_median"]) < 1e-5
