"""fn blocks end with out_proj and fc2, two affine maps with nothing between them (fn/snn_coder.py:393-394).  sapcu_model_create
folds them into one, W' = W_fc2 . W_out and b' = W_fc2 . b_out + b_fc2 (csrc/model.hip fold_affine_f64: f64 sums, rounded to f32
once), and the forward runs ONE GEMM per block instead of two; SAPCU_FN_FOLD_OUT=0 keeps the two-GEMM form.

* CPU: the fold routine against a numpy f64 product of the BatchNorm-folded layers, all three blocks, equal after rounding to f32.
* GPU: the forward with the fold on against SAPCU_FN_FOLD_OUT=0 on the golden fn inputs, one child process per setting.

The removed launches themselves (per step 2 x gemm_bt_kernel<EPI_BIAS, 256> + 1 x gemm_bt_kernel<EPI_BIAS, 128>) are NOT counted
here: the library has no launch counter, so that they are gone is asserted from the kernel table of the profile run
(profiles/r07_summary.md against profiles/r04_summary.md: the EPI_BIAS big-tile rows lose 3 calls per step)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

FN_BLK0, B_SLOTS, B_OUT_W, B_OUT_B, B_FC2_W, B_FC2_B = 3, 21, 17, 18, 19, 20      # csrc/model.hip FnSlot / FnBlkSlot
TOL = 1e-4


def _slot(blob, d, i, n):
    return np.ascontiguousarray(blob[int(d[i]):int(d[i]) + n])


def test_fold_routine_equals_the_f64_product_of_the_bn_folded_layers(weights):
    """sapcu_internal_fold_affine_host is the routine sapcu_model_create calls (same function, host pointers): its W', b' for the
    packed (BatchNorm-folded, f32) out_proj and fc2 of the three blocks equal numpy's f64 product rounded to f32, bit for bit."""
    import ctypes
    from sapcu_amd import _lib, packing
    lib = _lib.load()
    blob, dr = packing.pack_fn(weights("fn"))
    for l in range(3):
        d, sb = 128 << l, FN_BLK0 + l * B_SLOTS
        w1, b1 = _slot(blob, dr, sb + B_OUT_W, d * d), _slot(blob, dr, sb + B_OUT_B, d)
        w2, b2 = _slot(blob, dr, sb + B_FC2_W, 64 * d), _slot(blob, dr, sb + B_FC2_B, 64)
        wf, bf = np.full(64 * d, np.nan, np.float32), np.full(64, np.nan, np.float32)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        assert lib.sapcu_internal_fold_affine_host(p(w1), p(b1), p(w2), p(b2), d, 64, p(wf), p(bf)) == 0
        W1, W2 = w1.reshape(d, d).astype(np.float64), w2.reshape(64, d).astype(np.float64)
        want_w = (W2 @ W1).astype(np.float32)
        want_b = (W2 @ b1.astype(np.float64) + b2.astype(np.float64)).astype(np.float32)
        assert np.abs(want_w).max() > 1e-3                       # a real product, not zeros
        assert np.array_equal(wf.reshape(64, d), want_w), "block %d: %d of %d folded weights differ" % (l + 1, int((wf.reshape(64, d) != want_w).sum()), wf.size)
        assert np.array_equal(bf, want_b), "block %d: folded bias differs" % (l + 1)
        # what the fold replaces: the two layers applied one after the other, in f64
        x = np.random.default_rng(l).standard_normal((5, d))
        two = (x @ W1.T + b1) @ W2.T + b2
        assert np.abs(x @ wf.reshape(64, d).astype(np.float64).T + bf - two).max() <= 1e-5 * np.abs(two).max()
    assert lib.sapcu_internal_fold_affine_host(None, None, None, None, 128, 64, None, None) == -1


# ------------------------------------------------------------------------------------------------ the bar, from the oracle itself
def _oracle_fn(sd, patch, tail_f64):
    """oracle.snn_path.fn_forward spelled out with its own primitives, with out_proj and fc2 of every block evaluated in f32 (as the
    oracle does) or in f64 (rounded to f32 before the residual is added): -> ([block1, block2, block3], normals)."""
    from oracle import snn_path as O
    import torch.nn.functional as F
    import gpu_utils as U
    hp = U.FN_HP
    sd64 = {k: v.double() for k, v in sd.items() if (".out_proj." in k or ".fc2." in k) and v.is_floating_point()}
    x = patch.permute(0, 2, 1).contiguous()
    xyz = patch.contiguous()
    feat = O.neuron_selfloop(O.conv_bn(x, sd, "encoder.conv1"), O.neuron_params(sd, "encoder.snn_init"), hp["time_steps_enc"])
    feat = feat.permute(0, 2, 1).contiguous()
    outs = []
    for bi, (name, d) in enumerate(O.FN_BLOCKS):
        pfx, T = "encoder." + name, O.FN_BLOCK_T
        idx = O.inpatch_knn(x, min(hp["k_values"][bi], xyz.shape[1]))
        pos = xyz.permute(0, 2, 1)
        pos_diff = pos.unsqueeze(-1) - O.gather_cols(pos, idx)
        pre = feat.permute(0, 2, 1).contiguous()
        h = O.neuron_selfloop(O.conv_bn(pre, sd, pfx + ".fc1"), O.neuron_params(sd, pfx + ".snn1"), T)
        q = O.neuron_selfloop(O.conv_bn(h, sd, pfx + ".w_qs"), O.neuron_params(sd, pfx + ".snn_q"), T)
        kf = O.neuron_selfloop(O.conv_bn(h, sd, pfx + ".w_ks"), O.neuron_params(sd, pfx + ".snn_k"), T)
        v = O.neuron_selfloop(O.conv_bn(h, sd, pfx + ".w_vs"), O.neuron_params(sd, pfx + ".snn_v"), T)
        kg, vg = O.gather_cols(kf, idx), O.gather_cols(v, idx)
        pe = O.neuron_selfloop(O.conv_bn(pos_diff.contiguous(), sd, pfx + ".fc_delta"), O.neuron_params(sd, pfx + ".snn_delta"), T)
        pe = O.neuron_selfloop(O.conv_bn(pe, sd, pfx + ".fc_delta2"), O.neuron_params(sd, pfx + ".snn_delta2"), T)
        a = q.unsqueeze(-1) - kg + pe
        a = O.neuron_selfloop(O.conv_bn(a, sd, pfx + ".fc_gamma"), O.neuron_params(sd, pfx + ".snn_gamma"), T)
        a = F.softmax(O.conv_bn(a, sd, pfx + ".fc_gamma2") / np.sqrt(d // hp["num_heads"]), dim=-1)
        res = torch.einsum("bcnk,bcnk->bcn", a, vg + pe)
        if tail_f64:
            res = O.conv_bn(O.conv_bn(res.double(), sd64, pfx + ".out_proj"), sd64, pfx + ".fc2").float() + pre
        else:
            res = O.conv_bn(O.conv_bn(res, sd, pfx + ".out_proj"), sd, pfx + ".fc2") + pre
        feat = res.permute(0, 2, 1).contiguous()
        outs.append(feat)
    ms = torch.cat(outs, dim=2).permute(0, 2, 1)
    g = O.neuron_selfloop(O.conv_bn(ms, sd, "encoder.conv_final"), O.neuron_params(sd, "encoder.snn_final"), hp["time_steps_enc"])
    return [o.numpy() for o in outs], O.fn_decoder(sd, O.linear(g.max(dim=2)[0], sd, "encoder.fc_out")).numpy()


def _child(env_over, out):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAPCU_")}
    env.update(env_over)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fn_fold_out_check.py"), out], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0 and "FN_FOLD_OUT_CHECK_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    return dict(np.load(out))


@pytest.mark.gpu
@pytest.mark.parametrize("base", [{}, {"SAPCU_CHAIN": "0"}, {"SAPCU_GEMM": "f32"}], ids=["default", "unfused_chain", "f32_gemm"])
def test_folded_forward_against_the_two_gemm_form(weights, tmp_path, base):
    """Fold on (default) against SAPCU_FN_FOLD_OUT=0 on the golden fn inputs (4 patches of 48 points), one child process per setting;
    on the fused edge chain, on the five-kernel chain (SAPCU_CHAIN=0) and on the exact-f32 GEMMs (SAPCU_GEMM=f32).

    The bar is not a guess: the fold changes where the two layers round, nothing else, so the yardstick is what the ORACLE itself
    moves by when only the rounding of these two layers changes — its forward with out_proj and fc2 evaluated in f64 against its
    usual f32 evaluation, same patches, everything else identical (_oracle_fn above reproduces oracle.snn_path.fn_forward, which is
    checked first).  That spread is taken per block tap and for the normals (a block's tap carries what the earlier blocks' spread
    became on its way through the neurons, on the device as in the oracle), and the two device forms may differ by 4 x that.
    Both forms also stay within the suite's 1e-4 of the reference vectors.

    Measured on MI355X, max |fold - two GEMMs| on the device (the test prints them), beside the oracle's f32/f64 spread on that
    box and the bar = 4 x spread:
                  split-f16 GEMMs (fused and five-kernel chain: same figures)   SAPCU_GEMM=f32   oracle spread   bar
      block1      2.19e-05                                                      4.01e-05         2.52e-05        1.01e-04
      block2      3.15e-05                                                      4.77e-05         3.24e-05        1.30e-04
      block3      3.91e-05                                                      6.39e-05         3.90e-05        1.56e-04
      normals     4.03e-06                                                      6.85e-06         6.12e-06        2.45e-05
    (block outputs reach 3.8 / 5.4 / 6.8 in magnitude.)
    """
    from oracle import snn_path as O
    import gpu_utils as U
    g = golden("fn_taps.npz")
    sdn = weights("fn")
    patch = torch.from_numpy(g["patch"])
    with torch.no_grad():
        taps32, n32 = _oracle_fn(sdn, patch, False)
        taps64, n64 = _oracle_fn(sdn, patch, True)
        n_ref = O.fn_forward(sdn, patch, U.FN_HP).numpy()
    assert np.array_equal(n32, n_ref), "the spelled-out oracle forward is not the oracle's"
    spread = {"block%d" % (l + 1): float(np.abs(taps32[l] - taps64[l]).max()) for l in range(3)}
    spread["normals"] = float(np.abs(n32 - n64).max())

    on = _child(dict(base), str(tmp_path / "on.npz"))
    off = _child(dict(base, SAPCU_FN_FOLD_OUT="0"), str(tmp_path / "off.npz"))
    assert int(on["split_f16"]) == int(off["split_f16"]) == (0 if base.get("SAPCU_GEMM") == "f32" else 1)
    want_mask = 0 if (base.get("SAPCU_CHAIN") == "0" or base.get("SAPCU_GEMM") == "f32") else 7
    assert int(on["fused_mask"]) == int(off["fused_mask"]) == want_mask
    diff = {k: float(np.abs(on[k] - off[k]).max()) for k in spread}
    for k in ("block1", "block2", "block3", "normals"):
        print("fn fold_out [%s] %-7s |fold - two GEMMs| %.3e   oracle f32/f64 spread %.3e   bar %.3e" %
              (",".join("%s=%s" % kv for kv in base.items()) or "default", k, diff[k], spread[k], 4 * spread[k]), flush=True)
    assert diff["block1"] > 0, "the two settings ran the same arithmetic: the switch did nothing"
    # both forms against the reference vectors, the bars of test_gpu_parity.py::test_fn_stage_taps_against_reference_vectors
    for name, run in (("fold", on), ("two GEMMs", off)):
        for k in ("block1", "block2", "block3", "enc", "logits"):
            err = np.abs(run[k] - g[k]).max()
            assert err <= TOL * max(1.0, np.abs(g[k]).max()), "%s %s: %g" % (name, k, err)
        np.testing.assert_allclose(run["normals"], g["normals"], rtol=0, atol=TOL)
    for k in ("block1", "block2", "block3", "normals"):
        assert diff[k] <= 4 * spread[k], "%s: fold vs two GEMMs %.3e > 4 x the oracle's f32/f64 spread %.3e" % (k, diff[k], spread[k])
