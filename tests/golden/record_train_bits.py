#!/usr/bin/env python3
"""Record the SHA-256 of every output tensor of the training entry points -> train_bits.json (tests/test_gpu_train_bits.py replays
the cases and compares).

    python tests/golden/record_train_bits.py            (needs the GPU)

Public ABI through sapcu_amd._lib only, so the same file runs on any earlier commit.  train_bits.json is recorded AT THE PARENT of the
change that moved the training kernels' shared device idioms into csrc/train_common.h (the four-group column fold, the inverse
neighbour table, the clamp ranges, the batch statistics, bn_lrelu, the slab sum, the softmax weights): that change and every later one
must leave these bits alone, and the file is not to be re-recorded because a helper changed by accident.

Inputs come from numpy.random.RandomState seeded by the case's name and are copied to the device; no device RNG.  Outputs and
workspaces start zeroed.  The shapes are the smallest at which each shared piece can go wrong: more row blocks than a final pass's
stride (4097 rows: 17 blocks over a stride of 16; 300 points: 19 and 5 blocks over a stride of 4), a second, mostly dead channel
tile (65 channels), raw neuron parameters on both sides of every clamp range, groups with more entries / more destinations than
threads, repeated neighbours, destinations nobody points at, and indices outside their patch where the entry point counts them.
"""
import hashlib
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "train_bits.json")

BN_ROWS, BN_CH = (1, 255, 257, 4097), (3, 65)
LIF_STEPS, LIF_ROWS, LIF_CH = (1, 4, 8), (1, 65, 1025), (3, 65)
STEP_ROWS, STEP_CH = (1, 130), (3, 65)
GROUPS = ((1, 1), (5, 3), (100, 20), (257, 2))        # (m, kk), two groups each
GROUP_D = (3, 65)
EDGECONV = ((1, 1, 1, 3), (3, 100, 20, 65))           # (P, M, kk, C)
PIECES = ("bn", "lif", "step", "group", "edgeconv", "wgrad_f32", "wgrad_bf16")
# clamp range of each raw neuron parameter (the reference's torch.clamp bounds)
RANGES = {"md": (0.1, 0.99), "ta": (0.001, 0.1), "rd": (0.1, 0.95), "dT": (0.1, 5.0), "rh": (0.1, 2.0)}


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def _raw(rs, ch, key, shift):
    """ch raw values over a range 30 % wider than the clamp's on both sides; channel shift % 3 lies below it, the next one above"""
    lo, hi = RANGES[key]
    w = hi - lo
    v = rs.uniform(lo - 0.3 * w, hi + 0.3 * w, ch)
    v[shift % 3 % ch] = lo - 0.1 * w
    v[(shift + 1) % 3 % ch] = hi + 0.1 * w
    if ch >= 3:
        v[(shift + 2) % 3] = 0.5 * (lo + hi)
    return v.astype(np.float32)


def _table(rs, groups, m, kk, bad):
    """int32 [groups, m, kk] in-patch neighbours: repeated ones, nobody points at point m - 1 of group 0 (m > 1), and, with `bad`,
    entries outside [0, m) — every entry of the last group when a group has only one"""
    idx = rs.randint(0, m, (groups, m, kk)).astype(np.int32)
    idx[:, :, kk // 2] = idx[:, :, 0]
    if m > 1:
        idx[0][idx[0] == m - 1] = 0
    if bad:
        flat = idx.reshape(groups, -1)
        flat[-1, 0] = m
        flat[0, -1] = -1 if flat.shape[1] > 1 else flat[0, -1]
        flat[-1, flat.shape[1] // 2] = m + 3
    return idx


class Runner(object):
    def __init__(self, dev):
        import torch
        from sapcu_amd import _lib
        self.torch, self.L, self.lib, self.dev = torch, _lib, _lib.load(), dev

    def up(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a), device=self.dev)

    def f32(self, rs, *shape, scale=1.0):
        return self.up((rs.standard_normal(shape) * scale).astype(np.float32))

    def zeros(self, *shape, dtype=None):
        return self.torch.zeros(shape, dtype=dtype or self.torch.float32, device=self.dev)

    def ws(self, sizer, *sizes):
        n = int(getattr(self.lib, sizer)(*sizes))
        assert n >= 0, (sizer, sizes)
        return self.zeros(max(n, 8), dtype=self.torch.uint8), n

    def call(self, name, *args):
        self.L.call(name, self.dev, *args)

    # ---- one function per piece: {case id: [output tensors]}
    def bn(self):
        out = {}
        for rows in BN_ROWS:
            for ch in BN_CH:
                cid = "bn/r%d/c%d" % (rows, ch)
                rs = _rs(cid)
                y, gz = self.f32(rs, rows, ch, scale=2.0), self.f32(rs, rows, ch)
                gamma, beta = self.f32(rs, ch), self.f32(rs, ch)
                z, mean, var, invstd = self.zeros(rows, ch), self.zeros(ch), self.zeros(ch), self.zeros(ch)
                ws, n = self.ws("sapcu_train_workspace_bytes", rows, ch, 0)
                self.call("sapcu_bn_train_forward", y, rows, ch, gamma, beta, 1e-5, z, mean, var, invstd, ws, n)
                gy, gg, gb = self.zeros(rows, ch), self.zeros(ch), self.zeros(ch)
                ws, n = self.ws("sapcu_train_workspace_bytes", rows, ch, 0)
                self.call("sapcu_bn_train_backward", y, gz, rows, ch, gamma, mean, invstd, gy, gg, gb, ws, n)
                m2, v2, i2 = self.zeros(ch), self.zeros(ch), self.zeros(ch)
                ws, n = self.ws("sapcu_fd_bn_stats_workspace_bytes", rows, ch)
                self.call("sapcu_fd_bn_stats", y, rows, ch, 1e-5, m2, v2, i2, ws, n)
                out[cid] = [z, mean, var, invstd, gy, gg, gb, m2, v2, i2]
        return out

    def lif(self):
        out = {}
        for steps in LIF_STEPS:
            for rows in LIF_ROWS:
                for ch in LIF_CH:
                    cid = "lif/t%d/r%d/c%d" % (steps, rows, ch)
                    rs = _rs(cid)
                    x, g = self.f32(rs, rows, ch, scale=1.5), self.f32(rs, rows, ch)
                    prm = [self.up(_raw(rs, ch, k, i)) for i, k in enumerate(("md", "ta", "rd"))]
                    prm.append(self.up(rs.uniform(0.2, 1.0, ch).astype(np.float32)))
                    sp = self.zeros(rows, ch)
                    self.call("sapcu_lif_train_forward", x, rows, ch, steps, *prm, sp)
                    gx, gp = self.zeros(rows, ch), [self.zeros(ch) for _ in range(4)]
                    ws, n = self.ws("sapcu_lif_train_workspace_bytes", rows, ch)
                    self.call("sapcu_lif_train_backward", x, g, rows, ch, steps, *prm, gx, *gp, ws, n)
                    out[cid] = [sp, gx] + gp
        return out

    def step(self):
        out = {}
        for eif in (0, 1):
            for carried in (0, 1):
                for rows in STEP_ROWS:
                    for ch in STEP_CH:
                        cid = "step/%s/%s/r%d/c%d" % ("eif" if eif else "lif", "carried" if carried else "first", rows, ch)
                        rs = _rs(cid)
                        x, g = self.f32(rs, rows, ch, scale=1.5), self.f32(rs, rows, ch)
                        md, ta, rd = (self.up(_raw(rs, ch, k, i)) for i, k in enumerate(("md", "ta", "rd")))
                        tb = self.up(rs.uniform(0.2, 1.0, ch).astype(np.float32))
                        dT, rh = (self.up(_raw(rs, ch, "dT", 1)), self.up(_raw(rs, ch, "rh", 2))) if eif else (None, None)
                        state = [None] * 3
                        if carried:
                            state = [self.f32(rs, rows, ch), self.up(rs.uniform(0.3, 1.0, (rows, ch)).astype(np.float32)),
                                     self.up(rs.choice(np.float32([0, 0, 0.5, 1.0]), (rows, ch)))]
                        fw = [self.zeros(rows, ch) for _ in range(5)]
                        self.call("sapcu_fd_neuron_step_forward", x, rows, ch, eif, md, ta, rd, tb, dT, rh, *state, None, *fw)
                        gx, gmd, gtb = self.zeros(rows, ch), self.zeros(ch), self.zeros(ch)
                        gdT, grh = (self.zeros(ch), self.zeros(ch)) if eif else (None, None)
                        ws, n = self.ws("sapcu_fd_neuron_step_workspace_bytes", rows, ch)
                        self.call("sapcu_fd_neuron_step_backward", x, g, rows, ch, eif, md, tb, dT, rh, *state, gx, gmd, gtb, gdT, grh, ws, n)
                        out[cid] = fw + [gx, gmd, gtb] + ([gdT, grh] if eif else [])
        return out

    def group(self):
        t, out = self.torch, {}
        for m, kk in GROUPS:
            for d in GROUP_D:
                cid = "group/m%d/k%d/d%d" % (m, kk, d)
                rs = _rs(cid)
                G, gr = 2, m * kk
                bad_tab, ok_tab = _table(rs, G, m, kk, True), _table(rs, G, m, kk, False)
                # sapcu_scatter_add_rows_grouped: global int64 rows, some outside their group
                glob = self.up((bad_tab.astype(np.int64) + (np.arange(G, dtype=np.int64) * m).reshape(G, 1, 1)).reshape(-1))
                go = self.f32(rs, G * gr, d)
                gsrc, bad = self.zeros(G * m, d), self.zeros(1, dtype=t.int32)
                self.call("sapcu_scatter_add_rows_grouped", go, glob, G * gr, d, gsrc, d, G * m, m, gr, bad)
                res = [gsrc, bad]
                # the softmax aggregate reads v through the table: in-range tables only
                a, pe, v, gres = self.f32(rs, G * gr, d, scale=3.0), self.f32(rs, G * gr, d), self.f32(rs, G * m, d), self.f32(rs, G * m, d)
                keep = self.up((rs.uniform(0, 1, (G * gr, d)) > 0.25).astype(np.float32) / 0.75)
                idx = self.up(ok_tab.reshape(-1))
                for kp in (None, keep):
                    ga, gpe, gv = self.zeros(G * gr, d), self.zeros(G * gr, d), self.zeros(G * m, d)
                    self.call("sapcu_softmax_agg_backward", a, pe, v, d, idx, kp, gres, G * m, m, kk, d, 2.5, ga, gpe, gv, d)
                    res += [ga, gpe, gv]
                fwd = self.zeros(G * m, d)
                self.call("sapcu_softmax_agg_forward", a, pe, v, d, idx, keep, G * m, m, kk, d, 2.5, fwd)
                res.append(fwd)
                # sapcu_fd_edge_feature_backward counts the indices outside the patch
                oc = 2 * d + 2
                gf = self.f32(rs, G * gr, oc)
                gx, bad2 = self.zeros(G * m, d), self.zeros(1, dtype=t.int32)
                self.call("sapcu_fd_edge_feature_backward", gf, self.up(bad_tab), G, m, kk, d, oc, gx, d, bad2)
                out[cid] = res + [gx, bad2]
        return out

    def edgeconv(self):
        t, out = self.torch, {}
        for P, M, kk, C in EDGECONV:
            cid = "edgeconv/p%d/m%d/k%d/c%d" % (P, M, kk, C)
            rs = _rs(cid)
            pts = P * M
            idx = self.up(_table(rs, P, M, kk, M > 1))
            ab, go = self.f32(rs, pts, 2 * C), self.f32(rs, pts, C)
            gamma, beta = self.f32(rs, C), self.f32(rs, C)
            mean, var, invstd, bad = self.zeros(C), self.zeros(C), self.zeros(C), self.zeros(1, dtype=t.int32)
            ws, n = self.ws("sapcu_fd_edgeconv_stats_workspace_bytes", P, M, kk, C)
            self.call("sapcu_fd_edgeconv_stats", ab, idx, P, M, kk, C, 1e-5, mean, var, invstd, bad, ws, n)
            mx, arg = self.zeros(pts, C), self.zeros(pts, C, dtype=t.int32)
            self.call("sapcu_fd_edgeconv_max_forward", ab, idx, P, M, kk, C, mean, invstd, gamma, beta, mx, arg)
            gab, gg, gb, bad2 = self.zeros(pts, 2 * C), self.zeros(C), self.zeros(C), self.zeros(1, dtype=t.int32)
            ws, n = self.ws("sapcu_fd_edgeconv_backward_workspace_bytes", P, M, kk, C)
            self.call("sapcu_fd_edgeconv_backward", ab, idx, go, arg, P, M, kk, C, mean, invstd, gamma, beta, gab, gg, gb, bad2, ws, n)
            out[cid] = [mean, var, invstd, bad, mx, arg, gab, gg, gb, bad2]
        return out

    def _wgrad(self, entry, sizer, rows, n, k, bias):
        cid = "%s/r%d/n%d/k%d/%s" % (entry, rows, n, k, "bias" if bias else "nobias")
        rs = _rs(cid)
        gy, x = self.f32(rs, rows, n), self.f32(rs, rows, k)
        gw, gb = self.zeros(n, k), self.zeros(n) if bias else None
        ws, nb = self.ws(sizer, rows, n, k)
        self.call(entry, gy, n, x, k, rows, n, k, gw, gb, ws, nb)
        return cid, [gw] + ([gb] if bias else [])

    def wgrad_f32(self):
        return dict(self._wgrad("sapcu_conv1x1_wgrad_f32", "sapcu_train_workspace_bytes", 1031, 96, 40, b) for b in (True, False))

    def wgrad_bf16(self):
        return dict(self._wgrad("sapcu_conv1x1_wgrad_bf16", "sapcu_wgrad_bf16_workspace_bytes", r, 64, 32, True) for r in (1031, 100))


def digests(piece, dev):
    """{case id: [sha256 of each output tensor's bytes]} of one of PIECES on `dev`"""
    import torch
    res = getattr(Runner(dev), piece)()
    torch.cuda.synchronize(dev)
    return {cid: [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in outs] for cid, outs in res.items()}


def main():
    import torch
    dev = torch.device("cuda:0")
    data = {piece: digests(piece, dev) for piece in PIECES}
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %s" % (OUT, {p: len(data[p]) for p in data}))


if __name__ == "__main__":
    main()
