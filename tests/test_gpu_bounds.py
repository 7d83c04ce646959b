"""Memory contract of the C ABI (-m gpu): every pointer-taking entry point of include/sapcu.h under guard bands.

One table (CASES) drives the file.  For each case every output, workspace and input is a guarded buffer (tests/guarded.py):
  1. input bands 0xFF, workspaces pre-filled 0xFF, outputs pre-filled 0xFF (NaN / -1): every band and pitch gap intact, outputs
     fully written;
  2. input bands 0x00, workspaces pre-filled 0x00: outputs bit-identical to run 1 (a stray read that reaches a result shows);
  3. once more on the dirty workspaces of run 2: bit-identical again;
  4. the same call on compact, allocator-aligned arrays with pitch == width (the way tests/test_gpu_parity.py calls): bit-identical,
     and that result against the high-precision reference of the entry point's parity test at that test's tolerance.
Workspaces have exactly the size their sizer returns.  REFUSALS holds calls just outside a documented restriction: they must
return their status without launching (outputs and bands untouched).  tests/test_guarded.py holds the coverage gate.
"""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

from guarded import Arena
import gpu_utils as U

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
Case = namedtuple("Case", "id entry_points sizers build")
Built = namedtuple("Built", "call outs ref canon counters")
CASES, REFUSALS = [], []


def case(id_, entry_points, sizers=()):
    def deco(fn):
        CASES.append(Case(id_, tuple(entry_points), tuple(sizers), fn))
        return fn
    return deco


def _lib_():
    from sapcu_amd import _lib
    return _lib, _lib.load()


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    _lib_()[0].check(rc)


def built(call, outs, ref, canon=None, counters=None):
    """counters: None, or a callable returning {name: (value read from the device, expected value)} — counters that live inside a
    workspace (the split-f16 overflow counters) are no outputs, so the protocol reads them after EVERY run: on the 0xFF-filled,
    the zeroed and the dirty workspace they must hold what the call itself counted."""
    return Built(call, outs, ref, canon or {}, counters)


_SEEN = {}


def _check_counters(b, tag, key=None):
    """want = an int, or None: non-zero and the same count after every run of the case (the unit of the count is the kernel's)."""
    if b.counters is not None:
        for name, (got, want) in b.counters().items():
            if want is None:
                want = _SEEN.setdefault((key, name), got)
                assert got > 0, "%s: counter %s is 0 although values beyond the f16 range were fed" % (tag, name)
            assert got == want, "%s: counter %s holds %d, expected %d" % (tag, name, got, want)


def _bits(t):
    return t.detach().contiguous().clone().view(U8).cpu() if t.numel() else torch.empty(0, dtype=U8)


def _snapshot(b):
    out = {}
    for name, t in b.outs.items():
        c = t.detach().contiguous().clone()
        out[name] = _bits(b.canon[name](c) if name in b.canon else c)
    return out


def _assert_written(b, tag):
    for name, t in b.outs.items():
        if name in b.canon or not t.numel():                 # split rows: the f16 halves of a row do not fill its container
            continue
        c = t.detach().contiguous()
        allff = (c.view(U8).view(-1, c.element_size()) == 0xFF).all(dim=1)
        assert not bool(allff.any()), "%s: output %s has %d elements never written" % (tag, name, int(allff.sum()))


def _same(a, b, tag):
    for name in a:
        assert torch.equal(a[name], b[name]), "%s: output %s differs (%d bytes)" % (tag, name, int((a[name] != b[name]).sum()))


def run_protocol(c):
    dev = U.dev()
    A1 = Arena("guard", 0xFF, dev)
    b1 = c.build(A1)
    b1.call()
    torch.cuda.synchronize()
    A1.check()
    _check_counters(b1, c.id + " run 1 (workspace pre-filled 0xFF)", c.id)
    _assert_written(b1, c.id + " run 1")
    s1 = _snapshot(b1)
    A2 = Arena("guard", 0x00, dev)
    b2 = c.build(A2)
    b2.call()
    torch.cuda.synchronize()
    A2.check()
    _check_counters(b2, c.id + " run 2 (workspace pre-filled 0x00)", c.id)
    s2 = _snapshot(b2)
    _same(s1, s2, c.id + " run 2 (0x00 bands, zeroed workspace) vs run 1 (0xFF)")
    A2.refill_outputs()
    b2.call()
    torch.cuda.synchronize()
    A2.check()
    _check_counters(b2, c.id + " run 3 (dirty workspace)", c.id)
    _assert_written(b2, c.id + " run 3")
    _same(s1, _snapshot(b2), c.id + " run 3 (dirty workspace) vs run 1")
    A4 = Arena("compact", 0x00, dev)
    b4 = c.build(A4)
    b4.call()
    torch.cuda.synchronize()
    _check_counters(b4, c.id + " compact call", c.id)
    _same(s1, _snapshot(b4), c.id + " guarded / pitched / offset call vs the compact call")
    b4.ref({k: v.detach().cpu() for k, v in b4.outs.items()})


def _oracle_lif(pre, raw, steps):
    from oracle import snn_path as O
    names = ["membrane_decay", "threshold_adapt", "refractory_decay", "threshold_base"]
    prm = O.neuron_params({"n." + names[i]: torch.from_numpy(raw[i]) for i in range(4)}, "n")
    v, st = pre, None
    for _ in range(steps):
        v, st = O.neuron_step(v, st, prm)
    return v


def _decode_split_rows(t, n):
    """tests/test_gpu_parity.py _decode_split_rows for a container of pitch ld = t.shape[1] >= n floats."""
    rows, ld = t.shape
    halves = t.contiguous().view(torch.float16).view(rows, 2 * ld).float()
    if ld % 32 == 0:
        g = halves.view(rows, ld // 32, 2, 32)
        return (g[:, :, 0, :] + g[:, :, 1, :]).reshape(rows, ld)[:, :n].contiguous()
    return (halves[:, :n] + halves[:, ld:ld + n]).contiguous()


def _raw_lif(rng, n):
    return np.stack([rng.uniform(0.05, 1.1, n), rng.uniform(0.0, 0.2, n), rng.uniform(0.05, 1.0, n), rng.normal(0.5, 0.3, n)]).astype(np.float32)


# ================================================================================================ GEMMs
# tiles (csrc): exact-f32 and split-f16 with f32 A 128 x 128, ring 128 x 128, big-tile 256 x 256/128 (>= 1024 rows, n % 128 == 0)
def _al16(t):
    return t is None or t.data_ptr() % 16 == 0


def _split_rows_kernel(r, k, n, lda, ldc, allow_bt, C, Bv, L):
    """Which kernel a split-row GEMM reaches: csrc/gemm_sf16_bt.hip gemm_sf16_bt_ok (big tile: >= 1024 rows, n % 128 == 0, C / bias /
    lif4 16-byte aligned, ldc % 4 == 0) and csrc/gemm_sf16_ring.hip ring_vec_ok (float4 epilogue: n % 4 == 0, ldc % 4 == 0, the
    same alignments; else the element-wise epilogue).  The library cannot report it, so the rows state it and this mirrors the rule."""
    al = _al16(C) and _al16(Bv) and _al16(L) and ldc % 4 == 0
    if allow_bt and r >= 1024 and n % 128 == 0 and al:
        return "bt"
    return "ring-vec" if al and n % 4 == 0 else "ring-elem"


def _gemm_case(mode, r, k, n, lda_x=0, ldc_x=0, lif=False, csplit=0, in_x=0, aux=4, expect=None, hot=0):
    """aux: base offset (bytes past a 512-byte boundary) of C, bias and lif4: 16 = what the models pass (vector epilogues, big
    tile), 4 = only the element type's alignment (element-wise fall-back).  expect: the kernel a split-row row must reach UNDER
    GUARDS.  hot: number of A values put beyond the f16 range (split-f16 with f32 A counts them in the overflow counter)."""
    def build(A):
        _lib, lib = _lib_()
        rng = np.random.default_rng(r * 7 + n + k)
        a = rng.normal(size=(r, k)).astype(np.float32)
        for h in range(hot):
            a[(h * 37) % r, (h * 5) % k] = 7e4
        w = (rng.normal(size=(n, k)) / (np.sqrt(k) if lif else 1.0)).astype(np.float32)
        bias = rng.normal(size=n).astype(np.float32)
        raw = _raw_lif(rng, n)
        split_a = mode in ("ring", "bt")
        Wt = A.inp(w, offset=16, name="W")                                # the header's alignment: 16 bytes, no more
        Bv = A.inp(bias, offset=aux, name="bias")
        L = A.inp(raw, offset=aux, name="lif4") if lif else None
        ws = A.ws(4 * n * k + 16, tile_row_bytes=4 * k, name="w16_ws") if mode != "f32" else None
        lda = k + (0 if A.compact else lda_x)
        ldc = n + (0 if A.compact else ldc_x)
        if split_a:
            Ain = A.inp(a, pitch=k + (0 if A.compact else in_x), offset=16, name="A f32")
            At = A.out((r, lda), F32, offset=16, name="A split rows")          # a split row owns its whole pitch (sapcu.h)
        else:
            At = A.inp(a, pitch=lda, offset=16, name="A")
        C = A.out((r, ldc), F32, offset=16, name="C") if csplit else A.out((r, n), F32, pitch=ldc, offset=aux, name="C")
        if split_a and expect is not None and not A.compact:
            took = _split_rows_kernel(r, k, n, lda, ldc, mode == "bt", C, Bv, L)
            assert took == expect, "this row is meant to reach %s under guards, its operands select %s" % (expect, took)

        def call():
            if split_a:
                ok(lib.sapcu_to_split_rows(P(Ain), r, k, Ain.stride(0) if r > 1 else k, P(At), lda, S()))
            ok(lib.sapcu_gemm_f32(P(At), r, k, lda, P(Wt), n, P(Bv), P(L), 4 if lif else 0, P(C), ldc, P(ws),
                                  {"f32": 0, "sf16": 0, "ring": 2, "bt": 1}[mode], csplit, S()))

        def ref(o):
            got = _decode_split_rows(o["C"], n) if csplit else o["C"]
            pre = a.astype(np.float64) @ w.astype(np.float64).T + bias
            if hot:                                              # rows with a value beyond f16 are wrong by design: the counter says so
                cold = np.ones(r, bool)
                cold[[(h * 37) % r for h in range(hot)]] = False
                got, pre = got[torch.from_numpy(cold)], pre[cold]
            if lif:
                want = _oracle_lif(torch.from_numpy(pre.astype(np.float32)), raw, 4)
                err = (got - want).abs().max().item()
                assert err <= 2e-5, err
            else:
                err = np.abs(got.numpy() - pre).max()
                assert err <= 2e-6 * np.sqrt(k) * 4, err

        def counters():                                          # last 4 bytes of w16_ws: zeroed by the call, then counted (sapcu.h)
            return {"w16_ws overflow": (int(ws[4 * n * k:4 * n * k + 4].clone().view(I32).item()), None if hot else 0)} if ws is not None else {}
        outs = {"C": C}
        canon = {}
        if csplit:                                               # the split-row layout depends on ldc % 32: compare the decoded values
            canon["C"] = lambda t: _decode_split_rows(t, n)
        if split_a:
            outs["A split rows"] = At
            canon["A split rows"] = lambda t: _decode_split_rows(t, k)
        return built(call, outs, ref, canon, counters)
    return build


# (mode, r, k, n, lda+, ldc+, lif, c_split, aux offset of C / bias / lif4, kernel reached under guards, values beyond f16)
_G = [
    ("f32", 1, 32, 1, 0, 0, False, 0, 4, None, 0), ("f32", 129, 96, 33, 4, 3, False, 0, 4, None, 0), ("f32", 1025, 64, 260, 4, 0, True, 0, 16, None, 0),
    ("f32", 4099, 32, 3, 0, 5, False, 0, 4, None, 0), ("f32", 255, 960, 127, 4, 1, False, 0, 16, None, 0),
    ("sf16", 127, 64, 31, 4, 0, False, 0, 4, None, 0), ("sf16", 257, 960, 129, 4, 7, False, 0, 16, None, 0), ("sf16", 1023, 64, 640, 0, 0, True, 0, 16, None, 0),
    ("sf16", 1, 64, 3, 4, 1, True, 0, 4, None, 0), ("sf16", 128, 128, 128, 4, 32, False, 1, 16, None, 0), ("sf16", 300, 64, 33, 4, 3, False, 0, 4, None, 3),
    # ring kernel, float4 epilogue (what the models launch): smallest, full tile, ragged rows / columns, split-row output
    ("ring", 1, 32, 4, 8, 0, False, 0, 16, "ring-vec", 0), ("ring", 128, 64, 128, 8, 4, False, 0, 16, "ring-vec", 0),
    ("ring", 255, 96, 260, 32, 28, True, 1, 16, "ring-vec", 0), ("ring", 129, 960, 128, 32, 0, True, 0, 16, "ring-vec", 0),
    ("ring", 257, 64, 640, 8, 4, False, 0, 16, "ring-vec", 0), ("ring", 1025, 32, 132, 0, 28, True, 1, 16, "ring-vec", 0),
    # ring kernel, element-wise epilogue: odd n, odd ldc, or C / bias / lif4 at +4
    ("ring", 1, 32, 1, 8, 0, False, 0, 4, "ring-elem", 0), ("ring", 128, 64, 127, 8, 1, False, 0, 16, "ring-elem", 0),
    ("ring", 1025, 32, 33, 0, 31, True, 1, 16, "ring-elem", 0), ("ring", 257, 64, 640, 8, 4, True, 0, 4, "ring-elem", 0),
    # big-tile kernel (a_split_rows = 1, >= 1024 rows, n % 128 == 0): BN 128 and 256, bias / LIF, f32 / split-row output, ragged rows
    ("bt", 1024, 64, 128, 0, 0, False, 0, 16, "bt", 0), ("bt", 1025, 960, 640, 32, 4, True, 0, 16, "bt", 0), ("bt", 4099, 96, 256, 8, 32, True, 1, 16, "bt", 0),
    ("bt", 1281, 32, 256, 0, 0, False, 1, 16, "bt", 0), ("bt", 2049, 64, 128, 8, 4, True, 0, 16, "bt", 0),
    # the same entry (a_split_rows = 1) where the big tile does not take the shape or the alignment: falls to the ring kernel
    ("bt", 1023, 64, 128, 8, 0, False, 0, 16, "ring-vec", 0), ("bt", 1025, 64, 128, 8, 0, True, 0, 4, "ring-elem", 0),
]
for (_m, _r, _k, _n, _la, _lc, _lif, _cs, _aux, _exp, _hot) in _G:
    case("gemm-%s-r%d-k%d-n%d-lda+%d-ldc+%d-aux+%d%s%s%s%s" % (_m, _r, _k, _n, _la, _lc, _aux, "-lif" if _lif else "", "-csplit" if _cs else "",
                                                            "-reaches-" + _exp if _exp else "", "-overflow%d" % _hot if _hot else ""),
         ["sapcu_gemm_f32"] + (["sapcu_to_split_rows"] if _m in ("ring", "bt") else []))(
        _gemm_case(_m, _r, _k, _n, _la, _lc, _lif, _cs, in_x=3, aux=_aux, expect=_exp, hot=_hot))


def _to_split_case(rows, k, ld_in_x, ld_out_x):
    def build(A):
        _lib, lib = _lib_()
        a = np.random.default_rng(rows + k).normal(size=(rows, k)).astype(np.float32)
        Ain = A.inp(a, pitch=k + (0 if A.compact else ld_in_x), offset=4, name="in")
        ld_out = k + (0 if A.compact else ld_out_x)
        out = A.out((rows, ld_out), F32, offset=4, name="out")             # a split row owns its whole pitch

        def ref(o):
            got = _decode_split_rows(o["out"], k)                 # hi + lo reproduces an f32 to 2^-22 relative (two f16 halves)
            assert (got - torch.from_numpy(a)).abs().max().item() <= 2e-6 * np.abs(a).max()
        return built(lambda: ok(lib.sapcu_to_split_rows(P(Ain), rows, k, k + (0 if A.compact else ld_in_x), P(out), ld_out, S())),
                     {"out": out}, ref, {"out": lambda t: _decode_split_rows(t, k)})
    return build


for _rows, _k, _li, _lo in ((1, 32, 1, 0), (129, 96, 5, 32), (129, 32, 0, 8), (1, 96, 3, 3), (4099, 33, 2, 1)):
    case("to_split_rows-r%d-k%d-in+%d-out+%d" % (_rows, _k, _li, _lo), ["sapcu_to_split_rows"])(_to_split_case(_rows, _k, _li, _lo))


def _posenc_case(mode, b, m, kk, d):
    def build(A):
        _lib, lib = _lib_()
        rng = np.random.default_rng(b * 1000 + d)
        r = b * m * kk
        pe1 = rng.random((r, d)).astype(np.float32)
        w = (rng.normal(size=(d, d)) / np.sqrt(d)).astype(np.float32)
        bias = rng.normal(size=d).astype(np.float32)
        raw = _raw_lif(rng, d)
        qkv = rng.random((b * m, 3 * d)).astype(np.float32)
        idx = rng.integers(0, m, size=(b, m, kk)).astype(np.int32)
        split = {"f32": 0, "sf16": 0, "ring": 2, "bt": 1}[mode]
        W, Bv, L, Q, I = A.inp(w, offset=16, name="w"), A.inp(bias, offset=16, name="bias"), A.inp(raw, offset=16, name="lif4"), \
            A.inp(qkv, offset=16, name="qkv"), A.inp(idx, offset=4, name="idx")
        P1 = A.inp(pe1, offset=16, name="pe1")
        P1s = A.out((r, d), F32, offset=16, name="pe1 split rows") if split else None
        pe, att = A.out((r, d), F32, offset=16, name="pe"), A.out((r, d), F32, offset=16, name="attn_in")
        tab = A.ws(8 * r, offset=8, name="edge_table_ws")
        ws = None if mode == "f32" else A.ws(4 * d * d + 16, tile_row_bytes=4 * d, offset=16, name="w16_ws")

        def call():
            if split:
                ok(lib.sapcu_to_split_rows(P(P1), r, d, d, P(P1s), d, S()))
            ok(lib.sapcu_posenc_gemm_f32(P(P1s if split else P1), r, d, P(W), P(Bv), P(L), 4, P(Q), P(I), kk, m, P(pe), P(att), P(tab), P(ws), split, S()))

        def ref(o):
            pre = torch.from_numpy((pe1.astype(np.float64) @ w.astype(np.float64).T + bias).astype(np.float32))
            v = _oracle_lif(pre, raw, 4)
            pt = np.arange(r) // kk
            nbr = (pt // m) * m + idx.reshape(-1)
            want_att = torch.from_numpy(qkv[pt, :d] - qkv[nbr, d:2 * d]) + v
            got_att = _decode_split_rows(o["attn_in"], d) if split else o["attn_in"]
            assert (o["pe"] - v).abs().max().item() <= 2e-5
            assert (got_att - want_att).abs().max().item() <= 2e-5 + (2e-7 if split else 0.0)

        def counters():
            return {"w16_ws overflow": (int(ws[4 * d * d:4 * d * d + 4].clone().view(I32).item()), 0)} if ws is not None else {}
        return built(call, {"pe": pe, "attn_in": att}, ref, {"attn_in": (lambda t: _decode_split_rows(t, d))} if split else {}, counters)
    return build


for _mode, _b, _m, _kk, _d in (("f32", 1, 5, 4, 64), ("sf16", 1, 5, 4, 64), ("ring", 1, 5, 4, 64), ("f32", 3, 48, 24, 128), ("sf16", 3, 48, 24, 128),
                               ("ring", 3, 48, 24, 128), ("bt", 3, 48, 24, 128), ("bt", 37, 48, 12, 512), ("ring", 2, 100, 18, 256)):
    case("posenc-%s-b%d-m%d-kk%d-d%d" % (_mode, _b, _m, _kk, _d), ["sapcu_posenc_gemm_f32"])(_posenc_case(_mode, _b, _m, _kk, _d))


# ================================================================================================ fused edge chain
def _chain_operands(b, m, d, kk, seed):
    from oracle import snn_path as O
    rng = np.random.default_rng(seed)
    heads, T = 8, 4
    xyz = torch.from_numpy(rng.normal(0, 0.05, (b, m, 3)).astype(np.float32))
    idx = O.inpatch_knn(xyz.permute(0, 2, 1).contiguous(), kk)
    qkv = torch.from_numpy(rng.random((b * m, 3 * d)).astype(np.float32))

    def lin(n, k, gain):
        return (torch.from_numpy((rng.uniform(-1, 1, (n, k)) * gain / np.sqrt(k)).astype(np.float32)), torch.from_numpy(rng.normal(0.6, 0.4, n).astype(np.float32)))

    def lif():
        return torch.from_numpy(np.stack([rng.uniform(0.05, 1.1, d), rng.uniform(0.0, 0.2, d), rng.uniform(0.05, 1.0, d), rng.normal(0.8, 0.3, d)]).astype(np.float32))
    wd, bd = lin(d, 3, 20.0)
    w1, b1 = lin(d, d, 2.0)
    w2, b2 = lin(d, d, 2.0)
    w3, b3 = lin(d, d, 4.0)
    return xyz, idx, qkv, (wd, bd, lif(), w1, b1, lif(), w2, b2, lif(), w3, b3), heads, T


def _chain_want(b, m, d, xyz, idx, qkv, prm, heads, T):
    """The oracle primitives in the reference's own tensor shapes (test_fused_edge_chain_entry_against_the_oracle_primitives)."""
    from oracle import snn_path as O
    wd, bd, ld, w1, b1, l1, w2, b2, l2, w3, b3 = prm

    def npar(l):
        return {"decay": torch.clamp(l[0], 0.1, 0.99), "adapt": torch.clamp(l[1], 0.001, 0.1), "rdecay": torch.clamp(l[2], 0.1, 0.95), "theta0": l[3]}

    def conv(x, w, bias):
        return torch.nn.functional.conv2d(x, w[:, :, None, None], bias)
    with torch.no_grad():
        pos = xyz.permute(0, 2, 1)
        pos_diff = (pos.unsqueeze(-1) - O.gather_cols(pos, idx)).contiguous()
        q = qkv[:, :d].view(b, m, d).permute(0, 2, 1)
        kf = qkv[:, d:2 * d].view(b, m, d).permute(0, 2, 1).contiguous()
        v = qkv[:, 2 * d:].view(b, m, d).permute(0, 2, 1).contiguous()
        pe = O.neuron_selfloop(conv(pos_diff, wd, bd), npar(ld), T)
        pe = O.neuron_selfloop(conv(pe, w1, b1), npar(l1), T)
        a = q.unsqueeze(-1) - O.gather_cols(kf, idx) + pe
        a = O.neuron_selfloop(conv(a, w2, b2), npar(l2), T)
        a = torch.softmax(conv(a, w3, b3) / np.sqrt(d // heads), dim=-1)
        return torch.einsum("bcnk,bcnk->bcn", a, O.gather_cols(v, idx) + pe).permute(0, 2, 1).reshape(b * m, d)


def _chain_case(b, m, d, kk, ws_off=0):
    def build(A):
        _lib, lib = _lib_()
        xyz, idx, qkv, prm, heads, T = _chain_operands(b, m, d, kk, d + kk + b)
        Pn = b * m
        need = lib.sapcu_fn_edge_chain_workspace_bytes(Pn, d, kk)
        assert need > 0
        ins = [A.inp(xyz.reshape(Pn, 3), offset=16, name="patch"), A.inp(idx.reshape(-1).to(I32), offset=16, name="idx"), A.inp(qkv, offset=16, name="qkv")]
        ins += [A.inp(t, offset=16, name="param%d" % i) for i, t in enumerate(prm)]
        res = A.out((Pn, d), F32, offset=16, name="res")
        ws = A.ws(need, offset=ws_off, tile_row_bytes=16 * kk, name="chain workspace")

        def call():
            ok(lib.sapcu_fn_edge_chain_f32(P(ins[0]), P(ins[1]), Pn, m, d, kk, *[P(t) for t in ins[2:]], heads, T, P(res), P(ws), need, S()))

        def ref(o):
            want = _chain_want(b, m, d, xyz, idx, qkv, prm, heads, T)
            err = (o["res"] - want).abs().max().item()
            assert err <= 2e-5 * max(1.0, float(want.abs().max())), err

        def counters():                                          # model.hip sapcu_fn_edge_chain_f32: base rounded up to 256; table | records | 3 x (hi|lo|counter, packed)
            up = lambda x: (x + 255) & ~255
            base = (-ws.data_ptr()) % 256 + up(Pn * kk * 8) + up(Pn * kk * 16)
            out = {}
            for q in range(3):
                at = base + q * (up(d * d * 4 + 16) + up(d * d * 4)) + 4 * d * d
                assert at + 4 <= need
                out["split weights %d overflow" % q] = (int(ws[at:at + 4].clone().view(I32).item()), 0)
            return out
        return built(call, {"res": res}, ref, None, counters)
    return build


# points per group: 4 (d=128, kk=24), 7 (256, 18), 5 (512, 12): patches x m_pts chosen so that the last group is ragged
for _b, _m, _d, _kk in ((1, 48, 128, 24), (5, 48, 128, 24), (7, 100, 128, 24), (1, 48, 256, 18), (5, 48, 256, 18), (7, 100, 256, 18),
                        (1, 48, 512, 12), (7, 48, 512, 12), (5, 100, 512, 12), (37, 48, 512, 12)):
    # (the workspace's base at +16 where b is odd: the sizer's 256 bytes of slack are then really used by the rounding inside)
    case("edge_chain-b%d-m%d-d%d-kk%d-ws+%d" % (_b, _m, _d, _kk, 16 * (_b % 2 if _b > 1 else 0)), ["sapcu_fn_edge_chain_f32"],
         ["sapcu_fn_edge_chain_workspace_bytes"])(_chain_case(_b, _m, _d, _kk, 16 * (_b % 2 if _b > 1 else 0)))


# ================================================================================================ model forwards
_MODELS = {}


def _models(env_key):
    """(fn, fd, sdn, sdd) whose handles were created under the switches of env_key (read once, at sapcu_model_create)."""
    if env_key not in _MODELS:
        import os
        from conftest import FD_KW, FN_KW, golden
        import sapcu_amd
        from sapcu_amd import testing as T
        fn = sapcu_amd.ImprovedSNNNormalEstimation(**FN_KW)
        fd = sapcu_amd.EnhancedSNNDistanceEstimation(**FD_KW)
        sdn = T.conditioned_state_dict(fn.state_dict(), 0, bn_stats=dict(golden("bn_calib_fn.npz")))
        sdd = T.conditioned_state_dict(fd.state_dict(), 0, bn_stats=dict(golden("bn_calib_fd.npz")))
        fn.load_state_dict(sdn, strict=True)
        fd.load_state_dict(sdd, strict=True)
        fn, fd = fn.to(U.dev()), fd.to(U.dev())
        old = {k: os.environ.get(k) for k, _ in env_key}
        try:
            for k, v in env_key:
                os.environ[k] = v
            fn._engine(), fd._engine()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        fn.knn_cache_mode = "fresh"
        _MODELS[env_key] = (fn, fd, sdn, sdd)
    return _MODELS[env_key]


def _row_model(rid):
    """(model, state dict, oracle hp) of a row of tests/golden/hparams.npz — a handle away from the default hyper-parameters, created
    under the default environment."""
    if rid not in _MODELS:
        from conftest import golden
        row = U.hparam_row(golden("hparams.npz"), rid)
        _MODELS[rid] = U.build_gpu_hparam_model(row) + (row["hp"],)
    return _MODELS[rid]


def _fn_case(env_key, b, m, taps, row=None):
    def build(A):
        _lib, lib = _lib_()
        fn, sdn, hp = _row_model(row) if row else (_models(env_key)[0], _models(env_key)[2], U.FN_HP)
        h = fn._engine()
        patch = U.sphere_patches(b, m, skip=3)
        X = A.inp(patch, offset=4, name="patch")
        ks = [min(k, m) for k in fn.k_values]
        need = int(lib.sapcu_workspace_bytes(h, b, m))
        assert need > 0
        ws = A.ws(need, offset=16 if taps else 0, tile_row_bytes=4 * 960, name="fn workspace")   # +16: the sizer's slack for the rounding inside is used
        outs = {"normals": A.out((b, 3), F32, offset=4, name="normals"), "knn_out": A.out((b * m * sum(ks),), I32, offset=4, name="knn_out")}
        arr = None
        if taps:
            shp = {"stem": (b, m, 64), "block1": (b, m, 64), "block2": (b, m, 64), "block3": (b, m, 64), "pooled": (b, fn.emb_dims), "enc": (b, 2048), "logits": (b, 3)}
            arr = (ctypes.c_void_p * len(_lib.FN_TAPS))()
            for i, nme in enumerate(_lib.FN_TAPS):
                outs["tap " + nme] = A.out(shp[nme], F32, offset=4, name="tap " + nme)
                arr[i] = outs["tap " + nme].data_ptr()

        def call():
            ok(lib.sapcu_fn_forward(h, P(X), b, m, None, P(outs["knn_out"]), P(outs["normals"]), P(ws), need, arr, S()))
            torch.cuda.synchronize()
            assert fn.gemm_mode() == (True, 0)

        def ref(o):
            from oracle import snn_path as O
            assert torch.equal(fn(patch.to(U.dev())).cpu(), o["normals"])           # the module's own call
            with torch.no_grad():
                n_ref = torch.nn.functional.normalize(O.fn_forward(sdn, patch, hp), dim=-1)
            err = (torch.nn.functional.normalize(o["normals"], dim=-1) - n_ref).abs().max().item()
            assert err <= 1e-4, err
        return built(call, outs, ref)
    return build


def _fd_case(env_key, b, m, taps, row=None):
    def build(A):
        _lib, lib = _lib_()
        fd, sdd, hp = _row_model(row) if row else (_models(env_key)[1], _models(env_key)[3], U.FD_HP)
        h = fd._engine()
        patch = U.sphere_patches(b, m, skip=5)
        X = A.inp(patch, offset=4, name="patch")
        need = int(lib.sapcu_workspace_bytes(h, b, m))
        assert need > 0
        ws = A.ws(need, offset=16 if taps else 0, tile_row_bytes=4 * 960, name="fd workspace")
        kk, T, emb = min(fd.k, m), fd.time_steps_enc, fd.emb_dims
        outs = {"dist": A.out((b,), F32, offset=4, name="dist")}
        shp = {"fused0": ((b, m, 64), F32), "spikes": ((T, b, m, 960), F32), "knn": ((3, b, m, kk), I32), "pooled": ((T, b, emb), F32),
               "enc": ((b, emb), F32), "x0": ((b, m, 960), F32)}
        arr = (ctypes.c_void_p * len(_lib.FD_TAPS))()
        for i, nme in enumerate(_lib.FD_TAPS):
            if taps or nme == "knn":                                               # the neighbour tables feed the forced-neighbour reference
                outs["tap " + nme] = A.out(shp[nme][0], shp[nme][1], offset=4, name="tap " + nme)
                arr[i] = outs["tap " + nme].data_ptr()

        def call():
            ok(lib.sapcu_fd_forward(h, P(X), b, m, None, P(outs["dist"]), P(ws), need, arr, S()))
            torch.cuda.synchronize()
            assert fd.gate_violations() == 0 and fd.gemm_mode() == (True, 0)

        def ref(o):
            from oracle import snn_path as O
            assert torch.equal(fd(patch.to(U.dev())).cpu(), o["dist"])
            knn = o["tap knn"].long()
            with torch.no_grad():
                d_forced = O.fd_forward(sdd, patch, hp, force_idx=[knn[0], knn[1], knn[2]])
            err = (o["dist"] - d_forced).abs().max().item()
            assert err <= 1e-4, err
        return built(call, outs, ref)
    return build


_ENVS = {"default": (), "chunk7": (("SAPCU_CHUNK", "7"),), "chain0": (("SAPCU_CHAIN", "0"),), "fdmaxfuse0": (("SAPCU_FD_MAXFUSE", "0"),)}
for _env, _b, _m, _taps in (("default", 1, 5, True), ("default", 7, 48, True), ("default", 64, 48, False), ("default", 7, 12, False), ("default", 1, 20, True),
                            ("default", 7, 100, True), ("default", 1, 128, False), ("chunk7", 64, 48, True), ("chunk7", 7, 100, False),
                            ("chain0", 7, 48, True), ("chain0", 1, 100, False), ("fdmaxfuse0", 7, 48, True), ("fdmaxfuse0", 1, 128, True)):
    _tag = "%s-b%d-m%d-%s" % (_env, _b, _m, "taps" if _taps else "notaps")
    case("fn_forward-" + _tag, ["sapcu_fn_forward"], ["sapcu_workspace_bytes"])(_fn_case(_ENVS[_env], _b, _m, _taps))
    case("fd_forward-" + _tag, ["sapcu_fd_forward"], ["sapcu_workspace_bytes"])(_fd_case(_ENVS[_env], _b, _m, _taps))

# handles away from the default hyper-parameters (rows of tests/golden/hparams.npz): the all-unfused fn plan at kk = 20 / 16 and emb 1024,
# fd with three scales (NS = 3) at k = 20, T = 5, and with five scales (fd_edge0_patch_kernel, the x0 path at 48 points)
for _row, _b, _m in (("fn-ctor", 3, 48), ("fd-ctor", 3, 48), ("fd-ctor", 2, 100), ("fd-s5", 3, 48)):
    _kind = _row.split("-")[0]
    case("%s_forward-%s-b%d-m%d-taps" % (_kind, _row, _b, _m), ["sapcu_%s_forward" % _kind], ["sapcu_workspace_bytes"])(
        (_fn_case if _kind == "fn" else _fd_case)((), _b, _m, True, row=_row))

# ================================================================================================ in-patch kNN, geometry
def _patch_knn_case(b, m, c, ld_x, k):
    def build(A):
        from oracle import snn_path as O
        _lib, lib = _lib_()
        rng = np.random.default_rng(m * 100 + c + k)
        # integer-valued coordinates: every score is exact in f32 whatever the summation order, so the ranking has one answer
        pts = rng.integers(-8, 9, size=(b, m, c)).astype(np.float32)
        ld = c + (0 if A.compact else ld_x)
        F = A.inp(pts, pitch=ld, offset=4, name="feat")
        out = A.out((b, m, k), I32, offset=4, name="idx_out")

        def ref(o):
            sc = O.inpatch_knn_scores(torch.from_numpy(np.ascontiguousarray(pts.transpose(0, 2, 1)))).numpy()
            want = np.argsort(-sc, axis=-1, kind="stable")[..., :k]
            assert np.array_equal(o["idx_out"].numpy().astype(np.int64), want)
        return built(lambda: ok(lib.sapcu_patch_knn(P(F), b, m, c, ld, k, P(out), S())), {"idx_out": out}, ref)
    return build


for _b, _m, _c, _ldx, _k in ((3, 5, 3, 0, 1), (3, 5, 3, 1, 5), (2, 48, 64, 128, 1), (2, 48, 64, 0, 48), (3, 100, 256, 3, 100), (1, 100, 3, 189, 1),
                             (2, 48, 256, 512, 24), (1, 128, 64, 1, 128)):
    case("patch_knn-b%d-m%d-c%d-ld+%d-k%d" % (_b, _m, _c, _ldx, _k), ["sapcu_patch_knn"])(_patch_knn_case(_b, _m, _c, _ldx, _k))


def _geom_cloud(n, b, seed):
    rng = np.random.default_rng(seed)
    cloud = np.round(rng.uniform(-0.5, 0.5, (n, 3)), 6)
    q = np.round(rng.uniform(-0.5, 0.5, (b, 3)), 6)
    if n > 2:
        cloud[n // 2] = cloud[0]
        q[0] = cloud[n - 1]
    return cloud, q


def _knn_gather_case(n, b, k, opt):
    def build(A):
        from oracle import geom_path as G
        _lib, lib = _lib_()
        cloud, q = _geom_cloud(n, b, n * 1000 + b)
        Cl, Q = A.inp(cloud, offset=8, name="cloud"), A.inp(q, offset=8, name="queries")
        outs = {"idx": A.out((b, k), I64, offset=8, name="idx_out")}
        if opt:
            outs["dist"] = A.out((b, k), F64, offset=8, name="dist_out")
            outs["patch"] = A.out((b, k, 3), F32, offset=4, name="patch_out")

        def ref(o):
            want = G.knn_bruteforce(cloud, q, k)
            assert np.array_equal(o["idx"].numpy(), want)
            if opt:
                assert (np.diff(o["dist"].numpy(), axis=1) >= 0).all()
                assert np.array_equal(o["patch"].numpy(), G.gather_centre(cloud, q, want).astype(np.float32))
        return built(lambda: ok(lib.sapcu_knn_gather_f64(P(Cl), n, P(Q), b, k, P(outs["idx"]), P(outs.get("dist")), P(outs.get("patch")), S())), outs, ref)
    return build


for _n, _b, _k, _opt in ((1, 1, 1, True), (1, 130, 1, False), (1024, 1, 64, True), (1024, 130, 128, False), (1025, 130, 128, True), (1025, 1, 1, True),
                         (1025, 130, 64, False)):
    case("knn_gather-n%d-b%d-k%d-%s" % (_n, _b, _k, "all" if _opt else "idx"), ["sapcu_knn_gather_f64"])(_knn_gather_case(_n, _b, _k, _opt))


def _rotate_case(n, b, k, with_normals):
    def build(A):
        from oracle import geom_path as G
        _lib, lib = _lib_()
        cloud, q = _geom_cloud(n, b, n + b + k)
        idx = G.knn_bruteforce(cloud, q, k)
        rng = np.random.default_rng(b)
        nrm = rng.normal(size=(b, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
        dist = rng.uniform(0, 0.05, b).astype(np.float32)
        Cl, Q, I, N, D = A.inp(cloud, offset=8, name="cloud"), A.inp(q, offset=8, name="queries"), A.inp(idx, offset=8, name="idx"), \
            A.inp(nrm, offset=4, name="normals"), A.inp(dist, offset=4, name="dist")
        outs = {"patch": A.out((b, k, 3), F32, offset=4, name="patch_out"), "disp": A.out((b, 3), F64, offset=8, name="displaced"),
                "unit": A.out((b, 3), F32, offset=4, name="normalized")}
        raw = (nrm * rng.uniform(0.5, 3.0, (b, 1))).astype(np.float32)
        raw[0] = 0.0                                                   # the 1e-12 floor of F.normalize
        R = A.inp(raw, offset=4, name="raw normals")

        def call():
            ok(lib.sapcu_gather_rotate_f64(P(Cl), n, P(Q), b, P(I), k, P(N) if with_normals else None, P(outs["patch"]), S()))
            ok(lib.sapcu_displace_f64(P(Q), P(N), P(D), b, P(outs["disp"]), S()))
            ok(lib.sapcu_l2_normalize3(P(R), P(outs["unit"]), b, S()))

        def ref(o):
            centred = G.gather_centre(cloud, q, idx)
            if with_normals:
                want = G.rotate_patches(centred, nrm).astype(np.float32)
                got = o["patch"].numpy()
                assert int((got != want).sum()) <= max(2, got.size // 4096)          # last-ulp cases of test_rotation_and_displacement_exact (2 of 9216)
                np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
            else:
                assert np.array_equal(o["patch"].numpy(), centred.astype(np.float32))
            assert np.array_equal(o["disp"].numpy(), G.displace(q, nrm, dist))
            want_u = torch.nn.functional.normalize(torch.from_numpy(raw), dim=-1)
            assert (o["unit"] - want_u).abs().max().item() <= 1e-6
        return built(call, outs, ref)
    return build


for _n, _b, _k, _wn in ((1, 1, 1, True), (1024, 130, 64, True), (1025, 130, 128, False), (1025, 1, 48, True)):
    case("rotate_displace_normalize-n%d-b%d-k%d-%s" % (_n, _b, _k, "rot" if _wn else "plain"),
         ["sapcu_gather_rotate_f64", "sapcu_displace_f64", "sapcu_l2_normalize3"])(_rotate_case(_n, _b, _k, _wn))


# ================================================================================================ grid kNN + outlier statistics
def _grid_case(n, row0, row1, k, cell, nonfinite):
    def build(A):
        from oracle import geom_path as G
        from sapcu_amd import generation as gen
        _lib, lib = _lib_()
        rng = np.random.default_rng(n + k)
        pts = np.round(rng.uniform(-0.5, 0.5, (n, 3)), 6)
        if n > 2:
            pts[n // 2] = pts[0]
        if nonfinite:
            pts[n - 1, 1] = np.inf                                     # -> the brute-force kernel
        rows = row1 - row0
        X = A.inp(pts, offset=8, name="pts")
        need = int(lib.sapcu_knn_grid_workspace_bytes(n))
        assert need >= 0
        ws = A.ws(need, offset=8 if k == 30 else 0, name="grid workspace")           # 8 bytes: exactly what the header asks
        bufsize = 8192
        nchunk = gen.outlier_chunk_count(rows, k, bufsize) if rows else 0
        outs = {"idx": A.out((rows, k), I64, offset=8, name="idx_out"), "dist": A.out((rows, k), F64, offset=8, name="dist_out"),
                "row_mean": A.out((rows,), F64, offset=8, name="row_mean"), "chunk_sum": A.out((nchunk,), F64, offset=8, name="chunk_sum"),
                "keep": A.out((rows,), U8, offset=1, name="keep")}
        info = (ctypes.c_int64 * 4)()

        def call():
            ok(lib.sapcu_knn_self_grid_f64(P(X), n, row0, row1, k, cell, P(outs["idx"]) if rows else None, P(outs["dist"]) if rows else None,
                                           P(ws), need, info, S()))
            if rows:                                                    # an empty range launches nothing (and reports no grid)
                assert info[0] == (0 if nonfinite or (n < 4096 and cell == 0) else 1)
            ok(lib.sapcu_outlier_stats_f64(P(outs["dist"]), rows, k, bufsize, P(outs["row_mean"]), P(outs["chunk_sum"]), S()))
            ok(lib.sapcu_outlier_keep_f64(P(outs["row_mean"]), rows, 0.25, 1.1, P(outs["keep"]), S()))

        def ref(o):
            if not rows:
                return
            dist = o["dist"].numpy()
            if not nonfinite or row1 < n:                       # the non-finite point is not a query of this row range and is nobody's neighbour
                with np.errstate(all="ignore"):
                    want = G.knn_bruteforce(pts, pts[row0:row1], k)
                assert np.array_equal(o["idx"].numpy(), want)
                d2 = ((pts[row0:row1, None, :] - pts[want]) ** 2)
                assert np.array_equal(dist, np.sqrt((d2[..., 0] + d2[..., 1]) + d2[..., 2]))
                assert nonfinite is False or (np.isfinite(dist).all() and not (o["idx"].numpy() == n - 1).any())
            old = np.getbufsize()
            np.setbufsize(bufsize)
            try:
                assert np.array_equal(o["row_mean"].numpy(), np.mean(dist, axis=1), equal_nan=True)
                flat = dist.reshape(-1)
                sums = np.array([np.add.reduce(flat[i:i + bufsize]) for i in range(0, flat.size, bufsize)])
                assert np.array_equal(o["chunk_sum"].numpy(), sums, equal_nan=True)
            finally:
                np.setbufsize(old)
            assert np.array_equal(o["keep"].numpy().astype(bool), o["row_mean"].numpy() < 0.25 * 1.1)
        return built(call, outs, ref)
    return build


for _n, _r0, _r1, _k, _cell, _nf in ((1, 0, 1, 1, 0.0, False), (31, 0, 31, 30, 0.0, False), (31, 7, 7, 30, 0.05, False), (5000, 0, 5000, 30, 0.0, False),
                                     (5000, 4999, 5000, 64, 0.0, False), (12289, 12288, 12289, 30, 0.0, False), (12289, 8192, 12289, 30, 0.0, False),
                                     (5000, 1024, 2048, 30, 0.0, True), (31, 0, 31, 5, 0.2, False), (12289, 0, 0, 30, 0.0, False)):
    case("grid_knn-n%d-rows%d:%d-k%d-cell%g%s" % (_n, _r0, _r1, _k, _cell, "-nonfinite" if _nf else ""),
         ["sapcu_knn_self_grid_f64", "sapcu_outlier_stats_f64", "sapcu_outlier_keep_f64"], ["sapcu_knn_grid_workspace_bytes"])(_grid_case(_n, _r0, _r1, _k, _cell, _nf))


# ================================================================================================ farthest-point sampling
def _fps_case(n, npoint):
    def build(A):
        _lib, lib = _lib_()
        cloud = (np.random.default_rng(n).standard_normal((n, 3)) * np.array([2.0, 1.0, 0.5])).astype(np.float32)
        X = A.inp(cloud, offset=4, name="xyz")
        need = int(lib.sapcu_fps_workspace_bytes(npoint))
        assert need > 0
        ws = A.ws(need, offset=8 if npoint > 1 else 0, name="fps workspace")            # 8 bytes: exactly what the header asks
        out = A.out((npoint,), I64, offset=8, name="idx_out")
        xp, op = P(X), (P(out) if npoint else ctypes.c_void_p(A.inp(np.zeros(1, np.int64), name="unused idx_out").data_ptr()))

        def ref(o):
            from oracle import fps_path as Fp
            assert np.array_equal(o["idx"].numpy(), Fp.farthest_point_sample(cloud.astype(np.float64), npoint))
        return built(lambda: ok(lib.sapcu_fps_f32(xp, n, npoint, op, P(ws), need, S())), {"idx": out}, ref)
    return build


for _n, _np in ((1, 1), (255, 17), (255, 255), (256, 0), (256, 1), (257, 257), (65537, 300), (65537, 1)):
    case("fps-n%d-npoint%d" % (_n, _np), ["sapcu_fps_f32"], ["sapcu_fps_workspace_bytes"])(_fps_case(_n, _np))


# ================================================================================================ neuron unit
def _neuron_case(rows, ch, T, eif, pairv, optional):
    def build(A):
        from oracle import snn_path as O
        _lib, lib = _lib_()
        rng = np.random.default_rng(rows * 10 + ch + T)
        x = rng.normal(0.5, 1.5, (rows, ch)).astype(np.float32)
        raw = np.stack([rng.uniform(0.05, 1.1, ch), rng.uniform(0.0, 0.2, ch), rng.uniform(0.05, 1.0, ch), rng.normal(0.5, 0.3, ch),
                        rng.uniform(0.2, 1.0, ch), rng.normal(0.3, 0.2, ch)]).astype(np.float32)
        X = A.inp(x, offset=4, name="x")
        Rw = [A.inp(raw[i], offset=4, name="param%d" % i) for i in range(6)]
        dT, rh = (Rw[4], Rw[5]) if eif else (None, None)
        self_names, drive_names = ("spikes", "membrane", "threshold", "refractory"), ("membrane", "threshold", "refractory")
        outs = {"self " + nme: A.out((rows, ch), F32, offset=4, name="selfloop " + nme) for nme in self_names if optional or nme == "spikes"}
        outs["drive spikes"] = A.out((T, rows, ch), F32, offset=4, name="drive spikes")
        for nme in drive_names:
            if optional:
                outs["drive " + nme] = A.out((rows, ch), F32, offset=4, name="drive " + nme)
        gate = A.inp(np.full(1, -1, np.int32), offset=4, name="gate counter")          # the caller zeroes it (sapcu.h)

        def call():
            ok(lib.sapcu_neuron_selfloop(P(X), rows, ch, T, *[P(t) for t in Rw[:4]], P(dT), P(rh), *[P(outs.get("self " + nme)) for nme in self_names], S()))
            gate.zero_()
            ok(lib.sapcu_neuron_drive(P(X), rows, ch, T, *[P(t) for t in Rw[:4]], P(dT), P(rh), pairv, P(outs["drive spikes"]),
                                      *[P(outs.get("drive " + nme)) for nme in drive_names], P(gate), S()))
            torch.cuda.synchronize()
            assert int(gate.item()) == 0

        def ref(o):
            from oracle import snn_path as O
            names = ["membrane_decay", "threshold_adapt", "refractory_decay", "threshold_base", "delta_T", "theta_rh"]
            prm = O.neuron_params({"n." + names[i]: torch.from_numpy(raw[i]) for i in range(6 if eif else 4)}, "n")
            xt = torch.from_numpy(x)
            # tolerances of test_neuron_unit_against_reference_vectors / test_neuron_stepping_form_far_outside_the_spike_clamp
            def close(name, want, atol=1e-6):
                if name in o:
                    np.testing.assert_allclose(o[name].numpy(), want.numpy(), rtol=2e-5, atol=atol, err_msg=name)
            v, st = xt, None                                     # self-loop: the spikes are the next step's input
            for _ in range(T):
                v, st = O.neuron_step(v, st, prm)
            close("self spikes", v)
            close("self membrane", st[0])
            close("self threshold", st[1])
            close("self refractory", st[2])
            st, spikes = None, []                                # stepping form: x at every step, closed by the refractory gate from step 1 on
            for _ in range(T):
                sp, st = O.neuron_step(xt, st, prm)
                spikes.append(sp)
            close("drive spikes", torch.stack(spikes))
            close("drive membrane", st[0], 5e-5 if eif else 1e-6)
            close("drive threshold", st[1])
            close("drive refractory", st[2])
        return built(call, outs, ref)
    return build


for _rows, _ch, _T, _eif, _pv, _opt in ((1, 1, 1, False, 0, True), (1, 1, 1, False, 1, False), (2, 3, 2, True, 0, True), (2, 3, 2, False, 1, True),
                                        (257, 64, 4, False, 0, False), (257, 64, 4, True, 1, True), (257, 65, 4, False, 1, True), (257, 65, 1, False, 0, True),
                                        (1, 65, 2, True, 1, False), (2, 64, 4, False, 1, False)):
    case("neuron-r%d-c%d-T%d-%s-pairv%d-%s" % (_rows, _ch, _T, "eif" if _eif else "lif", _pv, "all" if _opt else "spikes"),
         ["sapcu_neuron_selfloop", "sapcu_neuron_drive"])(_neuron_case(_rows, _ch, _T, _eif, _pv, _opt))


# ================================================================================================ training ops
def _lif_train_case(rows, ch, steps):
    def build(A):
        from oracle import train_path as TP
        _lib, lib = _lib_()
        rng = np.random.default_rng(rows + ch + steps)
        x = rng.normal(0.6, 1.0, (rows, ch)).astype(np.float32)
        g = rng.normal(0.0, 1.0, (rows, ch)).astype(np.float32)
        raw = np.stack([rng.uniform(0.05, 1.1, ch), rng.uniform(-0.02, 0.15, ch), rng.uniform(0.05, 1.0, ch), rng.normal(0.7, 0.4, ch)]).astype(np.float32)
        X, Gt = A.inp(x, offset=4, name="x"), A.inp(g, offset=4, name="grad_spikes")
        Rw = [A.inp(raw[i], offset=4, name="param%d" % i) for i in range(4)]
        need = int(lib.sapcu_lif_train_workspace_bytes(rows, ch))
        assert need > 0
        ws = A.ws(need, offset=16 if steps == 8 else 0, tile_row_bytes=4 * ch, name="lif_train workspace")
        outs = {"spikes": A.out((rows, ch), F32, offset=4, name="spikes_out"), "gx": A.out((rows, ch), F32, offset=4, name="grad_x")}
        for i in range(4):
            outs["gp%d" % i] = A.out((ch,), F32, offset=4, name="grad_param%d" % i)

        def call():
            ok(lib.sapcu_lif_train_forward(P(X), rows, ch, steps, *[P(t) for t in Rw], P(outs["spikes"]), S()))
            ok(lib.sapcu_lif_train_backward(P(X), P(Gt), rows, ch, steps, *[P(t) for t in Rw], P(outs["gx"]), *[P(outs["gp%d" % i]) for i in range(4)],
                                            P(ws), need, S()))

        def ref(o):
            xo = torch.from_numpy(x).requires_grad_(True)
            ro = [torch.from_numpy(raw[i]).requires_grad_(True) for i in range(4)]
            oo = TP.lif_selfloop_train(xo, *ro, steps=steps)
            (oo * torch.from_numpy(g)).sum().backward()
            assert torch.equal(o["spikes"], oo.detach())
            np.testing.assert_allclose(o["gx"].numpy(), xo.grad.numpy(), rtol=2e-5, atol=1e-6)
            for i, prm in enumerate(ro):
                want = prm.grad if prm.grad is not None else torch.zeros(ch)     # one step: decay / adapt / rdecay take no part
                scale = float(want.abs().max()) + 1e-6
                assert float((o["gp%d" % i] - want).abs().max()) <= 2e-4 * scale + 1e-4
        return built(call, outs, ref)
    return build


for _rows, _ch, _st in ((1, 3, 1), (257, 33, 8), (4099, 128, 1), (257, 128, 8), (1, 33, 8), (4099, 3, 4)):
    case("lif_train-r%d-c%d-T%d" % (_rows, _ch, _st), ["sapcu_lif_train_forward", "sapcu_lif_train_backward"],
         ["sapcu_lif_train_workspace_bytes"])(_lif_train_case(_rows, _ch, _st))


def _bn_wgrad_case(rows, n, k, ldy_x, ldx_x, bf16):
    def build(A):
        _lib, lib = _lib_()
        rng = np.random.default_rng(rows + n + k)
        y = rng.normal(0.3, 1.2, (rows, n)).astype(np.float32)
        gz = rng.normal(0, 1, (rows, n)).astype(np.float32)
        x = rng.normal(0, 1, (rows, k)).astype(np.float32)
        w = (rng.normal(size=(n, k)) / np.sqrt(k)).astype(np.float32)
        gamma, beta, bias = rng.uniform(0.5, 1.5, n).astype(np.float32), rng.normal(0.4, 0.5, n).astype(np.float32), rng.normal(size=n).astype(np.float32)
        eps = 1e-5
        ldy, ldx = n + (0 if A.compact else ldy_x), k + (0 if A.compact else ldx_x)
        Y, GZ, Ga, Be = A.inp(y, offset=4, name="y"), A.inp(gz, offset=4, name="grad_z"), A.inp(gamma, offset=4, name="gamma"), A.inp(beta, offset=4, name="beta")
        GYp, Xp = A.inp(gz, pitch=ldy, offset=16, name="grad_y pitched"), A.inp(x, pitch=ldx, offset=16, name="x pitched")
        GYc = A.inp(gz, offset=4, name="grad_y compact")
        Wt, Bi = A.inp(w, offset=16, name="w"), A.inp(bias, offset=4, name="bias")
        need0, need = int(lib.sapcu_train_workspace_bytes(rows, n, 0)), int(lib.sapcu_train_workspace_bytes(rows, n, k))
        needb = int(lib.sapcu_wgrad_bf16_workspace_bytes(rows, n, k))
        assert need0 > 0 and need > 0 and needb >= 0
        wo = 16 if rows == 257 else 0
        ws0, ws1, wsb = A.ws(need0, offset=wo, tile_row_bytes=8 * n, name="bn workspace"), A.ws(need, offset=wo, tile_row_bytes=8 * n, name="wgrad workspace"), \
            A.ws(max(needb, 1), offset=wo, tile_row_bytes=8 * n, name="wgrad bf16 workspace")
        o = {nme: A.out((n,), F32, offset=4, name=nme) for nme in ("mean", "var", "invstd", "grad_gamma", "grad_beta", "grad_bias")}
        o["z"], o["grad_y"] = A.out((rows, n), F32, offset=4, name="z_out"), A.out((rows, n), F32, offset=4, name="grad_y out")
        o["grad_w"], o["grad_w nobias"] = A.out((n, k), F32, offset=4, name="grad_w"), A.out((n, k), F32, offset=4, name="grad_w nobias")
        k4 = k % 4 == 0
        if bf16:
            o["grad_w bf16"], o["grad_bias bf16"] = A.out((n, k), F32, offset=4, name="grad_w bf16"), A.out((n,), F32, offset=4, name="grad_bias bf16")
            if k4:
                o["c bf16"] = A.out((rows, n), F32, pitch=ldy, offset=4, name="c bf16")
                Xq = A.inp(x, pitch=k + (0 if A.compact else 4 * ((ldx_x + 3) // 4)), offset=16, name="x pitched % 4")

        def call():
            ok(lib.sapcu_bn_train_forward(P(Y), rows, n, P(Ga), P(Be), eps, P(o["z"]), P(o["mean"]), P(o["var"]), P(o["invstd"]), P(ws0), need0, S()))
            ok(lib.sapcu_bn_train_backward(P(Y), P(GZ), rows, n, P(Ga), P(o["mean"]), P(o["invstd"]), P(o["grad_y"]), P(o["grad_gamma"]), P(o["grad_beta"]),
                                           P(ws0), need0, S()))
            ok(lib.sapcu_conv1x1_wgrad_f32(P(GYc), n, P(Xp), ldx, rows, n, k, P(o["grad_w"]), P(o["grad_bias"]), P(ws1), need, S()))   # bias gradient: ldy == n
            ok(lib.sapcu_conv1x1_wgrad_f32(P(GYp), ldy, P(Xp), ldx, rows, n, k, P(o["grad_w nobias"]), None, P(ws1), need, S()))
            if bf16:
                ok(lib.sapcu_conv1x1_wgrad_bf16(P(GYc), n, P(Xp), ldx, rows, n, k, P(o["grad_w bf16"]), P(o["grad_bias bf16"]), P(wsb), needb, S()))
                if k4:
                    ok(lib.sapcu_gemm_bf16(P(Xq), rows, k, Xq.stride(0) if rows > 1 else k, P(Wt), n, P(Bi), P(o["c bf16"]), ldy, S()))

        def ref(r):
            y64, g64, x64 = y.astype(np.float64), gz.astype(np.float64), x.astype(np.float64)
            mean, var = y64.mean(0), y64.var(0)
            inv = 1.0 / np.sqrt(var + eps)
            yh = (y64 - mean) * inv
            tol = lambda want: 2e-5 * max(1.0, float(np.abs(want).max()))
            for nme, want in (("mean", mean), ("var", var), ("invstd", inv), ("z", yh * gamma + beta), ("grad_gamma", (g64 * yh).sum(0)), ("grad_beta", g64.sum(0)),
                              ("grad_y", gamma * inv * (g64 - g64.mean(0) - yh * (g64 * yh).mean(0))), ("grad_w", g64.T @ x64), ("grad_w nobias", g64.T @ x64),
                              ("grad_bias", g64.sum(0))):
                err = np.abs(r[nme].numpy() - want).max()
                assert err <= tol(want), (nme, err)
            if bf16:
                rb = lambda a: torch.from_numpy(a).to(torch.bfloat16).double().numpy()
                want = rb(gz).T @ rb(x)
                assert np.abs(r["grad_w bf16"].numpy() - want).max() <= 2e-5 * max(1.0, np.abs(want).max()) * np.sqrt(rows / 128 + 1)
                assert np.abs(r["grad_bias bf16"].numpy() - g64.sum(0)).max() <= tol(g64.sum(0))
                if k4:
                    wantc = rb(x) @ rb(w).T + bias
                    assert np.abs(r["c bf16"].numpy() - wantc).max() <= 2e-5 * max(1.0, np.abs(wantc).max())
        return built(call, o, ref)
    return build


for _rows, _n, _k, _ly, _lx, _bf in ((2, 3, 3, 1, 1, True), (257, 33, 128, 3, 4, True), (4099, 128, 33, 4, 3, True), (257, 128, 128, 32, 32, True),
                                     (4099, 3, 128, 1, 8, False), (1, 33, 4, 1, 4, True)):
    case("bn_wgrad-r%d-n%d-k%d-ldy+%d-ldx+%d" % (_rows, _n, _k, _ly, _lx),
         ["sapcu_bn_train_forward", "sapcu_bn_train_backward", "sapcu_conv1x1_wgrad_f32"] + (["sapcu_conv1x1_wgrad_bf16", "sapcu_gemm_bf16"] if _bf else []),
         ["sapcu_train_workspace_bytes"] + (["sapcu_wgrad_bf16_workspace_bytes"] if _bf else []))(_bn_wgrad_case(_rows, _n, _k, _ly, _lx, _bf))


def _softmax_agg_case(b, m, kk, d, hd, ldv_x, with_keep):
    def build(A):
        from oracle import train_path as TP
        _lib, lib = _lib_()
        rng = np.random.default_rng(b + m + d)
        pts = b * m
        ah, ph, vh = rng.normal(0, 2.0, (pts * kk, d)).astype(np.float32), rng.random((pts * kk, d)).astype(np.float32), rng.random((pts, d)).astype(np.float32)
        ih = rng.integers(0, m, size=pts * kk).astype(np.int32)
        gh = rng.normal(0, 1, (pts, d)).astype(np.float32)
        keep = ((rng.random((pts * kk, d)) > 0.1) / 0.9).astype(np.float32) if with_keep else None
        ldv = d + (0 if A.compact else ldv_x)
        a, pe, v, idx, g = A.inp(ah, offset=4, name="a"), A.inp(ph, offset=4, name="pe"), A.inp(vh, pitch=ldv, offset=4, name="v"), \
            A.inp(ih, offset=4, name="idx"), A.inp(gh, offset=4, name="grad_res")
        K = A.inp(keep, offset=4, name="keep") if with_keep else None
        o = {"res": A.out((pts, d), F32, offset=4, name="res"), "grad_a": A.out((pts * kk, d), F32, offset=4, name="grad_a"),
             "grad_pe": A.out((pts * kk, d), F32, offset=4, name="grad_pe"), "grad_v": A.out((pts, d), F32, pitch=ldv, offset=4, name="grad_v")}
        sq = float(np.sqrt(hd))

        def call():
            ok(lib.sapcu_softmax_agg_forward(P(a), P(pe), P(v), ldv, P(idx), P(K), pts, m, kk, d, sq, P(o["res"]), S()))
            ok(lib.sapcu_softmax_agg_backward(P(a), P(pe), P(v), ldv, P(idx), P(K), P(g), pts, m, kk, d, sq, P(o["grad_a"]), P(o["grad_pe"]), P(o["grad_v"]), ldv, S()))

        def ref(r):
            host = [torch.from_numpy(x).clone().requires_grad_(True) for x in (ah, ph, vh)]
            if with_keep:                                          # fn/snn_coder.py:383: dropout on the softmax weights
                at = torch.softmax(host[0].view(pts, kk, d) / sq, dim=1) * torch.from_numpy(keep).view(pts, kk, d)
                nb = ((torch.arange(pts * kk) // kk // m) * m + torch.from_numpy(ih).long())
                ro = (at * (host[2][nb].view(pts, kk, d) + host[1].view(pts, kk, d))).sum(1)
            else:
                ro = TP.softmax_agg(*host, torch.from_numpy(ih), m, sq)
            (ro * torch.from_numpy(gh)).sum().backward()
            assert (r["res"] - ro.detach()).abs().max() <= 2e-6
            for name, hh in zip(("grad_a", "grad_pe", "grad_v"), host):
                assert (r[name] - hh.grad).abs().max() <= 1e-5 * max(1.0, float(hh.grad.abs().max())), name
        return built(call, o, ref)
    return build


for _b, _m, _kk, _d, _hd, _lv, _kp in ((3, 48, 24, 128, 16, 64, False), (2, 48, 18, 256, 32, 4, True), (2, 20, 12, 512, 64, 1, False), (1, 5, 5, 64, 8, 3, True),
                                       (1, 1, 1, 3, 1, 1, False)):
    case("softmax_agg-b%d-m%d-kk%d-d%d-ldv+%d%s" % (_b, _m, _kk, _d, _lv, "-keep" if _kp else ""),
         ["sapcu_softmax_agg_forward", "sapcu_softmax_agg_backward"])(_softmax_agg_case(_b, _m, _kk, _d, _hd, _lv, _kp))


def _rows_case(groups, m, kk, d, ld_x):
    """gather_rows / scatter_add_rows / scatter_add_rows_grouped / group_max on one index set: `groups` patches of m points, kk edges each."""
    def build(A):
        _lib, lib = _lib_()
        rng = np.random.default_rng(groups + m + d)
        src_rows, rows = groups * m, groups * m * kk
        # small integers: every sum is exact in f32, so the float-atomic scatter has one answer whatever its order
        src = rng.integers(-4, 5, (src_rows, d)).astype(np.float32)
        index = ((np.arange(rows) // (m * kk)) * m + rng.integers(0, m, rows)).astype(np.int64)
        go = rng.integers(-3, 4, (rows, d)).astype(np.float32)
        gmax = rng.integers(-3, 4, (groups, d)).astype(np.float32)
        ld = d + (0 if A.compact else ld_x)
        Sr, Ix, Go, Gm = A.inp(src, pitch=ld, offset=4, name="src"), A.inp(index, offset=8, name="index"), A.inp(go, offset=4, name="grad_out"), \
            A.inp(gmax, offset=4, name="group grad_out")
        o = {"gathered": A.out((rows, d), F32, offset=4, name="gather out"), "scatter": A.out((src_rows, d), F32, pitch=ld, offset=4, name="grad_src atomics"),
             "scatter grouped": A.out((src_rows, d), F32, pitch=ld, offset=4, name="grad_src grouped"), "bad": A.out((1,), I32, offset=4, name="bad_count"),
             "max": A.out((groups, d), F32, offset=4, name="group max"), "argmax": A.out((groups, d), I32, offset=4, name="argmax"),
             "grad_x": A.out((src_rows, d), F32, offset=4, name="group max grad_x")}
        Sc = A.inp(src, offset=4, name="src compact")

        def call():
            ok(lib.sapcu_gather_rows(P(Sr), ld, P(Ix), rows, d, P(o["gathered"]), S()))
            ok(lib.sapcu_scatter_add_rows(P(Go), P(Ix), rows, d, P(o["scatter"]), ld, src_rows, S()))
            ok(lib.sapcu_scatter_add_rows_grouped(P(Go), P(Ix), rows, d, P(o["scatter grouped"]), ld, src_rows, m, m * kk, P(o["bad"]), S()))
            ok(lib.sapcu_group_max_forward(P(Sc), groups, m, d, P(o["max"]), P(o["argmax"]), S()))
            ok(lib.sapcu_group_max_backward(P(Gm), P(o["argmax"]), groups, m, d, P(o["grad_x"]), S()))

        def ref(r):
            assert np.array_equal(r["gathered"].numpy(), src[index])
            want = np.zeros((src_rows, d), np.float64)
            np.add.at(want, index, go.astype(np.float64))
            assert np.array_equal(r["scatter"].numpy(), want.astype(np.float32))
            assert np.array_equal(r["scatter grouped"].numpy(), want.astype(np.float32)) and int(r["bad"].item()) == 0
            xs = torch.from_numpy(src).view(groups, m, d)
            val = xs.max(dim=1)[0]
            first = (xs == val.unsqueeze(1)).float().argmax(dim=1)
            assert torch.equal(r["max"], val) and torch.equal(r["argmax"].long(), first)
            gx = torch.zeros(groups, m, d).scatter_(1, first.unsqueeze(1), torch.from_numpy(gmax).unsqueeze(1)).view(src_rows, d)
            assert torch.equal(r["grad_x"], gx)
        return built(call, o, ref)
    return build


for _g, _m, _kk, _d, _ldx in ((1, 1, 1, 3, 1), (3, 48, 12, 128, 64), (5, 20, 18, 33, 3), (2, 100, 24, 128, 0), (257, 7, 1, 33, 31), (86, 48, 1, 3, 61)):
    case("row_ops-g%d-m%d-kk%d-d%d-ld+%d" % (_g, _m, _kk, _d, _ldx),
         ["sapcu_gather_rows", "sapcu_scatter_add_rows", "sapcu_scatter_add_rows_grouped", "sapcu_group_max_forward", "sapcu_group_max_backward"])(
        _rows_case(_g, _m, _kk, _d, _ldx))


# ================================================================================================ the driver
@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_bounds(c):
    run_protocol(c)


# ================================================================================================ refusals: status only, nothing launched
def _refusal(id_, entry_point, want):
    def deco(fn):
        REFUSALS.append((id_, entry_point, want, fn))
        return fn
    return deco


def _gemm_refusal(mode, r, k, n, lda, ldc, a_off=16, w_off=16, csplit=0):
    def run(A):
        _lib, lib = _lib_()
        At = A.inp(np.ones((r, max(lda, k)), np.float32), offset=a_off, name="A")
        Wt = A.inp(np.ones((n, k), np.float32), offset=w_off, name="W")
        C = A.out((r, max(ldc, n)), F32, offset=16, name="C")
        ws = A.ws(4 * n * k + 16, name="w16_ws") if mode != "f32" else None
        return lib.sapcu_gemm_f32(P(At), r, k, lda, P(Wt), n, None, None, 0, P(C), ldc, P(ws), {"f32": 0, "sf16": 0, "ring": 2, "bt": 1}[mode], csplit, S())
    return run


_refusal("gemm-f32-k-not-multiple-of-32", "sapcu_gemm_f32", -1)(_gemm_refusal("f32", 130, 48, 8, 48, 8))
_refusal("gemm-f32-lda-not-multiple-of-4", "sapcu_gemm_f32", -1)(_gemm_refusal("f32", 130, 32, 8, 34, 8))
_refusal("gemm-f32-A-4-byte-aligned", "sapcu_gemm_f32", -1)(_gemm_refusal("f32", 130, 32, 8, 32, 8, a_off=4))
_refusal("gemm-f32-W-8-byte-aligned", "sapcu_gemm_f32", -1)(_gemm_refusal("f32", 130, 32, 8, 32, 8, w_off=8))
_refusal("gemm-sf16-A-4-byte-aligned", "sapcu_gemm_f32", -1)(_gemm_refusal("sf16", 130, 64, 8, 64, 8, a_off=4))
_refusal("gemm-sf16-W-8-byte-aligned", "sapcu_gemm_f32", -1)(_gemm_refusal("sf16", 130, 64, 8, 64, 8, w_off=8))
_refusal("gemm-ring-lda-not-multiple-of-8", "sapcu_gemm_f32", -1)(_gemm_refusal("ring", 130, 32, 8, 36, 8))
_refusal("gemm-ring-A-8-byte-aligned", "sapcu_gemm_f32", -1)(_gemm_refusal("ring", 130, 32, 8, 32, 8, a_off=8))
_refusal("gemm-lda-below-k", "sapcu_gemm_f32", -1)(_gemm_refusal("f32", 130, 64, 8, 32, 8))
_refusal("gemm-ldc-below-n", "sapcu_gemm_f32", -1)(_gemm_refusal("f32", 130, 32, 8, 32, 4))
_refusal("gemm-split-rows-without-w16_ws", "sapcu_gemm_f32", -1)(_gemm_refusal("f32", 130, 32, 8, 32, 8, csplit=1))


@_refusal("to_split_rows-ld_out-below-k", "sapcu_to_split_rows", -1)
def _r_split(A):
    _lib, lib = _lib_()
    a, out = A.inp(np.ones((4, 32), np.float32), name="in"), A.out((4, 32), F32, name="out")
    return lib.sapcu_to_split_rows(P(a), 4, 32, 32, P(out), 16, S())


@_refusal("edge_chain-workspace-one-byte-short", "sapcu_fn_edge_chain_f32", -2)
def _r_chain_ws(A, short=1, d=128, kk=24, steps=4):
    _lib, lib = _lib_()
    b, m = 2, 48
    xyz, idx, qkv, prm, heads, T = _chain_operands(b, m, 128, 24, 1)
    need = lib.sapcu_fn_edge_chain_workspace_bytes(b * m, 128, 24)
    ins = [A.inp(xyz.reshape(b * m, 3), name="patch"), A.inp(idx.reshape(-1).to(I32), name="idx"), A.inp(qkv, name="qkv")] + [A.inp(t, name="param") for t in prm]
    res, ws = A.out((b * m, 128), F32, name="res"), A.ws(need - short, name="chain workspace")
    return lib.sapcu_fn_edge_chain_f32(P(ins[0]), P(ins[1]), b * m, m, d, kk, *[P(t) for t in ins[2:]], heads, steps, P(res), P(ws), need - short, S())


_refusal("edge_chain-unsupported-d-kk", "sapcu_fn_edge_chain_f32", -1)(lambda A: _r_chain_ws(A, short=0, d=128, kk=18))
_refusal("edge_chain-zero-steps", "sapcu_fn_edge_chain_f32", -1)(lambda A: _r_chain_ws(A, short=0, steps=0))


def _lif_train_refusal(steps):
    def run(A):
        _lib, lib = _lib_()
        x, prm, out = A.inp(np.ones((5, 4), np.float32), name="x"), [A.inp(np.ones(4, np.float32), name="p") for _ in range(4)], A.out((5, 4), F32, name="spikes")
        return lib.sapcu_lif_train_forward(P(x), 5, 4, steps, *[P(t) for t in prm], P(out), S())
    return run


_refusal("lif_train-9-steps", "sapcu_lif_train_forward", -1)(_lif_train_refusal(9))
_refusal("lif_train-0-steps", "sapcu_lif_train_forward", -1)(_lif_train_refusal(0))


@_refusal("patch_knn-k-above-m", "sapcu_patch_knn", -1)
def _r_pknn(A):
    _lib, lib = _lib_()
    f, out = A.inp(np.ones((2, 5, 3), np.float32), name="feat"), A.out((2, 5, 6), I32, name="idx_out")
    return lib.sapcu_patch_knn(P(f), 2, 5, 3, 3, 6, P(out), S())


@_refusal("patch_knn-ld-below-c", "sapcu_patch_knn", -1)
def _r_pknn_ld(A):
    _lib, lib = _lib_()
    f, out = A.inp(np.ones((2, 5, 8), np.float32), name="feat"), A.out((2, 5, 2), I32, name="idx_out")
    return lib.sapcu_patch_knn(P(f), 2, 5, 8, 4, 2, P(out), S())


@_refusal("knn_gather-k-above-128", "sapcu_knn_gather_f64", -1)
def _r_knn(A):
    _lib, lib = _lib_()
    c, q, out = A.inp(np.ones((200, 3)), name="cloud"), A.inp(np.ones((2, 3)), name="queries"), A.out((2, 129), I64, name="idx_out")
    return lib.sapcu_knn_gather_f64(P(c), 200, P(q), 2, 129, P(out), None, None, S())


@_refusal("grid_knn-workspace-one-byte-short", "sapcu_knn_self_grid_f64", -1)
def _r_grid(A):
    _lib, lib = _lib_()
    n = 5000
    need = int(lib.sapcu_knn_grid_workspace_bytes(n))
    x, idx, dist, ws = A.inp(np.random.default_rng(0).random((n, 3)), name="pts"), A.out((n, 30), I64, name="idx"), A.out((n, 30), F64, name="dist"), A.ws(need - 1)
    return lib.sapcu_knn_self_grid_f64(P(x), n, 0, n, 30, 0.0, P(idx), P(dist), P(ws), need - 1, None, S())


@_refusal("grid_knn-k-above-64", "sapcu_knn_self_grid_f64", -1)
def _r_grid_k(A):
    _lib, lib = _lib_()
    n = 100
    need = int(lib.sapcu_knn_grid_workspace_bytes(n))
    x, idx, dist, ws = A.inp(np.random.default_rng(0).random((n, 3)), name="pts"), A.out((n, 65), I64, name="idx"), A.out((n, 65), F64, name="dist"), A.ws(need)
    return lib.sapcu_knn_self_grid_f64(P(x), n, 0, n, 65, 0.0, P(idx), P(dist), P(ws), need, None, S())


@_refusal("fps-workspace-one-byte-short", "sapcu_fps_f32", -2)
def _r_fps(A):
    _lib, lib = _lib_()
    need = int(lib.sapcu_fps_workspace_bytes(17))
    x, out, ws = A.inp(np.random.default_rng(0).random((255, 3)).astype(np.float32), name="xyz"), A.out((17,), I64, name="idx"), A.ws(need - 1)
    return lib.sapcu_fps_f32(P(x), 255, 17, P(out), P(ws), need - 1, S())


@_refusal("outlier_stats-kk-above-128", "sapcu_outlier_stats_f64", -1)
def _r_stats(A):
    _lib, lib = _lib_()
    d, rm, cs = A.inp(np.ones((4, 129)), name="dist"), A.out((4,), F64, name="row_mean"), A.out((1,), F64, name="chunk_sum")
    return lib.sapcu_outlier_stats_f64(P(d), 4, 129, 8192, P(rm), P(cs), S())


@_refusal("gemm_bf16-k-not-multiple-of-4", "sapcu_gemm_bf16", -1)
def _r_bf16(A):
    _lib, lib = _lib_()
    a, w, c = A.inp(np.ones((4, 8), np.float32), offset=16, name="a"), A.inp(np.ones((3, 6), np.float32), offset=16, name="w"), A.out((4, 3), F32, name="c")
    return lib.sapcu_gemm_bf16(P(a), 4, 6, 8, P(w), 3, None, P(c), 3, S())


@_refusal("wgrad-bias-gradient-with-pitched-grad_y", "sapcu_conv1x1_wgrad_f32", -1)
def _r_wgrad(A):
    _lib, lib = _lib_()
    need = int(lib.sapcu_train_workspace_bytes(5, 3, 4))
    gy, x, gw, gb, ws = A.inp(np.ones((5, 4), np.float32), name="grad_y"), A.inp(np.ones((5, 4), np.float32), name="x"), A.out((3, 4), F32, name="grad_w"), \
        A.out((3,), F32, name="grad_bias"), A.ws(need)
    return lib.sapcu_conv1x1_wgrad_f32(P(gy), 4, P(x), 4, 5, 3, 4, P(gw), P(gb), P(ws), need, S())


@_refusal("bn_train-workspace-one-byte-short", "sapcu_bn_train_forward", -1)
def _r_bn(A):
    _lib, lib = _lib_()
    need = int(lib.sapcu_train_workspace_bytes(300, 33, 0))
    y, ga, be = A.inp(np.ones((300, 33), np.float32), name="y"), A.inp(np.ones(33, np.float32), name="gamma"), A.inp(np.ones(33, np.float32), name="beta")
    z, o3, ws = A.out((300, 33), F32, name="z"), [A.out((33,), F32, name="stat") for _ in range(3)], A.ws(need - 1)
    return lib.sapcu_bn_train_forward(P(y), 300, 33, P(ga), P(be), 1e-5, P(z), *[P(t) for t in o3], P(ws), need - 1, S())


def _posenc_refusal(d, split, with_ws, tab_off=8):
    def run(A):
        _lib, lib = _lib_()
        b, m, kk = 2, 5, 4
        r = b * m * kk
        one = lambda *shape: np.ones(shape, np.float32)
        P1, W, Bv, L, Q = A.inp(one(r, d), offset=16, name="pe1"), A.inp(one(d, d), offset=16, name="w"), A.inp(one(d), name="bias"), \
            A.inp(one(4, d), name="lif4"), A.inp(one(b * m, 3 * d), name="qkv")
        I = A.inp(np.zeros((b, m, kk), np.int32), name="idx")
        pe, att, tab = A.out((r, d), F32, name="pe"), A.out((r, d), F32, name="attn_in"), A.ws(8 * r, offset=tab_off, name="edge_table_ws")
        ws = A.ws(4 * d * d + 16, offset=16, name="w16_ws") if with_ws else None
        return lib.sapcu_posenc_gemm_f32(P(P1), r, d, P(W), P(Bv), P(L), 4, P(Q), P(I), kk, m, P(pe), P(att), P(tab), P(ws), split, S())
    return run


_refusal("posenc-d-not-multiple-of-32", "sapcu_posenc_gemm_f32", -1)(_posenc_refusal(48, 0, False))
_refusal("posenc-split-rows-without-w16_ws", "sapcu_posenc_gemm_f32", -1)(_posenc_refusal(64, 1, False))
_refusal("posenc-edge_table_ws-4-byte-aligned", "sapcu_posenc_gemm_f32", -1)(_posenc_refusal(64, 0, True, tab_off=4))


@_refusal("fps-workspace-4-byte-aligned", "sapcu_fps_f32", -1)
def _r_fps_al(A):
    _lib, lib = _lib_()
    need = int(lib.sapcu_fps_workspace_bytes(17))
    x, out, ws = A.inp(np.random.default_rng(0).random((255, 3)).astype(np.float32), name="xyz"), A.out((17,), I64, name="idx"), A.ws(need, offset=4)
    return lib.sapcu_fps_f32(P(x), 255, 17, P(out), P(ws), need, S())


@_refusal("grid_knn-workspace-4-byte-aligned", "sapcu_knn_self_grid_f64", -1)
def _r_grid_al(A):
    _lib, lib = _lib_()
    n = 5000
    need = int(lib.sapcu_knn_grid_workspace_bytes(n))
    x, idx, dist, ws = A.inp(np.random.default_rng(0).random((n, 3)), name="pts"), A.out((n, 30), I64, name="idx"), A.out((n, 30), F64, name="dist"), \
        A.ws(need, offset=4)
    return lib.sapcu_knn_self_grid_f64(P(x), n, 0, n, 30, 0.0, P(idx), P(dist), P(ws), need, None, S())


@pytest.mark.gpu
@pytest.mark.parametrize("r", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_launches_nothing(r):
    id_, entry_point, want, run = r
    A = Arena("guard", 0xFF, U.dev())
    rc = run(A)
    torch.cuda.synchronize()
    assert rc == want, "%s returned %d, expected %d" % (entry_point, rc, want)
    A.check()
    for g in A.outs + A.wss:                                             # nothing ran: outputs and workspaces keep every byte
        assert bool((g.payload_bits() == 0xFF).all()), "%s: %s was written by a refused call" % (id_, g.name)
