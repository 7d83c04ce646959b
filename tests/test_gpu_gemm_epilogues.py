"""Every (GEMM launcher, epilogue) pair at its tile edges, on operands that make the arithmetic exact (tests/gemm_cases.py; the
conditions are checked on the host by tests/test_gemm_cases_host.py).

The launchers are reached directly through tests/micro/gemm_probe.hip, a kernel-less shim built once per module and linked against
the library under test.  Per pair a star of shapes runs — the row sweep at two widths, the column sweep, the K sweep, for the max
epilogues the group sizes —, each shape on both operand families, compact and in every pitched / misaligned / split-row form inside
guarded buffers (tests/guarded.py), C pre-filled with NaN bytes.

  BIAS, RESID, LRELU, LRELU_MAX   == on bits against the exact reference;
  every epilogue                  == on bits against another launcher on the same case, and every layout against the compact one;
  LIF, LIF_MAX, LIF_ATTN          the oracle's neuron step on the exact pre-activations, 2e-5 (the bar of
                                  test_ring_gemm_neuron_epilogue_and_split_row_output); attn_in == f32(q - kf) + c from the device's c;
  GELU, RESID_GELU                0.5 x (1 + erf(x / sqrt 2)) in f64 on the exact argument, GELU_BAR relative to max(|ref|, 1);
  the overflow word               0 on every case; raised by a c_split store beyond the f16 range and by a NaN.

Each parameter counts its launches against the count computed from the tables: a sweep that ran nothing fails."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gemm_cases as GC
import gpu_utils as U
import guarded as G
from oracle import snn_path as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c-users-sayakdutta-self-supervised-arbitrary-scale-point-cloud-upsampling-via-snn_amd", "csrc")
F32, I32 = torch.float32, torch.int32
NEURON_BAR = 2e-5
# Largest error of the device's gelu_erf over the whole sweep, relative to max(|ref|, 1), against the f64 reference: GELU_MEASURED;
# the bar is four times that, the margin for another OCML erff.
GELU_MEASURED = 1.1302e-07
GELU_BAR = 4 * GELU_MEASURED


def _ptr(t, byte_offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_offset)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Probe:
    def __init__(self, path):
        from sapcu_amd import _lib
        self.check = _lib.check
        self.lib = ctypes.CDLL(path)
        V, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        sigs = {"gemm_probe": [I, V, L, I, I, V, I, V, V, I, I, V, I, V, I, V, V, V, I, V, V, V, V, I, I, I, V, I, V, V],
                "gemm_probe_split_weights": [V, L, V, V, V, V], "gemm_probe_to_split_rows": [V, L, I, I, V, I, V],
                "gemm_probe_edge_table": [V, L, I, I, V, V], "gemm_probe_decode_max_keys": [V, L, V, V]}
        for name, args in sigs.items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = I, args


class Device:
    """What every case slices: the operands of a (family, k) on the device, W pre-split by launch_split_weights, the column
    parameters, the edge table from launch_edge_table."""

    def __init__(self, probe):
        self.p = probe
        dev = U.dev()
        bias, resid, raw, qk, idx = GC.columns()
        self.bias, self.resid, self.raw, self.qk = (torch.from_numpy(x.copy()).to(dev) for x in (bias, resid, raw, qk))
        self.ovf = torch.zeros(4, dtype=I32, device=dev)
        self.tab = torch.full((GC.R_MAX, 2), -1, dtype=I32, device=dev)
        probe.check(probe.lib.gemm_probe_edge_table(_ptr(torch.from_numpy(idx.copy()).to(dev)), GC.R_MAX, GC.ATTN_M, GC.ATTN_KK, _ptr(self.tab), _stream()))
        torch.cuda.synchronize()
        assert np.array_equal(self.tab.cpu().numpy(), GC.edge_rows())

    @functools.lru_cache(maxsize=None)
    def operands(self, family, k):
        a, w, _ = GC.operands(family, k)
        A, W = torch.from_numpy(a.copy()).to(U.dev()), torch.from_numpy(w.copy()).to(U.dev())
        hi = torch.empty((GC.N_MAX, k), dtype=torch.float16, device=U.dev())
        lo = torch.empty_like(hi)
        self.ovf.zero_()
        self.p.check(self.p.lib.gemm_probe_split_weights(_ptr(W), GC.N_MAX * k, _ptr(hi), _ptr(lo), _ptr(self.ovf), _stream()))
        torch.cuda.synchronize()
        wh, wl = GC.split16(w * np.float32(16.0))
        assert int(self.ovf[0].item()) == 0
        assert np.array_equal(hi.cpu().numpy().view(np.uint16), wh.view(np.uint16)) and np.array_equal(lo.cpu().numpy().view(np.uint16), wl.view(np.uint16))
        return A, W, hi, lo


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    from sapcu_amd import _lib
    _lib.load()
    libdir, libname = os.path.split(os.path.abspath(_lib.LIB_PATH))
    so = str(tmp_path_factory.mktemp("gemm_probe") / "gemm_probe.so")
    # ctypes loads libraries RTLD_LOCAL: the shim names the library it needs itself (-l: + rpath) and the loader hands it the loaded one
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "micro", "gemm_probe.hip"), "-o", so, "-L", libdir, "-l:" + libname, "-Wl,-rpath," + libdir],
                   check=True, capture_output=True, timeout=600)
    probe = Probe(so)
    return probe, Device(probe)


@functools.lru_cache(maxsize=16)
def reference(epi, family, k, T):
    """[R_MAX, N_MAX]: the epilogue of the exact argument — f32 where it is compared on bits or with the neuron bar, f64 for GELU."""
    x = GC.argument(family, k, epi in GC.RESID)
    if epi in ("BIAS", "RESID"):
        return x.astype(np.float32)
    if epi in ("LRELU", "LRELU_MAX"):
        return GC.lrelu(x.astype(np.float32))
    if epi in GC.GELU:
        return GC.gelu64(x)
    raw = GC.columns()[2]
    names = ["membrane_decay", "threshold_adapt", "refractory_decay", "threshold_base"]
    prm = O.neuron_params({"n." + names[i]: torch.from_numpy(raw[i].copy()) for i in range(4)}, "n")
    return O.neuron_selfloop(torch.from_numpy(x.astype(np.float32)), prm, T).numpy()


def _split_indices(ld, n):
    """Half indices of the hi and lo halves of columns 0..n-1 inside a split row of pitch ld floats (csrc/gemm_epi.h)."""
    col = np.arange(n)
    if ld % 32 == 0:
        hi = ((col >> 5) << 6) + (col & 31)
        return hi, hi + 32
    return col, ld + col


class Result:
    pass


def launch(ctx, launcher, epi, family, s, lay, T, bias=None, everything=False):
    """One call.  -> Result: rc, ovf, and what the call wrote, on the host: c / c2 ([r, n] f32, or the [r, ldc] container of split
    rows), mx ([groups, n] decoded maxima), raw (the outputs' payload bytes, for the refusals).  Guards and pitch gaps are checked here."""
    probe, D = ctx
    r, n, k = s.r, s.n, s.k
    A, W, hi, lo = D.operands(family, k)
    ar = G.Arena("compact" if lay.name == "compact" else "guard", device=U.dev())
    off = 4 if lay.misalign else 0
    what = GC.LAUNCHERS.index(launcher)
    a_split = int(launcher in GC.A_SPLIT)
    if a_split:
        a = ar.inp(torch.zeros((r, lay.lda), dtype=F32, device=U.dev()), name="A")
        probe.check(probe.lib.gemm_probe_to_split_rows(_ptr(A), r, k, k, _ptr(a), lay.lda, _stream()))
    else:
        a = ar.inp(A[:r], pitch=lay.lda, name="A")
    bias_t = ar.inp(D.bias[:n] if bias is None else bias, offset=off, name="bias")
    lif = resid = c = c2 = keys = mx_out = None
    if epi in GC.NEURON or everything:
        lif = ar.inp(D.raw[:, :n].contiguous(), offset=off, name="lif")
    if epi in GC.RESID or everything:
        resid = ar.inp(D.resid[:r, :n], pitch=lay.ldr, offset=off, name="resid")
    if epi not in GC.MAXES or everything:
        c = ar.out((r, lay.ldc if lay.c_split else n), pitch=lay.ldc, name="C")
    if epi == "LIF_ATTN" or everything:
        c2 = ar.out((r, lay.ldc if lay.c2_split else n), pitch=lay.ldc, name="C2")
    groups = -(-r // s.max_m) if s.max_m else 1
    if epi in GC.MAXES or everything:
        # zero bands and payload, checked in every layout: an atomicMax past the groups cannot change a band of 0xFF bytes
        kg = G.guarded((groups, n), I32, band_fill=0x00, device=U.dev(), name="keys")
        ar.bufs.append(kg)
        keys = kg.t
        mx_out = ar.out((groups, n), pitch=lay.ldc, name="max_out")
    ldq = D.qk.shape[1]
    args = (_ptr(a), r, k, lay.lda, _ptr(W), n, _ptr(bias_t), _ptr(c), lay.ldc, GC.EPI[epi], _ptr(lif), T, _ptr(resid), lay.ldr, _ptr(c2),
            _ptr(D.qk), _ptr(D.qk, 4 * (GC.N_MAX + lay.misalign)), ldq, _ptr(D.tab), _ptr(hi), _ptr(lo), _ptr(D.ovf), a_split, lay.c_split,
            lay.c2_split, _ptr(keys), s.max_m, _ptr(mx_out), _stream())
    res = Result()
    D.ovf.zero_()
    pred = {"bt": 5, "shortk": 6, "ring": 7}.get(launcher)
    res.accepted = None if pred is None else probe.lib.gemm_probe(pred, *args)
    res.rc = probe.lib.gemm_probe(what, *args)
    torch.cuda.synchronize()
    ar.check()
    res.ovf = int(D.ovf[0].item())
    res.c = None if c is None else c.cpu().numpy()
    res.c2 = None if c2 is None else c2.cpu().numpy()
    res.mx = None
    if res.rc == 0 and epi in GC.MAXES:
        if (launcher, epi) == ("shortk", "LIF_MAX"):
            res.mx = mx_out.cpu().numpy()
        else:
            dec = torch.full((groups, n), float("nan"), dtype=F32, device=U.dev())
            probe.check(probe.lib.gemm_probe_decode_max_keys(_ptr(keys), groups * n, _ptr(dec), _stream()))
            torch.cuda.synchronize()
            res.mx = dec.cpu().numpy()
    res.raw = [t.cpu().numpy().view(np.uint8) for t in (c, c2, mx_out) if t is not None] + ([keys.cpu().numpy()] if keys is not None else [])
    return res


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def assert_same(got, split, ld, want, tag):
    """got == want on bits; `got` is [r, n] f32, or (split) the container of split rows, whose halves must be the split of `want` and
    whose other halves must still hold the filler.  A zero half may carry either sign: where an epilogue ends in a multiplication the
    compiler forms hi with v_fma_mixlo_f16 (a, b, +0), which turns a product of -0 into +0 (lo is then -0: the same value)."""
    n = want.shape[1]
    if not split:
        bad = _bits(got) != _bits(want)
        first = [(int(i), int(j), hex(_bits(got)[i, j]), hex(_bits(want)[i, j])) for i, j in np.argwhere(bad)[:4]]
        assert not bad.any(), (tag, int(bad.sum()), "row, column, bits found, wanted", first)
        return
    halves = np.ascontiguousarray(got).view(np.uint16).reshape(got.shape[0], 2 * ld)
    hi_i, lo_i = _split_indices(ld, n)
    wh, wl = GC.split16(want)
    # on bits, but for the sign of a zero half, which is not part of the format (hi + lo is the value)
    fv = halves.view(np.float16)
    bad = ((halves[:, hi_i] != wh.view(np.uint16)) & ~((fv[:, hi_i] == 0) & (wh == 0))) | \
          ((halves[:, lo_i] != wl.view(np.uint16)) & ~((fv[:, lo_i] == 0) & (wl == 0)))
    first = [(int(i), int(j), hex(halves[i, hi_i[j]]), hex(halves[i, lo_i[j]]), hex(wh.view(np.uint16)[i, j]), hex(wl.view(np.uint16)[i, j]),
              hex(_bits(want)[i, j])) for i, j in np.argwhere(bad)[:4]]
    assert not bad.any(), (tag, int(bad.sum()), "row, column, hi and lo halves found, wanted, the f32 split", first)
    rest = np.ones(2 * ld, bool)
    rest[hi_i] = rest[lo_i] = False
    assert (halves[:, rest] == 0xFFFF).all(), (tag, "a half outside the n columns was written")


def _attn_in(ctx, s, lay, c):
    """f32(q - kf) + c with the kf this layout passes, in f32 as the kernels form it."""
    qk = GC.columns()[3]
    tab = GC.edge_rows()[:s.r]
    kf0 = GC.N_MAX + lay.misalign
    d = (qk[tab[:, 0], :s.n] - qk[tab[:, 1], kf0:kf0 + s.n]).astype(np.float32)
    return (d + c).astype(np.float32)


gelu_worst = {"err": 0.0}


def check_base(launcher, epi, family, s, T, res, tag):
    """The compact call against the reference."""
    ref = reference(epi, family, s.k, T)[:s.r, :s.n]
    got = res.mx if epi in GC.MAXES else res.c
    if epi in GC.MAXES:
        ref = GC.group_max(ref, s.max_m)
    if epi in GC.EXACT:
        assert_same(got, False, 0, ref, tag)
    elif epi in GC.GELU:
        err = float((np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)).max())
        gelu_worst["err"] = max(gelu_worst["err"], err)
        assert err <= GELU_BAR, (tag, err)                 # (a NaN left in the payload fails here too)
    else:
        err = float(np.abs(got.astype(np.float64) - ref).max())
        assert err <= NEURON_BAR, (tag, err)


@pytest.mark.parametrize("launcher,epi", GC.TABLE, ids=["%s-%s" % p for p in GC.TABLE])
def test_pair(ctx, launcher, epi):
    own = others = 0
    for s in GC.star(launcher, epi):
        for family in GC.families(launcher):
            for T in GC.steps(epi):
                lays = GC.layouts(launcher, epi, s)
                tag = (launcher, epi, family, tuple(s), T)
                base = launch(ctx, launcher, epi, family, s, lays[0], T)
                own += 1
                assert base.rc == 0 and base.ovf == 0 and base.accepted in (None, 1), (tag, base.rc, base.ovf, base.accepted)
                check_base(launcher, epi, family, s, T, base, tag)
                bval = base.mx if epi in GC.MAXES else base.c
                if epi == "LIF_ATTN":
                    assert_same(base.c2, False, 0, _attn_in(ctx, s, lays[0], base.c), tag + ("attn_in",))
                other = GC.partner(launcher, epi, family, s)
                if other is not None:
                    s2 = s
                    lay2 = GC.layouts(other, epi, s2)[0]
                    res = launch(ctx, other, epi, family, s2, lay2, T)
                    others += 1
                    assert res.rc == 0 and res.ovf == 0, (tag, other, res.rc, res.ovf)
                    assert_same(res.mx if epi in GC.MAXES else res.c, False, 0, bval, tag + (other,))
                    if epi == "LIF_ATTN":
                        assert_same(res.c2, False, 0, base.c2, tag + (other, "attn_in"))
                for lay in lays[1:]:
                    res = launch(ctx, launcher, epi, family, s, lay, T)
                    own += 1
                    ltag = tag + (lay.name,)
                    assert res.rc == 0 and res.ovf == 0 and res.accepted in (None, 1), (ltag, res.rc, res.ovf, res.accepted)
                    if epi in GC.MAXES:
                        assert_same(res.mx, False, 0, bval, ltag)
                        continue
                    assert_same(res.c, bool(lay.c_split), lay.ldc, bval, ltag)
                    if epi == "LIF_ATTN":
                        assert_same(res.c2, bool(lay.c2_split), lay.ldc, _attn_in(ctx, s, lay, base.c), ltag + ("attn_in",))
    if epi in GC.GELU:
        print("%s %s: largest gelu error relative to max(|ref|, 1) so far: %.4e" % (launcher, epi, gelu_worst["err"]))
    assert (own, others) == GC.expected_runs(launcher, epi)


def _base_shape(launcher, epi):
    r, n = (1153, 128) if launcher == "bt" else (144, 132) if launcher == "shortk" else (129, 132)
    return GC.Shape(r, n, GC.K0, 48 if epi in GC.MAXES else 0)


def _untouched(res):
    keys = res.raw[-1]
    return all((x == 0xFF).all() for x in res.raw[:-1]) and not keys.any()


@pytest.mark.parametrize("launcher,epi", GC.REFUSED, ids=["%s-%s" % p for p in GC.REFUSED])
def test_refused_pair_returns_its_status_and_writes_nothing(ctx, launcher, epi):
    """Every operand any epilogue could want is there: the refusal is about the epilogue alone."""
    s = _base_shape(launcher, epi)
    res = launch(ctx, launcher, epi, "I", s, GC.layouts(launcher, "LIF", s)[0], 4, everything=True)
    assert res.rc == -1 and res.accepted in (None, 0), (res.rc, res.accepted)      # SAPCU_ERR_ARG
    assert _untouched(res) and res.ovf == 0


@pytest.mark.parametrize("launcher,epi,r,n,k,max_m", [
    ("bt", "BIAS", 1023, 128, 64, 0),          # below four row tiles
    ("bt", "LIF", 1153, 132, 64, 0),           # n no multiple of 128
    ("shortk", "LIF", 129, 132, 256, 0),       # k beyond 192
    ("shortk", "LIF_MAX", 144, 132, 64, 5),    # the register max takes max_m = 48 only
    ("shortk", "LIF_MAX", 100, 132, 64, 48),   # ... and whole patches
    ("sf16", "BIAS", 129, 132, 96, 0),         # k no multiple of 64
])
def test_refused_shape_returns_its_status_and_writes_nothing(ctx, launcher, epi, r, n, k, max_m):
    s = GC.Shape(r, n, k, max_m)
    res = launch(ctx, launcher, epi, "I", s, GC.layouts(launcher, "LIF", s)[0], 4, everything=True)
    assert res.rc == -1 and res.accepted in (None, 0), (res.rc, res.accepted)
    assert _untouched(res) and res.ovf == 0


@pytest.mark.parametrize("launcher", ["f32", "sf16", "ring", "bt"])
def test_overflow_word_counts_a_split_store_beyond_the_f16_range(ctx, launcher):
    """EPI_BIAS into split rows: one column's output beyond 65504, then one NaN, then a clean call on the same word."""
    s = _base_shape(launcher, "BIAS")
    lay = GC.layouts(launcher, "BIAS", s)[-1]
    assert lay.c_split
    D = ctx[1]
    for value, want in ((1.0e5, True), (float("nan"), True), (None, False)):
        bias = D.bias[:s.n].clone()
        if value is not None:
            bias[7] = value
        res = launch(ctx, launcher, "BIAS", "I", s, lay, 0, bias=bias)
        assert res.rc == 0 and (res.ovf >= 1) == want, (launcher, value, res.rc, res.ovf)
