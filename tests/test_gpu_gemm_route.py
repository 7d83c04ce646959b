"""The two ways to one GEMM agree, and the router's refusals write nothing (-m gpu; csrc/model.hip gemm_route).

Which kernel a descriptor reaches is decided in one place for the model handles and for the raw entry points.  Kernels that serve
the same descriptor give the same bits, so no output test of a whole forward can see a call that took the other route; this file
pins the pairs against each other on the raw entry point, where the caller picks the route.

Form built: raw call against raw call.  fn's X (the fc1 output of a block) is not among the taps of sapcu_fn_forward (stem, block
outputs, pooled, enc, logits), so the handle's fc1 cannot be compared with a raw call at block granularity.  Instead: raw short-K
against raw SAPCU_SHORTK=0 (the f32-A split-f16 kernel) on fc1's shape class, r = 96, k = 64, n = 128, LIF x 4; and raw
a_split_rows = 1 (big tile) against 2 (ring) on r = 1024, the smallest row count the big-tile kernel takes, k = 64, n = 128, LIF x 4.

It pins behaviour only: it passes at the parent of the commit that added it.
"""
import ctypes

import numpy as np
import pytest
import torch

from guarded import Arena
import gpu_utils as U

pytestmark = pytest.mark.gpu

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
K, N, STEPS = 64, 128, 4


def _lib_():
    from sapcu_amd import _lib
    return _lib, _lib.load()


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _operands(r, seed):
    rng = np.random.default_rng(seed)
    dev = U.dev()
    a = torch.from_numpy(rng.normal(size=(r, K)).astype(np.float32)).to(dev)
    w = torch.from_numpy((rng.normal(size=(N, K)) / np.sqrt(K)).astype(np.float32)).to(dev)
    bias = torch.from_numpy(rng.normal(size=N).astype(np.float32)).to(dev)
    lif = np.stack([rng.uniform(0.05, 1.1, N), rng.uniform(0.0, 0.2, N), rng.uniform(0.05, 1.0, N), rng.normal(0.5, 0.3, N)])
    return a, w, bias, torch.from_numpy(lif.astype(np.float32)).to(dev)


def _gemm(a, r, w, bias, lif, a_split_rows):
    """(C's bit patterns, overflow word) of one sapcu_gemm_f32 call with a split scratch, C and scratch pre-filled 0xFF."""
    mod, lib = _lib_()
    C = torch.full((r, N), float("nan"), dtype=F32, device=U.dev())
    ws = torch.full((4 * N * K + 16,), 0xFF, dtype=U8, device=U.dev())
    mod.check(lib.sapcu_gemm_f32(P(a), r, K, K, P(w), N, P(bias), P(lif), STEPS, P(C), N, P(ws), a_split_rows, 0, S()))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(C).any())
    return C.view(I32).clone(), int(ws[4 * N * K:4 * N * K + 4].clone().view(I32).item())


def test_short_k_and_f32a_kernels_agree(monkeypatch):
    a, w, bias, lif = _operands(96, 1)
    monkeypatch.setenv("SAPCU_SHORTK", "0")
    c0, ovf0 = _gemm(a, 96, w, bias, lif, 0)
    monkeypatch.delenv("SAPCU_SHORTK")
    c1, ovf1 = _gemm(a, 96, w, bias, lif, 0)
    assert torch.equal(c0, c1)
    assert ovf0 == 0 and ovf1 == 0


def test_big_tile_and_ring_kernels_agree():
    mod, lib = _lib_()
    r = 1024
    a, w, bias, lif = _operands(r, 2)
    a_rows = torch.empty_like(a)
    mod.check(lib.sapcu_to_split_rows(P(a), r, K, K, P(a_rows), K, S()))
    c_bt, ovf_bt = _gemm(a_rows, r, w, bias, lif, 1)
    c_ring, ovf_ring = _gemm(a_rows, r, w, bias, lif, 2)
    assert torch.equal(c_bt, c_ring)
    assert ovf_bt == 0 and ovf_ring == 0


def _gemm_call(r, k, a_split_rows, c_split_rows, with_ws):
    def run(A):
        lib = _lib_()[1]
        At = A.inp(np.ones((max(r, 1), k), np.float32), offset=16, name="A")
        Wt = A.inp(np.ones((N, k), np.float32), offset=16, name="W")
        C = A.out((max(r, 1), N), F32, offset=16, name="C")
        ws = A.ws(4 * N * k + 16, offset=16, name="w16_ws") if with_ws else None
        return lib.sapcu_gemm_f32(P(At), r, k, k, P(Wt), N, None, None, 0, P(C), N, P(ws), a_split_rows, c_split_rows, S())
    return run


def _posenc_call(A):
    lib = _lib_()[1]
    b, m, kk, d = 2, 5, 4, 64
    r = b * m * kk
    one = lambda *shape: np.ones(shape, np.float32)
    pe1, w, bias, lif, qkv = A.inp(one(r, d), offset=16, name="pe1"), A.inp(one(d, d), offset=16, name="w"), A.inp(one(d), name="bias"), \
        A.inp(one(4, d), name="lif4"), A.inp(one(b * m, 3 * d), name="qkv")
    idx = A.inp(np.zeros((b, m, kk), np.int32), name="idx")
    pe, att, tab = A.out((r, d), F32, name="pe"), A.out((r, d), F32, name="attn_in"), A.ws(8 * r, offset=8, name="edge_table_ws")
    return lib.sapcu_posenc_gemm_f32(P(pe1), r, d, P(w), P(bias), P(lif), 4, P(qkv), P(idx), kk, m, P(pe), P(att), P(tab), None, 1, S())


REFUSALS = [("c_split_rows-with-k-96", _gemm_call(130, 96, 0, 1, True)),
            ("a_split_rows-without-scratch", _gemm_call(130, 64, 1, 0, False)),
            ("posenc-split_rows-without-scratch", _posenc_call)]


@pytest.mark.parametrize("id_,run", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_sets_the_error_and_writes_nothing(id_, run):
    """SAPCU_ERR_ARG, a text for sapcu_last_error, and every byte of C and of the scratch (its counter included) as it was."""
    A = Arena("guard", 0xFF, U.dev())
    rc = run(A)
    torch.cuda.synchronize()
    assert rc == -1, rc
    assert _lib_()[1].sapcu_last_error()
    A.check()
    for g in A.outs + A.wss:
        assert bool((g.payload_bits() == 0xFF).all()), "%s: %s was written by a refused call" % (id_, g.name)


@pytest.mark.parametrize("a_split_rows", [1, 2])
def test_empty_split_row_call_is_ok_and_leaves_c_alone(a_split_rows):
    """r = 0: SAPCU_OK on either split-row route, no GEMM launch: C keeps every byte.  (The scratch receives the split weights and a
    zeroed counter like that of any accepted call.)"""
    A = Arena("guard", 0xFF, U.dev())
    rc = _gemm_call(0, 64, a_split_rows, 0, True)(A)
    torch.cuda.synchronize()
    assert rc == 0, _lib_()[1].sapcu_last_error()
    A.check()
    for g in A.outs:
        assert bool((g.payload_bits() == 0xFF).all()), "%s was written by an empty call" % g.name
    ws = A.wss[0].t
    assert int(ws[4 * N * 64:4 * N * 64 + 4].clone().view(I32).item()) == 0
