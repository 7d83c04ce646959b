"""The short-K split-f16 GEMM (csrc/gemm_shortk.hip: fn's fc1 layers, K = 64, and conv_final, K = 192) against the kernel it
replaces (gemm_sf16_kernel, reached under SAPCU_SHORTK=0).

Same operand split, same products in the same order into one f32 accumulator, same neuron arithmetic; at M = 48 conv_final's max
over the patch's points is taken in registers instead of by integer atomicMax on order-preserving keys, which is the same number for
finite values.  Every comparison here is therefore torch.equal (on the bit patterns where a buffer keeps untouched NaN filler).
"""
import ctypes

import numpy as np
import pytest
import torch

import gpu_utils as U

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32


def _lib_():
    from sapcu_amd import _lib
    return _lib, _lib.load()


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw_lif(rng, n):
    return np.stack([rng.uniform(0.05, 1.1, n), rng.uniform(0.0, 0.2, n), rng.uniform(0.05, 1.0, n), rng.normal(0.5, 0.3, n)]).astype(np.float32)


def _decode_split_rows(t, n):
    rows, ld = t.shape
    halves = t.contiguous().view(torch.float16).view(rows, 2 * ld).float()
    if ld % 32 == 0:
        g = halves.view(rows, ld // 32, 2, 32)
        return (g[:, :, 0, :] + g[:, :, 1, :]).reshape(rows, ld)[:, :n].contiguous()
    return (halves[:, :n] + halves[:, ld:ld + n]).contiguous()


class _Gemm:
    """One sapcu_gemm_f32 problem on the device: split-f16 (w16_ws given), lif4 given, f32 A.  wide: A is the 64-column slice at
    column 64 of 192-wide rows (what fn blocks 2 and 3 read from `cat`)."""

    def __init__(self, r, k, n, wide, csplit, steps, hot=False):
        rng = np.random.default_rng(r * 131 + k * 7 + n)
        self.r, self.k, self.n, self.csplit, self.steps = r, k, n, csplit, steps
        self.lda = 192 if wide else k
        full = rng.normal(size=(r, self.lda)).astype(np.float32)
        if hot:
            full[r // 2, (64 if wide else 0) + 5] = 1e5
        self.A = torch.from_numpy(full).to(U.dev())
        self.a_off = 64 if wide else 0
        self.W = torch.from_numpy((rng.normal(size=(n, k)) / np.sqrt(k)).astype(np.float32)).to(U.dev())
        self.bias = torch.from_numpy(rng.normal(size=n).astype(np.float32)).to(U.dev())
        self.lif = torch.from_numpy(_raw_lif(rng, n)).to(U.dev())
        self.ldc = n if csplit else n + 4
        self.ws = torch.empty(4 * n * k + 16, dtype=torch.uint8, device=U.dev())

    def run(self, monkeypatch, shortk):
        """(C as int32 bit patterns, C's values [r, n], overflow word) of one call with the switch set (`shortk` False: SAPCU_SHORTK=0)."""
        mod, lib = _lib_()
        if shortk:
            monkeypatch.delenv("SAPCU_SHORTK", raising=False)
        else:
            monkeypatch.setenv("SAPCU_SHORTK", "0")
        C = torch.full((self.r, self.ldc), float("nan"), dtype=F32, device=U.dev())
        self.ws.fill_(0xFF)
        a_ptr = ctypes.c_void_p(self.A.data_ptr() + 4 * self.a_off)
        mod.check(lib.sapcu_gemm_f32(a_ptr, self.r, self.k, self.lda, P(self.W), self.n, P(self.bias), P(self.lif), self.steps, P(C), self.ldc,
                                     P(self.ws), 0, self.csplit, S()))
        torch.cuda.synchronize()
        monkeypatch.delenv("SAPCU_SHORTK", raising=False)
        ovf = int(self.ws[4 * self.n * self.k:4 * self.n * self.k + 4].clone().view(I32).item())
        vals = _decode_split_rows(C, self.n) if self.csplit else C[:, :self.n]
        return C.view(I32).clone(), vals, ovf


ROWS = [1, 47, 48, 49, 130, 1000]       # one ragged group, the 48 / 49 edge of a 64-row group's second tile, three groups, many
COLS = [128, 256, 512, 640, 160]        # the fc1 widths, conv_final's, and one that is no multiple of 64
# (k, A as the 64-column slice of 192-wide rows): every depth the kernel accepts
DEPTHS = [(64, False), (64, True), (128, False), (192, False)]


@pytest.mark.parametrize("steps", [4, 6])
@pytest.mark.parametrize("csplit", [0, 1])
@pytest.mark.parametrize("k,wide", DEPTHS)
def test_gemm_entry_equals_the_kernel_it_replaces(monkeypatch, k, wide, csplit, steps):
    for r in ROWS:
        for n in COLS:
            p = _Gemm(r, k, n, wide, csplit, steps)
            bits0, vals0, ovf0 = p.run(monkeypatch, shortk=False)
            bits1, vals1, ovf1 = p.run(monkeypatch, shortk=True)
            tag = (r, k, n, wide, csplit, steps)
            assert not bool(torch.isnan(vals0).any()) and not bool(torch.isnan(vals1).any()), tag    # C was pre-filled with NaN
            assert torch.equal(vals0, vals1), tag
            assert torch.equal(bits0, bits1), tag          # the pitch gap of an f32 C keeps its filler, a split row its every half
            assert ovf0 == 0 and ovf1 == 0, tag


@pytest.mark.parametrize("k,wide", [(64, True), (192, False)])
def test_gemm_entry_counts_a_value_beyond_the_f16_range(monkeypatch, k, wide):
    p = _Gemm(130, k, 256, wide, 0, 4, hot=True)
    assert p.run(monkeypatch, shortk=False)[2] >= 1
    assert p.run(monkeypatch, shortk=True)[2] >= 1


# ------------------------------------------------------------------------------------------------ the model
TAPS = {"block1": 64, "block2": 64, "block3": 64}
# (patches, points per patch).  (7, 48): more row groups than XCD ranges; (5, 13) and (2, 100): conv_final's general-M path
SHAPES = [(1, 48), (3, 48), (7, 48), (5, 13), (2, 100)]


def _handles(build, env):
    """(old routing, new routing): handles created under `env` + SAPCU_SHORTK=0 and under `env` alone."""
    mp = pytest.MonkeyPatch()
    try:
        mp.delenv("SAPCU_SHORTK", raising=False)
        old = build(mp, dict(env, SAPCU_SHORTK="0"))
        new = build(mp, dict(env))
    finally:
        mp.undo()
    return old, new


@pytest.fixture(scope="module")
def pair(weights):
    return _handles(lambda mp, env: U.build_gpu_models_under(weights, mp, env)[0], {})


def _patches(b, m):
    return U.sphere_patches(b, m, skip=700).to(U.dev())


def _forward(model, patch, emb):
    b, m = patch.shape[0], patch.shape[1]
    taps = {name: torch.full((b, m, c), float("nan"), device=U.dev()) for name, c in TAPS.items()}
    taps["pooled"] = torch.full((b, emb), float("nan"), device=U.dev())
    n = model(patch, taps=taps)
    torch.cuda.synchronize()
    return n, taps


def _assert_same(old, new, patch, tag, emb=640, dirty=False):
    n0, t0 = _forward(old, patch, emb)
    if dirty:
        _forward(new, patch, emb)             # sizes the model's workspace
        new._ws.fill_(0xFF)
    n1, t1 = _forward(new, patch, emb)
    for name in t0:
        assert not bool(torch.isnan(t0[name]).any()) and not bool(torch.isnan(t1[name]).any()), (tag, name)
        assert torch.equal(t0[name], t1[name]), (tag, name)
    assert not bool(torch.isnan(n1).any()), tag
    assert torch.equal(n0, n1), tag
    assert old.gemm_mode()[1] == 0 and new.gemm_mode()[1] == 0, tag      # no range overflows


@pytest.mark.parametrize("b,m", SHAPES)
def test_model_equals_the_old_routing_bit_for_bit(pair, b, m):
    old, new = pair
    assert new.gemm_mode()[0]
    _assert_same(old, new, _patches(b, m), (b, m))


def test_model_on_a_dirty_workspace(pair):
    """The key area at the head of edge buffer 1 is neither cleared nor read at M = 48 any more; nothing else may read it either."""
    old, new = pair
    _assert_same(old, new, _patches(3, 48), "dirty", dirty=True)


@pytest.mark.parametrize("rid", ["fn-e160", "fn-T1", "fn-ctor"])
def test_model_at_other_hyper_parameters(rid):
    """fn-e160: conv_final with n = 160 (five column tiles, not a multiple of 64).  fn-T1 and fn-ctor: time_steps_enc 1 and 8 — the
    neuron loop of conv_final with no middle step and with six."""
    from conftest import golden
    row = U.hparam_row(golden("hparams.npz"), rid)
    old, new = _handles(lambda mp, env: U.build_gpu_hparam_model(row, mp, env)[0], {})
    _assert_same(old, new, _patches(3, 48), rid, emb=row["kw"]["emb_dims"])


def test_f32_mode_is_untouched_by_the_switch(weights):
    old, new = _handles(lambda mp, env: U.build_gpu_models_under(weights, mp, env)[0], {"SAPCU_GEMM": "f32"})
    assert not new.gemm_mode()[0] and not old.gemm_mode()[0]
    _assert_same(old, new, _patches(3, 48), "f32")
