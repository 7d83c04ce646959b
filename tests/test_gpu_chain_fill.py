"""fn block 3 (d = 512, kk = 12) with FILLED groups against the plain grouping (a second handle created under SAPCU_CHAIN_FILL=0).

The plain fused chain runs five points of 12 neighbours in a 64-row group and replays an edge row in the four slots that are left.
The filled form (csrc/fn_edge_chain.hip, default) takes the points in super-groups of 16: three groups of five, and the sixteenth point
(the straddler) rides four neighbours at a time in the spare slots of the three; its softmax-aggregate runs in a small kernel behind the
chain.  Same split-f16 products in the same order, same neuron arithmetic, same softmax routine: every comparison here is torch.equal.
"""
import pytest
import torch

import gpu_utils as U

pytestmark = pytest.mark.gpu

# (patches, points per patch): P = b * m points in one chunk.  At m < 24 blocks 1 and 2 take the five-kernel chain, block 3 the fused one.
SHAPES = [
    (1, 15),     # P = 15: no super-group, tail groups only
    (1, 16),     # exactly one super-group
    (1, 17),     # one super-group and one tail group of one point
    (2, 24),     # three super-groups, all three blocks fused
    (5, 13),     # P = 65: super-groups straddle patch boundaries, tail of one point
    (4, 20),     # every super-group spans two patches
    (3, 26),     # P = 78: tail of 14 points = three tail groups
    (7, 48),     # 63 groups: more than 8, the XCD ranges are in play
]


def _handles(weights, env):
    """(plain, filled) fn models whose handles were created under `env` + SAPCU_CHAIN_FILL=0 and under `env` alone."""
    mp = pytest.MonkeyPatch()
    try:
        mp.delenv("SAPCU_CHAIN_FILL", raising=False)
        plain = U.build_gpu_models_under(weights, mp, dict(env, SAPCU_CHAIN_FILL="0"))[0]
        filled = U.build_gpu_models_under(weights, mp, dict(env))[0]
    finally:
        mp.undo()
    return plain, filled


@pytest.fixture(scope="module")
def pair(weights):
    return _handles(weights, {})


@pytest.fixture(scope="module")
def pair_wide(weights):
    return _handles(weights, {"SAPCU_CHAIN": "wide"})


def _patches(b, m):
    return U.sphere_patches(b, m, skip=700).to(U.dev())


def _forward(model, patch):
    b, m = patch.shape[0], patch.shape[1]
    tap = torch.full((b, m, 64), float("nan"), device=U.dev())
    n = model(patch, taps={"block3": tap})
    torch.cuda.synchronize()
    return n, tap


def _assert_same(plain, filled, patch, tag):
    n0, t0 = _forward(plain, patch)
    n1, t1 = _forward(filled, patch)
    assert not bool(torch.isnan(t0).any()) and not bool(torch.isnan(t1).any()), tag
    assert not bool(torch.isnan(n1).any()), tag
    assert torch.equal(t0, t1), tag             # block 3's output (SAPCU_FN_TAP_BLOCK1 + 2)
    assert torch.equal(n0, n1), tag
    assert plain.gemm_mode()[1] == 0 and filled.gemm_mode()[1] == 0, tag      # no range overflows


@pytest.mark.parametrize("b,m", SHAPES)
def test_filled_groups_equal_the_plain_grouping_bit_for_bit(pair, b, m):
    plain, filled = pair
    assert filled.fused_blocks(m) & 0b100 and plain.fused_blocks(m) & 0b100     # block 3 runs the fused chain in both
    assert filled.gemm_mode()[0]                                                # split-f16 mode: the chain writes split rows
    _assert_same(plain, filled, _patches(b, m), (b, m))


def test_filled_groups_with_64_bit_gather_addresses(pair_wide):
    """SAPCU_CHAIN=wide (the form q|k|v tensors of 4 GiB and more take) has a filled instantiation of its own."""
    plain, filled = pair_wide
    _assert_same(plain, filled, _patches(5, 13), "wide")


def test_f32_results_are_untouched_by_the_switch(weights):
    """Result format.  A handle's fused chain always writes split rows (the cases above); f32 result rows come with SAPCU_GEMM=f32,
    under which the blocks run the five-kernel chain — the switch must change nothing there."""
    plain, filled = _handles(weights, {"SAPCU_GEMM": "f32"})
    assert filled.fused_blocks(48) == 0 and not filled.gemm_mode()[0]
    _assert_same(plain, filled, _patches(5, 13), "f32")


def test_small_embedding_falls_back_to_the_plain_grouping(monkeypatch):
    """emb_dims = 160: edge buffer 1 ([P, emb] floats) cannot hold the straddlers' [P / 16][12][512] values, so block 3 runs the
    plain grouping under either setting: equal outputs.  (Which kernel ran is visible in a kernel trace only.)"""
    from conftest import golden
    row = U.hparam_row(golden("hparams.npz"), "fn-e160")
    monkeypatch.delenv("SAPCU_CHAIN_FILL", raising=False)
    plain, _ = U.build_gpu_hparam_model(row, monkeypatch, {"SAPCU_CHAIN_FILL": "0"})
    filled, _ = U.build_gpu_hparam_model(row, monkeypatch, {})
    assert filled.fused_blocks(48) == 0b111
    _assert_same(plain, filled, _patches(3, 48), "emb 160")


def test_filled_groups_on_a_dirty_workspace(pair):
    """The straddlers' scratch lives in workspace areas that other layers use before and after: every value read was written by this
    launch.  The whole workspace is set to 0xff bytes (NaN as floats) before the forward."""
    plain, filled = pair
    patch = _patches(5, 13)
    n0, t0 = _forward(plain, patch)
    _forward(filled, patch)                       # sizes the model's workspace
    filled._ws.fill_(0xFF)
    n1, t1 = _forward(filled, patch)
    assert torch.equal(t0, t1) and torch.equal(n0, n1)
    assert filled.gemm_mode()[1] == 0
