"""The fused fn edge chain with its trimmed epilogues (csrc/fn_edge_chain.hip, default) against the untrimmed forms (a second handle
created under SAPCU_CHAIN_TRIM=0) and against the five-kernel chain (a third, under SAPCU_CHAIN=0).

Trimmed: fc_delta runs on the exact-f32 MFMA instead of the VALU, and a point that lives in spare slots is summed by the lane groups
that hold its rows, the running sums handed from lane group to lane group in neighbour order, instead of by every lane group over
fetched copies.  Same products and sums in the same order: every comparison here is torch.equal, on the three block taps and on the
normals.
"""
import pytest
import torch

import gpu_utils as U

pytestmark = pytest.mark.gpu

# (patches, points per patch).  b = 1, m = 24 .. 30: P mod 7 = 3, 4, 5, 6, 0, 1, 2 — every tail length of the d = 256 groups of seven
# points (spare-slot points present: none, one, two, all three) — and at d = 512 one super-group of 16 plus plain tails of
# 8 .. 14 points (tail groups of 3, 4, 5 = with point 4, 1, 2, 3, 4 points).  All three blocks run fused from m = 24 on.
TAILS = [(1, m) for m in range(24, 31)]
SHAPES = TAILS + [(3, 48), (1, 100)]


def _handles(weights, env, fn_sd=None):
    """(default, SAPCU_CHAIN_TRIM=0, SAPCU_CHAIN=0) fn models whose handles were created under `env` plus that switch; `fn_sd`: a
    state dict to load instead of the default weights."""
    mp = pytest.MonkeyPatch()
    out = []
    try:
        mp.delenv("SAPCU_CHAIN_TRIM", raising=False)
        for extra in ({}, {"SAPCU_CHAIN_TRIM": "0"}, {"SAPCU_CHAIN": "0"}):
            if "SAPCU_CHAIN" in env and "SAPCU_CHAIN" in extra:
                continue                                     # (the wide pair has no five-kernel third)
            both = dict(env, **extra)
            out.append(U.build_gpu_models_under(weights, mp, both)[0] if fn_sd is None else _fn_model(fn_sd, mp, both))
    finally:
        mp.undo()
    return out


def _fn_model(sd, mp, env):
    """An fn model with the state dict `sd`, its handle created under `env`."""
    import sapcu_amd
    from conftest import FN_KW
    for k, v in env.items():
        mp.setenv(k, v)
    m = sapcu_amd.ImprovedSNNNormalEstimation(**FN_KW)
    m.load_state_dict(sd, strict=True)
    m = m.to(U.dev())
    m._engine()
    for k in env:
        mp.delenv(k, raising=False)
    m.knn_cache_mode = "fresh"
    return m


@pytest.fixture(scope="module")
def trio(weights):
    return _handles(weights, {})


def _patches(b, m):
    return U.sphere_patches(b, m, skip=700).to(U.dev())


def _forward(model, patch):
    b, m = patch.shape[0], patch.shape[1]
    taps = {"block%d" % i: torch.full((b, m, 64), float("nan"), device=U.dev()) for i in (1, 2, 3)}
    n = model(patch, taps=taps)
    torch.cuda.synchronize()
    return [n, taps["block1"], taps["block2"], taps["block3"]]


def _assert_same(models, patch, tag, overflow_free=True):
    outs = [_forward(m, patch) for m in models]
    for o in outs:
        for t in o:
            assert not bool(torch.isnan(t).any()), tag
    for o in outs[1:]:
        for name, x, y in zip(("normals", "block1", "block2", "block3"), outs[0], o):
            assert torch.equal(x, y), (tag, name)
    if overflow_free:
        for m in models:
            assert m.gemm_mode()[1] == 0, tag                # no range overflows
    return outs[0]


@pytest.mark.parametrize("b,m", SHAPES)
def test_trimmed_epilogues_equal_the_untrimmed_and_the_unfused_chain_bit_for_bit(trio, b, m):
    trim, plain, unfused = trio
    assert trim.fused_blocks(m) == 0b111 and plain.fused_blocks(m) == 0b111 and unfused.fused_blocks(m) == 0
    assert trim.gemm_mode()[0]
    _assert_same(trio, _patches(b, m), (b, m))


@pytest.mark.parametrize("b,m", [(1, 27), (3, 48)])
def test_trimmed_epilogues_with_64_bit_gather_addresses(weights, trio, b, m):
    wide = _handles(weights, {"SAPCU_CHAIN": "wide"})
    assert len(wide) == 2
    _assert_same([trio[0]] + wide, _patches(b, m), ("wide", b, m))


def test_trimmed_epilogues_in_plain_groups_of_five(weights, trio):
    """SAPCU_CHAIN_FILL=0: the d = 512 chain without straddlers, whose lane group 3 replays an edge row in its spare slots."""
    nofill = _handles(weights, {"SAPCU_CHAIN_FILL": "0"})
    _assert_same([trio[0]] + nofill, _patches(3, 48), "no fill")


# ---- inputs aimed at fc_delta on the matrix pipe: zero differences (the sign of a zero product), differences of one ulp, large coordinates
def test_a_patch_that_is_one_point_repeated(trio):
    p = _patches(1, 48)[:, 5:6, :].expand(1, 48, 3).contiguous()
    _assert_same(trio, p, "one point 48 times")


def test_a_patch_of_points_one_ulp_apart(trio):
    base = _patches(1, 48)[0, 5].clone()
    pts = base.repeat(48, 1)
    for i in range(48):                                      # a 4 x 4 x 3 lattice of neighbouring floats around the point
        step = (i % 4, (i // 4) % 4, i // 16)
        for c in range(3):
            for _ in range(step[c]):
                pts[i, c] = torch.nextafter(pts[i, c], torch.tensor(float("inf"), device=pts.device))
    _assert_same(trio, pts[None].contiguous(), "one ulp apart")


def test_coordinates_of_magnitude_1e3(trio):
    p = _patches(3, 48) + 1000.0
    _assert_same(trio, p, "offset 1e3", overflow_free=False)
    _assert_same(trio, _patches(3, 48) * 1000.0, "scaled 1e3", overflow_free=False)


# ---- inputs aimed at the handed-on softmax sums
def _scaled_gamma2(weights, scale):
    """Default fn weights with every block's fc_gamma2 output (the logits) multiplied by `scale[l]` through its BatchNorm's affine
    map; scale 0: convolution weights zeroed too, so that a column's logits are its bias for every neighbour."""
    sd = {k: v.clone() for k, v in weights("fn").items()}
    for l in range(3):
        p = "encoder.trans%d.fc_gamma2." % (l + 1)
        if scale[l] == 0.0:
            sd[p + "0.weight"].zero_()
        else:
            sd[p + "1.weight"].mul_(scale[l])
            sd[p + "1.bias"].mul_(scale[l])
    return sd


def test_uniform_softmax_from_zero_gamma2_weights(weights):
    models = _handles(weights, {}, _scaled_gamma2(weights, [0.0, 0.0, 0.0]))
    for b, m in ((1, 27), (3, 48)):
        _assert_same(models, _patches(b, m), ("zero gamma2", b, m))


def test_logits_of_magnitude_80(weights, monkeypatch):
    """fc_gamma2's output scaled so that the largest softmax argument of each block is 80 in magnitude on the (1, 27) patch (measured
    with the oracle on the CPU, whose softmax is watched for the call): most exponentials underflow, the maximum decides."""
    from oracle import snn_path as O
    seen = []
    real = O.F.softmax

    def watch(x, dim=-1, **kw):
        seen.append(float(x.abs().max()))
        return real(x, dim=dim, **kw)

    patch = U.sphere_patches(1, 27, skip=700)
    monkeypatch.setattr(O.F, "softmax", watch)
    with torch.no_grad():
        O.fn_forward(weights("fn"), patch, U.FN_HP)
    monkeypatch.setattr(O.F, "softmax", real)
    assert len(seen) == 3 and min(seen) > 0
    scale = [80.0 / s for s in seen]
    print("largest |logit| per block at the default weights:", seen, "scales:", scale)
    models = _handles(weights, {}, _scaled_gamma2(weights, scale))
    for b, m in ((1, 27), (3, 48)):
        _assert_same(models, _patches(b, m), ("logits 80", b, m))


def test_trimmed_epilogues_on_a_dirty_workspace(trio):
    """Every value the chain reads from the workspace was written by this forward: the whole workspace is set to 0xff bytes (NaN as
    floats) first."""
    trim, plain, _ = trio
    for b, m in ((1, 27), (3, 48)):
        patch = _patches(b, m)
        ref = _forward(plain, patch)
        _forward(trim, patch)                     # sizes the model's workspace
        trim._ws.fill_(0xFF)
        got = _forward(trim, patch)
        for x, y in zip(ref, got):
            assert torch.equal(x, y), (b, m)
        assert trim.gemm_mode()[1] == 0
