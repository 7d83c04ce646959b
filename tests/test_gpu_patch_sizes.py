"""GPU suite (-m gpu): fn and fd at the default configuration at EVERY patch size 1..128, and at row counts b*m on both sides of the
ring / big-tile switch (1024 rows).

Almost every kernel of the inference path changes shape with the patch size m: patch_knn_kernel<256> / <512> at m = 64, the fused
fn blocks at min(k_l, m) = 24 / 18 / 12 and the five-kernel chain with kk = m below 12, point groups of 5 / 16 (d = 512), 7 (d = 256)
and 4 (d = 128) against P = b*m, fd_encoder_kernel's row masks up to m = 48, the per-stage kernels and fd_msc_kernel's 16-point tiles
from m = 49, conv_final's direct max at m = 48 only, the big-tile GEMM from 1024 rows.  Each size is checked against the CPU oracle at
the project's 1e-4 and, bit for bit, against handles created under every switch that takes another path to the same result.

Inputs: sphere_patches(3, m, skip=...) with the skip of tests/patch_size_cases.py, chosen on the CPU from the oracle alone so that
the function is well conditioned and the outputs differ between the patches (rule: tests/golden/make_patch_size_cases.py; checked
without a GPU by tests/test_patch_sizes_host.py).  fd follows the forced-neighbour protocol of tests/test_gpu_parity.py.
"""
import pytest
import torch

from oracle import snn_path as O
import gpu_utils as U
import patch_size_cases as P

pytestmark = pytest.mark.gpu
TOL = 1e-4                                      # tests/test_gpu_parity.py
SIZES = list(range(1, 129))
SUB = 7                                         # sub-batch of the row-count cases

SWITCHES = ("SAPCU_GEMM", "SAPCU_BT", "SAPCU_CHAIN", "SAPCU_CHAIN_FILL", "SAPCU_CHAIN_TRIM", "SAPCU_SHORTK", "SAPCU_FN_MAXFUSE",
            "SAPCU_FN_FOLD_OUT", "SAPCU_FD_MAXFUSE", "SAPCU_FD_SPLIT", "SAPCU_FD_FUSED", "SAPCU_FD_X0", "SAPCU_CHUNK", "SAPCU_WS_BUDGET_MB")
# handles that must give the default handle's bits (include/sapcu.h, sapcu_model_create)
FN_ALT = ({"SAPCU_CHAIN": "0"}, {"SAPCU_CHAIN_FILL": "0"}, {"SAPCU_CHAIN_TRIM": "0"}, {"SAPCU_SHORTK": "0"}, {"SAPCU_FN_MAXFUSE": "0"})
FD_SLAB = {"SAPCU_FD_FUSED": "0", "SAPCU_FD_X0": "0"}
FD_ALT = ({"SAPCU_FD_FUSED": "0"}, FD_SLAB, dict(FD_SLAB, SAPCU_FD_MAXFUSE="0"), {"SAPCU_FD_SPLIT": "0"})

# rows = b*m around 4 * TBM = 1024, where the split-row GEMMs move from the ring kernel to the big-tile kernel
ROW_SHAPES = [(33, 31), (11, 93),                                       # 1023
              (128, 8), (64, 16), (32, 32), (16, 64), (8, 128),         # 1024
              (25, 41), (41, 25),                                       # 1025
              (13, 79)]                                                 # 1027
SLAB_SHAPES = [(3, 85), (4, 64), (5, 52)]       # T*b*m = 1020, 1024, 1040 rows of the SAPCU_FD_X0=0 path's multi_scale_conv GEMM (T = 4)

_ORACLE = {}                                    # (kind, m, ...) -> the oracle on the case's three patches, computed once


def _tag(env):
    return " ".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


def _under(weights, which, envs):
    mp = pytest.MonkeyPatch()
    try:
        for name in SWITCHES:
            mp.delenv(name, raising=False)
        return {_tag(env): U.build_gpu_models_under(weights, mp, dict(env))[which] for env in envs}
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def fn_handles(weights):
    """{switches: fn model}: the default handle, the five alternate paths and the ring-kernel-only handle of the row-count cases."""
    return _under(weights, 0, ({},) + FN_ALT + ({"SAPCU_BT": "0"},))


@pytest.fixture(scope="module")
def fd_handles(weights):
    return _under(weights, 1, ({},) + FD_ALT + ({"SAPCU_BT": "0"}, dict(FD_SLAB, SAPCU_BT="0")))


@pytest.fixture(scope="module")
def state(weights):
    return weights("fn"), weights("fd")


def _fn_mask(m):
    """include/sapcu.h sapcu_model_fused_blocks at the default k_values."""
    return sum(1 << l for l, k in enumerate((24, 18, 12)) if min(k, m) == k)


def _fn_run(fn, patch_dev):
    """(normals, the three neighbour tables the forward used)."""
    b, m = patch_dev.shape[0], patch_dev.shape[1]
    fn.knn_cache_mode = "reference"
    fn._knn_cache.clear()
    try:
        n = fn(patch_dev)
        torch.cuda.synchronize()
        tabs = [t.clone() for t in fn.knn_tables(b, m)]
    finally:
        fn.knn_cache_mode = "fresh"
        fn._knn_cache.clear()
    return n, tabs


def _fn_oracle(sdn, m, patch):
    key = ("fn", m)
    if key not in _ORACLE:
        taps = {}
        with torch.no_grad():
            ref = O.fn_forward(sdn, patch, U.FN_HP, taps=taps)
        _ORACLE[key] = (patch.clone(), ref, taps["knn_idx"])
    p0, ref, idx = _ORACLE[key]
    assert torch.equal(p0, patch)
    return ref, idx


def _fd_oracle_forced(sdd, m, patch, knn_cpu):
    """The oracle on the three patches with the feature-space neighbours `knn_cpu` [3, 3, m, kk] forced; one evaluation per distinct
    set of tables (the row-count cases see the sweep's tables again unless a result depends on the batch)."""
    key = ("fd", m)
    for p0, k0, d in _ORACLE.setdefault(key, []):
        if torch.equal(p0, patch) and torch.equal(k0, knn_cpu):
            return d
    with torch.no_grad():
        d = O.fd_forward(sdd, patch, U.FD_HP, force_idx=[knn_cpu[0], knn_cpu[1], knn_cpu[2]])
    _ORACLE[key].append((patch.clone(), knn_cpu.clone(), d))
    return d


def _fd_run(fd, patch_dev, enc=False, force=None):
    """(distances, knn tap, enc tap or None); the taps are pre-filled so that an unwritten entry shows."""
    b, m = patch_dev.shape[0], patch_dev.shape[1]
    taps = {"knn": torch.full((3, b, m, min(32, m)), -1, dtype=torch.int32, device=U.dev())}
    if enc:
        taps["enc"] = torch.full((b, 768), float("nan"), device=U.dev())
    d = fd(patch_dev, taps=taps, knn_force=force)
    torch.cuda.synchronize()
    return d, taps["knn"], taps.get("enc")


def _unscreened(kind, m):
    for mm, gap in P.UNSCREENED[kind]:
        if mm == m:
            return gap
    return None


# ------------------------------------------------------------------------------------------------------------- every patch size
@pytest.mark.parametrize("m", SIZES)
def test_fn_at_patch_size(m, fn_handles, state):
    fn, sdn = fn_handles["default"], state[0]
    assert fn.fused_blocks(m) == _fn_mask(m), "m=%d: fused_blocks %s, documented %s" % (m, bin(fn.fused_blocks(m)), bin(_fn_mask(m)))
    assert fn_handles["SAPCU_CHAIN=0"].fused_blocks(m) == 0, m             # (the switches were read: another path, not a second default)
    patch = P.patches("fn", m)
    patch_dev = patch.to(U.dev())
    n_dev, tabs = _fn_run(fn, patch_dev)
    n = n_dev.cpu()
    assert not bool(torch.isnan(n).any()), m
    assert float((n.norm(dim=1) - 1).abs().max()) < 1e-5, m
    for tag, alt in fn_handles.items():                         # every switch, whether or not it changes the path at this m
        if tag != "default":
            assert torch.equal(alt(patch_dev), n_dev), "m=%d: the %s handle differs (max %g)" % (m, tag, float((alt(patch_dev) - n_dev).abs().max()))
    for h in fn_handles.values():
        assert h.gemm_mode() == (True, 0), m
    ref, idx = _fn_oracle(sdn, m, patch)
    for l, (got, want) in enumerate(zip(tabs, idx)):
        assert torch.equal(got.cpu().long(), want), "m=%d: in-patch neighbour table %d must be bit-exact" % (m, l)
    gap = _unscreened("fn", m)
    err = float((n - ref).abs().max())
    print("fn m=%d: mask %s  |normals - oracle| %.3g" % (m, bin(_fn_mask(m)), err))
    if gap is not None:
        pytest.skip("fn m=%d: no candidate input is well conditioned (best |oracle f32 - f64| %.3g): oracle comparison not made" % (m, gap))
    assert err <= TOL, "m=%d: |normals - oracle| %g" % (m, err)


@pytest.mark.parametrize("m", SIZES)
def test_fd_at_patch_size(m, fd_handles, state):
    fd, sdd = fd_handles["default"], state[1]
    assert fd.fused_blocks(m) == (1 if m <= 48 else 2), m
    for env in FD_ALT[:3]:                                      # (the switches were read: per-stage kernels through HBM)
        assert fd_handles[_tag(env)].fused_blocks(m) == 0, (m, env)
    assert fd_handles["SAPCU_FD_SPLIT=0"].fused_blocks(m) == (1 if m <= 48 else 0), m       # f32 spike slabs instead of the x0 path
    patch = P.patches("fd", m)
    patch_dev = patch.to(U.dev())
    d_gpu, d_forced, d_free, flips, _ = U.fd_forward_forced(fd, sdd, patch)
    assert not bool(torch.isnan(d_gpu).any()), m
    # the alternate paths, the default handle's neighbours forced: same encoding, same distances
    da, knn, enc = _fd_run(fd, patch_dev, enc=True)
    assert not bool(torch.isnan(enc).any()) and int(knn.min()) >= 0 and int(knn.max()) < m, m
    assert torch.equal(da.cpu(), d_gpu), m
    for tag, alt in fd_handles.items():
        if tag == "default":
            continue
        db, used, enc_b = _fd_run(alt, patch_dev, enc=True, force=knn)
        assert torch.equal(used, knn), "m=%d: %s handle: forced tables not honoured" % (m, tag)
        assert not bool(torch.isnan(enc_b).any()), "m=%d: %s handle: encoding not fully written" % (m, tag)
        assert torch.equal(enc, enc_b), "m=%d: encoding differs from the %s handle (max %g)" % (m, tag, float((enc - enc_b).abs().max()))
        assert torch.equal(da, db), "m=%d: the %s handle differs" % (m, tag)
    for h in fd_handles.values():
        assert h.gate_violations() == 0 and h.gemm_mode() == (True, 0), m
    _ORACLE.setdefault(("fd", m), []).append((patch.clone(), knn.cpu().long(), d_forced))
    err = float((d_gpu - d_forced).abs().max())
    print("fd m=%d: |dist - oracle| %.3g (device's neighbours forced)  free-running: %d of %d rows with another neighbour set"
          % (m, err, sum(int(f.sum()) for f in flips), 9 * m))
    gap = _unscreened("fd", m)
    if gap is not None:
        pytest.skip("fd m=%d: no candidate input is well conditioned (best |oracle f32 - f64| %.3g): oracle comparison not made" % (m, gap))
    assert err <= TOL, "m=%d: |dist - oracle| %g" % (m, err)
    assert float(d_free.std()) > 1e-2, m


# ------------------------------------------------------------------------------------------------------------- row counts
def _sub_batches(run, patch_dev, step):
    parts = [run(patch_dev[i:i + step]) for i in range(0, patch_dev.shape[0], step)]
    return [torch.cat([p[j] for p in parts], dim=(1 if parts[0][j].dim() == 4 else 0)) for j in range(len(parts[0]))]


@pytest.mark.parametrize("b,m", ROW_SHAPES, ids=["%dx%d" % s for s in ROW_SHAPES])
def test_fn_rows_around_the_big_tile_threshold(b, m, fn_handles, state):
    """Results do not depend on the batch a patch is in — held across the ring / big-tile switch: the whole batch (b*m rows) equals
    sub-batches of 7 patches (at most 896 rows) and the ring-kernel-only handle, normals and neighbour tables."""
    fn, ring = fn_handles["default"], fn_handles["SAPCU_BT=0"]
    patch = P.patches("fn", m, b)
    patch_dev = patch.to(U.dev())

    def run(p):
        n, tabs = _fn_run(fn, p)
        return [n] + tabs

    whole = run(patch_dev)
    parts = _sub_batches(run, patch_dev, SUB)
    for name, a, c in zip(("normals", "table 1", "table 2", "table 3"), whole, parts):
        assert a.shape == c.shape and torch.equal(a, c), "%dx%d: %s differ between the whole batch and sub-batches of %d" % (b, m, name, SUB)
    assert torch.equal(ring(patch_dev), whole[0]), "%dx%d: the SAPCU_BT=0 handle differs" % (b, m)
    assert fn.gemm_mode() == (True, 0) and ring.gemm_mode() == (True, 0)
    ref, idx = _fn_oracle(state[0], m, patch[:3].clone())
    for got, want in zip(whole[1:], idx):
        assert torch.equal(got[:3].cpu().long(), want), (b, m)
    if _unscreened("fn", m) is None:
        err = float((whole[0][:3].cpu() - ref).abs().max())
        print("fn %dx%d: |normals - oracle| %.3g" % (b, m, err))
        assert err <= TOL, (b, m, err)


def _fd_rows(fd, ring, sdd, b, m, steps):
    patch = P.patches("fd", m, b)
    patch_dev = patch.to(U.dev())

    def run(p):
        d, knn, _ = _fd_run(fd, p)
        return [d, knn]

    d, knn = run(patch_dev)
    assert int(knn.min()) >= 0 and int(knn.max()) < m
    for step in steps:
        d_p, knn_p = _sub_batches(run, patch_dev, step)
        assert knn_p.shape == knn.shape and torch.equal(knn_p, knn), "%dx%d: neighbour tables differ between the whole batch and sub-batches of %d" % (b, m, step)
        assert torch.equal(d_p, d), "%dx%d: distances differ between the whole batch and sub-batches of %d" % (b, m, step)
    d_r, knn_r, _ = _fd_run(ring, patch_dev)
    assert torch.equal(knn_r, knn) and torch.equal(d_r, d), "%dx%d: the SAPCU_BT=0 handle differs" % (b, m)
    for h in (fd, ring):
        assert h.gate_violations() == 0 and h.gemm_mode() == (True, 0)
    if _unscreened("fd", m) is None:
        want = _fd_oracle_forced(sdd, m, patch[:3].clone(), knn[:, :3].cpu().long())
        err = float((d[:3].cpu() - want).abs().max())
        print("fd %dx%d: |dist - oracle| %.3g (device's neighbours forced)" % (b, m, err))
        assert err <= TOL, (b, m, err)
    return patch_dev, d, knn


@pytest.mark.parametrize("b,m", ROW_SHAPES, ids=["%dx%d" % s for s in ROW_SHAPES])
def test_fd_rows_around_the_big_tile_threshold(b, m, fd_handles, state):
    """As for fn: free-running neighbour tables and distances of the whole batch against sub-batches of 7 and the SAPCU_BT=0 handle."""
    _fd_rows(fd_handles["default"], fd_handles["SAPCU_BT=0"], state[1], b, m, (SUB,))


@pytest.mark.parametrize("b,m", SLAB_SHAPES, ids=["%dx%d" % s for s in SLAB_SHAPES])
def test_fd_spike_slab_rows_around_the_big_tile_threshold(b, m, fd_handles, state):
    """The SAPCU_FD_FUSED=0 + SAPCU_FD_X0=0 handle runs multi_scale_conv over T*b*m rows (T = 4): 1020, 1024 and 1040.  These
    batches are smaller than 7 patches, so they are also run one patch at a time (at most 340 rows: the ring kernel)."""
    slab = fd_handles[_tag(FD_SLAB)]
    assert slab.fused_blocks(m) == 0
    patch_dev, d, knn = _fd_rows(slab, fd_handles[_tag(dict(FD_SLAB, SAPCU_BT="0"))], state[1], b, m, (SUB, 1))
    d0, knn0, _ = _fd_run(fd_handles["default"], patch_dev, force=knn)
    assert torch.equal(knn0, knn) and torch.equal(d0, d), "%dx%d: the default handle differs" % (b, m)
