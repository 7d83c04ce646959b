"""GPU suite (-m gpu): fn and fd at every hyper-parameter setting sapcu_model_create accepts, one case per row of
tests/golden/hparams.npz (the reference run at that setting; matrix in tests/golden/make_fixtures.py), and the settings it refuses.

Per row and patch size, in dependency order: which kernels the handle takes (sapcu_model_fused_blocks against the rule of
include/sapcu.h, worked out HERE from the row's kwargs), neighbour tables, outputs against the reference run and against the oracle
at the project's 1e-4, counters, and the same bits from a second handle on the alternate path (SAPCU_CHAIN=0 / SAPCU_FD_FUSED=0).
fd follows the forced-neighbour protocol of tests/test_gpu_parity.py; free-running neighbour flips are printed, not bounded.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import FD_KW, FN_KW, golden
from oracle import snn_path as O
import gpu_utils as U

pytestmark = pytest.mark.gpu
TOL = 1e-4                                      # tests/test_gpu_parity.py

_G = golden("hparams.npz")
ROWS = [str(r) for r in _G["rows"]]
_MASKS = {}                                     # row id -> {m_pts: mask the default handle reported}


def _expected_mask(row, m):
    """include/sapcu.h sapcu_model_fused_blocks, from the kwargs alone."""
    kw = row["kw"]
    if row["kind"] == "fn":
        return sum(1 << l for l, (d, k) in enumerate(((128, 24), (256, 18), (512, 12))) if min(kw["k_values"][l], m) == k)
    if kw["emb_dims"] < 96:
        return 0
    return 1 if (m <= 48 and len(kw["k_scales"]) <= 4) else 2


def _mask_sizes(row):
    return sorted(set(row["sizes"]) | {48})


def _record_masks(row, model):
    _MASKS[row["id"]] = {m: model.fused_blocks(m) for m in _mask_sizes(row)}
    return _MASKS[row["id"]]


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=U.dev())
    return t.to(dtype) if dtype is not None else t


def _check_fn(row, monkeypatch):
    rid, hp = row["id"], row["hp"]
    fn, sd = U.build_gpu_hparam_model(row)
    masks = _record_masks(row, fn)
    unfused = None
    for m in row["sizes"]:
        tag = "%s m=%d" % (rid, m)
        want_mask = _expected_mask(row, m)
        assert masks[m] == want_mask, "%s: fused_blocks %s, documented %s" % (tag, bin(masks[m]), bin(want_mask))
        patch = torch.from_numpy(_G["%s/m%d:patch" % (rid, m)])
        fn.knn_cache_mode = "reference"
        fn._knn_cache.clear()
        n_dev = fn(patch.to(U.dev()))
        torch.cuda.synchronize()
        n = n_dev.cpu()
        taps = {}
        with torch.no_grad():
            ref = O.fn_forward(sd, patch, hp, taps=taps)
        for got, want in zip(fn.knn_tables(3, m), taps["knn_idx"]):
            assert torch.equal(got.cpu().long(), want), tag + ": in-patch xyz neighbour tables must be bit-exact"
        e_fix = float(np.abs(n.numpy() - _G["%s/m%d:normals" % (rid, m)]).max())
        e_ora = float((n - ref).abs().max())
        print("%s: mask %s  |normals - reference run| %.3g  |normals - oracle| %.3g" % (tag, bin(want_mask), e_fix, e_ora))
        assert e_fix <= TOL and e_ora <= TOL, tag
        assert ref.std(0).max() > 1e-2 and (n.norm(dim=1) - 1).abs().max() < 1e-5, tag
        fn.knn_cache_mode = "fresh"
        if want_mask:                                   # the switches change speed, not results (sapcu.h): the five-kernel chain, same bits
            if unfused is None:
                unfused, _ = U.build_gpu_hparam_model(row, monkeypatch, {"SAPCU_CHAIN": "0"})
            assert unfused.fused_blocks(m) == 0
            assert torch.equal(unfused(patch.to(U.dev())), n_dev), tag + ": SAPCU_CHAIN=0 handle differs"
    assert fn.gemm_mode() == (True, 0), rid


def _check_fd(row, monkeypatch):
    rid, hp = row["id"], row["hp"]
    fd, sd = U.build_gpu_hparam_model(row)
    masks = _record_masks(row, fd)
    stage, _ = U.build_gpu_hparam_model(row, monkeypatch, {"SAPCU_FD_FUSED": "0"})
    emb = hp["emb_dims"]
    for m in row["sizes"]:
        tag = "%s m=%d" % (rid, m)
        want_mask = _expected_mask(row, m)
        assert masks[m] == want_mask, "%s: fused_blocks %d, documented %d" % (tag, masks[m], want_mask)
        patch = torch.from_numpy(_G["%s/m%d:patch" % (rid, m)])
        b, kk = patch.shape[0], min(hp["k"], m)
        # (1) the reference's own feature-space neighbours forced: against the reference run
        force = _dev(np.stack([_G["%s/m%d:knn%d" % (rid, m, i)].astype(np.int32) for i in (1, 2, 3)]))
        assert tuple(force.shape) == (3, b, m, kk)
        used = torch.full_like(force, -1)
        d = fd(patch.to(U.dev()), taps={"knn": used}, knn_force=force)
        torch.cuda.synchronize()
        assert torch.equal(used, force), tag + ": forced tables not honoured"
        e_fix = float(np.abs(d.cpu().numpy() - _G["%s/m%d:dist" % (rid, m)]).max())
        # (2) the device's own tables: against the oracle on exactly those
        d_gpu, d_forced, d_free, flips, _ = U.fd_forward_forced(fd, sd, patch, hp)
        e_ora = float((d_gpu - d_forced).abs().max())
        print("%s: mask %d  |dist - reference run| %.3g (its neighbours forced)  |dist - oracle| %.3g (device's neighbours forced)  "
              "free-running: %d of %d rows with another neighbour set" % (tag, want_mask, e_fix, e_ora, sum(int(f.sum()) for f in flips), 3 * b * m))
        assert e_fix <= TOL and e_ora <= TOL, tag
        assert d_free.std() > 1e-2, tag
        # (3) the per-stage path through HBM, the first handle's neighbours forced: same bits
        assert stage.fused_blocks(m) == 0
        knn = torch.full((3, b, m, kk), -1, dtype=torch.int32, device=U.dev())
        ta = {"knn": knn, "enc": torch.full((b, emb), float("nan"), device=U.dev())}
        tb = {"enc": torch.full((b, emb), float("nan"), device=U.dev())}
        da = fd(patch.to(U.dev()), taps=ta)
        db = stage(patch.to(U.dev()), taps=tb, knn_force=knn)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(ta["enc"]).any())
        assert torch.equal(ta["enc"], tb["enc"]), tag + ": encoding differs from the SAPCU_FD_FUSED=0 handle (max %g)" % float((ta["enc"] - tb["enc"]).abs().max())
        assert torch.equal(da, db), tag + ": SAPCU_FD_FUSED=0 handle differs"
    for h in (fd, stage):
        assert h.gate_violations() == 0 and h.gemm_mode() == (True, 0), rid


@pytest.mark.parametrize("rid", ROWS, ids=ROWS)
def test_row_against_reference_run_and_oracle(rid, monkeypatch):
    row = U.hparam_row(_G, rid)
    (_check_fn if row["kind"] == "fn" else _check_fd)(row, monkeypatch)


def test_matrix_reaches_every_kernel_selection():
    """Guards the matrix against being trimmed into one that no longer leaves the default kernels: over the non-default rows the
    handles report a mixed fn mask, an all-zero fn mask, fd masks 1, 2 and 0, and the rows hold every scale count 1..4 (the four
    instances of fd_edge0_scalar_kernel) and one above 4 (the patch / thread-per-output kernels)."""
    fn_masks, fd_masks, scales = set(), set(), set()
    for rid in ROWS:
        row = U.hparam_row(_G, rid)
        assert row["kw"] != (FN_KW if row["kind"] == "fn" else FD_KW), rid + " is the default configuration"
        if rid not in _MASKS:                                   # (the row's own test did not run in this session)
            _record_masks(row, U.build_gpu_hparam_model(row)[0])
        for m, mask in _MASKS[rid].items():
            assert mask == _expected_mask(row, m), (rid, m)
            (fn_masks if row["kind"] == "fn" else fd_masks).add(mask)
        if row["kind"] == "fd":
            scales.add(len(row["kw"]["k_scales"]))
    assert any(mk not in (0, 0b111) for mk in fn_masks) and 0 in fn_masks, sorted(fn_masks)
    assert {0, 1, 2} <= fd_masks, sorted(fd_masks)
    assert {1, 2, 3, 4} <= scales and max(scales) > 4, sorted(scales)


# ---------------------------------------------------------------------------------------------- refusals at create
_FN0 = dict(k_values=[24, 18, 12], emb_dims=640, time_steps_enc=4, num_heads=8)
_FD0 = dict(k=32, emb_dims=768, time_steps_enc=4, num_heads=8, k_scales=[8, 16, 32, 48])
REFUSED = [("fn", "num_heads", 0), ("fn", "num_heads", 3), ("fn", "num_heads", 256), ("fn", "emb_dims", 0), ("fn", "emb_dims", 48),
           ("fn", "k_values", [24, 0, 12]), ("fn", "time_steps_enc", 0),
           ("fd", "num_heads", 0), ("fd", "num_heads", 3), ("fd", "num_heads", 128), ("fd", "k_scales", []),
           ("fd", "k_scales", [2, 4, 6, 8, 12, 16, 24, 32, 48]), ("fd", "k_scales", [8, 0, 32, 48]), ("fd", "k_scales", [8, 16, -1, 48]),
           ("fd", "k", 0), ("fd", "emb_dims", 48), ("fd", "time_steps_enc", 0), ("fd", "time_steps_enc", 65)]


@pytest.fixture(scope="module")
def default_blobs():
    """The packed default models on the device: a refusal comes back before the blob is looked at, and a create that wrongly went
    through would at least read memory that exists."""
    import sapcu_amd
    from sapcu_amd import packing
    out = {}
    for kind, cls, kw in (("fn", sapcu_amd.ImprovedSNNNormalEstimation, _FN0), ("fd", sapcu_amd.EnhancedSNNDistanceEstimation, _FD0)):
        model = cls(**kw)
        blob, d = model._pack(model.state_dict())
        out[kind] = (torch.from_numpy(blob).to(U.dev()), d)
    return out


@pytest.mark.parametrize("kind,name,value", REFUSED, ids=["%s-%s-%s" % (k, n, str(v).replace(" ", "")) for k, n, v in REFUSED])
def test_create_refuses(kind, name, value, default_blobs):
    """Hyper-parameters outside the ranges of include/sapcu.h: ValueError from the constructor; SAPCU_ERR_ARG, a NULL handle and a
    message from the raw sapcu_model_create — at create, never from inside a forward."""
    import sapcu_amd
    from sapcu_amd import _lib
    lib = _lib.load()
    kw = dict(_FN0 if kind == "fn" else _FD0, **{name: value})
    cls = sapcu_amd.ImprovedSNNNormalEstimation if kind == "fn" else sapcu_amd.EnhancedSNNDistanceEstimation
    with pytest.raises(ValueError):
        cls(**kw)
    if kind == "fn":
        hp = list(kw["k_values"]) + [kw["emb_dims"], kw["time_steps_enc"], kw["num_heads"]]
    else:
        hp = [kw["k"], kw["emb_dims"], kw["time_steps_enc"], kw["num_heads"], len(kw["k_scales"])] + list(kw["k_scales"])
    hp = np.asarray(hp, dtype=np.int32)
    blob, d = default_blobs[kind]
    handle = ctypes.c_void_p()
    rc = lib.sapcu_model_create(_lib.KIND_FN if kind == "fn" else _lib.KIND_FD, hp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), hp.size,
                                _lib.ptr(blob), blob.numel(), d.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), d.size, ctypes.byref(handle))
    if handle.value:
        lib.sapcu_model_destroy(handle)
    assert rc == -1, "sapcu_model_create returned %d for %s %s=%s" % (rc, kind, name, value)          # SAPCU_ERR_ARG
    assert not handle.value and b"model_create" in lib.sapcu_last_error()
