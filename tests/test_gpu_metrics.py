"""Cloud metrics on the device (-m gpu; include/sapcu_metrics.h, csrc/metrics.hip, sapcu_amd/metrics.py).

The nearest neighbour of every query in another cloud on the cell grid must equal the brute-force kernel bit for bit —
``generation.knn_gather(cloud, q, 1, want_dist=True, want_patch=False)`` is the reference throughout — for any cell size, for queries
anywhere (inside, outside, 1e12 extents away), for ties and duplicates (lowest index), on both routes; the entry point keeps the
memory contract of DESIGN §2 under guard bands; ``cloud_metrics`` equals numpy (``==``) on the device's own distances at two
buffer sizes, and every value the reference's evaluation script printed (tests/golden/cloud_metrics.npz)."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_utils as U
from conftest import golden
from guarded import Arena

pytestmark = pytest.mark.gpu

F64, I64 = torch.float64, torch.int64
_CACHE = {}


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(U.dev())


def _bits(t):
    return t.contiguous().view(I64) if t.dtype == F64 else t


def _reference(cloud, q):
    from sapcu_amd import generation as gen
    idx, dist, _ = gen.knn_gather(cloud, q, 1, want_dist=True, want_patch=False)
    return dist[:, 0], idx[:, 0]


def _assert_equal_to_brute_force(cloud, q, cell=0.0, grid=None, what=""):
    from sapcu_amd import metrics
    info = []
    d, i = metrics.nearest(q, cloud, cell, info)
    rd, ri = _reference(cloud, q)
    assert d.shape == rd.shape and d.dtype == F64 and i.dtype == I64
    bad = (_bits(d) != _bits(rd)) | (i != ri)
    assert not bool(bad.any()), "%s cell %g: %d of %d queries differ, first %d: (%r, %d) against brute force (%r, %d)" % (
        what, cell, int(bad.sum()), bad.numel(), int(bad.nonzero()[0]), d[bad][0].item(), i[bad][0].item(), rd[bad][0].item(),
        ri[bad][0].item())
    if grid is not None:
        assert info[0] == grid, (what, cell, info)
    return info


# ------------------------------------------------------------------------------------------------------ the clouds
def _cloud(name):
    if name in _CACHE:
        return _CACHE[name]
    rng = np.random.default_rng(["cube", "clusters", "plane", "triple", "lattice"].index(name) + 100)
    if name == "cube":
        c = rng.uniform(size=(20000, 3))
    elif name == "clusters":                                   # two clusters 500 apart: a long, mostly empty grid
        c = rng.normal(size=(16000, 3)) * 0.5
        c[8000:, 0] += 500.0
    elif name == "plane":                                      # constant z: gz = 1
        c = rng.uniform(size=(12000, 3))
        c[:, 2] = 0.25
    elif name == "triple":                                     # every point three times: the lowest index must win
        c = np.tile(rng.uniform(size=(4000, 3)), (3, 1))[rng.permutation(12000)]
    else:                                                      # a shuffled 24^3 lattice on dyadic coordinates: exact ties
        g = np.arange(24) * 0.125
        c = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(24 ** 3)]
    lo, hi = c.min(0), c.max(0)
    ext = (hi - lo).max()
    sets = {"self": c, "jitter": c + rng.normal(size=c.shape) * 0.01 * ext,
            "box": (lo + hi) / 2 + (rng.uniform(size=(20000, 3)) - 0.5) * 3 * ext}          # three times the bounding box
    if name == "lattice":                                      # the centres of the lattice cells: eight points at one distance
        sets["centres"] = c[:4000] + 0.0625
    for nq in (1, 63, 64, 65, 4097):
        sets["nq%d" % nq] = sets["jitter"][5:5 + nq]
    _CACHE[name] = (_dev(c), {k: _dev(v) for k, v in sets.items()}, float(ext))
    return _CACHE[name]


@pytest.mark.parametrize("name", ["cube", "clusters", "plane", "triple", "lattice"])
def test_equal_to_brute_force(name):
    from sapcu_amd import metrics
    cloud, sets, ext = _cloud(name)
    for cell in (0.0, 1e-9, 1e9, ext / 10):
        for sname, q in sets.items():
            info = _assert_equal_to_brute_force(cloud, q, cell, grid=1, what="%s/%s" % (name, sname))
            if name == "plane":
                assert info[3] == 1
            if cell == 1e9:
                assert info[1:] == [1, 1, 1]
    d, _ = metrics.nearest(sets["self"], cloud)
    assert float(d.max()) == 0.0                               # a cloud against itself: every distance is 0


def test_chunks_of_one_cell():
    """1000 queries inside one cell (sixteen chunks, the last one ragged), and cells that hold exactly 64 and 65 queries."""
    cloud, _, _ = _cloud("cube")
    rng = np.random.default_rng(7)
    q = np.concatenate([rng.uniform(0.26, 0.49, size=(1000, 3)), rng.uniform(0.51, 0.74, size=(64, 3)),
                        rng.uniform(0.76, 0.99, size=(65, 3))])
    q = q[rng.permutation(len(q))]
    info = _assert_equal_to_brute_force(cloud, _dev(q), 0.25, grid=1, what="chunks")
    assert info[1:] == [4, 4, 4]
    for part, count in ((q[(q > 0.25).all(1) & (q < 0.5).all(1)], 1000), (q[(q > 0.5).all(1) & (q < 0.75).all(1)], 64),
                        (q[(q > 0.75).all(1)], 65)):
        assert len(part) == count
        _assert_equal_to_brute_force(cloud, _dev(part), 0.25, grid=1, what="chunk of %d" % count)


def test_far_queries():
    """Queries 1e6, 1e9 and 1e12 away along every axis and diagonal (the slack must cover their magnitude), and a block of queries
    in the empty middle between two clusters."""
    cloud, _, _ = _cloud("cube")
    rng = np.random.default_rng(8)
    base = rng.uniform(size=(8, 3))
    dirs = [s * np.eye(3)[a] for a in range(3) for s in (1.0, -1.0)]
    dirs += [np.array([sx, sy, sz]) for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]
    dirs += [np.array([1.0, 1.0, 0.0]), np.array([0.0, -1.0, 1.0])]
    q = np.concatenate([base + d * s for s in (1e6, 1e9, 1e12) for d in dirs])
    for cell in (0.0, 0.05, 1e-9):
        _assert_equal_to_brute_force(cloud, _dev(q), cell, grid=1, what="far")
    clusters, _, _ = _cloud("clusters")
    mid = rng.normal(size=(500, 3)) * 20.0
    mid[:, 0] += 250.0
    for cell in (0.0, 2.0):
        _assert_equal_to_brute_force(clusters, _dev(mid), cell, grid=1, what="middle")


@pytest.mark.parametrize("n", [1, 2, 5, 70, 4095, 4096])
def test_small_sets(n):
    from sapcu_amd import metrics
    rng = np.random.default_rng(n)
    cloud = _dev(rng.uniform(size=(n, 3)))
    q = _dev(rng.uniform(-0.5, 1.5, size=(200, 3)))
    _assert_equal_to_brute_force(cloud, q, 0.0, grid=1 if n >= 4096 else 0, what="n=%d" % n)
    _assert_equal_to_brute_force(cloud, q, 0.1, grid=1, what="n=%d forced" % n)
    _assert_equal_to_brute_force(cloud, cloud, 0.3, grid=1, what="n=%d self" % n)
    info = [9]
    d, i = metrics.nearest(q[:0], cloud, 0.0, info)           # no query: nothing is launched
    assert d.shape == (0,) and i.shape == (0,) and d.dtype == F64 and i.dtype == I64 and info == [0, 0, 0, 0]


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 1e200])
def test_non_finite_and_huge_coordinates_take_the_brute_force_route(bad):
    cloud, sets, _ = _cloud("cube")
    q = sets["nq4097"]
    c2 = cloud.clone()
    c2[777, 1] = bad
    q2 = q.clone()
    q2[4000, 2] = bad
    for cell in (0.0, 0.05):
        _assert_equal_to_brute_force(c2, q, cell, grid=0, what="bad cloud")
        _assert_equal_to_brute_force(cloud, q2, cell, grid=0, what="bad query")
    _assert_equal_to_brute_force(cloud, q, 0.0, grid=1, what="clean")


# ------------------------------------------------------------------------------------------------- memory contract
def _lib():
    from sapcu_amd import _lib
    return _lib


def _call(arena, cloud, q, cell, want_idx, short=0, offset=8):
    """One call of the entry point on the arena's buffers; the workspace has exactly the sizer's size at an 8-byte aligned base."""
    L = _lib()
    lib = L.load()
    n, nq = cloud.shape[0], q.shape[0]
    nbytes = int(lib.sapcu_nn_cross_workspace_bytes(n, nq))
    assert nbytes > 0
    bufs = {"cloud": arena.inp(cloud, name="cloud"), "q": arena.inp(q, name="queries"), "dist": arena.out((nq,), F64, name="dist"),
            "idx": arena.out((nq,), I64, name="idx"), "ws": arena.ws(nbytes, offset=offset, name="workspace"), "nbytes": nbytes}
    return bufs, lambda: _launch(bufs, cell, want_idx)


def _launch(b, cell, want_idx, **over):
    L = _lib()
    lib = L.load()
    info = (ctypes.c_int64 * 4)(5, 5, 5, 5)
    a = {"cloud": L.ptr(b["cloud"]), "n": b["cloud"].shape[0], "q": L.ptr(b["q"]), "nq": b["q"].shape[0], "cell": float(cell),
         "dist": L.ptr(b["dist"]), "idx": L.ptr(b["idx"]) if want_idx else None, "ws": L.ptr(b["ws"]), "nbytes": b["nbytes"]}
    a.update(over)
    rc = lib.sapcu_nn_cross_grid_f64(a["cloud"], a["n"], a["q"], a["nq"], a["cell"], a["dist"], a["idx"], a["ws"], a["nbytes"], info,
                                     L.current_stream())
    torch.cuda.synchronize()
    return rc, list(info)


GUARD_CASES = {
    "grid": (5000, 4097 + 37, 0.0, True, None),
    "grid-no-idx": (5000, 1000, 0.0, False, None),
    "grid-forced-small": (70, 129, 0.2, True, None),
    "brute-small": (300, 200, 0.0, True, None),
    "brute-small-no-idx": (300, 200, 0.0, False, None),
    "brute-bad-query-no-idx": (5000, 300, 0.0, False, float("inf")),
}


@pytest.mark.parametrize("case", sorted(GUARD_CASES))
def test_memory_contract_under_guard_bands(case):
    """The three runs of DESIGN §2: 0xFF bands and workspace with NaN-prefilled outputs, 0x00 bands and workspace, the dirty
    workspace again — guards intact, outputs written in full and bit-identical, and identical to the compact call."""
    from sapcu_amd import metrics
    n, nq, cell, want_idx, bad = GUARD_CASES[case]
    rng = np.random.default_rng(n + nq)
    cloud, q = rng.uniform(size=(n, 3)), rng.uniform(-0.2, 1.2, size=(nq, 3))
    if bad is not None:
        q[nq // 2, 0] = bad
    results = []
    for fill in (0xFF, 0x00):
        arena = Arena("guard", fill=fill, device=U.dev())
        bufs, run = _call(arena, cloud, q, cell, want_idx)
        for again in range(2 if fill == 0x00 else 1):
            arena.refill_outputs()
            rc, info = run()
            assert rc == 0, _lib().load().sapcu_last_error()
            arena.check()
            results.append((bufs["dist"].clone(), bufs["idx"].clone(), info))
    d0, i0, info0 = results[0]
    assert info0[0] == (1 if (n >= 4096 or cell > 0) and bad is None else 0)
    for d, i, info in results[1:]:
        assert torch.equal(_bits(d), _bits(d0)) and torch.equal(i, i0) and info == info0
    cd, ci = metrics.nearest(_dev(q), _dev(cloud), cell)
    assert torch.equal(_bits(cd), _bits(d0))
    if want_idx:
        assert torch.equal(ci, i0)
    else:
        assert bool((i0 == -1).all())                          # a NULL idx_out: the buffer that was not passed is untouched
    if bad is None:
        assert not bool(torch.isnan(d0).any())


def test_refusals_launch_nothing():
    """Every refusal of include/sapcu_metrics.h returns SAPCU_ERR_ARG and leaves the NaN-prefilled outputs and the guards alone."""
    rng = np.random.default_rng(3)
    cloud, q = rng.uniform(size=(5000, 3)), rng.uniform(size=(300, 3))
    arena = Arena("guard", fill=0xFF, device=U.dev())
    bufs, _ = _call(arena, cloud, q, 0.0, True)
    L = _lib()
    wsp = bufs["ws"].data_ptr()
    refusals = [dict(cloud=None), dict(q=None), dict(dist=None), dict(n=0), dict(n=-5), dict(nq=-1), dict(n=(1 << 29) + 1),
                dict(nq=(1 << 31) - 63), dict(nbytes=bufs["nbytes"] - 1), dict(nbytes=0), dict(ws=None),
                dict(ws=ctypes.c_void_p(wsp + 4)), dict(ws=ctypes.c_void_p(wsp + 1)), dict(cell=-1.0), dict(cell=float("nan")),
                dict(cell=float("inf"))]
    for over in refusals:
        rc, info = _launch(bufs, over.pop("cell", 0.0), True, **over)
        assert rc == -1 and info == [5, 5, 5, 5], over
        assert L.load().sapcu_last_error()
        arena.check()
        for name in ("dist", "idx"):
            assert bool((bufs[name].view(torch.uint8) == 0xFF).all()), (over, name)
    assert bool((bufs["ws"] == 0xFF).all())
    rc, info = _launch(bufs, 0.0, True)                        # and the same buffers are accepted as they are
    assert rc == 0 and info[0] == 1
    arena.check()


def test_every_pointer_taking_entry_point_of_the_header_runs_under_guards():
    import test_metrics_host as H
    decl = H.header_entry_points()
    assert set(decl) == set(_lib().METRICS_EXPORTS)
    assert {n for n in decl if "*" in decl[n]} == {"sapcu_nn_cross_grid_f64"}        # _call / _launch above
    assert {n for n in decl if n.endswith("workspace_bytes")} == {"sapcu_nn_cross_workspace_bytes"}


# ------------------------------------------------------------------------------------------------------ statistics
def _numpy_figures(g2p, p2g, thresholds):
    with np.errstate(divide="ignore"):
        recall = tuple(np.mean(g2p <= t) for t in thresholds)
        precision = tuple(np.mean(p2g <= t) for t in thresholds)
        fscore = tuple(np.float64(0.0) if r == 0 or p == 0 else 2 / (1 / r + 1 / p) for r, p in zip(recall, precision))
    return {"gt2pre_mean": np.mean(g2p), "gt2pre_std": np.std(g2p), "gt2pre_max": np.max(g2p), "recall": recall,
            "pre2gt_mean": np.mean(p2g), "pre2gt_std": np.std(p2g), "pre2gt_max": np.max(p2g), "precision": precision,
            "cd": 0.5 * (np.mean(g2p) + np.mean(p2g)), "fscore": fscore, "hausdorff": max(np.max(g2p), np.max(p2g)),
            "n_gt": len(g2p), "n_pre": len(p2g)}


def _assert_figures_equal(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, tuple):
            assert isinstance(g, tuple) and len(g) == len(w) and all(a == b for a, b in zip(g, w)), (what, k, g, w)
        else:
            assert g == w, "%s: %s = %r, numpy %r" % (what, k, g, w)


@pytest.mark.parametrize("n", [1, 8191, 8192, 8193, 20000])
def test_cloud_metrics_equal_numpy_on_the_same_distances(n):
    from sapcu_amd import metrics
    rng = np.random.default_rng(n)
    pred, gt = _dev(rng.uniform(size=(n, 3))), _dev(rng.uniform(size=(n, 3)))
    g2p, p2g = metrics.nearest(gt, pred)[0].cpu().numpy(), metrics.nearest(pred, gt)[0].cpu().numpy()
    thresholds = (1e-2, 2e-2)
    old = np.getbufsize()
    try:
        for bufsize in (old, 4096):
            np.setbufsize(bufsize)
            got = metrics.cloud_metrics(pred, gt, thresholds)
            _assert_figures_equal(got, _numpy_figures(g2p, p2g, thresholds), "n=%d bufsize=%d" % (n, bufsize))
    finally:
        np.setbufsize(old)
    assert got["n_gt"] == n and got["n_pre"] == n and got["hausdorff"] >= got["gt2pre_max"] > 0
    if n >= 8191:
        assert 0 < got["recall"][0] < got["recall"][1] and got["fscore"][1] > 0
    # a threshold nothing meets: both rates 0, the F-score 0.0 and no exception
    none = metrics.cloud_metrics(pred, gt, (1e-12,))
    assert none["recall"] == (0.0,) and none["precision"] == (0.0,) and none["fscore"] == (0.0,)


# ---------------------------------------------------------------------------------------------------------- golden
def _pair_values(m):
    return np.array([m["gt2pre_mean"], m["gt2pre_std"], m["recall"][0], m["recall"][1], m["pre2gt_mean"], m["pre2gt_std"],
                     m["precision"][0], m["precision"][1], m["cd"], m["fscore"][0], m["fscore"][1]], dtype=np.float64)


def test_every_value_the_reference_script_printed():
    from sapcu_amd import metrics
    g = golden("cloud_metrics.npz")
    for name in g["pairs"]:
        m = metrics.cloud_metrics(g[name + "/pred"], g[name + "/gt"])
        got, want = _pair_values(m), g[name + "/values"]
        assert np.array_equal(got, want), "pair %s: %r against the script's %r" % (name, got, want)
        assert m["n_gt"] == len(g[name + "/gt"]) and m["n_pre"] == len(g[name + "/pred"])
    pooled = metrics.dataset_metrics([(g[n + "/pred"], g[n + "/gt"]) for n in g["pooled/order"]])
    assert np.array_equal(_pair_values(pooled), g["pooled/values"])
    assert pooled["n_gt"] == sum(len(g[n + "/gt"]) for n in g["pairs"])
    info = []
    d, _ = metrics.nearest(g["b/gt"], g["b/pred"], info=info)
    assert info[0] == 1 and np.array_equal(d.cpu().numpy(), g["b/gt2pre"])
    d, _ = metrics.nearest(g["b/pred"], g["b/gt"], info=info)
    assert info[0] == 1 and np.array_equal(d.cpu().numpy(), g["b/pre2gt"])
    metrics.nearest(g["c/gt"], g["c/pred"], info=info)
    assert info[0] == 0                                        # the small pair takes the brute-force route


# ---------------------------------------------------------------------------------------------------- Python layer
def test_python_layer_inputs_and_errors(tmp_path):
    import sapcu_amd
    from sapcu_amd import metrics
    rng = np.random.default_rng(21)
    pred, gt = rng.uniform(size=(5000, 3)), rng.uniform(size=(4500, 3))
    want = metrics.cloud_metrics(_dev(pred), _dev(gt))
    _assert_figures_equal(metrics.cloud_metrics(pred, gt), want, "numpy input")
    _assert_figures_equal(metrics.cloud_metrics(pred, _dev(gt)), want, "mixed input")
    wide = torch.zeros((5000, 7), dtype=F64, device=U.dev())
    wide[:, 2:5] = _dev(pred)
    _assert_figures_equal(metrics.cloud_metrics(wide[:, 2:5], _dev(gt).t().contiguous().t()), want, "non-contiguous input")
    p32, g32 = pred.astype(np.float32), gt.astype(np.float32)
    want32 = metrics.cloud_metrics(p32.astype(np.float64), g32.astype(np.float64))
    _assert_figures_equal(metrics.cloud_metrics(torch.from_numpy(p32).to(U.dev()), g32), want32, "f32 input")
    _assert_figures_equal(metrics.cloud_metrics(_dev(pred).half(), _dev(gt).half()),
                          metrics.cloud_metrics(_dev(pred).half().double(), _dev(gt).half().double()), "f16 input")
    assert want32["cd"] != want["cd"]
    with pytest.raises(RuntimeError):
        metrics.cloud_metrics(torch.from_numpy(pred), _dev(gt))
    with pytest.raises(RuntimeError):
        metrics.nearest(_dev(gt), torch.from_numpy(pred))
    for bad in (_dev(pred)[:, :2], _dev(pred)[:0], _dev(pred).reshape(-1), torch.zeros((4, 3), dtype=I64, device=U.dev())):
        with pytest.raises(ValueError):
            metrics.cloud_metrics(bad, _dev(gt))
        with pytest.raises(ValueError):
            metrics.cloud_metrics(_dev(pred), bad)
    for v in (float("nan"), float("inf")):
        x = _dev(pred)
        x[17, 2] = v
        with pytest.raises(ValueError):
            metrics.cloud_metrics(x, _dev(gt))
        with pytest.raises(ValueError):
            metrics.cloud_metrics(_dev(gt), x)
    with pytest.raises(ValueError):
        metrics.nearest(_dev(gt), _dev(pred)[:0])              # an empty cloud has no nearest point
    # files: the loader of process_file, the values of cloud_metrics on what it loads
    pp, gp = str(tmp_path / "pred.xyz"), str(tmp_path / "gt.xyz")
    np.savetxt(pp, pred, fmt="%.6f")
    np.savetxt(gp, gt, fmt="%.6f")
    m = sapcu_amd.pipeline.evaluate_file(pp, gp, device=str(U.dev()))
    _assert_figures_equal(m, metrics.cloud_metrics(np.loadtxt(pp), np.loadtxt(gp)), "evaluate_file")
    assert m["n_pre"] == 5000 and m["n_gt"] == 4500 and abs(m["cd"] - want["cd"]) < 1e-5
