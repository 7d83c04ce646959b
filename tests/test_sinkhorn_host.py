"""Sinkhorn / EMD without a GPU: the numpy definition (tests/sinkhorn_ref.py) against the stored cases
(tests/golden/sinkhorn_cases.npz) and against the exact optimum, the binding's tenth table against include/sapcu_sinkhorn.h, the
refusals of the C entry points that come before any launch, and the argument errors of the Python layer that need no device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sinkhorn_ref as R
import abi_tables
from conftest import ROOT, golden

HEADER = os.path.join(ROOT, "include", "sapcu_sinkhorn.h")
_CACHE = {}


def header_entry_points():
    """{name: argument list} of include/sapcu_sinkhorn.h."""
    return abi_tables.header_entry_points("sapcu_sinkhorn.h")


def _cases():
    from sapcu_amd import sinkhorn
    if "cases" not in _CACHE:
        _CACHE["cases"] = R.build_cases(sinkhorn.split_plan)
    return _CACHE["cases"], golden("sinkhorn_cases.npz")


def _plain(case):
    if case["name"] not in _CACHE:
        _CACHE[case["name"]] = R.run_case(case, np.float64)
    return _CACHE[case["name"]]


# ------------------------------------------------------------------------------------------------ the definition
def test_the_f64_definition_reproduces_the_stored_file_within_the_stored_error():
    cases, g = _cases()
    assert list(g["names"]) == [c["name"] for c in cases] and len(cases) >= 30
    assert max(max(c["n"], c["m"]) for c in cases) <= 320 and max(c["iters"] for c in cases) <= 600
    for c in cases:
        truth = {k: g["%s/%s" % (c["name"], k)] for k in ("f", "g", "r", "c", "ot", "primal_cost")}
        assert truth["f"].shape == (c["n"],) and truth["g"].shape == (c["m"],) and truth["r"].shape == (c["n"],)
        err = R.errors(_plain(c), truth)
        stored = g[c["name"] + "/err"]
        for k, q in enumerate(R.QUANTITIES):
            assert err[q] <= stored[k], "%s: %s of the f64 definition is %.3e from the stored truth, stored error %.3e" % (c["name"], q, err[q], stored[k])
        assert all(np.all(np.isfinite(truth[k])) for k in truth)
        me = float(np.abs(truth["r"] - 1.0 / c["n"]).sum())
        assert abs(me - float(g[c["name"] + "/marginal_error"])) <= 1e-12 + 1e-9 * me


def test_the_cases_cover_every_tile_and_split_boundary_and_every_probe():
    from sapcu_amd import sinkhorn
    cases, g = _cases()
    tile, min_cols = sinkhorn.split_plan(100, 320)[:2]
    assert list(g["split"]) == [tile, min_cols], "the stored cases were chosen for other constants: run tests/golden/make_sinkhorn_cases.py"
    cols, edges = R.boundary_columns(sinkhorn.split_plan, 100)
    have = {c["m"] for c in cases if c["family"] == "boundary" and c["n"] == 100}
    assert tile in edges and len(edges) >= 3
    for e in edges:
        assert {e - 1, e, e + 1} <= have, (e, sorted(have))
    for rows, m in ((1, 1), (100, 1), (64, 10 ** 6), (10 ** 6, 10 ** 6), (1 << 24, 1 << 24)):                 # the plan itself
        t, mc, split, chunk = sinkhorn.split_plan(rows, m)
        assert split >= 1 and chunk % t == 0 and split * chunk >= m and (split - 1) * chunk < m, (rows, m, split, chunk)
    assert sinkhorn.split_plan(8192, 8192)[2] > 1 and sinkhorn.split_plan(100, 1)[2] == 1
    fam = {c["family"] for c in cases}
    assert fam == {"sandwich", "tiny", "wave", "boundary", "duplicates", "separated", "offset", "large-blur", "scaled"}
    by = {c["name"]: c for c in cases}
    x, y = R.case_inputs(by["same-p1"])
    assert np.array_equal(x, y) and R.sqdist(x, y).diagonal().max() == 0.0                                   # s = 0 under p = 1
    x, y = R.case_inputs(by["dup-p1"])
    assert (R.sqdist(x, y) == 0.0).sum() > 50 and (R.sqdist(x, x) == 0.0).sum() > len(x)
    x, y = R.case_inputs(by["far-p1"])
    assert R.sqdist(x, y).min() > 49.0 ** 2 and by["far-p1"]["blur"] == 0.01 and by["far-p2"]["blur"] == 0.01
    f = R.softmin(x, y, np.zeros(len(y)), 2, 1e-4)                                                          # every term but the maximum underflows
    arg = -R.cost(x, y, 2) / 1e-4
    assert np.array_equal(np.exp(arg - arg.max(1)[:, None]).sum(1), np.ones(len(x))) and np.all(np.isfinite(f))
    x, y = R.case_inputs(by["offset-p1"])
    assert x.min() > 999.0 and by["blur10-p1"]["blur"] == 10.0
    c = by["scaled-p1"]
    x, y = R.case_inputs(c)
    seq = R.eps_list(c["p"], c["blur"], c["iters"], c["scaling"], R.diameter(x, y))
    assert len(seq) > c["iters"] + 3 and seq[0] == R.diameter(x, y) and seq[-c["iters"] - 1] > seq[-1] == 0.05 and seq == sorted(seq, reverse=True)


def test_the_package_schedule_is_the_definitions():
    from sapcu_amd import sinkhorn
    for p in (1, 2):
        for blur, scaling, diam in ((0.05, 0.5, 1.9), (0.05, 0.9, 1.0), (0.01, 0.3, 57.3), (10.0, 0.5, 1.7), (0.5, 0.5, 0.5), (0.05, None, 2.0)):
            pre = sinkhorn.eps_schedule(diam, p, blur, scaling)
            assert pre + [blur ** p] * 4 == R.eps_list(p, blur, 4, scaling, diam)
            assert all(e > blur ** p for e in pre) and (scaling is not None or pre == [])
    assert sinkhorn.eps_schedule(1.7, 1, 10.0, 0.5) == []                                                    # D^p below the final eps already


# ------------------------------------------------------------------------------------------------ the sandwich
def test_the_primal_cost_lies_between_the_exact_optimum_and_the_entropy_bound():
    """EMD - delta <= primal_cost <= EMD + eps log(max(n, m)) + delta with delta = 4 marginal_error max C: the entropy of a
    coupling of uniform marginals lies in [log n, 2 log n], and delta is the cost of rounding a near-coupling to a coupling."""
    cases, g = _cases()
    sandwich = [c for c in cases if c["sandwich"]]
    assert [(c["p"], c["blur"] ** c["p"], c["n"], c["m"], c["iters"]) for c in sandwich] == [
        (1, 0.05, 96, 96, 200), (1, 0.02, 96, 96, 600), (2, 0.1 ** 2, 96, 96, 600), (1, 0.05, 64, 160, 300)]
    for c in sandwich:
        x, y = R.case_inputs(c)
        assert x.min() >= 0 and x.max() <= 1 and y.min() >= 0.05 and y.max() <= 1.05
        emd = R.exact_emd(x, y, c["p"])
        assert abs(emd - float(g[c["name"] + "/emd"])) <= 1e-12
        eps = c["blur"] ** c["p"]
        for who, fig in (("stored truth", {k: float(g["%s/%s" % (c["name"], k)]) for k in ("primal_cost", "marginal_error")}), ("f64 definition", _plain(c))):
            me, primal = float(fig["marginal_error"]), float(fig["primal_cost"])
            assert me <= 1e-9, (c["name"], who, me)
            delta = 4.0 * me * float(R.cost(x, y, c["p"]).max())
            print("%-24s %-14s emd %.6f primal %.6f gap %.4f bound %.4f marginal error %.1e" % (
                c["name"], who, emd, primal, primal - emd, eps * np.log(max(c["n"], c["m"])), me))
            assert emd - delta <= primal <= emd + eps * np.log(max(c["n"], c["m"])) + delta, (c["name"], who)


# ------------------------------------------------------------------------------------------------ header and exports
def test_the_header_declares_exactly_the_tenth_table():
    from sapcu_amd import _lib
    decl = header_entry_points()
    assert set(decl) == set(_lib.SINKHORN_EXPORTS) == {"sapcu_sinkhorn_workspace_bytes", "sapcu_softmin_f64", "sapcu_sinkhorn_f64",
                                                       "sapcu_plan_stats_f64"}
    for other in (_lib.EXPORTS, _lib.SEEDS_EXPORTS, _lib.FD_TRAIN_EXPORTS, _lib.FD_EDGECONV_EXPORTS, _lib.TRAIN_STEP_EXPORTS, _lib.METRICS_EXPORTS,
                  _lib.DATA_EXPORTS, _lib.MESH_EXPORTS, _lib.SURFACE_EXPORTS, tuple(_lib._INTERNAL_SIGNATURES)):
        assert not set(other) & set(_lib.SINKHORN_EXPORTS)
    lib = _lib.load()
    for name in _lib.SINKHORN_EXPORTS:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len([a for a in decl[name].split(",") if a.strip()]), name
    with open(os.path.join(ROOT, "include", "sapcu.h")) as f:
        assert "sinkhorn" not in f.read() and "softmin" not in decl.get("sapcu_abi_version", "") and _lib.ABI_VERSION == 2
    with open(HEADER) as f:
        head = f.read()
    for word in ("Memory contract", "only read", "written in full", "NO initialisation", "8-byte", "SAPCU_ERR_ARG", "never synchronised"):
        assert word in head, word


def test_the_sizer_and_the_refusals_before_any_launch():
    """Everything include/sapcu_sinkhorn.h promises to refuse is refused with SAPCU_ERR_ARG (-1) on a machine without a GPU too: the
    checks come before the first HIP call, and no device pointer is dereferenced."""
    from sapcu_amd import _lib
    lib = _lib.load()
    size = lib.sapcu_sinkhorn_workspace_bytes
    cap = 1 << 24
    assert size(0, 5) == -1 and size(5, 0) == -1 and size(-1, 5) == -1 and size(cap + 1, 5) == -1 and size(5, cap + 1) == -1
    assert size(1, 1) > 0 and size(cap, cap) > 0 and size(5000, 4097) > size(5000, 100) > 0 and size(300, 257) % 8 == 0
    assert size(300, 257) == size(257, 300)
    n, m = 300, 257
    need = size(n, m)
    P = ctypes.c_void_p
    x, y, pot, out, out2, ws = P(0x10000), P(0x20000), P(0x30000), P(0x40000), P(0x50000), P(0x60000)        # never dereferenced
    nan, inf = float("nan"), float("inf")
    sched = (ctypes.c_double * 2)(0.4, 0.1)

    def softmin(x=x, n=n, y=y, m=m, pot=pot, p=1, eps=0.05, out=out, ws=ws, nbytes=need):
        return lib.sapcu_softmin_f64(x, n, y, m, pot, p, eps, out, ws, nbytes, None)

    def loop(x=x, n=n, y=y, m=m, p=1, sched=sched, ns=2, eps=0.05, iters=3, f=out, g=out2, ws=ws, nbytes=need):
        return lib.sapcu_sinkhorn_f64(x, n, y, m, p, sched, ns, eps, iters, f, g, ws, nbytes, None)

    def stats(x=x, n=n, y=y, m=m, f=pot, g=pot, p=1, eps=0.05, r=out, c=out2, ws=ws, nbytes=need):
        return lib.sapcu_plan_stats_f64(x, n, y, m, f, g, p, eps, r, c, ws, nbytes, None)

    common = [dict(x=None), dict(n=0), dict(n=cap + 1), dict(m=0), dict(m=cap + 1), dict(p=0), dict(p=3), dict(eps=0.0), dict(eps=-0.05),
              dict(eps=nan), dict(eps=inf), dict(ws=None), dict(ws=P(0x60004)), dict(nbytes=need - 1), dict(nbytes=0)]
    for call, extra in ((softmin, [dict(y=None), dict(pot=None), dict(out=None)]),
                        (stats, [dict(y=None), dict(f=None), dict(g=None), dict(r=None), dict(c=None)]),
                        (loop, [dict(f=None), dict(g=None), dict(iters=-1), dict(ns=-1), dict(iters=(1 << 20) + 1), dict(sched=None),
                                dict(sched=(ctypes.c_double * 2)(0.4, 0.0)), dict(sched=(ctypes.c_double * 2)(nan, 0.1)),
                                dict(sched=(ctypes.c_double * 2)(0.4, inf)), dict(sched=(ctypes.c_double * 2)(-1.0, 0.1))])):
        for kw in common + extra:
            assert call(**kw) == -1, (call.__name__, kw)
            assert lib.sapcu_last_error()
    # the symmetric problem: y NULL, m ignored, the workspace of (n, n)
    assert loop(y=None, g=None, nbytes=size(n, n) - 1, m=0) == -1 and loop(y=None, g=None, f=None, nbytes=size(n, n)) == -1
    out4 = (ctypes.c_int64 * 4)()
    assert lib.sapcu_internal_sinkhorn_split(0, 5, out4) == -1 and lib.sapcu_internal_sinkhorn_split(5, 5, None) == -1


# ------------------------------------------------------------------------------------------------ argument errors
def test_sinkhorn_argument_errors_that_need_no_device():
    import sapcu_amd
    from sapcu_amd import sinkhorn
    assert sapcu_amd.sinkhorn_metrics is sinkhorn.sinkhorn_metrics and sapcu_amd.softmin is sinkhorn.softmin
    assert callable(sapcu_amd.sinkhorn_potentials) and callable(sapcu_amd.dataset_sinkhorn) and callable(sapcu_amd.evaluate_sinkhorn_file)
    ok = np.zeros((5, 3))
    calls = (lambda a, b, **kw: sinkhorn.sinkhorn_metrics(a, b, **kw), lambda a, b, **kw: sinkhorn.sinkhorn_potentials(a, b, **kw))
    for call in calls:
        for bad in (np.zeros((5, 2)), np.zeros((5,)), np.zeros((2, 5, 3)), np.zeros((0, 3)), np.zeros((5, 3), dtype=np.int64)):
            with pytest.raises(ValueError):
                call(bad, ok)
            with pytest.raises(ValueError):
                call(ok, bad)
        for v in (np.nan, np.inf, -np.inf):
            bad = np.zeros((5, 3))
            bad[3, 1] = v
            with pytest.raises(ValueError):
                call(bad, ok)
            with pytest.raises(ValueError):
                call(ok, bad.astype(np.float32))
        with pytest.raises(RuntimeError):
            call(torch.zeros(5, 3), ok)
        with pytest.raises(RuntimeError):
            call(ok, torch.zeros(5, 3, dtype=torch.float64))
        for kw in (dict(p=0), dict(p=3), dict(p=1.5), dict(p=True), dict(p="2"), dict(blur=0.0), dict(blur=-0.1), dict(blur=float("nan")),
                   dict(blur=float("inf")), dict(blur="x"), dict(blur=1e-200, p=2), dict(iters=-1), dict(iters=2.5), dict(iters=True),
                   dict(iters=(1 << 20) + 1), dict(scaling=0.0), dict(scaling=1.0), dict(scaling=1.5), dict(scaling=-0.5),
                   dict(scaling=float("nan"))):
            with pytest.raises(ValueError):
                call(ok, ok, **kw)
    for k in (0, -1, 6, 2.5, True):
        with pytest.raises(ValueError):
            sinkhorn.sinkhorn_metrics(ok, ok, downsample_gt=k)
    with pytest.raises(ValueError):
        sinkhorn.sinkhorn_potentials(np.zeros((5, 2)))
    with pytest.raises(RuntimeError):
        sinkhorn.sinkhorn_potentials(torch.zeros(5, 3))
    with pytest.raises(ValueError):
        sinkhorn.dataset_sinkhorn([])
    with pytest.raises(ValueError):
        sinkhorn.dataset_sinkhorn([(ok, ok)], p=5)
    for kw in (dict(p=3, eps=0.1), dict(p=1, eps=0.0), dict(p=1, eps=float("nan")), dict(p=2, eps=-1.0)):
        with pytest.raises(ValueError):
            sinkhorn.softmin(ok, ok, torch.zeros(5), **kw)
        with pytest.raises(ValueError):
            sinkhorn.plan_stats(ok, ok, torch.zeros(5), torch.zeros(5), **kw)
    with pytest.raises(RuntimeError):
        sinkhorn.softmin(torch.zeros(5, 3), ok, torch.zeros(5), 1, 0.1)
    with pytest.raises(ValueError):
        sinkhorn.softmin(np.zeros((5, 2)), ok, torch.zeros(5), 1, 0.1)
