"""Sinkhorn / EMD on the device (-m gpu; include/sapcu_sinkhorn.h, csrc/sinkhorn.hip, sapcu_amd/sinkhorn.py).

Accuracy.  Every case of tests/sinkhorn_ref.py::build_cases is compared with the "truth" of tests/golden/sinkhorn_cases.npz (the
numpy definition evaluated in np.longdouble and rounded to f64).  The bar is relative to what the f64 numpy definition itself
achieves on the same case and quantity (the stored ``err``; for the potentials it is max |f64 definition - truth| over f and g; the
two scalar figures are credited with at least the error of one term of their sum: sinkhorn_ref.credited_errors):

    max |device - truth|  <=  8 * err_np + 4 * ulp(max |truth|)

for the potentials, ``ot``, ``primal_cost`` and the row vectors r and c.  The factor 8 covers a device exp / log a couple of ulps
off where numpy's is within one, and another summation tree; the iteration is a contraction, so rounding does not accumulate over
the iterations.  ``softmin`` alone (one half-step on the stored g) has the same bar against the definition evaluated in the test.

Worst measured ratio  max |device - truth| / err_np  per case family (MI355X; the largest over the five quantities, cases whose
err_np is 0 left out; the test prints them):
    sandwich 2.1   tiny 1.0   wave 2.0   boundary 5.0   duplicates 18.3   separated 1.1   offset 1.25   large-blur 1.6   scaled 2.8
On the potentials alone the worst is 4.4 (cols-255), on r and c 2.1.  The two ratios of 5 and above are ``primal_cost`` figures on
which numpy happens to be within a fifth of an ulp (cols-256: device 8.7e-18 against 1.7e-18; dup-p1: 2.8e-17, two ulps, against
1.5e-18): they pass through the bar's 4 ulp term, not through the factor.  No case needs more than 8.

Also here: chunks of columns that receive no column (the forced-split hook), determinism and independence of the workspace's
content, the memory contract under guard bands (the three runs of DESIGN §2), every refusal of the header, graph capture of the whole
loop, the Python layer, and one 2048 x 2048 run."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_utils as U
import sinkhorn_ref as R
from conftest import golden
from guarded import Arena

pytestmark = pytest.mark.gpu

F64 = torch.float64
FAMILIES = ("sandwich", "tiny", "wave", "boundary", "duplicates", "separated", "offset", "large-blur", "scaled")
_CACHE = {}


def _sk():
    from sapcu_amd import sinkhorn
    return sinkhorn


def _L():
    from sapcu_amd import _lib
    return _lib


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(U.dev())


def _bits(t):
    return t.contiguous().view(torch.int64)


def _cases():
    if "cases" not in _CACHE:
        _CACHE["cases"] = R.build_cases(_sk().split_plan)
        _CACHE["gold"] = golden("sinkhorn_cases.npz")
    return _CACHE["cases"], _CACHE["gold"]


def _bar(err_np, truth):
    return 8.0 * err_np + 4.0 * R.ulp(np.max(np.abs(truth)))


def _device_run(case):
    """The case on the device through the Python layer: everything run_case returns, as f64 numpy."""
    S = _sk()
    x, y = R.case_inputs(case)
    xd, yd = _dev(x), _dev(y)
    f, g = S.sinkhorn_potentials(xd, yd, case["p"], case["blur"], case["iters"], case["scaling"])
    r, c = S.plan_stats(xd, yd, f, g, case["p"], float(case["blur"]) ** case["p"])
    f, g, r, c = (t.cpu().numpy() for t in (f, g, r, c))
    return {"f": f, "g": g, "r": r, "c": c, "ot": np.sum(f) / len(f) + np.sum(g) / len(g), "primal_cost": np.sum(c)}


def _compare(name, got, truth, err_np, worst):
    dev_err = R.errors(got, truth)
    for k, q in enumerate(R.QUANTITIES):
        t = np.concatenate([truth["f"], truth["g"]]) if q == "pot" else np.atleast_1d(truth[q])
        bar = _bar(err_np[k], t)
        ratio = dev_err[q] / err_np[k] if err_np[k] > 0 else float("nan")
        print("%-26s %-12s device %.3e  numpy %.3e  ratio %6.2f  bar %.3e" % (name, q, dev_err[q], err_np[k], ratio, bar))
        if err_np[k] > 0:
            worst[0] = max(worst[0], ratio)
        assert np.all(np.isfinite(got["f"])) and dev_err[q] <= bar, "%s: %s off by %.3e, bar %.3e (numpy itself %.3e, ratio %.2f)" % (
            name, q, dev_err[q], bar, err_np[k], ratio)


@pytest.mark.parametrize("family", FAMILIES)
def test_accuracy_against_the_stored_truth(family):
    cases, g = _cases()
    mine = [c for c in cases if c["family"] == family]
    assert mine, family
    worst = [0.0]
    for c in mine:
        truth = {k: g["%s/%s" % (c["name"], k)] for k in ("f", "g", "r", "c", "ot", "primal_cost")}
        _compare(c["name"], _device_run(c), truth, R.credited_errors(g[c["name"] + "/err"]), worst)
    print("family %s: worst ratio device / numpy %.2f over %d cases" % (family, worst[0], len(mine)))


def test_every_tile_and_split_boundary_is_among_the_cases():
    cases, g = _cases()
    S = _sk()
    tile, min_cols = S.split_plan(100, 320)[:2]
    assert list(g["split"]) == [tile, min_cols], "the stored cases were chosen for other constants: run tests/golden/make_sinkhorn_cases.py"
    assert list(g["names"]) == [c["name"] for c in cases]
    cols, edges = R.boundary_columns(S.split_plan, 100)
    have = {c["m"] for c in cases if c["family"] == "boundary" and c["n"] == 100}
    assert tile in edges and len(edges) >= 3, edges                       # the tile, and two changes of the number of chunks
    for e in edges:
        assert {e - 1, e, e + 1} <= have, (e, sorted(have))
        if e != tile:
            assert S.split_plan(100, e)[2] + 1 == S.split_plan(100, e + 1)[2]
    assert {(c["n"], c["m"]) for c in cases if c["family"] == "tiny"} == {(1, 1), (1, 300), (300, 1)}
    assert {c["n"] for c in cases if c["family"] == "wave"} == {63, 64, 65}


def _softmin_reference(case, g):
    x, y = R.case_inputs(case)
    pot = g[case["name"] + "/g"]
    eps = float(case["blur"]) ** case["p"]
    truth = np.asarray(R.softmin(x, y, pot, case["p"], eps, np.longdouble), dtype=np.float64)
    plain = R.softmin(x, y, pot, case["p"], eps)
    return x, y, pot, eps, truth, float(np.max(np.abs(plain - truth)))


@pytest.mark.parametrize("family", FAMILIES)
def test_softmin_alone(family):
    cases, g = _cases()
    for c in (c for c in cases if c["family"] == family):
        x, y, pot, eps, truth, err_np = _softmin_reference(c, g)
        out = _sk().softmin(_dev(x), _dev(y), _dev(pot), c["p"], eps).cpu().numpy()
        dev_err, bar = float(np.max(np.abs(out - truth))), _bar(err_np, truth)
        print("%-26s softmin device %.3e numpy %.3e bar %.3e" % (c["name"], dev_err, err_np, bar))
        assert out.shape == (c["n"],) and np.all(np.isfinite(out)) and dev_err <= bar, (c["name"], dev_err, bar, err_np)


def _forced(x, y, pot, p, eps, split, fill=0x00):
    L = _L()
    n, m = x.shape[0], y.shape[0]
    nbytes = (m + 2 * split * n) * 8
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=U.dev())
    out = torch.full((n,), float("nan"), dtype=F64, device=U.dev())
    rc = L.load().sapcu_internal_softmin_split_f64(L.ptr(x), n, L.ptr(y), m, L.ptr(pot), p, eps, split, L.ptr(out), L.ptr(ws), nbytes,
                                                   L.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, L.load().sapcu_last_error()
    return out


def test_chunks_without_a_column_and_any_number_of_chunks():
    """m = 1 cut into 2, 8 and 64 chunks (all but the first are empty: -inf partials), 300 columns into 64 chunks of one tile
    (59 empty), 257 columns into 3: every result within the bar of the truth; one chunk and the planned number agree bit for bit
    with the entry point."""
    cases, g = _cases()
    by = {c["name"]: c for c in cases}
    for name, splits in (("tiny-300x1-p1", (1, 2, 8, 64)), ("tiny-300x1-p2", (1, 64)), ("tiny-1x300-p1", (1, 2, 5, 64)), ("tiny-1x1-p2", (1, 7)),
                         ("cols-257", (1, 2, 3, 4, 5, 64))):
        c = by[name]
        x, y, pot, eps, truth, err_np = _softmin_reference(c, g)
        xd, yd, pd = _dev(x), _dev(y), _dev(pot)
        plain = _sk().softmin(xd, yd, pd, c["p"], eps)
        planned = _sk().split_plan(c["n"], c["m"])[2]
        for s in splits:
            for fill in (0x00, 0xFF):
                out = _forced(xd, yd, pd, c["p"], eps, s, fill)
                dev_err = float(np.max(np.abs(out.cpu().numpy() - truth)))
                assert bool(torch.isfinite(out).all()) and dev_err <= _bar(err_np, truth), (name, s, dev_err, err_np)
                if s == planned:
                    assert torch.equal(_bits(out), _bits(plain)), (name, s)


# ------------------------------------------------------------------------------------------------- memory contract
ENTRY = ("softmin", "sinkhorn", "symmetric", "stats")


def _buffers(arena, entry, x, y, offset=8):
    lib = _L().load()
    n, m = x.shape[0], y.shape[0]
    nbytes = int(lib.sapcu_sinkhorn_workspace_bytes(n, n if entry == "symmetric" else m))
    assert nbytes > 0 and nbytes % 8 == 0
    rng = np.random.default_rng(n * 1000 + m)
    b = {"x": arena.inp(x, offset=offset, name="x"), "y": arena.inp(y, offset=offset, name="y"), "n": n, "m": m, "nbytes": nbytes,
         "ws": arena.ws(nbytes, offset=offset, name="workspace")}
    if entry == "softmin":
        b["pot"] = arena.inp(rng.normal(size=m) * 0.1, offset=offset, name="pot_y")
        b["out"] = [arena.out((n,), F64, offset=offset, name="out")]
    elif entry == "stats":
        b["f"] = arena.inp(rng.normal(size=n) * 0.05, offset=offset, name="f")
        b["g"] = arena.inp(rng.normal(size=m) * 0.05, offset=offset, name="g")
        b["out"] = [arena.out((n,), F64, offset=offset, name="r"), arena.out((n,), F64, offset=offset, name="c")]
    elif entry == "sinkhorn":
        b["out"] = [arena.out((n,), F64, offset=offset, name="f"), arena.out((m,), F64, offset=offset, name="g")]
    else:
        b["out"] = [arena.out((n,), F64, offset=offset, name="f")]
    return b


def _launch(entry, b, p=1, eps=0.05, sched=(0.4, 0.1), iters=3, sync=True, **over):
    L = _L()
    lib = L.load()
    a = {"x": L.ptr(b["x"]), "y": L.ptr(b["y"]), "n": b["n"], "m": b["m"], "p": p, "eps": eps, "ws": L.ptr(b["ws"]), "nbytes": b["nbytes"],
         "iters": iters, "n_sched": 2 if sched is None else len(sched), "stream": L.current_stream(),
         "sched": None if sched is None else (ctypes.c_double * max(len(sched), 1))(*sched)}
    for k in ("pot", "f", "g"):
        if k in b:
            a[k] = L.ptr(b[k])
    for k, t in enumerate(b["out"]):
        a["out%d" % k] = L.ptr(t)
    a.update(over)
    if entry == "softmin":
        rc = lib.sapcu_softmin_f64(a["x"], a["n"], a["y"], a["m"], a["pot"], a["p"], a["eps"], a["out0"], a["ws"], a["nbytes"], a["stream"])
    elif entry == "stats":
        rc = lib.sapcu_plan_stats_f64(a["x"], a["n"], a["y"], a["m"], a["f"], a["g"], a["p"], a["eps"], a["out0"], a["out1"], a["ws"], a["nbytes"],
                                      a["stream"])
    elif entry == "sinkhorn":
        rc = lib.sapcu_sinkhorn_f64(a["x"], a["n"], a["y"], a["m"], a["p"], a["sched"], a["n_sched"], a["eps"], a["iters"], a["out0"], a["out1"],
                                    a["ws"], a["nbytes"], a["stream"])
    else:
        rc = lib.sapcu_sinkhorn_f64(a["x"], a["n"], None, 0, a["p"], a["sched"], a["n_sched"], a["eps"], a["iters"], a["out0"], None, a["ws"],
                                    a["nbytes"], a["stream"])
    if sync:
        torch.cuda.synchronize()
    return rc


def _clouds(n, m):
    rng = np.random.default_rng(n + 7 * m)
    return rng.uniform(size=(n, 3)), rng.uniform(size=(m, 3)) + 0.05


def _compact(entry, b, p, blur):
    """The same call through the Python layer on compact tensors (eps = blur ** p, three iterations behind the schedule of _launch)."""
    S = _sk()
    x, y = b["x"].clone(), b["y"].clone()
    if entry == "softmin":
        return [S.softmin(x, y, b["pot"].clone(), p, blur ** p)]
    if entry == "stats":
        return list(S.plan_stats(x, y, b["f"].clone(), b["g"].clone(), p, blur ** p))
    f, g = S._potentials(x, y if entry == "sinkhorn" else None, p, blur, 3, [0.4, 0.1])
    return [f, g] if entry == "sinkhorn" else [f]


@pytest.mark.parametrize("shape", [(300, 257, 1), (65, 130, 2), (1, 1, 1)])
@pytest.mark.parametrize("entry", ENTRY)
def test_memory_contract_under_guard_bands(entry, shape):
    """The three runs of DESIGN §2 at a base address that is 8 (mod 512), the workspace exactly the sizer's size: 0xFF bands and
    workspace with NaN-prefilled outputs, 0x00 bands and workspace, the dirty workspace again — guards intact, outputs written in
    full and bit-identical, and identical to the compact call through the Python layer."""
    n, m, p = shape
    x, y = _clouds(n, m)
    blur = 0.05 if p == 1 else 0.25
    results = []
    for fill in (0xFF, 0x00):
        arena = Arena("guard", fill=fill, device=U.dev())
        b = _buffers(arena, entry, x, y)
        for again in range(2 if fill == 0x00 else 1):
            arena.refill_outputs()
            rc = _launch(entry, b, p=p, eps=blur ** p)
            assert rc == 0, _L().load().sapcu_last_error()
            arena.check()
            results.append([t.clone() for t in b["out"]])
    for t in results[0]:
        assert bool(torch.isfinite(t).all())                                 # NaN-prefilled and written in full
    for other in results[1:]:
        for t0, t in zip(results[0], other):
            assert torch.equal(_bits(t0), _bits(t))
    for t0, t in zip(results[0], _compact(entry, b, p, blur)):
        assert torch.equal(_bits(t0), _bits(t)), entry


def test_refusals_launch_nothing():
    """Every refusal of include/sapcu_sinkhorn.h returns SAPCU_ERR_ARG and leaves the NaN-prefilled outputs and the guards alone."""
    x, y = _clouds(130, 70)
    nan, inf = float("nan"), float("inf")
    common = [dict(x=None), dict(n=0), dict(n=-3), dict(n=(1 << 24) + 1), dict(p=0), dict(p=3), dict(eps=0.0), dict(eps=-1.0), dict(eps=nan),
              dict(eps=inf), dict(ws=None), dict(nbytes=0), dict(out0=None)]
    with_y = [dict(y=None), dict(m=0), dict(m=(1 << 24) + 1)]
    loop = [dict(iters=-1), dict(n_sched=-1), dict(iters=(1 << 20) + 1), dict(sched=None), dict(sched=(ctypes.c_double * 2)(0.4, 0.0)),
            dict(sched=(ctypes.c_double * 2)(nan, 0.1)), dict(sched=(ctypes.c_double * 2)(0.4, inf)), dict(sched=(ctypes.c_double * 2)(-0.4, 0.1))]
    extra = {"softmin": with_y + [dict(pot=None)], "stats": with_y + [dict(f=None), dict(g=None), dict(out1=None)],
             "sinkhorn": [dict(m=0), dict(m=(1 << 24) + 1), dict(out1=None)] + loop, "symmetric": loop}
    for entry in ENTRY:
        arena = Arena("guard", fill=0xFF, device=U.dev())
        b = _buffers(arena, entry, x, y)
        wsp = b["ws"].data_ptr()
        refusals = common + extra[entry] + [dict(nbytes=b["nbytes"] - 1), dict(ws=ctypes.c_void_p(wsp + 4)), dict(ws=ctypes.c_void_p(wsp + 1))]
        for over in refusals:
            rc = _launch(entry, b, **dict(over))
            assert rc == -1 and _L().load().sapcu_last_error(), (entry, over)
            arena.check()
            for t in b["out"]:
                assert bool((t.view(torch.uint8) == 0xFF).all()), (entry, over)
        assert bool((b["ws"] == 0xFF).all())
        assert _launch(entry, b) == 0                                        # and the same buffers are accepted as they are
        arena.check()
        assert all(bool(torch.isfinite(t).all()) for t in b["out"])
    b = _buffers(Arena("guard", fill=0xFF, device=U.dev()), "sinkhorn", x, y)
    assert _launch("sinkhorn", b, iters=0, sched=()) == 0
    assert all(bool((t == 0).all()) for t in b["out"])                       # no iteration: the start f = g = 0, written in full


def test_every_pointer_taking_entry_point_of_the_header_runs_under_guards():
    import test_sinkhorn_host as H
    decl = H.header_entry_points()
    assert set(decl) == set(_L().SINKHORN_EXPORTS)
    assert {n for n in decl if "*" in decl[n]} == {"sapcu_softmin_f64", "sapcu_sinkhorn_f64", "sapcu_plan_stats_f64"}      # ENTRY above
    assert {n for n in decl if n.endswith("workspace_bytes")} == {"sapcu_sinkhorn_workspace_bytes"}


def test_two_runs_and_any_workspace_content_give_the_same_bits():
    x, y = _clouds(700, 900)
    out = {}
    for entry in ENTRY:
        for fill in (0xFF, 0x00, 0xFF):
            arena = Arena("compact", device=U.dev())
            b = _buffers(arena, entry, x, y, offset=0)
            b["ws"].fill_(fill)
            assert _launch(entry, b, p=2, eps=0.01, sched=(0.5, 0.1), iters=5) == 0
            got = [t.clone() for t in b["out"]]
            assert all(bool(torch.isfinite(t).all()) for t in got)
            if entry in out:
                assert all(torch.equal(_bits(a), _bits(c)) for a, c in zip(out[entry], got)), (entry, fill)
            out[entry] = got


def test_graph_capture_of_the_whole_loop_equals_the_eager_call():
    x, y = _clouds(500, 640)
    for entry in ("sinkhorn", "symmetric"):
        arena = Arena("compact", device=U.dev())
        b = _buffers(arena, entry, x, y, offset=0)
        assert _launch(entry, b, p=1, iters=6) == 0
        eager = [t.clone() for t in b["out"]]
        for t in b["out"]:
            t.fill_(float("nan"))
        b["ws"].fill_(0xFF)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = _launch(entry, b, p=1, iters=6, sync=False)                 # the capturing stream is the current one
        assert rc == 0, _L().load().sapcu_last_error()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in b["out"])            # captured, not run
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(_bits(a), _bits(c)) for a, c in zip(eager, b["out"])), entry
        del graph


# ---------------------------------------------------------------------------------------------------- Python layer
def test_metrics_equal_the_host_reduction_of_the_device_vectors():
    S = _sk()
    x, y = _clouds(1000, 9000)                                               # 9000 > numpy's 8192-element buffer: chunked sums
    xd, yd = _dev(x), _dev(y)
    for p, blur, scaling in ((1, 0.05, None), (2, 0.1, 0.5)):
        m = S.sinkhorn_metrics(xd, yd, p=p, blur=blur, iters=12, scaling=scaling, debias=True)
        f, g = S.sinkhorn_potentials(xd, yd, p, blur, 12, scaling)
        eps = blur ** p
        r, c = S.plan_stats(xd, yd, f, g, p, eps)
        f, g, r, c = (t.cpu().numpy() for t in (f, g, r, c))
        assert m["ot"] == np.sum(f) / 1000 + np.sum(g) / 9000 and m["primal_cost"] == np.sum(c)
        assert m["marginal_error"] == np.sum(np.abs(r - 1.0 / 1000)) and m["eps"] == eps and (m["n_pre"], m["n_gt"]) == (1000, 9000)
        sched = S.eps_schedule(R.diameter(x, y), p, blur, scaling)
        assert sched + [eps] * 12 == R.eps_list(p, blur, 12, scaling, R.diameter(x, y)) and (len(sched) > 0) == (scaling is not None)
        fa = S._potentials(xd, None, p, blur, 12, sched)[0].cpu().numpy()
        fb = S._potentials(yd, None, p, blur, 12, sched)[0].cpu().numpy()
        assert m["divergence"] == m["ot"] - 0.5 * (np.sum(fa) / 1000 + np.sum(fa) / 1000) - 0.5 * (np.sum(fb) / 9000 + np.sum(fb) / 9000)
        for k in ("ot", "primal_cost", "marginal_error", "divergence", "eps"):
            assert isinstance(m[k], np.float64), k
        plain = S.sinkhorn_metrics(x, y.astype(np.float32).astype(np.float64), p=p, blur=blur, iters=12, scaling=scaling, debias=False)
        assert plain["divergence"] is None
        mixed = S.sinkhorn_metrics(x, torch.from_numpy(y.astype(np.float32)).to(U.dev()), p=p, blur=blur, iters=12, scaling=scaling, debias=False)
        assert mixed == plain                                                # numpy and device inputs, f32 widened exactly


def _definition_divergence(x, y, p, blur, iters, wp):
    seq = R.eps_list(p, blur, iters)
    f, g = R.potentials(x, y, p, seq, wp)
    fa, fb = R.symmetric_potential(x, p, seq, wp), R.symmetric_potential(y, p, seq, wp)
    terms = [f.sum() / wp(len(f)) + g.sum() / wp(len(g)), wp(2) * fa.sum() / wp(len(fa)), wp(2) * fb.sum() / wp(len(fb))]
    return terms[0] - wp(0.5) * terms[1] - wp(0.5) * terms[2], terms


@pytest.mark.parametrize("p,blur", [(1, 0.2), (2, 0.5)])
def test_divergence_is_positive_and_zero_on_equal_clouds(p, blur):
    """Settings at which 200 iterations converge to the last bit (the definition in np.longdouble gives |divergence(x, x)| < 1e-19),
    so that the definition's own divergence is positive and the one of a cloud with itself 0.  The bar: 8 x the f64 definition's own
    error on the figure + 4 ulp of its largest term."""
    S = _sk()
    rng = np.random.Generator(np.random.PCG64(5))
    x, y = rng.uniform(size=(150, 3)), rng.uniform(size=(170, 3)) + 0.05
    for a, b in ((x, y), (x, x)):
        truth, terms = _definition_divergence(a, b, p, blur, 200, np.longdouble)
        plain, _ = _definition_divergence(a, b, p, blur, 200, np.float64)
        bar = 8.0 * float(abs(plain - truth)) + 4.0 * R.ulp(max(float(abs(t)) for t in terms))
        got = S.sinkhorn_metrics(a, b, p=p, blur=blur, iters=200)["divergence"]
        print("p=%d blur=%g %s: divergence %.3e, definition %.3e, |difference| %.3e, bar %.3e" % (
            p, blur, "x,y" if a is not b else "x,x", got, float(truth), abs(got - float(truth)), bar))
        assert got >= -bar and abs(got - float(truth)) <= bar
        if a is b:
            assert abs(float(truth)) < 1e-18 and abs(got) <= bar
        else:
            assert got > 1e-3


def test_downsample_dataset_and_files(tmp_path):
    import sapcu_amd
    from sapcu_amd import pipeline
    S = _sk()
    rng = np.random.default_rng(31)
    pred, gt = rng.uniform(size=(400, 3)), rng.uniform(size=(1500, 3))
    kw = dict(p=1, blur=0.05, iters=10)
    idx = pipeline.farthest_point_sample_device(_dev(gt).float(), 333)
    assert torch.equal(idx, S.downsampled_indices(_dev(gt), 333)) and int(idx[0]) == 1500 // 2 and len(set(idx.tolist())) == 333
    small = S.sinkhorn_metrics(pred, gt, downsample_gt=333, **kw)
    assert small == S.sinkhorn_metrics(pred, gt[idx.cpu().numpy()], **kw) and small["n_gt"] == 333
    assert S.sinkhorn_metrics(pred, gt, downsample_gt=1500, **kw)["n_gt"] == 1500
    full = S.sinkhorn_metrics(pred, gt, **kw)
    assert full["n_gt"] == 1500 and full != small
    # dataset: the per-pair dicts and their means in the order given
    pairs = [(pred, gt), (pred[:100], gt[:200]), (gt[:300], pred)]
    d = S.dataset_sinkhorn(pairs, **kw)
    assert d["pairs"] == [S.sinkhorn_metrics(a, b, **kw) for a, b in pairs] and d["pairs"][0] == full and d["mean"]["n_pairs"] == 3
    for k in ("ot", "primal_cost", "marginal_error", "divergence"):
        assert d["mean"][k] == np.sum(np.array([q[k] for q in d["pairs"]])) / 3, k
    assert S.dataset_sinkhorn(pairs[:1], debias=False, **kw)["mean"]["divergence"] is None
    with pytest.raises(ValueError):
        S.dataset_sinkhorn([])
    # files
    pp, gp = str(tmp_path / "pred.xyz"), str(tmp_path / "gt.xyz")
    np.savetxt(pp, pred, fmt="%.6f")
    np.savetxt(gp, gt, fmt="%.6f")
    m = sapcu_amd.evaluate_sinkhorn_file(pp, gp, device=str(U.dev()), **kw)
    assert m == S.sinkhorn_metrics(np.loadtxt(pp), np.loadtxt(gp), **kw) and (m["n_pre"], m["n_gt"]) == (400, 1500)
    assert abs(m["ot"] - full["ot"]) < 1e-5
    # device-side input errors
    bad = _dev(pred)
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError):
        S.sinkhorn_metrics(bad, gt, **kw)
    with pytest.raises(ValueError):
        S.sinkhorn_potentials(_dev(gt), bad)
    with pytest.raises(RuntimeError):
        S.sinkhorn_metrics(torch.from_numpy(pred), _dev(gt), **kw)


def test_one_larger_run():
    """2048 x 2048, p = 1, blur 0.05, 20 iterations: finite, reproducible, and the total mass of the plan.  After an iteration the
    column marginals are exact, so sum_i r_i = sum_j b_j = 1.  Bar (no definition at this size): every P_ij carries the relative
    error of its exponent (f_i + g_j - C_ij) / eps, in which each of the three terms is a few ulps off — f and g as computed (4 ulps
    of the sums behind them), C one — so at most 16 u (max |f| + max |g| + max C) / eps with u = 2^-53; g, which makes the columns
    exact, enters with the same error once more (factor 2); the m terms of a row are added in sequence (m u relative at worst) and
    the rows by numpy (pairwise)."""
    S = _sk()
    n = m = 2048
    x, y = _clouds(n, m)
    xd, yd = _dev(x), _dev(y)
    runs = []
    for _ in range(2):
        f, g = S.sinkhorn_potentials(xd, yd, 1, 0.05, 20)
        r, c = S.plan_stats(xd, yd, f, g, 1, 0.05)
        runs.append((f, g, r, c))
    assert all(bool(torch.isfinite(t).all()) for t in runs[0])
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs))
    f, g, r, c = (t.cpu().numpy() for t in runs[0])
    u = 2.0 ** -53
    bar = 32 * u * (np.abs(f).max() + np.abs(g).max() + np.sqrt(3.0) + 0.05) / 0.05 + (m + 64) * u
    mass = np.sum(r)
    print("2048 x 2048: |sum r - 1| = %.3e (bar %.3e), marginal error %.3e, primal cost %.6f" % (abs(mass - 1.0), bar, np.sum(np.abs(r - 1.0 / n)),
                                                                                           np.sum(c)))
    assert abs(mass - 1.0) <= bar
    assert 0.0 < np.sum(c) < np.sqrt(3.0) + 0.1 and bool((r > 0).all())
    assert S.split_plan(n, m)[2] > 1                                          # the columns were split across wavefronts
