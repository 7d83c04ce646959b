"""PCA normals and normal angles on the device (-m gpu; include/sapcu_normals.h, csrc/normals.hip, sapcu_amd/normals.py): bit for bit
against the numpy definition (tests/normals_ref.py) on the device's own neighbour tables, against the reference's output
(tests/golden/pca_normals.npz), the memory contract under guard bands, the refusals, the angles and ``normal_metrics``."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gpu_utils as U
import normals_ref as R
from guarded import Arena

pytestmark = pytest.mark.gpu

F64, I64, I32 = torch.float64, torch.int64, torch.int32


def _dev(x):
    return torch.as_tensor(np.array(x, order="C"), device=U.dev())          # a copy: the shared clouds are read-only


def _bits(t):
    return t.contiguous().view(I64)


def _same_bits(dev_tensor, array):
    return np.array_equal(dev_tensor.cpu().numpy().view(np.int64), np.ascontiguousarray(array).view(np.int64))


def _lib():
    from sapcu_amd import _lib
    return _lib


_CLOUDS = {}


def cloud(name):
    """The test clouds, made once per session (read only)."""
    if name not in _CLOUDS:
        make = {"shell300": lambda: R.shell(300)[0], "shell5000": lambda: R.shell(5000)[0], "plane": R.dyadic_plane,
                "tripled": R.tripled, "lattice": R.lattice, "collinear": R.collinear, "shifted": lambda: R.shell(5000)[0] + 1e6,
                "sixteen": lambda: R.shell(16, seed=3)[0]}[name]
        p = np.ascontiguousarray(make())
        p.setflags(write=False)
        _CLOUDS[name] = p
    return _CLOUDS[name]


# ------------------------------------------------------------------------------------------ 1. bit for bit: the definition
CASES = [(name, k) for name in ("shell300", "shell5000", "plane", "tripled", "lattice", "collinear", "shifted") for k in (3, 16, 64)]
CASES.append(("sixteen", 16))


@pytest.mark.parametrize("name,k", CASES)
def test_normals_equal_the_definition_bit_for_bit(name, k):
    """The device's own neighbour table goes to the kernel and to the numpy definition: normals and eigenvalues agree in every bit,
    without a viewpoint, with the centroid and with a viewpoint at 1e9."""
    from sapcu_amd import generation, normals
    p = cloud(name)
    pts = _dev(p)
    info = []
    idx, _ = generation.knn_self_grid(pts, k, info=info)
    if name in ("shell300", "shell5000"):
        assert info[0] == (1 if name == "shell5000" else 0)              # 300 points: the brute-force route; 5000: the grid
    table = idx.cpu().numpy()
    assert np.array_equal(p[table[:, 0]], p)                             # the row's own position comes first
    for view in (None, p.mean(axis=0), np.array([1e9, 1e9, 1e9])):
        got, evals = normals.normals_from_neighbours(pts, idx, viewpoint=view, return_evals=True)
        want, want_evals, bad = R.pca_normals(p, table, view)
        assert bad == 0
        assert _same_bits(got, want), (name, k, view)
        assert _same_bits(evals, want_evals), (name, k, view)
    free = normals.normals_from_neighbours(pts, idx).cpu().numpy()
    assert not np.isnan(free).any()
    if name in ("shell300", "shell5000") and k == 16:
        assert (np.abs(np.linalg.norm(free, axis=1) - 1.0) < 8e-16).all()      # not renormalised (tests/test_normals_host.py)
    if name == "plane" and k >= 16:
        assert np.array_equal(free, np.tile([0.0, 0.0, 1.0], (len(p), 1)))
    if name == "tripled" and k == 3:
        assert np.array_equal(free, np.tile([1.0, 0.0, 0.0], (len(p), 1)))
    if name in ("shell5000", "shifted") and k == 16:
        radial = R.shell(5000)[1]
        assert np.degrees(np.arccos(np.abs((free * radial).sum(1)).clip(0, 1))).mean() < 3.0


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257, 4097])
def test_row_ranges_at_a_row_offset(rows):
    from sapcu_amd import generation, normals
    p = cloud("shell5000")
    pts = _dev(p)
    r0 = 701
    idx, _ = generation.knn_self_grid(pts, 16, rows=(r0, r0 + rows))
    got, evals = normals.normals_from_neighbours(pts, idx, return_evals=True)
    assert got.shape == (rows, 3) and evals.shape == (rows, 3)
    want, want_evals, _ = R.pca_normals(p, idx.cpu().numpy())
    assert _same_bits(got, want) and _same_bits(evals, want_evals)
    whole = normals.pca_normals(pts, 16)
    assert torch.equal(_bits(whole[r0:r0 + rows]), _bits(got))


def test_the_result_does_not_depend_on_chunk_rows():
    from sapcu_amd import generation, normals
    p = cloud("shell5000")
    pts = _dev(p)
    view = (0.1, -0.2, 3.0)
    whole, whole_evals = normals.pca_normals(pts, 16, viewpoint=view, return_evals=True)
    for chunk in (64, 1000):
        got, evals = normals.pca_normals(pts, 16, viewpoint=view, chunk_rows=chunk, return_evals=True)
        assert torch.equal(_bits(got), _bits(whole)) and torch.equal(_bits(evals), _bits(whole_evals)), chunk
    idx, _ = generation.knn_self_grid(pts, 16)
    want, want_evals, _ = R.pca_normals(p, idx.cpu().numpy(), view)
    assert _same_bits(whole, want) and _same_bits(whole_evals, want_evals)
    # numpy input, f32 input, a strided tensor and k above n: the same checks and conversions as the metrics
    assert torch.equal(_bits(normals.pca_normals(p, 16, viewpoint=view)), _bits(whole))
    wide = torch.zeros((5000, 5), dtype=F64, device=U.dev())
    wide[:, 1:4] = pts
    assert torch.equal(_bits(normals.pca_normals(wide[:, 1:4], 16, viewpoint=view)), _bits(whole))
    p32 = p.astype(np.float32)
    assert torch.equal(_bits(normals.pca_normals(_dev(p32), 16)), _bits(normals.pca_normals(p32.astype(np.float64), 16)))
    small = cloud("sixteen")
    assert torch.equal(_bits(normals.pca_normals(small, 40)), _bits(normals.pca_normals(small, 16)))      # k_eff = min(k, n)
    with pytest.raises(ValueError):
        normals.pca_normals(p, 65)


# ---------------------------------------------------------------------------------------------- 2. against the reference
def test_the_device_against_the_reference_script():
    """The normals the reference's script saved for the 5000-shell against the device on the same f32 points, under the bound and
    the condition of tests/test_normals_host.py (the device equals the definition, so this one cloud is enough)."""
    from sapcu_amd import normals
    case = R.fixture_case("shell5000")
    got = normals.pca_normals(case["points"], case["k"]).cpu().numpy()
    worst, left_out = R.check_against_script(got, case)
    print("device against the script: worst sin / bound %.3f, %d rows left out" % (worst, left_out))
    assert left_out == 0


# --------------------------------------------------------------------------------------------------- 3. memory contract
def _pca_call(arena, p, table, want_evals=True):
    bufs = {"pts": arena.inp(p, name="pts"), "idx": arena.inp(table, name="idx"), "normals": arena.out(table.shape[:1] + (3,), F64, name="normals"),
            "evals": arena.out(table.shape[:1] + (3,), F64, name="evals"), "bad": arena.out((1,), I32, name="bad_count")}
    return bufs


def _pca_launch(b, view=None, want_evals=True, **over):
    L = _lib()
    lib = L.load()
    a = {"pts": L.ptr(b["pts"]), "n": b["pts"].shape[0], "idx": L.ptr(b["idx"]), "rows": b["idx"].shape[0], "k": b["idx"].shape[1],
         "normals": L.ptr(b["normals"]), "evals": L.ptr(b["evals"]) if want_evals else None, "bad": L.ptr(b["bad"])}
    a.update(over)
    host = None if view is None else (ctypes.c_double * 3)(*view)
    rc = lib.sapcu_pca_normals_f64(a["pts"], a["n"], a["idx"], a["rows"], a["k"], host, a["normals"], a["evals"], a["bad"], L.current_stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", ["shell5000-16", "shell300-64", "shell5000-3-no-evals", "bad-indices"])
def test_pca_normals_memory_contract_under_guard_bands(case):
    """Bands of 0xFF and of 0x00, outputs pre-filled with 0xFF and with 0x00: guards intact, outputs written in full and the same
    in every run, a NULL evals_out untouched, bad_count exact and the rows concerned NaN."""
    from sapcu_amd import generation
    name, k = case.split("-")[:2] if not case.startswith("bad") else ("shell300", "16")
    k = int(k)
    p = cloud(name)
    want_evals = "no-evals" not in case
    table = generation.knn_self_grid(_dev(p), k)[0].cpu().numpy()
    rows_hurt = np.array([], dtype=np.int64)
    if case == "bad-indices":
        table = table.copy()
        table[5, 3], table[9, 0], table[9, 15], table[299, 7], table[64, 1] = -1, 300, -7, 1 << 40, 300
        rows_hurt = np.array([5, 9, 64, 299])
    want, want_evals_arr, want_bad = R.pca_normals(p, table, (0.0, 0.0, 9.0))
    assert want_bad == (5 if case == "bad-indices" else 0)
    results = []
    for fill in (0xFF, 0x00):
        arena = Arena("guard", fill=fill, device=U.dev())
        bufs = _pca_call(arena, p, table)
        for prefill in (0xFF, 0x00):
            for g in arena.outs:
                g.fill_payload_bytes(prefill)
            rc = _pca_launch(bufs, (0.0, 0.0, 9.0), want_evals)
            assert rc == 0, _lib().load().sapcu_last_error()
            arena.check()
            results.append((prefill, bufs["normals"].clone(), bufs["evals"].clone(), int(bufs["bad"].item())))
    for prefill, got, evals, bad in results:
        assert bad == want_bad
        assert _same_bits(got, want)
        if want_evals:
            assert _same_bits(evals, want_evals_arr)
        else:
            assert bool((evals.view(torch.uint8) == prefill).all())                  # the buffer that was not passed is untouched
    if len(rows_hurt):
        got = results[0][1].cpu().numpy()
        assert np.isnan(got[rows_hurt]).all() and not np.isnan(np.delete(got, rows_hurt, axis=0)).any()


def test_no_row_launches_nothing_and_zeroes_the_count():
    p = cloud("shell300")
    arena = Arena("guard", fill=0xFF, device=U.dev())
    bufs = _pca_call(arena, p, np.zeros((4, 16), dtype=np.int64))
    assert _pca_launch(bufs, rows=0) == 0
    arena.check()
    assert int(bufs["bad"].item()) == 0
    for name in ("normals", "evals"):
        assert bool((bufs[name].view(torch.uint8) == 0xFF).all()), name


# ------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing():
    """Every refusal of include/sapcu_normals.h returns SAPCU_ERR_ARG with a text and leaves the pre-filled outputs, the count and
    the guards alone."""
    from sapcu_amd import generation
    p = cloud("shell300")
    table = generation.knn_self_grid(_dev(p), 16)[0].cpu().numpy()
    arena = Arena("guard", fill=0xFF, device=U.dev())
    bufs = _pca_call(arena, p, table)
    L = _lib()
    for over in (dict(pts=None), dict(idx=None), dict(normals=None), dict(bad=None), dict(k=2), dict(k=65), dict(n=0), dict(n=-1),
                 dict(rows=-1), dict(rows=(1 << 31) - 63)):
        assert _pca_launch(bufs, **over) == -1, over
        assert b"pca_normals" in L.load().sapcu_last_error()
        arena.check()
        for name in ("normals", "evals", "bad"):
            assert bool((bufs[name].view(torch.uint8) == 0xFF).all()), (over, name)
    assert _pca_launch(bufs) == 0 and int(bufs["bad"].item()) == 0                   # and the same buffers are accepted as they are
    arena.check()
    ang = Arena("guard", fill=0xFF, device=U.dev())
    a, b = ang.inp(p, name="a"), ang.inp(p[::-1].copy(), name="b")
    cos, deg = ang.out((300,), F64, name="cos"), ang.out((300,), F64, name="deg")
    lib = L.load()
    for args in ((None, L.ptr(b), 300, 0, 0.0, L.ptr(cos), L.ptr(deg)), (L.ptr(a), None, 300, 0, 0.0, L.ptr(cos), L.ptr(deg)),
                 (L.ptr(a), L.ptr(b), 300, 0, 0.0, L.ptr(cos), None), (L.ptr(a), L.ptr(b), -1, 0, 0.0, L.ptr(cos), L.ptr(deg)),
                 (L.ptr(a), L.ptr(b), 300, 2, 0.0, L.ptr(cos), L.ptr(deg)), (L.ptr(a), L.ptr(b), 300, 0, -0.5, L.ptr(cos), L.ptr(deg)),
                 (L.ptr(a), L.ptr(b), 300, 0, float("nan"), L.ptr(cos), L.ptr(deg)), (L.ptr(a), L.ptr(b), 300, 1, 1.5, L.ptr(cos), L.ptr(deg))):
        assert lib.sapcu_normal_angles_f64(*args, L.current_stream()) == -1, args
        assert b"normal_angles" in lib.sapcu_last_error()
        torch.cuda.synchronize()
        ang.check()
        assert bool((cos.view(torch.uint8) == 0xFF).all()) and bool((deg.view(torch.uint8) == 0xFF).all())
    with pytest.raises(ValueError):                                                   # the Python layer turns a bad table into an error
        from sapcu_amd import normals
        hurt = table.copy()
        hurt[3, 3] = 300
        normals.normals_from_neighbours(_dev(p), _dev(hurt))


def test_every_pointer_taking_entry_point_of_the_header_runs_under_guards():
    import test_normals_host as H
    decl = H.header_entry_points()
    assert set(decl) == set(_lib().NORMALS_EXPORTS)
    assert {n for n in decl if "*" in decl[n]} == {"sapcu_pca_normals_f64", "sapcu_normal_angles_f64"}    # _pca_launch, _angles_guarded


# ---------------------------------------------------------------------------------------------------------- 5. angles
ULPS = 8        # OpenCL's bound for acos (4 ulp) + numpy's own (1 ulp) + one rounding of the product with 180 / pi on either side


def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def _angle_tables(rows, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.normal(size=(rows, 3)), rng.normal(size=(rows, 3))
    a[::3] *= 10.0 ** rng.uniform(-6, 6, size=(len(a[::3]), 1))
    if rows >= 63:
        b[8:16] = a[8:16]
        b[16:24] = -a[16:24]
        a[24:28] = 0.0
        b[28:32] = 0.0
        a[40, 1] = np.nan
    return a, b


def _angles_guarded(a, b, oriented, eps, want_cos=True):
    L = _lib()
    results = []
    for fill in (0xFF, 0x00):
        arena = Arena("guard", fill=fill, device=U.dev())
        ta, tb = arena.inp(a, name="a"), arena.inp(b, name="b")
        cos, deg = arena.out((len(a),), F64, name="cos"), arena.out((len(a),), F64, name="deg")
        for g in arena.outs:
            g.fill_payload_bytes(fill)
        rc = L.load().sapcu_normal_angles_f64(L.ptr(ta), L.ptr(tb), len(a), oriented, eps, L.ptr(cos) if want_cos else None, L.ptr(deg),
                                              L.current_stream())
        torch.cuda.synchronize()
        assert rc == 0, L.load().sapcu_last_error()
        arena.check()
        if not want_cos:
            assert bool((cos.view(torch.uint8) == fill).all())
        results.append((cos.clone(), deg.clone()))
    assert torch.equal(_bits(results[0][1]), _bits(results[1][1]))
    if want_cos:
        assert torch.equal(_bits(results[0][0]), _bits(results[1][0]))
    return results[0][0].cpu().numpy(), results[0][1].cpu().numpy()


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("oriented,eps", [(0, 0.0), (1, 1e-6), (1, 0.0)])
def test_angles_against_the_definition(rows, oriented, eps):
    """cos_out equals the numpy definition in every bit; deg_out is within 8 ulp of it (the device's acos is not numpy's); a NaN
    stays one; a NULL cos_out is honoured; nothing is written beyond the outputs."""
    a, b = _angle_tables(rows, rows + oriented)
    cos, deg = _angles_guarded(a, b, oriented, eps)
    want_deg, want_cos = R.angles(a, b, bool(oriented), eps)
    assert np.array_equal(cos.view(np.int64), want_cos.view(np.int64))
    nan = np.isnan(want_deg)
    assert np.array_equal(np.isnan(deg), nan) and nan.sum() == (1 if rows >= 63 else 0)
    worst = _ulps(deg[~nan], want_deg[~nan]).max()
    print("rows %d oriented %d eps %g: deg within %.1f ulp" % (rows, oriented, eps, worst))
    assert worst <= ULPS
    _, deg2 = _angles_guarded(a, b, oriented, eps, want_cos=False)
    assert np.array_equal(deg2.view(np.int64), deg.view(np.int64))


def test_angles_of_equal_opposite_and_zero_rows():
    """Equal rows: the script's 1e-9 in the denominator leaves acos(1 - 2e-9) = 0.0036 degrees, not 0 (tests/test_normals_host.py);
    opposite rows: the same unoriented, 180 less that oriented; with the trainer's clamp, acos(-+(1 - 1e-6)); zero rows: 90."""
    from sapcu_amd import normals
    rng = np.random.default_rng(2)
    a = rng.normal(size=(64, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    d = lambda x, y, **kw: normals.normal_angles(_dev(x), _dev(y), **kw).cpu().numpy()
    for got, want in ((d(a, a), R.angles(a, a)[0]), (d(a, -a), R.angles(a, -a)[0]), (d(a, -a, oriented=True), R.angles(a, -a, True)[0]),
                      (d(a, -a, oriented=True, clamp_eps=1e-6), R.angles(a, -a, True, 1e-6)[0]),
                      (d(a, a, oriented=True, clamp_eps=1e-6), R.angles(a, a, True, 1e-6)[0]), (d(a * 0, a), R.angles(a * 0, a)[0]),
                      (d(a, a * 0, oriented=True, clamp_eps=1e-6), R.angles(a, a * 0, True, 1e-6)[0])):
        assert _ulps(got, want).max() <= ULPS
    assert (d(a, a) < 0.004).all() and (d(a, -a) < 0.004).all() and (d(a, -a, oriented=True) > 179.996).all()
    assert np.allclose(d(a, -a, oriented=True, clamp_eps=1e-6), np.degrees(np.arccos(-(1 - 1e-6))), rtol=1e-14, atol=0)
    assert np.allclose(d(a * 0, a), 90.0, rtol=1e-15, atol=0)
    deg, cos = normals.normal_angles(a.astype(np.float32), _dev(a), return_cos=True)          # numpy and f32 input
    assert deg.shape == (64,) and cos.shape == (64,) and bool((cos > 0.999999).all())
    assert normals.normal_angles(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)
    with pytest.raises(ValueError):
        normals.normal_angles(a, a[:5])


# ---------------------------------------------------------------------------------------------------- 6. normal_metrics
def _numpy_figures(ang, thresholds):
    return {"mean_deg": np.mean(ang), "median_deg": np.median(ang), "rms_deg": np.sqrt(np.mean(ang * ang)),
            "pgp": tuple(np.mean(ang <= t) for t in thresholds), "count": len(ang)}


def _assert_figures_equal(got, want, what):
    assert sorted(got) == sorted(want), what
    for key in want:
        g, w = got[key], want[key]
        if isinstance(w, tuple):
            assert isinstance(g, tuple) and len(g) == len(w) and all(x == y for x, y in zip(g, w)), (what, key, g, w)
        else:
            assert g == w, "%s: %s = %r, numpy %r" % (what, key, g, w)


@pytest.mark.parametrize("n", [1, 2, 8191, 8192, 20001])
def test_normal_metrics_equal_numpy_on_the_same_angles(n):
    from sapcu_amd import normals
    rng = np.random.default_rng(n)
    a, b = _dev(rng.normal(size=(n, 3))), _dev(rng.normal(size=(n, 3)))
    thresholds = (5.0, 10.0, 20.0, 30.0, 90.0)
    old = np.getbufsize()
    try:
        for oriented, eps in ((False, 0.0), (True, 1e-6)):
            ang = normals.normal_angles(a, b, oriented, eps).cpu().numpy()
            for bufsize in (old, 4096):
                np.setbufsize(bufsize)
                got = normals.normal_metrics(a, b, oriented=oriented, clamp_eps=eps, thresholds=thresholds)
                _assert_figures_equal(got, _numpy_figures(ang, thresholds), "n=%d bufsize=%d oriented=%s" % (n, bufsize, oriented))
    finally:
        np.setbufsize(old)
    assert got["count"] == n and type(got["mean_deg"]) is np.float64 and type(got["median_deg"]) is np.float64
    hurt = b.clone()
    hurt[0, 0] = float("nan")
    got = normals.normal_metrics(a, hurt, thresholds=thresholds)
    assert np.isnan(got["mean_deg"]) and np.isnan(got["median_deg"]) and got["pgp"][-1] == np.float64(n - 1) / n
    with pytest.raises(ValueError):
        normals.normal_metrics(a, b[: n - 1] if n > 1 else torch.zeros((2, 3), dtype=F64, device=U.dev()))


def test_the_position_match_and_the_cloud_figure(tmp_path):
    from sapcu_amd import metrics, normals
    import sapcu_amd
    gt_points, gt_normals = R.shell(5000)
    pred_points = R.shell(3000, seed=6)[0]
    pred = normals.pca_normals(pred_points, 16)
    got = normals.normal_metrics(pred, gt_normals, pred_points, gt_points)
    j = metrics.nearest(_dev(pred_points), _dev(gt_points))[1]
    by_hand = normals.normal_metrics(pred, _dev(gt_normals)[j])
    _assert_figures_equal(got, by_hand, "position match")
    assert got["count"] == 3000 and got["mean_deg"] < 3.0 and got["pgp"][1] > 0.95
    _assert_figures_equal(normals.cloud_normal_metrics(pred_points, gt_points, gt_normals, k=16), got, "cloud_normal_metrics")
    # the surface figure of the 5000-shell against its analytic radial normals: what the definition gives on the CPU
    whole = normals.cloud_normal_metrics(gt_points, gt_points, gt_normals, k=16)
    mirror = R.pca_normals(gt_points, R.brute_knn(gt_points, 16))[0]
    cpu_mean = np.mean(R.angles(mirror, gt_normals)[0])
    print("5000-shell: mean angle to the radial normals %.6f degrees on the device, %.6f by the definition on the CPU" % (whole["mean_deg"], cpu_mean))
    assert whole["mean_deg"] < cpu_mean + 1e-9 and whole["count"] == 5000
    with pytest.raises(ValueError):
        normals.normal_metrics(pred, gt_normals)                                     # 3000 against 5000 rows and no points
    with pytest.raises(ValueError):
        normals.normal_metrics(pred, gt_normals, pred_points[:10], gt_points)
    # files: the keys generate_gt_normals.py writes; the ground truth's normals under the first of normals / fn / gt_normals
    pred_npz, gt_npz, gt_fn = (os.path.join(str(tmp_path), f) for f in ("pred.npz", "gt.npz", "gt_fn.npz"))
    np.savez_compressed(pred_npz, points=pred_points.astype(np.float32), normals=pred.cpu().numpy().astype(np.float32))
    np.savez_compressed(gt_npz, points=gt_points.astype(np.float32), normals=gt_normals.astype(np.float32))
    np.savez_compressed(gt_fn, points=gt_points.astype(np.float32), gt_normals=-gt_normals.astype(np.float32),
                        fn=gt_normals.astype(np.float32))
    from_files = sapcu_amd.evaluate_normals_file(pred_npz, gt_npz)
    want = normals.normal_metrics(pred.cpu().numpy().astype(np.float32), gt_normals.astype(np.float32), pred_points.astype(np.float32),
                                  gt_points.astype(np.float32))
    _assert_figures_equal(from_files, want, "evaluate_normals_file")
    _assert_figures_equal(sapcu_amd.evaluate_normals_file(pred_npz, gt_fn), want, "the key fn comes before gt_normals")
    assert abs(from_files["mean_deg"] - got["mean_deg"]) < 0.05        # f32 points and normals: a few matches move
    oriented = sapcu_amd.evaluate_normals_file(pred_npz, gt_fn, oriented=True, clamp_eps=1e-6)
    assert oriented["count"] == 3000 and oriented["mean_deg"] >= from_files["mean_deg"]
