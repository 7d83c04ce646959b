"""PCA normals and normal angles without a GPU: the binding's twelfth table against include/sapcu_normals.h, the refusals that come
before any launch, the numpy definition (tests/normals_ref.py) against LAPACK and against the reference's own output
(tests/golden/pca_normals.npz), exact cases, the angle mirror against the reference's function, and the host arithmetic of
``normal_metrics`` against numpy."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import normals_ref as R
import abi_tables
from conftest import GOLDEN, ROOT

HEADER = os.path.join(ROOT, "include", "sapcu_normals.h")
NAMES = {"sapcu_pca_normals_f64", "sapcu_normal_angles_f64"}
OTHER_HEADERS = ("sapcu.h", "sapcu_seeds.h", "sapcu_fd_train.h", "sapcu_fd_edgeconv.h", "sapcu_train_step.h", "sapcu_metrics.h",
                 "sapcu_data.h", "sapcu_mesh.h", "sapcu_surface.h", "sapcu_sinkhorn.h", "sapcu_ray.h")
EPS = 2.0 ** -52


def header_entry_points():
    """{name: argument list} of include/sapcu_normals.h."""
    return abi_tables.header_entry_points("sapcu_normals.h")


def test_the_header_declares_exactly_the_twelfth_table():
    from sapcu_amd import _lib
    decl = header_entry_points()
    assert set(decl) == set(_lib.NORMALS_EXPORTS) == NAMES
    others = (_lib.EXPORTS, _lib.SEEDS_EXPORTS, _lib.FD_TRAIN_EXPORTS, _lib.FD_EDGECONV_EXPORTS, _lib.TRAIN_STEP_EXPORTS,
              _lib.METRICS_EXPORTS, _lib.DATA_EXPORTS, _lib.MESH_EXPORTS, _lib.SURFACE_EXPORTS, _lib.SINKHORN_EXPORTS, _lib.RAY_EXPORTS)
    for other in others:
        assert not set(other) & NAMES
    for h in OTHER_HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            text = f.read()
        assert not any(name in text for name in NAMES), h
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len([a for a in decl[name].split(",") if a.strip()]), name
    assert _lib.ABI_VERSION == 2 and lib.sapcu_abi_version() == 2
    import sapcu_amd
    from sapcu_amd import normals
    for name in ("pca_normals", "normal_angles", "normal_metrics", "cloud_normal_metrics", "evaluate_normals_file"):
        assert getattr(sapcu_amd, name) is getattr(normals, name)
    with open(HEADER) as f:
        text = f.read()
    assert "#define SAPCU_PCA_NORMALS_MAX_K %d" % R.MAX_K in text and "#define SAPCU_PCA_NORMALS_SWEEPS %d" % R.SWEEPS in text
    assert normals.MAX_K == R.MAX_K


def test_the_refusals_before_any_launch():
    """Everything include/sapcu_normals.h promises to refuse is refused with SAPCU_ERR_ARG (-1) on a machine without a GPU too: the
    checks come before the first HIP call, and no pointer is dereferenced."""
    from sapcu_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    pts, idx, out, ev, bad, a, b, cos, deg = (P(0x10000 * k) for k in range(1, 10))               # never dereferenced
    view = (ctypes.c_double * 3)(0.0, 0.0, 0.0)

    def call(pts=pts, n=100, idx=idx, rows=10, k=16, view=None, out=out, ev=ev, bad=bad):
        return lib.sapcu_pca_normals_f64(pts, n, idx, rows, k, view, out, ev, bad, None)

    for kw in (dict(pts=None), dict(idx=None), dict(out=None), dict(bad=None), dict(k=2), dict(k=65), dict(k=0), dict(k=-1), dict(n=0),
               dict(n=-5), dict(rows=-1), dict(rows=(1 << 31) - 63), dict(pts=None, view=view)):
        assert call(**kw) == -1, kw
        assert b"pca_normals" in lib.sapcu_last_error()

    def call2(a=a, b=b, rows=10, oriented=0, eps=0.0, cos=cos, deg=deg):
        return lib.sapcu_normal_angles_f64(a, b, rows, oriented, eps, cos, deg, None)

    for kw in (dict(a=None), dict(b=None), dict(deg=None), dict(rows=-1), dict(rows=(1 << 31) - 63), dict(oriented=2), dict(oriented=-1),
               dict(eps=-1e-9), dict(eps=float("nan")), dict(eps=1.5), dict(eps=float("inf"))):
        assert call2(**kw) == -1, kw
        assert b"normal_angles" in lib.sapcu_last_error()
    assert call2(rows=0) == 0 and call2(rows=0, cos=None) == 0                                     # no row: nothing is launched


def test_the_python_refusals_before_the_device():
    from sapcu_amd import normals
    import torch
    p = R.shell(100)[0]
    for kw in (dict(points=p[:2]), dict(points=p, k=2), dict(points=p, k=65), dict(points=p[:, :2]), dict(points=p.astype(np.int64)),
               dict(points=np.where(np.arange(300).reshape(100, 3) == 7, np.nan, p)), dict(points=p, chunk_rows=0),
               dict(points=p, viewpoint=(0.0, 1.0)), dict(points=p, viewpoint=(0.0, 1.0, np.inf))):
        with pytest.raises(ValueError):
            normals.pca_normals(**kw)
    with pytest.raises(RuntimeError):
        normals.pca_normals(torch.from_numpy(p))                                                   # a CPU tensor: there is no CPU path
    with pytest.raises(ValueError):
        normals.normal_metrics(p, p, pred_points=p)


# ---------------------------------------------------------------------------------------------- the definition and LAPACK
def _against_lapack(c):
    """(worst sin / bound, worst r_mirror / (eps l2), worst r_eigh / (eps l2), rows compared) of the definition's smallest
    eigenvector against np.linalg.eigh's on the covariances c, with the two assertions of this comparison."""
    diag, v = R.jacobi(c)
    mine, evals = R.smallest(diag, v)
    w, ve = np.linalg.eigh(c)
    lam2 = w[:, 2]
    r_mine = R.residual(c, mine, evals[:, 0])
    r_eigh = R.residual(c, ve[:, :, 0], w[:, 0])
    with np.errstate(all="ignore"):
        take = (w[:, 1] - w[:, 0]) / lam2 >= 1e-6
    sin = R.sin_angle(mine, ve[:, :, 0])
    bound = (r_mine + r_eigh + 4 * EPS * lam2) / (w[:, 1] - w[:, 0])
    pos = lam2 > 0
    assert (r_mine[pos] <= 4 * EPS * lam2[pos]).all(), (r_mine[pos] / lam2[pos]).max() / EPS
    assert (sin[take] <= bound[take]).all(), (sin[take] / bound[take]).max()
    assert (np.abs(np.linalg.norm(mine, axis=1) - 1.0) < 8e-16).all()
    return (sin[take] / bound[take]).max(), (r_mine[pos] / lam2[pos]).max() / EPS, (r_eigh[pos] / lam2[pos]).max() / EPS, int(take.sum())


def test_the_definition_against_lapack_on_the_sweep_family():
    """The 20 000 covariances the sweep count was fixed on: Davis-Kahan for each vector plus the unit-length error bounds the sine of
    the angle between the two eigenvectors by (r_mirror + r_eigh + 4 eps l2) / (l1 - l0), the residuals in np.longdouble; the
    definition's own residual stays below 4 eps l2; and no pair rotates after the sixth sweep."""
    c = R.jacobi_family()
    count = []
    R.jacobi(c, count=count)
    assert count[6:] == [0, 0] and count[0] == len(c), count
    worst, mine, lapack, rows = _against_lapack(c)
    print("family: %d rows compared, worst sin / bound %.3f, residual %.2f eps l2 (LAPACK %.2f eps l2), rotating rows per sweep %s"
          % (rows, worst, mine, lapack, count))
    assert rows >= 0.999 * len(c)                      # (l1 - l0) / l2 >= 1e-6 holds for all but a row or two of the family


@pytest.mark.parametrize("name", ["shell300", "shell5000", "torus2000"])
def test_the_definition_against_lapack_on_the_fixture_clouds(name):
    case = R.fixture_case(name)
    worst, mine, lapack, rows = _against_lapack(case["cov"])
    print("%s: worst sin / bound %.3f, residual %.2f eps l2 (LAPACK %.2f eps l2)" % (name, worst, mine, lapack))
    assert rows == len(case["cov"])


@pytest.mark.parametrize("name", ["shell300", "shell5000", "torus2000"])
def test_the_definition_against_the_reference_script(name):
    """The normals scripts/generate_gt_normals.py saved (f32 centring, LAPACK, f32 storage) against the definition on the same f32
    points: sin(angle) <= 4 B 2^-23 l2 / (l1 - l0), B measured by the fixture's maker; no row is left out."""
    case = R.fixture_case(name)
    worst, left_out = R.check_against_script(case["normals"], case)
    print("%s: worst sin / bound %.3f (B = %.4f), %d rows left out" % (name, worst, case["B"], left_out))
    assert left_out == 0 and case["min_gap"] >= R.FIXTURE_GAP


def test_the_fixture_is_what_its_maker_makes():
    """tests/golden/make_normals_fixtures.py --check reruns the reference's scripts where they are installed."""
    sys.path.insert(0, GOLDEN)
    try:
        import make_normals_fixtures as maker
    finally:
        sys.path.remove(GOLDEN)
    if not (os.path.exists(maker.SCRIPT) and os.path.exists(maker.ANGLE_SCRIPT)):
        pytest.skip("the reference's scripts are not on this machine: the fixture cannot be rebuilt here")
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_normals_fixtures.py"), "--check"], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0 and "reproduced" in run.stdout, run.stdout


# --------------------------------------------------------------------------------------------------------- exact cases
def test_a_dyadic_plane_gives_exactly_the_z_axis():
    p = R.dyadic_plane()
    for k in (16, 64):                       # (3 neighbours of a lattice may be collinear: a second zero eigenvalue)
        normals, evals, bad = R.pca_normals(p, R.brute_knn(p, k))
        assert bad == 0 and np.array_equal(normals, np.tile([0.0, 0.0, 1.0], (len(p), 1))) and not np.signbit(normals).any()
        assert (evals[:, 0] == 0.0).all() and (evals[:, 1] <= evals[:, 2]).all()
        below = R.pca_normals(p, R.brute_knn(p, k), viewpoint=(0.5, 0.5, -3.0))[0]
        assert np.array_equal(below, np.tile([-0.0, -0.0, -1.0], (len(p), 1)))


def test_coincident_neighbours_give_a_zero_covariance_and_the_x_axis():
    p = R.tripled()
    normals, evals, _ = R.pca_normals(p, R.brute_knn(p, 3))
    assert np.array_equal(normals, np.tile([1.0, 0.0, 0.0], (len(p), 1))) and np.array_equal(evals, np.zeros((len(p), 3)))
    normals, _, _ = R.pca_normals(p, R.brute_knn(p, 3), viewpoint=(-9.0, 0.0, 0.0))
    assert np.array_equal(normals, np.tile([-1.0, -0.0, -0.0], (len(p), 1)))


def test_the_sign_rule_and_bad_indices():
    p, radial = R.shell(300)
    idx = R.brute_knn(p, 16)
    free, evals, _ = R.pca_normals(p, idx)
    big = np.abs(free).argmax(axis=1)
    assert (free[np.arange(300), big] > 0).all()
    out, _, _ = R.pca_normals(p, idx, viewpoint=(1e9, 1e9, 1e9))
    assert ((out * (1e9 - p)).sum(1) > 0).all() and np.array_equal(np.abs(out), np.abs(free))
    inward, _, _ = R.pca_normals(p, idx, viewpoint=(0.0, 0.0, 0.0))
    assert ((inward * radial).sum(1) < -0.9).all()
    assert (np.diff(evals, axis=1) >= 0).all()
    assert R.oriented(np.array([[-0.0, 0.0, 0.0], [-0.5, 0.5, 0.1], [0.5, -0.5, 0.1], [0.1, -0.5, -0.5]]), None).tolist() == \
        [[-0.0, 0.0, 0.0], [0.5, -0.5, -0.1], [0.5, -0.5, 0.1], [-0.1, 0.5, 0.5]]
    hurt = idx.copy()
    hurt[5, 3], hurt[9, 0], hurt[9, 15], hurt[299, 7] = -1, 300, -7, 1 << 40
    normals, evals2, bad = R.pca_normals(p, hurt)
    rows = np.array([5, 9, 299])
    keep = np.setdiff1d(np.arange(300), rows)
    assert bad == 4 and np.isnan(normals[rows]).all() and np.isnan(evals2[rows]).all()
    assert np.array_equal(normals[keep], free[keep]) and np.array_equal(evals2[keep], evals[keep])


# -------------------------------------------------------------------------------------------------------------- angles
def test_the_angle_mirror_is_the_script_bit_for_bit():
    with np.load(os.path.join(GOLDEN, "pca_normals.npz")) as d:
        a, b, want = d["angles/a"], d["angles/b"], d["angles/deg"]
    deg, cos = R.angles(a, b)
    assert np.array_equal(deg.view(np.int64), want.view(np.int64))
    zero = (np.abs(a).sum(1) == 0) | (np.abs(b).sum(1) == 0)
    assert zero.sum() == 40 and (deg[zero] == 90.0).all() and (cos[zero] == 0.0).all()
    assert (deg >= 0).all() and (deg <= 90.0).all()


def test_angles_of_equal_opposite_and_zero_rows():
    """The script divides by |x| + 1e-9, so two equal unit normals have the cosine (1 / (1 + 1e-9))^2 = 1 - 2e-9 and the angle
    acos(1 - 2e-9) = 0.0036 degrees, not 0: the definition keeps the script's arithmetic.  With the trainer's clamp the cosine of
    equal rows is 1 - 1e-6: 0.081 degrees."""
    rng = np.random.default_rng(2)
    a = rng.normal(size=(64, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    same, cos = R.angles(a, a)
    assert (same < 0.004).all() and (cos > 1 - 3e-9).all() and (cos < 1).all()
    assert (R.angles(a, -a)[0] < 0.004).all()
    opposite = R.angles(a, -a, True)[0]
    assert (opposite > 179.996).all() and (opposite <= 180.0).all()
    trainer = np.degrees(np.arccos(-(1.0 - 1e-6)))
    assert (R.angles(a, -a, True, 1e-6)[0] == trainer).all() and (R.angles(a, a, True, 1e-6)[0] == np.degrees(np.arccos(1.0 - 1e-6))).all()
    assert (R.angles(a * 0, a)[0] == 90.0).all() and (R.angles(a, a * 0, True, 1e-6)[0] == 90.0).all()
    hurt = a.copy()
    hurt[3, 1] = np.nan
    deg = R.angles(hurt, a)[0]
    assert np.isnan(deg[3]) and not np.isnan(np.delete(deg, 3)).any()


@pytest.mark.parametrize("n", [1, 2, 4096, 4097])
def test_the_host_arithmetic_of_normal_metrics_is_numpys(n):
    from sapcu_amd import normals
    ang = np.random.default_rng(n).uniform(0, 90, n)
    ang[: n // 3] = np.round(ang[: n // 3])                                                         # values on the thresholds
    ordered = np.sort(ang)
    thresholds = (5.0, 10.0, 20.0, 30.0)
    got = normals._host_figures(n, np.sum(ang), np.sum(ang * ang), ordered[(n - 1) // 2], ordered[n // 2],
                                [int((ang <= t).sum()) for t in thresholds])
    assert got["mean_deg"] == np.mean(ang) and got["median_deg"] == np.median(ang) and got["rms_deg"] == np.sqrt(np.mean(ang * ang))
    assert got["pgp"] == tuple(np.mean(ang <= t) for t in thresholds) and got["count"] == n
    assert all(type(got[key]) is np.float64 for key in ("mean_deg", "median_deg", "rms_deg")) and type(got["pgp"][0]) is np.float64
