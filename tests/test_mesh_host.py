"""Point-to-surface distance without a GPU: the binding's eighth table against include/sapcu_mesh.h, the sizer and the refusals of
the C entry point that come before any launch, the numpy definition (tests/mesh_ref.py) against the fixture of the reference's
CGAL tool (tests/golden/mesh_p2f.npz) and against exact rational arithmetic, regions, ties, skipped and duplicated faces, and the
OFF reader."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import mesh_ref as M
import abi_tables
from conftest import ROOT, golden

CASES = ("ico", "box", "sheet", "torus")


def header_entry_points():
    """{name: argument list} of include/sapcu_mesh.h."""
    return abi_tables.header_entry_points("sapcu_mesh.h")


def test_the_header_declares_exactly_the_eighth_table():
    from sapcu_amd import _lib
    decl = header_entry_points()
    assert set(decl) == set(_lib.MESH_EXPORTS) == {"sapcu_point_mesh_workspace_bytes", "sapcu_point_mesh_f64"}
    for other in (_lib.EXPORTS, _lib.SEEDS_EXPORTS, _lib.FD_TRAIN_EXPORTS, _lib.FD_EDGECONV_EXPORTS, _lib.TRAIN_STEP_EXPORTS,
                  _lib.METRICS_EXPORTS, _lib.DATA_EXPORTS):
        assert not set(other) & set(_lib.MESH_EXPORTS)
    lib = _lib.load()
    for name in _lib.MESH_EXPORTS:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len([a for a in decl[name].split(",") if a.strip()]), name
    for h in ("sapcu.h", "sapcu_metrics.h"):
        with open(os.path.join(ROOT, "include", h)) as f:
            assert "sapcu_point_mesh" not in f.read()
    assert _lib.ABI_VERSION == 2


def _r256(nbytes):
    return (nbytes + 255) & ~255


def restated_workspace_bytes(nf, nq):
    """The one layout of csrc/mesh_dist.hip (mesh_ws_layout over knn_grid.h's grid_ws_layout), every region rounded up to 256 bytes."""
    cap = 2 * nf + 64
    tiles = (cap + 1 + 1023) // 1024
    grid = lambda n: (_r256(8 * 256 * 8) + _r256(56) + _r256(4 * (cap + 1)) + _r256(4 * cap) + _r256(4 * tiles) + _r256(4 * n) +
                      3 * _r256(8 * n) + _r256(4 * n))
    faces_grid = grid(nf)
    queries_grid = grid(nq) - _r256(56)                          # the queries share the faces' grid parameters
    return faces_grid + queries_grid + _r256(8 * 256 * 8) + _r256(4 * (cap + 1)) + _r256(24 * nf) + _r256(8 * nf) + _r256(4 * nf) + 256


def test_the_sizer_and_the_refusals_before_any_launch():
    """Everything include/sapcu_mesh.h promises to refuse is refused with SAPCU_ERR_ARG (-1) on a machine without a GPU too: the
    checks come before the first HIP call, and no pointer is dereferenced."""
    from sapcu_amd import _lib
    lib = _lib.load()
    size = lib.sapcu_point_mesh_workspace_bytes
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, -1), (1 << 31, 5, 5), (5, (1 << 29) + 1, 5), (5, 5, (1 << 31) - 63)):
        assert size(*bad) == -1, bad
    assert size((1 << 31) - 1, 1, 0) > 0
    for nv, nf, nq in ((1, 1, 0), (8, 12, 2000), (2562, 5120, 8192), (50002, 100000, 385582), (7, 4097, 65)):
        assert size(nv, nf, nq) == restated_workspace_bytes(nf, nq), (nv, nf, nq)
        assert size(nv, nf, nq) == size(nv + 1000, nf, nq)       # the vertices take no workspace
    nv, nf, nq = 2562, 5120, 100
    need = size(nv, nf, nq)
    P = ctypes.c_void_p
    vs, fs, qs, dist, face, clo, ws = (P(0x10000 * k) for k in range(1, 8))             # never dereferenced
    info = (ctypes.c_int64 * 6)(7, 7, 7, 7, 7, 7)

    def call(vs=vs, nv=nv, fs=fs, nf=nf, qs=qs, nq=nq, cell=0.0, dist=dist, face=face, clo=clo, ws=ws, nbytes=need):
        return lib.sapcu_point_mesh_f64(vs, nv, fs, nf, qs, nq, cell, dist, face, clo, ws, nbytes, info, None)

    for kw in (dict(vs=None), dict(fs=None), dict(qs=None), dict(dist=None), dict(nv=0), dict(nf=0), dict(nv=1 << 31),
               dict(nf=(1 << 29) + 1), dict(nq=-1), dict(nq=(1 << 31) - 63), dict(nbytes=need - 1), dict(nbytes=0), dict(ws=None),
               dict(ws=P(0x70004)), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(cell=1e300)):
        assert call(**kw) == -1, kw
        assert lib.sapcu_last_error()
    assert list(info) == [7] * 6
    assert call(nq=0, qs=None, dist=None, face=None, clo=None) == 0 and list(info) == [0] * 6      # no query: nothing is launched


# ------------------------------------------------------------------------------------------------ the fixture
_REF = {}


def reference(name):
    """mesh_ref on every point of a fixture case, computed once per session and shared (tests/test_gpu_mesh.py uses it too)."""
    if name not in _REF:
        g = golden("mesh_p2f.npz")
        _REF[name] = M.point_mesh(g[name + "/points"], g[name + "/vertices"], g[name + "/faces"])
    return _REF[name]


def sample_std(d):
    return np.sqrt(np.sum((d - np.mean(d)) ** 2) / (len(d) - 1))


@pytest.mark.parametrize("name", CASES)
def test_the_definition_against_every_distance_the_reference_tool_wrote(name):
    """|sqrt(d2) - recorded| <= 1e-5 * recorded + 1e-12 on every point: six printed digits bound the difference by 5.06e-6 relative
    (half a unit of the sixth digit, plus the rounding to float), and 1e-5 is twice that.  Measured largest relative difference:
    ico 4.89e-6, box 4.63e-6, sheet 4.67e-6, torus 4.75e-6 (the four printed statistics: at most 7e-7)."""
    g = golden("mesh_p2f.npz")
    assert tuple(g["cases"]) == CASES
    dist, face, closest, region, skipped = reference(name)
    rec = g[name + "/dist"]
    assert dist.shape == rec.shape and skipped == 0 and int(g[name + "/n_faces"]) == len(g[name + "/faces"])
    assert (face >= 0).all() and np.isfinite(dist).all()
    err = np.abs(dist - rec)
    worst = int(np.argmax(err - 1e-5 * rec))
    print("%s: largest relative difference %.3g" % (name, float(np.max(err / np.maximum(rec, 1e-300)))))
    assert (err <= 1e-5 * rec + 1e-12).all(), (name, worst, dist[worst], rec[worst])
    mine = np.array([np.mean(dist), sample_std(dist), dist.min(), dist.max()])
    printed = g[name + "/stats"]
    print("%s: statistics %r against printed %r" % (name, mine, printed))
    assert (np.abs(mine - printed) <= 1e-5 * printed + 1e-12).all(), (name, mine, printed)
    # the closest point lies at the distance, and on the chosen face's plane side of things: |p - q| is the distance
    p = g[name + "/points"]
    assert np.allclose(np.linalg.norm(p - closest, axis=1), dist, rtol=1e-12, atol=1e-300)


def test_every_region_wins_and_ties_are_the_rule_in_the_box_case():
    g = golden("mesh_p2f.npz")
    dist, face, closest, region, _ = reference("box")
    wins = np.bincount(region, minlength=8)[1:]
    assert (wins >= 100).all(), wins
    dd, _ = M.all_d2(g["box/points"], g["box/vertices"], g["box/faces"])
    best = dd.min(1)
    tied = (dd == best[:, None]).sum(1)
    assert int((tied >= 2).sum()) >= 1000, int((tied >= 2).sum())
    assert np.array_equal(face, np.argmax(dd == best[:, None], axis=1))          # the lowest index of the tie set
    ico = reference("ico")
    assert int((ico[3] == 7).sum()) >= 8000                                       # near-surface points: the face interior


def _fr(x):
    return tuple(Fraction(float(v)) for v in x)


def _fdot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _fsub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def exact_d2(p, a, b, c):
    """The squared distance of p to the triangle in exact rational arithmetic (the same algorithm; exact predicates)."""
    ab, ac, ap = _fsub(b, a), _fsub(c, a), _fsub(p, a)
    d1, d2 = _fdot(ab, ap), _fdot(ac, ap)
    lin = lambda o, e, t: tuple(o[k] + t * e[k] for k in range(3))
    bp = _fsub(p, b)
    d3, d4 = _fdot(ab, bp), _fdot(ac, bp)
    cp = _fsub(p, c)
    d5, d6 = _fdot(ab, cp), _fdot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    if d1 <= 0 and d2 <= 0:
        q = a
    elif d3 >= 0 and d4 <= d3:
        q = b
    elif vc <= 0 and d1 >= 0 and d3 <= 0:
        q = lin(a, ab, d1 / (d1 - d3))
    elif d6 >= 0 and d5 <= d6:
        q = c
    elif vb <= 0 and d2 >= 0 and d6 <= 0:
        q = lin(a, ac, d2 / (d2 - d6))
    elif va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        q = lin(b, _fsub(c, b), (d4 - d3) / ((d4 - d3) + (d5 - d6)))
    else:
        den = va + vb + vc
        q = lin(lin(a, ab, vb / den), ac, vc / den)
    r = _fsub(p, q)
    return _fdot(r, r)


def test_exact_ties_on_an_integer_box_choose_the_lowest_face():
    """A cube of edge 4 on integer coordinates with integer queries: every difference, product and sum is an integer below 2^53, and
    every denominator (|edge|^2 = 16 or 32, |n|^2 = 256) a power of two, so all arithmetic of the definition is exact."""
    g = golden("mesh_p2f.npz")
    v, f = g["box/vertices"] * 4.0, g["box/faces"]
    rng = np.random.default_rng(5)
    q = rng.integers(-8, 13, size=(300, 3)).astype(np.float64)
    dist, face, closest, region, _ = M.point_mesh(q, v, f)
    ties = 0
    for i in range(len(q)):
        ex = [exact_d2(_fr(q[i]), _fr(v[t[0]]), _fr(v[t[1]]), _fr(v[t[2]])) for t in f]
        best = min(ex)
        tie_set = [k for k, e in enumerate(ex) if e == best]
        ties += len(tie_set) > 1
        assert face[i] == tie_set[0], (i, face[i], tie_set)
        assert Fraction(float(dist[i])) ** 2 == best or dist[i] == np.sqrt(float(best))
    assert ties >= 200 and len(set(region)) >= 6


def test_the_definition_against_exact_rational_arithmetic():
    """200 random well-shaped triangles (smallest angle >= 10 degrees) with queries at least 1e-3 triangle sizes away: the largest
    relative error of d2 measured on the CPU is 2.69e-13 (seed 9); four times that is asserted.  (It is far above 1e-16 because a
    triangle of size 0.01 near a point of magnitude 1 with a query 1e-5 away loses the digits of the magnitude in p - q: the error is
    absolute, a few units in the last place of the COORDINATES, which is what the grid route's slack is sized to.)"""
    rng = np.random.default_rng(9)
    worst, done = 0.0, 0
    while done < 200:
        tri = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-2, 2) + rng.normal(size=3)
        e = [tri[1] - tri[0], tri[2] - tri[1], tri[0] - tri[2]]
        ang = [np.arccos(np.clip(np.dot(-e[k - 1], e[k]) / (np.linalg.norm(e[k - 1]) * np.linalg.norm(e[k])), -1, 1)) for k in range(3)]
        size = max(np.linalg.norm(x) for x in e)
        if min(ang) < np.radians(10.0):
            continue
        p = tri[rng.integers(3)] + rng.normal(size=3) * size * 10.0 ** rng.uniform(-2, 1)
        _, dd, _ = M.closest_point(p, tri[0], tri[1], tri[2])
        ex = exact_d2(_fr(p), _fr(tri[0]), _fr(tri[1]), _fr(tri[2]))
        if float(ex) < (1e-3 * size) ** 2:
            continue
        worst = max(worst, abs(float((Fraction(float(dd)) - ex) / ex)))
        done += 1
    print("largest relative error of d2 against exact arithmetic: %.3g" % worst)
    assert worst <= 4 * 2.69e-13, worst


def test_skipped_and_duplicated_faces():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 1], [1, 1, 1.0]])
    f = np.array([[0, 1, 3],        # collinear
                  [0, 0, 2],        # a repeated vertex
                  [1, 1, 1],        # a point
                  [0, 1, 6],        # an index out of range
                  [0, -1, 2],       # a negative index
                  [0, 1, 2],        # the first real face
                  [0, 1, 2],        # its duplicate: the lower index wins
                  [1, 0, 2],        # the same triangle in another order
                  [0, 1, 4]])
    assert list(M.valid_faces(v, f)) == [False] * 5 + [True] * 4
    q = np.array([[0.25, 0.25, -0.5], [3.0, 0.0, 0.0], [0.2, -1.0, 0.2], [np.nan, 0.0, 0.0]])
    dist, face, closest, region, skipped = M.point_mesh(q, v, f)
    assert skipped == 5
    assert list(face) == [5, 5, 8, -1] and np.isnan(dist[3]) and np.isnan(closest[3]).all() and region[3] == 0
    assert dist[0] == 0.5 and np.array_equal(closest[0], [0.25, 0.25, 0.0]) and dist[1] == 2.0 and np.array_equal(closest[1], v[1])
    # the collinear face [0, 1, 3] would have put (3, 0, 0) at distance 1: it takes no part
    dist, face, closest, region, skipped = M.point_mesh(q, v, f[:5])
    assert skipped == 5 and (face == -1).all() and np.isnan(dist).all() and np.isnan(closest).all()
    big = np.array([[0, 0, 0], [1e200, 0, 0], [0, 1e200, 0.0]])
    assert list(M.valid_faces(big, np.array([[0, 1, 2]]))) == [False]              # dot(n, n) overflows


# ------------------------------------------------------------------------------------------------ the OFF reader
TRI = "0 0 0\n1 0 0\n0 1 0\n0 0 1\n"


def test_read_off_accepted_and_refused_forms(tmp_path):
    from sapcu_amd import mesh
    import sapcu_amd
    assert sapcu_amd.read_off is mesh.read_off and callable(sapcu_amd.point_to_mesh) and callable(sapcu_amd.mesh_metrics)
    assert callable(sapcu_amd.mesh_dataset_metrics) and callable(sapcu_amd.evaluate_mesh_file)
    want_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]])
    want_f = np.array([[0, 1, 2], [0, 3, 1]])
    accepted = {
        "same-line": "OFF 4 2 0\n" + TRI + "3 0 1 2\n3 0 3 1\n",
        "next-line": "OFF\n4 2 0\n" + TRI + "3 0 1 2\n3 0 3 1\n",
        "comments": "# a mesh\nOFF # header\n\n4 2 0 # counts\n\n" + TRI.replace("1 0 0\n", "1 0 0 # x\n\n") + "3 0 1 2\n# last\n3 0 3 1\n\n",
        "colours": "OFF\n4 2 5\n" + TRI + "3 0 1 2 255 0 0\n3  0 3 1  0.5 0.5 0.5 1.0\n",
        "no-edge-count": "OFF\n4 2\n" + TRI + "3 0 1 2\n3 0 3 1\n",
        "exponents": "OFF\n4 2 0\n0 0 0\n1e0 0 0\n0 1.0E+0 0\n0 0 1\n3 0 1 2\n3 0 3 1",
    }
    for name, text in accepted.items():
        p = tmp_path / (name + ".off")
        p.write_text(text)
        v, f = mesh.read_off(str(p))
        assert v.dtype == np.float64 and f.dtype == np.int64 and np.array_equal(v, want_v) and np.array_equal(f, want_f), name
    refused = {
        "quad": "OFF\n4 1 0\n" + TRI + "4 0 1 2 3\n",
        "truncated-faces": "OFF\n4 2 0\n" + TRI + "3 0 1 2\n",
        "truncated-vertices": "OFF\n4 2 0\n0 0 0\n",
        "truncated-face-line": "OFF\n4 2 0\n" + TRI + "3 0 1 2\n3 0 3\n",
        "short-vertex": "OFF\n4 2 0\n0 0\n1 0 0\n0 1 0\n0 0 1\n3 0 1 2\n3 0 3 1\n",
        "too-many-faces": "OFF\n4 1 0\n" + TRI + "3 0 1 2\n3 0 3 1\n",
        "no-counts": "OFF\n",
        "bad-counts": "OFF\nfour two\n",
        "not-off": "PLY\n4 2 0\n",
        "empty": "",
        "bad-number": "OFF\n4 2 0\n" + TRI.replace("1 0 0", "1 x 0") + "3 0 1 2\n3 0 3 1\n",
    }
    for name, text in refused.items():
        p = tmp_path / (name + ".off")
        p.write_text(text)
        with pytest.raises(ValueError):
            mesh.read_off(str(p))
    g = golden("mesh_p2f.npz")
    p = tmp_path / "sheet.off"
    with open(str(p), "w") as out:
        out.write("OFF\n%d %d 0\n" % (len(g["sheet/vertices"]), len(g["sheet/faces"])))
        out.writelines("%.17g %.17g %.17g\n" % tuple(r) for r in g["sheet/vertices"])
        out.writelines("3 %d %d %d\n" % tuple(r) for r in g["sheet/faces"])
    v, f = mesh.read_off(str(p))
    assert np.array_equal(v, g["sheet/vertices"]) and np.array_equal(f, g["sheet/faces"])


def test_argument_errors_that_need_no_device():
    from sapcu_amd import mesh
    v, f, p = np.zeros((4, 3)), np.array([[0, 1, 2]]), np.zeros((5, 3))
    for bad in (np.zeros((5, 2)), np.zeros((5,)), np.zeros((2, 5, 3)), np.zeros((5, 3), dtype=np.int64)):
        with pytest.raises(ValueError):
            mesh.point_to_mesh(bad, v, f)
        with pytest.raises(ValueError):
            mesh.point_to_mesh(p, bad, f)
        with pytest.raises(ValueError):
            mesh.mesh_metrics(bad, v, f)
    for bad in (np.zeros((1, 4), dtype=np.int64), np.zeros((3,), dtype=np.int64), np.zeros((1, 3)), np.zeros((0, 3), dtype=np.int32)):
        with pytest.raises(ValueError):
            mesh.point_to_mesh(p, v, bad)
    with pytest.raises(ValueError):
        mesh.point_to_mesh(p, np.zeros((0, 3)), f)
    with pytest.raises(ValueError):
        mesh.mesh_metrics(np.zeros((0, 3)), v, f)
    for val in (np.nan, np.inf):
        x = np.zeros((5, 3))
        x[2, 1] = val
        with pytest.raises(ValueError):
            mesh.mesh_metrics(x, v, f)
        with pytest.raises(ValueError):
            mesh.mesh_metrics(p, x[:4], f)
    for args in ((torch.zeros(5, 3), v, f), (p, torch.zeros(4, 3, dtype=torch.float64), f), (p, v, torch.zeros(1, 3, dtype=torch.int64))):
        with pytest.raises(RuntimeError):
            mesh.point_to_mesh(*args)
    with pytest.raises(ValueError):
        mesh.mesh_dataset_metrics([])
