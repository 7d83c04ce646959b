"""Ray casting without a GPU: the binding's eleventh table against include/sapcu_ray.h, the sizers and the refusals of the C entry
points that come before any launch, the numpy definition (tests/ray_ref.py) against exact rational arithmetic and on analytic cases
of the unit box, watertightness, and the numpy restatement of fd's ray sampler."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import ray_ref as R
import abi_tables
from conftest import ROOT

NAMES = {"sapcu_ray_mesh_workspace_bytes", "sapcu_ray_mesh_f64", "sapcu_ray_fd_samples_workspace_bytes", "sapcu_ray_fd_samples_f64"}
OTHER_HEADERS = ("sapcu.h", "sapcu_seeds.h", "sapcu_fd_train.h", "sapcu_fd_edgeconv.h", "sapcu_train_step.h", "sapcu_metrics.h",
                 "sapcu_data.h", "sapcu_mesh.h", "sapcu_surface.h", "sapcu_sinkhorn.h")


def header_entry_points():
    """{name: argument list} of include/sapcu_ray.h."""
    return abi_tables.header_entry_points("sapcu_ray.h")


def test_the_header_declares_exactly_the_eleventh_table():
    from sapcu_amd import _lib
    decl = header_entry_points()
    assert set(decl) == set(_lib.RAY_EXPORTS) == NAMES
    others = (_lib.EXPORTS, _lib.SEEDS_EXPORTS, _lib.FD_TRAIN_EXPORTS, _lib.FD_EDGECONV_EXPORTS, _lib.TRAIN_STEP_EXPORTS,
              _lib.METRICS_EXPORTS, _lib.DATA_EXPORTS, _lib.MESH_EXPORTS, _lib.SURFACE_EXPORTS, _lib.SINKHORN_EXPORTS)
    for other in others:
        assert not set(other) & set(_lib.RAY_EXPORTS)
    assert all(n.startswith("sapcu_ray_") for n in _lib.RAY_EXPORTS)
    assert not any(n.startswith("sapcu_ray_") for other in others for n in other)
    # no name of this table starts with another header's prefix, and no other header declares or mentions one of its names
    for prefix in ("sapcu_point_mesh", "sapcu_surface", "sapcu_sinkhorn", "sapcu_softmin", "sapcu_plan", "sapcu_nn_cross", "sapcu_train",
                   "sapcu_dense_seeds", "sapcu_fd_", "sapcu_multi"):
        assert not any(n.startswith(prefix) for n in _lib.RAY_EXPORTS), prefix
    for h in OTHER_HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            assert "sapcu_ray_" not in f.read(), h
    lib = _lib.load()
    for name in _lib.RAY_EXPORTS:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len([a for a in decl[name].split(",") if a.strip()]), name
    assert _lib.ABI_VERSION == 2
    import sapcu_amd
    from sapcu_amd import ray, data
    assert sapcu_amd.ray_to_mesh is ray.ray_to_mesh and sapcu_amd.signed_ray_distance is ray.signed_ray_distance
    assert sapcu_amd.ray_metrics is ray.ray_metrics and sapcu_amd.sample_fd_rays is ray.sample_fd_rays
    assert sapcu_amd.is_watertight is ray.is_watertight and sapcu_amd.as_fd_npz is ray.as_fd_npz
    assert sapcu_amd.FdRayPatches is data.FdRayPatches
    assert ray.COS_1RAD == R.COS_1RAD == float(np.cos(1.0))


def _r256(nbytes):
    return (nbytes + 255) & ~255


def restated_workspace_bytes(nf, nq):
    """The one layout of csrc/ray_cast.hip (ray_ws_layout over knn_grid.h's grid_ws_layout), every region rounded up to 256 bytes."""
    cap = 2 * nf + 64
    tiles = (cap + 1 + 1023) // 1024
    grid = lambda n: (_r256(8 * 256 * 8) + _r256(56) + _r256(4 * (cap + 1)) + _r256(4 * cap) + _r256(4 * tiles) + _r256(4 * n) +
                      3 * _r256(8 * n) + _r256(4 * n))
    faces_grid = grid(nf)
    rays_grid = grid(nq) - _r256(56)                             # the rays share the faces' grid parameters
    return (faces_grid + rays_grid + 2 * _r256(8 * 256 * 8) + _r256(24 * nf) + _r256(8 * nf) + _r256(4 * nf) + _r256(24 * nq) +
            2 * _r256(8 * nq) + _r256(4 * nq) + 256)


def test_the_sizers_and_the_refusals_before_any_launch():
    """Everything include/sapcu_ray.h promises to refuse is refused with SAPCU_ERR_ARG (-1) on a machine without a GPU too: the
    checks come before the first HIP call, and no pointer is dereferenced."""
    from sapcu_amd import _lib
    lib = _lib.load()
    for size, extra in ((lib.sapcu_ray_mesh_workspace_bytes, lambda n: 0), (lib.sapcu_ray_fd_samples_workspace_bytes, lambda n: 3 * _r256(8 * n))):
        for bad in ((0, 5, 5), (5, 0, 5), (5, 5, -1), (1 << 31, 5, 5), (5, (1 << 29) + 1, 5), (5, 5, (1 << 31) - 63)):
            assert size(*bad) == -1, bad
        assert size((1 << 31) - 1, 1, 0) > 0
        for nv, nf, nq in ((1, 1, 0), (8, 12, 2000), (2562, 5120, 8192), (50002, 100000, 385582), (7, 4097, 65)):
            assert size(nv, nf, nq) == restated_workspace_bytes(nf, nq) + extra(nq), (nv, nf, nq)
            assert size(nv, nf, nq) == size(nv + 1000, nf, nq)   # the vertices take no workspace
    nv, nf, nq = 2562, 5120, 100
    need = lib.sapcu_ray_mesh_workspace_bytes(nv, nf, nq)
    P = ctypes.c_void_p
    vs, fs, os_, ds, tm, t, face, hit, ws = (P(0x10000 * k) for k in range(1, 10))        # never dereferenced
    info = (ctypes.c_int64 * 6)(7, 7, 7, 7, 7, 7)

    def call(vs=vs, nv=nv, fs=fs, nf=nf, os_=os_, ds=ds, tm=tm, nq=nq, cell=0.0, t=t, face=face, hit=hit, ws=ws, nbytes=need):
        return lib.sapcu_ray_mesh_f64(vs, nv, fs, nf, os_, ds, tm, nq, cell, t, face, hit, ws, nbytes, info, None)

    for kw in (dict(vs=None), dict(fs=None), dict(os_=None), dict(ds=None), dict(t=None), dict(nv=0), dict(nf=0), dict(nv=1 << 31),
               dict(nf=(1 << 29) + 1), dict(nq=-1), dict(nq=(1 << 31) - 63), dict(nbytes=need - 1), dict(nbytes=0), dict(ws=None),
               dict(ws=P(0x90004)), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(cell=1e300)):
        assert call(**kw) == -1, kw
        assert lib.sapcu_last_error()
    assert list(info) == [7] * 6
    assert call(nq=0, os_=None, ds=None, tm=None, t=None, face=None, hit=None) == 0 and list(info) == [0] * 6     # no ray: nothing is launched

    need = lib.sapcu_ray_fd_samples_workspace_bytes(nv, nf, nq)
    surf, sface, g, w, pts, nrm, lens, keep = (P(0x10000 * k) for k in range(10, 18))
    info = (ctypes.c_int64 * 6)(7, 7, 7, 7, 7, 7)

    def call2(vs=vs, nv=nv, fs=fs, nf=nf, surf=surf, sface=sface, g=g, w=w, n=nq, cell=0.0, pts=pts, nrm=nrm, lens=lens, keep=keep, ws=ws,
              nbytes=need):
        return lib.sapcu_ray_fd_samples_f64(vs, nv, fs, nf, surf, sface, g, w, n, cell, pts, nrm, lens, keep, ws, nbytes, info, None)

    for kw in (dict(vs=None), dict(fs=None), dict(surf=None), dict(sface=None), dict(g=None), dict(w=None), dict(pts=None), dict(nrm=None),
               dict(lens=None), dict(keep=None), dict(nv=0), dict(nf=0), dict(nv=1 << 31), dict(nf=(1 << 29) + 1), dict(n=-1),
               dict(n=(1 << 31) - 63), dict(nbytes=need - 1), dict(nbytes=0), dict(ws=None), dict(ws=P(0x90004)), dict(cell=-1.0),
               dict(cell=float("nan")), dict(cell=float("inf")), dict(cell=1e300)):
        assert call2(**kw) == -1, kw
        assert lib.sapcu_last_error()
    assert list(info) == [7] * 6
    assert call2(n=0, surf=None, sface=None, g=None, w=None, pts=None, nrm=None, lens=None, keep=None) == 0 and list(info) == [0] * 6


# ------------------------------------------------------------------------------------------------ exact arithmetic
def _fr(x):
    return tuple(Fraction(float(v)) for v in x)


def _fdot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _fsub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def _fcross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def exact_ray_triangle(o, d, a, b, c):
    """(u, v, t) of the definition in exact rational arithmetic, or None when det == 0."""
    e1, e2 = _fsub(b, a), _fsub(c, a)
    h = _fcross(d, e2)
    det = _fdot(e1, h)
    if det == 0:
        return None
    s = _fsub(o, a)
    q = _fcross(s, e1)
    return _fdot(s, h) / det, _fdot(d, q) / det, _fdot(e2, q) / det


# the largest relative error of t against exact arithmetic measured on the inputs below (seed 11), and the asserted bound: four times
# that, rounded up to a power of ten
MEASURED_T_ERROR = 9.61e-14
T_ERROR_BOUND = 1e-12


def test_the_definition_against_exact_rational_arithmetic():
    """200 random well-shaped triangles (smallest angle >= 10 degrees), each with one ray aimed at an interior point with every
    barycentric >= 0.01 and one aimed at a point of its plane at least 0.01 outside (one barycentric <= -0.01), from 1e-3 to 10
    triangle sizes away, at 3 degrees or more from the plane, with directions of lengths 0.1 to 10: every hit / miss decision of
    the numpy definition equals the exact one.  A ray whose exact u, v, 1 - u - v or t lies within 1e-12 of its boundary could be
    left out (at most 2 % of them); these inputs leave out none, which is asserted.  The relative error of t on the hits is far
    above 1e-16 because a triangle of size 0.01 near a point of magnitude 1 with an origin 1e-5 away loses the digits of the
    magnitude in o - a: the error is absolute, a few units in the last place of the COORDINATES."""
    rng = np.random.default_rng(11)
    worst, done, left_out, hits, misses = 0.0, 0, 0, 0, 0
    while done < 200:
        tri = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-2, 2) + rng.normal(size=3)
        e = [tri[1] - tri[0], tri[2] - tri[1], tri[0] - tri[2]]
        ang = [np.arccos(np.clip(np.dot(-e[k - 1], e[k]) / (np.linalg.norm(e[k - 1]) * np.linalg.norm(e[k])), -1, 1)) for k in range(3)]
        size = max(np.linalg.norm(x) for x in e)
        if min(ang) < np.radians(10.0):
            continue
        n = np.cross(e[0], -e[2])
        n /= np.linalg.norm(n)
        for inside in (True, False):
            if inside:
                w = 0.01 + 0.97 * rng.dirichlet(np.ones(3))
            else:
                k = rng.integers(3)
                w = np.zeros(3)
                w[k] = -rng.uniform(0.01, 1.0)
                split = rng.uniform(0.01, 0.99)
                w[(k + 1) % 3], w[(k + 2) % 3] = (1 - w[k]) * split, (1 - w[k]) * (1 - split)
            target = w @ tri
            while True:
                d = rng.normal(size=3)
                d /= np.linalg.norm(d)
                if abs(np.dot(d, n)) >= np.sin(np.radians(3.0)):
                    break
            o = target - d * size * 10.0 ** rng.uniform(-3, 1)
            d = d * 10.0 ** rng.uniform(-1, 1)
            t, hit, u, v, det = R.ray_triangle(o, d, np.inf, tri[0], tri[1], tri[2])
            ex = exact_ray_triangle(_fr(o), _fr(d), _fr(tri[0]), _fr(tri[1]), _fr(tri[2]))
            assert ex is not None
            eu, ev, et = ex
            if min(abs(eu), abs(ev), abs(1 - eu - ev), abs(et)) <= Fraction(1, 10 ** 12):
                left_out += 1
                continue
            exact_hit = eu >= 0 and ev >= 0 and eu + ev <= 1 and et >= 0
            assert bool(hit) == exact_hit == inside, (done, inside, float(eu), float(ev), float(et), u, v, t)
            if exact_hit:
                worst = max(worst, abs(float((Fraction(float(t)) - et) / et)))
                hits += 1
            else:
                misses += 1
        done += 1
    print("largest relative error of t against exact arithmetic: %.3g (%d hits, %d misses, %d left out)" % (worst, hits, misses, left_out))
    assert left_out == 0 and hits == 200 and misses == 200
    assert worst <= T_ERROR_BOUND, worst
    assert T_ERROR_BOUND == 10.0 ** np.ceil(np.log10(4 * MEASURED_T_ERROR))


# ---------------------------------------------------------------------------------------------------- analytic cases
def test_the_unit_box_along_axes_and_diagonals():
    """Dyadic coordinates: every operation of the definition is exact, so the results are asserted with ==."""
    v, f = R.BOX_V, R.BOX_F
    o = np.array([[0.25, 0.5, 2.0], [0.25, 0.5, -1.0], [2.0, 0.25, 0.625], [-3.0, 0.25, 0.625], [0.75, 4.0, 0.125], [0.75, -0.5, 0.125],
                  [1.25, 1.375, 1.5], [-0.5, -0.25, -0.125], [0.25, 0.5, 0.5], [0.25, 0.5, 0.5]])
    d = np.array([[0, 0, -1.0], [0, 0, 1.0], [-1.0, 0, 0], [2.0, 0, 0], [0, -4.0, 0], [0, 0.5, 0],
                  [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0, 0, 1.0], [0, 0, -0.5]])
    t, face, hit, skipped = R.ray_mesh(o, d, v, f)
    assert skipped == 0
    assert list(t) == [1.0, 1.0, 1.0, 1.5, 0.75, 1.0, 0.5, 0.5, 0.5, 1.0]
    want = np.array([[0.25, 0.5, 1], [0.25, 0.5, 0], [1, 0.25, 0.625], [0, 0.25, 0.625], [0.75, 1, 0.125], [0.75, 0, 0.125],
                     [0.75, 0.875, 1], [0, 0.25, 0.375], [0.25, 0.5, 1], [0.25, 0.5, 0]])
    assert np.array_equal(hit, want)
    # the side met: z = 1 is faces 2, 3; z = 0: 0, 1; x = 1: 10, 11; x = 0: 8, 9; y = 1: 6, 7; y = 0: 4, 5
    assert [int(k) // 2 for k in face] == [1, 0, 5, 4, 3, 2, 1, 4, 1, 0]
    tt = R.all_t(o, d, v, f)
    assert np.array_equal(t, tt.min(1)) and np.array_equal(face, np.argmax(tt == tt.min(1)[:, None], axis=1))


def test_t_max_the_surface_behind_and_parallel():
    v, f = R.BOX_V, R.BOX_F
    o, d = np.array([[0.25, 0.5, 2.0]]), np.array([[0, 0, -1.0]])
    one = np.array([1.0])
    t, face, hit, _ = R.ray_mesh(o, d, v, f, t_max=one)                                                   # t == t_max hits
    assert t[0] == 1.0 and face[0] == 3 and np.array_equal(hit[0], [0.25, 0.5, 1.0])
    t, face, hit, _ = R.ray_mesh(o, d, v, f, t_max=np.nextafter(one, 0.0))                                # one ulp less misses
    assert t[0] == np.inf and face[0] == -1 and np.isnan(hit).all()
    t, face, hit, _ = R.ray_mesh(o, d, v, f, t_max=np.array([2.0]))
    assert t[0] == 1.0 and face[0] == 3
    for bad in (-1.0, np.nan, 0.0):
        assert R.ray_mesh(o, d, v, f, t_max=np.array([bad]))[1][0] == -1
    # t = 0: an origin on the surface hits, in either direction, and t_max = 0 admits exactly that
    on = np.array([[0.25, 0.5, 1.0]])
    for dz in (-1.0, 1.0):
        for tm in (None, np.array([0.0])):
            t, face, hit, _ = R.ray_mesh(on, np.array([[0, 0, dz]]), v, f, t_max=tm)
            assert t[0] == 0.0 and face[0] == 3 and np.array_equal(hit[0], on[0])
    # a hit behind the origin misses
    assert R.ray_mesh(o, -d, v, f)[1][0] == -1
    # a ray in the plane of a face: det == 0, a miss of that face (the box's side x = 1 is met instead)
    tt = R.all_t(on, np.array([[1.0, 0, 0]]), v, f)
    assert tt[0, 2] == np.inf and tt[0, 3] == np.inf
    assert R.ray_mesh(on, np.array([[1.0, 0, 0]]), v, f[2:4])[1][0] == -1
    t, face, _, _ = R.ray_mesh(on, np.array([[1.0, 0, 0]]), v, f)
    assert t[0] == 0.75 and face[0] // 2 == 5
    # a zero and a NaN direction, a NaN origin: misses
    for oo, dd in ((o, np.zeros((1, 3))), (o, np.array([[0, np.nan, -1.0]])), (np.array([[np.nan, 0.5, 2.0]]), d)):
        t, face, hit, _ = R.ray_mesh(oo, dd, v, f)
        assert t[0] == np.inf and face[0] == -1 and np.isnan(hit).all()


def test_the_shared_diagonal_gives_equal_t_on_two_faces_and_the_lower_index():
    v, f = R.BOX_V, R.BOX_F
    o = np.array([[0.5, 0.5, 2.0], [0.25, 0.25, 3.0], [0.5, -1.0, 0.5]])
    d = np.array([[0, 0, -1.0], [0, 0, -2.0], [0, 1.0, 0]])
    tt = R.all_t(o, d, v, f)
    t, face, hit, _ = R.ray_mesh(o, d, v, f)
    for i, (lo, hi, want) in enumerate(((2, 3, 1.0), (2, 3, 1.0), (4, 5, 1.0))):
        assert tt[i, lo] == tt[i, hi] == want == t[i] and face[i] == lo, (i, tt[i])
    # the same faces in the other order: the lower index still wins
    g = f.copy()
    g[[2, 3]] = f[[3, 2]]
    assert R.ray_mesh(o[:2], d[:2], v, g)[1].tolist() == [2, 2]
    # skipped faces take no part and are counted
    h = np.concatenate([[[0, 0, 1], [0, 1, 8], [-1, 2, 3]], f])
    t2, face2, hit2, skipped = R.ray_mesh(o, d, v, h)
    assert skipped == 3 and np.array_equal(face2, face + 3) and np.array_equal(t2, t) and np.array_equal(hit2, hit)


# --------------------------------------------------------------------------------------- watertightness, the sampler
def test_is_watertight():
    from sapcu_amd import ray
    f = R.BOX_F
    assert ray.is_watertight(f) and ray.is_watertight(f.astype(np.int32)) and ray.is_watertight(R.icosphere(1)[1])
    assert ray.is_watertight(R.torus(8, 5)[1])
    assert not ray.is_watertight(f[:-1])                                      # an opened box
    assert not ray.is_watertight(np.concatenate([f, f[:1]]))                  # a doubled face: three faces on its edges
    assert not ray.is_watertight(f[:1]) and not ray.is_watertight(np.zeros((0, 3), dtype=np.int64))
    import torch
    assert ray.is_watertight(torch.from_numpy(f))
    for bad in (np.zeros((4, 2), dtype=np.int64), np.zeros((4, 3)), np.zeros((12,), dtype=np.int64)):
        with pytest.raises(ValueError):
            ray.is_watertight(bad)
    d = ray.as_fd_npz(np.zeros((5, 3)), np.ones((5, 3)), np.arange(5.0))
    assert sorted(d) == ["lens", "normals", "points"] and d["lens"].shape == (5, 3) and d["lens"].dtype == np.float32
    assert np.array_equal(d["lens"][:, 0], np.arange(5.0)) and np.array_equal(d["lens"][:, 2], d["lens"][:, 0])


_SAMPLES = {}


def sampler_case(name, n=4096):
    """(vertices, faces, surf, sface, g, w) of one sampler test case and ``ray_ref.fd_samples`` on it, computed once per session
    (tests/test_gpu_ray.py shares it).  Vertices and surface points are f64 here: a surface point rounded to f32 lies up to 6e-8
    off its face at this scale, more than the 2^-20 of a short len that t_max allows."""
    if name not in _SAMPLES:
        rng = np.random.default_rng(len(name))
        v, f = {"ico": lambda: R.icosphere(2), "small": lambda: R.icosphere(1, radius=0.01)}[name]()
        surf, sface = R.surface_points(v, f, n, rng)
        g, w = rng.normal(size=(n, 3)), rng.uniform(size=n)
        _SAMPLES[name] = (v, f, surf, sface, g, w, R.fd_samples(v, f, surf, sface, g, w))
    return _SAMPLES[name]


def test_the_sampler_restated_in_numpy_on_an_icosphere():
    v, f, surf, sface, g, w, s = sampler_case("ico")
    keep = s["keep"]
    a, b, c = (v[f[sface, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1)[:, None]
    cosang = np.sum(n * -s["normals"], axis=1)
    assert 0.15 * len(keep) < keep.sum() < 0.30 * len(keep)                   # the cap of 1 rad: (1 - cos 1) / 2 = 23 % of the sphere
    assert (cosang[keep] > R.COS_1RAD).all() and np.array_equal(s["face"][keep], sface[keep])
    # every kept point lies outside (above its face's plane, the mesh is convex), and the ray back meets the surface at len
    assert (np.sum((s["points"][keep] - a[keep]) * n[keep], axis=1) > 0).all()
    assert (np.abs(s["t"][keep] - s["lens"][keep]) <= 1e-6 * s["lens"][keep]).all()
    assert (s["lens"] >= 0.003).all() and (s["lens"] < 0.03).all()
    assert np.allclose(np.linalg.norm(s["normals"], axis=1), 1.0, rtol=0, atol=1e-15)
    # what is dropped: the angle alone (the sampled face is still met first), or another face met first
    dropped = ~keep
    assert ((cosang[dropped] <= R.COS_1RAD) | (s["face"][dropped] != sface[dropped])).all()
    assert (cosang[dropped & (s["face"] == sface)] <= R.COS_1RAD).all()


def test_points_thrown_through_the_far_side_are_dropped():
    """An icosphere of radius 0.01: a length of up to 0.03 carries an inward throw out through the far side, where the ray back
    meets the far face first."""
    v, f, surf, sface, g, w, s = sampler_case("small")
    a, b, c = (v[f[sface, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1)[:, None]
    inward = np.sum(n * -s["normals"], axis=1) < 0
    through = inward & (np.linalg.norm(s["points"], axis=1) > 0.0101)
    assert through.sum() > 500
    assert not s["keep"][through].any() and (s["face"][through] != sface[through]).all() and (s["face"][through] >= 0).all()
    assert (s["t"][through] <= s["lens"][through]).all()                      # the far face comes before the sampled one
    assert s["keep"].sum() > 500 and not s["keep"][inward].any()
