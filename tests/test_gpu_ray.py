"""Ray casting on the device (-m gpu; include/sapcu_ray.h, csrc/ray_cast.hip, sapcu_amd/ray.py).

The brute-force kernel must equal the numpy definition (tests/ray_ref.py) bit for bit on t, face and hit point; the grid route must
equal the brute-force kernel bit for bit for any cell size, for rays of the sampler's length and unbounded ones from outside and
inside, on shifted and scaled meshes, with oversize, skipped and duplicated faces; hit points agree with the point-to-mesh distance
of DESIGN 4.9; both pointer-taking entry points keep the memory contract of DESIGN 2 under guard bands; ``sample_fd_rays`` equals
``ray_ref.fd_samples`` on the same draws; ``signed_ray_distance`` / ``ray_metrics`` equal numpy on the same vectors."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_utils as U
import ray_ref as R
import test_ray_host as H
from guarded import Arena

pytestmark = pytest.mark.gpu

F64, I64, I32, U8 = torch.float64, torch.int64, torch.int32, torch.uint8


def _dev(a, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(U.dev())


def _bits(t):
    t = t if torch.is_tensor(t) else torch.as_tensor(np.ascontiguousarray(t))
    return t.contiguous().view(I64).cpu() if t.dtype == F64 else t.cpu()


def _same(a, b):
    """Bit-equal, every NaN counting as equal to every NaN."""
    a, b = (x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x)) for x in (a, b))
    a, b = a.cpu(), b.cpu()
    if a.dtype != F64:
        return a.shape == b.shape and bool((a == b).all())
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


def _lib():
    from sapcu_amd import _lib
    return _lib


def device_call(origins, dirs, vertices, faces, t_max=None, cell=0.0, brute=False, mult=2.0, pop=4, piece=2.0, auto=False):
    """sapcu_internal_ray_mesh_tuned on compact tensors (the public entry point with its three constants given; forced to the
    brute-force route, or to the grid whatever the face count and the rays' length unless ``auto``) -> (t, face, hit, info).
    Outputs and workspace start from junk."""
    L = _lib()
    lib = L.load()
    o, d, v, f = _dev(origins), _dev(dirs), _dev(vertices), _dev(faces, np.int32)
    tm = None if t_max is None else _dev(t_max)
    nq, nv, nf = o.shape[0], v.shape[0], f.shape[0]
    t = torch.full((nq,), 7.0, dtype=F64, device=U.dev())
    face = torch.full((nq,), -7, dtype=I64, device=U.dev())
    hit = torch.full((nq, 3), 7.0, dtype=F64, device=U.dev())
    nbytes = int(lib.sapcu_ray_mesh_workspace_bytes(nv, nf, nq))
    ws = torch.full((nbytes,), 0xA5, dtype=U8, device=U.dev())
    info = (ctypes.c_int64 * 6)()
    L.check(lib.sapcu_internal_ray_mesh_tuned(L.ptr(v), nv, L.ptr(f), nf, L.ptr(o), L.ptr(d), L.ptr(tm), nq, float(cell), float(mult),
                                              int(pop), float(piece), 1 if brute else (0 if auto else 2), L.ptr(t), L.ptr(face), L.ptr(hit), L.ptr(ws), nbytes, info,
                                              L.current_stream()))
    torch.cuda.synchronize()
    return t, face, hit, list(info)


def assert_equals_definition(origins, dirs, vertices, faces, what, t_max=None, ref=None):
    t, face, hit, info = device_call(origins, dirs, vertices, faces, t_max=t_max, brute=True)
    rt, rf, rh, skipped = ref if ref is not None else R.ray_mesh(origins, dirs, vertices, faces, t_max=t_max)
    assert info[0] == 0 and info[5] == skipped, (what, info, skipped)
    bad = ~((_bits(t) == _bits(rt)) & (face.cpu() == torch.as_tensor(rf)))
    assert not bool(bad.any()), "%s: %d of %d rays differ from the definition, first %d: (%r, %d) against (%r, %d)" % (
        what, int(bad.sum()), bad.numel(), int(bad.nonzero()[0]), t[bad][0].item(), face[bad][0].item(), rt[bad.numpy()][0],
        rf[bad.numpy()][0])
    assert _same(hit, rh), what
    return t, face, hit


def assert_grid_equals_brute(origins, dirs, vertices, faces, cell, what, t_max=None, route=None, brute=None, **tuning):
    b = brute if brute is not None else device_call(origins, dirs, vertices, faces, t_max=t_max, brute=True)
    g = device_call(origins, dirs, vertices, faces, t_max=t_max, cell=cell, **tuning)
    assert b[3][0] == 0
    bad = (_bits(g[0]) != _bits(b[0])) | (g[1] != b[1]).cpu()
    assert not bool(bad.any()), "%s cell %g: %d of %d rays differ, first %d: (%r, %d) against brute force (%r, %d)" % (
        what, cell, int(bad.sum()), bad.numel(), int(bad.nonzero()[0]), g[0][bad][0].item(), g[1][bad][0].item(), b[0][bad][0].item(),
        b[1][bad][0].item())
    assert _same(g[2], b[2]), (what, cell)
    assert g[3][5] == b[3][5], (what, g[3], b[3])
    if route is not None:
        assert g[3][0] == route, (what, cell, g[3])
    return g[3], b


# ------------------------------------------------------------------------------------------------------ the meshes
def soup(nf, seed):
    """nf random triangles over 3 * nf / 2 + 3 shared vertices."""
    rng = np.random.default_rng(seed)
    nv = 3 * nf // 2 + 3
    v = rng.uniform(size=(nv, 3))
    f = np.stack([rng.permutation(nv)[:3] for _ in range(nf)])
    return v, f


def radii(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    g = ((a + b) + c) / 3.0
    return np.sqrt(np.maximum(np.maximum(((a - g) ** 2).sum(1), ((b - g) ** 2).sum(1)), ((c - g) ** 2).sum(1)))


_MESHES = {}


def mesh(name):
    if name not in _MESHES:
        _MESHES[name] = {"ico1280": lambda: R.icosphere(3), "ico5120": lambda: R.icosphere(4), "torus": lambda: R.torus(32, 44)}[name]()
    return _MESHES[name]


def rays(kind, v, f, n, seed):
    """n rays of one kind -> (origins, dirs, t_max or None): "sampler" (the sampler's: thrown 0.003 .. 0.03 times the mesh's size off the
    surface and cast back, t_max = len * (1 + 2^-20)), "outside" (unbounded, from three extents away towards the mesh, directions of
    any length), "inside" (unbounded, from anywhere in the box in any direction)."""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    ext = float((hi - lo).max())
    if kind == "sampler":
        surf, _ = R.surface_points(v, f, n, rng)
        p, d, lens, tm = R.fd_rays(surf / ext, rng.normal(size=(n, 3)), rng.uniform(size=n))
        return p * ext, d * ext, tm
    if kind == "outside":
        u = rng.normal(size=(n, 3))
        o = (lo + hi) / 2 + 3 * ext * u / np.linalg.norm(u, axis=1)[:, None]
        target = rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, size=(n, 3))
        return o, (target - o) * 10.0 ** rng.uniform(-2, 2, size=(n, 1)), None
    o = rng.uniform(lo, hi, size=(n, 3))
    return o, rng.normal(size=(n, 3)) * ext, None


# --------------------------------------------------------------------------------- brute force against the definition
@pytest.mark.parametrize("nf", [1, 2, 63, 64, 65, 130, 1000])
def test_brute_force_equals_the_definition_at_tile_and_wave_edges(nf):
    v, f = soup(nf, nf)
    rng = np.random.default_rng(1000 + nf)
    o = rng.uniform(-0.5, 1.5, size=(257, 3))
    target = rng.uniform(0.0, 1.0, size=(257, 3))
    d = (target - o) * 10.0 ** rng.uniform(-1, 1, size=(257, 1))
    tm = np.where(rng.uniform(size=257) < 0.3, np.inf, rng.uniform(0.0, 3.0, size=257) / 10.0 ** rng.uniform(-1, 1, size=257))
    tm[::17] = 0.0
    for t_max in (None, tm):
        ref = R.ray_mesh(o, d, v, f, t_max=t_max)
        if nf >= 63 and t_max is None:
            assert int((ref[1] >= 0).sum()) >= 100
        for nq in (1, 63, 64, 65, 257):
            assert_equals_definition(o[:nq], d[:nq], v, f, "nf=%d nq=%d" % (nf, nq), t_max=None if t_max is None else t_max[:nq],
                                     ref=tuple(r[:nq] if i < 3 else r for i, r in enumerate(ref)))


def test_brute_force_on_the_box_ties_boundaries_parallel_rays_and_t_max():
    v, f = R.BOX_V, R.BOX_F
    o = np.array([[0.5, 0.5, 2.0], [0.25, 0.25, 3.0], [0.5, -1.0, 0.5], [0.25, 0.5, 2.0], [0.25, 0.5, 2.0], [0.25, 0.5, 2.0],
                  [0.25, 0.5, 1.0], [0.25, 0.5, 1.0], [0.25, 0.5, 1.0], [0.25, 0.5, 2.0], [1.25, 1.375, 1.5], [0.25, 0.5, 0.5],
                  [0.25, 0.5, 2.0], [0.25, 0.5, 2.0], [np.nan, 0.5, 2.0], [0.25, 0.5, 2.0], [0.25, 0.5, 2.0], [2.0, 2.0, 2.0]])
    d = np.array([[0, 0, -1.0], [0, 0, -2.0], [0, 1.0, 0], [0, 0, -1.0], [0, 0, -1.0], [0, 0, -1.0],
                  [0, 0, -1.0], [0, 0, 1.0], [1.0, 0, 0], [0, 0, 1.0], [-1.0, -1.0, -1.0], [0, 0, -0.5],
                  [0, 0, 0], [0, np.nan, -1.0], [0, 0, -1.0], [0, 0, -1.0], [0, 0, -1.0], [-1.0, -1.0, -1.0]])
    one = 1.0
    tm = np.array([np.inf, np.inf, np.inf, one, np.nextafter(one, 0.0), 2.0, 0.0, 0.0, np.inf, np.inf, np.inf, np.inf, np.inf, np.inf, np.inf,
                   -1.0, np.nan, np.inf])
    t, face, hit = assert_equals_definition(o, d, v, f, "box", t_max=tm)
    assert face[:12].tolist() == [2, 2, 4, 3, -1, 3, 3, 3, face[8].item(), -1, face[10].item(), face[11].item()]
    assert t[:8].tolist() == [1.0, 1.0, 1.0, 1.0, float("inf"), 1.0, 0.0, 0.0] and t[8].item() == 0.75 and face[8].item() // 2 == 5
    assert face[12:17].tolist() == [-1] * 5 and bool(torch.isnan(hit[12:17]).all()) and bool(torch.isinf(t[12:17]).all())
    assert_equals_definition(o, d, v, f, "box, no t_max")                                       # t_max NULL: +inf for every ray
    assert_equals_definition(o, d, v, f[2:4], "the top side alone", t_max=tm)                   # the ray in its plane misses it
    g = f.copy()
    g[[2, 3]] = f[[3, 2]]
    _, face, _ = assert_equals_definition(o[:2], d[:2], v, g, "the tie in the other order")
    assert face.tolist() == [2, 2]


def test_brute_force_duplicated_zero_area_and_out_of_range_faces():
    v, f = R.icosphere(1)
    rng = np.random.default_rng(3)
    o, d, _ = rays("outside", v, f, 300, 3)
    dup = np.concatenate([f[::-1], f, f])                                                       # every face three times
    _, face, _ = assert_equals_definition(o, d, v, dup, "duplicated faces")
    assert int((face >= 0).sum()) > 100
    ref = R.ray_mesh(o, d, v, dup)
    tt = R.all_t(o, d, v, dup)
    assert np.array_equal(ref[1][ref[1] >= 0], np.argmax(tt == tt.min(1)[:, None], axis=1)[ref[1] >= 0])
    bad = np.concatenate([[[0, 0, 1], [5, 5, 5], [0, len(v), 1], [-1, 2, 3]], f[:40], [[2, 1, 2]], f[40:]])
    t, face, hit = assert_equals_definition(o, d, v, bad, "skipped faces")
    assert not bool(((face >= 0) & (face < 4)).any()) and not bool((face == 44).any())
    t, face, hit = assert_equals_definition(o, d, v, bad[:4], "every face skipped")
    assert bool((face == -1).all()) and bool(torch.isinf(t).all()) and bool(torch.isnan(hit).all())
    big = np.array([[0, 0, 0], [1e200, 0, 0], [0, 1e200, 0.0], [1, 0, 0], [0, 1, 0]])
    assert_equals_definition(np.array([[0.2, 0.2, 1.0]]), np.array([[0, 0, -1.0]]), big, np.array([[0, 1, 2], [0, 3, 4]]),
                             "a face whose normal overflows")


# ------------------------------------------------------------------------------------------- grid against brute force
KINDS = ("sampler", "outside", "inside")


@pytest.mark.parametrize("name", ["ico1280", "ico5120", "torus"])
def test_grid_equals_brute_force(name):
    """4096 rays of each kind at four explicit cell edges (from 0.6 to 5 of the largest face radius: the cap of two edges keeps
    every face in the grid) and the automatic one.  The torus has faces four times as long as wide."""
    v, f = mesh(name)
    rmax = float(radii(v, f).max())
    if name == "torus":
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        e = np.stack([np.linalg.norm(b - a, axis=1), np.linalg.norm(c - b, axis=1), np.linalg.norm(a - c, axis=1)], 1)
        assert 3.0 < np.median(e.max(1) / e.min(1)) < 6.0
    for k, kind in enumerate(KINDS):
        o, d, tm = rays(kind, v, f, 4096, 10 * len(name) + k)
        brute = None
        for cell in (0.6 * rmax, rmax, 2 * rmax, 5 * rmax, 0.0):
            info, brute = assert_grid_equals_brute(o, d, v, f, cell, "%s/%s" % (name, kind), t_max=tm, brute=brute, route=1)
            assert info[4] == 0 and info[5] == 0
        hits = int((brute[1] >= 0).sum())
        assert hits > (3500 if kind == "sampler" else 400), (name, kind, hits)
    from sapcu_amd import ray
    info = []
    t, face, hit = ray.ray_to_mesh(o, d, v, f, t_max=tm, info=info)              # the public entry point: the same bits, the automatic route
    assert _same(t, brute[0]) and _same(face, brute[1]) and _same(hit, brute[2]) and info[0] == 0       # rays that cross the mesh
    t, face, hit = ray.ray_to_mesh(o, d, v, f, t_max=tm, cell_size=rmax, info=info)
    assert _same(t, brute[0]) and _same(face, brute[1]) and _same(hit, brute[2]) and info[0] == 1 and info[5] == 0


def test_grid_piece_lengths_and_cell_populations():
    v, f = mesh("ico1280")
    for k, kind in enumerate(KINDS):
        o, d, tm = rays(kind, v, f, 1024, 50 + k)
        brute = None
        for piece, pop in ((0.125, 4), (0.5, 1), (2.0, 64), (8.0, 4), (1024.0, 16)):
            _, brute = assert_grid_equals_brute(o, d, v, f, 0.0, "piece %g pop %d %s" % (piece, pop, kind), t_max=tm, brute=brute, route=1,
                                                piece=piece, pop=pop)


def test_grid_on_a_shifted_and_on_a_scaled_mesh():
    v, f = mesh("ico1280")
    rmax = float(radii(v, f).max())
    for k, kind in enumerate(KINDS):
        o, d, tm = rays(kind, v, f, 2048, 70 + k)
        for cell in (0.0, rmax):
            assert_grid_equals_brute(o + 1e6, d, v + 1e6, f, cell, "shifted/" + kind, t_max=tm, route=1)
            assert_grid_equals_brute(o * 1e9, d * 1e9, v * 1e9, f, cell * 1e9, "scaled/" + kind, t_max=tm, route=1)
            assert_grid_equals_brute(o * 1e9, d, v * 1e9, f, cell * 1e9, "scaled, short directions/" + kind,
                                     t_max=None if tm is None else tm * 1e9, route=1)


def test_the_oversize_list_and_the_fallback():
    v, f = mesh("torus")
    lo, hi = v.min(0) - 0.2, v.max(0) + 0.2
    v2 = np.concatenate([v, [lo, [hi[0], lo[1], hi[2]], [lo[0], hi[1], hi[2]]]])               # one face spanning the whole box
    f2 = np.concatenate([f[:2000], [[len(v), len(v) + 1, len(v) + 2]], f[2000:]])
    rmax = float(radii(v, f).max())
    for k, kind in enumerate(KINDS):
        o, d, tm = rays(kind, v, f, 2048, 90 + k)
        brute = None
        for cell, mult in ((0.0, 2.0), (rmax, 1.0), (rmax, 2.0), (3 * rmax, 1.0)):
            info, brute = assert_grid_equals_brute(o, d, v2, f2, cell, "one big face/" + kind, t_max=tm, brute=brute, route=1, mult=mult)
            assert info[4] >= 1 and info[4] * 4 <= len(f2), info
        if kind != "sampler":
            assert int((brute[1] == 2000).sum()) > 0                                            # the big face is hit somewhere
    # the same cell at three caps: the list shrinks as the cap grows, the results do not move; above a quarter: brute force
    o, d, tm = rays("outside", v, f, 2048, 99)
    r = radii(v, f)
    cell = float(np.quantile(r, 0.9))
    brute, sizes = None, []
    for mult in (0.5, 1.0, 2.0):
        info, brute = assert_grid_equals_brute(o, d, v, f, cell, "cap %g" % mult, brute=brute, mult=mult)
        assert info[4] == int((r * (1 + 1e-9) > mult * cell).sum()) and info[0] == (1 if info[4] * 4 <= len(f) else 0), info
        sizes.append(info[4])
    assert sizes[0] == len(f) and sizes[1] > 0 and sizes[1] * 4 <= len(f) and sizes[2] == 0, sizes
    info, _ = assert_grid_equals_brute(o, d, v, f, rmax, "every face oversize", brute=brute, route=0, mult=0.25)
    assert info[:4] == [0, 0, 0, 0] and info[4] == len(f)
    info, _ = assert_grid_equals_brute(o, d, v, f, rmax / 100, "a cell edge far below the faces' size", brute=brute)   # the edge grows to the cell budget
    info, _ = assert_grid_equals_brute(o, d, v, f, 100.0, "one cell", brute=brute, route=1)
    assert info == [1, 1, 1, 1, 0, 0]
    # skipped faces inside a grid: reported, and they take no part
    f3 = np.concatenate([f, [[0, 0, 1], [5, 5, 5], [0, len(v), 1], [-1, 2, 3]]])
    info, _ = assert_grid_equals_brute(o, d, v, f3, rmax, "skipped in the grid", route=1)
    assert info[5] == 4
    # below the automatic threshold: brute force unless a cell edge is given
    sv, sf = R.icosphere(2)
    so, sd, _ = rays("outside", sv, sf, 500, 5)
    assert assert_grid_equals_brute(so, sd, sv, sf, 0.0, "small, automatic", route=0, auto=True)[0] == [0] * 6
    assert assert_grid_equals_brute(so, sd, sv, sf, 0.5, "small, a cell edge given", route=1, auto=True)[0][0] == 1
    assert assert_grid_equals_brute(so, sd, sv, sf, 0.0, "small, the grid forced", route=1)[0][0] == 1


def test_the_automatic_route_is_the_grid_for_short_rays_and_brute_force_for_rays_that_cross_the_mesh():
    from sapcu_amd import ray
    for name in ("ico1280", "ico5120"):
        v, f = mesh(name)
        for k, kind in enumerate(KINDS):
            o, d, tm = rays(kind, v, f, 2048, 60 + k)
            want = 1 if kind == "sampler" else 0
            info, brute = assert_grid_equals_brute(o, d, v, f, 0.0, "automatic/" + kind, t_max=tm, route=want, auto=True)
            assert (info[1] > 1) == (want == 1)
            got = []
            t, face, hit = ray.ray_to_mesh(o, d, v, f, t_max=tm, info=got)
            assert _same(t, brute[0]) and _same(face, brute[1]) and _same(hit, brute[2]) and got[0] == want
            assert_grid_equals_brute(o, d, v, f, 0.3, "a cell edge given/" + kind, t_max=tm, brute=brute, route=1, auto=True)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 1e200, 1e-200])
def test_non_finite_huge_and_tiny_coordinates_take_the_brute_force_route(bad):
    v, f = mesh("ico1280")
    rmax = float(radii(v, f).max())
    o, d, _ = rays("outside", v, f, 1000, 7)
    d2 = d.copy()
    d2[300, 1] = bad
    for cell in (0.0, rmax):
        assert_grid_equals_brute(o, d2, v, f, cell, "bad direction", route=0)
    assert_grid_equals_brute(o, d, v, f, 0.0, "clean", route=1)
    if bad == 1e-200:
        return
    v2 = v.copy()
    v2[777 % len(v), 1] = bad
    o2 = o.copy()
    o2[500, 2] = bad
    for cell in (0.0, rmax):
        assert_grid_equals_brute(o, d, v2, f, cell, "bad vertex", route=0)
        assert_grid_equals_brute(o2, d, v, f, cell, "bad origin", route=0)
    tm = np.full(len(o), np.inf)
    tm[::3] = np.nan if bad != bad else abs(bad)
    tm[1::3] = -1.0
    assert_grid_equals_brute(o, d, v, f, rmax, "odd t_max", t_max=tm, route=1)                  # t_max is no coordinate: the grid runs


# ---------------------------------------------------------------------------------------------- consistency with 4.9
def test_hit_points_lie_on_the_mesh_and_t_bounds_the_closest_distance():
    from sapcu_amd import mesh as mesh_mod, ray
    v, f = mesh("ico1280")
    for k, kind in enumerate(KINDS):
        o, d, tm = rays(kind, v, f, 4096, 30 + k)
        t, face, hit = ray.ray_to_mesh(o, d, v, f, t_max=tm)
        got = (face >= 0).cpu().numpy()
        assert got.sum() > 1000
        dist = mesh_mod.point_to_mesh(hit[face >= 0], v, f)[0].cpu().numpy()
        reach = t.cpu().numpy()[got] * np.linalg.norm(d[got], axis=1)
        bound = 1e-9 * (max(np.abs(v).max(), np.abs(o).max()) + reach)
        print("%s: largest distance of a hit point to the mesh %.3g, smallest bound %.3g" % (kind, dist.max(), bound.min()))
        assert (dist <= bound).all(), (kind, float(dist.max()))
        if kind == "outside":                                                                   # convex mesh, origins outside
            p2m = mesh_mod.point_to_mesh(o[got], v, f)[0].cpu().numpy()
            assert (reach >= p2m * (1 - 1e-12)).all()


# ------------------------------------------------------------------------------------------------- memory contract
def _buffers(arena, o, d, tm, v, f, offsets=(0, 0, 0, 0, 0, 0, 0, 0, 8)):
    lib = _lib().load()
    nq, nv, nf = len(o), len(v), len(f)
    nbytes = int(lib.sapcu_ray_mesh_workspace_bytes(nv, nf, nq))
    assert nbytes > 0
    k = offsets
    return {"v": arena.inp(np.ascontiguousarray(v, dtype=np.float64), offset=k[0], name="vertices"),
            "f": arena.inp(np.ascontiguousarray(f, dtype=np.int32), offset=k[1], name="faces"),
            "o": arena.inp(np.ascontiguousarray(o, dtype=np.float64), offset=k[2], name="origins"),
            "d": arena.inp(np.ascontiguousarray(d, dtype=np.float64), offset=k[3], name="dirs"),
            "tm": arena.inp(np.ascontiguousarray(tm if tm is not None else np.full(nq, np.inf), dtype=np.float64), offset=k[4], name="t_max"),
            "t": arena.out((nq,), F64, offset=k[5], name="t"), "face": arena.out((nq,), I64, offset=k[6], name="face"),
            "hit": arena.out((nq, 3), F64, offset=k[7], name="hit"), "ws": arena.ws(nbytes, offset=k[8], name="workspace"),
            "nbytes": nbytes, "has_tm": tm is not None}


def _launch(b, cell, optional, **over):
    L = _lib()
    lib = L.load()
    info = (ctypes.c_int64 * 6)(5, 5, 5, 5, 5, 5)
    a = {"v": L.ptr(b["v"]), "nv": b["v"].shape[0], "f": L.ptr(b["f"]), "nf": b["f"].shape[0], "o": L.ptr(b["o"]), "d": L.ptr(b["d"]),
         "tm": L.ptr(b["tm"]) if (optional and b["has_tm"]) else None, "nq": b["o"].shape[0], "cell": float(cell), "t": L.ptr(b["t"]),
         "face": L.ptr(b["face"]) if optional else None, "hit": L.ptr(b["hit"]) if optional else None, "ws": L.ptr(b["ws"]),
         "nbytes": b["nbytes"]}
    a.update(over)
    rc = lib.sapcu_ray_mesh_f64(a["v"], a["nv"], a["f"], a["nf"], a["o"], a["d"], a["tm"], a["nq"], a["cell"], a["t"], a["face"], a["hit"],
                                a["ws"], a["nbytes"], info, L.current_stream())
    torch.cuda.synchronize()
    return rc, list(info)


def _guard_case(name):
    if name.startswith("grid-oversize"):
        v, f = mesh("torus")
        v = np.concatenate([v, [[-1, -1, -1], [1, -1, 1], [-1, 1, 1.0]]])
        f = np.concatenate([f, [[len(v) - 3, len(v) - 2, len(v) - 1], [0, 0, 1]]])
        o, d, tm = rays("sampler", v[:-3], f[:-2], 1000 + 37, 1)
        return o, d, tm, v, f, 0.0, 1
    if name.startswith("grid-forced-small"):
        o, d, tm = rays("inside", R.BOX_V, R.BOX_F, 129, 2)
        return o, d, tm, R.BOX_V, R.BOX_F, 10.0, 1
    if name.startswith("grid"):
        v, f = mesh("ico1280")
        o, d, tm = rays("sampler", v, f, 1000 + 37, 3)
        return o, d, tm, v, f, (0.3 if "no-optional" in name else 0.0), 1      # without their t_max the rays cross the mesh: a cell edge is given
    v, f = R.icosphere(2)
    o, d, tm = rays("sampler", v, f, 200, 4)
    if "bad-ray" in name:
        o[100, 0] = np.inf
        return o, d, tm, v, f, 0.3, 0
    return o, d, tm, v, f, 0.0, 0


GUARD_CASES = ["grid", "grid-no-optional", "grid-oversize", "grid-forced-small", "brute-small", "brute-small-no-optional",
               "brute-bad-ray-no-optional"]


@pytest.mark.parametrize("name", GUARD_CASES)
def test_memory_contract_under_guard_bands(name):
    """The three runs of DESIGN 2: 0xFF bands and workspace with NaN-prefilled outputs, 0x00 bands and workspace, the dirty
    workspace again — guards intact, outputs written in full and bit-identical, and identical to the compact call.  Bases are
    moved off the allocator's alignment as far as the element types allow.  "no-optional": face_out, hit_out and t_max NULL."""
    from sapcu_amd import ray
    o, d, tm, v, f, cell, route = _guard_case(name)
    optional = "no-optional" not in name
    results = []
    for fill in (0xFF, 0x00):
        arena = Arena("guard", fill=fill, device=U.dev())
        bufs = _buffers(arena, o, d, tm, v, f, offsets=(8, 4, 24, 16, 8, 8, 16, 8, 8))
        for again in range(2 if fill == 0x00 else 1):
            arena.refill_outputs()
            rc, info = _launch(bufs, cell, optional)
            assert rc == 0, _lib().load().sapcu_last_error()
            arena.check()
            results.append((bufs["t"].clone(), bufs["face"].clone(), bufs["hit"].clone(), info))
    t0, f0, h0, info0 = results[0]
    assert info0[0] == route, info0
    for t, fa, h, info in results[1:]:
        assert _same(t, t0) and _same(fa, f0) and _same(h, h0) and info == info0
    ct, cf, ch = ray.ray_to_mesh(o, d, v, f, t_max=tm if optional else None, cell_size=cell)
    assert _same(ct, t0)
    if optional:
        assert _same(cf, f0) and _same(ch, h0)
    else:                                                      # NULL outputs: the buffers that were not passed are untouched
        assert bool((f0 == -1).all()) and bool((_bits(h0) == -1).all())
    assert not bool(torch.isnan(t0).any()) and int(torch.isfinite(t0).sum()) > len(o) // 4
    if "oversize" in name:
        assert info0[4] == 1 and info0[5] == 1


def test_refusals_launch_nothing():
    """Every refusal of include/sapcu_ray.h returns SAPCU_ERR_ARG and leaves the prefilled outputs, the workspace and the guards alone."""
    v, f = mesh("ico1280")
    o, d, tm = rays("sampler", v, f, 300, 6)
    arena = Arena("guard", fill=0xFF, device=U.dev())
    bufs = _buffers(arena, o, d, tm, v, f)
    L = _lib()
    wsp = bufs["ws"].data_ptr()
    refusals = [dict(v=None), dict(f=None), dict(o=None), dict(d=None), dict(t=None), dict(nv=0), dict(nv=-3), dict(nf=0), dict(nf=-1),
                dict(nq=-1), dict(nv=1 << 31), dict(nf=(1 << 29) + 1), dict(nq=(1 << 31) - 63), dict(nbytes=bufs["nbytes"] - 1),
                dict(nbytes=0), dict(ws=None), dict(ws=ctypes.c_void_p(wsp + 4)), dict(ws=ctypes.c_void_p(wsp + 1)), dict(cell=-1.0),
                dict(cell=float("nan")), dict(cell=float("inf"))]
    for over in refusals:
        rc, info = _launch(bufs, over.pop("cell", 0.0), True, **over)
        assert rc == -1 and info == [5] * 6, over
        assert L.load().sapcu_last_error()
        arena.check()
        for name in ("t", "face", "hit"):
            assert bool((bufs[name].contiguous().view(U8) == 0xFF).all()), (over, name)
    assert bool((bufs["ws"] == 0xFF).all())
    rc, info = _launch(bufs, 0.0, True)                        # and the same buffers are accepted as they are
    assert rc == 0 and info[0] == 1
    arena.check()
    rc, info = _launch(bufs, 0.0, True, nq=0, o=None, d=None, t=None)     # no ray: nothing is launched, nothing is written
    assert rc == 0 and info == [0] * 6


def _sampler_buffers(arena, v, f, surf, sface, g, w, offsets=(8, 4, 24, 8, 16, 8, 8, 16, 8, 3, 8)):
    lib = _lib().load()
    n, nv, nf = len(surf), len(v), len(f)
    nbytes = int(lib.sapcu_ray_fd_samples_workspace_bytes(nv, nf, n))
    assert nbytes > 0
    k = offsets
    return {"v": arena.inp(np.ascontiguousarray(v, dtype=np.float64), offset=k[0], name="vertices"),
            "f": arena.inp(np.ascontiguousarray(f, dtype=np.int32), offset=k[1], name="faces"),
            "surf": arena.inp(np.ascontiguousarray(surf, dtype=np.float64), offset=k[2], name="surf"),
            "sface": arena.inp(np.ascontiguousarray(sface, dtype=np.int64), offset=k[3], name="sface"),
            "g": arena.inp(np.ascontiguousarray(g, dtype=np.float64), offset=k[4], name="g"),
            "w": arena.inp(np.ascontiguousarray(w, dtype=np.float64), offset=k[5], name="w"),
            "points": arena.out((n, 3), F64, offset=k[6], name="points"), "normals": arena.out((n, 3), F64, offset=k[7], name="normals"),
            "lens": arena.out((n,), F64, offset=k[8], name="lens"), "keep": arena.out((n,), U8, offset=k[9], name="keep"),
            "ws": arena.ws(nbytes, offset=k[10], name="workspace"), "nbytes": nbytes}


def _sampler_launch(b, cell, **over):
    L = _lib()
    lib = L.load()
    info = (ctypes.c_int64 * 6)(5, 5, 5, 5, 5, 5)
    a = {k: L.ptr(b[k]) for k in ("v", "f", "surf", "sface", "g", "w", "points", "normals", "lens", "keep", "ws")}
    a.update(nv=b["v"].shape[0], nf=b["f"].shape[0], n=b["surf"].shape[0], cell=float(cell), nbytes=b["nbytes"])
    a.update(over)
    rc = lib.sapcu_ray_fd_samples_f64(a["v"], a["nv"], a["f"], a["nf"], a["surf"], a["sface"], a["g"], a["w"], a["n"], a["cell"], a["points"],
                                      a["normals"], a["lens"], a["keep"], a["ws"], a["nbytes"], info, L.current_stream())
    torch.cuda.synchronize()
    return rc, list(info)


@pytest.mark.parametrize("name,cell,route", [("ico", 0.0, 0), ("ico", 0.4, 1), ("small", 0.0, 0)])
def test_the_sampler_entry_point_under_guard_bands_against_the_definition(name, cell, route):
    """sapcu_ray_fd_samples_f64 on the cases of tests/test_ray_host.py: the three runs of DESIGN 2, and every output of every sample
    (kept or not) bit-equal to ray_ref.fd_samples."""
    v, f, surf, sface, g, w, ref = H.sampler_case(name)
    results = []
    for fill in (0xFF, 0x00):
        arena = Arena("guard", fill=fill, device=U.dev())
        bufs = _sampler_buffers(arena, v, f, surf, sface, g, w)
        for again in range(2 if fill == 0x00 else 1):
            arena.refill_outputs()
            rc, info = _sampler_launch(bufs, cell)
            assert rc == 0, _lib().load().sapcu_last_error()
            arena.check()
            results.append(tuple(bufs[k].clone() for k in ("points", "normals", "lens", "keep")) + (info,))
    first = results[0]
    assert first[4][0] == route
    for r in results[1:]:
        assert all(_same(x, y) for x, y in zip(r[:4], first[:4])) and r[4] == first[4]
    assert _same(first[0], ref["points"]) and _same(first[1], ref["normals"]) and _same(first[2], ref["lens"])
    assert np.array_equal(first[3].cpu().numpy().astype(bool), ref["keep"]) and bool((first[3] <= 1).all())


def test_sampler_refusals_launch_nothing():
    v, f, surf, sface, g, w, _ = H.sampler_case("ico")
    arena = Arena("guard", fill=0xFF, device=U.dev())
    bufs = _sampler_buffers(arena, v, f, surf[:300], sface[:300], g[:300], w[:300], offsets=(0,) * 10 + (8,))
    wsp = bufs["ws"].data_ptr()
    refusals = [{k: None} for k in ("v", "f", "surf", "sface", "g", "w", "points", "normals", "lens", "keep", "ws")]
    refusals += [dict(nv=0), dict(nf=0), dict(n=-1), dict(nv=1 << 31), dict(nf=(1 << 29) + 1), dict(n=(1 << 31) - 63),
                 dict(nbytes=bufs["nbytes"] - 1), dict(nbytes=0), dict(ws=ctypes.c_void_p(wsp + 4)), dict(cell=-1.0), dict(cell=float("nan")),
                 dict(cell=float("inf"))]
    for over in refusals:
        rc, info = _sampler_launch(bufs, over.pop("cell", 0.0), **over)
        assert rc == -1 and info == [5] * 6, over
        arena.check()
        for name in ("points", "normals", "lens", "keep"):
            assert bool((bufs[name].contiguous().view(U8) == 0xFF).all()), (over, name)
    assert bool((bufs["ws"] == 0xFF).all())
    rc, info = _sampler_launch(bufs, 0.0)
    assert rc == 0 and info[0] == 0
    arena.check()
    rc, info = _sampler_launch(bufs, 0.0, n=0, surf=None, sface=None, g=None, w=None, points=None, normals=None, lens=None, keep=None)
    assert rc == 0 and info == [0] * 6


def test_every_pointer_taking_entry_point_of_the_header_runs_under_guards():
    decl = H.header_entry_points()
    assert set(decl) == set(_lib().RAY_EXPORTS)
    assert {n for n in decl if "*" in decl[n]} == {"sapcu_ray_mesh_f64", "sapcu_ray_fd_samples_f64"}     # _launch / _sampler_launch above
    assert {n for n in decl if n.endswith("workspace_bytes")} == {"sapcu_ray_mesh_workspace_bytes", "sapcu_ray_fd_samples_workspace_bytes"}


# ------------------------------------------------------------------------------------------------------ the sampler
_DRAWS = {}


def sampler_reference(name, n=4096):
    """The tables of one mesh, n draws, the device's own surface points (``sample_surface``, tested in test_gpu_surface.py) and
    ``ray_ref.fd_samples`` on them, computed once per session; samples are independent, so the first k are the reference of k draws."""
    from sapcu_amd import surface
    if name not in _DRAWS:
        v, f = {"ico": lambda: R.icosphere(3), "torus": lambda: R.torus(24, 16)}[name]()
        tables = surface.build_surface_tables([(R.BOX_V.astype(np.float32), R.BOX_F), (v.astype(np.float32), f)], device=U.dev())
        gen = torch.Generator(device=U.dev())
        gen.manual_seed(len(name))
        u = torch.rand((n,), generator=gen, device=U.dev(), dtype=F64)
        r1 = torch.rand((n,), generator=gen, device=U.dev(), dtype=F64).float()
        r2 = torch.rand((n,), generator=gen, device=U.dev(), dtype=F64).float()
        g = torch.randn((n, 3), generator=gen, device=U.dev(), dtype=F64)
        w = torch.rand((n,), generator=gen, device=U.dev(), dtype=F64)
        idx = torch.ones((1,), dtype=I64, device=U.dev())
        surf, _, sface = surface.sample_surface(tables, idx, n, u.reshape(1, n), r1.reshape(1, n), r2.reshape(1, n))
        ref = R.fd_samples(v.astype(np.float32).astype(np.float64), f, surf[0].double().cpu().numpy(), sface[0].cpu().numpy(),
                           g.cpu().numpy(), w.cpu().numpy())
        _DRAWS[name] = (tables, (u, r1, r2, g, w), ref)
    return _DRAWS[name]


@pytest.mark.parametrize("name", ["ico", "torus"])
def test_sample_fd_rays_against_the_numpy_restatement(name):
    from sapcu_amd import ray
    tables, draws, ref = sampler_reference(name)
    assert 300 < ref["keep"].sum() < 1200
    for n in (1, 64, 4096):
        keep, points, normals, lens = ray.sample_fd_rays(tables, 1, *(x[:n] for x in draws))
        k = ref["keep"][:n]
        assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), k), (name, n)
        assert points.dtype == normals.dtype == lens.dtype == torch.float32
        for got, key in ((points, "points"), (normals, "normals"), (lens, "lens")):
            want = ref[key][:n][k].astype(np.float32)
            assert got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (name, n, key)
    npz = ray.as_fd_npz(points, normals, lens)
    assert npz["lens"].shape == (int(ref["keep"].sum()), 3) and np.array_equal(npz["points"], points.cpu().numpy())
    # any cell size: the same samples
    again = ray.sample_fd_rays(tables, 1, *draws, cell_size=0.2)
    assert all(_same(a, b) for a, b in zip(again, (keep, points, normals, lens)))


def test_sample_fd_rays_refuses_open_meshes_and_bad_input():
    from sapcu_amd import ray, surface
    v, f = R.icosphere(2)
    tables = surface.build_surface_tables([(v.astype(np.float32), f[:-1]), (v.astype(np.float32), np.concatenate([f, f[:1]]))], device=U.dev())
    n = 64
    gen = torch.Generator(device=U.dev())
    gen.manual_seed(1)
    u = torch.rand((n,), generator=gen, device=U.dev(), dtype=F64)
    r1, r2 = u.float(), (1 - u).float()
    g = torch.randn((n, 3), generator=gen, device=U.dev(), dtype=F64)
    for m in (0, 1):
        with pytest.raises(ValueError, match="watertight"):
            ray.sample_fd_rays(tables, m, u, r1, r2, g, u)
    keep, points, normals, lens = ray.sample_fd_rays(tables, 0, u, r1, r2, g, u, allow_open=True)
    assert keep.shape == (n,) and points.shape == (int(keep.sum()), 3) and lens.shape == (int(keep.sum()),)
    with pytest.raises(ValueError):
        ray.sample_fd_rays(tables, 2, u, r1, r2, g, u, allow_open=True)
    with pytest.raises(ValueError):
        ray.sample_fd_rays(tables, 0, u, r1, r2, g[:, :2], u, allow_open=True)
    with pytest.raises(ValueError):
        ray.sample_fd_rays(tables, 0, u, r1[:5], r2, g, u, allow_open=True)
    with pytest.raises(RuntimeError):
        ray.sample_fd_rays(tables, 0, u.cpu(), r1, r2, g, u, allow_open=True)
    with pytest.raises(ValueError):
        ray.sample_fd_rays(None, 0, u, r1, r2, g, u)
    e = u[:0]
    keep, points, normals, lens = ray.sample_fd_rays(tables, 0, e, e.float(), e.float(), g[:0], e, allow_open=True)
    assert keep.shape == (0,) and points.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ the higher layers
def _numpy_signed(o, n, v, f, t_max=None):
    tp, fp, _, _ = R.ray_mesh(o, n, v, f, t_max=t_max)
    tn, fn, _, _ = R.ray_mesh(o, -n, v, f, t_max=t_max)
    fwd = tp <= tn
    face = np.where(fwd, fp, fn)
    return np.where(face >= 0, np.where(fwd, tp, -tn), np.nan), face


def test_signed_ray_distance_and_ray_metrics_equal_numpy():
    from sapcu_amd import ray
    v, f = R.icosphere(2)
    rng = np.random.default_rng(12)
    p = rng.normal(size=(700, 3))
    p = p / np.linalg.norm(p, axis=1)[:, None] * rng.uniform(0.7, 1.2, size=(700, 1))
    n = p / np.linalg.norm(p, axis=1)[:, None] + rng.normal(size=(700, 3)) * 0.2
    n /= np.linalg.norm(n, axis=1)[:, None]
    for t_max in (None, 0.1, np.where(np.arange(700) % 2 == 0, 0.05, np.inf)):
        d, face = ray.signed_ray_distance(p, n, v, f, t_max=t_max)
        tm = None if t_max is None else np.broadcast_to(np.asarray(t_max, dtype=np.float64), (700,))
        rd, rf = _numpy_signed(p, n, v, f, tm)
        assert _same(d, rd) and _same(face, rf)
        got = rf >= 0
        assert got.sum() > 100 and (t_max is None or (~got).sum() > 50)
        assert (rd[got & (np.linalg.norm(p, axis=1) > 1.0)] < 0).all() and (rd[got & (np.linalg.norm(p, axis=1) < 0.93)] > 0).all()
        pred = rng.normal(size=700) * 0.05
        e = np.abs(pred[got] - rd[got])
        with np.errstate(all="ignore"):
            want = {"ray_mean": np.mean(e), "ray_std": np.sqrt(np.sum((e - np.mean(e)) ** 2) / np.float64(len(e) - 1)), "ray_min": e.min(),
                    "ray_max": e.max(), "n": int(got.sum()), "n_missed": int((~got).sum()), "n_faces": len(f), "n_skipped": 0}
        old = np.getbufsize()
        try:
            for bufsize in (old, 4096):
                np.setbufsize(bufsize)
                m = ray.ray_metrics(_dev(p), _dev(n), _dev(pred), v, f, t_max=t_max)
                assert sorted(m) == sorted(want)
                for k in want:
                    assert m[k] == want[k], (k, m[k], want[k], bufsize)
                    assert not k.startswith("ray_") or isinstance(m[k], np.float64)
        finally:
            np.setbufsize(old)
    # the displacement step: p + n * d is the hit point
    d, face = ray.signed_ray_distance(p, n, v, f)
    from sapcu_amd import mesh as mesh_mod
    moved = _dev(p) + _dev(n) * d[:, None]
    assert float(mesh_mod.point_to_mesh(moved, v, f)[0].max()) <= 1e-9
    m = ray.ray_metrics(p, n, d.cpu().numpy(), v, f)
    assert m["ray_max"] == 0.0 and m["ray_mean"] == 0.0 and m["n_missed"] == 0
    with pytest.raises(ValueError):
        ray.ray_metrics(p * 10, n, np.zeros(700), v, f, t_max=0.5)                              # no point meets the mesh
    with pytest.raises(ValueError):
        ray.ray_metrics(p, n, np.zeros(5), v, f)
    skipped = np.concatenate([f, [[0, 0, 1]]])
    assert ray.ray_metrics(p, n, np.zeros(700), v, skipped)["n_skipped"] == 1


def test_python_layer_inputs_and_errors():
    from sapcu_amd import ray
    v, f = R.icosphere(2)
    o, d, _ = rays("outside", v, f, 200, 8)
    want = ray.ray_to_mesh(_dev(o), _dev(d), _dev(v), _dev(f, np.int64))
    assert int((want[1] >= 0).sum()) > 50
    for faces in (f.astype(np.int64), f.astype(np.uint16), _dev(f, np.int32)):
        assert all(_same(a, b) for a, b in zip(ray.ray_to_mesh(o, _dev(d), v, faces), want))
    assert all(_same(a, b) for a, b in zip(ray.ray_to_mesh(o, d, v, f, t_max=np.inf), want))
    assert all(_same(a, b) for a, b in zip(ray.ray_to_mesh(o, d, v, f, t_max=torch.full((200,), float("inf"), device=U.dev())), want))
    info = [9]
    t, face, hit = ray.ray_to_mesh(o[:0], d[:0], v, f, info=info)                               # no ray: nothing is launched
    assert t.shape == (0,) and face.shape == (0,) and hit.shape == (0, 3) and t.dtype == F64 and face.dtype == I64 and info == [0] * 6
    for bad in (f + len(v), f - 1):
        with pytest.raises(ValueError):
            ray.ray_to_mesh(o, d, v, bad)
    with pytest.raises(ValueError):
        ray.ray_to_mesh(o, d[:100], v, f)
    with pytest.raises(ValueError):
        ray.ray_to_mesh(o, d, v, f, t_max=np.ones(5))
    with pytest.raises(ValueError):
        ray.ray_to_mesh(o[:, :2], d, v, f)
    for args in ((torch.from_numpy(o), d, v, f), (o, torch.from_numpy(d), v, f), (o, d, torch.from_numpy(v), f)):
        with pytest.raises(RuntimeError):
            ray.ray_to_mesh(*args)
    with pytest.raises(RuntimeError):
        ray.ray_to_mesh(o, d, v, f, t_max=torch.ones(200))


def test_fd_ray_patches_yield_the_same_items_from_the_same_seed(tmp_path):
    import sapcu_amd
    from sapcu_amd import ray
    meshes = [(v.astype(np.float32), f) for v, f in (R.icosphere(2), R.torus(16, 10), R.icosphere(1, radius=0.5))]
    a = list(sapcu_amd.FdRayPatches(meshes, num_rays=2048, split="all", seed=3, device=U.dev()))
    b = list(sapcu_amd.FdRayPatches(meshes, num_rays=2048, split="all", seed=3, device=U.dev()))
    c = list(sapcu_amd.FdRayPatches(meshes, num_rays=2048, split="all", seed=4, device=U.dev()))
    assert len(a) == len(b) == 3 and sorted(x["index"] for x in a) == [0, 1, 2]
    for x, y in zip(a, b):
        assert x["index"] == y["index"] and set(x) == {None, "input", "cloud", "normal", "len", "index", "keep"}
        for k in (None, "normal", "len", "keep"):
            assert torch.equal(x[k], y[k]), k
        K = int(x["keep"].sum())
        assert 100 < K < 1000 and x[None].shape == (K, 3) and x["normal"].shape == (K, 3) and x["len"].shape == (K, 3)
        assert x[None].dtype == x["normal"].dtype == x["len"].dtype == torch.float32 and x[None].is_cuda
        assert torch.equal(x["len"][:, 0], x["len"][:, 2]) and float(x["len"].min()) >= 0.003 and float(x["len"].max()) <= 0.03
    assert any(x["index"] != y["index"] or x[None].shape != y[None].shape or not torch.equal(x[None], y[None]) for x, y in zip(a, c))
    loader = sapcu_amd.FdRayPatches(meshes, num_rays=512, split="all", shuffle=False, seed=3, device=U.dev())
    first = [x[None].clone() for x in loader]
    again = [x[None].clone() for x in loader.set_epoch(1)]
    assert any(p.shape != q.shape or not torch.equal(p, q) for p, q in zip(first, again))        # a fresh sampling per epoch
    # the item is what sample_fd_rays gives on the loader's own draws, and it saves as the reference's fd.npz
    item = loader.sample(1)
    keep, points, normals, lens = ray.sample_fd_rays(loader.tables, 1, **loader.last_draws)
    assert torch.equal(item[None], points) and torch.equal(item["normal"], normals) and torch.equal(item["len"][:, 1], lens)
    np.savez(str(tmp_path / "fd.npz"), **ray.as_fd_npz(points, normals, lens))
    back = np.load(str(tmp_path / "fd.npz"))
    assert np.array_equal(back["lens"], item["len"].cpu().numpy()) and np.array_equal(back["points"], item[None].cpu().numpy())
    with pytest.raises(ValueError, match="watertight"):
        list(sapcu_amd.FdRayPatches([(meshes[0][0], meshes[0][1][:-1])], split="all", device=U.dev()))
    assert len(list(sapcu_amd.FdRayPatches([(meshes[0][0], meshes[0][1][:-1])], num_rays=64, split="all", device=U.dev(), allow_open=True))) == 1


def test_python_entry_points_do_not_depend_on_what_an_allocation_returns(monkeypatch):
    """ray_to_mesh, signed_ray_distance, ray_metrics, sample_fd_rays and FdRayPatches run clean, then under both patterns of
    tests/poison.py: bit-identical results (the workspace and the outputs never come from torch.empty)."""
    import poison
    import sapcu_amd
    from sapcu_amd import ray
    v, f = mesh("ico1280")
    o, d, tm = rays("sampler", v, f, 1000, 40)
    oo, od, _ = rays("outside", v, f, 1000, 41)
    tables, draws, _ = sampler_reference("ico")
    nrm = od / np.linalg.norm(od, axis=1)[:, None]
    meshes = [(v.astype(np.float32), f)]

    def run():
        a = ray.ray_to_mesh(o, d, v, f, t_max=tm)
        b = ray.ray_to_mesh(oo, od, v, f, cell_size=0.3)
        c = ray.signed_ray_distance(oo, nrm, v, f)
        s = ray.sample_fd_rays(tables, 1, *draws)
        item = next(iter(sapcu_amd.FdRayPatches(meshes, num_rays=1024, split="all", seed=5, device=U.dev())))
        return a, b, c, s, (item[None], item["normal"], item["len"]), ray.ray_metrics(oo, nrm, np.zeros(1000), v, f)

    clean = run()
    for pattern in poison.PATTERNS:
        with poison.poisoned(monkeypatch, pattern):
            got = run()
        for k in range(5):
            assert all(_same(x, y) if x.dtype == F64 or x.dtype == I64 else torch.equal(x, y) for x, y in zip(got[k], clean[k])), (pattern, k)
        assert got[5] == clean[5], pattern
