"""Point-to-surface distance on the device (-m gpu; include/sapcu_mesh.h, csrc/mesh_dist.hip, sapcu_amd/mesh.py).

The brute-force kernel must equal the numpy definition (tests/mesh_ref.py) bit for bit on distance, face and closest point; the
grid route must equal the brute-force kernel bit for bit for any cell size, for queries anywhere (inside, outside, 1e12 extents
away), with oversize, skipped and duplicated faces; the entry point keeps the memory contract of DESIGN §2 under guard bands;
``mesh_metrics`` equals numpy (``==``) on the device's own distances at two buffer sizes, and every value the reference's CGAL tool
printed (tests/golden/mesh_p2f.npz) within what its six digits allow."""
import ctypes

import numpy as np
import pytest
import torch

import gpu_utils as U
import mesh_ref as M
import test_mesh_host as H
from conftest import golden
from guarded import Arena

pytestmark = pytest.mark.gpu

F64, I64, I32 = torch.float64, torch.int64, torch.int32
CASES = H.CASES


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


def device_call(points, vertices, faces, cell=0.0, brute=False, mult=2.0, pop=4):
    """sapcu_internal_point_mesh_tuned on compact tensors (the public entry point with its two constants given, or forced to the
    brute-force route) -> (dist, face, closest, info)."""
    L = _lib()
    lib = L.load()
    p, v, f = _dev(points), _dev(vertices), _dev(faces, np.int32)
    nq, nv, nf = p.shape[0], v.shape[0], f.shape[0]
    dist = torch.full((nq,), 7.0, dtype=F64, device=U.dev())
    face = torch.full((nq,), -7, dtype=I64, device=U.dev())
    clo = torch.full((nq, 3), 7.0, dtype=F64, device=U.dev())
    nbytes = int(lib.sapcu_point_mesh_workspace_bytes(nv, nf, nq))
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=U.dev())
    info = (ctypes.c_int64 * 6)()
    L.check(lib.sapcu_internal_point_mesh_tuned(L.ptr(v), nv, L.ptr(f), nf, L.ptr(p), nq, float(cell), float(mult), int(pop), int(brute),
                                                L.ptr(dist), L.ptr(face), L.ptr(clo), L.ptr(ws), nbytes, info, L.current_stream()))
    torch.cuda.synchronize()
    return dist, face, clo, list(info)


def assert_equals_definition(points, vertices, faces, what, ref=None):
    dist, face, clo, info = device_call(points, vertices, faces, brute=True)
    rd, rf, rc, _, skipped = ref if ref is not None else M.point_mesh(points, vertices, faces)
    assert info[0] == 0 and info[5] == skipped, (what, info, skipped)
    bad = ~(((_bits(dist) == _bits(rd)) | (torch.isnan(dist.cpu()) & torch.isnan(torch.as_tensor(rd)))) & (face.cpu() == torch.as_tensor(rf)))
    assert not bool(bad.any()), "%s: %d of %d queries differ from the definition, first %d: (%r, %d) against (%r, %d)" % (
        what, int(bad.sum()), bad.numel(), int(bad.nonzero()[0]), dist[bad][0].item(), face[bad][0].item(), rd[bad.numpy()][0],
        rf[bad.numpy()][0])
    assert _same(clo, rc), what
    return dist, face, clo


def assert_grid_equals_brute(points, vertices, faces, cell, what, route=None, brute=None, **tuning):
    b = brute if brute is not None else device_call(points, vertices, faces, brute=True)
    g = device_call(points, vertices, faces, cell=cell, **tuning)
    assert b[3][0] == 0
    bad = ~((_bits(g[0]) == _bits(b[0])) | (torch.isnan(g[0].cpu()) & torch.isnan(b[0].cpu()))) | (g[1] != b[1]).cpu()
    assert not bool(bad.any()), "%s cell %g: %d of %d queries differ, first %d: (%r, %d) against brute force (%r, %d)" % (
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


def torus(nu, nw, R=0.35, r=0.12):
    u, w = np.arange(nu) * (2 * np.pi / nu), np.arange(nw) * (2 * np.pi / nw)
    gu, gw = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(gw)) * np.cos(gu), (R + r * np.cos(gw)) * np.sin(gu), r * np.sin(gw)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nw), indexing="ij")
    idx = lambda a, b: (a % nu) * nw + (b % nw)
    f = np.concatenate([np.stack([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], -1).reshape(-1, 3),
                        np.stack([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)], -1).reshape(-1, 3)])
    return v, f


def case(name):
    g = golden("mesh_p2f.npz")
    return g[name + "/points"], g[name + "/vertices"], g[name + "/faces"]


# --------------------------------------------------------------------------------- brute force against the definition
@pytest.mark.parametrize("nf", [1, 2, 63, 64, 65, 130, 1000])
def test_brute_force_equals_the_definition_at_tile_and_wave_edges(nf):
    v, f = soup(nf, nf)
    rng = np.random.default_rng(1000 + nf)
    q = rng.uniform(-0.5, 1.5, size=(200, 3))
    ref = M.point_mesh(q, v, f)
    for nq in (1, 63, 64, 65, 200):
        assert_equals_definition(q[:nq], v, f, "nf=%d nq=%d" % (nf, nq), ref=tuple(r[:nq] if i < 4 else r for i, r in enumerate(ref)))


@pytest.mark.parametrize("name", CASES)
def test_brute_force_equals_the_definition_on_the_fixture(name):
    p, v, f = case(name)
    if name in ("ico", "torus"):                                # a 512-point subset: numpy stays under a second
        p = p[:512]
        ref = tuple(r[:512] if i < 4 else r for i, r in enumerate(H._REF[name])) if name in H._REF else M.point_mesh(p, v, f)
    else:
        ref = H.reference(name)
    dist, face, clo = assert_equals_definition(p, v, f, name, ref=ref)
    rec = golden("mesh_p2f.npz")[name + "/dist"][:len(p)]
    assert bool((np.abs(dist.cpu().numpy() - rec) <= 1e-5 * rec + 1e-12).all())


def test_brute_force_ties_duplicates_skipped_faces_and_a_nan_query():
    p, v, f = case("box")
    rng = np.random.default_rng(5)
    q = rng.integers(-8, 13, size=(300, 3)).astype(np.float64)
    dist, face, clo = assert_equals_definition(q, v * 4.0, f, "integer box")                  # exact ties: the lowest face index
    dd, _ = M.all_d2(q, v * 4.0, f)
    assert np.array_equal(face.cpu().numpy(), np.argmax(dd == dd.min(1)[:, None], axis=1))
    dup = np.concatenate([f[::-1], f, f])                                                     # every face three times
    _, face, _ = assert_equals_definition(p[:500], v, dup, "duplicated faces")
    assert int(face.max()) < 12
    sv = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 1], [1, 1, 1.0]])
    sf = np.array([[0, 1, 3], [0, 0, 2], [1, 1, 1], [0, 1, 6], [0, -1, 2], [0, 1, 2], [0, 1, 2], [1, 0, 2], [0, 1, 4]])
    sq = np.concatenate([np.array([[0.25, 0.25, -0.5], [3.0, 0.0, 0.0], [0.2, -1.0, 0.2], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]]),
                         rng.uniform(-1, 2, size=(100, 3))])
    dist, face, clo = assert_equals_definition(sq, sv, sf, "skipped faces")
    assert face[:5].tolist() == [5, 5, 8, -1, -1] and bool(torch.isnan(dist[3:5]).all()) and bool(torch.isnan(clo[3:5]).all())
    dist, face, clo = assert_equals_definition(sq, sv, sf[:5], "every face skipped")
    assert bool((face == -1).all()) and bool(torch.isnan(dist).all()) and bool(torch.isnan(clo).all())
    big = np.array([[0, 0, 0], [1e200, 0, 0], [0, 1e200, 0.0], [1, 0, 0], [0, 1, 0]])
    assert_equals_definition(sq[:3], big, np.array([[0, 1, 2], [0, 3, 4]]), "a face whose normal overflows")


# ------------------------------------------------------------------------------------------- grid against brute force
# two cell edges per fixture mesh at which the grid runs at a cap of one edge (the largest radii: box 0.75, sheet 0.048, torus 0.032;
# the reference's Icosahedron.off has radii from 0.019 to 0.65, 164 of its 5120 faces above 0.5: an oversize list of its own), and one
# far below every face's size: the cell edge then grows until the grid fits its cell budget, or the call falls back to brute force
GRID_CELLS = {"ico": (0.5, 0.12), "box": (10.0, 2.0), "sheet": (0.3, 0.08), "torus": (0.12, 0.06)}


def radii(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    g = ((a + b) + c) / 3.0
    return np.sqrt(np.maximum(np.maximum(((a - g) ** 2).sum(1), ((b - g) ** 2).sum(1)), ((c - g) ** 2).sum(1)))


def _cells(name, v):
    ext = float((v.max(0) - v.min(0)).max())
    return ext, GRID_CELLS[name] + (ext / 100,)


@pytest.mark.parametrize("name", CASES)
def test_grid_equals_brute_force_on_the_fixture(name):
    p, v, f = case(name)
    ext, cells = _cells(name, v)
    brute = None
    for cell in cells + (0.0,):
        for mult in (0.5, 1.0, 2.0):
            info, brute = assert_grid_equals_brute(p, v, f, cell, name, brute=brute, mult=mult)
            if cell == 0.0 and mult >= 1.0:
                assert info[0] == (1 if len(f) >= 1280 else 0), (name, info)
            if cell in GRID_CELLS[name] and mult >= 1.0:
                assert info[0] == 1 and info[4] == int((radii(v, f) > mult * cell).sum()), (name, cell, info)
                assert name != "ico" or mult > 1.0 or info[4] in (164, 620)       # the reference's mesh has an oversize list of its own
    from sapcu_amd import mesh
    info = []
    d, fa, c = mesh.point_to_mesh(p, v, f, info=info)          # the public entry point: the same bits, the automatic route
    assert _same(d, brute[0]) and _same(fa, brute[1]) and _same(c, brute[2]) and info[0] == (1 if len(f) >= 1280 else 0)
    d, fa, c = mesh.point_to_mesh(p, v, f, cell_size=cells[1], info=info)
    assert _same(d, brute[0]) and _same(fa, brute[1]) and _same(c, brute[2]) and info[0] == 1 and info[5] == 0


def test_far_queries():
    """Queries 1e6, 1e9 and 1e12 extents outside along every axis and diagonal: the slack must cover their magnitude."""
    rng = np.random.default_rng(8)
    dirs = [s * np.eye(3)[a] for a in range(3) for s in (1.0, -1.0)]
    dirs += [np.array([sx, sy, sz]) for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]
    dirs += [np.array([1.0, 1.0, 0.0]), np.array([0.0, -1.0, 1.0])]
    for name in ("torus", "sheet"):
        _, v, f = case(name)
        ext, cells = _cells(name, v)
        base = rng.uniform(v.min(0), v.max(0), size=(8, 3))
        q = np.concatenate([base + d * s * ext for s in (1e6, 1e9, 1e12) for d in dirs] + [base])
        brute = None
        for cell in (0.0, cells[0], cells[1], cells[2]):
            _, brute = assert_grid_equals_brute(q, v, f, cell, "far/" + name, brute=brute, route=1 if cell in cells[:2] else None)
        # and a mesh far from the origin: the vertices' magnitude
        _, brute = assert_grid_equals_brute(np.concatenate([base, q[:40] / ext]) + 1e6, v + 1e6, f, cells[1], "shifted/" + name, route=1)


def test_chunks_of_one_cell():
    """1000 queries inside one cell (sixteen chunks, the last one ragged), and cells that hold exactly 64 and 65 queries."""
    _, v, f = case("torus")
    rng = np.random.default_rng(7)
    lo = (((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / 3.0).min(0)                  # the grid's origin: the centroids' box
    h = 0.2
    q = np.concatenate([lo + h * (1 + rng.uniform(0.05, 0.95, size=(1000, 3))), lo + h * (2 + rng.uniform(0.05, 0.95, size=(64, 3))),
                        lo + h * rng.uniform(0.05, 0.95, size=(65, 3))])
    q = q[rng.permutation(len(q))]
    info, _ = assert_grid_equals_brute(q, v, f, h, "chunks", route=1)
    assert info[1] >= 3 and info[2] >= 3


def test_the_oversize_list_and_the_fallback():
    p, v, f = case("torus")
    lo, hi = v.min(0) - 0.2, v.max(0) + 0.2
    v2 = np.concatenate([v, [lo, [hi[0], lo[1], hi[2]], [lo[0], hi[1], hi[2]]]])               # one face spanning the whole box
    f2 = np.concatenate([f[:2000], [[len(v), len(v) + 1, len(v) + 2]], f[2000:]])
    ext, cells = _cells("torus", v)
    brute = None
    for cell, mult in ((0.0, 1.0), (0.12, 0.5), (0.12, 1.0), (0.12, 2.0), (0.3, 1.0)):
        info, brute = assert_grid_equals_brute(p, v2, f2, cell, "one big face", brute=brute, route=1, mult=mult)
        assert info[4] >= 1 and info[4] * 4 <= len(f2), info
    assert int((brute[1] == 2000).sum()) > 0                                                    # the big face does win somewhere
    # the same cap at three multiples: the list shrinks as the cap grows, the results do not move
    sizes = [assert_grid_equals_brute(p, v, f, 0.032, "cap", mult=m)[0][4] for m in (0.5, 1.0, 2.0)]
    assert sizes[0] == len(f) and sizes[0] >= sizes[1] >= sizes[2] and sizes[2] < len(f) // 4
    # every face oversize: the brute-force route, and the list's size is reported
    bp, bv, bf = case("box")
    info, _ = assert_grid_equals_brute(bp, bv, bf, 0.1, "all oversize", route=0)
    assert info == [0, 0, 0, 0, 12, 0]
    info, _ = assert_grid_equals_brute(bp, bv, bf, 10.0, "one cell", route=1)
    assert info == [1, 1, 1, 1, 0, 0]
    # skipped faces inside a grid: reported, and they take no part
    f3 = np.concatenate([f, [[0, 0, 1], [5, 5, 5], [0, len(v), 1], [-1, 2, 3]]])
    info, _ = assert_grid_equals_brute(p, v, f3, cells[1], "skipped in the grid", route=1)
    assert info[5] == 4


def test_a_large_mesh_grid_against_device_brute_force():
    """20 000 faces and 20 000 queries, near the surface and anywhere in three times the box: numpy would take a minute, so the device
    brute force, which the tests above tie to the definition, is the reference."""
    v, f = torus(100, 100)
    assert len(f) == 20000
    rng = np.random.default_rng(20)
    q = np.concatenate([v[rng.integers(0, len(v), 10000)] + rng.normal(size=(10000, 3)) * 0.004, rng.uniform(-1.5, 1.5, size=(10000, 3))])
    q = q[rng.permutation(len(q))]
    info, brute = assert_grid_equals_brute(q, v, f, 0.0, "large", route=1)
    assert info[1] > 4 and info[2] > 4 and info[4] == 0 and info[5] == 0
    for pop in (4, 64):
        assert_grid_equals_brute(q, v, f, 0.0, "large pop %d" % pop, brute=brute, route=1, pop=pop)
    assert 0 < float(brute[0].min()) < 1e-4 and float(brute[0].max()) > 1.0


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 1e200])
def test_non_finite_and_huge_coordinates_take_the_brute_force_route(bad):
    p, v, f = case("torus")
    p = p[:1000]
    v2 = v.copy()
    v2[777, 1] = bad
    p2 = p.copy()
    p2[500, 2] = bad
    ext, cells = _cells("torus", v)
    for cell in (0.0, cells[1]):
        assert_grid_equals_brute(p, v2, f, cell, "bad vertex", route=0)
        assert_grid_equals_brute(p2, v, f, cell, "bad query", route=0)
    assert_grid_equals_brute(p, v, f, 0.0, "clean", route=1)
    v3 = np.concatenate([v, [[bad, 0.0, 0.0]]])                 # a bad vertex no face uses: still the brute-force route
    assert_grid_equals_brute(p, v3, f, cells[1], "bad unused vertex", route=0)


# ------------------------------------------------------------------------------------------------- memory contract
def _buffers(arena, p, v, f, offsets=(0, 0, 0, 0, 0, 0, 8)):
    """The arena's buffers of one call; the workspace has exactly the sizer's size.  The ABI has no pitch for closest_out, so every
    buffer is compact; the bases are moved off the allocator's alignment by `offsets` (element-aligned, the workspace 8-byte)."""
    lib = _lib().load()
    nq, nv, nf = len(p), len(v), len(f)
    nbytes = int(lib.sapcu_point_mesh_workspace_bytes(nv, nf, nq))
    assert nbytes > 0
    o = offsets
    return {"v": arena.inp(np.ascontiguousarray(v, dtype=np.float64), offset=o[0], name="vertices"),
            "f": arena.inp(np.ascontiguousarray(f, dtype=np.int32), offset=o[1], name="faces"),
            "q": arena.inp(np.ascontiguousarray(p, dtype=np.float64), offset=o[2], name="queries"),
            "dist": arena.out((nq,), F64, offset=o[3], name="dist"), "face": arena.out((nq,), I64, offset=o[4], name="face"),
            "clo": arena.out((nq, 3), F64, offset=o[5], name="closest"), "ws": arena.ws(nbytes, offset=o[6], name="workspace"),
            "nbytes": nbytes}


def _launch(b, cell, optional, **over):
    L = _lib()
    lib = L.load()
    info = (ctypes.c_int64 * 6)(5, 5, 5, 5, 5, 5)
    a = {"v": L.ptr(b["v"]), "nv": b["v"].shape[0], "f": L.ptr(b["f"]), "nf": b["f"].shape[0], "q": L.ptr(b["q"]), "nq": b["q"].shape[0],
         "cell": float(cell), "dist": L.ptr(b["dist"]), "face": L.ptr(b["face"]) if optional else None,
         "clo": L.ptr(b["clo"]) if optional else None, "ws": L.ptr(b["ws"]), "nbytes": b["nbytes"]}
    a.update(over)
    rc = lib.sapcu_point_mesh_f64(a["v"], a["nv"], a["f"], a["nf"], a["q"], a["nq"], a["cell"], a["dist"], a["face"], a["clo"], a["ws"],
                                  a["nbytes"], info, L.current_stream())
    torch.cuda.synchronize()
    return rc, list(info)


def _guard_case(name):
    rng = np.random.default_rng(len(name))
    if name.startswith("grid-oversize"):
        p, v, f = case("torus")
        v = np.concatenate([v, [[-1, -1, -1], [1, -1, 1], [-1, 1, 1.0]]])
        f = np.concatenate([f, [[len(v) - 3, len(v) - 2, len(v) - 1], [0, 0, 1]]])
        return p[:1000 + 37], v, f, 0.0, 1
    if name.startswith("grid-forced-small"):
        p, v, f = case("box")
        return p[:129], v, f, 10.0, 1
    if name.startswith("grid"):
        p, v, f = case("torus")
        return p[:1000 + 37], v, f, 0.0, 1
    p, v, f = case("sheet")
    p = p[:200].copy()
    if "bad-query" in name:
        p[100, 0] = np.inf
        return p, v, f, 0.05, 0
    return p, v, f, 0.0, 0


GUARD_CASES = ["grid", "grid-no-optional", "grid-oversize", "grid-forced-small", "brute-small", "brute-small-no-optional",
               "brute-bad-query-no-optional"]


@pytest.mark.parametrize("name", GUARD_CASES)
def test_memory_contract_under_guard_bands(name):
    """The three runs of DESIGN §2: 0xFF bands and workspace with NaN-prefilled outputs, 0x00 bands and workspace, the dirty
    workspace again — guards intact, outputs written in full and bit-identical, and identical to the compact call.  Bases are
    moved off the allocator's alignment as far as the element types allow."""
    from sapcu_amd import mesh
    p, v, f, cell, route = _guard_case(name)
    optional = "no-optional" not in name
    results = []
    for fill in (0xFF, 0x00):
        arena = Arena("guard", fill=fill, device=U.dev())
        bufs = _buffers(arena, p, v, f, offsets=(8, 4, 24, 8, 16, 8, 8))
        for again in range(2 if fill == 0x00 else 1):
            arena.refill_outputs()
            rc, info = _launch(bufs, cell, optional)
            assert rc == 0, _lib().load().sapcu_last_error()
            arena.check()
            results.append((bufs["dist"].clone(), bufs["face"].clone(), bufs["clo"].clone(), info))
    d0, f0, c0, info0 = results[0]
    assert info0[0] == route, info0
    for d, fa, c, info in results[1:]:
        assert _same(d, d0) and _same(fa, f0) and _same(c, c0) and info == info0
    cd, cf, cc = mesh.point_to_mesh(p, v, f, cell)
    assert _same(cd, d0)
    if optional:
        assert _same(cf, f0) and _same(cc, c0)
    else:                                                      # NULL outputs: the buffers that were not passed are untouched
        assert bool((f0 == -1).all()) and bool((_bits(c0) == -1).all())
    if "bad" not in name:
        assert not bool(torch.isnan(d0).any())
    if "oversize" in name:
        assert info0[4] == 1 and info0[5] == 1


def test_refusals_launch_nothing():
    """Every refusal of include/sapcu_mesh.h returns SAPCU_ERR_ARG and leaves the prefilled outputs, the workspace and the guards alone."""
    p, v, f = case("torus")
    arena = Arena("guard", fill=0xFF, device=U.dev())
    bufs = _buffers(arena, p[:300], v, f)
    L = _lib()
    wsp = bufs["ws"].data_ptr()
    refusals = [dict(v=None), dict(f=None), dict(q=None), dict(dist=None), dict(nv=0), dict(nv=-3), dict(nf=0), dict(nf=-1), dict(nq=-1),
                dict(nv=1 << 31), dict(nf=(1 << 29) + 1), dict(nq=(1 << 31) - 63), dict(nbytes=bufs["nbytes"] - 1), dict(nbytes=0),
                dict(ws=None), dict(ws=ctypes.c_void_p(wsp + 4)), dict(ws=ctypes.c_void_p(wsp + 1)), dict(cell=-1.0),
                dict(cell=float("nan")), dict(cell=float("inf"))]
    for over in refusals:
        rc, info = _launch(bufs, over.pop("cell", 0.0), True, **over)
        assert rc == -1 and info == [5] * 6, over
        assert L.load().sapcu_last_error()
        arena.check()
        for name in ("dist", "face", "clo"):
            assert bool((bufs[name].contiguous().view(torch.uint8) == 0xFF).all()), (over, name)
    assert bool((bufs["ws"] == 0xFF).all())
    rc, info = _launch(bufs, 0.0, True)                        # and the same buffers are accepted as they are
    assert rc == 0 and info[0] == 1
    arena.check()
    rc, info = _launch(bufs, 0.0, True, nq=0, q=None, dist=None)    # no query: nothing is launched, nothing is written
    assert rc == 0 and info == [0] * 6


def test_every_pointer_taking_entry_point_of_the_header_runs_under_guards():
    decl = H.header_entry_points()
    assert set(decl) == set(_lib().MESH_EXPORTS)
    assert {n for n in decl if "*" in decl[n]} == {"sapcu_point_mesh_f64"}           # _buffers / _launch above
    assert {n for n in decl if n.endswith("workspace_bytes")} == {"sapcu_point_mesh_workspace_bytes"}


# ------------------------------------------------------------------------------------------------------ statistics
def _numpy_figures(d, nf, ns):
    with np.errstate(all="ignore"):
        std = np.sqrt(np.sum((d - np.mean(d)) ** 2) / np.float64(len(d) - 1))
    return {"p2f_mean": np.mean(d), "p2f_std": std, "p2f_min": d.min(), "p2f_max": d.max(), "n_pre": len(d), "n_faces": nf, "n_skipped": ns}


def _assert_figures_equal(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), "%s: %s = %r, numpy %r" % (what, k, got[k], want[k])
        if k.startswith("p2f"):
            assert isinstance(got[k], np.float64), (what, k)


@pytest.mark.parametrize("name", CASES)
def test_every_statistic_the_reference_tool_printed(name):
    from sapcu_amd import mesh
    g = golden("mesh_p2f.npz")
    p, v, f = case(name)
    m = mesh.mesh_metrics(p, v, f)
    got = np.array([m["p2f_mean"], m["p2f_std"], m["p2f_min"], m["p2f_max"]])
    printed = g[name + "/stats"]
    print("%s: %r against printed %r" % (name, got, printed))
    assert (np.abs(got - printed) <= 1e-5 * printed + 1e-12).all(), (name, got, printed)
    assert m["n_pre"] == len(p) and m["n_faces"] == int(g[name + "/n_faces"]) and m["n_skipped"] == 0
    d = mesh.point_to_mesh(p, v, f)[0].cpu().numpy()
    _assert_figures_equal(m, _numpy_figures(d, len(f), 0), name)


@pytest.mark.parametrize("n", [1, 2, 8191, 8193])
def test_mesh_metrics_equal_numpy_on_the_same_distances(n):
    from sapcu_amd import mesh
    _, v, f = case("sheet")
    rng = np.random.default_rng(n)
    p = _dev(rng.uniform(-0.3, 1.3, size=(n, 3)))
    d = mesh.point_to_mesh(p, v, f)[0].cpu().numpy()
    old = np.getbufsize()
    try:
        for bufsize in (old, 4096):
            np.setbufsize(bufsize)
            _assert_figures_equal(mesh.mesh_metrics(p, v, f), _numpy_figures(d, len(f), 0), "n=%d bufsize=%d" % (n, bufsize))
    finally:
        np.setbufsize(old)


def test_dataset_metrics_and_files(tmp_path):
    import sapcu_amd
    from sapcu_amd import mesh
    triples = [case(name) for name in ("sheet", "box", "torus")]
    pooled = mesh.mesh_dataset_metrics(triples)
    d = np.concatenate([mesh.point_to_mesh(p, v, f)[0].cpu().numpy() for p, v, f in triples])
    _assert_figures_equal(pooled, _numpy_figures(d, sum(len(f) for _, _, f in triples), 0), "pooled")
    assert pooled["n_pre"] == 1500 + 2000 + 3000
    p, v, f = case("sheet")
    pp, mp = str(tmp_path / "pred.xyz"), str(tmp_path / "mesh.off")
    np.savetxt(pp, p, fmt="%.6f")
    with open(mp, "w") as out:
        out.write("OFF\n%d %d 0\n" % (len(v), len(f)))
        out.writelines("%.17g %.17g %.17g\n" % tuple(r) for r in v)
        out.writelines("3 %d %d %d 0.5 0.5 0.5\n" % tuple(r) for r in f)
    m = sapcu_amd.evaluate_mesh_file(pp, mp, device=str(U.dev()))
    _assert_figures_equal(m, mesh.mesh_metrics(np.loadtxt(pp), v, f), "evaluate_mesh_file")
    printed = golden("mesh_p2f.npz")["sheet/stats"]
    assert abs(m["p2f_mean"] - printed[0]) <= 1e-5 * printed[0] + 1e-12 and m["n_pre"] == 1500 and m["n_faces"] == 384


# ---------------------------------------------------------------------------------------------------- Python layer
def test_python_layer_inputs_and_errors():
    from sapcu_amd import mesh
    p, v, f = case("sheet")
    want = mesh.point_to_mesh(_dev(p), _dev(v), _dev(f, np.int64))
    for faces in (f.astype(np.int64), f.astype(np.uint16), f.astype(np.int16), _dev(f, np.int32), _dev(f, np.int64)):
        got = mesh.point_to_mesh(p, _dev(v), faces)
        assert all(_same(a, b) for a, b in zip(got, want))
    wide = torch.zeros((len(p), 7), dtype=F64, device=U.dev())
    wide[:, 2:5] = _dev(p)
    got = mesh.point_to_mesh(wide[:, 2:5], v, _dev(f, np.int64).t().contiguous().t())
    assert all(_same(a, b) for a, b in zip(got, want))
    got32 = mesh.point_to_mesh(p.astype(np.float32), v, f)
    assert all(_same(a, b) for a, b in zip(got32, mesh.point_to_mesh(p.astype(np.float32).astype(np.float64), v, f)))
    info = [9]
    d, fa, c = mesh.point_to_mesh(p[:0], v, f, info=info)      # no point: nothing is launched
    assert d.shape == (0,) and fa.shape == (0,) and c.shape == (0, 3) and d.dtype == F64 and fa.dtype == I64 and info == [0] * 6
    for bad in (f + len(v), f - 1, np.where(f == 7, len(v), f)):
        with pytest.raises(ValueError):
            mesh.point_to_mesh(p, v, bad)
        with pytest.raises(ValueError):
            mesh.point_to_mesh(p, v, _dev(bad, np.int64))
    with pytest.raises(ValueError):
        mesh.point_to_mesh(p, v, f.astype(np.uint64) + np.uint64(1 << 63))
    for args in ((torch.from_numpy(p), _dev(v), f), (_dev(p), torch.from_numpy(v), f), (_dev(p), _dev(v), torch.from_numpy(f))):
        with pytest.raises(RuntimeError):
            mesh.point_to_mesh(*args)
        with pytest.raises(RuntimeError):
            mesh.mesh_metrics(*args)
    for bad in (_dev(p)[:, :2], _dev(p).reshape(-1), torch.zeros((4, 3), dtype=I64, device=U.dev())):
        with pytest.raises(ValueError):
            mesh.point_to_mesh(bad, v, f)
        with pytest.raises(ValueError):
            mesh.point_to_mesh(p, bad, f)
    for bad in (_dev(f, np.int64)[:, :2], _dev(f, np.int64)[:0], _dev(f, np.float64), _dev(f, np.int64).reshape(-1)):
        with pytest.raises(ValueError):
            mesh.point_to_mesh(p, v, bad)
    with pytest.raises(ValueError):
        mesh.mesh_metrics(_dev(p)[:0], v, f)
    for val in (float("nan"), float("inf")):
        x = _dev(p)
        x[17, 2] = val
        with pytest.raises(ValueError):
            mesh.mesh_metrics(x, v, f)
        y = _dev(v)
        y[3, 0] = val
        with pytest.raises(ValueError):
            mesh.mesh_metrics(p, y, f)
    flat = np.zeros_like(f)
    flat[:, 1] = 1                                              # every face (0, 1, 0): nothing to measure against
    with pytest.raises(ValueError):
        mesh.mesh_metrics(p, v, flat)
    d, fa, c = mesh.point_to_mesh(p, v, flat, info=info)
    assert bool(torch.isnan(d).all()) and bool((fa == -1).all()) and info[5] == len(f)
    some = f.copy()
    some[:10] = flat[:10]
    m = mesh.mesh_metrics(p, v, some)
    assert m["n_skipped"] == 10 and m["n_faces"] == len(f) and np.isfinite(m["p2f_mean"])


def test_python_entry_points_do_not_depend_on_what_an_allocation_returns(tmp_path, monkeypatch):
    """point_to_mesh, mesh_metrics / mesh_dataset_metrics and evaluate_mesh_file run clean, then under both patterns of
    tests/poison.py: bit-identical results (the workspace and the outputs never come from torch.empty)."""
    import poison
    from sapcu_amd import mesh
    p, v, f = case("torus")
    sp, sv, sf = case("sheet")
    pp, mp = str(tmp_path / "pred.xyz"), str(tmp_path / "mesh.off")
    np.savetxt(pp, sp, fmt="%.6f")
    with open(mp, "w") as out:
        out.write("OFF %d %d 0\n" % (len(sv), len(sf)))
        out.writelines("%.17g %.17g %.17g\n" % tuple(r) for r in sv)
        out.writelines("3 %d %d %d\n" % tuple(r) for r in sf)

    def run():
        a = mesh.point_to_mesh(p, v, f)
        b = mesh.point_to_mesh(sp, sv, sf, cell_size=0.07)
        return (a, b, mesh.mesh_metrics(p, v, f), mesh.mesh_dataset_metrics([(p, v, f), (sp, sv, sf)]),
                mesh.evaluate_mesh_file(pp, mp, device=str(U.dev())))

    clean = run()
    for pattern in poison.PATTERNS:
        with poison.poisoned(monkeypatch, pattern):
            got = run()
        for k in (0, 1):
            assert all(_same(x, y) for x, y in zip(got[k], clean[k])), (pattern, k)
        for k in (2, 3, 4):
            _assert_figures_equal(got[k], clean[k], "pattern %s entry %d" % (pattern, k))
