"""Geodesic disks on the device (csrc/geodesic.hip, csrc/sapcu_geodesic.h, sapcu_amd/uniformity.py): the reference tool's counts
exactly, the definition's distances (tests/geodesic_ref.py) at rtol 1e-9 — a thousand times under the fixture's margin of 1e-6
between any candidate and a radius, far above the rounding of an unfolding chain of about 50 faces plus the filters' 1e-12 —
analytic geodesics, every LDS capacity, the smallest meshes, the memory contract, the refusals and the Python layer."""
import ctypes

import numpy as np
import pytest
import torch

import geodesic_ref as G
import gpu_utils as U
import uniformity_cases as C
from guarded import Arena

pytestmark = pytest.mark.gpu

F64, I64 = torch.float64, torch.int64
RTOL = 1e-9


def _L():
    from sapcu_amd import _lib
    return _lib


def _buffers(arena, v, f, tpoint, tface, sf, sb, nr, want_dist=True, offsets=(0,) * 9):
    lib = _L().load()
    nv, nf, nq, ns = len(v), len(f), len(tpoint), len(sf)
    nbytes = int(lib.sapcu_geodesic_disks_workspace_bytes(nv, nf, nq, ns, nr))
    assert nbytes > 0
    o = offsets
    b = {"v": arena.inp(np.ascontiguousarray(v, dtype=np.float64), offset=o[0], name="vertices"),
         "f": arena.inp(np.ascontiguousarray(f, dtype=np.int32), offset=o[1], name="faces"),
         "tp": arena.inp(np.ascontiguousarray(tpoint, dtype=np.float64).reshape(-1, 3), offset=o[2], name="target_point"),
         "tf": arena.inp(np.ascontiguousarray(tface, dtype=np.int64), offset=o[3], name="target_face"),
         "sf": arena.inp(np.ascontiguousarray(sf, dtype=np.int64), offset=o[4], name="seed_face"),
         "sb": arena.inp(np.ascontiguousarray(sb, dtype=np.float64).reshape(-1, 3), offset=o[5], name="seed_bary"),
         "counts": arena.out((ns, nr), I64, offset=o[6], name="counts"),
         "dist": arena.out((ns, nq), F64, offset=o[7], name="dist") if want_dist else None,
         "ws": arena.ws(nbytes, offset=o[8], name="workspace"), "nbytes": nbytes}
    return b


def _launch(b, radii_values, queue_slots=0, **over):
    L = _L()
    lib = L.load()
    info = (ctypes.c_int64 * 8)(*([5] * 8))
    radii = np.ascontiguousarray(radii_values, dtype=np.float64)
    a = {"v": L.ptr(b["v"]), "nv": b["v"].shape[0], "f": L.ptr(b["f"]), "nf": b["f"].shape[0], "tp": L.ptr(b["tp"]), "tf": L.ptr(b["tf"]),
         "nq": b["tf"].shape[0], "sf": L.ptr(b["sf"]), "sb": L.ptr(b["sb"]), "ns": b["sf"].shape[0],
         "radii": radii.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), "nr": len(radii), "counts": L.ptr(b["counts"]),
         "dist": L.ptr(b["dist"]), "slots": queue_slots, "ws": L.ptr(b["ws"]), "nbytes": b["nbytes"]}
    a.update(over)
    rc = lib.sapcu_geodesic_disks_f64(a["v"], a["nv"], a["f"], a["nf"], a["tp"], a["tf"], a["nq"], a["sf"], a["sb"], a["ns"], a["radii"],
                                      a["nr"], a["counts"], a["dist"], a["slots"], a["ws"], a["nbytes"], info, L.current_stream())
    torch.cuda.synchronize()
    return rc, list(info)


def device_call(v, f, tpoint, tface, sf, sb, radii, queue_slots=0):
    """the C entry point on compact buffers -> (counts [ns,nr], dist [ns,nq], info) as numpy"""
    arena = Arena("compact", device=U.dev())
    b = _buffers(arena, v, f, tpoint, tface, sf, sb, len(radii))
    rc, info = _launch(b, radii, queue_slots)
    assert rc == 0, _L().load().sapcu_last_error()
    return b["counts"].cpu().numpy(), b["dist"].cpu().numpy(), info


def assert_equals_definition(v, f, tpoint, tface, sf, sb, radii, what, queue_slots=0):
    want_c, want_d = G.geodesic_disks(v, f, tpoint, tface, sf, sb, radii, return_dist=True)
    got_c, got_d, info = device_call(v, f, tpoint, tface, sf, sb, radii, queue_slots)
    C.agree(got_d, want_d, float(radii[-1]), RTOL)
    assert np.array_equal(got_c, (got_d[:, :, None] <= np.asarray(radii)[None, None, :]).sum(1)), what
    near = np.abs(want_d[:, :, None] / np.asarray(radii)[None, None, :] - 1.0) < 1e-8
    if not near.any():
        assert np.array_equal(got_c, want_c), what
    return got_c, got_d, info


# ------------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("name", C.CASES)
def test_the_device_reproduces_every_count_of_the_tool_and_the_definition_s_distances(name):
    from sapcu_amd import uniformity
    c = C.case(name)
    sf, sb = G.tool_rows_to_seeds(c["rows"])
    info = []
    counts, dist = uniformity.geodesic_disks(c["points"], c["vertices"], c["faces"], sf, sb, return_dist=True, info=info)
    assert counts.dtype == I64 and dist.dtype == F64 and counts.is_cuda
    print(name, "windows", info[0], "peak queue", info[1], "seeds off LDS", info[2], "boundary edges", info[3], "pseudo-sources", info[4])
    assert np.array_equal(counts.cpu().numpy(), c["counts"]), int((counts.cpu().numpy() != c["counts"]).sum())
    want_c, want_d = C.oracle(name)
    worst = C.agree(dist.cpu().numpy(), want_d, float(uniformity.disk_radii(c["vertices"], c["faces"])[-1]), RTOL)
    print(name, "largest relative difference to the definition", worst)
    assert info[5] == 0 and info[6] == 0 and info[0] > 0
    plain = uniformity.geodesic_disks(c["points"], c["vertices"], c["faces"], sf, sb)
    assert np.array_equal(plain.cpu().numpy(), c["counts"])


# ------------------------------------------------------------------------------------------------------ analytic
def test_flat_grid_on_the_device():
    v, f, tpoint, tface, sf, sb, ref = C.flat_case()
    _, dist, _ = device_call(v, f, tpoint, tface, sf, sb, [0.3, 0.6])
    C.agree(dist, ref, 0.6, 1e-12)


def test_plate_with_hole_and_notch_on_the_device():
    v, f, tpoint, tface, sf, sb, radii, ref = C.plate_case()
    counts, dist, _ = device_call(v, f, tpoint, tface, sf, sb, radii)
    C.agree(dist, ref, radii[-1], RTOL)
    assert np.array_equal(counts, (ref[:, :, None] <= radii[None, None, :]).sum(1))


def test_cube_unfoldings_on_the_device():
    v, f, sf, sb, tpoint, tface, ref = C.cube_case()
    _, dist, _ = device_call(v, f, tpoint, tface, sf, sb, [2.0])
    got = dist[np.arange(len(ref)), np.arange(len(ref))]
    assert np.allclose(got, ref, rtol=1e-12, atol=0), (got, ref)


# ------------------------------------------------------------------------------------------------------ capacities
@pytest.mark.parametrize("name", ["sheet", "torus", "bumpy"])
def test_every_lds_capacity_gives_the_same_counts(name):
    c = C.case(name)
    sf, sb = G.tool_rows_to_seeds(c["rows"][:16])
    radii = G.disk_radii(c["vertices"], c["faces"])
    runs = {q: device_call(c["vertices"], c["faces"], c["tpoint"], c["tface"], sf, sb, radii, q) for q in (0, 1, 2, 64)}
    base_c, base_d, base_info = runs[0]
    assert np.array_equal(base_c, c["counts"][:16])
    if name == "sheet":
        assert base_info[2] == 0, base_info                                 # under 30 windows a seed: the automatic capacities hold them
    for q in (1, 2, 64):
        got_c, got_d, info = runs[q]
        assert np.array_equal(got_c, base_c), q
        assert np.array_equal(np.isinf(got_d), np.isinf(base_d)), q
        fin = np.isfinite(base_d)
        assert np.allclose(got_d[fin], base_d[fin], rtol=RTOL, atol=0), q
        assert info[5] == 0 and info[6] == 0, (q, info)
        if q <= 2:
            assert info[2] == 16, (q, info)                                 # three vertices do not fit: every seed went on in the workspace
        assert info[3:5] == base_info[3:5]


# ------------------------------------------------------------------------------------------------------ small shapes
def _random_targets(v, f, n, rng):
    faces = rng.integers(0, len(f), n)
    w = rng.uniform(0.0, 1.0, (n, 3)) ** 2
    w /= w.sum(-1, keepdims=True)
    return np.einsum("nk,nkc->nc", w, v[f[faces]]), faces.astype(np.int64)


def _small(name):
    if name == "one triangle":
        return np.array([[0.0, 0, 0], [1, 0, 0], [0.2, 0.9, 0.3]]), np.array([[0, 1, 2]])
    if name == "two triangles":
        return np.array([[0.0, 0, 0], [1, 0, 0], [0.4, 0.8, 0], [0.6, -0.5, 0.7]]), np.array([[0, 1, 2], [1, 0, 3]])
    if name == "tetrahedron":
        return C.tetrahedron()
    return C.cube_mesh()


@pytest.mark.parametrize("name", ["one triangle", "two triangles", "tetrahedron", "box"])
@pytest.mark.parametrize("slots", [0, 1])
def test_the_smallest_meshes(name, slots):
    v, f = _small(name)
    rng = np.random.default_rng(len(name))
    tpoint, tface = _random_targets(v, f, 150, rng)
    sf, sb = C.seeds_in_faces(v, f, rng.integers(0, len(f), 7), rng)
    diam = float(np.linalg.norm(v.max(0) - v.min(0)))
    radii = np.array([0.2, 0.6, 3.0]) * diam                                # the last one covers the whole mesh
    counts, dist, info = assert_equals_definition(v, f, tpoint, tface, sf, sb, radii, name, slots)
    assert np.isfinite(dist).all() and (counts[:, -1] == 150).all()
    own = tface[None, :] == sf[:, None]                                     # a target in the seed's face: the straight distance
    straight = np.sqrt(((C.seed_points(v, f, sf, sb)[:, None, :] - tpoint[None, :, :]) ** 2).sum(-1))
    assert own.any() and np.allclose(dist[own], straight[own], rtol=1e-14, atol=0)
    if name == "one triangle":
        assert info[0] == 0 or info[3] == 3                                 # nothing but boundary


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 530])
def test_seed_counts_at_the_wave_and_the_grid_edges(ns):
    """530 seeds: more than the 512 work groups of a launch, so some groups take a second seed after cleaning up their first."""
    c = C.case("sheet")
    rng = np.random.default_rng(ns)
    sf, sb = C.seeds_in_faces(c["vertices"], c["faces"], rng.integers(0, len(c["faces"]), ns), rng)
    radii = G.disk_radii(c["vertices"], c["faces"])
    counts, _, info = assert_equals_definition(c["vertices"], c["faces"], c["tpoint"], c["tface"], sf, sb, radii, ns)
    assert info[7] == min(ns, 512) and counts.shape == (ns, 7)


def test_a_disk_that_reaches_no_target_and_calls_without_targets_or_seeds():
    v, f = C.plate_mesh()
    far, _ = C.locate(np.array([[0.02, 0.03, 0.0], [0.05, 0.01, 0.0]]), v, f)
    tpoint, tface = C.locate(far, v, f)
    sf, sb = np.array([len(f) - 1, 0]), np.array([[0.3, 0.3, 0.4], [0.2, 0.5, 0.3]])
    radii = np.array([0.01, 0.1])
    counts, dist, _ = device_call(v, f, tpoint, tface, sf, sb, radii)
    assert (counts[0] == 0).all() and np.isinf(dist[0]).all()               # the last face is far from the corner (0, 0)
    assert counts[1, 1] == 2 and np.isfinite(dist[1]).all()
    arena = Arena("guard", device=U.dev())
    b = _buffers(arena, v, f, tpoint, tface, sf, sb, 2)
    rc, info = _launch(b, radii, nq=0, tp=None, tf=None, dist=None)         # no target: the counts are zeroed, nothing else
    assert rc == 0 and info == [0] * 8 and bool((b["counts"] == 0).all())
    assert bool((b["ws"] == 0xFF).all()) and bool((b["dist"].contiguous().view(torch.uint8) == 0xFF).all())
    arena.refill_outputs()
    rc, info = _launch(b, radii, ns=0, sf=None, sb=None, counts=None, dist=None)    # no seed: nothing is written
    assert rc == 0 and info == [0] * 8
    assert bool((b["counts"].contiguous().view(torch.uint8) == 0xFF).all()) and bool((b["ws"] == 0xFF).all())
    arena.check()


# ------------------------------------------------------------------------------------------------------ memory contract
@pytest.mark.parametrize("name,slots,want_dist", [("sheet", 0, True), ("sheet", 2, True), ("box", 0, False), ("bumpy", 64, True)])
def test_memory_contract_under_guard_bands(name, slots, want_dist):
    """0xFF bands and workspace with 0xFF-prefilled outputs, 0x00 bands and workspace, the dirty workspace again: guards intact,
    outputs written in full, counts identical, distances within rounding of each other and of the compact call."""
    c = C.case(name)
    sf, sb = G.tool_rows_to_seeds(c["rows"][:9])
    radii = G.disk_radii(c["vertices"], c["faces"])
    results = []
    for fill in (0xFF, 0x00):
        arena = Arena("guard", fill=fill, device=U.dev())
        b = _buffers(arena, c["vertices"], c["faces"], c["tpoint"], c["tface"], sf, sb, 7, want_dist, offsets=(8, 4, 24, 8, 16, 8, 8, 24, 8))
        for again in range(2 if fill == 0x00 else 1):
            arena.refill_outputs()
            rc, info = _launch(b, radii, slots)
            assert rc == 0, _L().load().sapcu_last_error()
            arena.check()
            results.append((b["counts"].cpu().numpy(), b["dist"].cpu().numpy() if want_dist else None, info))
    c0, d0, info0 = results[0]
    assert np.array_equal(c0, c["counts"][:9])
    for cc, dd, info in results[1:]:
        assert np.array_equal(cc, c0) and info[2:] == info0[2:]
        if want_dist:
            assert not np.isnan(dd).any() and np.array_equal(np.isinf(dd), np.isinf(d0))
            assert np.allclose(dd[np.isfinite(d0)], d0[np.isfinite(d0)], rtol=RTOL, atol=0)
    if want_dist:
        C.agree(d0, C.oracle(name)[1][:9], float(radii[-1]), RTOL)


@pytest.mark.parametrize("pattern", ["A", "B"])
def test_a_dirty_workspace_changes_nothing(pattern):
    import poison
    c = C.case("torus")
    sf, sb = G.tool_rows_to_seeds(c["rows"][:12])
    radii = G.disk_radii(c["vertices"], c["faces"])
    arena = Arena("compact", device=U.dev())
    b = _buffers(arena, c["vertices"], c["faces"], c["tpoint"], c["tface"], sf, sb, 7)
    rc, _ = _launch(b, radii, 2)
    assert rc == 0
    clean_c, clean_d = b["counts"].cpu().numpy(), b["dist"].cpu().numpy()
    poison.fill(b["ws"], pattern)
    arena.refill_outputs()
    rc, _ = _launch(b, radii, 2)
    assert rc == 0
    assert np.array_equal(b["counts"].cpu().numpy(), clean_c) and np.array_equal(clean_c, c["counts"][:12])
    got = b["dist"].cpu().numpy()
    assert np.array_equal(np.isinf(got), np.isinf(clean_d))
    assert np.allclose(got[np.isfinite(got)], clean_d[np.isfinite(got)], rtol=RTOL, atol=0)


def test_refusals_launch_nothing():
    """Every refusal of csrc/sapcu_geodesic.h returns SAPCU_ERR_ARG and leaves the prefilled outputs, the workspace and the guards alone."""
    c = C.case("sheet")
    sf, sb = G.tool_rows_to_seeds(c["rows"][:5])
    radii = G.disk_radii(c["vertices"], c["faces"])
    arena = Arena("guard", fill=0xFF, device=U.dev())
    b = _buffers(arena, c["vertices"], c["faces"], c["tpoint"], c["tface"], sf, sb, 7)
    dev = U.dev()
    wsp = b["ws"].data_ptr()
    rad = lambda r: np.ascontiguousarray(r, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    keep = []                                                               # bad seed arrays stay alive while they are in use

    def seeds(face=None, bary=None):
        over = {}
        if face is not None:
            keep.append(torch.as_tensor(np.array(face, dtype=np.int64)).to(dev))
            over["sf"] = _L().ptr(keep[-1])
        if bary is not None:
            keep.append(torch.as_tensor(np.array(bary, dtype=np.float64)).to(dev))
            over["sb"] = _L().ptr(keep[-1])
        return over

    ok_f, ok_b = list(sf), [list(x) for x in sb]
    bad_bary = lambda row: ok_b[:2] + [row] + ok_b[3:]
    refusals = [dict(v=None), dict(f=None), dict(tp=None), dict(tf=None), dict(sf=None), dict(sb=None), dict(counts=None), dict(radii=None),
                dict(nv=0), dict(nv=-1), dict(nv=(1 << 24) + 1), dict(nf=0), dict(nf=-2), dict(nf=(1 << 24) + 1), dict(nq=-1),
                dict(nq=(1 << 30) + 1), dict(ns=-1), dict(ns=(1 << 24) + 1), dict(nr=0), dict(nr=17), dict(slots=-1),
                dict(radii=rad([0.1, 0.05, 0.2, 0.3, 0.4, 0.5, 0.6])), dict(radii=rad([0.1, 0.2, 0.3, float("nan"), 0.4, 0.5, 0.6])),
                dict(radii=rad([0.0, 0.2, 0.3, 0.35, 0.4, 0.5, 0.6])), dict(radii=rad([0.1, 0.2, 0.3, 0.35, 0.4, 0.5, float("inf")])),
                dict(nbytes=b["nbytes"] - 1), dict(nbytes=0), dict(ws=None), dict(ws=ctypes.c_void_p(wsp + 4)), dict(ws=ctypes.c_void_p(wsp + 1)),
                seeds(face=ok_f[:4] + [len(c["faces"])]), seeds(face=[-1] + ok_f[1:]),
                seeds(bary=bad_bary([0.5, 0.5, 0.0])), seeds(bary=bad_bary([1.0, 0.0, 0.0])), seeds(bary=bad_bary([0.7, 0.5, -0.2])),
                seeds(bary=bad_bary([0.3, 0.3, 0.3])), seeds(bary=bad_bary([float("nan"), 0.3, 0.3])),
                seeds(bary=bad_bary([float("inf"), 0.3, 0.3])), seeds(bary=bad_bary([0.4, 0.4, 0.2 + 1e-8]))]
    for over in refusals:
        rc, info = _launch(b, radii, **dict(over))
        assert rc == -1 and info == [5] * 8, (over, rc, info)
        assert _L().load().sapcu_last_error()
        arena.check()
        for name in ("counts", "dist"):
            assert bool((b[name].contiguous().view(torch.uint8) == 0xFF).all()), (over, name)
        assert bool((b["ws"] == 0xFF).all()), over
    rc, info = _launch(b, radii)                                            # and the same buffers are accepted as they are
    assert rc == 0 and np.array_equal(b["counts"].cpu().numpy(), c["counts"][:5])
    arena.check()
    lib = _L().load()
    for sizes in [(0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, -1, 1, 1), (1, 1, 1, -1, 1), (1, 1, 1, 1, 0), (1, 1, 1, 1, 17), ((1 << 24) + 1, 1, 1, 1, 1)]:
        assert lib.sapcu_geodesic_disks_workspace_bytes(*sizes) == -1, sizes


def test_the_two_bounded_ends_of_the_loop_are_counted_and_returned():
    """A window cap and a workspace queue far below the header's, through the test hook: the seeds that reach either are counted in
    info_host, the call returns SAPCU_ERR_LIMIT (-6), nothing is retried and the guards hold; the seeds that stay below both have
    the counts of the unlimited call."""
    c = C.case("bumpy")
    sf, sb = G.tool_rows_to_seeds(c["rows"][:8])
    radii = G.disk_radii(c["vertices"], c["faces"])
    L = _L()
    lib = L.load()
    for cap, limit, which in ((40, len(c["faces"]) + 4096, 5), (96 * len(c["faces"]) + 4096, 4, 6)):
        arena = Arena("guard", fill=0xFF, device=U.dev())
        b = _buffers(arena, c["vertices"], c["faces"], c["tpoint"], c["tface"], sf, sb, 7)
        info = (ctypes.c_int64 * 8)()
        rr = np.ascontiguousarray(radii, dtype=np.float64)
        rc = lib.sapcu_internal_geodesic_disks_limited(L.ptr(b["v"]), len(c["vertices"]), L.ptr(b["f"]), len(c["faces"]), L.ptr(b["tp"]),
                                                       L.ptr(b["tf"]), len(c["tpoint"]), L.ptr(b["sf"]), L.ptr(b["sb"]), 8,
                                                       rr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 7, L.ptr(b["counts"]),
                                                       L.ptr(b["dist"]), 0, cap, limit, L.ptr(b["ws"]), b["nbytes"], info, L.current_stream())
        torch.cuda.synchronize()
        info = list(info)
        assert rc == -6 and lib.sapcu_last_error(), (rc, info)
        assert info[which] == 8 and info[11 - which] == 0, info                 # every seed of this mesh needs more than 40 windows, or 4 slots
        if which == 5:
            assert info[0] <= 8 * cap
        arena.check()
    arena = Arena("guard", fill=0xFF, device=U.dev())                           # limits that hold: the public call's result
    b = _buffers(arena, c["vertices"], c["faces"], c["tpoint"], c["tface"], sf, sb, 7)
    info = (ctypes.c_int64 * 8)()
    rc = lib.sapcu_internal_geodesic_disks_limited(L.ptr(b["v"]), len(c["vertices"]), L.ptr(b["f"]), len(c["faces"]), L.ptr(b["tp"]),
                                                   L.ptr(b["tf"]), len(c["tpoint"]), L.ptr(b["sf"]), L.ptr(b["sb"]), 8,
                                                   rr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 7, L.ptr(b["counts"]), L.ptr(b["dist"]),
                                                   0, 2000, 600, L.ptr(b["ws"]), b["nbytes"], info, L.current_stream())
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(b["counts"].cpu().numpy(), c["counts"][:8])
    arena.check()


def test_meshes_that_are_no_oriented_manifold_are_refused():
    from sapcu_amd import uniformity
    v, f = C.cube_mesh()
    pts = np.array([[0.5, 0.5, 0.0], [1.0, 0.5, 0.5]])
    sf, sb = np.array([0]), np.array([[0.3, 0.3, 0.4]])
    bad = {"a third face on an edge": np.concatenate([f, [[0, 3, 2]]]),
           "two faces of opposite orientation": np.concatenate([f[:1], [f[1][[0, 2, 1]]], f[2:]]),
           "a zero-area face": np.concatenate([f, [[0, 0, 1]]]),
           "a collinear face": None}
    for what, faces in bad.items():
        vv = v
        if faces is None:
            vv = np.concatenate([v, [[2.0, 0, 0], [3.0, 0, 0], [4.0, 0, 0]]])
            faces = np.concatenate([f, [[8, 9, 10]]])
        with pytest.raises(ValueError):
            uniformity.geodesic_disks(pts, vv, faces, sf, sb, radii=[0.5])
        tpoint, tface = C.locate(pts, v, f)
        arena = Arena("compact", device=U.dev())
        b = _buffers(arena, vv, faces, tpoint, tface, sf, sb, 1)
        rc, _ = _launch(b, [0.5])
        assert rc == -5, (what, rc)                                         # SAPCU_ERR_MESH, a status of its own
        assert bool((b["counts"].contiguous().view(torch.uint8) == 0xFF).all()), what    # the propagation was not launched
    with pytest.raises(ValueError):                                         # a seed on an edge
        uniformity.geodesic_disks(pts, v, f, sf, np.array([[0.5, 0.5, 0.0]]), radii=[0.5])
    good = uniformity.geodesic_disks(pts, v, f, sf, sb, radii=[0.5])
    assert good.shape == (1, 1)


# ------------------------------------------------------------------------------------------------------ Python layer
def _write_case(tmp_path, c, rows):
    pp, mp, sp = str(tmp_path / "pred.xyz"), str(tmp_path / "mesh.off"), str(tmp_path / "seeds.txt")
    np.savetxt(pp, c["points"], fmt="%.17g")
    with open(mp, "w") as out:
        out.write("OFF %d %d 0\n" % (len(c["vertices"]), len(c["faces"])))
        out.writelines("%.17g %.17g %.17g\n" % tuple(r) for r in c["vertices"])
        out.writelines("3 %d %d %d\n" % tuple(r) for r in c["faces"])
    with open(sp, "w") as out:
        out.writelines("%d %.17g %.17g %.17g\n" % tuple(r) for r in rows)
    return pp, mp, sp


def test_the_python_layer_s_figures_are_numpy_s_on_the_same_counts(tmp_path):
    from sapcu_amd import uniformity
    c = C.case("sheet")
    seeds = G.tool_rows_to_seeds(c["rows"])
    m = uniformity.uniformity_metrics(c["points"], c["vertices"], c["faces"], seeds=seeds)
    fr = uniformity.TOOL_FRACTIONS.astype(np.float64)
    density = c["counts"] / (np.float64(len(c["points"])) * fr)[None, :]
    assert np.array_equal(m["counts"], c["counts"]) and np.array_equal(m["density"], density)
    assert np.array_equal(m["nuc"], np.std(density, 0)) and np.array_equal(m["mean_density"], np.mean(density, 0))
    assert m["n_pre"] == len(c["points"]) and m["n_seeds"] == 48
    assert np.allclose(m["density"], c["density"], rtol=5e-6, atol=1e-12) and np.allclose(m["radii"], c["radii"], rtol=5e-6)
    pp, mp, sp = _write_case(tmp_path, c, c["rows"])
    e = uniformity.evaluate_uniformity_file(pp, mp, sp, device=str(U.dev()))
    assert np.array_equal(e["counts"], c["counts"]) and np.array_equal(e["nuc"], m["nuc"])
    drawn = uniformity.uniformity_metrics(torch.as_tensor(c["points"]).to(U.dev()), c["vertices"], c["faces"], n_seeds=70, generator=4)
    sf, sb = uniformity.uniformity_seeds(c["vertices"], c["faces"], 70, generator=4)
    assert np.array_equal(drawn["counts"], G.geodesic_disks(c["vertices"], c["faces"], c["tpoint"], c["tface"], sf, sb, m["radii"]))
    pooled = uniformity.dataset_uniformity([m, drawn])
    both = np.concatenate([m["density"], drawn["density"]])
    assert np.array_equal(pooled["nuc"], np.std(both, 0)) and pooled["n_seeds"] == 118
    with pytest.raises(RuntimeError):
        uniformity.geodesic_disks(torch.as_tensor(c["points"]), c["vertices"], c["faces"], *seeds)       # a CPU tensor
    with pytest.raises(ValueError):
        uniformity.geodesic_disks(c["points"], c["vertices"], c["faces"], seeds[0], seeds[1][:, :2])
    with pytest.raises(ValueError):
        uniformity.geodesic_disks(c["points"], c["vertices"], c["faces"], *seeds, fractions=[0.2, 0.1])
    none = uniformity.geodesic_disks(c["points"][:0], c["vertices"], c["faces"], *seeds)
    assert none.shape == (48, 7) and int(none.sum()) == 0


def test_python_entry_points_do_not_depend_on_what_an_allocation_returns(tmp_path, monkeypatch):
    import poison
    from sapcu_amd import uniformity
    c = C.case("sheet")
    seeds = G.tool_rows_to_seeds(c["rows"])
    pp, mp, sp = _write_case(tmp_path, c, c["rows"])

    def run():
        a = uniformity.geodesic_disks(c["points"], c["vertices"], c["faces"], *seeds, return_dist=True)
        return (a[0].cpu().numpy(), a[1].cpu().numpy(), uniformity.uniformity_metrics(c["points"], c["vertices"], c["faces"], seeds=seeds),
                uniformity.evaluate_uniformity_file(pp, mp, sp, device=str(U.dev())))

    clean = run()
    for pattern in poison.PATTERNS:
        with poison.poisoned(monkeypatch, pattern):
            got = run()
        assert np.array_equal(got[0], clean[0]) and np.array_equal(np.isinf(got[1]), np.isinf(clean[1])), pattern
        fin = np.isfinite(clean[1])
        assert np.allclose(got[1][fin], clean[1][fin], rtol=RTOL, atol=0), pattern
        for k in (2, 3):
            for key in ("counts", "density", "nuc", "mean_density", "radii"):
                assert np.array_equal(got[k][key], clean[k][key]), (pattern, k, key)
