"""Poisson-disk selection on the device (-m gpu; csrc/sapcu_poisson.h, csrc/poisson.hip, sapcu_amd/poisson.py,
data.PoissonPU1KPatches).

Every output of ``sapcu_poisson_select_f32`` and ``sapcu_poisson_subsample_f32`` must equal tests/poisson_ref.py — brute force, no
grid — with ``==``: there is no tolerance anywhere in this file.  Sizes are 1, 2, the wavefront and the 256 boundaries, a size that
is no multiple of anything, the resident path's last sizes and the grid path's first, and 20011; the small ones run again through
the grid path's test hook (one round per read-back).  Both paths run synchronous rounds, so ``rounds`` equals
``poisson_ref.select_rounds``'s count, which is inside the bound the contract states (1 <= rounds <= that count).  Every call is
made twice and has to answer the same."""
import ctypes
import math

import numpy as np
import pytest
import torch

import data_ref as DR
import gpu_utils as U
import poisson_cases as K
import surface_ref as SR
from guarded import Arena

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
f32 = np.float32
RM = K.RESIDENT_MAX
SMALL = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
SIZES = SMALL + (RM - 1, RM, RM + 1, 20011)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(U.dev())


def _select(P, r, path=None, **kw):
    """poisson_select twice -> (keep, count, rounds) as numpy, the two runs equal."""
    from sapcu_amd import poisson
    P = _dev(P)
    r = _dev(np.asarray(r, f32)) if np.ndim(r) else float(r)
    runs = [[t.cpu().numpy() for t in poisson.poisson_select(P, r, path=path, **kw)] for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    return runs[0]


def _check_select(clouds, radii, path):
    P = np.stack(clouds)
    keep, count, rounds = _select(P, np.asarray(radii, f32), path)
    assert keep.dtype == bool and keep.shape == P.shape[:2] and count.dtype == np.int32 and rounds.dtype == np.int32
    for e, (cloud, r) in enumerate(zip(clouds, radii)):
        want, n = K.ref_select(cloud, r)
        assert np.array_equal(keep[e], want), (e, int((keep[e] != want).sum()))
        assert count[e] == n
        assert 1 <= rounds[e] <= K.ref_rounds(cloud, r)[2]
        assert rounds[e] == K.ref_rounds(cloud, r)[2]                 # synchronous rounds on both paths: the count itself
    return keep, count, rounds


def test_the_constants_are_the_header_s():
    from sapcu_amd import poisson
    assert poisson.PD_RESIDENT_MAX == RM >= 8192


# -------------------------------------------------------------------------------------------------------------- select
@pytest.mark.parametrize("C,path", [(C, None) for C in SIZES] + [(C, "grid") for C in SMALL])
def test_select_at_every_boundary_size(C, path):
    """b = 3: a sphere, a plane and the sphere again, each entry at its own radius; the repeated cloud gives the same row."""
    a, p = K.sphere(C), K.plane(C)
    ra, rp = K.typical_radius(C), K.typical_radius(C, area=1.0)
    keep, count, rounds = _check_select([a, p, a], [ra, rp, ra], path)
    assert np.array_equal(keep[0], keep[2]) and count[0] == count[2] and rounds[0] == rounds[2]


@pytest.mark.parametrize("C,path", [(C, None) for C in SMALL + (RM + 1,)] + [(C, "grid") for C in SMALL])
def test_radius_zero_keeps_everything(C, path):
    keep, count, rounds = _select(np.stack([K.sphere(C), K.equal(C)]), 0.0, path)
    assert keep.all() and (count == C).all() and (rounds == 1).all()
    assert K.ref_select(K.equal(C), 0.0)[1] == C and K.ref_rounds(K.equal(C), 0.0)[2] == 1


SPECIAL = [("equal-1", K.equal(1), 0.1), ("equal-2", K.equal(2), 0.1), ("equal-64", K.equal(64), 0.1), ("equal-257", K.equal(257), 0.1),
           ("equal-1000", K.equal(1000), 1e-20), ("one-cell-256", K.plane(256), 2.0), ("one-cell-1000", K.sphere(1000), 2.5),
           ("lattice-tie", K.lattice(), 0.25), ("lattice-above", K.lattice(), np.nextafter(f32(0.25), f32(1))),
           ("offset-1000", K.offset(1000), K.typical_radius(1000)), ("offset-257-wide", K.offset(257), 0.9), ("line-300", K.line(), 0.015),
           ("plane-1000-dense", K.plane(1000), 0.2)]


@pytest.mark.parametrize("path", [None, "grid"])
@pytest.mark.parametrize("name,P,r", SPECIAL, ids=[c[0] for c in SPECIAL])
def test_special_inputs_without_a_batch_dimension(name, P, r, path):
    keep, count, rounds = _select(P, r, path)
    want, n, want_rounds = K.ref_rounds(P, r)
    assert keep.shape == (len(P),) and count.shape == () and np.array_equal(keep, want) and np.array_equal(want, K.ref_select(P, r)[0])
    assert count == n and 1 <= rounds <= want_rounds and rounds == want_rounds
    if name.startswith("one-cell"):
        assert n == 1
    if name == "lattice-tie":
        assert n == 64
    if name == "line-300":
        assert n == 150 and want_rounds == 300


@pytest.mark.parametrize("path", [None, "grid"])
def test_sixty_four_entries(path):
    clouds = [K.sphere(257, s % 8) for s in range(64)]
    radii = [f32(0.1 + 0.05 * (s % 8)) for s in range(64)]
    keep, count, rounds = _check_select(clouds, radii, path)
    for s in range(8, 64):
        assert np.array_equal(keep[s], keep[s % 8]) and count[s] == count[s % 8] and rounds[s] == rounds[s % 8]


# ----------------------------------------------------------------------------------------------------------- subsample
@pytest.mark.parametrize("steps", [0, 1, 20])
@pytest.mark.parametrize("C,n", [(1, 1), (64, 1), (64, 64), (2048, 256), (RM, 1024), (RM + 8, 1000)])
def test_subsample_equals_the_bisection(C, n, steps):
    from sapcu_amd import poisson
    clouds = [K.sphere(C, 3), K.plane(C, 4)]
    P = _dev(np.stack(clouds))
    runs = [[t.cpu().numpy() for t in poisson.poisson_subsample(P, n, steps)] for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    idx, radius, count, rounds = runs[0]
    assert idx.dtype == np.int32 and idx.shape == (2, n) and radius.dtype == f32
    for e, cloud in enumerate(clouds):
        want_idx, want_r, want_count, _ = K.ref_subsample(cloud, n, steps)
        assert radius[e].tobytes() == want_r.tobytes(), (radius[e], want_r)
        assert count[e] == want_count >= n and np.array_equal(idx[e], want_idx)
        assert steps + 1 <= rounds[e] <= (steps + 1) * C
    one = [t.cpu().numpy() for t in poisson.poisson_subsample(P[1], n, steps)]
    assert one[0].shape == (n,) and all(np.array_equal(a, b[1]) for a, b in zip(one, runs[0]))


# -------------------------------------------------------------------------------------------------------------- meshes
def _meshes():
    from test_gpu_surface import mesh_and_tables
    return [mesh_and_tables("icosphere"), mesh_and_tables("polygons")]


def _ref_clouds(meshes, mesh_idx, u, r1, r2):
    return SR.batch([m for m, _ in meshes], [t for _, t in meshes], mesh_idx, u.cpu().numpy(), r1.cpu().numpy(), r2.cpu().numpy())


def test_disk_sample_of_meshes_across_the_split_of_the_draws():
    from sapcu_amd import poisson, surface
    meshes = _meshes()
    tables = surface.build_surface_tables([m for m, _ in meshes], device=U.dev())
    b, C, n = 2, 2 * surface.MAX_N, 700
    assert C <= RM
    gen = torch.Generator(device=U.dev()).manual_seed(21)
    u = torch.rand((b, C), generator=gen, device=U.dev(), dtype=F64)
    r1, r2 = torch.rand((b, C), generator=gen, device=U.dev()), torch.rand((b, C), generator=gen, device=U.dev())
    mesh_idx = np.array([1, 0], np.int64)
    points, normals, faces, radius, count, idx = [t.cpu().numpy() for t in
                                                  poisson.poisson_disk_sample(tables, _dev(mesh_idx), n, u, r1, r2, steps=16)]
    rp, rn, rf = _ref_clouds(meshes, mesh_idx, u, r1, r2)
    for e in range(b):
        want_idx, want_r, want_count, _ = K.ref_subsample(rp[e], n, 16)
        assert np.array_equal(idx[e], want_idx) and radius[e].tobytes() == want_r.tobytes() and count[e] == want_count
        assert np.array_equal(points[e], rp[e][want_idx]) and np.array_equal(normals[e], rn[e][want_idx])
        assert np.array_equal(faces[e], rf[e][want_idx])


def _loader(**kw):
    from sapcu_amd import data
    meshes = [m for m, _ in _meshes()] * 5
    return data.PoissonPU1KPatches(meshes, **dict(dict(num_input=64, num_dense=160, oversample=4, k_neighbors=24, split="all", batch_size=2,
                                                       seed=5, augment=True, device=U.dev()), **kw))


def test_the_loader_s_batch_is_data_ref_on_the_clouds_poisson_ref_selects():
    loader = _loader()
    batch = next(iter(loader))
    d = loader.last_draws
    mesh_idx = batch["index"].cpu().numpy()
    meshes = (_meshes() * 5)
    clouds = {}
    for tag, n in (("input", 64), ("dense", 160)):
        assert d["u_" + tag].shape == (2, 4 * n)
        pts = _ref_clouds(meshes, mesh_idx, d["u_" + tag], d["r1_" + tag], d["r2_" + tag])[0]
        sel = [K.ref_subsample(p, n, 20) for p in pts]
        assert np.array_equal(d["idx_" + tag].cpu().numpy(), np.stack([s[0] for s in sel]))
        assert d["radius_" + tag].cpu().numpy().tobytes() == np.stack([s[1] for s in sel]).tobytes()
        assert np.array_equal(d["count_" + tag].cpu().numpy(), [s[2] for s in sel])
        clouds[tag] = np.stack([p[s[0]] for p, s in zip(pts, sel)])
    want = DR.batch(clouds["input"], np.arange(2), 24, dense=clouds["dense"], rot=d["rotation"].cpu().numpy(), scale=d["scale"].cpu().numpy(),
                    jitter=d["jitter"].cpu().numpy())
    assert sorted(batch) == ["cloud", "index", "input", "len", "points"]
    for key, ref in (("input", "patches"), ("len", "len"), ("cloud", "cloud"), ("points", "dense")):
        assert np.array_equal(batch[key].cpu().numpy(), want[ref]), key
    assert batch["input"].shape == (2, 64, 24, 3) and batch["points"].shape == (2, 160, 3)


def test_the_loader_is_deterministic_per_seed_epoch_and_batch():
    first = [{k: v.clone() for k, v in b.items()} for b in _loader()]
    again = list(_loader())
    assert len(first) == 5
    for a, b in zip(first, again):
        assert all(torch.equal(a[k], b[k]) for k in a)
    other = next(iter(_loader().set_epoch(1)))
    assert not torch.equal(other["cloud"], first[0]["cloud"])
    assert not torch.equal(first[0]["cloud"], first[1]["cloud"])


def test_an_fd_training_step_on_a_poisson_batch():
    from test_gpu_data import _fd_trainer, _params
    batch = next(iter(_loader()))
    model, tr = _fd_trainer()
    before = _params(model)
    loss, _ = tr.train_step(batch)
    assert loss is not None and math.isfinite(float(loss)), loss
    assert any(not torch.equal(a, b) for a, b in zip(before, _params(model)))


# ------------------------------------------------------------------------------------------------------ memory contract
def _raw_select(arena, P, r, name="sapcu_poisson_select_f32"):
    from sapcu_amd import _lib
    b, C = P.shape[:2]
    pts, rad = arena.inp(P, name="points"), arena.inp(np.asarray(r, f32), name="radius")
    keep, count, rounds = arena.out((b, C), torch.uint8, name="keep"), arena.out((b,), I32, name="count"), arena.out((b,), I32, name="rounds")
    nbytes = int(_lib.load().sapcu_poisson_workspace_bytes(b, C))
    ws = arena.ws(nbytes)
    _lib.call(name, U.dev(), pts, b, C, rad, keep, count, rounds, ws, nbytes)
    torch.cuda.synchronize()
    arena.check()
    return [t.cpu().numpy() for t in (keep, count, rounds)]


def _raw_subsample(arena, P, n, steps):
    from sapcu_amd import _lib
    b, C = P.shape[:2]
    pts = arena.inp(P, name="points")
    outs = (arena.out((b, n), I32, name="idx"), arena.out((b,), F32, name="radius"), arena.out((b,), I32, name="count"),
            arena.out((b,), I32, name="rounds"))
    nbytes = int(_lib.load().sapcu_poisson_workspace_bytes(b, C))
    ws = arena.ws(nbytes)
    _lib.call("sapcu_poisson_subsample_f32", U.dev(), pts, b, C, n, steps, *outs, ws, nbytes)
    torch.cuda.synchronize()
    arena.check()
    return [t.cpu().numpy() for t in outs]


@pytest.mark.parametrize("C,name", [(257, "sapcu_poisson_select_f32"), (257, "sapcu_internal_poisson_select_grid"),
                                    (RM + 1, "sapcu_poisson_select_f32")])
def test_select_under_guard_bands_with_a_dirty_workspace(C, name):
    P = np.stack([K.sphere(C), K.plane(C), K.offset(C)])
    r = np.array([K.typical_radius(C), 0.0, K.typical_radius(C)], f32)
    runs = [_raw_select(Arena("guard", fill=fill, device=U.dev()), P, r, name) for fill in (0xFF, 0x00)]
    runs.append(_raw_select(Arena("compact", device=U.dev()), P, r, name))
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], other))
    for e in range(3):
        assert np.array_equal(runs[0][0][e].astype(bool), K.ref_select(P[e], r[e])[0]) and set(np.unique(runs[0][0])) <= {0, 1}


@pytest.mark.parametrize("C,n,steps", [(2048, 256, 20), (300, 100, 5), (RM + 8, 100, 3)])
def test_subsample_under_guard_bands_with_a_dirty_workspace(C, n, steps):
    P = np.stack([K.sphere(C, 3), K.line(C) if C == 300 else K.plane(C, 4)])
    runs = [_raw_subsample(Arena("guard", fill=fill, device=U.dev()), P, n, steps) for fill in (0xFF, 0x00)]
    runs.append(_raw_subsample(Arena("compact", device=U.dev()), P, n, steps))
    for other in runs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], other))
    for e in range(2):
        want = K.ref_subsample(P[e], n, steps)
        assert np.array_equal(runs[0][0][e], want[0]) and runs[0][1][e].tobytes() == want[1].tobytes() and runs[0][2][e] == want[2]


def test_the_resident_path_replays_as_a_graph():
    from sapcu_amd import poisson
    P = _dev(np.stack([K.sphere(2048, 3), K.plane(2048, 4), K.offset(2048)]))
    radii = _dev(np.array([0.1, 0.05, 0.2], f32))

    def run():
        return poisson.poisson_select(P, radii, validate=False) + poisson.poisson_subsample(P, 256, 20, validate=False)

    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=U.dev())
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = run()
    for _ in range(2):
        for v in out:
            v.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
    assert int(eager[1].min()) >= 1 and (eager[5] >= 256).all()


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("path", [None, "grid"])
def test_an_entry_that_is_not_finite_keeps_nothing_without_validation(path):
    from sapcu_amd import poisson
    P = np.stack([K.sphere(300), K.sphere(300, 1), K.sphere(300, 2)])
    P[1, 17, 2] = np.nan
    P[2, 299, 0] = np.inf
    with pytest.raises(ValueError):
        poisson.poisson_select(_dev(P), 0.2, path=path)
    keep, count, rounds = _select(P, 0.2, path, validate=False)
    assert np.array_equal(keep[0], K.ref_select(P[0], 0.2)[0]) and count[0] == keep[0].sum()
    assert not keep[1:].any() and (count[1:] == 0).all() and (rounds[1:] == 0).all()
    if path is None:
        with pytest.raises(ValueError):
            poisson.poisson_subsample(_dev(P), 10)
        idx, radius, count, rounds = [t.cpu().numpy() for t in poisson.poisson_subsample(_dev(P), 10, validate=False)]
        assert np.array_equal(idx[0], K.ref_subsample(P[0], 10, 20)[0]) and (idx[1:] == -1).all() and (count[1:] == 0).all()


def test_the_grid_path_s_subsample_keeps_nothing_of_an_entry_that_is_not_finite():
    from sapcu_amd import poisson
    P = np.stack([K.sphere(RM + 8, 3), K.sphere(RM + 8, 1)])
    P[1, 5, 1] = -np.inf
    idx, radius, count, rounds = [t.cpu().numpy() for t in poisson.poisson_subsample(_dev(P), 1000, 1, validate=False)]
    assert np.array_equal(idx[0], K.ref_subsample(P[0], 1000, 1)[0]) and (idx[1] == -1).all() and count[1] == 0 and radius[1] == 0


def test_refusals_in_python():
    from sapcu_amd import poisson, surface
    P = _dev(K.sphere(64))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            poisson.poisson_select(P, bad)
        with pytest.raises(ValueError):
            poisson.poisson_select(P[None], _dev(np.array([bad], f32)))
    with pytest.raises(ValueError):
        poisson.poisson_select(P[None], _dev(np.array([0.1, 0.1], f32)))
    for shape in ((64,), (64, 2), (2, 2, 64, 3), (0, 3)):
        with pytest.raises(ValueError):
            poisson.poisson_select(torch.zeros(shape, device=U.dev()), 0.1)
    with pytest.raises(ValueError):
        poisson.poisson_select(torch.zeros((4, 3), dtype=I32, device=U.dev()), 0.1)
    with pytest.raises(RuntimeError):
        poisson.poisson_select(P.cpu(), 0.1)
    for n, steps in ((0, 20), (65, 20), (-3, 20), (8, -1), (8, 65)):
        with pytest.raises(ValueError):
            poisson.poisson_subsample(P, n, steps)
    tables = surface.build_surface_tables([m for m, _ in _meshes()], device=U.dev())
    u = torch.rand((1, 32), device=U.dev(), dtype=F64)
    r = torch.rand((1, 32), device=U.dev())
    for n in (0, 33):
        with pytest.raises(ValueError):
            poisson.poisson_disk_sample(tables, _dev(np.array([0], np.int64)), n, u, r, r)
    with pytest.raises(ValueError):
        poisson.poisson_disk_sample(tables, _dev(np.array([2], np.int64)), 8, u, r, r)
    empty = poisson.poisson_select(torch.zeros((0, 8, 3), device=U.dev()), 0.1)
    assert empty[0].shape == (0, 8) and empty[1].shape == (0,)


def test_refusals_of_the_entry_points_launch_nothing():
    from sapcu_amd import _lib
    lib = _lib.load()
    arena = Arena("guard", fill=0xFF, device=U.dev())
    b, C, n = 2, 100, 10
    pts, rad = arena.inp(np.stack([K.sphere(C), K.plane(C)])), arena.inp(np.array([0.1, 0.1], f32))
    keep, count, rounds = arena.out((b, C), torch.uint8), arena.out((b,), I32), arena.out((b,), I32)
    idx, radius = arena.out((b, n), I32), arena.out((b,), F32)
    nbytes = int(lib.sapcu_poisson_workspace_bytes(b, C))
    ws = arena.ws(nbytes)

    def refused(code, name, *args):
        with pytest.raises(_lib.SapcuError) as e:
            _lib.call(name, U.dev(), *args)
        assert e.value.args[0] == code and e.value.args[1], (name, e.value.args)

    ARG, WS = -1, -2
    sel, sub = "sapcu_poisson_select_f32", "sapcu_poisson_subsample_f32"
    for name in (sel, "sapcu_internal_poisson_select_grid"):
        refused(ARG, name, pts, -1, C, rad, keep, count, rounds, ws, nbytes)
        refused(ARG, name, pts, 65536, C, rad, keep, count, rounds, ws, nbytes)
        refused(ARG, name, pts, b, 0, rad, keep, count, rounds, ws, nbytes)
        refused(ARG, name, pts, b, (1 << 24) + 1, rad, keep, count, rounds, ws, nbytes)
        refused(WS, name, pts, b, C, rad, keep, count, rounds, ws, nbytes - 1)
        refused(ARG, name, pts, b, C, rad, keep, count, rounds, None, nbytes)
        refused(ARG, name, pts, b, C, rad, keep, count, rounds, ctypes.c_void_p(ws.data_ptr() + 4), nbytes)
        for hole in range(5):
            args = [pts, rad, keep, count, rounds]
            args[hole] = None
            refused(ARG, name, args[0], b, C, *args[1:], ws, nbytes)
    for bad_n, bad_steps in ((0, 20), (C + 1, 20), (-1, 20), (n, -1), (n, 65)):
        refused(ARG, sub, pts, b, C, bad_n, bad_steps, idx, radius, count, rounds, ws, nbytes)
    refused(ARG, sub, pts, b, 0, n, 20, idx, radius, count, rounds, ws, nbytes)
    refused(ARG, sub, pts, -1, C, n, 20, idx, radius, count, rounds, ws, nbytes)
    refused(WS, sub, pts, b, C, n, 20, idx, radius, count, rounds, ws, nbytes - 1)
    for hole in range(5):
        args = [pts, idx, radius, count, rounds]
        args[hole] = None
        refused(ARG, sub, args[0], b, C, n, 20, *args[1:], ws, nbytes)
    assert lib.sapcu_poisson_workspace_bytes(b, 0) < 0 and lib.sapcu_poisson_workspace_bytes(-1, C) < 0
    _lib.call(sel, U.dev(), pts, 0, C, rad, keep, count, rounds, ws, nbytes)            # b == 0: nothing launched, nothing written
    torch.cuda.synchronize()
    arena.check()
    for g in arena.outs:
        assert bool((g.payload_bits() == 0xFF).all()), g.name


def test_the_headers_under_include_are_unchanged_in_number():
    import os
    from sapcu_amd import _lib
    from abi_tables import HEADERS, ROOT
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(h for h, _ in HEADERS) and len(HEADERS) == 12
    assert "sapcu_poisson.h" in os.listdir(os.path.join(os.path.dirname(_lib.__file__), "csrc"))
