"""Mesh sampling on the device (-m gpu; include/sapcu_surface.h, csrc/surface_sample.hip, sapcu_amd/surface.py, data.MeshSurfacePatches).

Every output of ``sapcu_surface_tables_f32`` and ``sapcu_surface_sample_f32`` must equal tests/surface_ref.py — the numpy restatement
that tests/test_surface_host.py pins bit for bit to the reference's sampler — with ``==``: there is no tolerance anywhere in this file.
Mesh sizes are the leaf, split and remainder boundaries of numpy's pairwise sum, its 8192-element chunks, and the 1024-face tile of
the cdf kernel (SS_CDF_TILE) minus one, itself, plus one and twice plus one; the draws sit exactly on cdf entries, repeated ones
included.  Then the reference fixture itself, the loader, the memory contract of DESIGN section 2 under guard bands, every refusal,
the sampler and the patch builder captured into one graph, and one training step of fn on a loader's batch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import data_ref as R
import gpu_utils as U
import surface_ref as SR
from conftest import golden
from guarded import Arena
from test_surface_host import ITEMS, K, MESHES, N, _case, header_entry_points

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
f32 = np.float32
CDF_TILE = 1024                                                  # csrc/surface_sample.hip SS_CDF_TILE
SIZES = (1, 2, 7, 8, 9, 127, 128, 129, 135, 136, 137, 255, 256, 257, 1023, 1024, 1025, 4097, 20011,
         CDF_TILE - 1, CDF_TILE, CDF_TILE + 1, 2 * CDF_TILE + 1, 8191, 8192, 8193, 16385)
_CACHE = {}


# ------------------------------------------------------------------------------------------------------------ the meshes
def synthetic_mesh(F, seed=0):
    """F random triangles over F // 2 + 3 vertices whose coordinates spread over three orders of magnitude (areas over six); every
    37th face has a repeated corner (area exactly 0)."""
    rng = np.random.default_rng(1000 * seed + F)
    nv = F // 2 + 3
    v = (rng.normal(size=(nv, 3)) * np.exp(rng.uniform(-3.5, 3.5, size=(nv, 1)))).astype(f32)
    f = np.stack([rng.permutation(nv)[:3] for _ in range(F)]).astype(np.int32) if F < 300 else rng.integers(0, nv, size=(F, 3)).astype(np.int32)
    f[::37, 1] = f[::37, 0]
    if F < 37:
        f[0] = np.sort(rng.permutation(nv)[:3])                  # a small mesh keeps a face with area
    return v, f


def fixture_mesh(name):
    c = _case(golden("surface_sample.npz"), name)
    return c["vertices"], c["faces"]


def mesh_and_tables(key):
    """((vertices, faces), surface_ref's tables) of a fixture mesh (by name) or a synthetic one (by size), computed once and shared."""
    if key not in _CACHE:
        mesh = fixture_mesh(key) if isinstance(key, str) else synthetic_mesh(key)
        _CACHE[key] = (mesh, SR.tables(*mesh))
    return _CACHE[key]


def device_tables(keys):
    from sapcu_amd import surface
    k = ("tables",) + tuple(keys)
    if k not in _CACHE:
        _CACHE[k] = surface.build_surface_tables([mesh_and_tables(key)[0] for key in keys], device=U.dev())
    return _CACHE[k]


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(U.dev())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _assert_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = got != want
    assert not bad.any(), "%s differs in %d of %d elements, first at %s: %r against %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])


def _assert_tables(t, keys, what):
    normals, cdf = t.face_normals.cpu().numpy(), t.cdf.cpu().numpy()
    area_sum, prob_sum = t.area_sum.cpu().numpy(), t.prob_sum.cpu().numpy()
    f0 = 0
    for m, key in enumerate(keys):
        (_, faces), tab = mesh_and_tables(key)
        F = len(faces)
        assert t.face_counts[m] == F
        _assert_equal(normals[f0:f0 + F], tab["normals"], "%s: normals of mesh %s" % (what, key))
        _assert_equal(area_sum[m], tab["area_sum"], "%s: area sum of mesh %s" % (what, key))
        _assert_equal(prob_sum[m], tab["prob_sum"], "%s: prob sum of mesh %s" % (what, key))
        _assert_equal(cdf[f0:f0 + F], tab["cdf"], "%s: cdf of mesh %s" % (what, key))
        assert cdf[f0 + F - 1] == 1.0
        f0 += F
    assert f0 == len(cdf)


# ------------------------------------------------------------------------------------------------------------ the tables
def test_tables_of_every_boundary_size_in_one_ragged_call():
    """All synthetic sizes as ONE ragged data set: normals, cdf, area sum and prob sum of every mesh equal the restatement."""
    _assert_tables(device_tables(SIZES), SIZES, "ragged")
    for F in SIZES:                                              # the cases are what they claim: zero-area faces among the others
        areas = mesh_and_tables(F)[1]["areas"]
        assert (areas > 0).any() and (F < 37 or (areas == 0).any())


@pytest.mark.parametrize("name", MESHES)
def test_tables_of_the_fixture_meshes(name):
    _assert_tables(device_tables((name,)), (name,), name)


@pytest.mark.parametrize("F", [1, 129, CDF_TILE + 1, 8193])
def test_tables_of_a_single_mesh(F):
    """The same mesh alone: its tables do not depend on its neighbours in the ragged arrays."""
    _assert_tables(device_tables((F,)), (F,), "alone")


# ------------------------------------------------------------------------------------------------------------ the sampler
def _sample(keys, mesh_idx, u, r1, r2, **kw):
    from sapcu_amd import surface
    t = device_tables(keys)
    n = u.shape[1]
    p, nr, f = surface.sample_surface(t, _dev(np.asarray(mesh_idx, np.int64)), n, _dev(u), _dev(r1), _dev(r2), **kw)
    return p.cpu().numpy(), nr.cpu().numpy(), f.cpu().numpy()


def _reference(keys, mesh_idx, u, r1, r2):
    return SR.batch([mesh_and_tables(k)[0] for k in keys], [mesh_and_tables(k)[1] for k in keys], mesh_idx, u, r1, r2)


def _assert_sampling(got, ref, what):
    for g, r, name in zip(got, ref, ("points", "normals", "faces")):
        assert not (g.dtype.kind == "f" and np.isnan(g).any()), "%s: NaN in %s" % (what, name)
        _assert_equal(g, r, "%s: %s" % (what, name))


@pytest.mark.parametrize("key", ["degenerate", "torus", 137, 2 * CDF_TILE + 1])
def test_draws_on_the_cdf_entries_themselves(key):
    """u equal to cdf entries exactly (every entry below 1, those repeated by zero-area faces included), one ulp below each, 0 and
    nextafter(1, 0); r1 and r2 at 0, at 1 and random.  searchsorted's side='right' decides, and no face of zero area comes back."""
    (_, faces), tab = mesh_and_tables(key)
    cdf = tab["cdf"]
    inner = cdf[cdf < 1.0]
    rng = np.random.default_rng(17)
    u = np.concatenate([inner, np.nextafter(inner[inner > 0], 0.0), [0.0, np.nextafter(1.0, 0.0)], rng.random(64)])
    n = 1024
    b = -(-len(u) // n)
    u = np.concatenate([u, rng.random(b * n - len(u))]).reshape(b, n)
    r1, r2 = rng.random((b, n)).astype(f32), rng.random((b, n)).astype(f32)
    corners = np.array([(0, 0), (0, 1), (1, 0), (1, 1)], f32)
    r1.reshape(-1)[:400:4], r2.reshape(-1)[:400:4] = np.tile(corners[:, 0], 25), np.tile(corners[:, 1], 25)
    got = _sample((key,), [0] * b, u, r1, r2)
    _assert_sampling(got, _reference((key,), [0] * b, u, r1, r2), str(key))
    assert (tab["areas"][got[2]] > 0).all(), "a face of zero area was selected"
    if key != "torus":                                           # the case is what it claims: cdf entries repeated by zero-area faces
        assert (tab["areas"] == 0).any() and len(np.unique(cdf)) < len(cdf)
    # outside the draws' range the face is clamped to the mesh's last one, as the restatement clamps it
    edge = np.array([[1.0, 2.0, -1.0, 0.5]])
    ones = np.full((1, 4), 0.25, f32)
    got = _sample((key,), [0], edge, ones, ones)
    _assert_sampling(got, _reference((key,), [0], edge, ones, ones), "%s, u outside [0, 1)" % key)
    assert got[2][0, 0] == got[2][0, 1] == len(faces) - 1 and got[2][0, 2] == 0


RAGGED = ("icosphere", 9, "torus")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 512, 4096])
def test_ragged_batches(n):
    """Three meshes of different sizes, mesh_idx with repeats and in reverse order."""
    mesh_idx = [2, 1, 0] if n == 4096 else [2, 2, 1, 0, 0, 2, 1]
    rng = np.random.default_rng(n)
    b = len(mesh_idx)
    u, r1, r2 = rng.random((b, n)), rng.random((b, n)).astype(f32), rng.random((b, n)).astype(f32)
    got = _sample(RAGGED, mesh_idx, u, r1, r2)
    _assert_sampling(got, _reference(RAGGED, mesh_idx, u, r1, r2), "n = %d" % n)
    assert got[0].shape == (b, n, 3) and got[2].shape == (b, n)


def test_the_recorded_draws_give_the_reference_sampling():
    """The reference fixture: its u, r1, r2 in; its points, normals and faces out — every mesh, and the two __getitem__ cases."""
    g = golden("surface_sample.npz")
    for name in MESHES + ITEMS:
        c = _case(g, name)
        mesh = str(c["mesh"]) if name in ITEMS else name
        m = MESHES.index(mesh)
        points, normals, faces = _sample(MESHES, [m], c["u"][None], c["r1"][None], c["r2"][None])
        _assert_equal(points[0], c["points"], name + ": points")
        _assert_equal(normals[0], c["normals"], name + ": normals")
        _assert_equal(faces[0], c["face"], name + ": faces")


def test_the_getitem_cases_through_sampler_and_patch_builder():
    """The whole __getitem__ on the device from the recorded draws: the val case from u, r1, r2 alone; the train case through the
    reference's own augmented arrays (its rotation is a BLAS product: tests/test_gpu_data.py holds that stage to its bound)."""
    from sapcu_amd import data, surface
    g = golden("surface_sample.npz")
    c = _case(g, "item_val")
    t = device_tables(MESHES)
    idx = _dev(np.array([MESHES.index(str(c["mesh"]))], np.int64))
    points, normals, _ = surface.sample_surface(t, idx, N, _dev(c["u"][None]), _dev(c["r1"][None]), _dev(c["r2"][None]))
    o = data.build_patches(points, _dev(np.zeros(1, np.int64)), K, normals=normals, centres=_dev(c["centres"][None]))
    for key, out in (("cloud", "cloud"), ("all_normals", "normals"), ("normal", "patch_normals"), ("idx", "idx")):
        _assert_equal(o[out][0].cpu().numpy(), c[key], "item_val: " + key)
    c = _case(g, "item_train")
    o = data.build_patches(_dev(c["aug_cloud"][None]), _dev(np.zeros(1, np.int64)), K, normals=_dev(c["aug_normals"][None]),
                           centres=_dev(c["centres"][None]))
    for key, out in (("cloud", "cloud"), ("all_normals", "normals"), ("normal", "patch_normals"), ("idx", "idx")):
        _assert_equal(o[out][0].cpu().numpy(), c[key], "item_train: " + key)


# -------------------------------------------------------------------------------------------------------------- the loader
def _loader_meshes():
    return [mesh_and_tables(k)[0] for k in ("icosphere", "degenerate", "polygons", 129, 257, 9, "icosphere", 137, 255, 1023)]


def _same_batches(a, b):
    return len(a) == len(b) and all(x.keys() == y.keys() and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


def _assert_batch_is_the_restatement(loader, batch, meshes, what):
    d = loader.last_draws
    idx = batch["index"].cpu().numpy()
    tabs = [SR.tables(*m) for m in meshes]
    u, r1, r2 = d["u"].cpu().numpy(), d["r1"].cpu().numpy(), d["r2"].cpu().numpy()
    assert u.dtype == np.float64 and r1.dtype == r2.dtype == f32 and ((u >= 0) & (u < 1)).all() and ((r1 >= 0) & (r1 <= 1)).all()
    points, normals, faces = SR.batch(meshes, tabs, idx, u, r1, r2)
    _assert_equal(d["faces"].cpu().numpy(), faces, what + ": faces")
    num = lambda key: None if d[key] is None else d[key].cpu().numpy()
    ref = R.batch(points, np.arange(len(idx)), loader.k_neighbors, None, normals, num("rotation"), num("scale"), num("jitter"),
                  batch["centres"].cpu().numpy())
    for key, out in (("input", "patches"), ("normal", "patch_normals"), ("cloud", "cloud"), ("all_normals", "normals")):
        _assert_equal(batch[key].cpu().numpy(), ref[out], "%s: %s" % (what, key))
    from sapcu_amd import data                                   # ... and build_patches fed surface_ref's sampling on the same draws
    o = data.build_patches(_dev(points), _dev(np.arange(len(idx))), loader.k_neighbors, normals=_dev(normals), rotation=d["rotation"],
                           scale=d["scale"], jitter=d["jitter"], centres=batch["centres"].contiguous())
    for key, out in (("input", "patches"), ("normal", "patch_normals"), ("cloud", "cloud"), ("all_normals", "normals")):
        assert torch.equal(batch[key], o[out]), "%s: %s against build_patches" % (what, key)


def test_the_loader_samples_afresh_and_reproducibly():
    from sapcu_amd import data
    meshes = _loader_meshes()
    make = lambda **kw: data.MeshSurfacePatches(meshes, num_points=128, num_patches=16, k_neighbors=12, batch_size=4, seed=3,
                                                device=U.dev(), **kw)
    train, val = make(), make(split="val")
    assert train.samples == 9 and val.samples == 1 and len(train) == 3 and train.augment and not val.augment
    first = list(train)
    assert [b["input"].shape for b in first] == [(4, 16, 12, 3), (4, 16, 12, 3), (1, 16, 12, 3)]
    assert first[0]["normal"].shape == (4, 16, 3) and first[0]["cloud"].shape == first[0]["all_normals"].shape == (4, 128, 3)
    assert sorted(torch.cat([b["index"] for b in first]).tolist()) == list(range(9))
    assert _same_batches(first, list(make())) and _same_batches(first, list(train))         # the same (seed, epoch, batch): bit-identical
    for batch in train:                                          # every batch is build_patches fed surface_ref on last_draws
        _assert_batch_is_the_restatement(train, batch, meshes[:9], "train")
        assert set(train.last_draws) == {"u", "r1", "r2", "faces", "theta", "rotation", "scale", "jitter", "centres"}
    # two epochs: a different sampling of the same mesh — the raw sampled points, not only their augmentation
    train.augment = False
    clouds = {}
    for epoch in (0, 1):
        for batch in train.set_epoch(epoch):
            for i, cloud in zip(batch["index"].tolist(), batch["cloud"]):
                clouds[(epoch, i)] = cloud
    assert all(not torch.equal(clouds[(0, i)], clouds[(1, i)]) for i in range(9))
    # the val split samples too, without augmenting: the last tenth of the meshes, a new cloud per epoch
    seen = []
    for epoch in (0, 2):
        (vb,) = list(val.set_epoch(epoch))
        d = val.last_draws
        assert d["rotation"] is None and d["scale"] is None and d["jitter"] is None and d["theta"] is None and d["u"] is not None
        assert vb["index"].tolist() == [0]
        _assert_batch_is_the_restatement(val, vb, meshes[9:], "val")
        seen.append(vb["cloud"])
    assert not torch.equal(seen[0], seen[1])
    # n <= num_patches: every point is a centre, in order
    few = data.MeshSurfacePatches(meshes, num_points=16, num_patches=16, k_neighbors=12, batch_size=3, split="all", device=U.dev())
    batch = next(iter(few))
    assert batch["input"].shape == (3, 16, 12, 3) and (batch["centres"].cpu().numpy() == np.arange(16)).all()


def test_the_loader_reads_a_folder_as_the_reference_does(tmp_path):
    from sapcu_amd import data
    g = golden("surface_sample.npz")
    text = _case(g, "polygons")["off_text"].tobytes()
    for cat, name in (("b", "two.off"), ("a", "one.off"), ("b", "three.off")):
        (tmp_path / cat).mkdir(exist_ok=True)
        (tmp_path / cat / name).write_bytes(text)
    loader = data.MeshSurfacePatches(str(tmp_path), num_points=64, num_patches=8, k_neighbors=4, split="all", batch_size=3, shuffle=False,
                                     augment=False, device=U.dev())
    assert [n.split("/")[-2:] for n in loader.tables.names] == [["a", "one.off"], ["b", "three.off"], ["b", "two.off"]]
    (batch,) = list(loader)
    mesh = fixture_mesh("polygons")                              # the reference loader's vertices and fanned faces of the same text
    _assert_equal(loader.tables.mesh(1)[0].cpu().numpy(), mesh[0], "vertices")
    _assert_equal(loader.tables.mesh(1)[1].cpu().numpy(), mesh[1], "faces")
    _assert_batch_is_the_restatement(loader, batch, [mesh] * 3, "folder")
    assert data.MeshSurfacePatches(str(tmp_path), split="train", device=U.dev()).samples == 2


def test_meshes_that_cannot_be_sampled_are_refused_by_name():
    from sapcu_amd import data, surface
    good = mesh_and_tables("icosphere")[0]
    v, f = good
    bad_index = (v, np.concatenate([f[:5], [[0, 1, len(v)]]]).astype(np.int32))
    negative = (v, np.concatenate([f[:5], [[0, -1, 2]]]).astype(np.int32))
    flat = (v, np.tile(np.array([[4, 4, 9]], np.int32), (6, 1)))                       # every face without area
    tiny = ((v * f32(1e-6)).astype(f32), f)                                            # so small that + 1e-8 matters
    cases = (("bad", bad_index), ("bad", negative), ("bad", (v, f[:0])), ("bad", (v[:0], f)), ("bad", flat), ("bad", tiny))
    for name, mesh in cases:
        with pytest.raises(ValueError, match="bad"):
            surface.build_surface_tables([good, mesh], device=U.dev(), names=["good", name])
        with pytest.raises(ValueError, match="mesh 1"):
            data.MeshSurfacePatches([good, mesh], split="all", device=U.dev())
    with pytest.raises(ValueError):
        _sample(("icosphere",), [0, 1], np.zeros((2, 4)), np.zeros((2, 4), f32), np.zeros((2, 4), f32))       # mesh_idx outside [0, S)
    with pytest.raises(ValueError):
        _sample(("icosphere",), [-1], np.zeros((1, 4)), np.zeros((1, 4), f32), np.zeros((1, 4), f32))
    with pytest.raises(RuntimeError):
        surface.sample_surface(device_tables(("icosphere",)), torch.zeros(1, dtype=I64), 4, torch.zeros(1, 4, dtype=F64),
                               torch.zeros(1, 4), torch.zeros(1, 4))


# ------------------------------------------------------------------------------------------------------- the C entry points
def _lib():
    from sapcu_amd import _lib
    return _lib


def _ragged(meshes):
    vcount, fcount = [len(v) for v, _ in meshes], [len(f) for _, f in meshes]
    return {"vertices": np.concatenate([v for v, _ in meshes]).astype(f32), "faces": np.concatenate([f for _, f in meshes]).astype(np.int32),
            "vert_off": np.concatenate([[0], np.cumsum(vcount)]).astype(np.int64),
            "face_off": np.concatenate([[0], np.cumsum(fcount)]).astype(np.int64)}


TABLE_OUT = ("face_normals", "cdf", "area_sum", "prob_sum")
SAMPLE_OUT = ("points", "normals_out", "face")
GUARD_MESHES = ("degenerate", 9, CDF_TILE + 1, 1, 8193)


def _buffers(arena, keys, mesh_idx, n, odd=False, ragged=None):
    """The buffers of both calls in `arena`; with `odd` every base address is an odd multiple of its element size away from the
    512-byte boundary the allocator gives (the f64 arrays stay 8-byte aligned, the workspace 4-byte)."""
    rg = _ragged([mesh_and_tables(k)[0] for k in keys]) if ragged is None else ragged
    S, tv, tf, b = len(rg["vert_off"]) - 1, len(rg["vertices"]), len(rg["faces"]), len(mesh_idx)
    off = iter(range(1, 99, 2))
    nxt = (lambda esize: esize * next(off)) if odd else (lambda esize: 0)
    rng = np.random.default_rng(b * n + 1)
    bufs = {"S": S, "tv": tv, "tf": tf, "b": b, "n": n}
    inputs = dict(rg, midx=np.asarray(mesh_idx, np.int64), u=rng.random((b, n)), r1=rng.random((b, n)).astype(f32),
                  r2=rng.random((b, n)).astype(f32))
    bufs["host"] = inputs
    for name, a in inputs.items():
        bufs[name] = arena.inp(a, offset=nxt(a.dtype.itemsize), name=name)
    shapes = {"face_normals": ((tf, 3), F32), "cdf": ((tf,), F64), "area_sum": ((S,), F32), "prob_sum": ((S,), F64),
              "points": ((b, n, 3), F32), "normals_out": ((b, n, 3), F32), "face": ((b, n), I32)}
    for name, (shape, dtype) in shapes.items():
        bufs[name] = arena.out(shape, dtype, offset=nxt(8 if dtype == F64 else 4), name=name)
    bufs["nbytes"] = int(_lib().load().sapcu_surface_tables_workspace_bytes(S, tf))
    bufs["ws"] = arena.ws(bufs["nbytes"], offset=nxt(4), name="workspace")
    return bufs


def _args(bufs, over):
    L = _lib()
    a = {k: (L.ptr(v) if torch.is_tensor(v) else v) for k, v in bufs.items() if k != "host"}
    a.update(over)
    return a


def _launch_tables(bufs, **over):
    L, a = _lib(), _args(bufs, over)
    rc = L.load().sapcu_surface_tables_f32(a["vertices"], a["vert_off"], a["tv"], a["faces"], a["face_off"], a["tf"], a["S"],
                                           a["face_normals"], a["cdf"], a["area_sum"], a["prob_sum"], a["ws"], a["nbytes"],
                                           L.current_stream())
    torch.cuda.synchronize()
    return rc


def _launch_sample(bufs, **over):
    L, a = _lib(), _args(bufs, over)
    rc = L.load().sapcu_surface_sample_f32(a["vertices"], a["vert_off"], a["tv"], a["faces"], a["face_off"], a["tf"], a["face_normals"],
                                           a["cdf"], a["S"], a["midx"], a["b"], a["n"], a["u"], a["r1"], a["r2"], a["points"],
                                           a["normals_out"], a["face"], L.current_stream())
    torch.cuda.synchronize()
    return rc


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def _assert_c_outputs(bufs, keys, mesh_idx, what, skip=()):
    f0 = 0
    got = {k: bufs[k].cpu().numpy() for k in TABLE_OUT + SAMPLE_OUT if k not in skip}
    for m, key in enumerate(keys):
        (_, faces), tab = mesh_and_tables(key)
        F = len(faces)
        for name, want in (("face_normals", tab["normals"]), ("cdf", tab["cdf"])):
            if name not in skip:
                _assert_equal(got[name][f0:f0 + F], want, "%s: %s of mesh %s" % (what, name, key))
        for name in ("area_sum", "prob_sum"):
            if name not in skip:
                _assert_equal(got[name][m], tab[name], "%s: %s of mesh %s" % (what, name, key))
        f0 += F
    h = bufs["host"]
    ref = _reference(keys, mesh_idx, h["u"], h["r1"], h["r2"])
    for name, want in zip(SAMPLE_OUT, ref):
        if name not in skip:
            _assert_equal(got[name], want, "%s: %s" % (what, name))


def test_memory_contract_under_guard_bands():
    """The three runs of DESIGN section 2 for both calls: 0xFF bands and workspace with 0xFF-prefilled outputs, 0x00 bands and
    workspace, the dirty workspace again — guards intact, every output written in full, bit-identical across the runs and equal to
    the restatement; every base address odd."""
    mesh_idx = [4, 0, 2, 2, 1, 3, 0]
    results = []
    for fill in (0xFF, 0x00):
        arena = Arena("guard", fill=fill, device=U.dev())
        bufs = _buffers(arena, GUARD_MESHES, mesh_idx, 65, odd=True)
        for again in range(2 if fill == 0x00 else 1):
            arena.refill_outputs()
            assert _launch_tables(bufs) == 0, _lib().load().sapcu_last_error()
            assert _launch_sample(bufs) == 0, _lib().load().sapcu_last_error()
            arena.check()
            _assert_c_outputs(bufs, GUARD_MESHES, mesh_idx, "fill %#x run %d" % (fill, again))      # nothing left 0xFF: written in full
            results.append({k: _bits(bufs[k].cpu().numpy()) for k in TABLE_OUT + SAMPLE_OUT})
    for got in results[1:]:
        for key in got:
            assert np.array_equal(got[key], results[0][key]), key


def test_every_optional_output_null_in_turn():
    """A NULL optional output changes nothing in the others, and the buffer that was not passed is not written."""
    mesh_idx = [1, 0, 1]
    keys = ("degenerate", 257)
    for drop in (("area_sum",), ("prob_sum",), ("face",), ("area_sum", "prob_sum", "face")):
        bufs = _buffers(Arena("compact", device=U.dev()), keys, mesh_idx, 64)
        over = {d: None for d in drop}
        assert _launch_tables(bufs, **over) == 0 and _launch_sample(bufs, **over) == 0, _lib().load().sapcu_last_error()
        _assert_c_outputs(bufs, keys, mesh_idx, "without " + "+".join(drop), skip=drop)
        for d in drop:
            assert _untouched(bufs[d]), d


def test_refusals_launch_nothing():
    """Every refusal of include/sapcu_surface.h returns SAPCU_ERR_ARG and leaves the 0xFF-prefilled outputs, the workspace and the
    guards alone; b == 0 and S == 0 launch nothing; the same buffers are then accepted as they are."""
    mesh_idx = [1, 0]
    keys = ("degenerate", 129)
    arena = Arena("guard", fill=0xFF, device=U.dev())
    bufs = _buffers(arena, keys, mesh_idx, 63)
    wsp = bufs["ws"].data_ptr()
    tables_refusals = [dict(S=-1), dict(S=(1 << 20) + 1), dict(tf=0), dict(tf=-1), dict(tf=(1 << 29) + 1), dict(tv=0), dict(tv=1 << 31),
                       dict(vertices=None), dict(vert_off=None), dict(faces=None), dict(face_off=None), dict(face_normals=None),
                       dict(cdf=None), dict(ws=None), dict(nbytes=bufs["nbytes"] - 1), dict(nbytes=0), dict(ws=ctypes.c_void_p(wsp + 2))]
    sample_refusals = [dict(S=-1), dict(S=(1 << 20) + 1), dict(tf=0), dict(tf=(1 << 29) + 1), dict(tv=0), dict(n=0), dict(n=4097),
                       dict(b=-1), dict(b=(1 << 20) + 1), dict(vertices=None), dict(vert_off=None), dict(faces=None), dict(face_off=None),
                       dict(face_normals=None), dict(cdf=None), dict(midx=None), dict(u=None), dict(r1=None), dict(r2=None),
                       dict(points=None), dict(normals_out=None)]

    def nothing_written(what):
        arena.check()
        for name in TABLE_OUT + SAMPLE_OUT + ("ws",):
            assert _untouched(bufs[name]), (what, name)

    for launch, refusals in ((_launch_tables, tables_refusals), (_launch_sample, sample_refusals)):
        for over in refusals:
            assert launch(bufs, **over) == -1, over
            assert _lib().load().sapcu_last_error()
            nothing_written(over)
    assert _launch_tables(bufs, S=0) == 0 and _launch_sample(bufs, S=0) == 0 and _launch_sample(bufs, b=0) == 0
    nothing_written("b == 0 or S == 0")
    assert _launch_tables(bufs) == 0 and _launch_sample(bufs) == 0
    arena.check()
    _assert_c_outputs(bufs, keys, mesh_idx, "after the refusals")


def test_bad_index_values_are_harmless_in_the_kernels():
    """The documented split (include/sapcu_surface.h): the Python layer validates index VALUES; the kernels stay memory-safe on bad
    ones — a face with a vertex index outside its mesh counts as area 0 and normal 0 and is never selected, an entry whose mesh_idx
    is outside [0,S) keeps its 0xFF, and nothing is read or written out of bounds (guards)."""
    keys = ("degenerate", 129)
    meshes = [mesh_and_tables(k)[0] for k in keys]
    v1, f1 = meshes[1]
    f1 = f1.copy()
    f1[7], f1[50], f1[128] = [0, 1, len(v1)], [-1, 2, 3], [1 << 30, 0, 1]
    bad = [meshes[0], (v1, f1)]
    valid = np.ones(129, bool)
    valid[[7, 50, 128]] = False
    tab = SR.tables(v1, np.where(valid[:, None], f1, 0))          # the bad faces as (0, 0, 0): area 0, normal 0
    mesh_idx = [1, 2, 0, -1, 1, 1 << 40]
    arena = Arena("guard", fill=0xFF, device=U.dev())
    bufs = _buffers(arena, keys, mesh_idx, 512, odd=True, ragged=_ragged(bad))
    assert _launch_tables(bufs) == 0 and _launch_sample(bufs) == 0
    arena.check()
    F0 = len(meshes[0][1])
    _assert_equal(bufs["face_normals"].cpu().numpy()[F0:], tab["normals"], "normals")
    _assert_equal(bufs["cdf"].cpu().numpy()[F0:], tab["cdf"], "cdf")
    _assert_equal(bufs["area_sum"].cpu().numpy()[1], tab["area_sum"], "area sum")
    assert (bufs["face_normals"].cpu().numpy()[F0:][~valid] == 0).all()
    h = bufs["host"]
    for e, m in enumerate(mesh_idx):
        if not 0 <= m < 2:
            assert all(_untouched(bufs[k][e]) for k in SAMPLE_OUT), e
            continue
        mesh, t = (meshes[0], mesh_and_tables(keys[0])[1]) if m == 0 else ((v1, np.where(valid[:, None], f1, 0)), tab)
        ref = SR.sample(mesh[0], mesh[1], t, h["u"][e], h["r1"][e], h["r2"][e])
        for name, want in zip(SAMPLE_OUT, ref):
            _assert_equal(bufs[name][e].cpu().numpy(), want, "entry %d: %s" % (e, name))
        assert m == 0 or valid[ref[2]].all()


def test_every_pointer_taking_entry_point_of_the_header_runs_under_guards():
    decl = header_entry_points()
    assert set(decl) == set(_lib().SURFACE_EXPORTS)
    assert {n for n in decl if "*" in decl[n]} == {"sapcu_surface_tables_f32", "sapcu_surface_sample_f32"}     # _launch_tables / _launch_sample
    assert {n for n in decl if n.endswith("workspace_bytes")} == {"sapcu_surface_tables_workspace_bytes"}


# ------------------------------------------------------------------------------------------------------------------ capture
def test_sampler_and_patch_builder_replay_as_one_graph():
    """sample_surface followed by build_patches(validate=False) on pre-drawn draws, captured once on one stream and replayed twice:
    the outputs equal the eager ones."""
    from sapcu_amd import data, surface
    t = device_tables(RAGGED)
    b, n = 4, 128
    gen = torch.Generator(device=U.dev()).manual_seed(11)
    idx = _dev(np.array([2, 0, 1, 2], np.int64))
    rows = torch.arange(b, dtype=I64, device=U.dev())
    u = torch.rand((b, n), generator=gen, device=U.dev(), dtype=F64)
    r1, r2 = torch.rand((b, n), generator=gen, device=U.dev()), torch.rand((b, n), generator=gen, device=U.dev())
    centres = torch.argsort(torch.rand((b, n), generator=gen, device=U.dev()), dim=1)[:, :16].to(I32).contiguous()
    jitter = torch.randn((b, n, 3), generator=gen, device=U.dev()) * 0.002

    def run():
        p, nr, f = surface.sample_surface(t, idx, n, u, r1, r2, validate=False)
        o = data.build_patches(p, rows, 12, normals=nr, jitter=jitter, centres=centres, validate=False)
        return dict(o, points=p, sampled_normals=nr, faces=f)

    eager = {k: v.clone() for k, v in run().items()}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=U.dev())
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = run()
    for _ in range(2):
        for v in out.values():
            v.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(out[k], eager[k]), k
    assert not torch.isnan(eager["patches"]).any() and (eager["faces"] >= 0).all()


# ----------------------------------------------------------------------------------------------------------- into the trainer
def test_an_fn_training_step_on_a_mesh_surface_batch():
    from sapcu_amd import data
    from test_gpu_data import _fn_trainer, _params
    meshes = [mesh_and_tables("icosphere")[0], mesh_and_tables("polygons")[0]]
    loader = data.MeshSurfacePatches(meshes, num_points=128, num_patches=8, k_neighbors=12, split="all", batch_size=2, seed=3, augment=True,
                                     device=U.dev())
    batch = next(iter(loader))
    assert batch["input"].shape == (2, 8, 12, 3) and batch["normal"].shape == (2, 8, 3)
    model, tr = _fn_trainer()
    before = _params(model)
    loss, _ = tr.train_step(batch)
    assert loss is not None and math.isfinite(float(loss)), loss
    assert any(not torch.equal(a, b) for a, b in zip(before, _params(model)))
