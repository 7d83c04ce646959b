"""sapcu_amd.pointing and the seed-centred loaders on the device against the definition (tests/pointing_ref.py on the cases of
tests/pointing_cases.py): every output bit for bit on the brute-force route, on the grid at any cell size, across the split into
calls, under guard bands with a dirty workspace, and through the loaders into one training step of fn and of fd."""
import ctypes
import math

import numpy as np
import pytest
import torch

import gpu_utils as U
import poison
import pointing_cases as K
import pointing_ref as R
from guarded import Arena

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
ENTRY = "sapcu_pointing_samples_f32"


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(U.dev())


def _np(d):
    return {key: v.cpu().numpy() for key, v in d.items()}


def _run(name, **kw):
    """pointing_samples on the case `name` with every per-candidate output -> (numpy dict, info)."""
    from sapcu_amd import pointing
    c, info = K.CASES[name], []
    args = dict(K.geometry(c), return_all=True, info=info)
    args.update(kw)
    got = _np(pointing.pointing_samples(_dev(c["P"]), _dev(c["voxels"]), _dev(c["jitter"]), **args))
    return got, info


def _assert_is_ref(got, ref, what):
    """Every output against the definition's: bit for bit, a NaN equal to a NaN."""
    if "keep" in got:
        assert np.array_equal(got["keep"], ref["keep"]), what
        assert got["d1"].dtype == np.float64 and np.array_equal(got["d1"], ref["d1"]), what
        assert got["idx"].dtype == np.int32 and np.array_equal(got["idx"], ref["idx"]), what
    assert got["points"].shape == (ref["count"], 3) and got["candidate"].dtype == np.int64, what
    assert np.array_equal(got["candidate"], ref["candidate"]), what
    assert np.array_equal(got["points"], ref["points"]), what
    assert np.array_equal(got["pointing"], ref["pointing"], equal_nan=True), what


def _assert_same(a, b, what):
    assert sorted(a) == sorted(b), what
    for key in a:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), (what, key)


# ---------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("name", K.PLAIN + K.MADE)
def test_every_output_equals_the_definition_on_the_automatic_route(name):
    c = K.CASES[name]
    got, info = _run(name)
    _assert_is_ref(got, K.reference(name), name)
    grid = len(c["P"]) >= K.GRID_MIN_N and bool(np.isfinite(c["P"]).all())
    assert info[0] == int(grid) and (all(g >= 1 for g in info[1:]) if grid else info[1:] == [0, 0, 0])
    if name in K.PLAIN:
        unit = np.sqrt((got["pointing"] ** 2).sum(1))
        assert np.abs(unit - 1).max() < 1e-15 * 4


FORCED = ("sphere-500", "sphere-5000", "sphere-5000-k1", "sphere-5000-k16", "torus-6000", "lattice-tie-k1", "lattice-tie-k6",
          "lattice-tie-k10", "zero-len-k6", "k-equals-n", "one-point", "duplicates")


@pytest.mark.parametrize("name", FORCED)
def test_the_grid_at_a_tiny_a_moderate_and_a_one_cell_size(name):
    ref, runs = K.reference(name), []
    for cell in (0.004, 0.06, 10.0):
        got, info = _run(name, cell_size=cell)
        assert info[0] == 1, (name, cell, info)
        if cell == 10.0:
            assert info[1:] == [1, 1, 1]
        elif len(K.CASES[name]["P"]) >= 500:
            assert max(info[1:]) > 1
        _assert_is_ref(got, ref, (name, cell))
        runs.append(got)
    _assert_same(runs[0], runs[1], name)
    _assert_same(runs[0], runs[2], name)


def test_non_finite_surface_points_take_the_fallback_and_are_never_neighbours():
    for cell in (0.0, 0.05):
        got, info = _run("non-finite", cell_size=cell)
        assert info == [0, 0, 0, 0]
        _assert_is_ref(got, K.reference("non-finite"), cell)
        assert not np.isin(got["idx"], (17, 101, 150)).any()
    from sapcu_amd import pointing
    c = K.CASES["non-finite"]                                        # a bounding box that is not finite prunes no centre
    assert np.array_equal(pointing.near_voxels(_dev(c["P"]), c["origin"], c["step"], c["count"]).cpu().numpy(), c["voxels"])


@pytest.mark.parametrize("name", ("sphere-5000-k1", "sphere-5000-k6", "sphere-5000", "sphere-5000-k16", "sphere-500"))
def test_idx_and_d1_equal_knn_gather(name):
    from sapcu_amd import generation
    c, ref = K.CASES[name], K.reference(name)
    assert c["k"] in (1, 6, 10, 16)
    got, _ = _run(name)
    idx, dist, _ = generation.knn_gather(_dev(c["P"].astype(np.float64)), _dev(ref["q"]), c["k"], want_dist=True, want_patch=False)
    assert np.array_equal(got["idx"], idx.cpu().numpy().astype(np.int32))
    assert np.array_equal(got["d1"], dist.cpu().numpy()[:, 0])


@pytest.mark.parametrize("name", ("sphere-5000", "torus-6000", "lattice-tie-k6", "sphere-500", "zero-len-k6", "non-finite"))
@pytest.mark.parametrize("cell", (0.0, 0.004))
def test_without_the_per_candidate_outputs_the_walk_may_leave_early_and_keeps_the_same(name, cell):
    got, _ = _run(name, cell_size=cell, return_all=False)
    assert sorted(got) == ["candidate", "pointing", "points"]
    _assert_is_ref(got, K.reference(name), (name, cell))


def test_a_band_of_one_distance_keeps_exactly_the_candidates_at_it():
    for name in ("sphere-500", "sphere-5000", "lattice-tie-k6"):
        c = K.CASES[name]
        first, _ = _run(name)
        d = float(np.sort(first["d1"][first["keep"]])[len(first["points"]) // 2])
        for all_outputs in (True, False):
            got, _ = _run(name, band=(d, d), return_all=all_outputs)
            want = R.export_pointing(c["P"], c["voxels"], c["jitter"], **dict(K.geometry(c), band=(d, d)))
            _assert_is_ref(got, want, name)
            assert np.array_equal(got["candidate"], np.flatnonzero(first["d1"] == d)) and len(got["candidate"]) >= 1
        for band in ((np.nextafter(d, 1), 1.0), (0.0, np.nextafter(d, 0))):        # both ends are inclusive, and no wider
            got, _ = _run(name, band=band)
            assert not np.isin(np.flatnonzero(first["d1"] == d), got["candidate"]).any()


def test_more_neighbours_than_points_is_refused():
    from sapcu_amd import pointing
    c = K.CASES["k-equals-n"]
    with pytest.raises(ValueError):
        pointing.pointing_samples(_dev(c["P"]), _dev(c["voxels"]), None, **dict(K.geometry(c), k=8))
    with pytest.raises(ValueError):
        pointing.pointing_samples(_dev(c["P"][:1]), _dev(c["voxels"]), None, **dict(K.geometry(c), k=2))


@pytest.mark.parametrize("name", ("duplicates", "noisy-4097-nojitter"))
def test_the_split_into_calls_changes_nothing(name):
    whole, _ = _run(name)
    _assert_is_ref(whole, K.reference(name), name)
    for per in (1, 7):
        part, _ = _run(name, voxels_per_call=per)
        _assert_same(whole, part, (name, per))


def test_no_jitter_is_a_zero_jitter():
    from sapcu_amd import pointing
    name = "noisy-4097-nojitter"
    c = K.CASES[name]
    assert c["jitter"] is None
    none, _ = _run(name)
    zero = _np(pointing.pointing_samples(_dev(c["P"]), _dev(c["voxels"]), torch.zeros((len(c["voxels"]) * c["sub"] ** 3, 3), dtype=F64, device=U.dev()),
                                         return_all=True, **K.geometry(c)))
    _assert_same(none, zero, name)


def test_an_empty_voxel_list_gives_empty_tensors():
    from sapcu_amd import pointing
    c = K.CASES["sphere-500"]
    out = pointing.pointing_samples(_dev(c["P"]), torch.zeros((0,), dtype=I64, device=U.dev()), None, return_all=True, **K.geometry(c))
    assert out["points"].shape == (0, 3) and out["pointing"].shape == (0, 3) and out["candidate"].shape == (0,)
    assert out["keep"].shape == (0,) and out["d1"].shape == (0,) and out["idx"].shape == (0, 10)
    assert out["points"].dtype == F64 and out["candidate"].dtype == I64 and out["keep"].dtype == torch.bool and out["idx"].dtype == I32
    assert all(v.is_cuda for v in out.values())


# ------------------------------------------------------------------------------------------------------ memory contract
def _raw(arena, name, per_candidate=True, cell_size=0.0):
    """One call of the entry point on the arena's buffers -> ([keep, d1, idx, points, pointing, candidate, count] as numpy, the
    compacted ones whole, info)."""
    from sapcu_amd import _lib
    c = K.CASES[name]
    n, nv, sub, k = len(c["P"]), len(c["voxels"]), c["sub"], c["k"]
    m = nv * sub ** 3
    P, vox = arena.inp(c["P"], name="surface"), arena.inp(c["voxels"], name="voxels")
    jit = None if c["jitter"] is None else arena.inp(c["jitter"], name="jitter")
    keep = arena.out((m,), torch.uint8, name="keep")
    d1 = arena.out((m,), F64, name="d1") if per_candidate else None
    idx = arena.out((m, k), I32, name="idx") if per_candidate else None
    points, pointing = arena.out((m, 3), F64, name="points"), arena.out((m, 3), F64, name="pointing")
    candidate, count = arena.out((m,), I64, name="candidate"), arena.out((1,), I64, name="count")
    nbytes = int(_lib.load().sapcu_pointing_workspace_bytes(n, nv, sub, k))
    assert nbytes > 0
    ws = arena.ws(nbytes)
    info = (ctypes.c_int64 * 4)()
    step2 = c["step"] / sub
    _lib.call(ENTRY, U.dev(), P, n, vox, nv, c["origin"], c["step"], c["count"], sub, step2, step2 / 2, jit, k, c["band"][0], c["band"][1],
              cell_size, 0, keep, d1, idx, points, pointing, candidate, count, ws, nbytes, info)
    torch.cuda.synchronize()
    arena.check()
    return [None if t is None else t.cpu().numpy() for t in (keep, d1, idx, points, pointing, candidate, count)], list(info)


@pytest.mark.parametrize("name,cell,per_candidate", [("sphere-500", 0.0, True), ("sphere-5000", 0.0, True), ("sphere-5000", 0.0, False),
                                                     ("torus-6000", 0.004, True), ("non-finite", 0.0, True), ("lattice-tie-k6", 0.06, False)])
def test_the_entry_point_under_guard_bands_with_a_dirty_workspace(name, cell, per_candidate):
    ref = K.reference(name)
    runs = [_raw(Arena("guard", fill=fill, device=U.dev()), name, per_candidate, cell)[0] for fill in (0xFF, 0x00, 0xFF)]
    runs.append(_raw(Arena("compact", device=U.dev()), name, per_candidate, cell)[0])
    for other in runs[1:]:                                            # two equal runs, and nothing read from the workspace's past
        for a, b in zip(runs[0], other):
            assert (a is None and b is None) or a.tobytes() == b.tobytes()
    keep, d1, idx, points, pointing, candidate, count = runs[0]
    c = int(count[0])
    assert c == ref["count"] and np.array_equal(keep.astype(bool), ref["keep"]) and set(np.unique(keep)) <= {0, 1}
    if per_candidate:
        assert np.array_equal(d1, ref["d1"]) and np.array_equal(idx, ref["idx"])
    assert np.array_equal(points[:c], ref["points"]) and np.array_equal(pointing[:c], ref["pointing"], equal_nan=True)
    assert np.array_equal(candidate[:c], ref["candidate"])
    # the compacted outputs are written in their first `count` rows and nowhere else
    assert (points[c:].view(np.uint8) == 0xFF).all() and (pointing[c:].view(np.uint8) == 0xFF).all() and (candidate[c:] == -1).all()


def test_results_do_not_depend_on_what_torch_empty_returns(monkeypatch):
    from sapcu_amd import data, pointing
    c = K.CASES["sphere-5000-k6"]
    ref = K.reference("sphere-5000-k6")

    def scenario():
        out = pointing.pointing_samples(_dev(c["P"]), _dev(c["voxels"]), _dev(c["jitter"]), return_all=True, voxels_per_call=50, **K.geometry(c))
        q = out["points"][:64].contiguous()
        out["patches"] = data.seed_patches(_dev(c["P"]), q, 12)
        out["rotated"] = data.seed_patches(_dev(c["P"]), q, 12, normals=out["pointing"][:64].float())
        return _np(out)

    clean = scenario()
    _assert_is_ref(clean, ref, "clean")
    for pattern in poison.PATTERNS:
        with poison.poisoned(monkeypatch, pattern):
            got = scenario()
        _assert_same(clean, got, pattern)


def test_refusals_of_the_entry_point_leave_every_output_byte_as_it_was():
    from sapcu_amd import _lib
    lib = _lib.load()
    arena = Arena("guard", fill=0xFF, device=U.dev())
    c = K.CASES["sphere-500"]
    n, nv, sub, k = len(c["P"]), len(c["voxels"]), c["sub"], c["k"]
    m = nv * sub ** 3
    P, vox, jit = arena.inp(c["P"]), arena.inp(c["voxels"]), arena.inp(c["jitter"])
    outs = [arena.out((m,), torch.uint8, name="keep"), arena.out((m,), F64, name="d1"), arena.out((m, k), I32, name="idx"),
            arena.out((m, 3), F64, name="points"), arena.out((m, 3), F64, name="pointing"), arena.out((m,), I64, name="candidate"),
            arena.out((1,), I64, name="count")]
    nbytes = int(lib.sapcu_pointing_workspace_bytes(n, nv, sub, k))
    ws = arena.ws(nbytes)
    step2 = c["step"] / sub
    good = dict(surface=P, n=n, voxels=vox, nv=nv, origin=c["origin"], step=c["step"], count=c["count"], sub=sub, step2=step2, half2=step2 / 2,
                jitter=jit, k=k, lo=c["band"][0], hi=c["band"][1], cell=0.0, first=0, keep=outs[0], d1=outs[1], idx=outs[2], points=outs[3],
                pointing=outs[4], candidate=outs[5], kept=outs[6], ws=ws, nbytes=nbytes)

    def refused(**change):
        a = dict(good, **change)
        with pytest.raises(_lib.SapcuError) as e:
            _lib.call(ENTRY, U.dev(), *[a[key] for key in good], None)
        assert e.value.args[0] == -1 and e.value.args[1], (change, e.value.args)

    nan, inf = float("nan"), float("inf")
    for change in (dict(n=0), dict(n=(1 << 29) + 1), dict(nv=-1), dict(nv=(1 << 31) // 27 + 1), dict(count=0), dict(count=(1 << 20) + 1),
                   dict(sub=0), dict(sub=1025), dict(k=0), dict(k=17), dict(n=5), dict(origin=nan), dict(step=inf), dict(step2=nan),
                   dict(half2=-inf), dict(lo=nan), dict(hi=nan), dict(cell=-1.0), dict(cell=inf), dict(cell=nan), dict(first=-1),
                   dict(nbytes=nbytes - 1), dict(ws=None), dict(ws=ctypes.c_void_p(ws.data_ptr() + 4)),
                   dict(surface=None), dict(voxels=None), dict(keep=None), dict(points=None), dict(pointing=None), dict(candidate=None),
                   dict(kept=None)):
        refused(**change)
    assert lib.sapcu_pointing_workspace_bytes(n, nv, sub, 17) < 0 and lib.sapcu_pointing_workspace_bytes(0, nv, sub, k) < 0
    info = (ctypes.c_int64 * 4)(9, 9, 9, 9)
    _lib.call(ENTRY, U.dev(), *[dict(good, nv=0)[key] for key in good], info)             # no voxel: nothing launched, nothing written
    torch.cuda.synchronize()
    assert list(info) == [0, 0, 0, 0]
    arena.check()
    for g in arena.outs:
        assert bool((g.payload_bits() == 0xFF).all()), g.name
    _lib.call(ENTRY, U.dev(), *[good[key] for key in good], info)                         # and the arguments as they are run
    torch.cuda.synchronize()
    arena.check()
    assert int(outs[6].item()) == K.reference("sphere-500")["count"]


# ------------------------------------------------------------------------------------------------------------ near_voxels
@pytest.mark.parametrize("name", K.PLAIN + ("lattice-tie-k6", "one-point", "duplicates"))
def test_near_voxels_equals_the_definition(name):
    from sapcu_amd import pointing
    c = K.CASES[name]
    got = pointing.near_voxels(_dev(c["P"]), c["origin"], c["step"], c["count"], c["near"])
    assert got.dtype == I64 and got.is_cuda and np.array_equal(got.cpu().numpy(), c["voxels"])
    default = pointing.near_voxels(_dev(c["P"]), c["origin"], c["step"], c["count"])
    assert np.array_equal(default.cpu().numpy(), R.near_voxels(c["P"], c["origin"], c["step"], c["count"]))


def test_a_voxel_whose_centre_is_exactly_near_away_is_left_out():
    from sapcu_amd import pointing
    P = np.array([[0.0, 0.0, 0.0]], np.float32)
    d = np.sqrt(R.dist2(R.centres(-0.5, 0.25, 4), P.astype(np.float64))[:, 0])
    near = float(np.sort(np.unique(d))[1])
    got = pointing.near_voxels(_dev(P), -0.5, 0.25, 4, near).cpu().numpy()
    assert np.array_equal(got, np.flatnonzero(d < near)) and len(got) < np.count_nonzero(d <= near)
    assert np.array_equal(pointing.near_voxels(_dev(P), -0.5, 0.25, 4, np.nextafter(near, 1)).cpu().numpy(), np.flatnonzero(d <= near))


# ------------------------------------------------------------------------------------------------------ sample_fn_pointing
GEOMETRY = dict(origin=-0.5, step=0.125, count=8, sub=3, k=10, band=(0.01, 0.05))
_SHARED = {}


def _tables():
    from sapcu_amd import surface
    if "tables" not in _SHARED:
        _SHARED["tables"] = surface.build_surface_tables([K.octasphere(), K.box()], device=U.dev())
    return _SHARED["tables"]


def _sample(seed, mesh=0, **kw):
    from sapcu_amd import pointing
    gen = torch.Generator(device=U.dev()).manual_seed(seed)
    return pointing.sample_fn_pointing(_tables(), mesh, 5000, gen, **dict(dict(GEOMETRY, pointing_size=700), **kw))


def test_sample_fn_pointing_stays_in_the_band_of_its_own_surface_cloud_and_is_deterministic():
    from sapcu_amd import pointing
    out = _sample(11)
    got = _np(out)
    assert got["surface"].shape == (5000, 3) and got["surface"].dtype == np.float32
    assert got["points"].shape == (700, 3) and got["pointing"].shape == (700, 3) and got["candidate"].shape == (700,)
    assert len(np.unique(got["candidate"])) == 700 and not np.array_equal(got["candidate"], np.sort(got["candidate"]))
    idx, dist, _ = R.neighbours(got["surface"], got["points"], 10)
    assert (dist[:, 0] >= 0.01).all() and (dist[:, 0] <= 0.05).all()
    direction, length = R.pointing(got["surface"], idx, got["points"])
    assert (length > 0).all() and np.array_equal(got["pointing"], direction)
    # the candidates are those of the returned cloud's near voxels
    voxels = R.near_voxels(got["surface"], -0.5, 0.125, 8)
    assert got["candidate"].max() < len(voxels) * 27
    q = R.candidates(voxels, -0.5, 0.125, 8, 3)
    assert np.abs(got["points"] - q[got["candidate"]]).max() <= 0.001 and (got["points"] >= q[got["candidate"]]).all()
    _assert_same(got, _np(_sample(11)), "the same seed")
    assert not np.array_equal(got["points"], _np(_sample(12))["points"])
    whole = _np(_sample(11, pointing_size=10 ** 6))
    assert len(whole["points"]) > 700 and np.isin(got["candidate"], whole["candidate"]).all()
    z = pointing.as_fn_npz(out["points"], out["pointing"])
    assert np.array_equal(z["points"], got["points"]) and np.array_equal(z["normals"], got["pointing"])


# ---------------------------------------------------------------------------------------------------------------- loaders
def _fn_loader(**kw):
    from sapcu_amd import data
    meshes = [K.octasphere(), K.box()] * 5
    return data.FnPointingPatches(meshes, **dict(dict(surface_points=5000, pointing_size=600, cloud_points=256, num_patches=8, k_neighbors=12,
                                                      split="all", batch_size=2, seed=5, device=U.dev(), geometry=GEOMETRY), **kw))


def _fd_loader(**kw):
    from sapcu_amd import data
    meshes = [K.octasphere(), K.box()] * 5
    return data.FdSeedPatches(meshes, **dict(dict(num_rays=512, cloud_points=300, num_patches=5, k_neighbors=24, split="all", batch_size=2,
                                                  seed=5, device=U.dev()), **kw))


def test_fn_pointing_batches_are_the_inference_calls_on_the_drawn_seeds():
    from sapcu_amd import generation
    loader = _fn_loader()
    batch = next(iter(loader))
    d = loader.last_draws
    assert sorted(batch) == ["cloud", "index", "input", "normal"]
    assert batch["input"].shape == (2, 8, 12, 3) and batch["normal"].shape == (2, 8, 3) and batch["cloud"].shape == (2, 256, 3)
    assert all(batch[key].dtype == F32 and batch[key].is_cuda for key in ("input", "normal", "cloud")) and batch["index"].dtype == I64
    assert d["queries"].shape == (2, 8, 3) and d["queries"].dtype == F64
    for e, m in enumerate(batch["index"].tolist()):
        made = loader.mesh_samples(m)
        assert torch.equal(batch["cloud"][e], made["surface"][d["cloud_idx"][e]])
        assert torch.equal(d["queries"][e], made["points"][d["sample_idx"][e]].float().double())
        assert torch.equal(batch["normal"][e], made["pointing"][d["sample_idx"][e]].float())
        _, _, patch = generation.knn_gather(batch["cloud"][e].double(), d["queries"][e].contiguous(), 12)
        assert torch.equal(batch["input"][e], patch)
        want = R.neighbours(batch["cloud"][e].cpu().numpy(), d["queries"][e].cpu().numpy(), 12)[0]
        cloud = batch["cloud"][e].cpu().numpy().astype(np.float64)
        assert np.array_equal(batch["input"][e].cpu().numpy(), (cloud[want] - d["queries"][e].cpu().numpy()[:, None, :]).astype(np.float32))
    # the seeds lie off the surface: every patch row is at least band[0] long, up to the f32 rounding of the seed
    assert float(batch["input"].double().norm(dim=-1).min()) > 0.009


def test_fd_seed_batches_are_the_inference_calls_on_the_drawn_rays():
    from sapcu_amd import generation
    loader = _fd_loader()
    batch = next(iter(loader))
    d = loader.last_draws
    assert sorted(batch) == ["cloud", "index", "input", "len"]
    assert batch["input"].shape == (2, 5, 24, 3) and batch["len"].shape == (2, 5) and batch["cloud"].shape == (2, 300, 3)
    assert all(batch[key].dtype == F32 and batch[key].is_cuda for key in ("input", "len", "cloud"))
    for e in range(2):
        cloud, q = batch["cloud"][e].double(), d["queries"][e].contiguous()
        idx, dist, _ = generation.knn_gather(cloud, q, 24, want_dist=True, want_patch=False)
        assert torch.equal(batch["input"][e], generation.gather_rotate(cloud, q, idx, d["directions"][e].contiguous()))
        # a turn keeps lengths: f32 rows of an f64 rotation, three roundings of 2^-24 relative each
        assert float((batch["input"][e].double().norm(dim=-1) - dist).abs().max()) < 1e-6
    assert bool((batch["len"] >= 0.003).all()) and bool((batch["len"] <= 0.0300001).all())


@pytest.mark.parametrize("make", (_fn_loader, _fd_loader), ids=("fn", "fd"))
def test_the_seed_loaders_are_deterministic_per_seed_epoch_and_batch(make):
    first = [{k: v.clone() for k, v in b.items()} for b in make()]
    again = list(make())
    assert len(first) == 5
    for a, b in zip(first, again):
        assert all(torch.equal(a[k], b[k]) for k in a)
    other = next(iter(make().set_epoch(1)))
    assert not torch.equal(other["input"], first[0]["input"])
    assert not torch.equal(first[0]["input"], first[1]["input"])


def test_resample_remakes_the_pointing_samples():
    loader = _fn_loader()
    a = loader.mesh_samples(0)["points"].clone()
    assert loader.mesh_samples(0)["points"] is loader.mesh_samples(0)["points"]
    b = loader.resample().mesh_samples(0)["points"]
    assert a.shape[1] == 3 and not (a.shape == b.shape and torch.equal(a, b))


def test_an_fn_training_step_on_a_pointing_batch():
    from sapcu_amd import train_step
    from test_gpu_data import _fn_trainer, _params
    loader = _fn_loader(batch_size=2, drop_last=True)
    model, tr = _fn_trainer()
    before = _params(model)
    loss, _ = tr.train_step(next(iter(loader)))
    assert loss is not None and math.isfinite(float(loss)), loss
    assert any(not torch.equal(a, b) for a, b in zip(before, _params(model)))
    assert callable(train_step.run_epoch)


def test_an_fd_training_step_on_a_seed_batch():
    from test_gpu_data import _fd_trainer, _params
    batch = next(iter(_fd_loader()))
    model, tr = _fd_trainer()
    before = _params(model)
    loss, _ = tr.train_step(batch)
    assert loss is not None and math.isfinite(float(loss)), loss
    assert any(not torch.equal(a, b) for a, b in zip(before, _params(model)))
