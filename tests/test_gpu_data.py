"""Training samples built on the device (-m gpu; include/sapcu_data.h, csrc/train_patches.hip, sapcu_amd/data.py).

Every output of ``sapcu_train_patches_f32`` must equal tests/data_ref.py — the numpy restatement that tests/test_data_host.py pins
bit for bit to the reference's dataset classes — with ``==``: there is no tolerance anywhere in this file.  Shapes are the two the
trainers use and the smallest at which a path changes (a ragged last 64-point slab, k = n, the two-slot k-list, one dense point,
several dense tiles, n = 4096 once), clouds with many exact distance ties (the (distance, index) rule decides), and a cloud of radius
0.  Then the reference fixture itself, the memory contract of DESIGN section 2 under guard bands, every refusal, the two loaders and
one training step of each network on a loader's batch."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import data_ref as R
import gpu_utils as U
from conftest import golden
from guarded import Arena
from test_data_host import FD_K, FN_K, ROTATION_ULPS, _case, header_entry_points, rotation_products

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
f32 = np.float32
INPUTS = ("clouds", "dense", "normals", "sidx", "rot", "scale", "jitter", "centres")
OUTPUTS = ("patches", "idx", "cloud", "dense_out", "len", "normals_out", "patch_normals")
REF_KEY = {"patches": "patches", "idx": "idx", "cloud": "cloud", "dense_out": "dense", "len": "len", "normals_out": "normals",
           "patch_normals": "patch_normals"}
PY_KEY = {"patches": "patches", "idx": "idx", "cloud": "cloud", "dense": "dense", "len": "len", "normals": "normals",
          "patch_normals": "patch_normals"}


# ------------------------------------------------------------------------------------------------------------ the cases
def _rotations(rng, b):
    """Full 3-D rotations (the kernel takes any matrix; the loaders pass rotations about z)."""
    q, _ = np.linalg.qr(rng.normal(size=(b, 3, 3)))
    return q.astype(f32)


def _make_case(name):
    """dict of numpy inputs: clouds [S,n,3], dense / normals or None, sidx [b], rot / scale / jitter or None, centres or None, k."""
    rng = np.random.default_rng(sum(map(ord, name)))
    shapes = {  # S, n, g, normals, b, pc (0 = all points), k, augmented
        "fd": (6, 256, 1024, False, 4, 0, 32, True),
        "fn": (5, 512, 0, True, 4, 64, 12, True),
        "n100-k100": (3, 100, 300, True, 3, 0, 100, True),
        "k1": (3, 70, 50, False, 2, 0, 1, True),
        "g1": (2, 64, 1, False, 2, 0, 8, False),
        "k65-n129": (2, 129, 2500, True, 2, 40, 65, True),
        "n4096": (1, 4096, 4096, False, 1, 256, 128, True),
        "b1": (3, 80, 90, True, 1, 0, 16, True),
        "b17": (3, 80, 90, True, 17, 10, 16, True),
        "n1": (2, 1, 3, True, 2, 0, 1, True),
        # the edges of the neighbour kernel's slot switch: the first slab alone, the largest one-slot list with insertions, both slots full
        "k64-n64": (2, 64, 0, False, 2, 0, 64, False),
        "k64-n130": (2, 130, 0, False, 2, 0, 64, True),
        "k128-n128": (2, 128, 0, False, 2, 0, 128, False),
        "k128-n193": (2, 193, 0, False, 2, 0, 128, True),
    }
    if name in shapes:
        S, n, g, nrm, b, pc, k, aug = shapes[name]
        c = {"clouds": (rng.normal(size=(S, n, 3)) * 0.4 + [0.5, -1.0, 2.0]).astype(f32),
             "dense": (rng.normal(size=(S, g, 3)) * 0.4 + [0.5, -1.0, 2.0]).astype(f32) if g else None,
             "normals": rng.normal(size=(S, n, 3)).astype(f32) if nrm else None,
             "sidx": rng.integers(0, S, size=b).astype(np.int64),
             "rot": _rotations(rng, b) if aug else None, "scale": rng.uniform(0.8, 1.2, size=b).astype(f32) if aug else None,
             "jitter": (rng.normal(size=(b, n, 3)) * 0.002).astype(f32) if aug else None,
             "centres": rng.integers(0, n, size=(b, pc)).astype(np.int32) if pc else None, "k": k}
        return c
    if name in ("lattice", "lattice-k64"):                     # a shuffled 7^3 integer lattice: every distance is tied many times
                                                               # (-k64: ties at the one-slot list's last entry)
        grid = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32)
        clouds = np.stack([grid[rng.permutation(343)] for _ in range(2)])
        dense = np.stack([(grid[rng.permutation(343)][:200] + 0.5).astype(f32) for _ in range(2)])
        return {"clouds": clouds, "dense": dense, "normals": None, "sidx": np.array([1, 0], np.int64), "rot": None, "scale": None,
                "jitter": None, "centres": None, "k": 64 if name == "lattice-k64" else 100}
    if name == "duplicates":                                   # every point four times, shuffled: the lower index must come first
        base = rng.normal(size=(2, 50, 3)).astype(f32)
        clouds = np.stack([np.tile(base[s], (4, 1))[rng.permutation(200)] for s in range(2)])
        return {"clouds": clouds, "dense": base.copy(), "normals": None, "sidx": np.array([0, 1, 1], np.int64), "rot": None,
                "scale": np.array([1.0, 0.5, 2.0], f32), "jitter": None, "centres": None, "k": 32}
    if name == "identical":                                    # radius 0: no division, no NaN; one zero normal: 0 / (0 + 1e-8)
        clouds = np.tile(np.array([[0.25, -3.0, 7.5]], f32), (2, 90, 1))
        normals = rng.normal(size=(2, 90, 3)).astype(f32)
        normals[0, 5] = 0
        return {"clouds": clouds, "dense": rng.normal(size=(2, 30, 3)).astype(f32), "normals": normals, "sidx": np.array([0, 1], np.int64),
                "rot": None, "scale": None, "jitter": None, "centres": None, "k": 70}
    if name == "repeats":                                      # one sample three times with different draws; one centre many times
        c = _make_case("b1")
        b = 4
        c.update(sidx=np.array([2, 2, 0, 2], np.int64), rot=_rotations(rng, b), scale=rng.uniform(0.8, 1.2, size=b).astype(f32),
                 jitter=(rng.normal(size=(b, 80, 3)) * 0.002).astype(f32),
                 centres=np.array([[7, 7, 7, 3, 7, 79, 0, 0, 3]] * b, np.int32))
        return c
    raise KeyError(name)


CASES = ["fd", "fn", "n100-k100", "k1", "g1", "k65-n129", "n4096", "lattice", "duplicates", "identical", "repeats", "b1", "b17", "n1",
         "k64-n64", "k64-n130", "k128-n128", "k128-n193", "lattice-k64"]
_CACHE = {}


def _case_and_reference(name):
    """(inputs, data_ref's outputs), computed once and shared by the tests that need them; nobody writes to them."""
    if name not in _CACHE:
        c = _make_case(name)
        _CACHE[name] = (c, R.batch(c["clouds"], c["sidx"], c["k"], c["dense"], c["normals"], c["rot"], c["scale"], c["jitter"], c["centres"]))
    return _CACHE[name]


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(U.dev())


def _build(c, **kw):
    from sapcu_amd import data
    out = data.build_patches(_dev(c["clouds"]), _dev(c["sidx"]), c["k"], dense=_dev(c["dense"]), normals=_dev(c["normals"]),
                             rotation=_dev(c["rot"]), scale=_dev(c["scale"]), jitter=_dev(c["jitter"]), centres=_dev(c["centres"]), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_outputs_equal(got, ref, keys, what):
    for gk, rk in keys.items():
        if ref[rk] is None:
            assert gk not in got or got[gk] is None, (what, gk)
            continue
        g, r = got[gk], ref[rk]
        assert g.dtype == r.dtype and g.shape == r.shape, (what, gk, g.dtype, g.shape, r.dtype, r.shape)
        assert not np.isnan(g).any(), "%s: NaN in %s" % (what, gk)
        bad = g != r
        assert not bad.any(), "%s: %s differs in %d of %d elements, first at %s: %r against %r" % (
            what, gk, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), g[bad][0], r[bad][0])


@pytest.mark.parametrize("name", CASES)
def test_every_output_equals_the_numpy_restatement(name):
    c, ref = _case_and_reference(name)
    got = _build(c)
    _assert_outputs_equal(got, ref, PY_KEY, name)
    assert (got["patches"] == got["cloud"][np.arange(len(c["sidx"]))[:, None, None], got["idx"]]).all()
    if name == "identical":
        assert (got["cloud"] == 0).all() and (got["len"] > 0).all() and (got["normals"][0, 5] == 0).all()
        assert (got["idx"] == np.arange(70)).all()             # all distances 0: ascending index
    if name in ("lattice", "lattice-k64", "duplicates"):       # the case is what it claims: ties inside the first k + 1 distances
        cloud = ref["cloud"][0]
        _, d = R.neighbours(cloud, np.arange(len(cloud)), c["k"] + 1, want_dist=True)
        assert (np.diff(d, axis=1) == 0).any(axis=1).all()


def test_k_is_clamped_to_the_cloud_as_the_reference_does():
    c, ref = _case_and_reference("n100-k100")
    got = _build(dict(c, k=128))                               # min(128, 100)
    _assert_outputs_equal(got, ref, PY_KEY, "k clamped")
    assert got["patches"].shape == (3, 100, 100, 3)


# ------------------------------------------------------------------------------------------------------- the C entry point
def _lib():
    from sapcu_amd import _lib
    return _lib


def _buffers(arena, c, odd=False):
    """The call's buffers in `arena` (guarded or compact); with `odd`, every base address is an odd multiple of its element size
    away from the 512-byte boundary the allocator gives."""
    b, n, S = len(c["sidx"]), c["clouds"].shape[1], c["clouds"].shape[0]
    g = 0 if c["dense"] is None else c["dense"].shape[1]
    pc = n if c["centres"] is None else c["centres"].shape[1]
    k = c["k"]
    off = iter(range(1, 99, 2))
    nxt = (lambda esize: esize * next(off)) if odd else (lambda esize: 0)
    bufs = {"n": n, "S": S, "g": g, "pc": pc, "k": k, "b": b}
    for name in INPUTS:
        a = c[name]
        bufs[name] = None if a is None else arena.inp(a, offset=nxt(a.dtype.itemsize), name=name)
    shapes = {"patches": ((b, pc, k, 3), F32), "idx": ((b, pc, k), I32), "cloud": ((b, n, 3), F32), "dense_out": ((b, g, 3), F32),
              "len": ((b, n), F32), "normals_out": ((b, n, 3), F32), "patch_normals": ((b, pc, 3), F32)}
    for name, (shape, dtype) in shapes.items():
        needs = c["dense"] if name in ("dense_out", "len") else c["normals"] if name in ("normals_out", "patch_normals") else 1
        bufs[name] = None if needs is None else arena.out(shape, dtype, offset=nxt(4), name=name)
    bufs["nbytes"] = int(_lib().load().sapcu_train_patches_workspace_bytes(b))
    bufs["ws"] = arena.ws(bufs["nbytes"], offset=nxt(4), name="workspace")
    return bufs


def _launch(bufs, **over):
    L = _lib()
    a = {k: (L.ptr(v) if torch.is_tensor(v) else v) for k, v in bufs.items()}
    a.update(over)
    rc = L.load().sapcu_train_patches_f32(a["clouds"], a["S"], a["n"], a["dense"], a["g"], a["normals"], a["sidx"], a["b"], a["rot"],
                                          a["scale"], a["jitter"], a["centres"], a["pc"], a["k"], a["patches"], a["idx"], a["cloud"],
                                          a["dense_out"], a["len"], a["normals_out"], a["patch_normals"], a["ws"], a["nbytes"],
                                          L.current_stream())
    torch.cuda.synchronize()
    return rc


def _outputs(bufs):
    return {name: (None if bufs[name] is None else bufs[name].cpu().numpy()) for name in OUTPUTS}


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


@pytest.mark.parametrize("name", ["n100-k100", "repeats"])
def test_every_optional_output_null_in_turn(name):
    """A NULL optional output changes nothing in the others, and the buffer that was not passed is not written."""
    c, ref = _case_and_reference(name)
    for drop in ("idx", "dense_out", "len", "normals_out", "patch_normals", ("dense_out", "len"), ("normals_out", "patch_normals"),
                 ("idx", "dense_out", "len", "normals_out", "patch_normals")):
        drop = (drop,) if isinstance(drop, str) else drop
        if any(_case_and_reference(name)[1][REF_KEY[d]] is None for d in drop):
            continue
        bufs = _buffers(Arena("compact", device=U.dev()), c)
        assert _launch(bufs, **{d: None for d in drop}) == 0, _lib().load().sapcu_last_error()
        got = _outputs(bufs)
        _assert_outputs_equal({k: v for k, v in got.items() if k not in drop}, ref, {k: v for k, v in REF_KEY.items() if k not in drop},
                              "%s without %s" % (name, "+".join(drop)))
        for d in drop:
            assert _untouched(bufs[d]), (name, d)


def test_optional_inputs_null_in_turn():
    """Each augmentation part alone, and dense / normals left out with their outputs."""
    c, _ = _case_and_reference("n100-k100")
    for keep in ("rot", "scale", "jitter"):
        cc = dict(c, **{p: None for p in ("rot", "scale", "jitter") if p != keep})
        _assert_outputs_equal(_build(cc), R.batch(cc["clouds"], cc["sidx"], cc["k"], cc["dense"], cc["normals"], cc["rot"], cc["scale"],
                                                  cc["jitter"], cc["centres"]), PY_KEY, "only " + keep)
    for gone in ("dense", "normals"):
        cc = dict(c, **{gone: None})
        got = _build(cc)
        assert ("len" in got) == (gone != "dense") and ("normals" in got) == (gone != "normals")
        _assert_outputs_equal(got, R.batch(cc["clouds"], cc["sidx"], cc["k"], cc["dense"], cc["normals"], cc["rot"], cc["scale"],
                                           cc["jitter"], cc["centres"]), PY_KEY, "without " + gone)


GUARD_CASES = ["fd", "fn", "n100-k100", "k65-n129", "g1", "b17", "n1"]


@pytest.mark.parametrize("name", GUARD_CASES)
def test_memory_contract_under_guard_bands(name):
    """The three runs of DESIGN section 2: 0xFF bands and workspace with NaN-prefilled outputs, 0x00 bands and workspace, the dirty
    workspace again — guards intact, every output written in full and bit-identical across the runs and equal to data_ref; every
    base address odd."""
    c, ref = _case_and_reference(name)
    results = []
    for fill in (0xFF, 0x00):
        arena = Arena("guard", fill=fill, device=U.dev())
        bufs = _buffers(arena, c, odd=True)
        for again in range(2 if fill == 0x00 else 1):
            arena.refill_outputs()
            assert _launch(bufs) == 0, _lib().load().sapcu_last_error()
            arena.check()
            results.append(_outputs(bufs))
    for got in results:
        _assert_outputs_equal(got, ref, REF_KEY, name)           # no NaN left: written in full
    for got in results[1:]:
        for key in OUTPUTS:
            if got[key] is not None:
                assert np.array_equal(got[key].view(np.int32), results[0][key].view(np.int32)), (name, key)


def test_refusals_launch_nothing():
    """Every refusal of include/sapcu_data.h returns SAPCU_ERR_ARG and leaves the 0xFF-prefilled outputs, the workspace and the
    guards alone; the same buffers are then accepted as they are."""
    c, ref = _case_and_reference("n100-k100")
    arena = Arena("guard", fill=0xFF, device=U.dev())
    bufs = _buffers(arena, c)
    wsp = bufs["ws"].data_ptr()
    refusals = [dict(n=0), dict(n=4097), dict(g=-1), dict(g=65537), dict(k=0), dict(k=101), dict(k=129), dict(pc=0), dict(pc=99),
                dict(S=0), dict(b=-1), dict(b=(1 << 20) + 1), dict(dense=None), dict(g=0), dict(dense=None, g=0),
                dict(dense=None, g=0, dense_out=None), dict(dense=None, g=0, len=None), dict(normals=None),
                dict(normals=None, normals_out=None), dict(normals=None, patch_normals=None), dict(clouds=None), dict(sidx=None),
                dict(patches=None), dict(cloud=None), dict(ws=None), dict(nbytes=bufs["nbytes"] - 1), dict(nbytes=0),
                dict(ws=ctypes.c_void_p(wsp + 2))]
    for over in refusals:
        assert _launch(bufs, **over) == -1, over
        assert _lib().load().sapcu_last_error()
        arena.check()
        for name in OUTPUTS:
            assert _untouched(bufs[name]), (over, name)
        assert _untouched(bufs["ws"]), over
    assert _launch(bufs, b=0) == 0                               # no entry: nothing is launched, nothing is written
    assert all(_untouched(bufs[name]) for name in OUTPUTS)
    assert _launch(bufs) == 0
    arena.check()
    _assert_outputs_equal(_outputs(bufs), ref, REF_KEY, "after the refusals")


def test_index_values_are_refused_by_the_python_layer_and_harmless_in_the_kernels():
    """The documented split (include/sapcu_data.h): build_patches validates index VALUES and raises ValueError; the entry point does
    not read device memory on the host, and its kernels skip a bad sample's entry and a bad centre's rows — nothing is read or
    written out of bounds (guards), the other rows are right, the skipped rows keep their 0xFF."""
    c, ref = _case_and_reference("repeats")
    S, n = c["clouds"].shape[:2]
    for bad in (S, -1, 1 << 40):
        with pytest.raises(ValueError):
            _build(dict(c, sidx=np.array([2, bad, 0, 2], np.int64)))
    for bad in (n, -1, 1 << 30):
        cen = c["centres"].copy()
        cen[1, 4] = bad
        with pytest.raises(ValueError):
            _build(dict(c, centres=cen))
    cen = c["centres"].copy()
    cen[0, 2], cen[3, 8] = n, -5
    cc = dict(c, sidx=np.array([2, S + 3, 0, 2], np.int64), centres=cen)
    arena = Arena("guard", fill=0xFF, device=U.dev())
    bufs = _buffers(arena, cc, odd=True)
    assert _launch(bufs) == 0
    arena.check()
    got = _outputs(bufs)
    for key in OUTPUTS:
        assert _untouched(bufs[key][1]), key                     # the entry of the bad sample index
        per_centre = key in ("patches", "idx", "patch_normals")
        for e in (0, 2, 3):
            g, r = got[key][e], ref[REF_KEY[key]][e]
            if per_centre:
                skip = {0: 2, 3: 8}.get(e)
                rows = [i for i in range(g.shape[0]) if i != skip]
                assert (g[rows] == r[rows]).all(), (key, e)
                if skip is not None:
                    assert _untouched(bufs[key][e, skip]), (key, e)
            else:
                assert (g == r).all(), (key, e)


def test_every_pointer_taking_entry_point_of_the_header_runs_under_guards():
    decl = header_entry_points()
    assert set(decl) == set(_lib().DATA_EXPORTS)
    assert {n for n in decl if "*" in decl[n]} == {"sapcu_train_patches_f32"}        # _buffers / _launch above
    assert {n for n in decl if n.endswith("workspace_bytes")} == {"sapcu_train_patches_workspace_bytes"}


# ---------------------------------------------------------------------------------------------------- the reference fixture
def _fd_inputs(cloud, dense, rot=None, scale=None, jitter=None):
    one = lambda a: None if a is None else np.asarray(a, f32)[None]
    return {"clouds": one(cloud), "dense": one(dense), "normals": None, "sidx": np.zeros(1, np.int64), "rot": one(rot),
            "scale": None if scale is None else np.array([scale], f32), "jitter": one(jitter), "centres": None, "k": FD_K}


def _fn_inputs(cloud, normals, centres, rot=None, scale=None, jitter=None):
    c = _fd_inputs(cloud, None, rot, scale, jitter)
    c.update(normals=np.asarray(normals, f32)[None], centres=np.asarray(centres, np.int32)[None], k=FN_K)
    return c


def _assert_fixture(got, c, fd, what):
    pairs = (("cloud", "cloud"), ("points", "dense"), ("len", "len"), ("idx", "idx")) if fd else \
        (("cloud", "cloud"), ("all_normals", "normals"), ("normal", "patch_normals"), ("idx", "idx"))
    for key, out in pairs:
        g, r = got[out][0], c[key]
        assert g.dtype == r.dtype and g.shape == r.shape and (g == r).all(), "%s: %s differs from the reference's in %d elements" % (
            what, key, int((g != r).sum()))
    assert (got["patches"][0] == c["cloud"][c["idx"]]).all(), what


def test_unaugmented_samples_equal_the_reference():
    g = golden("train_data.npz")
    for name in ("fd_val0", "fd_val1"):
        c = _case(g, name)
        _assert_fixture(_build(_fd_inputs(c["input_raw"], c["dense_raw"])), c, True, name)
    c = _case(g, "fn_val")
    _assert_fixture(_build(_fn_inputs(c["points_raw"], c["normals_raw"], c["centres"])), c, False, "fn_val")


def test_augmented_samples_equal_the_reference_from_its_augmented_cloud():
    """Teacher-forced on the reference's own augmented arrays: every later stage equals the reference bit for bit."""
    g = golden("train_data.npz")
    for name in ("fd_train0", "fd_train1"):
        c = _case(g, name)
        _assert_fixture(_build(_fd_inputs(c["aug_cloud"], c["aug_dense"])), c, True, name)
    c = _case(g, "fn_train")
    _assert_fixture(_build(_fn_inputs(c["aug_cloud"], c["aug_normals"], c["centres"])), c, False, "fn_train")


@pytest.mark.parametrize("name", ["fd_train0", "fd_train1", "fn_train"])
def test_the_augmentation_stage_on_the_recorded_draws(name):
    """Rotation, scale and jitter with the reference's own draws: the device equals data_ref's plain-order product (==, every
    output), and that product is within ROTATION_ULPS of the reference's recorded BLAS product — the bound measured on the fixture
    on a CPU (1 ulp) plus one, in the unit data_ref.rotation_ulps names; it is not fitted to the device."""
    c = _case(golden("train_data.npz"), name)
    scale = np.float32(c["scale"])
    if name.startswith("fd"):
        inp = _fd_inputs(c["input_raw"], c["dense_raw"], c["rot"], scale, c["jitter"])
    else:
        inp = _fn_inputs(c["points_raw"], c["normals_raw"], c["centres"], c["rot"], scale, c["jitter"])
    ref = R.batch(inp["clouds"], inp["sidx"], inp["k"], inp["dense"], inp["normals"], inp["rot"], inp["scale"], inp["jitter"], inp["centres"])
    _assert_outputs_equal(_build(inp), ref, PY_KEY, name)
    for raw, product in rotation_products(c, name):
        ulps = R.rotation_ulps(raw, c["rot"], product)
        print("%s: plain-order rotation against the reference's product: %g ulp" % (name, ulps))
        assert ulps <= ROTATION_ULPS


# ------------------------------------------------------------------------------------------------------------- the loaders
def _pairs(S=20, n=64, g=200, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(S, n, 3)) * 0.3 + 1).astype(f32), (rng.normal(size=(S, g, 3)) * 0.3 + 1).astype(f32)


def _same_batches(a, b):
    return len(a) == len(b) and all(x.keys() == y.keys() and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


def test_pu1k_loader_batches_splits_and_determinism():
    from sapcu_amd import data
    inputs, dense = _pairs()
    make = lambda **kw: data.PU1KPatches(inputs, dense, k_neighbors=24, batch_size=4, seed=5, device=U.dev(), **kw)
    train, val = make(), make(split="val")
    assert train.samples == 18 and val.samples == 2 and len(train) == 5 and len(val) == 1 and train.augment and not val.augment
    assert len(make(drop_last=True)) == 4
    first = list(train)
    assert [b["input"].shape[0] for b in first] == [4, 4, 4, 4, 2]
    b0 = first[0]
    assert b0["input"].shape == (4, 64, 24, 3) and b0["len"].shape == (4, 64) and b0["cloud"].shape == (4, 64, 3)
    assert b0["points"].shape == (4, 200, 3) and all(b0[k].dtype == F32 and b0[k].is_cuda for k in ("input", "len", "cloud", "points"))
    assert sorted(torch.cat([b["index"] for b in first]).tolist()) == list(range(18))           # every sample once per epoch
    assert _same_batches(first, list(make()))                    # the same (seed, epoch): bit-identical
    assert _same_batches(first, list(train))                     # and again from the same object
    other = list(train.set_epoch(1))
    assert not _same_batches(first, other) and _same_batches(other, list(make().set_epoch(1)))
    assert not _same_batches(first, list(data.PU1KPatches(inputs, dense, k_neighbors=24, batch_size=4, seed=6, device=U.dev())))
    # the draws of the last batch are inside their ranges, and the batch is data_ref's on them
    train.set_epoch(0)
    for batch in train:
        d = train.last_draws
        theta, scale, jit, rot = d["theta"].cpu().numpy(), d["scale"].cpu().numpy(), d["jitter"].cpu().numpy(), d["rotation"].cpu().numpy()
        assert ((theta >= 0) & (theta < 2 * np.pi)).all() and ((scale >= 0.8) & (scale <= 1.2)).all()
        assert np.abs(jit).max() < 8 * 0.002 and 0.5 < jit.std() / 0.002 < 1.5
        assert (rot[:, 2, 2] == 1).all() and (rot[:, 2, :2] == 0).all() and (rot[:, :2, 2] == 0).all()
        # (two f64 cosines of the same angle may differ in their last place, so their f32 roundings by one f32 ulp below 1)
        assert np.abs(rot[:, 0, 0] - np.cos(theta)).max() <= 2.0 ** -23 and np.abs(rot[:, 1, 0] - np.sin(theta)).max() <= 2.0 ** -23
        assert (rot[:, 0, 1] == -rot[:, 1, 0]).all() and (rot[:, 1, 1] == rot[:, 0, 0]).all()
    idx = batch["index"].cpu().numpy()
    ref = R.batch(inputs[:18], idx, 24, dense[:18], None, rot, scale, jit)
    _assert_outputs_equal({"input": batch["input"].cpu().numpy(), "len": batch["len"].cpu().numpy(), "cloud": batch["cloud"].cpu().numpy(),
                           "points": batch["points"].cpu().numpy()}, ref, {"input": "patches", "len": "len", "cloud": "cloud", "points": "dense"},
                          "last train batch")
    # the val split is never augmented: the last tenth of the samples, exactly data_ref on the raw pair
    for epoch in (0, 3):
        (vb,) = list(val.set_epoch(epoch))
        assert val.last_draws == {"theta": None, "rotation": None, "scale": None, "jitter": None}
        vi = vb["index"].cpu().numpy()
        assert sorted(vi.tolist()) == [0, 1]
        ref = R.batch(inputs[18:], vi, 24, dense[18:])
        _assert_outputs_equal({"input": vb["input"].cpu().numpy(), "len": vb["len"].cpu().numpy(), "cloud": vb["cloud"].cpu().numpy(),
                               "points": vb["points"].cpu().numpy()}, ref, {"input": "patches", "len": "len", "cloud": "cloud", "points": "dense"},
                              "val batch")
    assert make(split="val", augment=True).augment and not make(augment=False).augment
    assert data.PU1KPatches(inputs[:, :20], dense, k_neighbors=32, batch_size=2, device=U.dev()).__iter__().__next__()["input"].shape == (2, 20, 20, 3)


def test_pu1k_loader_reads_the_reference_keys_from_files(tmp_path):
    from sapcu_amd import data
    inputs, dense = _pairs(S=10)
    path = str(tmp_path / "pairs.npz")
    np.savez(path, poisson_256=inputs, poisson_1024=dense)
    np.save(str(tmp_path / "in.npy"), inputs)
    kw = dict(split="all", k_neighbors=8, batch_size=5, shuffle=False, augment=False, device=U.dev())
    a = list(data.PU1KPatches(path, path, **kw))
    assert _same_batches(a, list(data.PU1KPatches(inputs, torch.from_numpy(dense), **kw)))
    assert _same_batches(a, list(data.PU1KPatches(str(tmp_path / "in.npy"), torch.from_numpy(dense).to(U.dev()).double(), **kw)))
    assert torch.cat([b["index"] for b in a]).tolist() == list(range(10))


def test_mesh_loader_centres_and_batches():
    from sapcu_amd import data
    rng = np.random.default_rng(9)
    points, normals = (rng.normal(size=(10, 128, 3)) * 0.3).astype(f32), rng.normal(size=(10, 128, 3)).astype(f32)
    make = lambda **kw: data.MeshPatches(points, normals, num_patches=16, k_neighbors=12, batch_size=4, seed=2, device=U.dev(), **kw)
    train = make()
    first = list(train)
    assert [b["input"].shape for b in first] == [(4, 16, 12, 3), (4, 16, 12, 3), (1, 16, 12, 3)] and train.samples == 9
    assert _same_batches(first, list(make())) and not _same_batches(first, list(make().set_epoch(2)))
    seen = set()
    for batch in train:
        d = train.last_draws
        cen = batch["centres"].cpu().numpy()
        assert cen.dtype == np.int32 and ((cen >= 0) & (cen < 128)).all() and all(len(set(row.tolist())) == 16 for row in cen)
        seen.update(cen.reshape(-1).tolist())
        idx = batch["index"].cpu().numpy()
        ref = R.batch(points[:9], idx, 12, None, normals[:9], d["rotation"].cpu().numpy(), d["scale"].cpu().numpy(),
                      d["jitter"].cpu().numpy(), cen)
        got = {k: batch[k].cpu().numpy() for k in ("input", "normal", "cloud", "all_normals")}
        _assert_outputs_equal(got, ref, {"input": "patches", "normal": "patch_normals", "cloud": "cloud", "all_normals": "normals"}, "mesh batch")
    assert len(seen) > 64                                        # the centres are a fresh choice per sample
    (vb,) = list(make(split="val"))
    assert train.augment and vb["input"].shape == (1, 16, 12, 3)
    # n <= num_patches: every point is a centre, in order
    few = data.MeshPatches(points[:, :16], normals[:, :16], num_patches=16, k_neighbors=12, batch_size=3, split="all", device=U.dev())
    batch = next(iter(few))
    assert batch["input"].shape == (3, 16, 12, 3) and (batch["centres"].cpu().numpy() == np.arange(16)).all()
    assert few.last_draws["centres"] is None


# -------------------------------------------------------------------------------------------------------- into the trainers
FD_KW = dict(k=8, emb_dims=64, time_steps_enc=3, num_heads=4, k_scales=[4, 8, 16])
FN_MODEL_KW = dict(k_values=[24, 18, 12], emb_dims=640, time_steps_enc=4, time_steps_dec=12, num_heads=8, use_snn_decoder=False,
                   decoder_dropout=0.1)


def _fd_trainer():
    import sapcu_amd
    from sapcu_amd import fd_trainer
    torch.manual_seed(0)
    model = sapcu_amd.TrainableSNNDistanceEstimation(dropout=0.0, **FD_KW).to(U.dev())
    model.dropout_generator = torch.Generator(device=U.dev()).manual_seed(7)
    opt = torch.optim.AdamW(model.parameters(), lr=3e-3, capturable=True)
    return model, fd_trainer.Trainer(model, opt, device=U.dev(), grad_clip=0.1)


_FN_SD = {}


def _fn_trainer():
    import sapcu_amd
    from sapcu_amd import fn_trainer, testing as T
    if not _FN_SD:
        _FN_SD["sd"] = T.training_state_dict(sapcu_amd.ImprovedSNNNormalEstimation(**FN_MODEL_KW).state_dict(), 0)
    model = sapcu_amd.ImprovedSNNNormalEstimation(**FN_MODEL_KW)
    model.load_state_dict(copy.deepcopy(_FN_SD["sd"]), strict=True)
    model.attn_dropout = model.decoder_dropout = 0.0
    model.to(U.dev())
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4, capturable=True)
    return model, fn_trainer.Trainer(model, opt, device=U.dev(), grad_clip=0.15, grad_clip_type="norm")


def _params(model):
    return [p.detach().clone() for p in model.parameters()]


def _one_step_twice_and_a_replay(make_trainer, batch, graph_cls):
    import math
    runs = []
    for _ in range(2):
        model, tr = make_trainer()
        loss, parts = tr.train_step(batch)
        assert loss is not None and math.isfinite(float(loss)), loss
        runs.append((float(loss), _params(model)))
    assert runs[0][0] == runs[1][0] and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    model, tr = make_trainer()
    step = graph_cls(tr, batch, warmup=0)
    loss, _ = step.train_step(batch)
    assert step.replays == 1 and step.eager_fallbacks == 0 and loss is not None and math.isfinite(float(loss))
    assert float(loss) == runs[0][0] and all(torch.equal(a, b) for a, b in zip(_params(model), runs[0][1]))


def test_an_fd_training_step_on_a_loader_batch():
    from sapcu_amd import data, fd_trainer, train_step
    inputs, dense = _pairs(S=20, n=64, g=200, seed=4)
    loader = data.PU1KPatches(inputs, dense, k_neighbors=24, batch_size=2, seed=1, device=U.dev())
    batch = next(iter(loader))
    assert batch["input"].shape == (2, 64, 24, 3)
    _one_step_twice_and_a_replay(_fd_trainer, batch, fd_trainer.GraphedTrainStep)
    # and the loader drives run_epoch unchanged
    model, tr = _fd_trainer()
    short = data.PU1KPatches(inputs[:5], dense[:5], k_neighbors=24, batch_size=2, seed=1, device=U.dev())       # 4 training samples
    it, losses, stats = train_step.run_epoch(tr, short, clamp_parameters=True)
    assert it == 2 and len(losses) == 2 and stats["clouds"] == 4 and stats["skipped"] == 0 and np.isfinite(losses).all()


def test_an_fn_training_step_on_a_loader_batch():
    from sapcu_amd import data, fn_trainer
    rng = np.random.default_rng(12)
    u, v = rng.uniform(0, 2 * np.pi, (10, 128)), rng.uniform(-1, 1, (10, 128))
    normals = np.stack([np.sqrt(1 - v * v) * np.cos(u), np.sqrt(1 - v * v) * np.sin(u), v], -1).astype(f32)   # a sphere: normal = point
    loader = data.MeshPatches(normals * f32(0.5), normals, num_patches=16, k_neighbors=12, batch_size=2, seed=3, device=U.dev())
    batch = next(iter(loader))
    assert batch["input"].shape == (2, 16, 12, 3) and batch["normal"].shape == (2, 16, 3)
    _one_step_twice_and_a_replay(_fn_trainer, batch, fn_trainer.GraphedTrainStep)
