"""Training-sample construction without a GPU: the binding's seventh table against include/sapcu_data.h, the numpy restatement
(tests/data_ref.py) against what the reference's dataset classes returned (tests/golden/train_data.npz) bit for bit, the fixture's
tie-freeness, the split arithmetic, the clamp of k, the argument errors that need no device, and the refusals of the C entry point
that come before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import data_ref as R
import abi_tables
from conftest import ROOT, golden

FD_CASES = ("fd_val0", "fd_val1", "fd_train0", "fd_train1")
FN_CASES = ("fn_val", "fn_train")
FD_K, FN_K = 32, 12
ROTATION_ULPS = 2          # the plain-order rotation against the reference's BLAS product: 1 ulp measured on this fixture, plus one
                           # (the unit: data_ref.rotation_ulps)


def header_entry_points():
    """{name: argument list} of include/sapcu_data.h."""
    return abi_tables.header_entry_points("sapcu_data.h")


def test_the_header_declares_exactly_the_seventh_table():
    from sapcu_amd import _lib
    decl = header_entry_points()
    assert set(decl) == set(_lib.DATA_EXPORTS) == {"sapcu_train_patches_workspace_bytes", "sapcu_train_patches_f32"}
    for other in (_lib.EXPORTS, _lib.SEEDS_EXPORTS, _lib.FD_TRAIN_EXPORTS, _lib.FD_EDGECONV_EXPORTS, _lib.TRAIN_STEP_EXPORTS,
                  _lib.METRICS_EXPORTS):
        assert not set(other) & set(_lib.DATA_EXPORTS)
    lib = _lib.load()
    for name in _lib.DATA_EXPORTS:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len([a for a in decl[name].split(",") if a.strip()]), name
    with open(os.path.join(ROOT, "include", "sapcu.h")) as f:
        assert "sapcu_train_patches" not in f.read() and _lib.ABI_VERSION == 2


def c_call(lib, **over):
    """sapcu_train_patches_f32 on pointers that are never dereferenced (every refusal comes before the first HIP call)."""
    P = ctypes.c_void_p
    a = dict(clouds=P(0x10000), S=10, n=256, dense=P(0x20000), g=1024, normals=P(0x30000), sidx=P(0x40000), b=4, rot=P(0x50000),
             scale=P(0x60000), jitter=P(0x70000), centres=P(0x80000), pc=64, k=32, patches=P(0x90000), idx=P(0xa0000), cloud=P(0xb0000),
             dense_out=P(0xc0000), len=P(0xd0000), normals_out=P(0xe0000), pn=P(0xf0000), ws=P(0x100000), nbytes=64)
    a.update(over)
    return lib.sapcu_train_patches_f32(a["clouds"], a["S"], a["n"], a["dense"], a["g"], a["normals"], a["sidx"], a["b"], a["rot"],
                                       a["scale"], a["jitter"], a["centres"], a["pc"], a["k"], a["patches"], a["idx"], a["cloud"],
                                       a["dense_out"], a["len"], a["normals_out"], a["pn"], a["ws"], a["nbytes"], None)


REFUSALS = [dict(n=0), dict(n=4097), dict(g=-1), dict(g=65537), dict(k=0), dict(k=129, n=200), dict(k=257), dict(k=33, n=32), dict(pc=0),
            dict(pc=-3), dict(centres=None), dict(centres=None, pc=255), dict(S=0), dict(b=-1), dict(b=(1 << 20) + 1),
            dict(dense=None), dict(g=0), dict(dense=None, g=0), dict(dense=None, g=0, dense_out=None), dict(dense=None, g=0, len=None),
            dict(normals=None), dict(normals=None, normals_out=None), dict(normals=None, pn=None), dict(clouds=None), dict(sidx=None),
            dict(patches=None), dict(cloud=None), dict(ws=None), dict(nbytes=63), dict(ws=ctypes.c_void_p(0x100002))]


def test_the_sizer_and_the_refusals_before_any_launch():
    from sapcu_amd import _lib
    lib = _lib.load()
    size = lib.sapcu_train_patches_workspace_bytes
    assert size(-1) == -1 and size((1 << 20) + 1) == -1 and size(0) == 0 and size(4) == 64 and size(64) == 16 * 64
    for over in REFUSALS:
        assert c_call(lib, **over) == -1, over
        assert lib.sapcu_last_error()
    assert c_call(lib, b=0) == 0                                # no entry: nothing is launched
    assert c_call(lib, b=0, clouds=None, sidx=None, patches=None, cloud=None, ws=None, nbytes=0) == 0


# ------------------------------------------------------------------------------------------------ fixture and data_ref
def _case(g, name):
    return {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/")}


def test_the_fixture_holds_what_the_issue_lists():
    g = golden("train_data.npz")
    assert sorted(g["cases"]) == sorted(FD_CASES + FN_CASES)
    for name in FD_CASES:
        c = _case(g, name)
        assert c["input_raw"].shape == (256, 3) and c["dense_raw"].shape == (1024, 3) and c["idx"].shape == (256, FD_K)
        assert c["cloud"].shape == (256, 3) and c["points"].shape == (1024, 3) and c["len"].shape == (256,)
        assert all(c[k].dtype == np.float32 for k in ("input_raw", "dense_raw", "cloud", "points", "len")) and c["idx"].dtype == np.int32
        assert ("theta" in c) == ("train" in name) == ("aug_cloud" in c) == ("jitter" in c)
    for name in FN_CASES:
        c = _case(g, name)
        assert c["points_raw"].shape == (512, 3) and c["normals_raw"].shape == (512, 3) and c["idx"].shape == (64, FN_K)
        assert c["centres"].shape == (64,) and len(set(c["centres"].tolist())) == 64 and c["normal"].shape == (64, 3)
        assert ("theta" in c) == ("train" in name) == ("aug_normals" in c)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "train_data.npz")) < 512 * 1024


def _assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), "%s: %d of %d elements differ" % (what, int((got != want).sum()), want.size)


@pytest.mark.parametrize("name", ["fd_val0", "fd_val1"])
def test_data_ref_equals_the_reference_on_unaugmented_fd_samples(name):
    c = _case(golden("train_data.npz"), name)
    o = R.sample(c["input_raw"], FD_K, dense=c["dense_raw"])
    for key, ref in (("cloud", "cloud"), ("points", "dense"), ("len", "len"), ("idx", "idx")):
        _assert_same(o[ref], c[key], "%s/%s" % (name, key))
    _assert_same(o["patches"], c["cloud"][c["idx"]], name + "/input")


def test_data_ref_equals_the_reference_on_the_unaugmented_fn_sample():
    c = _case(golden("train_data.npz"), "fn_val")
    o = R.sample(c["points_raw"], FN_K, normals=c["normals_raw"], centres=c["centres"])
    for key, ref in (("cloud", "cloud"), ("all_normals", "normals"), ("normal", "patch_normals"), ("idx", "idx")):
        _assert_same(o[ref], c[key], "fn_val/" + key)


@pytest.mark.parametrize("name", ["fd_train0", "fd_train1", "fn_train"])
def test_data_ref_equals_the_reference_from_the_recorded_augmented_cloud(name):
    """Teacher-forced: every stage after the augmentation, started from the reference's own augmented arrays."""
    c = _case(golden("train_data.npz"), name)
    if name.startswith("fd"):
        o = R.sample(c["aug_cloud"], FD_K, dense=c["aug_dense"])
        pairs = (("cloud", "cloud"), ("points", "dense"), ("len", "len"), ("idx", "idx"))
    else:
        o = R.sample(c["aug_cloud"], FN_K, normals=c["aug_normals"], centres=c["centres"])
        pairs = (("cloud", "cloud"), ("all_normals", "normals"), ("normal", "patch_normals"), ("idx", "idx"))
    for key, ref in pairs:
        _assert_same(o[ref], c[key], "%s/%s" % (name, key))


def rotation_products(c, name):
    """(raw array, the reference's BLAS product of it) pairs of one augmented fixture case."""
    if name.startswith("fd"):
        return [(c["input_raw"], c["rot_cloud"]), (c["dense_raw"], c["rot_dense"])]
    return [(c["points_raw"], c["rot_cloud"]), (c["normals_raw"], c["aug_normals"])]


@pytest.mark.parametrize("name", ["fd_train0", "fd_train1", "fn_train"])
def test_the_plain_order_rotation_is_within_its_bound_of_the_reference_product(name):
    """The one stage that cannot be held bit for bit: the reference's `pc @ rotation.T` is an f32 BLAS call.  The recorded draws
    reproduce its matrix exactly; the plain-order product is within ROTATION_ULPS of the recorded BLAS one (data_ref.rotation_ulps
    names the unit); and scale and jitter, applied to the reference's own product, reproduce its augmented cloud to the bit."""
    c = _case(golden("train_data.npz"), name)
    cs, sn = np.cos(c["theta"]), np.sin(c["theta"])
    _assert_same(np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1]], dtype=np.float32), c["rot"], name + "/rot")
    assert 0 <= c["theta"] < 2 * np.pi and 0.8 <= c["scale"] <= 1.2 and c["jitter"].dtype == np.float32
    for raw, product in rotation_products(c, name):
        ulps = R.rotation_ulps(raw, c["rot"], product)
        print("%s: plain-order rotation against the reference's product: %g ulp" % (name, ulps))
        assert ulps <= ROTATION_ULPS
    cloud, dense, _ = R.augment(c["rot_cloud"], c.get("rot_dense"), scale=np.float32(c["scale"]), jitter=c["jitter"])
    _assert_same(cloud, c["aug_cloud"], name + "/aug_cloud")
    if dense is not None:
        _assert_same(dense, c["aug_dense"], name + "/aug_dense")


def test_the_fixture_is_free_of_neighbour_ties():
    g = golden("train_data.npz")
    for name in FD_CASES + FN_CASES:
        c = _case(g, name)
        fd = name.startswith("fd")
        centres = np.arange(256) if fd else c["centres"]
        k = FD_K if fd else FN_K
        _, d = R.neighbours(c["cloud"], centres, k + 1, want_dist=True)
        assert (np.diff(d, axis=1) > 0).all(), name
        assert (d[:, 0] == 0).all()                              # the point itself comes first


def test_the_restated_centroid_is_numpys_mean():
    rng = np.random.default_rng(5)
    for n in (1, 7, 100, 256, 1000, 4096):
        x = rng.normal(size=(n, 3)).astype(np.float32) * 3 + 1
        _assert_same(R.centroid(x), x.mean(axis=0), "n=%d" % n)


# ------------------------------------------------------------------------------------------------ Python layer, no device
def test_split_arithmetic_and_the_clamp_of_k():
    import sapcu_amd
    from sapcu_amd import data
    assert sapcu_amd.build_patches is data.build_patches and sapcu_amd.PU1KPatches is data.PU1KPatches
    assert sapcu_amd.MeshPatches is data.MeshPatches
    for total in (1, 9, 10, 11, 19, 20, 1019, 24000):
        cut = int(total * 0.9)
        assert data.split_range(total, "train") == (0, cut) and data.split_range(total, "val") == (cut, total)
        assert data.split_range(total, "all") == (0, total)
    assert data.clamp_k(32, 256) == 32 and data.clamp_k(32, 20) == 20 and data.clamp_k(128, 4096) == 128 and data.clamp_k(1, 1) == 1
    for k, n in ((0, 10), (-1, 10), (129, 4096), (200, 150)):
        with pytest.raises(ValueError):
            data.clamp_k(k, n)


def test_argument_errors_that_need_no_device(tmp_path):
    from sapcu_amd import data
    f32 = np.float32
    ok_in, ok_dense = np.zeros((20, 256, 3), f32), np.zeros((20, 1024, 3), f32)
    for bad in (np.zeros((20, 256, 2), f32), np.zeros((256, 3), f32), np.zeros((20, 256, 3), np.int64)):
        with pytest.raises(ValueError):
            data.PU1KPatches(bad, ok_dense)
        with pytest.raises(ValueError):
            data.PU1KPatches(ok_in, bad)
        with pytest.raises(ValueError):
            data.MeshPatches(bad, bad)
    for kw in (dict(split="test"), dict(batch_size=0), dict(k_neighbors=0)):
        with pytest.raises(ValueError):
            data.PU1KPatches(ok_in, ok_dense, **kw)
    with pytest.raises(ValueError):
        data.PU1KPatches(ok_in, ok_dense[:19])                   # sample counts differ
    with pytest.raises(ValueError):
        data.PU1KPatches(np.zeros((20, 5000, 3), f32), ok_dense)  # more points than a workgroup's tile holds
    with pytest.raises(ValueError):
        data.PU1KPatches(ok_in[:1], ok_dense[:1], split="train")  # int(0.9 * 1) = 0 training samples
    with pytest.raises(ValueError):
        data.MeshPatches(ok_in, np.zeros((20, 255, 3), f32))
    with pytest.raises(ValueError):
        data.MeshPatches(ok_in, ok_in, num_patches=0)
    with pytest.raises(RuntimeError):
        data.PU1KPatches(ok_in, ok_dense, device="cpu")
    with pytest.raises(RuntimeError):
        data.MeshPatches(ok_in, ok_in, device="cpu")
    # files: the reference's keys
    path = str(tmp_path / "pairs.npz")
    np.savez(path, poisson_256=ok_in, poisson_1024=ok_dense)
    with pytest.raises(RuntimeError):
        data.PU1KPatches(path, path, device="cpu")               # both arrays were found and accepted; only the device is refused
    np.savez(path, other=ok_in)
    with pytest.raises(ValueError):
        data.PU1KPatches(path, path, device="cpu")
    with pytest.raises(ValueError):
        data.PU1KPatches(str(tmp_path / "pairs.txt"), ok_dense)
    # build_patches: CPU tensors are refused, whatever else is wrong with them
    idx = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        data.build_patches(torch.zeros(4, 256, 3), idx, 32)
    with pytest.raises(ValueError):
        data.build_patches(ok_in, idx, 32)                       # a numpy array is not a device tensor
