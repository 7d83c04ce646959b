"""Mesh sampling without a GPU: the numpy restatement (tests/surface_ref.py, then tests/data_ref.py) against what the reference's
``_sample_points_from_mesh`` and ``__getitem__`` returned (tests/golden/surface_sample.npz) bit for bit, the two orders a parallel
implementation would get wrong shown to matter on the fixture's torus, the binding's ninth table against include/sapcu_surface.h,
the sizer and the refusals of the C entry points that come before any launch, ``read_off(triangulate=True)`` against the reference's
loader, and the argument errors of the Python layer that need no device."""
import ctypes
import os

import numpy as np
import pytest

import data_ref as R
import surface_ref as SR
import abi_tables
from conftest import ROOT, golden

MESHES = ("icosphere", "torus", "degenerate", "polygons")
ITEMS = ("item_train", "item_val")
N, PATCHES, K = 512, 64, 12
F32 = np.float32


def header_entry_points():
    """{name: argument list} of include/sapcu_surface.h."""
    return abi_tables.header_entry_points("sapcu_surface.h")


def _case(g, name):
    return {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/")}


def _assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), "%s: %d of %d elements differ" % (what, int((got != want).sum()), want.size)


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_declares_exactly_the_ninth_table():
    from sapcu_amd import _lib
    decl = header_entry_points()
    assert set(decl) == set(_lib.SURFACE_EXPORTS) == {"sapcu_surface_tables_workspace_bytes", "sapcu_surface_tables_f32",
                                                      "sapcu_surface_sample_f32"}
    others = (_lib.EXPORTS, _lib.SEEDS_EXPORTS, _lib.FD_TRAIN_EXPORTS, _lib.FD_EDGECONV_EXPORTS, _lib.TRAIN_STEP_EXPORTS,
              _lib.METRICS_EXPORTS, _lib.DATA_EXPORTS, _lib.MESH_EXPORTS)
    for other in others:
        assert not set(other) & set(_lib.SURFACE_EXPORTS)
    assert len(_lib.EXPORTS) == 46 and _lib.ABI_VERSION == 2
    assert not any(n.startswith(("sapcu_point_mesh", "sapcu_train_patches")) for n in _lib.SURFACE_EXPORTS)
    lib = _lib.load()
    for name in _lib.SURFACE_EXPORTS:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len([a for a in decl[name].split(",") if a.strip()]), name
    for other in ("sapcu.h", "sapcu_data.h", "sapcu_mesh.h", "sapcu_metrics.h"):
        with open(os.path.join(ROOT, "include", other)) as f:
            assert "sapcu_surface" not in f.read(), other


P = ctypes.c_void_p


def tables_call(lib, **over):
    """sapcu_surface_tables_f32 on pointers that are never dereferenced (every refusal comes before the first HIP call)."""
    a = dict(vertices=P(0x10000), vert_off=P(0x20000), tv=100, faces=P(0x30000), face_off=P(0x40000), tf=200, S=3, normals=P(0x50000),
             cdf=P(0x60000), area_sum=P(0x70000), prob_sum=P(0x80000), ws=P(0x90000), nbytes=812)
    a.update(over)
    return lib.sapcu_surface_tables_f32(a["vertices"], a["vert_off"], a["tv"], a["faces"], a["face_off"], a["tf"], a["S"], a["normals"],
                                        a["cdf"], a["area_sum"], a["prob_sum"], a["ws"], a["nbytes"], None)


def sample_call(lib, **over):
    a = dict(vertices=P(0x10000), vert_off=P(0x20000), tv=100, faces=P(0x30000), face_off=P(0x40000), tf=200, normals=P(0x50000),
             cdf=P(0x60000), S=3, midx=P(0x70000), b=4, n=512, u=P(0x80000), r1=P(0x90000), r2=P(0xa0000), points=P(0xb0000),
             normals_out=P(0xc0000), face=P(0xd0000))
    a.update(over)
    return lib.sapcu_surface_sample_f32(a["vertices"], a["vert_off"], a["tv"], a["faces"], a["face_off"], a["tf"], a["normals"], a["cdf"],
                                        a["S"], a["midx"], a["b"], a["n"], a["u"], a["r1"], a["r2"], a["points"], a["normals_out"], a["face"],
                                        None)


TABLES_REFUSALS = [dict(S=-1), dict(S=(1 << 20) + 1), dict(tf=0), dict(tf=-5), dict(tf=(1 << 29) + 1), dict(tv=0), dict(tv=1 << 31),
                   dict(vertices=None), dict(vert_off=None), dict(faces=None), dict(face_off=None), dict(normals=None), dict(cdf=None),
                   dict(ws=None), dict(nbytes=811), dict(nbytes=0), dict(ws=P(0x90002)), dict(ws=P(0x90001))]
SAMPLE_REFUSALS = [dict(S=-1), dict(S=(1 << 20) + 1), dict(tf=0), dict(tf=(1 << 29) + 1), dict(tv=0), dict(n=0), dict(n=-1), dict(n=4097),
                   dict(b=-1), dict(b=(1 << 20) + 1), dict(vertices=None), dict(vert_off=None), dict(faces=None), dict(face_off=None),
                   dict(normals=None), dict(cdf=None), dict(midx=None), dict(u=None), dict(r1=None), dict(r2=None), dict(points=None),
                   dict(normals_out=None)]


def test_the_sizer_and_the_refusals_before_any_launch():
    from sapcu_amd import _lib
    lib = _lib.load()
    size = lib.sapcu_surface_tables_workspace_bytes
    assert size(3, 200) == 4 * (200 + 3) and size(1, 1) == 8 and size(0, 7) == 28 and size(1 << 20, 1 << 29) == 4 * ((1 << 29) + (1 << 20))
    for S, tf in ((-1, 10), ((1 << 20) + 1, 10), (3, 0), (3, -1), (3, (1 << 29) + 1)):
        assert size(S, tf) == -1, (S, tf)
    for over in TABLES_REFUSALS:
        assert tables_call(lib, **over) == -1, over
        assert lib.sapcu_last_error()
    for over in SAMPLE_REFUSALS:
        assert sample_call(lib, **over) == -1, over
        assert lib.sapcu_last_error()
    assert tables_call(lib, S=0) == 0                           # no mesh, no entry: nothing is launched
    assert sample_call(lib, b=0) == 0 and sample_call(lib, S=0) == 0 and sample_call(lib, b=0, face=None) == 0


# ------------------------------------------------------------------------------------------- the fixture and surface_ref
def test_the_fixture_holds_what_the_issue_lists():
    g = golden("surface_sample.npz")
    assert sorted(g["cases"]) == sorted(MESHES + ITEMS)
    for name in MESHES:
        c = _case(g, name)
        assert c["vertices"].dtype == F32 and c["vertices"].shape[1] == 3 and c["faces"].dtype == np.int32 and c["faces"].shape[1] == 3
        assert c["u"].dtype == np.float64 and c["u"].shape == (N,) and c["r1"].dtype == c["r2"].dtype == F32
        assert c["points"].shape == c["normals"].shape == (N, 3) and c["face"].shape == (N,) and c["face"].dtype == np.int32
        assert ((c["u"] >= 0) & (c["u"] < 1)).all() and ((c["r1"] >= 0) & (c["r1"] <= 1)).all() and ((c["r2"] >= 0) & (c["r2"] <= 1)).all()
    assert len(_case(g, "icosphere")["faces"]) == 320 and len(_case(g, "torus")["faces"]) == 5000
    areas = SR.face_tables(*[_case(g, "torus")[k] for k in ("vertices", "faces")])[1]
    assert areas.max() / areas[areas > 0].min() > 1e4           # several orders of magnitude
    d = _case(g, "degenerate")
    zero = np.flatnonzero(SR.face_tables(d["vertices"], d["faces"])[1] == 0)
    assert zero.tolist() == [0, 41, len(d["faces"]) - 1]        # the first, a middle and the last face
    for name in ITEMS:
        c = _case(g, name)
        assert c["cloud"].shape == (N, 3) and c["idx"].shape == (PATCHES, K) and c["centres"].shape == (PATCHES,)
        assert ("theta" in c) == (name == "item_train") == ("aug_cloud" in c) == ("jitter" in c)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "surface_sample.npz")) < 256 * 1024


@pytest.mark.parametrize("name", MESHES)
def test_surface_ref_equals_the_reference_sampler(name):
    """The restatement on the recorded draws: the reference's points and normals with ==, the recorded faces, and no face of zero
    area among them."""
    c = _case(golden("surface_sample.npz"), name)
    tab = SR.tables(c["vertices"], c["faces"])
    points, normals, face = SR.sample(c["vertices"], c["faces"], tab, c["u"], c["r1"], c["r2"])
    _assert_same(points, c["points"], name + "/points")
    _assert_same(normals, c["normals"], name + "/normals")
    _assert_same(face, c["face"], name + "/face")
    assert (tab["areas"][face] > 0).all()
    assert tab["cdf"][-1] == 1.0 and (np.diff(tab["cdf"]) >= 0).all() and abs(tab["prob_sum"] - 1) < 1e-6


@pytest.mark.parametrize("name", MESHES)
def test_the_restated_sums_are_numpys(name):
    """np_sum_f32 is ndarray.sum() and the cdf is what the legacy RandomState.choice builds (cumsum of the f64 copy, / its last)."""
    c = _case(golden("surface_sample.npz"), name)
    tab = SR.tables(c["vertices"], c["faces"])
    areas = tab["areas"]
    assert tab["area_sum"] == areas.sum() and tab["area_sum"].dtype == F32
    p = (areas / (areas.sum() + 1e-8)).astype(np.float64)
    cdf = p.cumsum()
    cdf /= cdf[-1]
    _assert_same(tab["cdf"], cdf, name + "/cdf")


def test_np_sum_f32_at_the_boundaries_of_the_pairwise_sum():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 8, 9, 127, 128, 129, 135, 136, 137, 255, 256, 257, 1023, 1024, 1025, 4097, 8191, 8192, 8193, 16385, 20011, 40000):
        a = (rng.random(n) ** 6).astype(F32)
        assert SR.np_sum_f32(a) == a.sum(), n


def test_the_torus_tells_the_orders_apart():
    """What keeps the GPU tests from passing with the wrong order: on the torus a scan of p in two blocks is not the sequential cdf,
    and a sequential f32 sum of the areas is not numpy's pairwise one."""
    c = _case(golden("surface_sample.npz"), "torus")
    tab = SR.tables(c["vertices"], c["faces"])
    areas = tab["areas"]
    p = (areas / F32(tab["area_sum"] + F32(1e-8))).astype(F32).astype(np.float64)
    sequential = np.add.accumulate(p, dtype=np.float64)
    assert sequential[-1] == tab["prob_sum"]
    differing = int((SR.two_block_scan(p, len(p) // 2) != sequential).sum())
    print("two-block scan: %d of %d cdf entries differ from the sequential sum" % (differing, len(p)))
    assert differing >= 1
    assert np.add.accumulate(areas, dtype=F32)[-1] != tab["area_sum"]


@pytest.mark.parametrize("name", ITEMS)
def test_the_whole_getitem_from_the_recorded_draws(name):
    """surface_ref on the recorded u, r1, r2 gives the sampling the reference's __getitem__ started from; data_ref on it (from the
    reference's own augmented arrays in the train case: its rotation is a BLAS product) gives every array it returned."""
    g = golden("surface_sample.npz")
    c = _case(g, name)
    m = _case(g, str(c["mesh"]))
    tab = SR.tables(m["vertices"], m["faces"])
    points, normals, face = SR.sample(m["vertices"], m["faces"], tab, c["u"], c["r1"], c["r2"])
    _assert_same(points, c["points"], name + "/points")
    _assert_same(normals, c["normals"], name + "/normals")
    _assert_same(face, c["face"], name + "/face")
    if name == "item_train":
        cs, sn = np.cos(c["theta"]), np.sin(c["theta"])
        _assert_same(np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1]], dtype=F32), c["rot"], name + "/rot")
        for raw, product in ((points, c["rot_cloud"]), (normals, c["aug_normals"])):
            assert R.rotation_ulps(raw, c["rot"], product) <= 2  # tests/test_data_host.py ROTATION_ULPS
        cloud, _, _ = R.augment(c["rot_cloud"], scale=F32(c["scale"]), jitter=c["jitter"])
        _assert_same(cloud, c["aug_cloud"], name + "/aug_cloud")
        points, normals = c["aug_cloud"], c["aug_normals"]
    o = R.sample(points, K, normals=normals, centres=c["centres"])
    for key, ref in (("cloud", "cloud"), ("all_normals", "normals"), ("normal", "patch_normals"), ("idx", "idx")):
        _assert_same(o[ref], c[key], "%s/%s" % (name, key))


# ----------------------------------------------------------------------------------------------------------------- read_off
def test_read_off_triangulates_as_the_reference_loader(tmp_path):
    from sapcu_amd import mesh
    c = _case(golden("surface_sample.npz"), "polygons")
    path = str(tmp_path / "polygons.off")
    with open(path, "wb") as f:
        f.write(c["off_text"].tobytes())
    vertices, faces = mesh.read_off(path, triangulate=True)
    assert vertices.dtype == np.float64 and faces.dtype == np.int64
    _assert_same(vertices.astype(F32), c["vertices"], "vertices")
    _assert_same(faces.astype(np.int32), c["faces"], "faces")
    assert len(faces) == 14                                      # 4 quads -> 8, a pentagon -> 3, 3 triangles, the two-corner face dropped
    with pytest.raises(ValueError):                              # the default is unchanged: a polygon is refused
        mesh.read_off(path)
    with pytest.raises(ValueError):
        mesh.read_off(path, triangulate=False)
    tri = str(tmp_path / "tri.off")
    with open(tri, "w") as f:
        f.write("OFF\n4 2 0\n0 0 0\n1 0 0\n0 1 0\n0 0 1\n3 0 1 2\n3 0 2 3 255 0 0\n")
    v0, f0 = mesh.read_off(tri)
    v1, f1 = mesh.read_off(tri, triangulate=True)
    _assert_same(v1, v0, "vertices of a triangle file")
    _assert_same(f1, f0, "faces of a triangle file")
    assert f0.tolist() == [[0, 1, 2], [0, 2, 3]]
    bad = str(tmp_path / "bad.off")
    with open(bad, "w") as f:
        f.write("OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n4 0 1 2\n")
    with pytest.raises(ValueError):
        mesh.read_off(bad, triangulate=True)                     # four corners announced, three given


# ------------------------------------------------------------------------------------------------ Python layer, no device
def test_exports_and_argument_errors_that_need_no_device(tmp_path):
    import sapcu_amd
    from sapcu_amd import data, surface
    assert sapcu_amd.MeshSurfacePatches is data.MeshSurfacePatches and sapcu_amd.build_surface_tables is surface.build_surface_tables
    assert sapcu_amd.sample_surface is surface.sample_surface
    tri = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32), np.array([[0, 1, 2]], np.int32))
    with pytest.raises(RuntimeError):
        surface.build_surface_tables([tri], device="cpu")
    with pytest.raises(ValueError):
        surface.build_surface_tables([], device="cpu")
    with pytest.raises(ValueError):
        surface.sample_surface(object(), None, 4, None, None, None)
    meshes = [tri] * 10
    for kw in (dict(split="test"), dict(batch_size=0), dict(k_neighbors=0), dict(num_points=0), dict(num_points=4097), dict(num_patches=0)):
        with pytest.raises(ValueError):
            data.MeshSurfacePatches(meshes, device="cpu", **kw)
    with pytest.raises(ValueError):
        data.MeshSurfacePatches(meshes[:1], device="cpu")        # int(0.9 * 1) = 0 training meshes
    with pytest.raises(RuntimeError):
        data.MeshSurfacePatches(meshes, device="cpu")            # everything else was accepted; only the device is refused
    # the folder rule of the reference: category sub-folders when there are any, else the folder's own files, sorted
    with pytest.raises(ValueError):
        data.mesh_files(str(tmp_path))
    for name in ("b.off", "a.off", "c.txt"):
        (tmp_path / name).write_text("OFF\n")
    assert [os.path.basename(f) for f in data.mesh_files(str(tmp_path))] == ["a.off", "b.off"]
    for cat, name in (("chair", "z.off"), ("bed", "y.off"), ("bed", "x.off")):
        (tmp_path / cat).mkdir(exist_ok=True)
        (tmp_path / cat / name).write_text("OFF\n")
    assert [os.path.relpath(f, str(tmp_path)) for f in data.mesh_files(str(tmp_path))] == ["bed/x.off", "bed/y.off", "chair/z.off"]
    with pytest.raises(RuntimeError):
        data.MeshSurfacePatches(str(tmp_path), split="all", device="cpu")        # three files found; only the device is refused
