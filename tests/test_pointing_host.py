"""The definition of csrc/sapcu_pointing.h as tests/pointing_ref.py states it, without a GPU: its neighbours against sklearn's KDTree
on the tie-free cases, the screening of tests/pointing_cases.py, the header against the binding, and the refusals of
sapcu_amd.pointing / sapcu_amd.data that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import pointing_cases as K
import pointing_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", K.PLAIN)
def test_the_definitions_neighbours_are_kdtrees(name):
    from sklearn.neighbors import KDTree
    c, r = K.CASES[name], K.reference(name)
    dist, idx = KDTree(c["P"]).query(r["q"], c["k"])                 # the script's tree: built on the f32 points
    assert np.array_equal(idx, r["idx"])
    assert np.array_equal(dist[:, 0], r["d1"])
    _, full, _ = R.neighbours(c["P"], r["q"], c["k"])
    assert np.array_equal(dist, full)


@pytest.mark.parametrize("name", K.PLAIN)
def test_plain_cases_pass_their_screening(name):
    s = K.screen(name)
    print(name, s)
    assert s["ties"] == 0 and s["band_edge"] == 0 and s["zero_len"] == 0 and s["candidates"] > 0


def test_the_cases_cover_what_they_are_there_for():
    s = {name: K.screen(name) for name in K.CASES}
    assert any(0.1 * v["candidates"] <= v["kept"] <= 0.9 * v["candidates"] for name, v in s.items() if name in K.PLAIN)
    assert any(v["outside"] for name, v in s.items() if name in K.PLAIN)
    assert any(len(K.CASES[n]["P"]) < K.GRID_MIN_N for n in K.PLAIN) and any(len(K.CASES[n]["P"]) >= K.GRID_MIN_N for n in K.PLAIN)
    assert {K.CASES[n]["k"] for n in K.PLAIN} >= {1, 6, 10, 16}
    for k in (1, 6, 10):
        assert s["lattice-tie-k%d" % k]["ties"] == s["lattice-tie-k%d" % k]["candidates"] == 512
    z = K.reference("zero-len-k6")
    assert s["zero-len-k6"]["zero_len"] == 1 and z["keep"][0] and np.isnan(z["pointing"][0]).all() and z["length"][0] == 0
    assert np.isfinite(z["pointing"][1:]).all()
    assert s["duplicates"]["ties"] > 0
    bad = K.reference("non-finite")
    assert not np.isin(bad["idx"], (17, 101, 150)).any() and (bad["idx"] >= 0).all()
    assert len(K.CASES["k-equals-n"]["P"]) == K.CASES["k-equals-n"]["k"] and len(K.CASES["one-point"]["P"]) == 1
    for name in K.CASES:                                             # the shapes the GPU tests pay for
        assert len(K.CASES[name]["P"]) <= 6000 and s[name]["candidates"] <= 30000
        assert 3 <= K.CASES[name]["count"] <= 8 and 2 <= K.CASES[name]["sub"] <= 4


def test_no_jitter_is_a_zero_jitter_without_the_addition():
    c = K.CASES["noisy-4097-nojitter"]
    a = R.candidates(c["voxels"], c["origin"], c["step"], c["count"], c["sub"])
    b = R.candidates(c["voxels"], c["origin"], c["step"], c["count"], c["sub"], np.zeros((len(a), 3)))
    assert np.array_equal(a, b)                                      # x + 0.0 = x for every x but -0.0, and no coordinate is -0.0
    assert not np.signbit(a[a == 0]).any()


def test_the_strict_near_bound():
    P = np.array([[0.0, 0.0, 0.0]], np.float32)
    centre = R.centres(-0.5, 0.25, 4)
    d = np.sqrt(R.dist2(centre, P.astype(np.float64))[:, 0])
    near = float(np.sort(np.unique(d))[1])                           # the distance of some voxel centres exactly
    inside = R.near_voxels(P, -0.5, 0.25, 4, near)
    assert len(inside) == np.count_nonzero(d < near) < np.count_nonzero(d <= near)


def test_the_binding_and_the_header_agree():
    """csrc/sapcu_pointing.h lies outside include/ (tests/test_abi_tables.py holds that folder's list closed): the same checks here."""
    from sapcu_amd import _lib, pointing
    from abi_tables import parameter_count
    with open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "sapcu_pointing.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(sapcu_\w+)\s*\(([^;{]*)\)\s*;", text)}
    assert set(decl) == set(_lib.POINTING_SIGNATURES) == set(_lib.POINTING_EXPORTS) and len(decl) == 2
    lib = _lib.load()
    for name in decl:
        assert len(getattr(lib, name).argtypes) == parameter_count(decl[name]) == len(_lib.POINTING_SIGNATURES[name][1]), name
    assert int(re.search(r"#define SAPCU_POINTING_MAX_K (\d+)", text).group(1)) == pointing.MAX_K == 16
    assert len(os.listdir(os.path.join(ROOT, "include"))) == len([h for h in _lib.TABLES if h is not None])
    size = lib.sapcu_pointing_workspace_bytes
    assert size(1, 0, 1, 1) > 0 and size(5000, 1024, 10, 10) > size(5000, 8, 10, 10) > 0
    assert size(5000, 64, 4, 16) > size(5000, 64, 4, 1)
    assert size(0, 1, 2, 1) < 0 and size((1 << 29) + 1, 1, 2, 1) < 0 and size(10, -1, 2, 1) < 0 and size(10, 1, 0, 1) < 0
    assert size(10, 1, 1025, 1) < 0 and size(10, 1, 2, 0) < 0 and size(10, 1, 2, 17) < 0
    assert size(10, ((1 << 31) - 64) // 1000 + 1, 10, 10) < 0 and size(10, ((1 << 31) - 64) // 1000, 10, 10) > 0        # m beyond int32


def test_refusals_come_before_the_library_loads(monkeypatch):
    import sapcu_amd
    from sapcu_amd import _lib, data, pointing

    def no_library(*a, **kw):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(_lib, "load", no_library)
    P, v = torch.zeros((8, 3)), torch.zeros((2,), dtype=torch.int64)
    with pytest.raises(RuntimeError):
        pointing.near_voxels(P)
    with pytest.raises(RuntimeError):
        pointing.pointing_samples(P, v)
    for bad in (dict(step=0.0), dict(step=float("nan")), dict(origin=float("inf")), dict(count=0), dict(count=2000), dict(near=float("nan"))):
        with pytest.raises(ValueError):
            pointing.near_voxels(P, **bad)
    with pytest.raises(ValueError):
        pointing.near_voxels(P.numpy())
    for bad in (dict(sub=0), dict(sub=2000), dict(k=0), dict(k=17), dict(band=(float("nan"), 1.0)), dict(cell_size=-1.0),
                dict(cell_size=float("inf")), dict(voxels_per_call=0), dict(step=-1.0), dict(count=0)):
        with pytest.raises(ValueError):
            pointing.pointing_samples(P, v, **bad)
    with pytest.raises(ValueError):
        pointing.sample_fn_pointing(None, 0, 100, None)
    with pytest.raises(ValueError):
        pointing.as_fn_npz(np.zeros((4, 3)), np.zeros((5, 3)))
    z = pointing.as_fn_npz(torch.ones((4, 3), dtype=torch.float64), np.zeros((4, 3)))
    assert sorted(z) == ["normals", "pointing", "points"] and z["normals"] is z["pointing"] and z["points"].dtype == np.float64
    with pytest.raises(RuntimeError):
        data.seed_patches(P, torch.zeros((2, 3), dtype=torch.float64), 4)
    with pytest.raises(ValueError):
        data.seed_patches(P.numpy(), None, 4)
    tri = [(np.eye(3, dtype=np.float32), np.array([[0, 1, 2]]))] * 10
    for cls in (data.FnPointingPatches, data.FdSeedPatches):
        for kw in (dict(num_patches=0), dict(split="test"), dict(cloud_points=0), dict(cloud_points=data.MAX_N + 1), dict(k_neighbors=0),
                   dict(batch_size=0), dict(cloud_points=16, k_neighbors=17)):
            with pytest.raises(ValueError):
                cls(tri, **kw)
        with pytest.raises(RuntimeError):
            cls(tri, device="cpu")
    for kw in (dict(surface_points=0), dict(pointing_size=0), dict(geometry={"radius": 1.0})):
        with pytest.raises(ValueError):
            data.FnPointingPatches(tri, **kw)
    with pytest.raises(ValueError):
        data.FdSeedPatches(tri, num_rays=0)
    assert sapcu_amd.FnPointingPatches is data.FnPointingPatches and sapcu_amd.pointing_samples is pointing.pointing_samples
    assert "pointing_samples" not in sapcu_amd.__all__ and len(sapcu_amd.__all__) == 7
