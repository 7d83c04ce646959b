"""The definition of csrc/sapcu_poisson.h as tests/poisson_ref.py states it, without a GPU: the synchronous-round form selects what
the greedy form selects, the strict comparison, duplicates, the adversarial line, the invariants of the bisection, the blue-noise
property the definition is there for, and the refusals of sapcu_amd.poisson / data.PoissonPU1KPatches that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import poisson_cases as K
import poisson_ref as R

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [("sphere-1", K.sphere(1), 0.3), ("sphere-2", K.sphere(2), 3.0), ("sphere-65", K.sphere(65), 0.5), ("sphere-257", K.sphere(257), 0.25),
         ("sphere-1000", K.sphere(1000), K.typical_radius(1000)), ("sphere-1000-r0", K.sphere(1000), 0.0),
         ("plane-1000", K.plane(1000), 0.05), ("equal-255", K.equal(255), 0.1), ("equal-255-r0", K.equal(255), 0.0),
         ("one-cell-256", K.plane(256), 2.0), ("offset-1000", K.offset(1000), K.typical_radius(1000)),
         ("lattice-tie", K.lattice(), 0.25), ("lattice-above", K.lattice(), np.nextafter(F32(0.25), F32(1))), ("line-300", K.line(), 0.015)]


@pytest.mark.parametrize("name,P,r", CASES, ids=[c[0] for c in CASES])
def test_the_round_form_selects_what_the_greedy_form_selects(name, P, r):
    keep, count = K.ref_select(P, r)
    keep_r, count_r, rounds = K.ref_rounds(P, r)
    assert np.array_equal(keep, keep_r) and count == count_r == int(keep.sum())
    assert 1 <= rounds <= len(P) and keep[0]


def test_the_comparison_is_strict():
    P = K.lattice()
    keep, count = R.select(P, F32(0.25))
    assert count == 64 and keep.all()                               # neighbours at exactly r: both stay
    above = np.nextafter(F32(0.25), F32(1))
    keep, count = R.select(P, above)
    i, j, k = np.unravel_index(np.arange(64), (4, 4, 4))
    # greedy in row order on the lattice: a point goes iff an axis neighbour before it stayed, which leaves the even-parity points
    assert np.array_equal(keep, (i + j + k) % 2 == 0) and count == 32


def test_duplicates():
    P = K.equal(17)
    assert R.select(P, 0.0)[1] == 17                                  # r = 0 keeps everything, duplicates included
    keep, count = R.select(P, np.nextafter(F32(0), F32(1)))
    assert count == 17                                                # r * r underflows to 0: still nothing is < r2
    keep, count = R.select(P, 1e-20)
    assert count == 1 and keep[0]                                     # any r with r * r > 0 drops the later of two equal rows
    two = np.concatenate([K.sphere(40), K.sphere(40)])
    keep, count = R.select(two, 1e-6)
    assert count == 40 and keep[:40].all() and not keep[40:].any()


def test_the_sorted_line_needs_a_round_per_point():
    keep, count, rounds = K.ref_rounds(K.line(), 0.015)
    assert rounds == 300 and count == 150 and np.array_equal(keep, np.arange(300) % 2 == 0)


@pytest.mark.parametrize("C,n,steps", [(1, 1, 20), (64, 1, 20), (64, 64, 20), (2048, 256, 20), (2048, 256, 1), (2048, 256, 0), (300, 100, 7)])
def test_subsample_invariants(C, n, steps):
    P = K.line(C) if C == 300 else K.sphere(C, 3)
    idx, r, count, keep = K.ref_subsample(P, n, steps)
    assert count >= n and count == int(keep.sum()) and len(idx) == n
    assert np.array_equal(idx, np.flatnonzero(keep)[:n]) and r.dtype == F32 and 0 <= r <= R.start_radius(P)
    if steps == 0:
        assert r == 0 and count == C
    r2 = R.radius2(r)
    d = P[:, None, :] - P[None, :, :]
    d *= d
    d2 = (d[..., 0] + d[..., 1]) + d[..., 2]
    near = d2 < r2
    kept = np.flatnonzero(keep)
    pair = near[np.ix_(kept, kept)]
    assert not pair[~np.eye(len(kept), dtype=bool)].any()           # every kept pair has d2 >= r2
    lower = np.tril(np.ones((C, C), bool), -1)
    assert (near & lower & keep[None, :]).any(1)[~keep].all()       # every dropped row has a kept lower row with d2 < r2


def test_twenty_steps_reach_the_count_on_a_sphere_and_the_result_is_blue_noise():
    P = K.sphere(8192, 5)
    idx, r, count, _ = K.ref_subsample(P, 1024, 20)
    assert count == 1024                                             # the prototype's figure; the contract is only count >= n
    assert 0.6 <= float(r) / np.sqrt(4 * np.pi / 1024) <= 0.8
    cv, cv_first = R.nn_cv(P[idx]), R.nn_cv(P[:1024])
    print("nearest-neighbour CV: subsample %.3f, first n candidates %.3f" % (cv, cv_first))
    assert cv < 0.5 * cv_first


def test_refusals_without_a_device():
    import sapcu_amd
    from sapcu_amd import data, poisson
    P = torch.zeros((8, 3))
    with pytest.raises(ValueError):
        poisson.poisson_select(P.numpy(), 0.1)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            poisson.poisson_select(P, bad)
    with pytest.raises(ValueError):
        poisson.poisson_select(P, 0.1, path="brute")
    with pytest.raises(RuntimeError):
        poisson.poisson_select(P, 0.1)
    with pytest.raises(RuntimeError):
        poisson.poisson_subsample(P, 4)
    with pytest.raises(ValueError):
        poisson.poisson_subsample([[0.0, 0.0, 0.0]], 1)
    with pytest.raises(ValueError):
        poisson.poisson_disk_sample(None, None, 5, torch.zeros((1, 4), dtype=torch.float64), None, None)
    with pytest.raises(ValueError):
        poisson.poisson_disk_sample(None, None, 1, [0.5], None, None)
    tri = [(np.eye(3, dtype=F32), np.array([[0, 1, 2]]))] * 10
    for kw in (dict(num_dense=0), dict(num_dense=data.MAX_G + 1), dict(oversample=0), dict(split="test"), dict(num_input=0),
               dict(num_input=data.MAX_N + 1), dict(k_neighbors=0), dict(batch_size=0)):
        with pytest.raises(ValueError):
            data.PoissonPU1KPatches(tri, **kw)
    with pytest.raises(ValueError):
        data.PoissonPU1KPatches([], split="all")
    with pytest.raises(RuntimeError):
        data.PoissonPU1KPatches(tri, device="cpu")
    assert sapcu_amd.PoissonPU1KPatches is data.PoissonPU1KPatches and sapcu_amd.poisson_subsample is poisson.poisson_subsample


def test_the_binding_and_the_header_agree():
    """csrc/sapcu_poisson.h lies outside include/ (tests/test_abi_tables.py holds that folder's list closed): the same checks here."""
    from sapcu_amd import _lib, poisson
    from abi_tables import parameter_count
    with open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "sapcu_poisson.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(sapcu_\w+)\s*\(([^;{]*)\)\s*;", text)}
    assert set(decl) == set(_lib.POISSON_SIGNATURES) == set(_lib.POISSON_EXPORTS)
    lib = _lib.load()
    for name in decl:
        assert len(getattr(lib, name).argtypes) == parameter_count(decl[name]), name
    assert len(getattr(lib, "sapcu_internal_poisson_select_grid").argtypes) == len(_lib.POISSON_SIGNATURES["sapcu_poisson_select_f32"][1])
    assert int(re.search(r"#define SAPCU_PD_RESIDENT_MAX (\d+)", text).group(1)) == poisson.PD_RESIDENT_MAX == K.RESIDENT_MAX >= 8192
    assert len(os.listdir(os.path.join(ROOT, "include"))) == len([h for h in _lib.TABLES if h is not None])
    # the sizer's refusals
    size = lib.sapcu_poisson_workspace_bytes
    assert size(1, 1) > 0 and size(0, 5) > 0 and size(4, 1 << 24) > size(4, 8192) > 0
    assert size(1, 0) < 0 and size(1, (1 << 24) + 1) < 0 and size(-1, 8) < 0 and size(65536, 8) < 0
