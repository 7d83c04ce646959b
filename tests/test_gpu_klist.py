"""The lane-spread k-list through the entry points, at every k, on clouds whose ties are exact, and the rule for non-finite
distances.

Clouds, queries and the numpy reference are tests/klist_cases.py (tests/test_klist_host.py checks their conditions): dyadic
coordinates, so every squared distance is exact and (distance, index) alone decides the order.  Every comparison is ``==`` on bits or
integers.  knn_outer.hip keeps its own written-out copy of the arrival-order insertion of csrc/wave_ops.h: the knn_gather sweeps hold
that copy to the rule at every k in 1..128, the training-patch sweep the header's (through tp_knn_kernel), the grid sweep the keyed
list.  Launches are tiny (n <= 1331, 9 queries)."""
import numpy as np
import pytest
import torch

import data_ref as R
import gpu_utils as U
import klist_cases as KC
from guarded import Arena

pytestmark = pytest.mark.gpu

F32, F64, I64 = torch.float32, torch.float64, torch.int64


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(U.dev())          # a copy: the shared cases are read-only


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _assert_gather_equals(got, ref, what):
    """idx, the bits of dist, the bits of patch (NaN rows included)."""
    for name, g, r in zip(("idx", "dist", "patch"), got, ref):
        g = g.cpu().numpy()
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.dtype, r.shape)
        bad = (g != r) if name == "idx" else (_bits(g) != _bits(r))
        assert not bad.any(), "%s: %s differs in %d of %d elements, first at %s: %r against %r" % (
            what, name, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), g[bad][0], r[bad][0])


def _canonical_nan(patch):
    """NaN rows with one bit pattern (numpy's default NaN), as the kernels' __builtin_nanf("") writes."""
    return np.where(np.isnan(patch), np.float32(np.nan), patch)


def _sweep(cases):
    from sapcu_amd import generation as gen
    resident, count = {}, 0
    for name, n, k in cases:
        c, q, idx, dist, patch = KC.reference_at(name, n, k)
        if (name, n) not in resident:
            resident[(name, n)] = (_dev(c), _dev(q))
        got = gen.knn_gather(*resident[(name, n)], k, want_dist=True)
        _assert_gather_equals(got, (idx, dist, patch), "%s n=%d k=%d" % (name, n, k))
        count += 1
    return count


def test_knn_gather_at_every_k_on_small_clouds_of_exact_ties():
    """Every k in 1..128 on lattice7, dup4 and line, whole and cut to k, 64 and 65 points."""
    assert _sweep(KC.small_cases()) == len(list(KC.small_cases())) > 3 * 128


def test_knn_gather_at_the_edge_of_the_cloud_tile():
    """lattice11 cut to 1023, 1024, 1025 and 1331 points (KNN_TILE = 1024), k at the slot switch and at both ends."""
    assert _sweep(KC.tile_cases()) == 24


def test_knn_self_grid_at_every_k_against_numpy():
    """Every k in 1..64 on lattice7 and dup4 with the grid route forced by an explicit cell size; the reference is numpy's, not
    knn_gather's."""
    from sapcu_amd import generation as gen
    for name in ("lattice7", "dup4"):
        c = KC.cloud(name)
        idx, dist, _ = KC.reference(c, c, 64)
        pts = _dev(c)
        for k in range(1, 65):
            info = []
            gi, gd = gen.knn_self_grid(pts, k, cell_size=2.0 / 64, info=info)
            assert info[0] == 1, "%s k=%d: the grid did not run (%r)" % (name, k, info)
            assert np.array_equal(gi.cpu().numpy(), idx[:, :k]), (name, k)
            assert np.array_equal(_bits(gd.cpu().numpy()), _bits(dist[:, :k])), (name, k)


def test_training_patches_at_every_k():
    """tp_knn_kernel (WaveTopK first_slab + offer) at every k in 1..128 on a dyadic f32 cloud of 193 points, against data_ref."""
    from sapcu_amd import data
    clouds = KC.train_cloud()
    sidx = np.zeros(1, np.int64)
    ref = R.batch(clouds, sidx, 128)
    cd, sd = _dev(clouds), _dev(sidx)
    for k in range(1, 129):
        out = data.build_patches(cd, sd, k)
        assert np.array_equal(out["idx"].cpu().numpy(), ref["idx"][:, :, :k]), k
        assert np.array_equal(_bits(out["patches"].cpu().numpy()), _bits(ref["patches"][:, :, :k])), k
    _, d = R.neighbours(ref["cloud"][0], np.arange(193), 128, want_dist=True)
    assert (np.diff(d, axis=1) == 0).any(), "the cloud has no tied distances"


# --------------------------------------------------------------------------------------------------- non-finite candidates
@pytest.mark.parametrize("kind", KC.BAD_KINDS)
def test_non_finite_candidates_follow_the_rule(kind):
    """A candidate at a NaN or +inf squared distance is no candidate; finite ones in (distance, index) order, then empty entries
    (index -1, distance +inf, a NaN row); no index twice in a row; finite queries see the cloud without the bad point."""
    from sapcu_amd import generation as gen
    ran = 0
    for kd, n, k in KC.bad_cases():
        if kd != kind:
            continue
        c, q, _, _ = KC.bad_inputs(kind, n)
        idx, dist, patch = KC.reference(c, q, k)
        got = gen.knn_gather(_dev(c), _dev(q), k, want_dist=True)
        gi = got[0].cpu().numpy()
        for row in gi:
            kept = row[row >= 0]
            assert len(set(kept.tolist())) == len(kept), "%s n=%d k=%d: an index twice in %r" % (kind, n, k, row.tolist())
        _assert_gather_equals((got[0], got[1], torch.from_numpy(_canonical_nan(got[2].cpu().numpy()))), (idx, dist, _canonical_nan(patch)),
                              "%s n=%d k=%d" % (kind, n, k))
        ran += 1
    assert ran == (6 if kind == "nan70" else 6 + 3)      # 200 points: six k; 64 points: the three k that fit, no index 70


@pytest.mark.parametrize("kind", ("nan-query", "huge-query"))
@pytest.mark.parametrize("k", (65, 100, 128))
def test_empty_entries_load_nothing_from_in_front_of_the_cloud(kind, k):
    """Fewer than k finite distances at k > 64 leave the second slot's entries empty.  The call runs in guarded buffers twice, the
    band in front of the cloud 0xFF and then 0x00: a gather through index -1 reads that band and the two outputs differ."""
    from sapcu_amd import _lib
    lib = _lib.load()
    n = 200
    c, q, _, _ = KC.bad_inputs(kind, n)
    idx, dist, patch = KC.reference(c, q, k)
    outs = []
    for fill in (0xFF, 0x00):
        A = Arena("guard", fill=fill, device=U.dev())
        Cl, Q = A.inp(c, offset=8, name="cloud"), A.inp(q, offset=8, name="queries")
        o = (A.out((9, k), I64, offset=8, name="idx_out"), A.out((9, k), F64, offset=8, name="dist_out"),
             A.out((9, k, 3), F32, offset=4, name="patch_out"))
        _lib.check(lib.sapcu_knn_gather_f64(_lib.ptr(Cl), n, _lib.ptr(Q), 9, k, _lib.ptr(o[0]), _lib.ptr(o[1]), _lib.ptr(o[2]),
                                            _lib.current_stream()))
        torch.cuda.synchronize()
        A.check()
        outs.append([t.cpu().numpy().copy() for t in o])
    for name, a, b in zip(("idx", "dist", "patch"), *outs):
        assert np.array_equal(_bits(a), _bits(b)), "%s depends on the bytes in front of the cloud" % name
    _assert_gather_equals([torch.from_numpy(a) for a in (outs[0][0], outs[0][1], _canonical_nan(outs[0][2]))],
                          (idx, dist, _canonical_nan(patch)), "%s k=%d" % (kind, k))


@pytest.mark.parametrize("cell", (0.0, 2.0 / 64))
def test_nearest_with_a_bad_point_in_the_first_slab(cell):
    """metrics.nearest with a NaN point at index 5, against numpy (not against knn_gather, the kernel it runs on this route)."""
    from sapcu_amd import metrics
    c, q, _, _ = KC.bad_inputs("nan5", 200)
    idx, dist, _ = KC.reference(c, q, 1)
    info = []
    gd, gi = metrics.nearest(_dev(q), _dev(c), cell_size=cell, info=info)
    assert info[0] == 0, "a non-finite cloud must take the brute-force route"
    assert np.array_equal(gi.cpu().numpy(), idx[:, 0]) and np.array_equal(_bits(gd.cpu().numpy()), _bits(dist[:, 0]))
    assert not (gi == 5).any()


@pytest.mark.parametrize("at", (5, 70))
def test_training_patches_of_a_non_finite_cloud_are_empty(at):
    """A NaN coordinate makes the cloud's centroid, so every normalised point and every distance, NaN: no candidate anywhere.  The
    rule then says index -1 and NaN rows in every entry (before it, the first slab's network left arbitrary indices there)."""
    from sapcu_amd import data
    clouds = KC.train_cloud().copy()
    clouds[0, at, 1] = np.nan
    for k in (1, 64, 65, 128):
        out = data.build_patches(_dev(clouds), _dev(np.zeros(1, np.int64)), k)
        assert (out["idx"] == -1).all(), (at, k)
        assert torch.isnan(out["patches"]).all(), (at, k)


class _NoModel:
    def eval(self):
        return self

    def __call__(self, *a, **kw):
        raise AssertionError("a model ran")


def test_the_python_entries_refuse_a_non_finite_cloud_before_any_launch(monkeypatch):
    """Generator3D6.generateiopoint / upsample_seeds and dist.upsample_cloud_sharded raise ValueError as the reference's KDTree does,
    on the host array, with nothing loaded or launched."""
    from sapcu_amd import _lib, dist, generation as gen

    def launched(*a, **kw):
        raise AssertionError("the library was reached")

    g = gen.Generator3D6(_NoModel(), _NoModel(), U.dev(), k_neighbors=48)
    monkeypatch.setattr(_lib, "load", launched)
    monkeypatch.setattr(g, "_dense_seeds", launched)
    monkeypatch.setattr(g, "refine", launched)
    good = KC.cloud("lattice7").copy()
    for bad in (np.nan, np.inf, -np.inf):
        cloud = good.copy()
        cloud[5, 1] = bad
        with pytest.raises(ValueError):
            g.generateiopoint(cloud)
        with pytest.raises(ValueError):
            g.upsample(cloud[None])
        with pytest.raises(ValueError):
            g.upsample_seeds(cloud, good[:9])
        with pytest.raises(ValueError):
            g.upsample_seeds(good, cloud[:9])
        with pytest.raises(ValueError):
            dist.upsample_cloud_sharded(g, cloud)
