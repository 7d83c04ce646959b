"""The conditions of tests/klist_cases.py, checked without a GPU: the sweeps of tests/test_gpu_klist.py decide ties by the
(distance, index) rule only if every squared distance is exact, only where ties sit inside the first k + 1 distances, and only if
the reference covers every case and states the rule for non-finite distances as include/sapcu.h does."""
import numpy as np

import klist_cases as KC
from oracle import geom_path as G


def _exact_dist2(c, q):
    """The squared distances as integers / 128^2, in integer arithmetic."""
    ci, qi = np.rint(c * 128).astype(np.int64), np.rint(q * 128).astype(np.int64)
    assert (ci == c * 128).all() and (qi == q * 128).all(), "a coordinate is no multiple of 1/128"
    d = qi[:, None, :] - ci[None, :, :]
    return (d * d).sum(-1)


def _all_cuts():
    return sorted({(name, n) for name, n, _ in list(KC.small_cases()) + list(KC.tile_cases())})


def test_the_sweeps_cover_what_they_claim():
    small, tile, grid, bad = list(KC.small_cases()), list(KC.tile_cases()), list(KC.grid_cases()), list(KC.bad_cases())
    for name, n_whole in (("lattice7", 343), ("dup4", 320), ("line", 300)):
        assert len(KC.cloud(name)) == n_whole
        ks = sorted({k for nm, _, k in small if nm == name})
        assert ks == list(range(1, 129)), name
        for k in (1, 63, 64, 65, 128):
            assert sorted(n for nm, n, kk in small if nm == name and kk == k) == sorted({n_whole, k, 64, 65} - set(range(k))), (name, k)
    assert len(small) == len(set(small)) and len(small) == sum(len(KC.cuts(len(KC.cloud(nm)), k)) for nm in ("lattice7", "dup4", "line")
                                                              for k in range(1, 129))
    assert len(KC.cloud("lattice11")) == 1331 and len(tile) == 24
    assert len(grid) == 128
    # 6 kinds at 200 points and the 6 k values, 5 kinds (index 70 does not exist) at 64 points and the 3 k values that fit
    assert len(bad) == 6 * 6 + 5 * 3
    assert KC.train_cloud().shape == (1, 193, 3) and KC.train_cloud().dtype == np.float32
    assert (KC.train_cloud() * 64 == np.rint(KC.train_cloud() * 64)).all()


def test_every_squared_distance_is_exact():
    for name, n in _all_cuts():
        c, q, _ = KC.cut_with_queries(name, n)
        assert q.shape == (9, 3)
        exact = _exact_dist2(c, q)
        assert exact.max() < 2 ** 52
        assert (KC.dist2(c, q) * 16384.0 == exact).all(), (name, n)


def test_every_case_has_ties_inside_its_first_k_plus_one_distances():
    """Rows 4..8 are the centres: each has two (on a whole lattice up to eight) nearest points at one distance."""
    for name, n, k in list(KC.small_cases()) + list(KC.tile_cases()):
        if n < 2:
            continue
        c, q, _ = KC.cut_with_queries(name, n)
        d = np.sort(_exact_dist2(c, q[4:]), axis=1)[:, :min(k + 1, n)]
        assert (np.diff(d, axis=1) == 0).any(axis=1).all(), (name, n, k)
    for name in ("lattice7", "lattice11"):                               # the whole lattices: eight-fold ties at three cell centres
        c, q, _ = KC.cut_with_queries(name, len(KC.cloud(name)))
        d = np.sort(_exact_dist2(c, q[4:7]), axis=1)
        assert (d[:, :8] == d[:, :1]).all() and (d[:, 8] > d[:, 0]).all(), name
    for name, k in KC.grid_cases():                                      # the grid sweep: every point is a query, of every point
        if name == "lattice7" and k == 1:                                # (a lattice point is alone at distance 0; from k = 2 on its
            continue                                                     # three or more neighbours at one edge length tie)
        c = KC.cloud(name)
        d = np.sort(_exact_dist2(c, c), axis=1)[:, :k + 1]
        assert (np.diff(d, axis=1) == 0).any(axis=1).all(), (name, k)


def test_the_reference_leaves_no_case_out():
    for name, n in _all_cuts():
        c, q, (idx, dist, patch) = KC.cut_with_queries(name, n)
        kmax = min(KC.K_MAX, n)
        assert idx.shape == (9, kmax) and dist.shape == (9, kmax) and patch.shape == (9, kmax, 3) and patch.dtype == np.float32
        assert (idx >= 0).all() and (idx < n).all() and np.isfinite(dist).all() and np.isfinite(patch).all()
        assert all(len(set(row.tolist())) == kmax for row in idx)
        assert np.array_equal(idx, G.knn_bruteforce(c, q, kmax))
        exact = np.take_along_axis(_exact_dist2(c, q), idx, axis=1)
        assert (np.diff(exact, axis=1) >= 0).all()
        assert ((np.diff(exact, axis=1) > 0) | (np.diff(idx, axis=1) > 0)).all(), "ties are not in ascending index"
        assert (dist == np.sqrt(exact / 16384.0)).all()
        for k in (1, kmax // 2 + 1):                                     # a prefix of the stable sort is the shorter sort
            assert np.array_equal(KC.reference_at(name, n, k)[2], G.knn_bruteforce(c, q, k))


def test_the_reference_states_the_rule_for_non_finite_distances():
    for kind, n, k in KC.bad_cases():
        c, q, c0, q0 = KC.bad_inputs(kind, n)
        idx, dist, patch = KC.reference(c, q, k)
        clean = KC.reference(c0, q0, k)
        empty = idx < 0
        assert (np.isposinf(dist) == empty).all() and (np.isnan(patch).all(-1) == empty).all() and not np.isnan(dist).any()
        assert not np.isnan(patch[~empty]).any()
        assert (np.diff(empty.astype(int), axis=1) >= 0).all(), "an empty entry in front of a finite one"
        for row in idx:
            kept = row[row >= 0]
            assert len(set(kept.tolist())) == len(kept)
        if kind.endswith("query"):                                       # the bad row is empty, the others are the clean ones
            assert empty[KC.BAD_QUERY_ROW].all()
            rows = np.arange(9) != KC.BAD_QUERY_ROW
            for got, ref in zip((idx, dist, patch), clean):
                assert np.array_equal(got[rows], ref[rows])
        else:                                                            # the cloud without the bad point, its indices shifted back
            b = int(kind.lstrip("nanifhuge"))
            assert not (idx == b).any()
            assert (empty.sum(1) == max(0, k - (n - 1))).all()
            keep = np.arange(n) != b
            if k <= n - 1:
                ridx, rdist, rpatch = KC.reference(c0[keep], q0, k)
                assert np.array_equal(idx, np.arange(n)[keep][ridx]) and np.array_equal(dist, rdist) and np.array_equal(patch, rpatch)
