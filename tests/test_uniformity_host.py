"""Uniformity without a GPU: the definition (tests/geodesic_ref.py) against the reference tool's counts (tests/golden/uniformity.npz)
and against analytic geodesics, and the host parts of sapcu_amd/uniformity.py (radii, seeds, seed files, the NUC arithmetic)."""
import numpy as np
import pytest

import geodesic_ref as G
import uniformity_cases as C


@pytest.mark.parametrize("name", C.CASES)
def test_the_definition_reproduces_every_count_of_the_tool(name, tmp_path):
    """All 48 seeds x 7 radii, with the seeds taken from the fixture's rows through write-as-the-file / read_seeds."""
    from sapcu_amd import uniformity
    c = C.case(name)
    path = str(tmp_path / "seeds.txt")
    with open(path, "w") as f:
        f.writelines("%d %.17g %.17g %.17g\n" % (r[0], r[1], r[2], r[3]) for r in c["rows"])
    sf, sb = uniformity.read_seeds(path)
    rf, rb = G.tool_rows_to_seeds(c["rows"])
    assert np.array_equal(sf, rf) and np.array_equal(sb, rb)
    counts, _ = C.oracle(name)
    assert counts.shape == c["counts"].shape == (48, 7)
    assert np.array_equal(counts, c["counts"]), int((counts != c["counts"]).sum())
    assert counts[:, -1].max() > 0


@pytest.mark.parametrize("name", C.CASES)
def test_disk_radii_are_the_printed_ones_to_their_six_digits(name):
    from sapcu_amd import uniformity
    c = C.case(name)
    r = uniformity.disk_radii(c["vertices"], c["faces"])
    assert r.dtype == np.float64 and np.array_equal(r, r.astype(np.float32).astype(np.float64))       # float32 values
    assert np.allclose(r, c["radii"], rtol=5e-6, atol=0)
    assert np.array_equal(r, G.disk_radii(c["vertices"], c["faces"]))
    assert np.array_equal(uniformity.TOOL_FRACTIONS, G.TOOL_FRACTIONS)
    d = c["counts"] / (len(c["points"]) * uniformity.TOOL_FRACTIONS.astype(np.float64))[None, :]
    assert np.allclose(d, c["density"], rtol=5e-6, atol=1e-12)


def test_on_a_flat_grid_the_geodesic_is_the_straight_distance():
    v, f, tpoint, tface, sf, sb, ref = C.flat_case()
    _, dist = G.geodesic_disks(v, f, tpoint, tface, sf, sb, [0.3, 0.6], return_dist=True)
    C.agree(dist, ref, 0.6, 1e-12)
    assert (ref <= 0.6).sum() > 500


def test_on_the_plate_the_geodesic_bends_round_the_corners_of_the_hole_and_the_notch():
    v, f, tpoint, tface, sf, sb, radii, ref = C.plate_case()
    counts, dist = G.geodesic_disks(v, f, tpoint, tface, sf, sb, radii, return_dist=True)
    C.agree(dist, ref, radii[-1], 1e-9)
    straight = np.sqrt(((C.seed_points(v, f, sf, sb)[:, None, :] - tpoint[None, :, :]) ** 2).sum(-1))
    bent = (ref <= radii[-1]) & (ref > straight * (1 + 1e-6))
    assert bent.sum() > 50                                              # the case is about paths that bend
    assert np.array_equal(counts, (ref[:, :, None] <= radii[None, None, :]).sum(1))


def test_on_the_cube_the_geodesic_is_the_shortest_unfolding():
    v, f, sf, sb, tpoint, tface, ref = C.cube_case()
    _, dist = G.geodesic_disks(v, f, tpoint, tface, sf, sb, [2.0], return_dist=True)
    got = dist[np.arange(len(ref)), np.arange(len(ref))]
    assert np.allclose(got, ref, rtol=1e-12, atol=0), (got, ref)
    straight_across = [np.hypot(1 + q[2] - p[0], q[1] - p[1]) for p, q in C.CUBE_PAIRS]
    assert ref[1] < straight_across[1] - 1e-3 and ref[2] < straight_across[2] - 1e-3      # two of the paths go round a corner


def test_non_manifold_and_zero_area_meshes_are_refused_by_the_definition():
    v, f = C.cube_mesh()
    with pytest.raises(ValueError):
        G.Mesh(v, np.concatenate([f, [[0, 3, 2]]]))                      # a face on an edge that already has two: a direction twice
    with pytest.raises(ValueError):
        G.Mesh(v, np.concatenate([f[:1], [f[1][[0, 2, 1]]]]))            # two faces crossing their edge in the same direction
    with pytest.raises(ValueError):
        G.Mesh(v, np.concatenate([f, [[0, 0, 1]]]))


def test_nuc_is_numpy_s_population_standard_deviation():
    from sapcu_amd import uniformity
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 200, (57, 7))
    fr = uniformity.TOOL_FRACTIONS.astype(np.float64)
    radii = np.arange(1.0, 8.0)
    m = uniformity._figures(counts, 8192, fr, radii)
    density = counts / (np.float64(8192) * fr)[None, :]
    assert np.array_equal(m["density"], density) and np.array_equal(m["counts"], counts)
    assert np.array_equal(m["nuc"], np.std(density, 0)) and np.array_equal(m["mean_density"], np.mean(density, 0))
    assert m["n_pre"] == 8192 and m["n_seeds"] == 57 and m["radii"] is radii
    other = uniformity._figures(rng.integers(0, 50, (9, 7)), 2048, fr, radii)
    pooled = uniformity.dataset_uniformity([m, other])
    both = np.concatenate([m["density"], other["density"]])
    assert np.array_equal(pooled["nuc"], np.std(both, 0)) and np.array_equal(pooled["mean_density"], both.mean(0))
    assert pooled["n_seeds"] == 66 and pooled["n_pre"] == 8192 + 2048
    with pytest.raises(ValueError):
        uniformity.dataset_uniformity([])


def test_seed_files_round_trip_with_the_tool_s_weight_order(tmp_path):
    from sapcu_amd import uniformity
    faces = np.array([5, 0, 11])
    bary = np.array([[0.2, 0.3, 0.5], [0.6, 0.3, 0.1], [1 / 3, 1 / 3, 1 / 3]])
    path = str(tmp_path / "s.txt")
    uniformity.write_seeds(path, faces, bary)
    rows = np.loadtxt(path, ndmin=2)
    assert np.array_equal(rows[:, 0], faces)
    assert np.array_equal(rows[:, 1], bary[:, 2]) and np.array_equal(rows[:, 2], bary[:, 0]) and np.array_equal(rows[:, 3], bary[:, 1])
    f2, b2 = uniformity.read_seeds(path)
    assert np.array_equal(f2, faces) and f2.dtype == np.int64 and np.array_equal(b2, bary)
    with open(path, "w") as f:
        f.write("1 0.5 0.5\n")
    with pytest.raises(ValueError):
        uniformity.read_seeds(path)


def test_random_seeds_follow_the_tool_s_distribution():
    from sapcu_amd import uniformity
    v, f = C.plate_mesh()
    v2 = np.concatenate([v, [[2.0, 0, 0], [4.0, 0, 0], [2.0, 2.0, 0]]])          # one large face: 2 of 2.847.. of the area
    f2 = np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]])
    faces, bary = uniformity.uniformity_seeds(v2, f2, 4000, generator=11)
    assert faces.dtype == np.int64 and bary.shape == (4000, 3)
    assert np.allclose(bary.sum(-1), 1.0, rtol=0, atol=1e-15) and bary.min() >= 0.01 / 2.01 - 1e-15
    share = np.mean(faces == len(f))
    area = 2.0 + len(f) * 0.5 / 576
    assert abs(share - 2.0 / area) < 4 * np.sqrt(0.25 / 4000)                    # four standard deviations of a share
    again = uniformity.uniformity_seeds(v2, f2, 4000, generator=np.random.default_rng(11))
    assert np.array_equal(again[0], faces) and np.array_equal(again[1], bary)
