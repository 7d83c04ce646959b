"""Fixture of the uniformity figures (tests/golden/uniformity.npz), made by RUNNING the reference's CGAL tool on the CPU.

Run where the reference tree is (make_mesh_fixtures.py's REF; it never travels with the suite):

    python tests/golden/make_uniformity_fixtures.py            # writes uniformity.npz
    python tests/golden/make_uniformity_fixtures.py --check    # rebuilds in memory and compares with the committed file

The prebuilt ``evaluation`` tool is copied to a temporary directory, given its execute bit and run there as
``evaluation mesh.off pred.xyz F seeds.txt`` exactly as make_mesh_fixtures.py does, this time with seeds in ``seeds.txt``
(rows ``id x1 x2 x3``; x1 weighs the face's THIRD vertex, x2 its first, x3 its second).  It prints the seven disk radii and writes
``pred_density.xyz``, one row of seven densities count / (n * fraction) per seed, six digits.  Only data is stored.

Cases: ico, box, sheet, torus take mesh and points from mesh_p2f.npz (read, not duplicated); bumpy is a 40 x 40 grid with
z = 0.04 sin 9x cos 7y (saddle vertices everywhere) and 4000 points near it; plate is a flat 24 x 24 grid less a 6 x 4 hole and an
8 x 8 corner notch, 3000 points over its own cells (a point over the hole projects onto the rim, and a rim point seen round a
corner of the hole is reached ALONG the rim: there the tool's floating-point answer came out above the rim path for 2 seeds of 48,
so such targets are no input to hold an exact count against).  48 seeds each, of the tool's
own distribution (area-weighted face, three U(0.01, 1) weights, normalised); box: every second seed within 2 % of an edge, every
fourth near a corner; plate: drawn in the faces around the hole and the notch.

Condition on the inputs, checked with tests/geodesic_ref.py when the fixture is made: every candidate's |d / r_j - 1| > 1e-6 for
all j.  A seed that violates it is redrawn and logged; at most 4 of 48 per case.

Stored per case ``<name>/seeds`` f64 [48,4] (the file's rows as read back), ``<name>/radii`` [7] and ``<name>/density`` [48,7] as
printed, ``<name>/counts`` int64 [48,7] = round(density * n * fraction), which must land within 0.01 of an integer; for bumpy and
plate also ``<name>/vertices``, ``<name>/faces``, ``<name>/points``; ``cases``; ``tool_seconds`` (the tool's own elapsed time per
case, on 16 threads).
"""
import os
import re
import shutil
import stat
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]
from make_mesh_fixtures import TOOL, write_off          # noqa: E402
import geodesic_ref as G                                # noqa: E402
import mesh_ref                                         # noqa: E402

OUT = os.path.join(HERE, "uniformity.npz")
CASES = ("ico", "box", "sheet", "torus", "bumpy", "plate")
NS = 48
PCT = G.TOOL_FRACTIONS.astype(np.float64)


def bumpy_mesh(n=40):
    xs = np.linspace(0.0, 1.0, n + 1)
    gx, gy = np.meshgrid(xs, xs, indexing="ij")
    v = np.stack([gx, gy, 0.04 * np.sin(9.0 * gx) * np.cos(7.0 * gy)], -1).reshape(-1, 3)
    idx = lambda i, j: i * (n + 1) + j
    f = []
    for i in range(n):
        for j in range(n):
            f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return v, np.array(f)


def plate_cells(n=24):
    """the cells (i, j) of the plate: the grid less the hole i in [8, 14), j in [10, 14) and the notch i, j >= 16"""
    return [(i, j) for i in range(n) for j in range(n) if not (8 <= i < 14 and 10 <= j < 14) and not (i >= 16 and j >= 16)]


def plate_mesh(n=24):
    xs = np.linspace(0.0, 1.0, n + 1)
    gx, gy = np.meshgrid(xs, xs, indexing="ij")
    v = np.stack([gx, gy, np.zeros_like(gx)], -1).reshape(-1, 3)
    idx = lambda i, j: i * (n + 1) + j
    f = []
    for i, j in plate_cells(n):
        f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    f = np.array(f)
    used = np.unique(f)
    remap = -np.ones(len(v), np.int64)
    remap[used] = np.arange(len(used))
    return v[used], remap[f]


def generated(name):
    rng = np.random.default_rng({"bumpy": 41, "plate": 42}[name])
    if name == "bumpy":
        v, f = bumpy_mesh()
        xy = rng.uniform(0.0, 1.0, size=(4000, 2))
        p = np.concatenate([xy, (0.04 * np.sin(9.0 * xy[:, :1]) * np.cos(7.0 * xy[:, 1:]) + rng.normal(size=(4000, 1)) * 0.003)], -1)
    else:
        v, f = plate_mesh()
        xy = rng.uniform(0.0, 1.0, size=(6000, 2))
        cells = set(plate_cells())
        xy = np.array([q for q in xy if (min(int(q[0] * 24), 23), min(int(q[1] * 24), 23)) in cells])[:3000]
        assert len(xy) == 3000
        p = np.concatenate([xy, rng.normal(size=(3000, 1)) * 0.003], -1)
    return v, f, p


def face_areas(v, f):
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return 0.5 * np.sqrt(np.sum(n * n, -1))


def draw_seed(name, i, rng, v, f, area_cdf):
    """one seed (face, weights in the face's own vertex order)"""
    w = rng.uniform(0.01, 1.0, 3)
    w /= w.sum()
    face = int(np.searchsorted(area_cdf, rng.uniform(0.0, 1.0), side="right"))
    face = min(face, len(f) - 1)
    if name == "box":
        if i % 4 == 1:                                      # near a corner: one weight carries 97 %
            w = np.array([0.97, 0.02, 0.01])[rng.permutation(3)]
        elif i % 2 == 1:                                    # within 2 % of an edge
            t = rng.uniform(0.1, 0.9)
            w = np.array([t * 0.985, (1 - t) * 0.985, 0.015])[rng.permutation(3)]
    if name == "plate":                                     # faces whose centroid lies within 0.1 of the hole or the notch
        c = v[f].mean(1)[:, :2]
        box = lambda lo, hi: np.maximum(np.maximum(lo[0] - c[:, 0], c[:, 0] - hi[0]), np.maximum(lo[1] - c[:, 1], c[:, 1] - hi[1]))
        near = np.nonzero((box((8 / 24, 10 / 24), (14 / 24, 14 / 24)) < 0.1) | (box((16 / 24, 16 / 24), (1.0, 1.0)) < 0.1))[0]
        face = int(near[rng.integers(0, len(near))])
    return face, w


def seed_row(face, w):
    return "%d %.17g %.17g %.17g" % (face, w[2], w[0], w[1])


def margin_ok(mesh, tpoint, tface, face, w, radii):
    d = G.geodesic_from_seed(mesh, face, w, tpoint, tface, float(radii[-1]) * (1 + 2e-6))
    d = d[np.isfinite(d)]
    return bool(np.all(np.abs(d[:, None] / radii[None, :] - 1.0) > 1e-6))


def run_tool(tool, tmp, name):
    res = subprocess.run([tool, name + ".off", name + ".xyz", "F", "seeds.txt"], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True)
    if res.returncode != 0:
        raise RuntimeError("case %s: the tool exited %d\n%s\n%s" % (name, res.returncode, res.stdout[-2000:], res.stderr[-2000:]))
    m = re.search(r"The disk radius are:((?:\s+\S+){7})", res.stdout)
    t = re.search(r"elapsed time:\s*(\S+)s", res.stdout)
    dens = np.loadtxt(os.path.join(tmp, name + "_density.xyz"), ndmin=2)
    if not (m and t):
        raise RuntimeError("case %s: unexpected output\n%s" % (name, res.stdout[-2000:]))
    return np.array([float(x) for x in m.group(1).split()]), dens, float(t.group(1))


def build():
    p2f = np.load(os.path.join(HERE, "mesh_p2f.npz"))
    out = {"cases": np.array(CASES)}
    seconds = []
    with tempfile.TemporaryDirectory() as tmp:
        tool = os.path.join(tmp, "evaluation")
        shutil.copyfile(TOOL, tool)
        os.chmod(tool, os.stat(tool).st_mode | stat.S_IXUSR)
        for ci, name in enumerate(CASES):
            if name + "/vertices" in p2f.files:
                v, f, p = p2f[name + "/vertices"], p2f[name + "/faces"].astype(np.int64), p2f[name + "/points"]
                np.savetxt(os.path.join(tmp, name + ".xyz"), p, fmt="%.17g")           # a round trip of every f64
            else:
                v, f, p = generated(name)
                np.savetxt(os.path.join(tmp, name + ".xyz"), p, fmt="%.6f")
                out[name + "/vertices"], out[name + "/faces"] = v, f.astype(np.int32)
            write_off(os.path.join(tmp, name + ".off"), v, f)
            p = np.loadtxt(os.path.join(tmp, name + ".xyz"), ndmin=2)[:, :3]           # what the tool reads
            if name + "/vertices" not in p2f.files:
                out[name + "/points"] = np.ascontiguousarray(p)
            _, tface, tpoint, _, _ = mesh_ref.point_mesh(p, v, f)
            mesh = G.Mesh(v, f)
            radii = G.disk_radii(v, f)
            rng = np.random.default_rng(500 + ci)
            cdf = np.cumsum(face_areas(v, f))
            cdf /= cdf[-1]
            rows, redrawn = [], 0
            for i in range(NS):
                while True:
                    face, w = draw_seed(name, i, rng, v, f, cdf)
                    row = np.array(seed_row(face, w).split(), np.float64)               # as the file holds it
                    sf, sb = G.tool_rows_to_seeds(row)
                    if margin_ok(mesh, tpoint, tface, int(sf[0]), sb[0], radii):
                        break
                    redrawn += 1
                    print("%s: seed %d redrawn (a candidate within 1e-6 of a radius)" % (name, i))
                rows.append(seed_row(face, w))
            assert redrawn <= 4, (name, redrawn)
            with open(os.path.join(tmp, "seeds.txt"), "w") as fh:
                fh.write("\n".join(rows) + "\n")
            seeds = np.loadtxt(os.path.join(tmp, "seeds.txt"), ndmin=2)
            printed, dens, secs = run_tool(tool, tmp, name)
            assert dens.shape == (NS, 7), (name, dens.shape)
            raw = dens * (len(p) * PCT)[None, :]
            counts = np.rint(raw).astype(np.int64)
            worst = float(np.abs(raw - counts).max())
            assert worst < 0.01, (name, worst)
            print("%-6s %5d faces %5d points  tool elapsed %.3f s  recovery off an integer by at most %.1e  redrawn %d"
                  % (name, len(f), len(p), secs, worst, redrawn))
            out[name + "/seeds"], out[name + "/radii"], out[name + "/density"], out[name + "/counts"] = seeds, printed, dens, counts
            seconds.append(secs)
    out["tool_seconds"] = np.array(seconds)
    return out


def main():
    out = build()
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out)
        for k in out:
            if k != "tool_seconds":
                assert np.array_equal(old[k], out[k]), k
        print("uniformity.npz reproduced (%d arrays)" % len(out))
        return
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
