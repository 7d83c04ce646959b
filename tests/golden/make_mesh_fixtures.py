"""Fixture of the point-to-surface distance (tests/golden/mesh_p2f.npz), made by RUNNING the reference's CGAL tool on the CPU.

Run in the build container only (needs /root/reference, which never travels, and numpy):

    python tests/golden/make_mesh_fixtures.py            # writes mesh_p2f.npz
    python tests/golden/make_mesh_fixtures.py --check    # rebuilds in memory and compares with the committed file

The prebuilt ``external/Meta-PU_evaluation/evaluation_code/build/evaluation`` is copied to a temporary directory (it only lacks its
execute bit) and run there as ``evaluation mesh.off pred.xyz F seeds.txt`` with an empty ``seeds.txt``, which skips the uniformity
part.  It writes ``pred_point2mesh_distance.xyz`` (x y z distance, six significant digits, the distance held as ``float``) and
prints the face count and ``Mean: .. std: .. min: .. max: ..`` (std: the sample one, n - 1).  NOTHING is written if the binary does
not run or a case does not exit 0.  No text of the reference is stored: only data its program read and wrote.

Cases (valid 2-manifold triangle meshes only; CGAL's Surface_mesh reader rejects others):
  ico    the reference's own external/SPU-PMD/evaluation_code/Icosahedron.off (2562 vertices, 5120 faces) and Icosahedron.xyz (8192
         points), both as they lie there;
  box    the unit cube as 12 triangles, 2000 points drawn from [-2, 3]^3: every region of the triangle wins, ties are the rule;
  sheet  an open, wavy 16 x 12 sheet with a boundary (384 faces), 1500 points on both sides and beyond the rim;
  torus  a 64 x 32 torus (4096 faces), 3000 points: half of them within 0.01 of the surface, half anywhere in its box and beyond.
Generated vertices are written with %.17g (a round trip of every f64); generated points are written with %.6f and READ BACK from
that text, so the fixture holds what the tool read.

Stored per case ``<name>/vertices`` f64 [nv,3], ``<name>/faces`` int32 [nf,3], ``<name>/points`` f64 [nq,3], ``<name>/dist`` f64 [nq]
(the distance column as parsed), ``<name>/stats`` = [mean, std, min, max] as printed, ``<name>/n_faces`` as printed; ``cases``.
"""
import glob
import os
import re
import shutil
import stat
import subprocess
import sys
import tempfile
import time

import numpy as np

REF = "/root/reference"
TOOL = os.path.join(REF, "external", "Meta-PU_evaluation", "evaluation_code", "build", "evaluation")
ICO = os.path.join(REF, "external", "SPU-PMD", "evaluation_code", "Icosahedron")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesh_p2f.npz")
CASES = ("ico", "box", "sheet", "torus")


def box_mesh():
    v = np.array([[x, y, z] for z in (0.0, 1.0) for y in (0.0, 1.0) for x in (0.0, 1.0)])
    f = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2],
                  [1, 3, 7], [1, 7, 5]])
    return v, f


def sheet_mesh(nx=16, ny=12):
    xs, ys = np.linspace(0.0, 1.0, nx + 1), np.linspace(0.0, 0.75, ny + 1)
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    v = np.stack([gx, gy, 0.05 * np.sin(5.0 * gx) * np.cos(4.0 * gy)], -1).reshape(-1, 3)
    idx = lambda i, j: i * (ny + 1) + j
    f = []
    for i in range(nx):
        for j in range(ny):
            f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return v, np.array(f)


def torus_mesh(nu=64, nw=32, R=0.35, r=0.12):
    u, w = np.arange(nu) * (2 * np.pi / nu), np.arange(nw) * (2 * np.pi / nw)
    gu, gw = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(gw)) * np.cos(gu), (R + r * np.cos(gw)) * np.sin(gu), r * np.sin(gw)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nw + (j % nw)
    f = []
    for i in range(nu):
        for j in range(nw):
            f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return v, np.array(f)


def generated(name):
    rng = np.random.default_rng({"box": 31, "sheet": 32, "torus": 33}[name])
    if name == "box":
        v, f = box_mesh()
        p = rng.uniform(-2.0, 3.0, size=(2000, 3))
    elif name == "sheet":
        v, f = sheet_mesh()
        p = np.stack([rng.uniform(-0.3, 1.3, 1500), rng.uniform(-0.3, 1.05, 1500), rng.uniform(-0.3, 0.3, 1500)], -1)
    else:
        v, f = torus_mesh()
        on = v[rng.integers(0, len(v), 1500)] + rng.normal(size=(1500, 3)) * 0.005
        p = np.concatenate([on, rng.uniform(-0.7, 0.7, size=(1500, 3))])[rng.permutation(3000)]
    return v, f, p


def write_off(path, v, f):
    with open(path, "w") as out:
        out.write("OFF\n%d %d 0\n" % (len(v), len(f)))
        for row in v:
            out.write("%.17g %.17g %.17g\n" % tuple(row))
        for row in f:
            out.write("3 %d %d %d\n" % tuple(row))


def run_tool(tool, tmp, name):
    """-> (distance rows [nq,4] as parsed, [mean, std, min, max], face count, wall seconds)"""
    for old in glob.glob(os.path.join(tmp, "*_point2mesh_distance.xyz")):
        os.remove(old)
    t0 = time.perf_counter()
    res = subprocess.run([tool, name + ".off", name + ".xyz", "F", "seeds.txt"], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True)
    wall = time.perf_counter() - t0
    if res.returncode != 0:
        raise RuntimeError("case %s: the tool exited %d\n%s\n%s" % (name, res.returncode, res.stdout[-2000:], res.stderr[-2000:]))
    m = re.search(r"Mean:\s*(\S+)\s+std:\s*(\S+)\s+min:\s*(\S+)\s+max:\s*(\S+)", res.stdout)
    nf = re.search(r"This mesh has\s+(\d+)\s+faces", res.stdout)
    outs = glob.glob(os.path.join(tmp, "*_point2mesh_distance.xyz"))
    if not (m and nf and len(outs) == 1):
        raise RuntimeError("case %s: unexpected output\n%s" % (name, res.stdout[-2000:]))
    rows = np.loadtxt(outs[0], ndmin=2)
    return rows, np.array([float(m.group(k)) for k in range(1, 5)]), int(nf.group(1)), wall


def build():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from sapcu_amd.mesh import read_off
    assert os.path.exists(TOOL), TOOL
    out = {"cases": np.array(CASES)}
    with tempfile.TemporaryDirectory() as tmp:
        tool = os.path.join(tmp, "evaluation")
        shutil.copyfile(TOOL, tool)
        os.chmod(tool, os.stat(tool).st_mode | stat.S_IXUSR)
        open(os.path.join(tmp, "seeds.txt"), "w").close()
        for name in CASES:
            if name == "ico":
                shutil.copyfile(ICO + ".off", os.path.join(tmp, "ico.off"))
                shutil.copyfile(ICO + ".xyz", os.path.join(tmp, "ico.xyz"))
                v, f = read_off(os.path.join(tmp, "ico.off"))
            else:
                v, f, p = generated(name)
                write_off(os.path.join(tmp, name + ".off"), v, f)
                np.savetxt(os.path.join(tmp, name + ".xyz"), p, fmt="%.6f")
                v2, f2 = read_off(os.path.join(tmp, name + ".off"))
                assert np.array_equal(v2, v) and np.array_equal(f2, f)
            p = np.loadtxt(os.path.join(tmp, name + ".xyz"), ndmin=2)[:, :3]       # what the tool reads
            rows, stats, nf, wall = run_tool(tool, tmp, name)
            assert rows.shape == (len(p), 4) and nf == len(f), (name, rows.shape, nf)
            assert np.allclose(rows[:, :3], p, rtol=1e-5, atol=1e-6), name        # same points in the same order (six digits)
            print("%-6s %5d vertices %5d faces %5d points  tool wall %.3f s  mean %g std %g min %g max %g"
                  % (name, len(v), len(f), len(p), wall, *stats))
            out[name + "/vertices"], out[name + "/faces"], out[name + "/points"] = v, f.astype(np.int32), np.ascontiguousarray(p)
            out[name + "/dist"], out[name + "/stats"], out[name + "/n_faces"] = rows[:, 3].copy(), stats, np.int64(nf)
    return out


def main():
    out = build()
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out)
        for k in out:
            assert np.array_equal(old[k], out[k]), k
        print("mesh_p2f.npz reproduced (%d arrays)" % len(out))
        return
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
