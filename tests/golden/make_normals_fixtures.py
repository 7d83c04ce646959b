"""Fixture of the PCA normals and the normal angles (tests/golden/pca_normals.npz), made by RUNNING the reference's scripts on the CPU.

Run in the build container only (needs /root/reference, which never travels, sklearn and numpy):

    python tests/golden/make_normals_fixtures.py            # writes pca_normals.npz
    python tests/golden/make_normals_fixtures.py --check    # rebuilds in memory and compares with the committed file

``scripts/generate_gt_normals.py`` is run from where it lies, as a subprocess, unchanged: its working directory is a temporary
directory and so is its ``argv[1]``, where the clouds lie as ``.xyz`` written with ``%.17g``.  Stored per cloud are the ``points``
and ``normals`` of the ``.npz`` it saved next to each cloud, both f32 as it stores them.  ``angular_error_deg`` of
``scripts/old_metrics/eval_normals.py`` (whose module needs the reference's training packages to import) is compiled from the file
where it lies, that one function, and called on random normal tables; stored are the tables and the angles it returned.  No text of
the reference is stored: only data its programs read and wrote.

Checked before anything is written (tests/normals_ref.py is this project's definition in numpy):
  * sklearn's neighbour sets on the f32 points equal the brute-force ones in f64, and the k-th and (k+1)-th distances differ: no
    result hangs on a tie;
  * every row of every cloud has (l1 - l0) / l2 >= 0.05 (l0 <= l1 <= l2 the eigenvalues of the definition's covariance): the
    condition of the comparison leaves no row out;
  * B, the largest sin(angle between the script's normal and the definition's) * (l1 - l0) / (2^-23 * l2) over all rows.  The script
    centres and stores in f32, so the difference is f32 rounding (2^-23 relative) amplified by l2 / (l1 - l0), not the algorithm's
    error.  Stored as ``B``; the tests assert 4 B.

Stored: ``clouds`` (names); per cloud ``<name>/points``, ``<name>/normals`` (f32 [n,3]) and ``<name>/min_gap``; ``B``; ``k``;
``angles/a``, ``angles/b`` (f64 [m,3]) and ``angles/deg`` (f64 [m]).
"""
import ast
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import normals_ref as R  # noqa: E402

REF = "/root/reference"
SCRIPT = os.path.join(REF, "scripts", "generate_gt_normals.py")
ANGLE_SCRIPT = os.path.join(REF, "scripts", "old_metrics", "eval_normals.py")
OUT = os.path.join(HERE, "pca_normals.npz")
K = 16
MIN_GAP = 0.05
CLOUDS = {"shell300": lambda: R.shell(300)[0], "shell5000": lambda: R.shell(5000)[0], "torus2000": lambda: R.torus(2000)}


def script_normals(clouds):
    """{name: (points f32, normals f32)} as the script saved them."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, p in clouds.items():
            np.savetxt(os.path.join(tmp, name + ".xyz"), p, fmt="%.17g")
            assert np.array_equal(np.loadtxt(os.path.join(tmp, name + ".xyz")), p)
        run = subprocess.run([sys.executable, SCRIPT, tmp], cwd=tmp, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             universal_newlines=True)
        assert "Failed" not in run.stdout, run.stdout
        for name in clouds:
            with np.load(os.path.join(tmp, name + ".npz")) as d:
                out[name] = (d["points"], d["normals"])
            with np.load(os.path.join(tmp, "out", "tmp_eval", name + ".npz")) as d:
                assert np.array_equal(d["normals"], out[name][1])
    return out


def script_angle_function():
    """``angular_error_deg`` compiled from the reference's file, that function alone."""
    with open(ANGLE_SCRIPT) as f:
        tree = ast.parse(f.read(), ANGLE_SCRIPT)
    fn = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "angular_error_deg"]
    assert len(fn) == 1
    space = {"np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), ANGLE_SCRIPT, "exec"), space)
    return space["angular_error_deg"]


def angle_tables(m=4096, seed=21):
    """Random pairs: unit and unnormalised rows (lengths 1e-6 .. 1e6), equal and opposite rows, zero rows on either side."""
    rng = np.random.default_rng(seed)
    a, b = rng.normal(size=(m, 3)), rng.normal(size=(m, 3))
    a[: m // 2] /= np.linalg.norm(a[: m // 2], axis=1, keepdims=True)
    b[: m // 4] /= np.linalg.norm(b[: m // 4], axis=1, keepdims=True)
    a[m // 2:] *= 10.0 ** rng.uniform(-6, 6, size=(m - m // 2, 1))
    b[64:128] = a[64:128]
    b[128:192] = -a[128:192]
    b[192:256] = a[192:256] * 3.0
    a[256:272] = 0.0
    b[272:288] = 0.0
    a[288:296] = b[288:296] = 0.0
    return a, b


def compare(points32, normals32, k=K):
    """(gap = (l1 - l0) / l2, ratio = sin * gap / 2^-23) per row of the script's normals against the definition on the f32 points."""
    p = points32.astype(np.float64)
    idx = R.brute_knn(p, k)
    mine, evals, bad = R.pca_normals(p, idx)
    assert bad == 0
    gap = (evals[:, 1] - evals[:, 0]) / evals[:, 2]
    sin = R.sin_angle(normals32.astype(np.float64), mine)
    return gap, sin * gap / 2.0 ** -23, idx


def build():
    from sklearn.neighbors import NearestNeighbors
    assert os.path.exists(SCRIPT) and os.path.exists(ANGLE_SCRIPT), REF
    clouds = {name: make() for name, make in CLOUDS.items()}
    saved = script_normals(clouds)
    out = {"clouds": np.array(sorted(clouds)), "k": np.int64(K)}
    worst = 0.0
    for name in sorted(clouds):
        p32, n32 = saved[name]
        assert p32.dtype == np.float32 and n32.dtype == np.float32 and p32.shape == n32.shape == clouds[name].shape
        assert np.array_equal(p32, clouds[name].astype(np.float32))
        gap, ratio, idx = compare(p32, n32)
        sk = NearestNeighbors(n_neighbors=K).fit(p32).kneighbors(p32)[1]
        assert np.array_equal(np.sort(sk, axis=1), np.sort(idx, axis=1)), "%s: sklearn's neighbour sets are not the brute-force ones" % name
        p = p32.astype(np.float64)
        far = R.brute_knn(p, K + 1)
        d = lambda col: np.linalg.norm(p - p[far[:, col]], axis=1)
        assert (d(K) > d(K - 1)).all(), "%s: the k-th distance ties with the next" % name
        assert gap.min() >= MIN_GAP, "%s: (l1 - l0) / l2 goes down to %g: rows would be left out" % (name, gap.min())
        print("%-10s n = %5d  min (l1-l0)/l2 = %.3f  worst sin * gap / 2^-23 = %.3f  mean |cos| to the script = %.9f"
              % (name, len(p32), gap.min(), ratio.max(), np.abs((n32 * R.pca_normals(p, idx)[0]).sum(1)).mean()))
        worst = max(worst, float(ratio.max()))
        out[name + "/points"], out[name + "/normals"], out[name + "/min_gap"] = p32, n32, np.float64(gap.min())
    out["B"] = np.float64(worst)
    a, b = angle_tables()
    deg = script_angle_function()(a.copy(), b.copy())
    mine = R.angles(a, b)[0]
    assert np.array_equal(deg.view(np.int64), mine.view(np.int64)), "the angle mirror is not the script's function"
    out["angles/a"], out["angles/b"], out["angles/deg"] = a, b, deg
    print("B = %.4f; %d angle rows, equal to the mirror bit for bit" % (worst, len(deg)))
    return out


def main():
    out = build()
    if "--check" in sys.argv[1:]:
        with np.load(OUT) as old:
            assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
            for key in out:
                assert np.array_equal(old[key], out[key]), key
        print("pca_normals.npz reproduced (%d arrays)" % len(out))
        return
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
