"""Fixture of the cloud metrics (tests/golden/cloud_metrics.npz), made by RUNNING the reference's evaluation script on the CPU.

Run in the build container only (needs /root/reference, which never travels, sklearn and numpy):

    python tests/golden/make_metrics_fixtures.py            # writes cloud_metrics.npz
    python tests/golden/make_metrics_fixtures.py --check    # rebuilds in memory and compares with the committed file

``external/Meta-PU_evaluation/evaluation_code/evaluation_cd.py`` is run from where it lies, as a subprocess, unchanged; its one
missing import (``pyemd``, for the EMD line that is not part of this fixture) is a stub made in a temporary directory.  Cloud
pairs are written as ``.xyz`` with ``%.17g`` (a round trip of every f64).  The script runs once per pair (one file per directory,
so the order is unambiguous) and once over all pairs (the ``os.listdir`` order of that directory is recorded).  It prints every
value with ``'{}'.format``, which round-trips, so the parsed values are its values.  They are recomputed here with sklearn and
numpy, and sklearn's distances with the plain f64 expression sqrt(((dx*dx + dy*dy) + dz*dz).min()); NOTHING is written if any
value differs.  No text of the reference is stored: only data its program read and wrote.

Stored: ``pairs`` (names); per pair ``<name>/pred``, ``<name>/gt`` (f64 [n,3]) and ``<name>/values``; ``pooled/order`` (names in
the script's order) and ``pooled/values``; ``b/gt2pre`` and ``b/pre2gt``, the per-point vectors of pair b.  ``values`` =
[gt2pre mean, std, recall@1e-2, recall@2e-2, pre2gt mean, std, precision@1e-2, precision@2e-2, cd, fscore@1e-2, fscore@2e-2].
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REF = "/root/reference"
SCRIPT = os.path.join(REF, "external", "Meta-PU_evaluation", "evaluation_code", "evaluation_cd.py")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cloud_metrics.npz")
VALUE_NAMES = ("gt2pre_mean", "gt2pre_std", "recall0", "recall1", "pre2gt_mean", "pre2gt_std", "precision0", "precision1", "cd",
               "fscore0", "fscore1")


def shell(rng, n, noise):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return 0.5 * v + rng.normal(size=(n, 3)) * noise


def make_pair(seed, n_pred, n_gt, hits, dups, noise=0.004):
    """Two samplings of a sphere shell of radius 0.5; `hits` points of gt are exact copies of points of pred (distance 0),
    `dups` points of pred are repeated inside pred (ties between equal points)."""
    rng = np.random.default_rng(seed)
    pred, gt = shell(rng, n_pred, noise), shell(rng, n_gt, noise)
    gt[rng.choice(n_gt, hits, replace=False)] = pred[rng.choice(n_pred, hits, replace=False)]
    src = rng.choice(n_pred, dups, replace=False)
    pred[(src + 1) % n_pred] = pred[src]
    return np.ascontiguousarray(pred), np.ascontiguousarray(gt)


PAIRS = {"a": (11, 4500, 6100, 50, 10), "b": (12, 5000, 4097, 50, 10), "c": (13, 300, 200, 30, 4)}


def run_script(pre_dir, gt_dir, stub_dir):
    env = dict(os.environ, PYTHONPATH=stub_dir + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, SCRIPT, "--pre_path", pre_dir, "--gt_path", gt_dir], env=env, check=True,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True).stdout
    vals = []
    for line in out.splitlines():
        text = line.split(":", 1)[1] if ":" in line else (line if line.startswith("\t") else "")
        if text.strip():
            vals.append(float(text))
    assert len(vals) == 12 and np.isnan(vals[11]), out          # the 11 values and the stub's EMD
    return np.array(vals[:11], dtype=np.float64)


def sklearn_distances(pred, gt):
    from sklearn.neighbors import NearestNeighbors
    gt2pre, _ = NearestNeighbors(n_neighbors=1, algorithm="auto").fit(pred).kneighbors(gt)
    pre2gt, _ = NearestNeighbors(n_neighbors=1, algorithm="auto").fit(gt).kneighbors(pred)
    return np.squeeze(gt2pre), np.squeeze(pre2gt)


def plain_distances(cloud, queries):
    out = np.empty(len(queries))
    for i, q in enumerate(queries):
        d = q - cloud
        out[i] = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).min())
    return out


def numpy_values(gt2pre, pre2gt):
    r = [np.mean(gt2pre <= t) for t in (1e-2, 2e-2)]
    p = [np.mean(pre2gt <= t) for t in (1e-2, 2e-2)]
    return np.array([np.mean(gt2pre), np.std(gt2pre), r[0], r[1], np.mean(pre2gt), np.std(pre2gt), p[0], p[1],
                     0.5 * (np.mean(gt2pre) + np.mean(pre2gt)), 2 / (1 / r[0] + 1 / p[0]), 2 / (1 / r[1] + 1 / p[1])])


def build():
    assert os.path.exists(SCRIPT), SCRIPT
    clouds = {name: make_pair(*args) for name, args in PAIRS.items()}
    out = {"pairs": np.array(sorted(clouds)), "value_names": np.array(VALUE_NAMES)}
    dists = {}
    with tempfile.TemporaryDirectory() as tmp:
        stub = os.path.join(tmp, "stub")
        os.makedirs(stub)
        with open(os.path.join(stub, "pyemd.py"), "w") as f:
            f.write("def emd_samples(a, b):\n    return float('nan')\n")
        for where in list(clouds) + ["all"]:
            for side in ("pre", "gt"):
                os.makedirs(os.path.join(tmp, where, side))
        for name, (pred, gt) in clouds.items():
            for where in (name, "all"):
                np.savetxt(os.path.join(tmp, where, "pre", name + ".xyz"), pred, fmt="%.17g")
                np.savetxt(os.path.join(tmp, where, "gt", name + ".xyz"), gt, fmt="%.17g")
            assert np.array_equal(np.loadtxt(os.path.join(tmp, name, "gt", name + ".xyz")), gt)
            printed = run_script(os.path.join(tmp, name, "pre"), os.path.join(tmp, name, "gt"), stub)
            g2p, p2g = sklearn_distances(pred, gt)
            assert np.array_equal(g2p, plain_distances(pred, gt)) and np.array_equal(p2g, plain_distances(gt, pred)), \
                "pair %s: sklearn's distances are not the plain f64 expression" % name
            mine = numpy_values(g2p, p2g)
            assert np.array_equal(printed, mine), "pair %s: printed %r, recomputed %r" % (name, printed, mine)
            assert printed[2] > 0 and printed[6] > 0, "pair %s: an F-score would divide by zero" % name
            dists[name] = (g2p, p2g)
            out[name + "/pred"], out[name + "/gt"], out[name + "/values"] = pred, gt, printed
        order = [f[:-4] for f in os.listdir(os.path.join(tmp, "all", "gt")) if f.endswith(".xyz")]
        printed = run_script(os.path.join(tmp, "all", "pre"), os.path.join(tmp, "all", "gt"), stub)
        mine = numpy_values(np.hstack([dists[n][0] for n in order]), np.hstack([dists[n][1] for n in order]))
        assert np.array_equal(printed, mine), "pooled (%s): printed %r, recomputed %r" % (order, printed, mine)
        out["pooled/order"], out["pooled/values"] = np.array(order), printed
    out["b/gt2pre"], out["b/pre2gt"] = dists["b"]
    return out


def main():
    out = build()
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out)
        for k in out:
            if k == "pooled/order":                       # a directory's listing order may differ; the pooled values then too
                continue
            if k == "pooled/values" and list(old["pooled/order"]) != list(out["pooled/order"]):
                continue
            assert np.array_equal(old[k], out[k]), k
        print("cloud_metrics.npz reproduced (%d arrays)" % len(out))
        return
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
