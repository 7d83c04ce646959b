"""Writes tests/golden/sinkhorn_cases.npz (CPU only, run by hand: python tests/golden/make_sinkhorn_cases.py).

Per case of tests/sinkhorn_ref.py::build_cases, whose inputs are regenerated from (name, seed) and not stored:
  <name>/f, /g, /r, /c, /ot, /primal_cost, /marginal_error   the definition evaluated in np.longdouble, rounded to f64 (the "truth")
  <name>/err                                                 max |f64 definition - truth| per quantity of sinkhorn_ref.QUANTITIES
                                                             (err[0], over f and g, is the err_np of the potentials)
  <name>/emd                                                 sandwich cases: the exact optimum (scipy)
and "names", "split" (the library's tile and chunk constants the boundary cases were chosen for).
A sandwich case must reach marginal_error <= 1e-9; the script refuses to write the file otherwise."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import sinkhorn_ref as R  # noqa: E402


def main():
    from sapcu_amd import sinkhorn
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not wider than f64 on this machine"
    cases = R.build_cases(sinkhorn.split_plan)
    out = {"names": np.array([c["name"] for c in cases]), "split": np.array(sinkhorn.split_plan(100, 320)[:2], dtype=np.int64)}
    for c in cases:
        truth = {k: np.asarray(v, dtype=np.float64) for k, v in R.run_case(c, np.longdouble).items()}       # rounded: what is stored
        plain = R.run_case(c, np.float64)
        err = R.errors(plain, truth)
        for k in ("f", "g", "r", "c", "ot", "primal_cost", "marginal_error"):
            out["%s/%s" % (c["name"], k)] = truth[k]
        out[c["name"] + "/err"] = np.array([err[q] for q in R.QUANTITIES], dtype=np.float64)
        line = "%-26s %3d x %3d p=%d blur=%-5g iters=%3d  marginal %.1e  err pot %.1e ot %.1e primal %.1e r %.1e c %.1e" % (
            c["name"], c["n"], c["m"], c["p"], c["blur"], c["iters"], float(truth["marginal_error"]), err["pot"], err["ot"],
            err["primal_cost"], err["r"], err["c"])
        if c["sandwich"]:
            assert float(truth["marginal_error"]) <= 1e-9, "sandwich case %s is not converged: %r" % (c["name"], truth["marginal_error"])
            x, y = R.case_inputs(c)
            out[c["name"] + "/emd"] = np.float64(R.exact_emd(x, y, c["p"]))
            line += "  emd %.6f gap %.4f" % (out[c["name"] + "/emd"], float(truth["primal_cost"]) - out[c["name"] + "/emd"])
        print(line, flush=True)
    path = os.path.join(HERE, "sinkhorn_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
