#!/usr/bin/env python3
"""Record what the evaluation modules (metrics, mesh, ray, normals, sinkhorn, surface, data) raise on every bad input of
tests/eval_cases.py -> eval_refusals.json, and what they return on valid input in every accepted form -> eval_inputs_ok.npz
(tests/test_eval_inputs_host.py and tests/test_gpu_eval_inputs.py compare).

    python tests/golden/record_eval_refusals.py

Public functions only, so the same file runs on any earlier commit: both files were recorded at the commit BEFORE the input checks
of the seven modules became one module (sapcu_amd/_inputs.py), and they are not to be re-recorded because a message or a
precedence changed by accident.  Two sections of the json, {case id: [exception type, message]} each ([null, null]: no exception):

  "host"    the cases built from numpy arrays and CPU tensors, with torch.cuda.current_device made to raise: what is refused
            before anything touches a device.  A case that reaches the device is left out.  Needs no GPU.
  "device"  every case, the same ones included, on a GPU.

Without a GPU only "host" is recorded, and "device" and the npz are kept as they are.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "eval_refusals.json")
OUT_OK = os.path.join(HERE, "eval_inputs_ok.npz")


def record_host():
    import torch
    import eval_cases as E
    saved = torch.cuda.current_device
    E.without_device(setattr)
    out = {}
    try:
        for cid, thunk in E.cases(None):
            try:
                out[cid] = E.outcome(thunk)
            except E.NeedsDevice:
                pass
    finally:
        torch.cuda.current_device = saved
    return out


def record_device(dev):
    import eval_cases as E
    return {cid: E.outcome(thunk) for cid, thunk in E.cases(dev)}


def record_ok(dev):
    import eval_cases as E
    out = {}
    for cid, thunk in E.ok_calls(dev):
        for name, value in E.flatten(thunk()).items():
            out["%s/%s" % (cid, name)] = value
    return out


def main():
    import warnings
    import numpy as np
    import sapcu_amd                                                          # noqa: F401 - registers the package
    import torch
    warnings.simplefilter("ignore")
    data = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            data = json.load(f)
    data["host"] = record_host()
    if torch.cuda.is_available():
        dev = torch.device("cuda:0")
        data["device"] = record_device(dev)
        np.savez_compressed(OUT_OK, **record_ok(dev))
    else:
        print("no GPU: 'device' section and %s %s" % (os.path.basename(OUT_OK), "kept as recorded" if "device" in data else "NOT recorded"))
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": {\n' % sec + ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in data[sec].items())
                                   + "\n }" for sec in data) + "\n}\n")
    print("wrote %s: %s" % (OUT, {sec: len(data[sec]) for sec in data}))


if __name__ == "__main__":
    main()
