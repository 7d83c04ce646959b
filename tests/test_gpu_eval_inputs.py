"""The evaluation modules on a device against the record of the commit before their input checks became sapcu_amd/_inputs.py
(tests/golden/record_eval_refusals.py wrote both files there; neither is regenerated from the result): every bad input of
tests/eval_cases.py raises the recorded exception with the recorded message (or, as recorded, none), and every valid call, in
every accepted form of its inputs, returns the recorded values bit for bit."""
import json
import os
import warnings
from collections import defaultdict

import numpy as np
import pytest
import torch

import eval_cases as E
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
# see tests/test_eval_inputs_host.py: no recorded outcome changes
CHANGED = {}


def _record():
    with open(os.path.join(GOLDEN, "eval_refusals.json")) as f:
        return json.load(f)["device"]


def _groups(ids):
    out = defaultdict(list)
    for cid in ids:
        out[cid.split("/", 1)[0]].append(cid)
    return out


@pytest.fixture(scope="module")
def cases():
    found = E.cases(torch.device("cuda:0"))
    ids = [cid for cid, _ in found]
    assert len(ids) == len(set(ids)) and set(ids) == set(_record())
    return found


@pytest.fixture(scope="module")
def ok_calls():
    return dict(E.ok_calls(torch.device("cuda:0")))


@pytest.mark.parametrize("group", sorted(_groups(_record())))
def test_refusals_are_what_they_were(group, cases):
    record = _record()
    wrong = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for cid, thunk in cases:
            if cid.split("/", 1)[0] == group:
                got, want = E.outcome(thunk), CHANGED.get(cid, record[cid])
                if got != want:
                    wrong.append((cid, got, want))
    assert not wrong, "\n".join("%s: %s, recorded %s" % w for w in wrong)


def _recorded_calls():
    with np.load(os.path.join(GOLDEN, "eval_inputs_ok.npz")) as g:
        return sorted({k.rsplit("/", 1)[0] for k in g.files})


@pytest.mark.parametrize("call", sorted(_groups(_recorded_calls())))
def test_valid_input_in_every_form_gives_the_recorded_bits(call, ok_calls):
    with np.load(os.path.join(GOLDEN, "eval_inputs_ok.npz")) as g:
        want = {k: g[k] for k in g.files if k.startswith(call + "/")}
    forms = [cid for cid in ok_calls if cid.split("/", 1)[0] == call]
    assert forms
    got = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for cid in forms:
            got.update({"%s/%s" % (cid, name): v for name, v in E.flatten(ok_calls[cid]()).items()})
    assert set(got) == set(want)
    wrong = [k for k in sorted(want) if not E.same_bits(got[k], want[k])]
    assert not wrong, wrong


def test_every_recorded_call_is_still_made(ok_calls):
    assert set(ok_calls) == set(_recorded_calls())
