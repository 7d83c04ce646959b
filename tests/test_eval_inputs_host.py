"""What the evaluation modules refuse before anything touches a device, against the record of the commit before their input checks
became sapcu_amd/_inputs.py (tests/golden/eval_refusals.json, section "host", written by tests/golden/record_eval_refusals.py and
never regenerated from the result): exception type and message, word for word.  No GPU needed: torch.cuda.current_device is made
to raise, and a case that gets that far is one the record leaves to the device section."""
import json
import os
from collections import defaultdict

import pytest

import eval_cases as E
from conftest import GOLDEN

# cases whose recorded outcome the shared module changes on purpose: none.  (The one intended change of precedence, shape before
# device in device_tensor as data.build_patches had it, needs a tensor on a second device and so has no row in the record.)
CHANGED = {}


def _record():
    with open(os.path.join(GOLDEN, "eval_refusals.json")) as f:
        return json.load(f)["host"]


def _groups():
    out = defaultdict(list)
    for cid in _record():
        out[cid.split("/", 1)[0]].append(cid)
    return out


def test_the_table_holds_every_recorded_case_once():
    ids = [cid for cid, _ in E.cases(None)]
    assert len(ids) == len(set(ids))
    assert set(_record()) <= set(ids)
    assert len(_record()) > 500 and not CHANGED


@pytest.mark.parametrize("group", sorted(_groups()))
def test_refusals_before_any_device_work_are_what_they_were(group, monkeypatch):
    record = _record()
    E.without_device(monkeypatch.setattr)
    wrong = []
    for cid, thunk in E.cases(None):
        if cid.split("/", 1)[0] != group:
            continue
        try:
            got = E.outcome(thunk)
        except E.NeedsDevice:
            got = "reached the device"
        want = CHANGED.get(cid, record.get(cid, "reached the device"))
        if got != want:
            wrong.append((cid, got, want))
    assert not wrong, "\n".join("%s: %s, recorded %s" % w for w in wrong)
