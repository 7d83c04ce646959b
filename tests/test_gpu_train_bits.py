"""The training entry points write the bits tests/golden/train_bits.json recorded at the parent of the change that moved their shared
device idioms into csrc/train_common.h (tests/golden/record_train_bits.py: cases, shapes and inputs live there).  A digest that
differs names its case and the position of the output tensor in that case's list."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN
import gpu_utils as U

_spec = importlib.util.spec_from_file_location("record_train_bits", os.path.join(GOLDEN, "record_train_bits.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

with open(os.path.join(GOLDEN, "train_bits.json")) as _f:
    RECORDED = json.load(_f)


def test_every_piece_is_recorded():
    assert sorted(RECORDED) == sorted(R.PIECES)
    assert all(RECORDED[p] for p in R.PIECES)


@pytest.mark.gpu
@pytest.mark.parametrize("piece", R.PIECES)
def test_training_ops_write_the_recorded_bits(piece):
    got, want = R.digests(piece, U.dev()), RECORDED[piece]
    assert sorted(got) == sorted(want), "%s: the case list changed without re-recording" % piece
    bad = [(cid, i) for cid in sorted(got) for i, (g, w) in enumerate(zip(got[cid], want[cid])) if g != w]
    assert not bad and all(len(got[c]) == len(want[c]) for c in got), "%s: (case, output) whose bits differ: %s" % (piece, bad[:8])
