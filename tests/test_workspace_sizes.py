"""Every workspace sizer of the C ABI returns what tests/golden/workspace_sizes.json recorded at the commit before sizer and carving
became one layout function per workspace (tests/golden/record_workspace_sizes.py: grids, environments and rows live there).

A caller allocates exactly the sizer's bytes, and tests/test_gpu_bounds.py holds the forwards to them under guard bands at the shapes
of its case table; this file pins the numbers themselves, over many more shapes, so a layout edit that moves a size (or the chunk
size behind it) shows as a diff in integers.  The handle-free sizers need no GPU; sapcu_workspace_bytes needs real handles.
"""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, golden
import gpu_utils as U

_spec = importlib.util.spec_from_file_location("record_workspace_sizes", os.path.join(GOLDEN, "record_workspace_sizes.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

with open(os.path.join(GOLDEN, "workspace_sizes.json")) as _f:
    RECORDED = json.load(_f)


def _lib():
    from sapcu_amd import _lib
    return _lib.load()


def _assert_same(got, want, what):
    assert len(got) == len(want), "%s: %d cases, %d recorded (grid changed without re-recording?)" % (what, len(got), len(want))
    bad = [(g, w[-1]) for g, w in zip(got, want) if g != w]
    assert not bad, "%s: %d of %d differ; first (args..., got) vs recorded: %s" % (what, len(bad), len(got), bad[:4])


def test_handle_free_sizers_return_the_recorded_bytes():
    got = R.record_sizers(_lib())
    assert sorted(got) == sorted(RECORDED["sizers"])
    for name in got:
        _assert_same(got[name], RECORDED["sizers"][name], name)
    # the grid holds what it is meant to hold: accepted and refused shapes, and sizes that differ
    chain = [v[-1] for v in got["sapcu_fn_edge_chain_workspace_bytes"]]
    assert any(v < 0 for v in chain) and len(set(v for v in chain if v > 0)) > 12


@pytest.mark.gpu
@pytest.mark.parametrize("env", R.ENVS, ids=[R.env_id(e) for e in R.ENVS])
def test_default_handles_return_the_recorded_bytes(env, weights, monkeypatch):
    fn, fd, _, _ = U.build_gpu_models_under(weights, monkeypatch, env)
    want = RECORDED["handles"][R.env_id(env)]
    for kind, model in (("fn", fn), ("fd", fd)):
        _assert_same(R.record_handle(_lib(), model), want[kind], "%s %s" % (R.env_id(env), kind))


@pytest.mark.gpu
@pytest.mark.parametrize("rid", R.HPARAM_ROWS)
def test_hparam_row_handles_return_the_recorded_bytes(rid):
    row = U.hparam_row(golden("hparams.npz"), rid)
    model, _ = U.build_gpu_hparam_model(row)
    _assert_same(R.record_handle(_lib(), model), RECORDED["handles"][rid][row["kind"]], rid)
