"""CPU tests of the bounds harness itself (tests/guarded.py), the header coverage gate and the host seed generator under
guards.  The stand-in "kernels" here are torch indexing on CPU tensors; no deliberately bad kernel ever runs on a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from guarded import Arena, GuardDamage, MIN_BAND, guarded


def _raw_elems(g):
    """The whole allocation as elements of g's dtype, and the element index of the payload's first element."""
    e = g.esize
    lead = g.p0 % e
    n = (g.raw.numel() - lead) // e
    return g.raw[lead:lead + n * e].view(g.dtype), (g.p0 - lead) // e


@pytest.mark.parametrize("fill", [0xFF, 0x00])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.float16])
def test_clean_op_passes_and_view_has_the_asked_alignment_and_pitch(dtype, fill):
    for shape, pitch, align, offset in (((7, 33), 40, 512, 16), ((129, 64), None, 512, 0), ((5,), None, 256, 8), ((3, 4, 6), 8, 64, 16),
                                        ((1, 1), 4, 512, 496), ((0, 8), 8, 512, 0)):
        g = guarded(shape, dtype, pitch=pitch, align=align, offset=offset, band_fill=fill)
        assert tuple(g.t.shape) == shape and g.t.dtype == dtype
        if g.t.numel():
            assert g.t.data_ptr() % align == offset
            assert g.t.stride(-1) == 1
            if len(shape) > 1:
                assert g.t.stride(-2) == (pitch or shape[-1])
            if len(shape) == 3:
                assert g.t.stride(0) == shape[1] * pitch
        assert g.band >= MIN_BAND and g.band >= 256 * (pitch or 1) * g.esize
        assert g.p0 >= g.band and g.raw.numel() - g.p1 >= g.band            # both bands have their full size
        g.t.copy_(torch.ones(shape).to(dtype))                               # a clean op: writes every declared element
        g.check()
        if g.t.numel():
            assert bool((g.t == 1).all())
        patt = g.raw[:g.p0]
        assert bool((patt == fill).all())


def test_the_0xff_pattern_reads_as_nan_and_minus_one():
    for dtype in (torch.float16, torch.float32, torch.float64):
        g = guarded((4, 4), dtype, pitch=8)
        raw, at = _raw_elems(g)
        assert bool(torch.isnan(raw[at - 1])) and bool(torch.isnan(raw[at + 4]))
    for dtype in (torch.int32, torch.int64):
        g = guarded((4, 4), dtype, pitch=8)
        raw, at = _raw_elems(g)
        assert int(raw[at - 1]) == -1 and int(raw[at + 5]) == -1


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_one_element_before_after_and_into_a_pitch_gap_is_reported_with_its_offsets(fill):
    rows, width, pitch = 6, 10, 16
    span = ((rows - 1) * pitch + width) * 4

    def fresh():
        g = guarded((rows, width), torch.float32, pitch=pitch, offset=16, band_fill=fill, name="c")
        raw, at = _raw_elems(g)
        return g, raw, at

    g, raw, at = fresh()
    raw[at - 1] = 3.0                                     # a stand-in op that writes one element BEFORE the payload
    with pytest.raises(GuardDamage) as e:
        g.check()
    (r,) = e.value.reports
    # 3.0f = 00 00 40 40: two of its four bytes equal the 0x00 pattern and cannot show
    want = (-4, -1, 4) if fill == 0xFF else (-2, -1, 2)
    assert (r["side"], r["first"], r["last"], r["count"]) == ("front",) + want and r["buffer"] == "c"
    assert "front" in str(e.value) and str(want[0]) in str(e.value)

    g, raw, at = fresh()
    raw[at + (rows - 1) * pitch + width] = -1.5           # one element AFTER the last row (the gap after the last row is back band)
    with pytest.raises(GuardDamage) as e:
        g.check()
    (r,) = e.value.reports
    assert r["side"] == "back" and span <= r["first"] <= r["last"] == span + 3

    g, raw, at = fresh()
    raw[at + 2 * pitch + width + 1] = 7.0                 # row 2, second gap column
    with pytest.raises(GuardDamage) as e:
        g.check()
    (r,) = e.value.reports
    lo = (2 * pitch + width + 1) * 4
    assert r["side"] == "gap" and lo <= r["first"] <= r["last"] == lo + 3

    g, raw, at = fresh()                                  # a whole ragged tile past the end still lands inside the band
    raw[at + rows * pitch: at + (rows + 255) * pitch] = 1.0
    with pytest.raises(GuardDamage) as e:
        g.check()
    (r,) = e.value.reports
    assert r["side"] == "back" and r["last"] < span + g.band

    g, raw, at = fresh()                                  # far ends of both bands are watched too
    g.raw[0] = 0x5A
    g.raw[-1] = 0x5A
    with pytest.raises(GuardDamage) as e:
        g.check()
    assert sorted(r["side"] for r in e.value.reports) == ["back", "front"]


def test_arena_protocol_pieces_on_the_cpu():
    """Arena: input bands take the run's pattern, outputs start as 0xFF, workspaces start as the pattern; a stand-in op that
    lets a value from an input's band reach its result gives different outputs under the two patterns — how a stray read shows."""
    outs = []
    for fill in (0xFF, 0x00):
        A = Arena("guard", fill)
        x = A.inp(np.arange(12, dtype=np.float32).reshape(3, 4), pitch=8, offset=16)
        y = A.out((3, 4), torch.float32, pitch=12)
        w = A.ws(100)
        assert bool(torch.isnan(y).all()) and bool((w == fill).all()) and x.stride(0) == 8 and x.data_ptr() % 512 == 16
        flat = torch.as_strided(x, (3, 5), (8, 1))       # the stand-in reads one column past the declared width
        y.copy_(flat[:, :4] + torch.nan_to_num(flat[:, 4:5], nan=1.0))
        A.check()
        outs.append(A.outs[0].payload_bits())
    assert not torch.equal(outs[0], outs[1])
    C = Arena("compact")
    x = C.inp(np.zeros((3, 4), np.float32), pitch=8, offset=16)
    assert x.is_contiguous() and bool((C.ws(10) == 0).all())


# ------------------------------------------------------------------------------------------------ coverage gate
EXEMPT = {
    "sapcu_abi_version": "no pointer, no device work",
    "sapcu_last_error": "returns the calling thread's error text",
    "sapcu_model_create": "copies a parameter blob into library-owned memory; exercised by every model case",
    "sapcu_model_destroy": "frees the handle",
    "sapcu_workspace_bytes": "sizer (its result is the exact size of the guarded model workspaces)",
    "sapcu_knn_grid_workspace_bytes": "sizer (exercised with exactly its size)",
    "sapcu_fps_workspace_bytes": "sizer (exercised with exactly its size)",
    "sapcu_lif_train_workspace_bytes": "sizer (exercised with exactly its size)",
    "sapcu_train_workspace_bytes": "sizer (exercised with exactly its size)",
    "sapcu_wgrad_bf16_workspace_bytes": "sizer (exercised with exactly its size)",
    "sapcu_fn_edge_chain_workspace_bytes": "sizer (exercised with exactly its size)",
    "sapcu_model_gate_violations": "status getter: host int out",
    "sapcu_model_gemm_mode": "status getter: host ints out",
    "sapcu_model_fused_blocks": "status getter: host int out, no device work",
    "sapcu_dense_seeds_host": "host code: test_dense_seeds_host_under_guards below",
}


from abi_tables import header_entry_points                # include/sapcu.h by default: the table this gate covers


def uncovered_entry_points(covered):
    decl = header_entry_points()
    return sorted(n for n, args in decl.items() if ("*" in args or "sapcu_model_t" in args) and n not in covered and n not in EXEMPT)


def test_every_pointer_taking_entry_point_has_a_bounds_case():
    import test_gpu_bounds as B
    from sapcu_amd import _lib
    decl = header_entry_points()
    assert set(decl) == set(_lib.EXPORTS), "the header parser and the binding disagree: %s" % sorted(set(decl) ^ set(_lib.EXPORTS))
    covered = set()
    for c in B.CASES:
        assert c.entry_points, c.id
        covered.update(c.entry_points)
    assert covered <= set(decl), "the case table names entry points the header does not declare: %s" % sorted(covered - set(decl))
    missing = uncovered_entry_points(covered)
    assert not missing, "entry points without a bounds case in tests/test_gpu_bounds.py (add a case, or an exemption with a reason): %s" % missing
    # the gate itself: an entry point whose cases are all removed is named
    some = "sapcu_patch_knn"
    assert uncovered_entry_points(covered - {some}) == [some]
    # every sizer is exercised with exactly its size by at least one case
    sizers = {n for n in decl if n.endswith("workspace_bytes")}
    used = set()
    for c in B.CASES:
        used.update(c.sizers)
    assert sizers <= used, "sizers never used at exactly their size: %s" % sorted(sizers - used)


# ------------------------------------------------------------------------------------------------ host seed generator
def test_dense_seeds_host_under_guards():
    """sapcu_dense_seeds_host (CPU code) with guarded numpy buffers, the three-run protocol: bands intact, results independent
    of the band pattern and of what the output held, equal to the reference's own dense.cpp run (tests/golden/dense_seeds.npz);
    a capacity one short is refused with SAPCU_ERR_WORKSPACE and the count."""
    from sapcu_amd import _lib, testing as T
    lib = _lib.load()
    g = golden("dense_seeds.npz")
    for name, cloud in (("cube300_c050", T.analytic_cloud("cube", 300, 2)), ("tiny7_c050", T.sphere_cloud(7, 3)),
                        ("sphere2048_c030", T.sphere_cloud(2048, 0))):
        want = g[name].reshape(-1, 3)
        cell = float(g[name + "_cell"])
        n, cap = cloud.shape[0], want.shape[0]
        results = []
        for fill, offset in ((0xFF, 8), (0x00, 8), (0x00, 0)):
            cg = guarded((n, 3), torch.float64, band_fill=fill, offset=offset, name="cloud").set(np.ascontiguousarray(cloud, dtype=np.float64))
            sg = guarded((cap, 3), torch.float64, offset=offset, name="seeds").fill_payload_bytes(0xFF)     # exactly the needed capacity
            for rep in range(2):                                                                             # second pass: dirty output
                count = ctypes.c_int64(-1)
                rc = lib.sapcu_dense_seeds_host(ctypes.c_void_p(cg.t.data_ptr()), n, cell, ctypes.c_void_p(sg.t.data_ptr()), cap, ctypes.byref(count))
                assert rc == 0 and count.value == cap, (name, rc, count.value)
                cg.check()
                sg.check()
                results.append(sg.t.numpy().copy())
        for r in results:
            assert np.array_equal(r, want), name
        if cap > 1:
            sg = guarded((cap - 1, 3), torch.float64, name="seeds").fill_payload_bytes(0xFF)
            count = ctypes.c_int64(-1)
            rc = lib.sapcu_dense_seeds_host(ctypes.c_void_p(cg.t.data_ptr()), n, cell, ctypes.c_void_p(sg.t.data_ptr()), cap - 1, ctypes.byref(count))
            assert rc == -2 and count.value == cap
            sg.check()
            cg.check()
