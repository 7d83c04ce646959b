"""Seed generation on the device (include/sapcu_seeds.h, csrc/dense_seeds_dev.hip): the voxel flood of sapcu_dense_seeds_host with
the seeds left in HBM — the same seeds in the same order with the same 6-decimal values, bit for bit (np.array_equal everywhere).

  * against runs of the reference's own `dense` (fixtures of tests/golden/), with the host recomputation path idle (stats[2] == 0);
  * against the host generator where no reference run exists: exact ties (lattice, duplicated points — the host path must be
    seen working there), the origin, n = 1..11, keys that leave the grid, an x index outside the 6-decimal table;
  * determinism, capacity and table refusals, the memory contract under guard bands (the four-run protocol of
    tests/test_gpu_bounds.py), a gate over include/sapcu_seeds.h, the public interface (seed_source = "device"), ranks on one GPU.
"""
import ctypes
import hashlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_tables
from conftest import ROOT, golden
import gpu_utils as U

F64 = torch.float64


def _gen():
    from sapcu_amd import generation
    return generation


def _device_seeds(cloud, cell, **kw):
    st = []
    s = _gen().dense_seeds_device(cloud, cell, U.dev(), stats=st, **kw)
    assert s.is_cuda and s.dtype == F64 and s.ndim == 2 and s.shape[1] == 3
    return s.cpu().numpy(), st


def _reference_cases():
    """(name, cloud, cell, seeds of the reference's own dense) — every small fixture of item 1 of the issue."""
    from sapcu_amd import testing as T
    g = golden("dense_seeds.npz")
    out = [(name, cloud, float(g[name + "_cell"]), g[name].reshape(-1, 3)) for name, cloud in
           (("sphere2048_c030", T.sphere_cloud(2048, 0)), ("torus2048_c020", T.analytic_cloud("torus", 2048, 1)),
            ("cube300_c050", T.analytic_cloud("cube", 300, 2)), ("tiny7_c050", T.sphere_cloud(7, 3)))]
    out.append(("e2e_upsample", T.sphere_cloud(2048, 0), 0.03, golden("e2e_upsample.npz")["seeds"]))
    suite = golden("shape_suite.npz")
    for name, _, _, spacing in T.SHAPE_SUITE:
        out.append(("suite_" + name, T.suite_cloud(name, suite), spacing, suite[name + "_seeds"]))
    s16 = golden("scale16.npz")
    out.append(("scale16", s16["norm_cloud"], T.SCALE16_CASE["spacing"], s16["seeds"]))
    return out


# ================================================================================================ 1 + 3: the reference's runs
@pytest.mark.gpu
def test_device_seeds_match_the_reference_dense_runs_bit_for_bit():
    """Items 1 and 3: every fixture made by the reference's `dense`; the host recomputation carries none of them."""
    assert len(_reference_cases()) == 12
    for name, cloud, cell, want in _reference_cases():
        got, st = _device_seeds(cloud, cell)
        print("%s: %d seeds, stats %s" % (name, got.shape[0], st))
        assert got.shape == want.shape and np.array_equal(got, want), name
        assert st[2] == 0, "%s: %d of %d voxels were recomputed on the host" % (name, st[2], st[1])
        if name in ("sphere2048_c030", "e2e_upsample"):
            assert st[:2] == [7, 8675], st
    assert _reference_cases()[3][3].shape[0] == 0                     # tiny7_c050: a flood without a single seed


@pytest.mark.gpu
def test_device_seeds_full_size_case_by_count_hash_head_and_tail():
    """Sphere 5000 at 0.004 as tests/test_host.py checks the host generator: 385 582 seeds, SHA-256, head, tail; 20 levels,
    1 755 588 voxels, none on the host."""
    from sapcu_amd import testing as T
    g = golden("dense_seeds.npz")
    big, st = _device_seeds(T.sphere_cloud(5000, 0), 0.004)
    print("sphere5000_c004: %d seeds, stats %s" % (big.shape[0], st))
    assert big.shape[0] == int(g["sphere5000_c004_count"]) == 385582
    assert hashlib.sha256(big.tobytes()).hexdigest() == str(g["sphere5000_c004_sha256"])
    assert np.array_equal(big[:64], g["sphere5000_c004_head"]) and np.array_equal(big[-64:], g["sphere5000_c004_tail"])
    assert st[0] == 20 and st[1] == 1755588 and st[2] == 0, st


# ================================================================================================ 2: the host as yardstick
def _lattice(m=6, step=0.05, lo=-0.125):
    return np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3) * step + lo


def _host_cases():
    from sapcu_amd import testing as T
    sph = T.sphere_cloud(512, 11)
    dup = np.concatenate([sph[:200], sph[:200], sph[100:150]])                  # exact duplicates: ties at distance-equal pairs
    origin = np.concatenate([T.sphere_cloud(300, 12) * 0.5, np.zeros((1, 3))])      # the cloud holds the extra point's twin
    edge = T.analytic_cloud("cube", 600, 13)
    edge = edge / np.abs(edge).max() * 0.5                                       # faces at exactly +-0.5: keys leave the grid
    far = T.sphere_cloud(256, 14) * 0.4 + np.array([3.0, 0.0, 0.0])                 # x index beyond 2 * boxsize: no table entry
    cases = [("lattice", _lattice(), 0.0175), ("lattice_c050", _lattice(), 0.05), ("duplicates", dup, 0.0175), ("origin", origin, 0.0175),
             ("edge_c0175", edge, 0.0175), ("edge_c050", edge, 0.05), ("far_x", far, 0.05), ("sphere512_c004", sph * 0.2, 0.004),
             ("sphere512_c0175", sph, 0.0175), ("sphere512_c050", sph, 0.05)]
    for n in (1, 5, 9, 10, 11):
        cases.append(("n%d" % n, T.sphere_cloud(64, 20 + n)[:n] * 0.05 + 0.01, 0.0175))
        cases.append(("n%d_c004" % n, T.sphere_cloud(64, 40 + n)[:n] * 0.02 - 0.003, 0.004))
    return cases


@pytest.mark.gpu
def test_device_seeds_equal_the_host_generator_on_ties_small_n_and_grid_edges():
    """Item 2.  The tie rule (a voxel whose 10th and 11th nearest are equidistant goes to the host's own fan_distance) is derived
    from reading the host code: the lattice and the duplicated cloud confirm it, and must show the host path at work."""
    gen = _gen()
    redone = {}
    for name, cloud, cell in _host_cases():
        got, st = _device_seeds(cloud, cell)
        want = gen.dense_seeds(cloud, cell)
        print("%s: %d seeds (host %d), stats %s" % (name, got.shape[0], want.shape[0], st))
        assert got.shape == want.shape and np.array_equal(got, want), name
        redone[name] = st[2]
    assert redone["lattice"] > 0 or redone["duplicates"] > 0, redone          # else the tie path is untested
    assert redone["far_x"] > 0, redone                                        # and so would be the off-table path
    assert sum(_gen().dense_seeds(c, s).shape[0] > 0 for _, c, s in _host_cases()) >= 8      # the cases do produce seeds


# ================================================================================================ 4: determinism, capacity
def _raw_call(cloud_dev, n, cell, seeds, cap, maxv, ws, nbytes, stats=True):
    from sapcu_amd import _lib
    lib = _lib.load()
    count = ctypes.c_int64(-7)
    st = (ctypes.c_int64 * 4)()
    rc = lib.sapcu_dense_seeds_f64(_lib.ptr(cloud_dev), n, cell, _lib.ptr(seeds), cap, maxv, ctypes.byref(count), st if stats else None,
                                   _lib.ptr(ws), nbytes, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, int(count.value), list(st)


@pytest.mark.gpu
def test_device_seeds_determinism_capacity_and_table_refusals():
    from sapcu_amd import _lib, testing as T
    lib = _lib.load()
    cloud, cell = T.sphere_cloud(2048, 0), 0.03
    want = golden("e2e_upsample.npz")["seeds"]
    a, st_a = _device_seeds(cloud, cell)
    b, st_b = _device_seeds(cloud, cell)
    assert np.array_equal(a, b) and np.array_equal(a, want) and st_a == st_b
    n, total, voxels = cloud.shape[0], want.shape[0], st_a[1]
    c_dev = torch.as_tensor(cloud, device=U.dev())
    # a seed capacity one short: the full count comes back, nothing is written past the capacity
    maxv = voxels
    nbytes = int(lib.sapcu_dense_seeds_workspace_bytes(n, maxv))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=U.dev())
    seeds = torch.full((total + 8, 3), -77.0, dtype=F64, device=U.dev())
    rc, count, st = _raw_call(c_dev, n, cell, seeds, total - 1, maxv, ws, nbytes)
    assert rc == -2 and count == total and st[1] == voxels, (rc, count, st)
    assert np.array_equal(seeds[:total - 1].cpu().numpy(), want[:-1]) and bool((seeds[total - 1:] == -77.0).all())
    rc, count, st = _raw_call(c_dev, n, cell, seeds, total, maxv, ws, nbytes)          # exactly enough of both
    assert rc == 0 and count == total and np.array_equal(seeds[:total].cpu().numpy(), want) and bool((seeds[total:] == -77.0).all())
    assert st[3] >= 2 * maxv and st[3] & (st[3] - 1) == 0
    # a table one voxel short, and a much smaller one: detected, refused, nothing past the buffers (guards: the bounds test)
    for small in (voxels - 1, 600, 1):
        nb = int(lib.sapcu_dense_seeds_workspace_bytes(n, small))
        ws2 = torch.empty(nb, dtype=torch.uint8, device=U.dev())
        seeds.fill_(-77.0)
        rc, count, st = _raw_call(c_dev, n, cell, seeds, total, small, ws2, nb)
        assert rc == -2 and 0 <= count <= total, (small, rc, count)
        assert bool((seeds[total:] == -77.0).all())
    # the Python wrapper starts small on both and retries up to the full result
    got, st = _device_seeds(cloud, cell, max_voxels=100, capacity=3)
    assert np.array_equal(got, want) and st[:2] == st_a[:2]


# ================================================================================================ 5: the memory contract
SEED_CASES, SEED_REFUSALS = [], []


def seeds_header_entry_points():
    """{name: argument list} of include/sapcu_seeds.h."""
    return abi_tables.header_entry_points("sapcu_seeds.h")


def _seed_case(name, cloud_fn, cell, ws_offset):
    import test_gpu_bounds as B

    def build(A):
        from sapcu_amd import _lib
        lib = _lib.load()
        gen = _gen()
        cloud = np.ascontiguousarray(cloud_fn(), dtype=np.float64)
        want = gen.dense_seeds(cloud, cell)
        n, total = cloud.shape[0], want.shape[0]
        X = A.inp(cloud, offset=8, name="cloud")
        st0 = []
        gen.dense_seeds_device(cloud, cell, U.dev(), stats=st0)
        maxv = st0[1]                                                  # exactly the voxels the flood meets
        need = int(lib.sapcu_dense_seeds_workspace_bytes(n, maxv))
        assert need > 0
        ws = A.ws(need, offset=ws_offset, name="seed workspace")       # exactly the sizer's bytes
        out = A.out((total, 3), F64, offset=8, name="seeds_out")       # exactly the seeds there are

        def call():
            rc, count, st = _raw_call(X, n, cell, out, total, maxv, ws, need)
            _lib.check(rc)
            assert count == total and st[1] == maxv, (count, st)

        def ref(o):
            assert np.array_equal(o["seeds"].numpy(), want)
        return B.built(call, {"seeds": out}, ref)
    SEED_CASES.append(B.Case(name, ("sapcu_dense_seeds_f64",), ("sapcu_dense_seeds_workspace_bytes",), build))


def _make_seed_cases():
    from sapcu_amd import testing as T
    _seed_case("seeds-sphere2048-c030", lambda: T.sphere_cloud(2048, 0), 0.03, 0)
    _seed_case("seeds-sphere2048-c030-ws+8", lambda: T.sphere_cloud(2048, 0), 0.03, 8)      # once off the allocator's alignment
    _seed_case("seeds-lattice-c0175-ws+8", _lattice, 0.0175, 8)                                # with the host path at work
    _seed_case("seeds-n5-c0175", lambda: T.sphere_cloud(64, 25)[:5] * 0.05 + 0.01, 0.0175, 8)


_make_seed_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("c", SEED_CASES, ids=[c.id for c in SEED_CASES])
def test_seed_bounds(c):
    """0xFF bands, 0x00 bands, dirty workspace, compact call: bands intact, the four results bit-identical and equal to the host's."""
    import test_gpu_bounds as B
    B.run_protocol(c)


def _refusal(id_, want):
    def deco(fn):
        SEED_REFUSALS.append((id_, want, fn))
        return fn
    return deco


def _refusal_args(A, n=300, maxv=4096, short=0, ws_off=0, cap=512):
    from sapcu_amd import _lib, testing as T
    lib = _lib.load()
    need = int(lib.sapcu_dense_seeds_workspace_bytes(n, maxv))
    X = A.inp(T.sphere_cloud(n, 1), name="cloud")
    out = A.out((cap, 3), F64, name="seeds_out")
    ws = A.ws(need - short, offset=ws_off, name="seed workspace")
    return lib, _lib.ptr, X, out, ws, need - short


def _call(lib, *args):
    count = ctypes.c_int64(0)
    a = list(args)
    a[6] = ctypes.byref(count) if a[6] == "count" else a[6]
    return lib.sapcu_dense_seeds_f64(*a)


@_refusal("workspace-one-byte-short", -1)
def _r_short(A):
    lib, P, X, out, ws, nb = _refusal_args(A, short=1)
    return _call(lib, P(X), 300, 0.05, P(out), 512, 4096, "count", None, P(ws), nb, B_S())


@_refusal("workspace-4-byte-aligned", -1)
def _r_align(A):
    lib, P, X, out, ws, nb = _refusal_args(A, ws_off=4)
    return _call(lib, P(X), 300, 0.05, P(out), 512, 4096, "count", None, P(ws), nb, B_S())


@_refusal("n-zero", -1)
def _r_n0(A):
    lib, P, X, out, ws, nb = _refusal_args(A)
    return _call(lib, P(X), 0, 0.05, P(out), 512, 4096, "count", None, P(ws), nb, B_S())


@_refusal("cell-zero", -1)
def _r_cell0(A):
    lib, P, X, out, ws, nb = _refusal_args(A)
    return _call(lib, P(X), 300, 0.0, P(out), 512, 4096, "count", None, P(ws), nb, B_S())


@_refusal("cell-nan", -1)
def _r_cellnan(A):
    lib, P, X, out, ws, nb = _refusal_args(A)
    return _call(lib, P(X), 300, float("nan"), P(out), 512, 4096, "count", None, P(ws), nb, B_S())


@_refusal("cell-below-one-thousandth", -1)
def _r_cellsmall(A):
    lib, P, X, out, ws, nb = _refusal_args(A)
    return _call(lib, P(X), 300, 0.0005, P(out), 512, 4096, "count", None, P(ws), nb, B_S())


@_refusal("null-cloud", -1)
def _r_nullcloud(A):
    lib, P, X, out, ws, nb = _refusal_args(A)
    return _call(lib, None, 300, 0.05, P(out), 512, 4096, "count", None, P(ws), nb, B_S())


@_refusal("null-count", -1)
def _r_nullcount(A):
    lib, P, X, out, ws, nb = _refusal_args(A)
    return _call(lib, P(X), 300, 0.05, P(out), 512, 4096, None, None, P(ws), nb, B_S())


@_refusal("null-seeds-with-capacity", -1)
def _r_nullseeds(A):
    lib, P, X, out, ws, nb = _refusal_args(A)
    return _call(lib, P(X), 300, 0.05, None, 512, 4096, "count", None, P(ws), nb, B_S())


@_refusal("null-workspace", -1)
def _r_nullws(A):
    lib, P, X, out, ws, nb = _refusal_args(A)
    return _call(lib, P(X), 300, 0.05, P(out), 512, 4096, "count", None, None, nb, B_S())


@_refusal("non-finite-point", -1)
def _r_nonfinite(A):
    from sapcu_amd import _lib, testing as T
    lib = _lib.load()
    cloud = T.sphere_cloud(300, 1)
    cloud[17, 1] = np.inf
    need = int(lib.sapcu_dense_seeds_workspace_bytes(300, 4096))
    X, out, ws = A.inp(cloud, name="cloud"), A.out((512, 3), F64, name="seeds_out"), A.ws(need, name="seed workspace")
    return _call(lib, _lib.ptr(X), 300, 0.05, _lib.ptr(out), 512, 4096, "count", None, _lib.ptr(ws), need, B_S())


@_refusal("voxel-key-outside-int", -1)
def _r_hugekey(A):
    from sapcu_amd import _lib, testing as T
    lib = _lib.load()
    cloud = T.sphere_cloud(300, 1)
    cloud[5, 0] = 1e7
    need = int(lib.sapcu_dense_seeds_workspace_bytes(300, 4096))
    X, out, ws = A.inp(cloud, name="cloud"), A.out((512, 3), F64, name="seeds_out"), A.ws(need, name="seed workspace")
    return _call(lib, _lib.ptr(X), 300, 0.05, _lib.ptr(out), 512, 4096, "count", None, _lib.ptr(ws), need, B_S())


def B_S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.gpu
@pytest.mark.parametrize("r", SEED_REFUSALS, ids=[r[0] for r in SEED_REFUSALS])
def test_seed_refusal_launches_nothing(r):
    from guarded import Arena
    id_, want, run = r
    A = Arena("guard", 0xFF, U.dev())
    rc = run(A)
    torch.cuda.synchronize()
    assert rc == want, "%s returned %d, expected %d" % (id_, rc, want)
    A.check()
    for g in A.outs + A.wss:                                             # nothing ran: outputs and workspaces keep every byte
        assert bool((g.payload_bits() == 0xFF).all()), "%s: %s was written by a refused call" % (id_, g.name)


def test_every_entry_point_of_the_seeds_header_has_a_bounds_case():
    """The gate of tests/test_guarded.py over include/sapcu_seeds.h: the binding's second table equals the header, every
    pointer-taking entry point has a case above, every sizer is used at exactly its size — and sapcu.h's table is untouched."""
    import test_guarded as TG
    from sapcu_amd import _lib
    decl = seeds_header_entry_points()
    assert set(decl) == set(_lib.SEEDS_EXPORTS) == {"sapcu_dense_seeds_workspace_bytes", "sapcu_dense_seeds_f64"}
    assert set(TG.header_entry_points()) == set(_lib.EXPORTS) and not set(_lib.EXPORTS) & set(_lib.SEEDS_EXPORTS)
    covered, used = set(), set()
    for c in SEED_CASES:
        assert c.entry_points, c.id
        covered.update(c.entry_points)
        used.update(c.sizers)

    def uncovered(cov):
        return sorted(n for n, args in decl.items() if "*" in args and n not in cov)
    assert covered <= set(decl) and not uncovered(covered), uncovered(covered)
    assert uncovered(covered - {"sapcu_dense_seeds_f64"}) == ["sapcu_dense_seeds_f64"]          # the gate itself
    assert {n for n in decl if n.endswith("workspace_bytes")} <= used
    assert {r[0] for r in SEED_REFUSALS} >= {"workspace-one-byte-short", "workspace-4-byte-aligned", "n-zero", "cell-zero",
                                             "null-cloud", "non-finite-point"}


def test_seed_argument_refusals_need_no_gpu():
    """Everything include/sapcu_seeds.h promises to refuse before any launch or copy is refused on a machine without a GPU
    (the pointers are never dereferenced), and the sizer answers -1 for what the flood would refuse."""
    from sapcu_amd import _lib
    lib = _lib.load()
    assert lib.sapcu_abi_version() == _lib.ABI_VERSION == 2
    size = lib.sapcu_dense_seeds_workspace_bytes
    assert size(0, 10) == -1 and size(10, 0) == -1 and size((1 << 28) + 1, 10) == -1 and size(10, (1 << 28) + 1) == -1
    need = size(100, 1000)
    assert need > 0 and size(100, 2000) > need and size(200, 1000) > need
    count = ctypes.c_int64(5)
    fake = ctypes.c_void_p(4096)                                     # 8-byte aligned, never touched by a refused call

    def call(cloud=fake, n=100, cell=0.05, seeds=fake, cap=10, maxv=1000, cnt=ctypes.byref(count), ws=fake, nbytes=need):
        return lib.sapcu_dense_seeds_f64(cloud, n, cell, seeds, cap, maxv, cnt, None, ws, nbytes, None)
    for kw in (dict(cloud=None), dict(cnt=None), dict(ws=None), dict(seeds=None), dict(n=0), dict(n=-3), dict(n=(1 << 28) + 1),
               dict(maxv=0), dict(maxv=(1 << 28) + 1), dict(cap=-1), dict(cell=0.0), dict(cell=-0.03), dict(cell=float("nan")),
               dict(cell=float("inf")), dict(cell=3.0), dict(cell=0.0009), dict(nbytes=need - 1), dict(nbytes=0),
               dict(ws=ctypes.c_void_p(4100))):
        assert call(**kw) == -1, kw
        assert lib.sapcu_last_error()
    assert count.value == 5                                          # a refused call does not touch *count_host either


# ================================================================================================ 6: the public interface
@pytest.mark.gpu
def test_generator_seed_source_device_equals_upsample_seeds_of_the_reference_seeds(weights):
    import sapcu_amd
    from sapcu_amd import testing as T
    fn, fd, _, _ = U.build_gpu_models(weights)
    g = golden("e2e_upsample.npz")
    cloud = T.sphere_cloud(2048, 0)
    gen = sapcu_amd.Generator3D6(fn, fd, U.dev(), k_neighbors=48, dense_spacing=0.03, batch_size=64)
    assert gen.seed_source == "inprocess"                            # the default did not move
    fn.knn_cache_mode = "reference"
    fn._knn_cache.clear()
    want = gen.upsample_seeds(cloud, g["seeds"])
    gen.seed_source = "device"
    seeds = gen._dense_seeds(cloud)
    assert torch.is_tensor(seeds) and seeds.is_cuda and np.array_equal(seeds.cpu().numpy(), g["seeds"])
    fn._knn_cache.clear()
    got = gen.upsample(cloud[None])
    assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)
    fn._knn_cache.clear()
    assert np.array_equal(gen.upsample_seeds(cloud, seeds), want)     # a device tensor of seeds is taken as it is
    empty = sapcu_amd.Generator3D6(fn, fd, U.dev(), k_neighbors=5, dense_spacing=0.05, batch_size=64)
    empty.seed_source = "device"
    assert empty.upsample(T.sphere_cloud(7, 3)).shape == (0, 3)       # tiny7_c050: nothing in the band


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", [2, 3])
def test_whole_cloud_sharded_with_device_seeds_ranks_on_one_gpu(ranks):
    """tests/seeds_rehearsal.py under torch.distributed.run, every rank on cuda:0 over gloo: upsample_cloud_sharded with
    seed_source = "device" (every rank floods, no seed broadcast) against the single-process upsample, bit for bit."""
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "seeds_rehearsal.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=700, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0 and ("SEEDS_REHEARSAL_OK ranks=%d" % ranks) in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
