"""Whole-cloud upsampling across ranks and the device outlier filter (csrc/knn_grid.hip, sapcu_amd/dist.py).

CPU: the aligned row blocks of the sharded filter, numpy's np.mean summation order, and the seed broadcast / chunk-sum and
keep-mask gathers over gloo with a stand-in generator.  GPU: grid kNN == the brute-force kernel bit for bit, the device
statistics == numpy bit for bit, keep sets == the reference runs', and the sharded whole-cloud entry points == the
single-process ones (2 and 3 ranks on one GPU over gloo, RCCL world 1)."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

import sapcu_amd
from sapcu_amd import dist as sdist
from sapcu_amd import generation as gen
from sapcu_amd import testing as T


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


# ------------------------------------------------------------------------------------------------------------------ CPU
def _np_leaf(a):
    n = len(a)
    if n < 8:
        r = 0.0
        for v in a:
            r += v
        return r
    r, i = list(a[:8]), 8
    while i < n - n % 8:
        for j in range(8):
            r[j] += a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[i:]:
        res += v
    return res


def _np_pairwise(a):
    if len(a) <= 128:
        return _np_leaf(a)
    n2 = len(a) // 2
    n2 -= n2 % 8
    return _np_pairwise(a[:n2]) + _np_pairwise(a[n2:])


@pytest.mark.parametrize("bufsize", [4096, 8192, 16384])
def test_numpy_mean_order_model(bufsize):
    """The contract the device statistics implement, held to this numpy: row means = the pairwise leaf / kk; the global mean =
    pairwise sums of bufsize-element chunks of the flattened table, added in sequence from 0.0."""
    old = np.getbufsize()
    try:
        np.setbufsize(bufsize)
        rng = np.random.default_rng(1)
        for n in (1, 7, 29, 30, 4095, 4097, 9001):
            kk = min(30, n)
            d = rng.random((n, kk)) * rng.random((n, 1)) * 0.01
            assert np.array_equal(np.array([_np_leaf(list(r)) / kk for r in d]), np.mean(d, axis=1))
            flat = d.ravel().tolist()
            total = 0.0
            for s in range(0, len(flat), bufsize):
                total += _np_pairwise(flat[s:s + bufsize])
            assert total / (n * kk) == np.mean(d), n
    finally:
        np.setbufsize(old)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_outlier_row_ranges_are_aligned_and_cover(world):
    for bufsize in (4096, 8192, 16384):
        for n in (1, 29, 30, 4095, 4096, 4097, 8192, 12289, 40000, 385582):
            kk = min(30, n)
            align = bufsize // math.gcd(kk, bufsize)
            assert gen.outlier_row_align(kk, bufsize) == align
            r = sdist.outlier_row_ranges(n, world, kk, bufsize)
            assert len(r) == world and r[0][0] == 0 and r[-1][1] == n
            assert all(r[i][1] == r[i + 1][0] for i in range(world - 1))
            for s, e in r:
                assert s <= e and (s % align == 0 or s == n) and (e % align == 0 or e == n)
                assert s == n or s * kk % bufsize == 0            # every chunk of np.mean lies inside one rank's rows
                assert gen.outlier_filter_range(n, (s, e), bufsize) == (s, e)     # the filter's own check takes every range
            assert sum(gen.outlier_chunk_count(e - s, kk, bufsize) for s, e in r) == -(-n * kk // bufsize)
            blocks = -(-n // align)
            if blocks < world:
                assert sum(1 for s, e in r if e == s) == world - blocks


def test_outlier_filter_range_rejects_unaligned_rows():
    n = 40000
    for rows in ((0, 4095), (1, 4096), (4096, 8000), (4097, 4097 + 4096), (0, n + 1), (5000, 4096), (-1, 0)):
        with pytest.raises(ValueError):
            gen.outlier_filter_range(n, rows, 8192)
    for rows in ((0, n), (0, 4096), (36864, n), (n, n), (4096, 4096), (0, 0)):
        assert gen.outlier_filter_range(n, rows, 8192) == rows


def _cloud_gloo_worker(rank, world, port, n, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ranges = sdist.outlier_row_ranges(n, world)

        class FakeGen:                      # stands in for the GPU stages: the broadcasts and gathers are what is under test
            device = torch.device("cpu")
            model1 = type("M", (), {"knn_cache_mode": "reference"})()
            floods = 0
            sums_seen = None

            def _dense_seeds(self, data):
                self.floods += 1
                return np.arange(n * 3, dtype=np.float64).reshape(n, 3) + data.sum()

            def refine(self, cloud, s):
                return s * 2.0 + 1.0, None, None

            def outlier_filter_rows(self, pts, rows, gather_sums):
                s, e = gen.outlier_filter_range(pts.shape[0], rows)       # the real filter's range check, empty ranks included
                assert (s, e) == ranges[rank]
                local = torch.full((gen.outlier_chunk_count(e - s, min(30, n)),), float(rank + 1), dtype=torch.float64)
                self.sums_seen = gather_sums(local)
                return (pts[s:e, 0].long() // 3) % 3 != 0, local

            def check_numeric_guards(self):
                pass

        g = FakeGen()
        data = np.full((4, 3), 0.5)
        out = sapcu_amd.dist.upsample_cloud_sharded(g, data)
        refined = (np.arange(n * 3, dtype=np.float64).reshape(n, 3) + 6.0) * 2.0 + 1.0
        expect = refined[(refined[:, 0].astype(np.int64) // 3) % 3 != 0]
        sums = np.concatenate([np.full(gen.outlier_chunk_count(e - s, min(30, n)), float(r + 1)) for r, (s, e) in enumerate(ranges)])
        q.put((rank, g.floods, bool(np.array_equal(out, expect)), bool(np.array_equal(g.sums_seen.numpy(), sums)),
               g.model1.knn_cache_mode))
    finally:
        dist.destroy_process_group()


def _run_gloo(world, n):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_cloud_gloo_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
    assert [r[0] for r in res] == list(range(world))
    assert [r[1] for r in res] == [1] + [0] * (world - 1), res          # seeds flooded once, on rank 0
    assert all(r[2] for r in res), res                                   # every rank: the same filtered cloud
    assert all(r[3] for r in res), res                                   # every rank: all chunk sums, in rank order
    assert all(r[4] == "reference" for r in res)


@pytest.mark.parametrize("n", [1, 5000, 12289])
def test_cloud_sharded_gloo_world2(n):
    _run_gloo(2, n)


@pytest.mark.parametrize("n", [5, 40000])
def test_cloud_sharded_gloo_world8(n):
    """n = 5: one block, ranks 1..7 filter nothing; n = 40000: ten 4096-row blocks, two per rank, ranks 5..7 empty."""
    _run_gloo(8, n)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int64)


def _check_grid(pts, k, rows, cell_size=0.0):
    info = []
    idx, dist = gen.knn_self_grid(pts, k, rows, cell_size, info)
    ref_idx, ref_dist, _ = gen.knn_gather(pts, pts[rows[0]:rows[1]].contiguous(), k, want_dist=True, want_patch=False)
    assert torch.equal(idx, ref_idx), (k, rows, cell_size, info)
    assert torch.equal(_bits(dist), _bits(ref_dist)), (k, rows, cell_size, info)
    return info


def _point_sets():
    rng = np.random.default_rng(7)
    base = rng.random((4000, 3))
    lattice = np.stack(np.meshgrid(np.arange(24), np.arange(24), np.arange(24), indexing="ij"), -1).reshape(-1, 3)
    return {
        "cube": rng.random((20000, 3)),
        "two_clusters": np.concatenate([rng.random((8000, 3)) * 0.01, rng.random((8000, 3)) * 0.01 + 500.0]),
        "plane": np.concatenate([rng.random((12000, 2)) * 2 - 1, np.full((12000, 1), 0.25)], axis=1),
        "duplicates": base[rng.permutation(np.repeat(np.arange(4000), 3))],
        "lattice": lattice[rng.permutation(lattice.shape[0])].astype(np.float64),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube", "two_clusters", "plane", "duplicates", "lattice"])
def test_grid_knn_equals_brute_force(name):
    pts = _dev(_point_sets()[name])
    n = pts.shape[0]
    for k in (1, 16, 30, 48, 64):
        for rows in ((0, n), (n // 7, n - n // 5)):
            info = _check_grid(pts, k, rows)
            assert info[0] == 1                                           # n >= 4096: the grid ran
        info = _check_grid(pts, k, (n // 3, n // 3 + 999), 1e-9)          # tiny cells: clamped to <= 2n + 64, many shells
        assert info[0] == 1 and info[1] * info[2] * info[3] > n // 4, info
        info = _check_grid(pts, k, (n // 2, n // 2 + 777), 1e9)           # one cell: every point in shell 0
        assert info[:4] == [1, 1, 1, 1], info


@pytest.mark.gpu
def test_grid_knn_on_the_real_seed_cloud():
    """The 385 582 seeds of the whole-cloud workload (sphere 5000, spacing 0.004)."""
    pts = _dev(gen.dense_seeds(T.sphere_cloud(5000, 0), 0.004))
    n = pts.shape[0]
    assert n == 385582
    info = _check_grid(pts, 30, (0, n))
    assert info[0] == 1
    for k in (1, 16, 48, 64):
        _check_grid(pts, k, (1000, 201001))
    _check_grid(pts, 30, (123457, 180001), 0.002)
    _check_grid(pts, 30, (5, 40005), 0.05)


@pytest.mark.gpu
def test_grid_knn_small_sets_and_fallback():
    rng = np.random.default_rng(11)
    for k in (1, 16, 30, 48, 64):
        pts = _dev(rng.random((k, 3)))                                     # n = k
        assert _check_grid(pts, k, (0, k))[0] == 0                         # automatic below 4096 points: brute force
        assert _check_grid(pts, k, (0, k), 0.05)[0] == 1
        assert _check_grid(pts, k, (k // 3, k), 1e-9)[0] == 1
    one = _dev(rng.random((1, 3)))
    assert _check_grid(one, 1, (0, 1), 0.1)[:4] == [1, 1, 1, 1]
    _check_grid(one, 1, (0, 1))
    for bad in (np.nan, np.inf, 1e200):
        a = rng.random((6000, 3))
        a[77, 1] = bad
        pts = _dev(a)
        for cs in (0.0, 0.01):
            assert _check_grid(pts, 30, (0, 6000), cs)[0] == 0             # non-finite / huge coordinates: brute force
    with pytest.raises(sapcu_amd.SapcuError):
        gen.knn_self_grid(_dev(rng.random((100, 3))), 65)


@pytest.mark.gpu
@pytest.mark.parametrize("bufsize", [None, 4096])
def test_outlier_statistics_equal_numpy_bit_for_bit(bufsize):
    old = np.getbufsize()
    try:
        if bufsize:
            np.setbufsize(bufsize)
        rng = np.random.default_rng(3)
        for n in (1, 29, 30, 4095, 4096, 4097, 385582):
            kk = min(30, n)
            d = np.sort(rng.random((n, kk)) * rng.random((n, 1)) * 0.05, axis=1)
            d[:, 0] = 0.0
            row_mean, sums = gen.outlier_stats_device(_dev(d))
            assert np.array_equal(row_mean.cpu().numpy(), np.mean(d, axis=1)), n
            assert gen.outlier_global_mean(sums.cpu(), n * kk) == np.mean(d), n
            # aligned row blocks (the sharded filter) give the same chunk sums, in order
            align = gen.outlier_row_align(kk)
            if n > align:
                parts = [gen.outlier_stats_device(_dev(d[s:s + align]))[1] for s in range(0, n, align)]
                assert torch.equal(torch.cat(parts), sums), n
    finally:
        np.setbufsize(old)


@pytest.mark.gpu
def test_device_filter_reproduces_the_reference_keep_sets():
    cases = [(golden(f)["unfiltered"], golden(f)["filtered"]) for f in ("e2e_upsample.npz", "e2e_default.npz", "scale16.npz")]
    g = golden("shape_suite.npz")
    cases += [(g[s + "_unfiltered"], g[s + "_filtered"]) for s in ("sphere", "torus", "cube", "cylinder", "two_spheres", "icosahedron")]
    for unf, filt in cases:
        keep = gen.outlier_filter_device(_dev(unf), 1.5)
        assert keep.dtype == torch.bool and keep.is_cuda
        keep = keep.cpu().numpy()
        assert np.array_equal(unf[keep], filt)


@pytest.mark.gpu
@pytest.mark.parametrize("n,world", [(5000, 8), (7341, 3), (40000, 8), (1, 2)])
def test_device_filter_on_every_rank_range_including_empty_ones(n, world):
    """The real outlier_filter_device on each range outlier_row_ranges hands the ranks, empty ones included (the ranks past the
    last 4096-row block), in one process: gather_sums returns the whole cloud's chunk sums, as the all-gather would."""
    pts = _dev(np.random.default_rng(n).random((n, 3)))
    full_keep = gen.outlier_filter_device(pts, 1.5)
    _, full_dist = gen.knn_self_grid(pts, min(30, n))
    _, full_sums = gen.outlier_stats_device(full_dist)
    ranges = sdist.outlier_row_ranges(n, world)
    assert any(e == s for s, e in ranges)
    local_sums = []
    for s, e in ranges:
        keep, sums = gen.outlier_filter_device(pts, 1.5, (s, e), lambda _: full_sums)
        assert keep.shape == (e - s,) and keep.dtype == torch.bool
        assert torch.equal(keep, full_keep[s:e]), (s, e)
        local_sums.append(sums)
    assert torch.equal(torch.cat(local_sums), full_sums)


@pytest.mark.gpu
def test_device_filter_equals_the_host_filter_on_a_385k_refined_cloud(weights):
    import gpu_utils as U
    fn, fd, _, _ = U.build_gpu_models(weights)
    fn.knn_cache_mode = "fresh"
    g = sapcu_amd.Generator3D6(fn, fd, U.dev(), k_neighbors=48, batch_size=4096)
    assert g.outlier_filter_impl == "host"
    cloud = T.sphere_cloud(5000, 0)
    seeds = gen.dense_seeds(cloud, 0.004)
    with torch.no_grad():
        refined, _, _ = g.refine(_dev(cloud), _dev(seeds))
    host = g.outlier_filter(refined)
    g.outlier_filter_impl = "device"
    device = g.outlier_filter(refined)
    assert device.dtype == np.bool_ and np.array_equal(host, device)
    assert 0.85 < host.mean() < 1.0
    _check_grid(refined, 30, (0, refined.shape[0]))
    g.outlier_filter_impl = "other"
    with pytest.raises(ValueError):
        g.outlier_filter(refined)


def _rehearsal_env():
    return dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", [2, 3])
def test_whole_cloud_sharded_ranks_on_one_gpu(ranks, tmp_path):
    """tests/cloud_rehearsal.py under torch.distributed.run, every rank on cuda:0 over gloo: upsample_cloud_sharded,
    process_cloud_sharded and process_files_sharded against their single-process counterparts, bit for bit / byte for byte."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "cloud_rehearsal.py"), "gloo", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=_rehearsal_env())
    assert r.returncode == 0 and ("CLOUD_REHEARSAL_OK ranks=%d" % ranks) in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.gpu
def test_rccl_world1_whole_cloud_on_device_tensors(tmp_path):
    """One nccl (RCCL) rank with device_id=cuda:0: the seed broadcast and the chunk-sum / keep-mask gathers on device tensors."""
    env = dict(_rehearsal_env(), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cloud_rehearsal.py"), "nccl", str(tmp_path)], capture_output=True,
                       text=True, timeout=900, env=env)
    assert r.returncode == 0 and "CLOUD_REHEARSAL_OK ranks=1 backend=nccl" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
