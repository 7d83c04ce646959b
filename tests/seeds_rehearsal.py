"""Worker of tests/test_gpu_seeds.py::test_whole_cloud_sharded_with_device_seeds_ranks_on_one_gpu — run under
torch.distributed.run with 2 or 3 ranks, ALL on cuda:0, gloo backend: sapcu_amd.dist.upsample_cloud_sharded with
seed_source = "device" (every rank floods its own copy of the seeds on the GPU; no seed broadcast) against the rank's own
single-process upsample with the host seeds (knn_cache_mode 'fresh'), bit for bit."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SPACING = 0.01           # sphere 2048 -> ~24 k seeds: six 4096-row blocks of the outlier filter, a split for 2 and 3 ranks


def main():
    import sapcu_amd
    from sapcu_amd import dist as sdist, generation as gen_mod, testing as T
    from conftest import FD_KW, FN_KW, GOLDEN
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        fn = sapcu_amd.ImprovedSNNNormalEstimation(**FN_KW)
        fd = sapcu_amd.EnhancedSNNDistanceEstimation(**FD_KW)
        fn.load_state_dict(T.conditioned_state_dict(fn.state_dict(), 0, bn_stats=dict(np.load(os.path.join(GOLDEN, "bn_calib_fn.npz")))))
        fd.load_state_dict(T.conditioned_state_dict(fd.state_dict(), 0, bn_stats=dict(np.load(os.path.join(GOLDEN, "bn_calib_fd.npz")))))
        fn, fd = fn.to(dev), fd.to(dev)
        gen = sapcu_amd.Generator3D6(fn, fd, dev, k_neighbors=48, dense_spacing=SPACING, batch_size=256)
        cloud = T.sphere_cloud(2048, 0)
        fn.knn_cache_mode = "fresh"
        assert gen.seed_source == "inprocess"
        single = gen.upsample(cloud[None])                              # host seeds, one process
        host_seeds = gen_mod.dense_seeds(cloud, SPACING)
        gen.seed_source = "device"
        calls = []
        real = sdist.broadcast_seeds
        sdist.broadcast_seeds = lambda *a, **k: calls.append(1) or real(*a, **k)
        try:
            sharded = sdist.upsample_cloud_sharded(gen, cloud[None])
        finally:
            sdist.broadcast_seeds = real
        assert not calls, "rank %d: the seeds were broadcast although every rank floods on its device" % rank
        assert np.array_equal(gen._dense_seeds(cloud).cpu().numpy(), host_seeds)
        assert host_seeds.shape[0] > 4096 and all(e > s for s, e in sdist.outlier_row_ranges(host_seeds.shape[0], world))
        assert sharded.dtype == np.float64 and sharded.shape == single.shape, (sharded.shape, single.shape)
        assert np.array_equal(sharded, single), "rank %d: sharded whole cloud with device seeds differs from the single-process upsample" % rank
        dist.barrier()
        if rank == 0:
            print("SEEDS_REHEARSAL_OK ranks=%d seeds=%d" % (world, host_seeds.shape[0]), flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
