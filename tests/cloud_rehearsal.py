"""Worker of tests/test_cloud_sharded.py::test_whole_cloud_sharded_ranks_on_one_gpu — run under torch.distributed.run with 2 or 3
ranks, ALL on cuda:0, gloo backend: the real Generator3D6 through sapcu_amd.dist.upsample_cloud_sharded / process_cloud_sharded /
process_files_sharded; every rank checks the results against its own single-process run (knn_cache_mode 'fresh'), bit for bit,
and rank 0 checks the written files byte for byte against pipeline.process_file's.

`cloud_rehearsal.py nccl DIR` (test_rccl_world1_whole_cloud_on_device_tensors): ONE rank with the nccl (= RCCL) backend and
device_id=cuda:0 — the seed broadcast and the gathers of the sharded filter on device tensors."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SPACING = 0.01           # sphere 2048 -> ~24 k seeds: six 4096-row blocks of the outlier filter, a split for 2 and 3 ranks
SMALL_SPACING = 0.015    # sphere 2048 -> 7341 seeds: two blocks, so the third of 3 ranks filters no rows
FILE_SPACING = 0.02      # the three small clouds of process_files_sharded


def main():
    import sapcu_amd
    from sapcu_amd import dist as sdist, generation as gen_mod, pipeline, testing as T
    from conftest import FD_KW, FN_KW, GOLDEN
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    backend = sys.argv[1]
    outdir = sys.argv[2]
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        fn = sapcu_amd.ImprovedSNNNormalEstimation(**FN_KW)
        fd = sapcu_amd.EnhancedSNNDistanceEstimation(**FD_KW)
        fn.load_state_dict(T.conditioned_state_dict(fn.state_dict(), 0, bn_stats=dict(np.load(os.path.join(GOLDEN, "bn_calib_fn.npz")))))
        fd.load_state_dict(T.conditioned_state_dict(fd.state_dict(), 0, bn_stats=dict(np.load(os.path.join(GOLDEN, "bn_calib_fd.npz")))))
        fn, fd = fn.to(dev), fd.to(dev)
        gen = sapcu_amd.Generator3D6(fn, fd, dev, k_neighbors=48, dense_spacing=SPACING, batch_size=256)
        cloud = T.sphere_cloud(2048, 0)

        # (1) the whole upsample: single process ('fresh' cache) against the sharded run (cache mode left as it was)
        fn.knn_cache_mode = "fresh"
        single = gen.upsample(cloud[None])
        fn.knn_cache_mode = "reference"
        sharded = sdist.upsample_cloud_sharded(gen, cloud[None])
        assert fn.knn_cache_mode == "reference"
        n_seeds = gen_mod.dense_seeds(cloud, SPACING).shape[0]
        ranges = sdist.outlier_row_ranges(n_seeds, world)
        assert n_seeds > 4096 and all(e > s for s, e in ranges), (n_seeds, ranges)        # the filter really splits
        assert sharded.dtype == np.float64 and sharded.shape == single.shape, (sharded.shape, single.shape)
        assert np.array_equal(sharded, single), "rank %d: sharded whole cloud differs from the single-process upsample" % rank

        # (1b) a cloud of two filter blocks: with 3 ranks the last one has an empty range and still joins every collective
        small = sapcu_amd.Generator3D6(fn, fd, dev, k_neighbors=48, dense_spacing=SMALL_SPACING, batch_size=256)
        fn.knn_cache_mode = "fresh"
        single_small = small.upsample(cloud[None])
        small_ranges = sdist.outlier_row_ranges(gen_mod.dense_seeds(cloud, SMALL_SPACING).shape[0], world)
        assert world < 3 or any(e == s for s, e in small_ranges), small_ranges
        sharded_small = sdist.upsample_cloud_sharded(small, cloud[None])
        assert np.array_equal(sharded_small, single_small), "rank %d: sharded small cloud differs (ranges %s)" % (rank, small_ranges)

        # (2) process_cloud: normalise -> upsample -> denormalise -> FPS
        target = 4 * 2048
        fn.knn_cache_mode = "fresh"
        pc = pipeline.process_cloud(cloud, gen, target)
        pcs = sdist.process_cloud_sharded(cloud, gen, target)
        assert pcs.shape == (target, 3) and np.array_equal(pc, pcs), "rank %d: process_cloud_sharded differs" % rank

        # (3) a directory of clouds: file i on rank i % world, byte-identical to process_file
        fgen = sapcu_amd.Generator3D6(fn, fd, dev, k_neighbors=48, dense_spacing=FILE_SPACING, batch_size=256)
        inputs = [os.path.join(outdir, "in_%d.xyz" % i) for i in range(3)]
        outputs = [os.path.join(outdir, "out_%d.xyz" % i) for i in range(3)]
        if rank == 0:
            for i, p in enumerate(inputs):
                np.savetxt(p, T.sphere_cloud(512, 10 + i) * (1.0 + 0.25 * i) + i, fmt="%.6f")
        dist.barrier()
        fn.knn_cache_mode = "reference"
        mine = sdist.process_files_sharded(inputs, outputs, fgen, 1024)
        assert mine == list(range(rank, 3, world)) and fn.knn_cache_mode == "reference"
        if rank == 0:
            fn.knn_cache_mode = "fresh"
            for i in range(3):
                ref = os.path.join(outdir, "ref_%d.xyz" % i)
                pipeline.process_file(inputs[i], ref, fgen, 1024)
                with open(ref, "rb") as a, open(outputs[i], "rb") as b:
                    assert a.read() == b.read(), "file %d differs from process_file's" % i
        dist.barrier()
        if rank == 0:
            print("CLOUD_REHEARSAL_OK ranks=%d backend=%s seeds=%d kept=%d filter_rows=%s small_filter_rows=%s"
                  % (world, dist.get_backend(), n_seeds, sharded.shape[0], ranges, small_ranges), flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
