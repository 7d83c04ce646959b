"""Multi-GPU: shard the query points, one process per GPU, one all-gather of the refined cloud.

The path shards embarrassingly: every seed is independent given the replicated
input cloud (<= 120 KB) and weights (33 MB).  Rank r refines the contiguous range
``seeds[r*ceil(n/G) : (r+1)*ceil(n/G)]``; the only exchange is ONE all-gather of the refined
points per cloud (``[ceil(n/G), 3]`` f64 per rank, last rank padded, trimmed after).  On the
fully connected xGMI mesh that is ~1 MB per rank — latency bound; it is issued once, not per batch.
``torch.distributed`` backend "nccl" is RCCL on ROCm; "gloo" runs the same code on CPU tensors
(tests).

fn's shape-keyed neighbour cache (fn/snn_coder.py:47-59) makes reference-mode results depend on
which batch a process sees first, so a sharded run cannot reproduce a single-process reference run
bit for bit; sharded runs therefore use ``knn_cache_mode='fresh'`` (stated in DESIGN.md).
"""
import os

import numpy as np
import torch
import torch.distributed as dist


def visible_gpu_count(sysfs_root="/sys/class/kfd/kfd/topology/nodes", dev_root="/dev/dri", environ=None):
    """Number of GPUs a process started from here would see — WITHOUT loading the HIP runtime (a launcher parent must stay
    GPU-free so that it may start ranks; touching HIP and then exec'ing / forking rank processes is what takes boxes down).
    Counts the KFD topology nodes that are GPUs (``simd_count`` > 0; CPU nodes have 0) and whose render node
    ``/dev/dri/renderD<drm_render_minor>`` this process can open (a container sees every node of the host in sysfs but only its
    own device files), then applies the runtime's visibility lists the way ROCm does: ROCR_VISIBLE_DEVICES filters the
    physical list, HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES index into the result (an empty string hides everything; an
    entry the list cannot resolve ends it, as in the runtime).  Returns None when there is no KFD topology to read (not a ROCm
    box) — the caller decides what that means."""
    env = os.environ if environ is None else environ
    try:
        nodes = sorted(os.listdir(sysfs_root), key=lambda s: (len(s), s))
    except OSError:
        return None
    gpus = []
    for nd in nodes:
        try:
            props = dict(line.split()[:2] for line in open(os.path.join(sysfs_root, nd, "properties")) if len(line.split()) >= 2)
        except OSError:
            continue
        if int(props.get("simd_count", "0")) <= 0:
            continue
        minor = int(props.get("drm_render_minor", "-1"))
        node = os.path.join(dev_root, "renderD%d" % minor)
        if minor < 0 or not os.access(node, os.R_OK | os.W_OK):
            continue
        gpus.append(nd)
    count = len(gpus)

    def apply(var, n):
        if var not in env:
            return n
        entries = [e.strip() for e in env[var].split(",")] if env[var].strip() else []
        k = 0
        for e in entries:
            if e.isdigit():
                if int(e) >= n:
                    break
            elif not e.upper().startswith("GPU-"):          # neither an index nor a UUID: the runtime stops here
                break
            k += 1
        return min(k, n)

    count = apply("ROCR_VISIBLE_DEVICES", count)
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        count = apply(var, count)
    return count


def shard_range(n, rank, world):
    """Contiguous [start, end) of rank's share of n items; equal ceil(n/world) slabs, last ones short."""
    per = -(-n // world) if world > 0 else n
    s = min(n, rank * per)
    return s, min(n, s + per)


def gather_refined(local, n_total, group=None):
    """All-gather row slabs of a [n_local, C] tensor sharded by ``shard_range`` -> [n_total, C] on every rank."""
    world = dist.get_world_size(group)
    per = -(-n_total // world)
    dev = local.device
    if local.is_cuda and dist.get_backend(group) == "gloo":
        local = local.cpu()               # rehearsals of the N > 1 path on one GPU: gloo moves host memory
    padded = local.new_zeros((per,) + tuple(local.shape[1:]))
    padded[: local.shape[0]] = local
    out = local.new_empty((world * per,) + tuple(local.shape[1:]))
    dist.all_gather_into_tensor(out, padded.contiguous(), group=group)
    return out[:n_total].to(dev)


def upsample_sharded(generator, cloud_dev, seeds_dev, group=None):
    """Refine this rank's shard with ``generator.refine`` and all-gather the refined cloud.
    Returns (refined [n,3] f64 on every rank, (start, end) of the local shard)."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    n = seeds_dev.shape[0]
    s, e = shard_range(n, rank, world)
    model = generator.model1
    old = getattr(model, "knn_cache_mode", None)
    if old is not None:
        model.knn_cache_mode = "fresh"
    try:
        if e > s:
            local, _, _ = generator.refine(cloud_dev, seeds_dev[s:e])
        else:
            local = seeds_dev.new_empty((0, 3))
    finally:
        if old is not None:
            model.knn_cache_mode = old
    return gather_refined(local, n, group), (s, e)


# -- the whole cloud across ranks: seeds -> sharded refine -> sharded outlier filter (-> FPS) ---------------------------------
# Every rank returns what Generator3D6.upsample returns in one process with knn_cache_mode='fresh', bit for bit: the seeds are
# flooded once on rank 0 and broadcast, the refine is upsample_sharded, and the outlier filter's rows are cut into blocks that
# hold whole chunks of np.mean (generation.outlier_row_align), so that the chunk sums of all ranks, gathered in rank order, are
# the single-process chunk sums.  Collectives: two broadcasts (seed count, seeds), the refine's all-gather, one all-gather of the
# chunk sums and one of the keep mask.  gloo moves host tensors, nccl (RCCL) device tensors, as in gather_refined.
# With generator.seed_source == "device" every rank floods its own copy of the seeds on its GPU (csrc/dense_seeds_dev.hip is
# deterministic) and the two broadcasts fall away.

def outlier_row_ranges(n, world, kk=None, bufsize=None):
    """[(start, end)] of every rank's rows of the outlier filter over n points: contiguous, in rank order, each start and each
    end but n a multiple of bufsize / gcd(kk, bufsize) rows (4096 for kk = 30 and numpy's default buffer); equal numbers of
    whole blocks per rank, so ranks past the last block get empty ranges."""
    from . import generation
    kk = min(generation.OUTLIER_K, n) if kk is None else kk
    align = generation.outlier_row_align(kk, bufsize)
    blocks = -(-n // align)
    per = -(-blocks // world)
    return [(min(n, r * per * align), min(n, (r + 1) * per * align)) for r in range(world)]


def _src0(group):
    return 0 if group is None else dist.get_global_rank(group, 0)


def _comm_device(group, dev):
    return torch.device("cpu") if dist.get_backend(group) == "gloo" else dev


def broadcast_seeds(generator, data, group=None):
    """The seeds of cloud ``data`` [N,3], flooded ONCE on the group's rank 0 (``generator._dense_seeds``: the in-process
    generator with all its host threads) and broadcast — the count, then the array.  Returns f64 [n,3] on generator.device."""
    rank = dist.get_rank(group)
    dev = torch.device(generator.device)
    cdev = _comm_device(group, dev)
    seeds = None
    if rank == 0:
        seeds = torch.from_numpy(np.ascontiguousarray(generator._dense_seeds(data), dtype=np.float64).reshape(-1, 3))
    count = torch.tensor([seeds.shape[0] if rank == 0 else 0], dtype=torch.int64, device=cdev)
    dist.broadcast(count, src=_src0(group), group=group)
    n = int(count.item())
    buf = seeds.to(cdev) if rank == 0 else torch.empty((n, 3), dtype=torch.float64, device=cdev)
    if n:
        dist.broadcast(buf, src=_src0(group), group=group)
    return buf.to(dev)


def _all_gather_rows(local, counts, group=None):
    """All-gather of per-rank row blocks whose sizes ``counts`` every rank knows -> their concatenation in rank order."""
    world = len(counts)
    per = max(counts)
    dev = local.device
    if local.is_cuda and dist.get_backend(group) == "gloo":
        local = local.cpu()
    padded = local.new_zeros((per,) + tuple(local.shape[1:]))
    padded[: local.shape[0]] = local
    out = local.new_empty((world * per,) + tuple(local.shape[1:]))
    dist.all_gather_into_tensor(out, padded.contiguous(), group=group)
    return torch.cat([out[r * per: r * per + counts[r]] for r in range(world)]).to(dev)


def upsample_cloud_sharded(generator, data, group=None):
    """``generator.upsample(data)`` over the ranks of ``group``: every rank returns the same filtered ndarray [M',3] f64, bit for
    bit the single-process result with ``knn_cache_mode='fresh'`` (the sharded refine needs it; see upsample_sharded)."""
    from . import generation
    data = np.squeeze(data, 0) if np.ndim(data) == 3 else np.asarray(data)
    generation.require_finite("the cloud", data)               # as generator.upsample: ValueError on every rank, before any launch
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    if getattr(generator, "seed_source", None) == "device":     # every rank floods its own copy: deterministic, nothing to send
        seeds_dev = generator._dense_seeds(data)
    else:
        seeds_dev = broadcast_seeds(generator, data, group)
    n = seeds_dev.shape[0]
    if n == 0:                              # nothing in the distance band (Generator3D6.upsample_seeds)
        return np.zeros((0, 3), dtype=np.float64)
    cloud_dev = torch.as_tensor(np.ascontiguousarray(data, dtype=np.float64), device=generator.device)
    kk = min(generation.OUTLIER_K, n)
    bufsize = np.getbufsize()
    ranges = outlier_row_ranges(n, world, kk, bufsize)
    chunks = [generation.outlier_chunk_count(e - s, kk, bufsize) for s, e in ranges]
    with torch.no_grad():
        refined, _ = upsample_sharded(generator, cloud_dev, seeds_dev, group)
        keep_local, _ = generator.outlier_filter_rows(refined, ranges[rank], lambda sums: _all_gather_rows(sums, chunks, group))
        keep = _all_gather_rows(keep_local.to(torch.uint8), [e - s for s, e in ranges], group)
    generator.check_numeric_guards()
    return refined.cpu().numpy()[keep.cpu().numpy().astype(bool)]


def process_cloud_sharded(cloud, generator, target_points, group=None):
    """``pipeline.process_cloud`` on top of upsample_cloud_sharded: every rank returns the same [target_points, 3] FPS output."""
    from . import pipeline
    return pipeline._process_cloud_with(cloud, lambda d: upsample_cloud_sharded(generator, d, group), generator.device,
                                         target_points)


def process_files_sharded(inputs, outputs, generator, target_points, group=None):
    """generate.py's loop over a directory of clouds (BASELINE config 4) across ranks: file i goes to rank i % world, which
    writes outputs[i] with ``pipeline.process_file``; no collective but the closing barrier.  The files are refined with
    ``knn_cache_mode='fresh'`` (a rank's cache history differs from one process's), so each output is byte-identical to
    process_file's in that mode.  Returns the indices of the files this rank processed.  A rank whose file fails still reaches
    the barrier (it is in a ``finally``), so the other ranks are released and the error is raised on that rank alone."""
    from . import pipeline
    if len(inputs) != len(outputs):
        raise ValueError("process_files_sharded: %d inputs but %d outputs" % (len(inputs), len(outputs)))
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    mine = list(range(rank, len(inputs), world))
    model = generator.model1
    old = getattr(model, "knn_cache_mode", None)
    if old is not None:
        model.knn_cache_mode = "fresh"
    try:
        for i in mine:
            pipeline.process_file(inputs[i], outputs[i], generator, target_points)
    finally:
        if old is not None:
            model.knn_cache_mode = old
        dist.barrier(group=group)
    return mine
