"""Helpers for the GPU parity tests (and __graft_entry__.smoke / bench cpu-baseline checks)."""
import numpy as np
import torch

from oracle import geom_path as G
from oracle import snn_path as O

FN_HP = {"k_values": [24, 18, 12], "emb_dims": 640, "time_steps_enc": 4, "num_heads": 8}
FD_HP = {"k": 32, "k_scales": [8, 16, 32, 48], "emb_dims": 768, "time_steps_enc": 4, "num_heads": 8}


def dev():
    return torch.device("cuda:0")


def build_gpu_models(weights, fn_over=None, fd_over=None):
    import sapcu_amd
    from conftest import FD_KW, FN_KW
    fn = sapcu_amd.ImprovedSNNNormalEstimation(**dict(FN_KW, **(fn_over or {})))
    fd = sapcu_amd.EnhancedSNNDistanceEstimation(**dict(FD_KW, **(fd_over or {})))
    sdn, sdd = weights("fn", **(fn_over or {})), weights("fd", **(fd_over or {}))
    fn.load_state_dict(sdn, strict=True)
    fd.load_state_dict(sdd, strict=True)
    return fn.to(dev()), fd.to(dev()), sdn, sdd


def build_gpu_models_under(weights, monkeypatch, env, fn_over=None, fd_over=None):
    """Models whose HANDLES were created under the environment switches `env` (sapcu_model_create reads SAPCU_* once; a forward
    never reads the environment): the switches are set, both engines are built, the switches are removed again."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = build_gpu_models(weights, fn_over, fd_over)
    out[0]._engine(), out[1]._engine()
    for k in env:
        monkeypatch.delenv(k, raising=False)
    out[0].knn_cache_mode = "fresh"
    return out


def hparam_row(g, rid):
    """One row of tests/golden/hparams.npz (`g`: the loaded file): kind 'fn' / 'fd', the constructor override, the oracle's `hp`
    dict, the patch sizes and the BatchNorm statistics the row carries."""
    from conftest import FD_KW, FN_KW
    kind = rid.split("-")[0]
    over = {}
    for n in g[rid + "/kw_names"]:
        v = g["%s/kw:%s" % (rid, n)]
        over[str(n)] = [int(x) for x in v] if str(n) in ("k_values", "k_scales") else int(v[0])
    kw = dict(FN_KW if kind == "fn" else FD_KW, **over)
    names = ("k_values", "emb_dims", "time_steps_enc", "num_heads") if kind == "fn" else ("k", "k_scales", "emb_dims", "time_steps_enc", "num_heads")
    bn = {str(n): g["%s/bn:%s" % (rid, n)] for n in g[rid + "/bn_names"]}
    return {"id": rid, "kind": kind, "over": over, "kw": kw, "hp": {n: kw[n] for n in names}, "sizes": [int(m) for m in g[rid + "/sizes"]], "bn": bn}


def hparam_model(row):
    """(module on the CPU, conditioned state dict) for a row of hparams.npz: seed-0 weights, the committed BatchNorm calibration
    wherever the row's shapes still match it, the row's own statistics on top (make_fixtures.py calibrate_bn_from)."""
    import sapcu_amd
    from conftest import golden
    from sapcu_amd import testing as T
    cls = sapcu_amd.ImprovedSNNNormalEstimation if row["kind"] == "fn" else sapcu_amd.EnhancedSNNDistanceEstimation
    model = cls(**row["kw"])
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    bn = {k: v for k, v in dict(golden("bn_calib_%s.npz" % row["kind"])).items() if shapes.get(k) == tuple(v.shape)}
    bn.update(row["bn"])
    sd = T.conditioned_state_dict(model.state_dict(), 0, bn_stats=bn)
    model.load_state_dict(sd, strict=True)
    return model, sd


def build_gpu_hparam_model(row, monkeypatch=None, env=None):
    """The device model of a row of hparams.npz, its handle created under the environment switches `env` (see
    build_gpu_models_under)."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    model, sd = hparam_model(row)
    model = model.to(dev())
    model._engine()
    for k in (env or {}):
        monkeypatch.delenv(k, raising=False)
    if row["kind"] == "fn":
        model.knn_cache_mode = "fresh"
    return model, sd


def sphere_patches(nq, k, n=5000, qseed=0, skip=0):
    from sapcu_amd import testing as T
    cloud = T.sphere_cloud(n, 0)
    q = T.grid_queries(nq + skip, qseed)[skip:]
    idx = G.knn_bruteforce(cloud, q, k)
    return torch.from_numpy(G.gather_centre(cloud, q, idx)).float()


def fd_forward_forced(fd_gpu, sdd, patch_cpu, hp=FD_HP):
    """Run the device fd, read back the feature-space neighbour tables it chose, evaluate the oracle on
    exactly those.  Returns (gpu_dist, oracle_dist_forced, oracle_dist_free, flip_rows[3], taps)."""
    b, m = patch_cpu.shape[0], patch_cpu.shape[1]
    kk = min(hp["k"], m)
    knn = torch.empty((3, b, m, kk), dtype=torch.int32, device=dev())
    d_gpu = fd_gpu(patch_cpu.to(dev()), taps={"knn": knn})
    torch.cuda.synchronize()
    knn_cpu = knn.cpu().long()
    taps_free = {}
    with torch.no_grad():
        d_forced = O.fd_forward(fd_state(sdd), patch_cpu, hp, force_idx=[knn_cpu[0], knn_cpu[1], knn_cpu[2]])
        d_free = O.fd_forward(fd_state(sdd), patch_cpu, hp, taps=taps_free)
    flips = []
    for i in (1, 2, 3):
        a = taps_free["encoder.knn%d" % i].sort(-1)[0]
        g = knn_cpu[i - 1].sort(-1)[0]
        flips.append((a != g).any(-1))           # [b, m] rows whose neighbour SET differs
    return d_gpu.cpu(), d_forced, d_free, flips, taps_free


def fd_state(sd):
    return sd
