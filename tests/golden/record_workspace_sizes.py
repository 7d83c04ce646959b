#!/usr/bin/env python3
"""Record what every workspace sizer of the C ABI returns -> workspace_sizes.json (tests/test_workspace_sizes.py compares).

    python tests/golden/record_workspace_sizes.py

Public ABI only, so the same file runs on any earlier commit: the recorded numbers are the sizers' values at the commit BEFORE sizer
and carving became one layout function per workspace (the four sizers of the grid searches: at the commit before their query
tables became one layout, csrc/knn_grid.h), and they are not to be re-recorded because a layout changed by accident.  Two
sections:

  "sizers"   the handle-free *_workspace_bytes functions over a grid of small and awkward arguments (the library loads without a GPU)
  "handles"  sapcu_workspace_bytes of fn / fd handles created under each environment switch and at three rows of hparams.npz, at
             b x m_pts = HANDLE_B x HANDLE_M.  The sizer launches and allocates nothing, so the large b are free; at m_pts = 100 and
             under the 64 MB budget the value depends on the chunk size, which is what pins it.

Without a GPU only "sizers" is recorded and the "handles" section of the existing file is kept.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "workspace_sizes.json")

# rows: 0, 1, around 256 (column-reduction and bf16 column-sum slabs), one past 64 (lif rows per workgroup), 512 (bf16 weight-gradient
# slab), 1024 (f32 weight-gradient slab) and 64 * 1024 (where the f32 slab count stops growing)
ROWS = (0, 1, 65, 255, 256, 257, 513, 1025, 65537)
CH_K = ((1, 0), (3, 1), (64, 64), (128, 0), (257, 96))
CHAIN_POINTS = (0, 1, 255, 256, 257, 4800)
CHAIN_DKK = ((128, 24), (256, 18), (512, 12), (128, 12))          # the last one is refused
NS = (1, 300, 4096, 385582)

ENVS = ({}, {"SAPCU_CHAIN": "0"}, {"SAPCU_FN_MAXFUSE": "0"}, {"SAPCU_FD_FUSED": "0"}, {"SAPCU_FD_X0": "0"}, {"SAPCU_FD_MAXFUSE": "0"},
        {"SAPCU_FD_SPLIT": "0"}, {"SAPCU_GEMM": "f32"}, {"SAPCU_CHUNK": "7"}, {"SAPCU_WS_BUDGET_MB": "64"})
HPARAM_ROWS = ("fn-ctor", "fd-ctor", "fd-s5")
HANDLE_B = (0, 1, 7, 64, 4096, 5000)
HANDLE_M = (1, 5, 12, 20, 48, 49, 100, 128)


def env_id(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


def record_sizers(lib):
    """{function: [[args..., value], ...]}"""
    out = {}
    out["sapcu_fn_edge_chain_workspace_bytes"] = [[p, d, kk, int(lib.sapcu_fn_edge_chain_workspace_bytes(p, d, kk))]
                                                  for p in CHAIN_POINTS for d, kk in CHAIN_DKK]
    out["sapcu_train_workspace_bytes"] = [[r, c, k, int(lib.sapcu_train_workspace_bytes(r, c, k))] for r in ROWS for c, k in CH_K]
    out["sapcu_wgrad_bf16_workspace_bytes"] = [[r, c, k, int(lib.sapcu_wgrad_bf16_workspace_bytes(r, c, k))] for r in ROWS for c, k in CH_K]
    out["sapcu_lif_train_workspace_bytes"] = [[r, c, int(lib.sapcu_lif_train_workspace_bytes(r, c))] for r in ROWS for c, _ in CH_K]
    out["sapcu_knn_grid_workspace_bytes"] = [[n, int(lib.sapcu_knn_grid_workspace_bytes(n))] for n in NS]
    out["sapcu_dense_seeds_workspace_bytes"] = [[n, v, int(lib.sapcu_dense_seeds_workspace_bytes(n, v))] for n in NS for v in NS]
    out["sapcu_fps_workspace_bytes"] = [[n, int(lib.sapcu_fps_workspace_bytes(n))] for n in NS]
    # the searches on the cell grid: every count over NS, and one refused argument each (-1)
    out["sapcu_nn_cross_workspace_bytes"] = [[n, q, int(lib.sapcu_nn_cross_workspace_bytes(n, q))] for n in NS for q in NS] + \
        [[0, 1, int(lib.sapcu_nn_cross_workspace_bytes(0, 1))]]
    for name in ("sapcu_point_mesh_workspace_bytes", "sapcu_ray_mesh_workspace_bytes", "sapcu_ray_fd_samples_workspace_bytes"):
        fn = getattr(lib, name)
        out[name] = [[v, f, q, int(fn(v, f, q))] for v in NS for f in NS for q in NS] + [[1, 0, 1, int(fn(1, 0, 1))]]
    return out


def record_handle(lib, model):
    """[[b, m_pts, bytes], ...] of a device model's handle"""
    h = model._engine()
    return [[b, m, int(lib.sapcu_workspace_bytes(h, b, m))] for b in HANDLE_B for m in HANDLE_M]


def _default_models(env):
    """fn and fd at the default hyper-parameters, handles created under `env` (tests/gpu_utils.py build_gpu_models_under)"""
    import numpy as np
    import sapcu_amd
    import torch
    from conftest import FD_KW, FN_KW
    from sapcu_amd import testing as T
    out = []
    os.environ.update(env)
    try:
        for kind, cls, kw in (("fn", sapcu_amd.ImprovedSNNNormalEstimation, FN_KW), ("fd", sapcu_amd.EnhancedSNNDistanceEstimation, FD_KW)):
            m = cls(**kw)
            bn = dict(np.load(os.path.join(HERE, "bn_calib_%s.npz" % kind)))
            m.load_state_dict(T.conditioned_state_dict(m.state_dict(), 0, bn_stats=bn), strict=True)
            m = m.to(torch.device("cuda:0"))
            m._engine()
            out.append(m)
    finally:
        for k in env:
            os.environ.pop(k, None)
    return out


def record_handles(lib):
    import numpy as np
    import gpu_utils as U
    out = {}
    for env in ENVS:
        fn, fd = _default_models(env)
        out[env_id(env)] = {"fn": record_handle(lib, fn), "fd": record_handle(lib, fd)}
    g = np.load(os.path.join(HERE, "hparams.npz"))
    for rid in HPARAM_ROWS:
        model, _ = U.build_gpu_hparam_model(U.hparam_row(g, rid))
        out[rid] = {rid.split("-")[0]: record_handle(lib, model)}
    return out


def main():
    import torch
    from sapcu_amd import _lib
    lib = _lib.load()
    data = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            data = json.load(f)
    data["sizers"] = record_sizers(lib)
    if torch.cuda.is_available():
        data["handles"] = record_handles(lib)
    else:
        print("no GPU: 'handles' section %s" % ("kept as recorded" if "handles" in data else "NOT recorded"))
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": {\n' % sec + ",\n".join('  "%s": %s' % (k, json.dumps(v, separators=(",", ":")))
                                                                   for k, v in data[sec].items()) + "\n }" for sec in data) + "\n}\n")
    print("wrote %s: %s" % (OUT, {sec: len(data[sec]) for sec in data}))


if __name__ == "__main__":
    main()
