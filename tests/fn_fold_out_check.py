"""Worker of tests/test_fn_fold_out.py: one fn forward on the golden fn inputs (tests/golden/fn_taps.npz) in a process of its own, so
that the handle is created under exactly the SAPCU_* switches of this process's environment (sapcu_model_create reads them once).
usage: python fn_fold_out_check.py <out.npz>   — writes the three block taps, the encoding, the logits, the normals and which
blocks ran the fused edge chain."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(out):
    import gpu_utils as U
    from conftest import FN_KW, golden
    import sapcu_amd
    from sapcu_amd import testing as T
    fn = sapcu_amd.ImprovedSNNNormalEstimation(**FN_KW)
    sdn = T.conditioned_state_dict(fn.state_dict(), 0, bn_stats=dict(golden("bn_calib_fn.npz")))
    fn.load_state_dict(sdn, strict=True)
    fn = fn.to(U.dev())
    fn.knn_cache_mode = "fresh"
    g = golden("fn_taps.npz")
    b, m = g["patch"].shape[:2]
    z = lambda *s: torch.empty(s, dtype=torch.float32, device=U.dev())
    taps = {"block1": z(b, m, 64), "block2": z(b, m, 64), "block3": z(b, m, 64), "enc": z(b, 2048), "logits": z(b, 3)}
    n = fn(torch.as_tensor(g["patch"], device=U.dev()), taps=taps)
    torch.cuda.synchronize()
    split, overflows = fn.gemm_mode()
    assert overflows == 0, overflows
    np.savez(out, normals=n.cpu().numpy(), fused_mask=np.int64(fn.fused_blocks(m)), split_f16=np.int64(split),
             **{k: v.cpu().numpy() for k, v in taps.items()})
    print("FN_FOLD_OUT_CHECK_OK", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
