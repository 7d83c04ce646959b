#!/usr/bin/env python3
"""Reader of the fused fn edge chain's diagnostic stamps (library built with EXTRA_CXXFLAGS=-DCHAIN_STAMPS, selected with
SAPCU_AB_LIB=<.so>): s_memtime at the phase boundaries of fn_edge_chain_kernel as thread 0 of a group passes them, median over the
groups of one launch per fn block shape, (d, kk) = (128, 24), (256, 18), (512, 12) at 4096 patches x 48 points, through the C-ABI
entry (so d = 512 runs plain groups of five, not the filled form).  The diagnostic build honours SAPCU_CHAIN_TRIM=0 per call:
    SAPCU_AB_LIB=profiles/ab/lib_stamps.so SAPCU_CHAIN_TRIM=0 python3 profiles/chain_stamps.py      (untrimmed epilogues)
    SAPCU_AB_LIB=profiles/ab/lib_stamps.so python3 profiles/chain_stamps.py                         (trimmed, the default)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sapcu_amd import _lib  # noqa: E402

if os.environ.get("SAPCU_AB_LIB"):
    _lib.LIB_PATH = os.environ["SAPCU_AB_LIB"]

PPG = {128: 4, 256: 7, 512: 5}                       # points per group
SPANS = [("phase 0: edge records", 0, 1), ("phase 0: fc_delta + neurons", 1, 2), ("(barrier)", 2, 3), ("GEMM 1", 3, 4),
         ("(barrier)", 4, 5), ("epilogue 1", 5, 6), ("(barrier)", 6, 7), ("GEMM 2", 7, 8), ("(barrier)", 8, 9), ("epilogue 2", 9, 10),
         ("(barrier)", 10, 11), ("GEMM 3", 11, 12), ("epilogue 3", 12, 15)]


def main():
    lib = _lib.load()
    dev = torch.device("cuda")
    B, M, heads, T = 4096, 48, 8, 4
    P = B * M
    print("lib %s, SAPCU_CHAIN_TRIM=%s; s_memtime ticks per group, median over the groups of one launch"
          % (os.environ.get("SAPCU_AB_LIB", "default"), os.environ.get("SAPCU_CHAIN_TRIM", "(unset)")))
    for d, kk in ((128, 24), (256, 18), (512, 12)):
        g = torch.Generator(device="cpu").manual_seed(0)
        patch = (torch.randn((B, M, 3), generator=g) * 0.05).to(dev)
        idx = torch.stack([torch.randperm(M, generator=g)[:kk] for _ in range(P)]).to(torch.int32).to(dev)
        qkv = torch.rand((P, 3 * d), generator=g).to(dev)

        def lin(n, k, gain):
            return ((torch.rand((n, k), generator=g) * 2 - 1) * gain / k ** 0.5).to(dev), (torch.randn(n, generator=g) * 0.4 + 0.6).to(dev)

        def lif():
            return torch.stack([torch.full((d,), 0.9), torch.full((d,), 0.01), torch.full((d,), 0.5), torch.ones(d)]).to(dev)

        wd, bd = lin(d, 3, 20.0)
        (w1, b1), (w2, b2), (w3, b3) = lin(d, d, 2.0), lin(d, d, 2.0), lin(d, d, 4.0)
        ops = [patch.view(P, 3), idx.view(-1), qkv, wd, bd, lif(), w1, b1, lif(), w2, b2, lif(), w3, b3]
        need = lib.sapcu_fn_edge_chain_workspace_bytes(P, d, kk)
        off = (need + 255) // 256 * 256                  # where the diagnostic build puts the stamps: behind what the entry needs
        sbytes = (P // 4 + 1) * 16 * 8
        ws = torch.zeros(off + sbytes + 512, dtype=torch.uint8, device=dev)
        res = torch.empty((P, d), device=dev)
        for _ in range(2):                                # the second launch is the one read
            _lib.check(lib.sapcu_fn_edge_chain_f32(_lib.ptr(ops[0]), _lib.ptr(ops[1]), P, M, d, kk, *[_lib.ptr(t) for t in ops[2:]],
                                                   heads, T, _lib.ptr(res), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
        torch.cuda.synchronize()
        base = (-ws.data_ptr()) % 256                     # the entry aligns the workspace to 256 bytes
        ngroups = (P + PPG[d] - 1) // PPG[d]
        s = ws[base + off: base + off + ngroups * 128].cpu().numpy().view(np.int64).reshape(ngroups, 16).astype(np.float64)
        if not s[:, 15].any():
            print("d = %d: no stamps (not a -DCHAIN_STAMPS build?)" % d)
            continue
        total = np.median(s[:, 15] - s[:, 0])
        print("d = %d, kk = %d: %d groups, total %.0f ticks per group, result sum %.6f" % (d, kk, ngroups, total, float(res.double().sum())))
        for name, i0, i1 in SPANS:
            v = np.median(s[:, i1] - s[:, i0])
            print("  %-30s %8.0f  (%4.1f %%)" % (name, v, 100 * v / total))
        print("  %-30s %8.0f   own points\n  %-30s %8.0f   points in spare slots" % ("  of epilogue 3:", np.median(s[:, 13]), "", np.median(s[:, 14])))


if __name__ == "__main__":
    main()
