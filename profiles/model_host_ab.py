"""Launch lists of one fn and one fd forward, for comparing two builds of the library (profiles/model_host_ab.txt).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/model_host_ab.py run M
        the handles are created under whatever SAPCU_* switches the environment holds, the library is SAPCU_LIB_PATH's; one fn and
        one fd forward of 64 patches of M points
    python profiles/model_host_ab.py list DIR
        every dispatch of that trace in order — kernel name, grid, block — then the count and the sha1 of the list, and of the list
        without the HIP runtime's own copy / fill kernels (a hipMemcpy to pageable host memory uses one or not from run to run)

The list starts at model creation (the weight split and the packing kernels are dispatches too), so it covers the order of the
launches of sapcu_model_create as well as the two forwards.
"""
import csv
import glob
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(m):
    import numpy as np
    import torch
    import sapcu_amd
    import gpu_utils as U
    from sapcu_amd import testing as T
    gold = os.path.join(ROOT, "tests", "golden")
    fn = sapcu_amd.ImprovedSNNNormalEstimation(**U.FN_HP)
    fd = sapcu_amd.EnhancedSNNDistanceEstimation(**U.FD_HP)
    fn.load_state_dict(T.conditioned_state_dict(fn.state_dict(), 0, bn_stats=dict(np.load(os.path.join(gold, "bn_calib_fn.npz")))))
    fd.load_state_dict(T.conditioned_state_dict(fd.state_dict(), 0, bn_stats=dict(np.load(os.path.join(gold, "bn_calib_fd.npz")))))
    fn, fd = fn.to(U.dev()), fd.to(U.dev())
    fn.knn_cache_mode = "fresh"
    patch = U.sphere_patches(64, m).to(U.dev())
    n, d = fn(patch), fd(patch)
    torch.cuda.synchronize()
    print("fn %s fd %s fused blocks fn %d fd %d" % (tuple(n.shape), tuple(d.shape), fn.fused_blocks(m), fd.fused_blocks(m)))


def listing(d):
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    dims = lambda r, p: "x".join(r[k] for k in sorted(r) if k.startswith(p))
    lines = ["%s grid %s block %s" % (r["Kernel_Name"], dims(r, "Grid_Size"), dims(r, "Workgroup_Size")) for r in rows]
    print("\n".join(lines))
    own = [l for l in lines if not l.startswith("__amd_rocclr_")]        # without the HIP runtime's copy / fill kernels
    for tag, ls in (("dispatches", lines), ("library dispatches", own)):
        print("%s %d sha1 %s" % (tag, len(ls), hashlib.sha1("\n".join(ls).encode()).hexdigest()))


if __name__ == "__main__":
    run(int(sys.argv[2])) if sys.argv[1] == "run" else listing(sys.argv[2])
