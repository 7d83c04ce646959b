"""ctypes binding of ``csrc/libsapcu_hip.so`` (the C ABI declared in ``include/sapcu.h``).

There is no CPU fallback: if the shared library is missing or fails to load, every product
entry point raises ``SapcuLibraryError`` — build it with ``python -c "import __graft_entry__ as g;
g.build()"`` or ``make -C <package>/csrc``.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# SAPCU_LIB_PATH: another build of the same library (e.g. csrc/libsapcu_hip_exact.so, `make -C csrc exact`: every neuron update in
# the reference's operation order); read once, at import
LIB_PATH = os.environ.get("SAPCU_LIB_PATH") or os.path.join(_HERE, "csrc", "libsapcu_hip.so")
EXACT_LIB_PATH = os.path.join(_HERE, "csrc", "libsapcu_hip_exact.so")

FN_TAPS = ("stem", "block1", "block2", "block3", "pooled", "enc", "logits")
FD_TAPS = ("fused0", "spikes", "knn", "pooled", "enc", "x0")
KIND_FN, KIND_FD = 0, 1
ABI_VERSION = 2        # include/sapcu.h SAPCU_ABI_VERSION this binding was written against (2: six fd taps)


class SapcuLibraryError(RuntimeError):
    """The HIP library is absent or unloadable (never silently replaced by a CPU path)."""


class SapcuError(RuntimeError):
    """A C entry point returned a non-zero status: args = (code, text)."""


# header under include/ -> {entry point: (restype, argtypes)}, in the order the headers were added; None: the test hooks in no header.
# load() binds every table, and tests/abi_tables.py holds each against its header: a new header is one entry here
TABLES = {}
TABLES["sapcu.h"] = {
    "sapcu_abi_version": (c_int, []),
    "sapcu_last_error": (c_char_p, []),
    "sapcu_knn_gather_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sapcu_gather_rotate_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "sapcu_displace_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "sapcu_knn_grid_workspace_bytes": (c_int64, [c_int64]),
    "sapcu_knn_self_grid_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_double, c_void_p, c_void_p, c_void_p, c_int64,
                                        POINTER(c_int64), c_void_p]),
    "sapcu_outlier_stats_f64": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    "sapcu_outlier_keep_f64": (c_int, [c_void_p, c_int64, c_double, c_double, c_void_p, c_void_p]),
    "sapcu_fps_workspace_bytes": (c_int64, [c_int64]),
    "sapcu_fps_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "sapcu_dense_seeds_host": (c_int, [c_void_p, c_int64, c_double, c_void_p, c_int64, POINTER(c_int64)]),
    "sapcu_lif_train_forward": (c_int, [c_void_p, c_int64, c_int, c_int] + [c_void_p] * 4 + [c_void_p, c_void_p]),
    "sapcu_lif_train_workspace_bytes": (c_int64, [c_int64, c_int]),
    "sapcu_lif_train_backward": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int] + [c_void_p] * 4 + [c_void_p] * 5 +
                                 [c_void_p, c_int64, c_void_p]),
    "sapcu_train_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "sapcu_bn_train_forward": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_float] + [c_void_p] * 4 + [c_void_p, c_int64, c_void_p]),
    "sapcu_bn_train_backward": (c_int, [c_void_p, c_void_p, c_int64, c_int] + [c_void_p] * 3 + [c_void_p] * 3 + [c_void_p, c_int64, c_void_p]),
    "sapcu_conv1x1_wgrad_f32": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "sapcu_gemm_bf16": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "sapcu_wgrad_bf16_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "sapcu_conv1x1_wgrad_bf16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "sapcu_softmax_agg_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "sapcu_softmax_agg_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float,
                                          c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "sapcu_gather_rows": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "sapcu_scatter_add_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int, c_int64, c_void_p]),
    "sapcu_scatter_add_rows_grouped": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "sapcu_group_max_forward": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "sapcu_group_max_backward": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "sapcu_neuron_selfloop": (c_int, [c_void_p, c_int64, c_int, c_int] + [c_void_p] * 6 + [c_void_p] * 4 + [c_void_p]),
    "sapcu_neuron_drive": (c_int, [c_void_p, c_int64, c_int, c_int] + [c_void_p] * 6 + [c_int] + [c_void_p] * 5 + [c_void_p]),
    "sapcu_patch_knn": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "sapcu_model_create": (c_int, [c_int, POINTER(c_int32), c_int, c_void_p, c_int64, POINTER(c_int64), c_int,
                                   POINTER(c_void_p)]),
    "sapcu_model_destroy": (c_int, [c_void_p]),
    "sapcu_workspace_bytes": (c_int64, [c_void_p, c_int64, c_int]),
    "sapcu_model_gate_violations": (c_int, [c_void_p, POINTER(c_int)]),
    "sapcu_l2_normalize3": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "sapcu_fn_forward": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                 POINTER(c_void_p), c_void_p]),
    "sapcu_fd_forward": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int64,
                                 POINTER(c_void_p), c_void_p]),
    "sapcu_gemm_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                               c_int, c_void_p, c_int, c_int, c_void_p]),
    "sapcu_to_split_rows": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_void_p]),
    "sapcu_posenc_gemm_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                      c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "sapcu_model_gemm_mode": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "sapcu_model_fused_blocks": (c_int, [c_void_p, c_int, POINTER(c_int)]),
    "sapcu_fn_edge_chain_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "sapcu_fn_edge_chain_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int] + [c_void_p] * 12 + [c_int, c_int, c_void_p, c_void_p,
                                        c_int64, c_void_p]),
}

EXPORTS = tuple(TABLES["sapcu.h"])

# include/sapcu_seeds.h: the device seed flood (additions to the same library; EXPORTS stays "what sapcu.h declares")
TABLES["sapcu_seeds.h"] = {
    "sapcu_dense_seeds_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "sapcu_dense_seeds_f64": (c_int, [c_void_p, c_int64, c_double, c_void_p, c_int64, c_int64, POINTER(c_int64), POINTER(c_int64),
                              c_void_p, c_int64, c_void_p]),
}
SEEDS_EXPORTS = tuple(TABLES["sapcu_seeds.h"])

# include/sapcu_fd_train.h: the training ops of fd (additions to the same library, a third table like SEEDS_EXPORTS)
TABLES["sapcu_fd_train.h"] = {
    "sapcu_fd_neuron_step_forward": (c_int, [c_void_p, c_int64, c_int, c_int] + [c_void_p] * 6 + [c_void_p] * 3 + [c_void_p] + [c_void_p] * 5 +
                                     [c_void_p]),
    "sapcu_fd_neuron_step_workspace_bytes": (c_int64, [c_int64, c_int]),
    "sapcu_fd_neuron_step_backward": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int] + [c_void_p] * 4 + [c_void_p] * 3 + [c_void_p] * 5 +
                                      [c_void_p, c_int64, c_void_p]),
    "sapcu_fd_edge_feature_forward": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "sapcu_fd_edge_feature_backward": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "sapcu_fd_bn_stats_workspace_bytes": (c_int64, [c_int64, c_int]),
    "sapcu_fd_bn_stats": (c_int, [c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "sapcu_fd_bn_lrelu_max_forward": (c_int, [c_void_p, c_int64, c_int, c_int] + [c_void_p] * 4 + [c_void_p, c_void_p, c_void_p]),
    "sapcu_fd_bn_lrelu_max_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int] + [c_void_p] * 4 + [c_void_p, c_void_p]),
}
FD_TRAIN_EXPORTS = tuple(TABLES["sapcu_fd_train.h"])

# include/sapcu_fd_edgeconv.h: the factored EdgeConv training op of fd's blocks 1-3 (a fourth table)
TABLES["sapcu_fd_edgeconv.h"] = {
    "sapcu_fd_edgeconv_stats_workspace_bytes": (c_int64, [c_int64, c_int, c_int, c_int]),
    "sapcu_fd_edgeconv_stats": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float] + [c_void_p] * 4 + [c_void_p, c_int64, c_void_p]),
    "sapcu_fd_edgeconv_max_forward": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int] + [c_void_p] * 4 + [c_void_p, c_void_p, c_void_p]),
    "sapcu_fd_edgeconv_backward_workspace_bytes": (c_int64, [c_int64, c_int, c_int, c_int]),
    "sapcu_fd_edgeconv_backward": (c_int, [c_void_p] * 4 + [c_int64, c_int, c_int, c_int] + [c_void_p] * 4 + [c_void_p] * 4 +
                                   [c_void_p, c_int64, c_void_p]),
}
FD_EDGECONV_EXPORTS = tuple(TABLES["sapcu_fd_edgeconv.h"])

# include/sapcu_train_step.h: the device-side skip of a graphed training step (a fifth table); flag, dst, src and nbytes are DEVICE arrays
TABLES["sapcu_train_step.h"] = {
    "sapcu_multi_select": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
}
TRAIN_STEP_EXPORTS = tuple(TABLES["sapcu_train_step.h"])

# include/sapcu_metrics.h: the nearest neighbour of every query in another cloud on the device cell grid (a sixth table)
TABLES["sapcu_metrics.h"] = {
    "sapcu_nn_cross_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "sapcu_nn_cross_grid_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_int64,
                                        POINTER(c_int64), c_void_p]),
}
METRICS_EXPORTS = tuple(TABLES["sapcu_metrics.h"])

# include/sapcu_data.h: fd's and fn's training samples from raw cloud pairs (a seventh table)
TABLES["sapcu_data.h"] = {
    "sapcu_train_patches_workspace_bytes": (c_int64, [c_int64]),
    "sapcu_train_patches_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_int, c_int] + [c_void_p] * 7 + [c_void_p, c_int64, c_void_p]),
}
DATA_EXPORTS = tuple(TABLES["sapcu_data.h"])

# include/sapcu_mesh.h: the distance from every query to a triangle mesh, nearest face and closest point (an eighth table)
TABLES["sapcu_mesh.h"] = {
    "sapcu_point_mesh_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "sapcu_point_mesh_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_double, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_int64, POINTER(c_int64), c_void_p]),
}
MESH_EXPORTS = tuple(TABLES["sapcu_mesh.h"])

# include/sapcu_surface.h: area-weighted sampling of triangle meshes, fn's training clouds from .off files (a ninth table)
TABLES["sapcu_surface.h"] = {
    "sapcu_surface_tables_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "sapcu_surface_tables_f32": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64] + [c_void_p] * 4 +
                                 [c_void_p, c_int64, c_void_p]),
    "sapcu_surface_sample_f32": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                         c_void_p, c_int64, c_int] + [c_void_p] * 3 + [c_void_p] * 3 + [c_void_p]),
}
SURFACE_EXPORTS = tuple(TABLES["sapcu_surface.h"])

# include/sapcu_sinkhorn.h: entropic optimal transport between two clouds without the cost matrix (a tenth table)
TABLES["sapcu_sinkhorn.h"] = {
    "sapcu_sinkhorn_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "sapcu_softmin_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_double, c_void_p, c_void_p, c_int64, c_void_p]),
    "sapcu_sinkhorn_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, POINTER(c_double), c_int64, c_double, c_int64, c_void_p,
                                   c_void_p, c_void_p, c_int64, c_void_p]),
    "sapcu_plan_stats_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p,
                                     c_void_p, c_int64, c_void_p]),
}
SINKHORN_EXPORTS = tuple(TABLES["sapcu_sinkhorn.h"])

# include/sapcu_ray.h: where every ray first meets a triangle mesh, and the fused step of fd's ray sampler (an eleventh table)
TABLES["sapcu_ray.h"] = {
    "sapcu_ray_mesh_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "sapcu_ray_mesh_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_int64, POINTER(c_int64), c_void_p]),
    "sapcu_ray_fd_samples_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "sapcu_ray_fd_samples_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double] +
                                 [c_void_p] * 4 + [c_void_p, c_int64, POINTER(c_int64), c_void_p]),
}
RAY_EXPORTS = tuple(TABLES["sapcu_ray.h"])

# include/sapcu_normals.h: PCA normals from a neighbour table and the angle between two tables of normals (a twelfth table);
# viewpoint_host is a HOST double[3] or None
TABLES["sapcu_normals.h"] = {
    "sapcu_pca_normals_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, POINTER(c_double), c_void_p, c_void_p, c_void_p, c_void_p]),
    "sapcu_normal_angles_f64": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_double, c_void_p, c_void_p, c_void_p]),
}
NORMALS_EXPORTS = tuple(TABLES["sapcu_normals.h"])

# test hooks in no header (host pointers, no device work): the f64 fold of an fn block's out_proj and fc2 that sapcu_model_create runs
TABLES[None] = _INTERNAL_SIGNATURES = {
    "sapcu_internal_fold_affine_host": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    # sapcu_point_mesh_f64 with the oversize cap (in cell edges) and the cell population given, or forced to the brute-force route: profiles/mesh_dist.py, tests/test_gpu_mesh.py
    "sapcu_internal_point_mesh_tuned": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_double, c_double, c_int, c_int, c_void_p,
                                                c_void_p, c_void_p, c_void_p, c_int64, POINTER(c_int64), c_void_p]),
    # csrc/sinkhorn.hip: {tile, shortest planned chunk, chunks, columns per chunk} of rows x columns (host only), and sapcu_softmin_f64
    # with the number of column chunks forced (chunks without a column): sapcu_amd/sinkhorn.py, tests/test_gpu_sinkhorn.py
    "sapcu_internal_sinkhorn_split": (c_int, [c_int64, c_int64, POINTER(c_int64)]),
    "sapcu_internal_softmin_split_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_double, c_int, c_void_p, c_void_p,
                                                 c_int64, c_void_p]),
    # sapcu_ray_mesh_f64 with the oversize cap and the piece length (in cell edges) and the cell population given, or forced to the
    # brute-force route: profiles/ray_cast.py, tests/test_gpu_ray.py
    "sapcu_internal_ray_mesh_tuned": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double,
                                              c_int, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, POINTER(c_int64),
                                              c_void_p]),
    # sapcu_geodesic_disks_f64 (csrc/sapcu_geodesic.h) with a smaller window cap and a shorter workspace queue: tests/test_gpu_uniformity.py
    "sapcu_internal_geodesic_disks_limited": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                                      c_int64, POINTER(c_double), c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                                      c_void_p, c_int64, POINTER(c_int64), c_void_p]),
    # sapcu_poisson_select_f32 (csrc/sapcu_poisson.h) on the grid path at any C, one round per chunk: tests/test_gpu_poisson.py
    "sapcu_internal_poisson_select_grid": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                                   c_void_p]),
}
# csrc/sapcu_geodesic.h: geodesic disks on a mesh, the counts behind the uniformity figure (sapcu_amd/uniformity.py).  radii_host is a
# HOST double[nr], info_host a HOST int64[8].  Bound by load() like a table; kept beside TABLES because tests/abi_tables.py holds
# the list of TABLES' headers and of include/ closed (moving the header there is one entry in that list)
GEODESIC_SIGNATURES = {
    "sapcu_geodesic_disks_workspace_bytes": (c_int64, [c_int64] * 5),
    "sapcu_geodesic_disks_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                         POINTER(c_double), c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, POINTER(c_int64),
                                         c_void_p]),
}
GEODESIC_EXPORTS = tuple(GEODESIC_SIGNATURES)
# csrc/sapcu_poisson.h: Poisson-disk selection and the exact-count subsample of a cloud (sapcu_amd/poisson.py); every pointer is a
# DEVICE array.  Beside TABLES for the reason GEODESIC_SIGNATURES is
POISSON_SIGNATURES = {
    "sapcu_poisson_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "sapcu_poisson_select_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "sapcu_poisson_subsample_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_int64, c_void_p]),
}
POISSON_EXPORTS = tuple(POISSON_SIGNATURES)
# csrc/sapcu_pointing.h: fn's seed-centred samples, the band of candidates off a surface cloud with their pointing directions
# (sapcu_amd/pointing.py); info_host is a HOST int64[4], every other pointer a DEVICE array.  Beside TABLES for the same reason
POINTING_SIGNATURES = {
    "sapcu_pointing_workspace_bytes": (c_int64, [c_int64, c_int64, c_int, c_int]),
    "sapcu_pointing_samples_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_double, c_double, c_int, c_int, c_double, c_double,
                                           c_void_p, c_int, c_double, c_double, c_double, c_int64] + [c_void_p] * 7 +
                                   [c_void_p, c_int64, POINTER(c_int64), c_void_p]),
}
POINTING_EXPORTS = tuple(POINTING_SIGNATURES)
_lib = None


def load(path=None):
    """Load (once) and return the ctypes library; raises SapcuLibraryError when unavailable."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise SapcuLibraryError(
            "HIP library not built: %s is missing. Run `make -C %s` (needs hipcc, gfx950). "
            "There is no CPU fallback." % (p, os.path.dirname(p)))
    try:
        lib = ctypes.CDLL(p)
    except OSError as e:  # missing ROCm runtime etc.
        raise SapcuLibraryError("cannot load %s: %s" % (p, e)) from e
    for name, (res, args) in ((name, sig) for table in list(TABLES.values()) + [GEODESIC_SIGNATURES, POISSON_SIGNATURES, POINTING_SIGNATURES] for name, sig in table.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise SapcuLibraryError("%s does not export %s" % (p, name)) from e
        fn.restype = res
        fn.argtypes = args
    if lib.sapcu_abi_version() != ABI_VERSION:
        raise SapcuLibraryError("ABI version mismatch: library %d, binding %d" % (lib.sapcu_abi_version(), ABI_VERSION))
    if path is None:
        _lib = lib
    return lib


def check(rc):
    if rc != 0:
        text = load().sapcu_last_error()
        raise SapcuError(int(rc), text.decode("utf-8", "replace") if text else "")


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else c_void_p(t.data_ptr())


def current_stream():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(sizer, sizes, dev, refusal):
    """(workspace, nbytes) for one call: what the sizer ``sizer`` returns for the integer arguments ``sizes``, as a zeroed uint8
    tensor on ``dev``.  A negative size is the sizer's refusal: ``ValueError(refusal)``."""
    import torch
    nbytes = int(getattr(load(), sizer)(*sizes))
    if nbytes < 0:
        raise ValueError(refusal)
    return torch.zeros((nbytes,), dtype=torch.uint8, device=dev), nbytes


def call(name, dev, *args):
    """Run the entry point ``name`` on the current stream of ``dev``: a tensor argument goes in as its device pointer, None, numbers
    and ctypes values as they are, the stream is appended as the last argument, and a non-zero status raises ``SapcuError``."""
    import torch
    fn, tensor = getattr(load(), name), torch.Tensor
    with torch.cuda.device(dev):
        check(fn(*[c_void_p(a.data_ptr()) if isinstance(a, tensor) else a for a in args], current_stream()))
