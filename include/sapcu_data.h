/*
 * sapcu_data.h — the self-supervised training samples of fd and fn built on the device from raw cloud pairs: what the reference's
 * fd/datacore.py PU1KDataset.__getitem__ (:91-149) and fn/datacore.py PU1KMeshDataset.__getitem__ (:201-258, after the mesh has been
 * sampled) compute per sample on DataLoader workers with two scipy cKDTree builds (sapcu_amd/data.py is the Python layer).
 *
 * Part of libsapcu_hip.so; the conventions and status codes of sapcu.h apply (device pointers, the caller owns every buffer, 0 on
 * success, sapcu_last_error() for the text).  SAPCU_ABI_VERSION is unchanged: these entry points are additions.
 *
 * Semantics, per batch entry i (sample s = sample_idx[i]); every operation is one separately rounded f32 operation unless f64 is named:
 *   1. augmentation (each part only when its pointer is given): p = ((x r00 + y r01) + z r02, (x r10 + y r11) + z r12, (x r20 + y r21)
 *      + z r22) with r = rot[i] row-major, on cloud, dense and normals; p *= scale[i] on cloud and dense; p += jitter[i] on the cloud;
 *   2. centroid = the sum of the cloud's rows in index order (row 0, + row 1, ...) / (float)n, subtracted from cloud and dense;
 *   3. radius = max sqrtf((x^2 + y^2) + z^2) over the cloud; cloud and dense are divided by it only if it is > 0;
 *   4. normals_out = nrm / (sqrtf((x^2 + y^2) + z^2) + 1e-8f);
 *   5. len_out[j] = (float) sqrt(min over the dense points of ((dx^2 + dy^2) + dz^2)) with dx = (double)c - (double)d: separately
 *      rounded f64 operations on the f32 coordinates, the correctly rounded f64 square root (the convention of sapcu_metrics.h);
 *   6. idx_out[c] = the k cloud points nearest to cloud_out[centres[c]] in (that f64 squared distance, index) ascending order — the
 *      point itself included, and among equal distances the lower index first; patches_out[c] = cloud_out's rows at those indices;
 *   7. patch_normals_out[c] = normals_out's row centres[c].
 * Coordinates are expected to be finite (a NaN or infinity gives unspecified values, never an access outside a buffer).
 *
 * Memory contract (as sapcu.h; checked under guard bands by tests/test_gpu_data.py):
 *   - clouds [S,n,3], dense [S,g,3], normals [S,n,3], sample_idx [b] int64, rot [b,9], scale [b], jitter [b,n,3], centres [b,pc]
 *     int32 are only read; every output that is passed is written in full — patches_out [b,pc,k,3], idx_out [b,pc,k] int32,
 *     cloud_out [b,n,3], dense_out [b,g,3], len_out [b,n], normals_out [b,n,3], patch_normals_out [b,pc,3] — and nothing else;
 *   - the workspace (the centroid and radius of every batch entry) needs NO initialisation and 4-byte alignment;
 *   - b == 0 launches nothing and writes nothing;
 *   - refused before anything is launched, with SAPCU_ERR_ARG: n outside 1..4096; g outside 0..65536; k outside 1..min(n,128);
 *     pc < 1 or pc > 2^20; centres == NULL with pc != n; n_samples < 1; b < 0 or b > 2^20; a NULL clouds, sample_idx, patches_out or
 *     cloud_out with b > 0; dense given with g == 0 or g > 0 without dense; dense_out or len_out without dense; normals_out or
 *     patch_normals_out without normals; a NULL, short or misaligned workspace with b > 0;
 *   - INDEX VALUES are validated by the caller (sapcu_amd.data.build_patches does it and raises ValueError): the entry point does
 *     not read device memory on the host and never synchronises `stream`, so it can be captured into a graph.  It stays memory-safe
 *     on bad values: a batch entry whose sample index is outside [0,S) is skipped whole (none of its output rows is written), a
 *     centre outside [0,n) skips that centre's rows of patches_out / idx_out / patch_normals_out.
 */
#ifndef SAPCU_DATA_H
#define SAPCU_DATA_H

#include "sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for a batch of b entries; -1 for a b the call would refuse. */
int64_t sapcu_train_patches_workspace_bytes(int64_t b);

int sapcu_train_patches_f32(
    const float* clouds, int64_t n_samples, int n,   /* data set [S,n,3] */
    const float* dense, int g,                       /* [S,g,3], or NULL with g = 0 */
    const float* normals,                            /* [S,n,3] or NULL */
    const int64_t* sample_idx, int64_t b,            /* the b samples of this batch (repeats allowed) */
    const float* rot,                                /* [b,9] row-major or NULL */
    const float* scale,                              /* [b] or NULL */
    const float* jitter,                             /* [b,n,3] or NULL: added to the cloud only */
    const int32_t* centres, int pc,                  /* [b,pc] indices into the cloud; NULL = all n points in order (pc = n) */
    int k,
    float* patches_out,                              /* [b,pc,k,3] */
    int32_t* idx_out,                                /* [b,pc,k] or NULL */
    float* cloud_out,                                /* [b,n,3] */
    float* dense_out,                                /* [b,g,3] or NULL */
    float* len_out,                                  /* [b,n] or NULL; both need dense */
    float* normals_out,                              /* [b,n,3] or NULL; needs normals */
    float* patch_normals_out,                        /* [b,pc,3] or NULL; needs normals */
    void* workspace, int64_t workspace_bytes,
    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_DATA_H */
