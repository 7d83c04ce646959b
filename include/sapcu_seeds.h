/*
 * sapcu_seeds.h — seed generation on the device: the voxel flood of sapcu_dense_seeds_host (sapcu.h; the reference's
 * dense.cpp:175-252) with the seeds left in HBM.  Same seeds, same order, same 6-decimal values, bit for bit.
 *
 * Part of libsapcu_hip.so; the conventions and status codes of sapcu.h apply (device pointers unless named *_host, the caller owns
 * every buffer, 0 on success, sapcu_last_error() for the text).  SAPCU_ABI_VERSION is unchanged: these entry points are additions.
 *
 * How it runs (csrc/dense_seeds_dev.hip).  Level by level like the host flood: (1) every voxel of the frontier is evaluated by one
 * thread — the 11 nearest of the n+1 points (the cloud plus the reference's all-zero point) on the cell grid of csrc/knn_grid.hip,
 * squared distances ((0+dx^2)+dy^2)+dz^2 in separately rounded f64, then the 8 point-triangle tests in the host's operation order;
 * (2) the FIFO bookkeeping is reproduced in parallel: every candidate key (a point's voxel, later the 6 neighbours +x -x +y -y +z -z
 * of an expanding voxel) carries its position in the host's queue as a sequence number, a device open-addressing table keeps the
 * MINIMUM sequence number per key (integer atomicCAS / atomicMin only), a candidate enters the next frontier iff the table holds its
 * own number, and an order-preserving compaction (exclusive scan) appends the band voxels (0.011 <= distance <= 0.015) to the seeds
 * and builds the next frontier.  Voxel keys and their % and / decomposition are the host's `int` arithmetic.
 *
 * What still runs on the host, by design:
 *   - a voxel whose 10th and 11th nearest points are at exactly the same squared distance: which of them the host keeps depends on
 *     its k-d traversal, so that voxel's distance is recomputed by the host's own routine;
 *   - a voxel whose x index lies outside [-boxsize, 2*boxsize] (boxsize = round(1/cell)): the 6-decimal values ("%lf" -> strtod)
 *     are a table built on the host for that index range, and such a voxel is outside it.
 *   stats_host[2] counts both.  For this the cloud is copied to the host once at the start (n*24 bytes).
 *
 * Memory contract (as sapcu.h; checked under guard bands by tests/test_gpu_seeds.py):
 *   - cloud_dev [n,3] f64 is only read; seeds_out_dev [capacity,3] f64: rows [0, min(count, capacity)) are written, nothing else;
 *     nothing is written beyond the workspace_bytes a sizer call returned for the same (n, max_voxels);
 *   - the workspace needs NO initialisation (the key table, every counter and flag are initialised by the call on `stream`) and
 *     8-byte alignment (f64 tables inside);
 *   - refused before anything is launched or copied, with SAPCU_ERR_ARG: a NULL cloud_dev, count_host or workspace, a NULL
 *     seeds_out_dev with capacity > 0, n < 1 or n > 2^28, max_voxels < 1 or > 2^28, capacity < 0, cell <= 0 or NaN or
 *     round(1/cell) outside 1..1000, a workspace shorter than the sizer's bytes or not 8-byte aligned;
 *   - refused after the cloud was copied to the host, before any kernel: a non-finite coordinate, or a point whose voxel key
 *     floor((x+.5)/cell)*boxsize^2 + floor((y+.5)/cell)*boxsize + floor((z+.5)/cell) lies outside +-2e9 (the host converts that
 *     value to `int`) -> SAPCU_ERR_ARG;
 *   - SAPCU_ERR_WORKSPACE: more than max_voxels distinct voxels were met (the table is never overrun; detected on the device,
 *     reported at the next level; *count_host = seeds counted so far), or more than `capacity` seeds exist (all of them are
 *     counted, *count_host = the full count, only the first `capacity` are written).  Call again with more room;
 *   - `stream` is synchronised once for the cloud copy, once for the grid parameters, once per flood level and once for the empty
 *     frontier that ends the flood (the frontier size and the count of host-recomputed voxels come back together; a level with
 *     such voxels synchronises twice more).  The call returns with all its work complete.
 *
 * stats_host (HOST int64[4], may be NULL) = {flood levels, voxels evaluated, voxels recomputed on the host, table slots}.
 */
#ifndef SAPCU_SEEDS_H
#define SAPCU_SEEDS_H

#include "sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for a cloud of n points and at most max_voxels distinct voxels met by the flood (every voxel evaluated is
 * one; 1 755 588 for a 5000-point unit sphere at cell 0.004); -1 for arguments the flood would refuse. */
int64_t sapcu_dense_seeds_workspace_bytes(int64_t n, int64_t max_voxels);

int sapcu_dense_seeds_f64(const double* cloud_dev, int64_t n, double cell, double* seeds_out_dev, int64_t capacity,
                          int64_t max_voxels, int64_t* count_host, int64_t* stats_host, void* workspace,
                          int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_SEEDS_H */
