/*
 * sapcu_metrics.h — the exact nearest neighbour of every query in ANOTHER cloud, on the device: the distance vectors behind Chamfer
 * distance, Hausdorff distance, precision / recall and F-score (sapcu_amd/metrics.py; the quantities the reference's
 * external/Meta-PU_evaluation/evaluation_code/evaluation_cd.py prints from two sklearn NearestNeighbors(n_neighbors=1) queries).
 *
 * Part of libsapcu_hip.so; the conventions and status codes of sapcu.h apply (device pointers unless named *_host, the caller owns
 * every buffer, 0 on success, sapcu_last_error() for the text).  SAPCU_ABI_VERSION is unchanged: these entry points are additions.
 *
 * Result.  dist_out[i] and idx_out[i] are bit for bit what sapcu_knn_gather_f64(cloud, n, queries, nq, 1, idx, dist, NULL) returns:
 * the squared distance is ((q-p)_x^2 + (q-p)_y^2) + (q-p)_z^2 in separately rounded f64 operations, the output the correctly rounded
 * square root of it, and among points at the minimal distance the lowest index wins.
 *
 * How it runs (csrc/metrics.hip).  The cell grid of csrc/knn_grid.hip is built over the cloud; the queries are counting-sorted by the
 * cell of that grid they fall in (clamped: a query may lie anywhere); one query per lane, all lanes of a wavefront in one cell,
 * Chebyshev shells around it until every lane's distance to the faces of the visited block, less a slack that covers the rounding
 * at the cloud's AND the queries' magnitude, is strictly above its best.  cell_size 0 = automatic; any value gives the same result.
 * The brute-force kernel runs instead, with info_host[0] = 0, for n < 4096 with the automatic cell size, and for a non-finite or
 * |x| > 1e150 coordinate in the cloud or in the queries.
 *
 * Memory contract (as sapcu.h; checked under guard bands by tests/test_gpu_metrics.py):
 *   - cloud [n,3] and queries [nq,3] f64 are only read; dist_out [nq] f64 and idx_out [nq] int64 (may be NULL) are written in full,
 *     nothing else; nothing is written beyond the workspace_bytes the sizer returned for the same (n, nq);
 *   - the workspace needs NO initialisation and 8-byte alignment (f64 tables inside);
 *   - nq == 0 launches nothing and writes nothing (queries and dist_out may then be NULL);
 *   - refused before anything is launched, with SAPCU_ERR_ARG: a NULL cloud, a NULL queries or dist_out with nq > 0, n < 1 or
 *     n > 2^29, nq < 0 or nq > 2^31 - 64, cell_size negative, NaN or >= 1e300, a NULL workspace, one shorter than the sizer's bytes
 *     or not 8-byte aligned;
 *   - `stream` is synchronised once (the grid parameters are read back), not at all on the n < 4096 route.
 *
 * info_host (HOST int64[4], may be NULL) = {1 if the grid ran else 0, gx, gy, gz}.
 */
#ifndef SAPCU_METRICS_H
#define SAPCU_METRICS_H

#include "sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for a cloud of n points and nq queries; -1 for sizes the search would refuse. */
int64_t sapcu_nn_cross_workspace_bytes(int64_t n, int64_t nq);

int sapcu_nn_cross_grid_f64(const double* cloud, int64_t n, const double* queries, int64_t nq, double cell_size,
                            double* dist_out, int64_t* idx_out, void* workspace, int64_t workspace_bytes,
                            int64_t* info_host, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_METRICS_H */
