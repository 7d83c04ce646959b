/*
 * sapcu_pointing.h — seed-centred training samples of fn: query points in a band off a surface cloud, each with the unit vector
 * from the query towards the mean of its k nearest surface points (sapcu_amd/pointing.py; the reference's
 * scripts/sample_mesh-fn.py export_pointing, which writes them as fn.npz).  csrc/pointing.hip; tests/pointing_ref.py states the
 * definition in numpy.
 *
 * Part of libsapcu_hip.so; the conventions and status codes of include/sapcu.h apply (device pointers unless named *_host, the
 * caller owns every buffer, 0 on success, sapcu_last_error() for the text).  SAPCU_ABI_VERSION is unchanged: these entry points are
 * additions.  The header lies beside its source, and its table in sapcu_amd/_lib.py beside TABLES, as csrc/sapcu_geodesic.h does
 * and for its reason.
 *
 * Definition.  f64 unless said, every operation rounded once (the library is built with -ffp-contract=off).  surface is P f32
 * [n,3]; a distance is taken to the point widened to f64, its square is ((q-p)_x^2 + (q-p)_y^2) + (q-p)_z^2 and its root is
 * correctly rounded, as in sapcu_knn_gather_f64.
 *   voxels[t], t = 0 .. nv-1: v = (ix*count + iy)*count + iz; corner c1 = i*step + origin per axis.
 *   candidate i = t*sub^3 + j, j = (jx*sub + jy)*sub + jz:  q = ((c1 + jc*step2) + half2) + jitter[i] per axis (jitter NULL: no
 *     addition); step2 and half2 are the caller's (step / sub and step2 / 2 as the caller's language evaluates them).
 *   neighbours: the k nearest points of P in ascending (distance, index); a point whose squared distance is NaN or +inf is no
 *     candidate (the rule of sapcu_knn_gather_f64); behind fewer than k of them the entries are empty: index -1.
 *   d1 = the first distance, +inf when there is none.
 *   keep[i]  <=>  all k entries exist and band_lo <= d1 <= band_hi (both ends inclusive).
 *   For a kept candidate: s = the f32 sum of the k neighbours' rows of P in list order from neighbour 0, mean = s / f32(k) (an f32
 *     division), w = f64(mean) - q, len = sqrt((w_x^2 + w_y^2) + w_z^2), pointing = w / len per component (IEEE division; a zero
 *     len gives NaN, and the row stays).
 *   Compacted outputs, kept candidates in ascending i: points = q, pointing, candidate = candidate0 + i; *count_out = their number.
 *
 * How it runs.  P is widened into the workspace and sorted into the cell grid of csrc/knn_grid.h.  One candidate per thread
 * (consecutive candidates are neighbours in space, so the lanes of a wavefront walk nearly the same cells): the running k-list
 * lives in registers, one kernel instance per k with every index a compile-time constant; the walk is grid_shell_walk with a
 * per-thread stop against the k-th squared distance, the margin GridParams.slack + 1e-11 * (the query's largest |coordinate|);
 * the band test and the pointing run in the same kernel.  When neither d1_out nor idx_out is asked for, a candidate whose every
 * unvisited point is provably beyond band_hi, and whose nearest visited one is too, leaves the walk early: its keep byte is 0
 * either way.  Compaction is flag, exclusive scan (launch_exclusive_scan_int), scatter: no floating-point atomics, the order is
 * the candidates'.  A query with a coordinate that is not finite or beyond 1e150 in magnitude is compared with every point.
 * Non-finite or |x| > 1e150 surface coordinates, and n < 4096 with cell_size 0, take the brute-force kernel of knn_outer.hip in
 * chunks of SAPCU_POINTING_BRUTE_CHUNK candidates into a table in the workspace, then the same finishing code.  cell_size is the
 * cell edge, 0 = automatic; any value gives the same result.  One stream synchronisation (the grid's size is read back).
 *
 * Memory contract (checked under guard bands by tests/test_gpu_pointing.py):
 *   - surface, voxels and jitter [m,3] f64 (m = nv * sub^3; the rows of THIS call's candidates) are only read;
 *   - keep_out u8 [m] is written in full, and so are d1_out f64 [m] and idx_out i32 [m,k] when given (either may be NULL);
 *     points_out f64 [m,3], pointing_out f64 [m,3] and candidate_out i64 [m] are written in their first *count_out rows and nowhere
 *     else; count_out is one DEVICE int64;
 *   - nothing is written beyond the sizer's bytes of the workspace, which needs NO initialisation and 8-byte alignment;
 *   - info_host (HOST int64[4], may be NULL) receives {1 if the grid ran else 0, gx, gy, gz};
 *   - nv == 0 launches and writes nothing (info_host is zeroed);
 *   - refused with SAPCU_ERR_ARG before anything is launched: a NULL pointer among the required ones, n outside [1, 2^29], nv < 0,
 *     count outside [1, 2^20], sub outside [1, 1024], m > 2^31 - 64, k outside [1, SAPCU_POINTING_MAX_K] or above n, origin, step,
 *     step2, half2 or cell_size not finite, cell_size < 0, a NaN band end, candidate0 < 0, a misaligned workspace or one with
 *     fewer bytes than the sizer's.
 */
#ifndef SAPCU_POINTING_H
#define SAPCU_POINTING_H

#include "../../include/sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAPCU_POINTING_MAX_K 16
#define SAPCU_POINTING_BRUTE_CHUNK 65536

/* Bytes of workspace for sapcu_pointing_samples_f32; -1 for sizes the call would refuse. */
int64_t sapcu_pointing_workspace_bytes(int64_t n, int64_t nv, int sub, int k);

int sapcu_pointing_samples_f32(const float* surface, int64_t n, const int64_t* voxels, int64_t nv, double origin, double step, int count,
                               int sub, double step2, double half2, const double* jitter, int k, double band_lo, double band_hi,
                               double cell_size, int64_t candidate0, uint8_t* keep_out, double* d1_out, int32_t* idx_out,
                               double* points_out, double* pointing_out, int64_t* candidate_out, int64_t* count_out, void* workspace,
                               int64_t workspace_bytes, int64_t* info_host, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_POINTING_H */
