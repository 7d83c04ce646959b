/*
 * sapcu_normals.h — PCA normals of a cloud from its neighbour table, and the angle between two tables of normals, on the device
 * (sapcu_amd/normals.py).  The quantities of the reference's scripts/generate_gt_normals.py (estimate_normals_pca: sklearn
 * NearestNeighbors(k), then np.cov + np.linalg.eigh per point in a Python loop) and scripts/old_metrics/eval_normals.py
 * (angular_error_deg), with the oriented variant of fn/trainer.py:eval_step.
 *
 * Part of libsapcu_hip.so; the conventions and status codes of sapcu.h apply (device pointers unless named *_host, the caller owns
 * every buffer, 0 on success, sapcu_last_error() for the text).  SAPCU_ABI_VERSION is unchanged: these entry points are additions.
 *
 * ---- sapcu_pca_normals_f64 -------------------------------------------------------------------------------------------------------
 * pts [n,3] f64; idx [rows,k] int64 is the neighbour table of those rows, as sapcu_knn_self_grid_f64 returns it: the row's own
 * point (or a point at the same position) is its first entry, as in sklearn's kneighbors(pts).  3 <= k <= 64.
 *
 * Definition (every operation a separately rounded f64 operation, no FMA; tests/normals_ref.py states it in numpy, op for op):
 *   1. mean_c = (((0 + p_0c) + p_1c) + ... ) / k, the neighbours p_j = pts[idx[row,j]] in table order;
 *   2. d_j = p_j - mean; the six sums S_ab = ((0 + d_0a*d_0b) + d_1a*d_1b) + ... in table order, C_ab = S_ab / (k - 1)
 *      (np.cov's ddof);
 *   3. cyclic Jacobi on C with V = I: exactly 8 sweeps over the pairs (p,q) = (0,1), (0,2), (1,2), no convergence test.  A pair
 *      whose off-diagonal a_pq is exactly 0.0 is skipped (nothing changes, not even the sign of a zero).  Otherwise, r the third
 *      index:
 *          theta = (a_qq - a_pp) / (2 * a_pq)
 *          t     = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta*theta + 1))        (an infinite theta or theta*theta: t = +-0)
 *          c     = 1 / sqrt(t*t + 1),   s = t * c                                   (sqrt correctly rounded)
 *          a_pp' = a_pp - t*a_pq,   a_qq' = a_qq + t*a_pq,   a_pq' = 0
 *          a_rp' = c*a_rp - s*a_rq, a_rq' = s*a_rp + c*a_rq
 *          V[:,p]' = c*V[:,p] - s*V[:,q],   V[:,q]' = s*V[:,p] + c*V[:,q]
 *   4. the normal is the column of V under the smallest diagonal entry, the lowest column among equal ones (a zero covariance
 *      gives (1, 0, 0)).  It is not renormalised: | |v| - 1 | stays below 8e-16;
 *   5. sign.  viewpoint_host == NULL: the component of largest magnitude is made positive (the first such component among equal
 *      magnitudes; -0.0 is not negative), by negating all three components.  Otherwise the normal is negated when
 *      ((n_x*(v_x - p_x) + n_y*(v_y - p_y)) + n_z*(v_z - p_z)) < 0, p = pts[idx[row,0]]: it then points to the viewpoint's side;
 *   evals_out (may be NULL): the three diagonal entries, ascending: the smallest as chosen in 4, then the other two in column
 *   order, swapped when the later one is smaller.
 *
 * Bad indices.  Every entry of idx outside [0, n) adds one to *bad_count (device int32, zeroed by the call); its row gets NaN in
 * normals_out and evals_out, and nothing outside pts is read.
 *
 * How it runs (csrc/normals.hip): one row per lane, 256 lanes per workgroup, no LDS, no scratch.  The neighbours are gathered
 * straight from pts, twice (mean, then covariance); covariance, rotations and V stay in registers.
 *
 * ---- sapcu_normal_angles_f64 -----------------------------------------------------------------------------------------------------
 * a, b [rows,3] f64.  Per row, in the script's order:
 *   |x| = sqrt((x_x^2 + x_y^2) + x_z^2) (correctly rounded);   xh = x / (|x| + 1e-9);
 *   dot = (ah_x*bh_x + ah_y*bh_y) + ah_z*bh_z, clamped to [-1 + clamp_eps, 1 - clamp_eps] (a NaN stays a NaN);
 *   cos_out[row] (may be NULL) = the clamped dot;
 *   deg_out[row] = acos(oriented ? dot : |dot|) * (180 / pi).
 * oriented = 0, clamp_eps = 0: angular_error_deg of eval_normals.py.  oriented = 1, clamp_eps = 1e-6: the trainer's eval_step.
 * A zero normal gives dot = 0 and 90 degrees, as in the script.  cos_out equals numpy bit for bit; deg_out is within the error of
 * the device's acos of it (4 ulp).
 *
 * ---- memory contract (as sapcu.h; checked under guard bands by tests/test_gpu_normals.py) ----------------------------------------
 *   - inputs are only read; normals_out [rows,3], evals_out [rows,3] (when given), deg_out [rows] and cos_out [rows] (when given)
 *     are written in full whatever they held, bad_count is written, nothing else; no workspace;
 *   - rows == 0 launches nothing (bad_count is still zeroed);
 *   - refused before anything is launched, with SAPCU_ERR_ARG: a NULL pts, idx, normals_out or bad_count; a NULL a, b or deg_out;
 *     k < 3 or k > 64; n < 1; rows < 0 or rows > 2^31 - 64; oriented not 0 or 1; clamp_eps negative, NaN or > 1;
 *   - nothing is synchronised.
 */
#ifndef SAPCU_NORMALS_H
#define SAPCU_NORMALS_H

#include "sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAPCU_PCA_NORMALS_MAX_K 64
#define SAPCU_PCA_NORMALS_SWEEPS 8

int sapcu_pca_normals_f64(const double* pts, int64_t n, const int64_t* idx, int64_t rows, int k,
                          const double* viewpoint_host /* NULL or HOST double[3] */,
                          double* normals_out /* [rows,3] */, double* evals_out /* [rows,3] ascending, may be NULL */,
                          int32_t* bad_count /* device, zeroed by the call */, void* stream);

int sapcu_normal_angles_f64(const double* a, const double* b, int64_t rows, int oriented, double clamp_eps,
                            double* cos_out /* may be NULL */, double* deg_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_NORMALS_H */
