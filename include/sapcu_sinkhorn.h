/*
 * sapcu_sinkhorn.h — entropic optimal transport (Sinkhorn) between two clouds on the device, without the n x m cost matrix: the
 * transport figures of the upsampling literature (sapcu_amd/sinkhorn.py; the "Sinkhorn" rows of the reference README's "Metrics &
 * Evaluation", whose scripts/compute_sinkhorn.py is not in its tree, and the EMD column of evaluation_cd.py, which needs pyemd).
 *
 * Part of libsapcu_hip.so; the conventions and status codes of sapcu.h apply (device pointers unless named *_host, the caller owns
 * every buffer, 0 on success, sapcu_last_error() for the text).  SAPCU_ABI_VERSION is unchanged: these entry points are additions.
 *
 * Definition (tests/sinkhorn_ref.py states it in numpy).  Clouds x [n,3] and y [m,3], uniform weights a_i = 1/n, b_j = 1/m.
 *   s_ij = ((x-y)_x^2 + (x-y)_y^2) + (x-y)_z^2 in separately rounded f64 operations (as sapcu_metrics.h);
 *   C_ij = s_ij / 2 for p = 2, sqrt(s_ij) for p = 1;
 *   softmin_eps(y, pot)[i] = -eps * log sum_j exp(h_j - C_ij / eps),   h_j = log b_j + pot_j / eps;
 *   one iteration: f <- softmin over y with g, then g <- softmin over x with the NEW f; start f = g = 0;
 *   the symmetric problem (y NULL): f <- (f + softmin over x with f) / 2;
 *   plan P_ij = a_i b_j exp((f_i + g_j - C_ij) / eps);  r_i = sum_j P_ij,  c_i = sum_j P_ij C_ij.
 *
 * How it runs (csrc/sinkhorn.hip).  One row per lane; the other cloud and its h_j stream through LDS in tiles of 64 columns, each
 * read back by all lanes at once (a broadcast); the cost is recomputed per pair; the log-sum-exp is online (running maximum and
 * rescaled sum).  The columns are cut into `split` contiguous chunks, one wavefront each, split = f(rows, columns) only; the
 * (max, sum) partials go to the workspace with ordinary stores and a second kernel merges them in chunk order.  No atomics: the
 * result is bit-identical from run to run and does not depend on what the workspace held.
 *
 * Memory contract (as sapcu.h; checked under guard bands by tests/test_gpu_sinkhorn.py):
 *   - x [n,3], y [m,3], pot_y [m], f [n], g [m] inputs are f64 and only read; the outputs named below are written in full, nothing
 *     else; nothing is written beyond the workspace_bytes the sizer returned for the same (n, m) (for the symmetric problem: (n, n));
 *   - the workspace needs NO initialisation and 8-byte alignment (f64 tables inside);
 *   - refused before anything is launched, with SAPCU_ERR_ARG: a NULL input or output (sapcu_sinkhorn_f64: y NULL selects the
 *     symmetric problem, g_out is then not used and may be NULL; eps_schedule_host may be NULL only with n_schedule == 0), n or m < 1
 *     or > 2^24, p not 1 or 2, eps or any schedule entry not finite or <= 0, iters < 0, n_schedule < 0, n_schedule + iters > 2^20, a
 *     NULL workspace, one shorter than the sizer's bytes or not 8-byte aligned;
 *   - `stream` is never synchronised and nothing is read back: every call only enqueues launches and can be captured in a graph.
 */
#ifndef SAPCU_SINKHORN_H
#define SAPCU_SINKHORN_H

#include "sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for clouds of n and m points (any of the three entry points below); -1 for sizes they would refuse. */
int64_t sapcu_sinkhorn_workspace_bytes(int64_t n, int64_t m);

/* One half-step: out[i] = softmin_eps(y, pot_y)[i] for every row of x.  Writes out [n]. */
int sapcu_softmin_f64(const double* x, int64_t n, const double* y, int64_t m, const double* pot_y, int p, double eps, double* out,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* The whole loop: one iteration at each eps_schedule_host[k] (HOST array, read during the call), then `iters` iterations at `eps`.
 * Writes f_out [n] and g_out [m]; with y NULL the symmetric problem of x, f_out [n] only (m is ignored). */
int sapcu_sinkhorn_f64(const double* x, int64_t n, const double* y, int64_t m, int p, const double* eps_schedule_host,
                       int64_t n_schedule, double eps, int64_t iters, double* f_out, double* g_out, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* Row statistics of the plan of (f, g): writes r_out [n] and c_out [n]. */
int sapcu_plan_stats_f64(const double* x, int64_t n, const double* y, int64_t m, const double* f, const double* g, int p, double eps,
                         double* r_out, double* c_out, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_SINKHORN_H */
