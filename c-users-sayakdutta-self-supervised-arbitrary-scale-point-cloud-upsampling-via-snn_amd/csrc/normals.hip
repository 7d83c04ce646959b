// PCA normals of a cloud from its neighbour table, and the angle between two tables of normals (sapcu_amd/normals.py).  Replaces
// the per-point Python loop (np.cov + np.linalg.eigh) of the reference's scripts/generate_gt_normals.py and the host arithmetic of
// scripts/old_metrics/eval_normals.py.  The definition, op for op, is in include/sapcu_normals.h and in numpy in
// tests/normals_ref.py; every operation below is a separately rounded f64 operation (__dadd_rn .. and -ffp-contract=off).
//
// pca_normals_kernel, one row per lane, 256 lanes per workgroup, no LDS, no scratch:
//   * pass 1 reads the row's k indices, checks each against [0, n), and sums the neighbours in table order (mean);
//   * pass 2 reads them again (24 B per neighbour, neighbours are spatially close: L2 hits) and accumulates the six sums of the
//     covariance; nothing indexed by j is kept, so k up to 64 costs no registers;
//   * 8 Jacobi sweeps over (0,1), (0,2), (1,2): the six entries of the symmetric matrix and the nine of V are named registers, a
//     rotation is one inlined function on references; the sweep loop is not unrolled (three rotations per trip);
//   * the column under the smallest diagonal entry is picked with selects, never with a runtime index;
//   * a row with an index outside [0, n) reads nothing through it, adds its bad entries to *bad (one atomic per lane that has any;
//     integer, order-free) and stores NaN;
//   * results leave through ordinary vector stores.
// normal_angles_kernel, one row per lane: the script's normalisation, dot, clamp, acos and degrees.
#include "common.h"
#include "../../include/sapcu_normals.h"

namespace sapcu {

constexpr int NORMALS_THREADS = 256;

// The correctly rounded square root, from the device's sqrt (taken as at most one ulp off) and the exact residual r = d - s*s (one
// FMA; exact for such an s): s stays when -s*dn < r <= s*up, dn / up its distances to the neighbouring doubles, and moves one
// double otherwise.  r, s*up and s*dn are multiples of ulp(s)^2 and the u^2/4 of (s +- u/2)^2 is below that step, so the two
// comparisons decide exactly.  Not common.h's sqrt_cr: its rounding FMA s + r * (0.5 / s) returns 1.0 for d = 1 - 2^-53 (the true
// root lies 2^-109 below the midpoint of 1 - 2^-53 and 1, the rounding of 0.5 / s lifts the sum above it), an argument that
// |n|^2 of a unit normal takes in one row of thirty, and NaN for d = +inf, which theta * theta + 1 reaches one sweep before an
// off-diagonal reaches 0 (the definition wants sqrt(inf) = inf there: t = +-0).  Zero, arguments below 1e-280 (the step ulp(s)^2 would leave
// the normal range), infinite and NaN arguments return the device's sqrt.
__device__ __forceinline__ double sqrt_exact(double d) {
    const double s = sqrt(d);
    if (!(d >= 1e-280 && d < __builtin_huge_val())) return s;
    const double r = __fma_rn(-s, s, d);
    const long long b = __double_as_longlong(s);
    const double above = __longlong_as_double(b + 1), below = __longlong_as_double(b - 1);
    if (r > __dmul_rn(s, __dsub_rn(above, s))) return above;
    if (r <= -__dmul_rn(s, __dsub_rn(s, below))) return below;
    return s;
}

// one Jacobi rotation of the pair (p, q), r the third index: the definition's step 3.  vXp / vXq: rows X of the columns p, q of V.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                              double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = __ddiv_rn(__dsub_rn(aqq, app), __dmul_rn(2.0, apq));
    const double den = __dadd_rn(fabs(theta), sqrt_exact(__dadd_rn(__dmul_rn(theta, theta), 1.0)));
    const double t = __ddiv_rn(theta >= 0.0 ? 1.0 : -1.0, den);
    const double c = __ddiv_rn(1.0, sqrt_exact(__dadd_rn(__dmul_rn(t, t), 1.0)));
    const double s = __dmul_rn(t, c);
    const double tap = __dmul_rn(t, apq);
    app = __dsub_rn(app, tap);
    aqq = __dadd_rn(aqq, tap);
    apq = 0.0;
    const double rp = __dsub_rn(__dmul_rn(c, arp), __dmul_rn(s, arq));
    const double rq = __dadd_rn(__dmul_rn(s, arp), __dmul_rn(c, arq));
    arp = rp;
    arq = rq;
    const double n0p = __dsub_rn(__dmul_rn(c, v0p), __dmul_rn(s, v0q)), n0q = __dadd_rn(__dmul_rn(s, v0p), __dmul_rn(c, v0q));
    const double n1p = __dsub_rn(__dmul_rn(c, v1p), __dmul_rn(s, v1q)), n1q = __dadd_rn(__dmul_rn(s, v1p), __dmul_rn(c, v1q));
    const double n2p = __dsub_rn(__dmul_rn(c, v2p), __dmul_rn(s, v2q)), n2q = __dadd_rn(__dmul_rn(s, v2p), __dmul_rn(c, v2q));
    v0p = n0p; v0q = n0q;
    v1p = n1p; v1q = n1q;
    v2p = n2p; v2q = n2q;
}

__global__ __launch_bounds__(NORMALS_THREADS) void pca_normals_kernel(const double* __restrict__ pts, int64_t n,
                                                                      const int64_t* __restrict__ idx, int64_t rows, int k, int has_view,
                                                                      double vx, double vy, double vz, double* __restrict__ normals,
                                                                      double* __restrict__ evals, int* __restrict__ bad) {
    const int64_t row = (int64_t)blockIdx.x * NORMALS_THREADS + threadIdx.x;
    if (row >= rows) return;
    const int64_t* __restrict__ tab = idx + row * (int64_t)k;
    double* __restrict__ nout = normals + row * 3;
    double* __restrict__ eout = evals ? evals + row * 3 : nullptr;

    // pass 1: the indices, the mean
    int nbad = 0;
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int j = 0; j < k; ++j) {
        const int64_t i = tab[j];
        const bool ok = i >= 0 && i < n;
        nbad += ok ? 0 : 1;
        const int64_t s = ok ? i : 0;                                    // n >= 1: point 0 exists; the row's result is dropped
        mx = __dadd_rn(mx, pts[s * 3 + 0]);
        my = __dadd_rn(my, pts[s * 3 + 1]);
        mz = __dadd_rn(mz, pts[s * 3 + 2]);
    }
    if (nbad) {
        atomicAdd(bad, nbad);
        const double qnan = __builtin_nan("");
        nout[0] = qnan; nout[1] = qnan; nout[2] = qnan;
        if (eout) { eout[0] = qnan; eout[1] = qnan; eout[2] = qnan; }
        return;
    }
    const double kd = (double)k;
    mx = __ddiv_rn(mx, kd);
    my = __ddiv_rn(my, kd);
    mz = __ddiv_rn(mz, kd);

    // pass 2: the covariance (every index is known to be in range)
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
    for (int j = 0; j < k; ++j) {
        const int64_t i = tab[j];
        const double dx = __dsub_rn(pts[i * 3 + 0], mx);
        const double dy = __dsub_rn(pts[i * 3 + 1], my);
        const double dz = __dsub_rn(pts[i * 3 + 2], mz);
        a00 = __dadd_rn(a00, __dmul_rn(dx, dx));
        a01 = __dadd_rn(a01, __dmul_rn(dx, dy));
        a02 = __dadd_rn(a02, __dmul_rn(dx, dz));
        a11 = __dadd_rn(a11, __dmul_rn(dy, dy));
        a12 = __dadd_rn(a12, __dmul_rn(dy, dz));
        a22 = __dadd_rn(a22, __dmul_rn(dz, dz));
    }
    const double km1 = (double)(k - 1);
    a00 = __ddiv_rn(a00, km1);
    a01 = __ddiv_rn(a01, km1);
    a02 = __ddiv_rn(a02, km1);
    a11 = __ddiv_rn(a11, km1);
    a12 = __ddiv_rn(a12, km1);
    a22 = __ddiv_rn(a22, km1);

    // V = I; v<row><column>
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < SAPCU_PCA_NORMALS_SWEEPS; ++sweep) {
        jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0,1), r = 2
        jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0,2), r = 1
        jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1,2), r = 0
    }

    // the column under the smallest diagonal entry, the lowest column among equal ones
    int col = 0;
    double lo = a00;
    if (a11 < lo) { col = 1; lo = a11; }
    if (a22 < lo) { col = 2; lo = a22; }
    double nx = col == 0 ? v00 : (col == 1 ? v01 : v02);
    double ny = col == 0 ? v10 : (col == 1 ? v11 : v12);
    double nz = col == 0 ? v20 : (col == 1 ? v21 : v22);
    if (eout) {
        const double x = col == 0 ? a11 : a00;                            // the other two, in column order
        const double y = col == 2 ? a11 : a22;
        const bool swap = y < x;
        eout[0] = lo;
        eout[1] = swap ? y : x;
        eout[2] = swap ? x : y;
    }

    bool flip;
    if (has_view) {
        const int64_t own = tab[0];
        const double px = pts[own * 3 + 0], py = pts[own * 3 + 1], pz = pts[own * 3 + 2];
        const double d = __dadd_rn(__dadd_rn(__dmul_rn(nx, __dsub_rn(vx, px)), __dmul_rn(ny, __dsub_rn(vy, py))),
                                   __dmul_rn(nz, __dsub_rn(vz, pz)));
        flip = d < 0.0;
    } else {
        double big = nx;
        if (fabs(ny) > fabs(big)) big = ny;
        if (fabs(nz) > fabs(big)) big = nz;
        flip = big < 0.0;                                                 // -0.0 < 0.0 is false
    }
    nout[0] = flip ? -nx : nx;
    nout[1] = flip ? -ny : ny;
    nout[2] = flip ? -nz : nz;
}

__global__ __launch_bounds__(NORMALS_THREADS) void normal_angles_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                                        int64_t rows, int oriented, double lo, double hi,
                                                                        double* __restrict__ cos_out, double* __restrict__ deg_out) {
    const int64_t row = (int64_t)blockIdx.x * NORMALS_THREADS + threadIdx.x;
    if (row >= rows) return;
    const double ax = a[row * 3 + 0], ay = a[row * 3 + 1], az = a[row * 3 + 2];
    const double bx = b[row * 3 + 0], by = b[row * 3 + 1], bz = b[row * 3 + 2];
    const double na = __dadd_rn(sqrt_exact(__dadd_rn(__dadd_rn(__dmul_rn(ax, ax), __dmul_rn(ay, ay)), __dmul_rn(az, az))), 1e-9);
    const double nb = __dadd_rn(sqrt_exact(__dadd_rn(__dadd_rn(__dmul_rn(bx, bx), __dmul_rn(by, by)), __dmul_rn(bz, bz))), 1e-9);
    const double px = __dmul_rn(__ddiv_rn(ax, na), __ddiv_rn(bx, nb));
    const double py = __dmul_rn(__ddiv_rn(ay, na), __ddiv_rn(by, nb));
    const double pz = __dmul_rn(__ddiv_rn(az, na), __ddiv_rn(bz, nb));
    double dot = __dadd_rn(__dadd_rn(px, py), pz);
    dot = dot < lo ? lo : (dot > hi ? hi : dot);                          // a NaN fails both comparisons and stays
    if (cos_out) cos_out[row] = dot;
    deg_out[row] = __dmul_rn(acos(oriented ? dot : fabs(dot)), 57.29577951308232);     // np.degrees: x * (180 / pi)
}

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

extern "C" {

int sapcu_pca_normals_f64(const double* pts, int64_t n, const int64_t* idx, int64_t rows, int k, const double* viewpoint_host,
                          double* normals_out, double* evals_out, int32_t* bad_count, void* stream) {
    SAPCU_CHECK_ARG(pts && idx && normals_out && bad_count, "pca_normals: null pointer (pts, idx, normals_out and bad_count are required)");
    SAPCU_CHECK_ARG(k >= 3 && k <= SAPCU_PCA_NORMALS_MAX_K, "pca_normals: need 3 <= k <= %d (k=%d)", SAPCU_PCA_NORMALS_MAX_K, k);
    SAPCU_CHECK_ARG(n >= 1, "pca_normals: need n >= 1 (n=%lld)", (long long)n);
    SAPCU_CHECK_ARG(rows >= 0 && rows <= (1LL << 31) - 64, "pca_normals: need 0 <= rows <= 2^31 - 64 (rows=%lld)", (long long)rows);
    hipStream_t st = (hipStream_t)stream;
    const int zrc = zero_count(bad_count, st);
    if (zrc != SAPCU_OK) return zrc;
    if (rows == 0) return SAPCU_OK;
    const double vx = viewpoint_host ? viewpoint_host[0] : 0.0, vy = viewpoint_host ? viewpoint_host[1] : 0.0,
                 vz = viewpoint_host ? viewpoint_host[2] : 0.0;
    const unsigned grid = (unsigned)((rows + NORMALS_THREADS - 1) / NORMALS_THREADS);
    hipLaunchKernelGGL(pca_normals_kernel, dim3(grid), dim3(NORMALS_THREADS), 0, st, pts, n, idx, rows, k, viewpoint_host ? 1 : 0, vx, vy,
                       vz, normals_out, evals_out, bad_count);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int sapcu_normal_angles_f64(const double* a, const double* b, int64_t rows, int oriented, double clamp_eps, double* cos_out,
                            double* deg_out, void* stream) {
    SAPCU_CHECK_ARG(a && b && deg_out, "normal_angles: null pointer (a, b and deg_out are required)");
    SAPCU_CHECK_ARG(rows >= 0 && rows <= (1LL << 31) - 64, "normal_angles: need 0 <= rows <= 2^31 - 64 (rows=%lld)", (long long)rows);
    SAPCU_CHECK_ARG(oriented == 0 || oriented == 1, "normal_angles: oriented must be 0 or 1 (%d)", oriented);
    SAPCU_CHECK_ARG(clamp_eps >= 0.0 && clamp_eps <= 1.0, "normal_angles: clamp_eps must lie in [0, 1]");
    if (rows == 0) return SAPCU_OK;
    const double lo = -1.0 + clamp_eps, hi = 1.0 - clamp_eps;
    const unsigned grid = (unsigned)((rows + NORMALS_THREADS - 1) / NORMALS_THREADS);
    hipLaunchKernelGGL(normal_angles_kernel, dim3(grid), dim3(NORMALS_THREADS), 0, (hipStream_t)stream, a, b, rows, oriented, lo, hi,
                       cos_out, deg_out);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

}  // extern "C"
