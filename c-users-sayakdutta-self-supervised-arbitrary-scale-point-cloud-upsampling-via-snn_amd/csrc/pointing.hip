// Seed-centred training samples of fn on the device: the candidates of the reference's scripts/sample_mesh-fn.py export_pointing
// (fine cells of the voxels near a surface cloud, jittered), their k nearest surface points, the band test on the first distance
// and the unit vector towards the neighbours' mean.  Replaces one host KDTree.query(candidates, 10) of a few million rows against
// 800 000 points per mesh.  csrc/sapcu_pointing.h has the definition, operation by operation; tests/pointing_ref.py states it in numpy.
//
// pointing_search_kernel<K>, one candidate per thread:
//   * the surface cloud, widened to f64, is sorted into knn_grid.hip's cell grid by its launchers;
//   * candidate i = t * sub^3 + j evaluates its own position: consecutive candidates are neighbouring fine cells of one voxel, so
//     the lanes of a wavefront walk nearly the same cells and most of their loads share an address;
//   * the running k nearest are a PtList<K> in registers, ascending on (squared distance, index), the scheme of
//     dense_seeds_dev.hip's SeedList: one instance per k, every index a compile-time constant, no scratch;
//   * the search is grid_shell_walk (knn_grid.h) with a per-thread stop against the K-th squared distance.  The queries are foreign
//     to the grid, so the margin is formed as nn_cross_kernel forms it, per thread: GridParams.slack + 1e-11 * (the query's largest
//     |coordinate|).  A query that is not finite or beyond 1e150 (the caller's jitter decides) is compared with every point;
//   * `early`: when the caller wants neither d1 nor the neighbour table of every candidate, a walk also ends once everything
//     unvisited is beyond band_hi (the same comparison, against band_hi^2) and the nearest visited point is too — keep is 0 then;
//   * pt_finish: the band test and the pointing, in the same kernel; a kept candidate parks q and the pointing in the workspace;
//   * compaction: the keep flags, knn_grid.hip's three-kernel exclusive scan, one scatter kernel — the candidates' own order.
// Non-finite or huge (|x| > 1e150) surface coordinates, and n < KNN_GRID_MIN_N with the automatic cell size, run knn_outer.hip's
// brute-force kernel instead, PT_BRUTE_CHUNK candidates at a time into a table, and pointing_table_kernel finishes from the table.
#include "common.h"
#include "knn_grid.h"
#include "sapcu_pointing.h"

namespace sapcu {

constexpr int PT_CELL_POP = 16;                  // automatic cell edge: emax * sqrt(2 * PT_CELL_POP / n) (profiles/pointing.txt)
constexpr int PT_MAX_K = SAPCU_POINTING_MAX_K;
constexpr int64_t PT_BRUTE_CHUNK = SAPCU_POINTING_BRUTE_CHUNK;
constexpr int PT_EMPTY = 0x7fffffff;

struct PtGeom {
    double origin, step, step2, half2;
    int count, sub, sub3;
};

struct PtOut {
    const float* surface;      // [n,3] f32: the rows the sum is taken over
    double lo, hi;
    uint8_t* keep;             // [m]
    double* d1;                // [m] or null
    int32_t* idx;              // [m,k] or null
    int* flags;                // [m + 1] workspace: keep as int, then its exclusive scan
    double* wq;                // [m,3] workspace: q (every row on the brute-force route, kept rows on the grid's)
    double* wp;                // [m,3] workspace: pointing of kept rows
};

struct PtWs {
    double* p64;               // [n,3] the surface widened
    GridWs grid;
    int* flags;
    int* tile_sums;
    double* wq;
    double* wp;
    int64_t* bidx;             // [min(m, PT_BRUTE_CHUNK), k] the brute-force route's table
    double* bdist;
    size_t bytes;
};

static PtWs pt_ws_layout(void* base, int64_t n, int64_t m, int k) {
    WsCarver c(base);
    PtWs w;
    w.p64 = c.take<double>(3 * n);
    w.grid = grid_ws_layout(c.take<char>((int64_t)grid_ws_layout(nullptr, n).bytes), n);
    w.flags = c.take<int>(m + 1);
    w.tile_sums = c.take<int>((m + 1 + SCAN_TILE - 1) / SCAN_TILE);
    w.wq = c.take<double>(3 * m);
    w.wp = c.take<double>(3 * m);
    const int64_t ch = m < PT_BRUTE_CHUNK ? m : PT_BRUTE_CHUNK;
    w.bidx = c.take<int64_t>(ch * k);
    w.bdist = c.take<double>(ch * k);
    w.bytes = c.bytes();
    return w;
}

__global__ __launch_bounds__(256) void pointing_widen_kernel(const float* __restrict__ in, int64_t count, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = (double)in[i];
}

// the position of candidate i (of this call): sapcu_pointing.h, operation by operation
__device__ __forceinline__ void pt_query(const PtGeom& g, const int64_t* __restrict__ voxels, const double* __restrict__ jitter, int64_t i,
                                         double& qx, double& qy, double& qz) {
    const int64_t t = i / g.sub3;
    int j = (int)(i - t * g.sub3);
    int64_t v = voxels[t];
    const int jz = j % g.sub;
    j /= g.sub;
    const int jy = j % g.sub, jx = j / g.sub;
    const int64_t iz = v % g.count;
    v /= g.count;
    const int64_t iy = v % g.count, ix = v / g.count;
    qx = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn((double)ix, g.step), g.origin), __dmul_rn((double)jx, g.step2)), g.half2);
    qy = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn((double)iy, g.step), g.origin), __dmul_rn((double)jy, g.step2)), g.half2);
    qz = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn((double)iz, g.step), g.origin), __dmul_rn((double)jz, g.step2)), g.half2);
    if (jitter) {
        qx = __dadd_rn(qx, jitter[3 * i + 0]);
        qy = __dadd_rn(qy, jitter[3 * i + 1]);
        qz = __dadd_rn(qz, jitter[3 * i + 2]);
    }
}

// steps 4 and 5 for candidate i: nb(j) is neighbour j (-1: empty), d1 the first distance (+inf: none).  K > 0: k = K at compile time
template <int K, typename Nb>
__device__ __forceinline__ void pt_finish(const PtOut& o, int64_t i, int k, double d1, double qx, double qy, double qz, Nb nb) {
    const int kk = K ? K : k;
    const bool keep = nb(kk - 1) >= 0 && d1 >= o.lo && d1 <= o.hi;
    o.keep[i] = keep ? 1 : 0;
    o.flags[i] = keep ? 1 : 0;
    if (o.d1) o.d1[i] = d1;
    if (o.idx) {
#pragma unroll
        for (int j = 0; j < kk; ++j) o.idx[i * kk + j] = nb(j);
    }
    if (!keep) return;
    const float* p0 = o.surface + 3 * (int64_t)nb(0);
    float sx = p0[0], sy = p0[1], sz = p0[2];
#pragma unroll
    for (int j = 1; j < kk; ++j) {
        const float* p = o.surface + 3 * (int64_t)nb(j);
        sx = __fadd_rn(sx, p[0]);
        sy = __fadd_rn(sy, p[1]);
        sz = __fadd_rn(sz, p[2]);
    }
    const float fk = (float)kk;
    const double wx = __dsub_rn((double)__fdiv_rn(sx, fk), qx);
    const double wy = __dsub_rn((double)__fdiv_rn(sy, fk), qy);
    const double wz = __dsub_rn((double)__fdiv_rn(sz, fk), qz);
    const double len = sqrt_cr(__dadd_rn(__dadd_rn(__dmul_rn(wx, wx), __dmul_rn(wy, wy)), __dmul_rn(wz, wz)));
    o.wq[3 * i + 0] = qx;
    o.wq[3 * i + 1] = qy;
    o.wq[3 * i + 2] = qz;
    o.wp[3 * i + 0] = __ddiv_rn(wx, len);
    o.wp[3 * i + 1] = __ddiv_rn(wy, len);
    o.wp[3 * i + 2] = __ddiv_rn(wz, len);
}

// the running K nearest of one thread, ascending on (d, i), in registers (every index below is a compile-time constant)
template <int K>
struct PtList {
    double d[K];
    int i[K];
};

__device__ __forceinline__ bool pt_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

template <int K>
__device__ __forceinline__ void pt_scan_range(PtList<K>& L, int a, int b, double qx, double qy, double qz, const double* __restrict__ sx,
                                              const double* __restrict__ sy, const double* __restrict__ sz,
                                              const int* __restrict__ sidx) {
    for (int j = a; j < b; ++j) {
        const double cd = dist2_rn(qx, qy, qz, sx[j], sy[j], sz[j]);
        const int ci = sidx[j];
        if (!(cd < __builtin_huge_val())) continue;                      // NaN or +inf: no candidate
        if (!pt_less(cd, ci, L.d[K - 1], L.i[K - 1])) continue;
#pragma unroll
        for (int p = K - 1; p >= 0; --p) {                               // downwards: entry p-1 is still the old one
            const bool below_prev = p > 0 && pt_less(cd, ci, L.d[p > 0 ? p - 1 : 0], L.i[p > 0 ? p - 1 : 0]);
            const bool below_cur = pt_less(cd, ci, L.d[p], L.i[p]);
            if (below_prev) {
                L.d[p] = L.d[p > 0 ? p - 1 : 0];
                L.i[p] = L.i[p > 0 ? p - 1 : 0];
            } else if (below_cur) {
                L.d[p] = cd;
                L.i[p] = ci;
            }
        }
    }
}

template <int K>
__global__ __launch_bounds__(256) void pointing_search_kernel(PtGeom g, const int64_t* __restrict__ voxels, const double* __restrict__ jitter,
                                                              int64_t m, int64_t n, const GridParams* __restrict__ prm,
                                                              const int* __restrict__ start, const double* __restrict__ sx,
                                                              const double* __restrict__ sy, const double* __restrict__ sz,
                                                              const int* __restrict__ sidx, int early, double hi2, PtOut o) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double qx, qy, qz;
    pt_query(g, voxels, jitter, i, qx, qy, qz);
    const GridParams p = *prm;
    const double INF = __builtin_huge_val();
    PtList<K> L;
#pragma unroll
    for (int q = 0; q < K; ++q) {
        L.d[q] = INF;
        L.i[q] = PT_EMPTY;
    }
    const double amax = fmax(fmax(fabs(qx), fabs(qy)), fabs(qz));
    if (!(amax <= 1e150)) {                                              // a NaN, an infinity, or a square that could overflow
        pt_scan_range<K>(L, 0, (int)n, qx, qy, qz, sx, sy, sz, sidx);
    } else {
        const int cx = grid_coord(qx, p.ox, p.h, p.gx);
        const int cy = grid_coord(qy, p.oy, p.h, p.gy);
        const int cz = grid_coord(qz, p.oz, p.h, p.gz);
        grid_shell_walk(                                                 // one candidate per thread: a per-thread stop rule
            p, start, cx, cy, cz, qx, qy, qz, __dadd_rn(p.slack, __dmul_rn(1e-11, amax)),
            [&](int a, int b) { pt_scan_range<K>(L, a, b, qx, qy, qz, sx, sy, sz, sidx); },
            [&](double bnd) {
                if (grid_bound_clears(bnd, L.d[K - 1])) return true;
                return early && grid_bound_clears(bnd, hi2) && !(sqrt_cr(L.d[0]) <= o.hi);    // nothing, seen or unseen, within band_hi
            });
    }
    pt_finish<K>(o, i, K, sqrt_cr(L.d[0]), qx, qy, qz, [&](int j) { return L.i[j] == PT_EMPTY ? -1 : L.i[j]; });
}

// ---------------------------------------------------------------------------------------------- the brute-force route
__global__ __launch_bounds__(256) void pointing_queries_kernel(PtGeom g, const int64_t* __restrict__ voxels, const double* __restrict__ jitter,
                                                               int64_t i0, int64_t i1, double* __restrict__ wq) {
    const int64_t i = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= i1) return;
    double qx, qy, qz;
    pt_query(g, voxels, jitter, i, qx, qy, qz);
    wq[3 * i + 0] = qx;
    wq[3 * i + 1] = qy;
    wq[3 * i + 2] = qz;
}

// candidates [i0, i1) from knn_outer.hip's table of their chunk (row i - i0)
__global__ __launch_bounds__(256) void pointing_table_kernel(int64_t i0, int64_t i1, int k, const int64_t* __restrict__ tidx,
                                                             const double* __restrict__ tdist, PtOut o) {
    const int64_t i = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= i1) return;
    const int64_t* row = tidx + (i - i0) * k;
    const double qx = o.wq[3 * i + 0], qy = o.wq[3 * i + 1], qz = o.wq[3 * i + 2];
    pt_finish<0>(o, i, k, tdist[(i - i0) * k], qx, qy, qz, [&](int j) { return (int)row[j]; });
}

// kept candidates to their slots, in the candidates' order; thread m: the count
__global__ __launch_bounds__(256) void pointing_scatter_kernel(int64_t m, const uint8_t* __restrict__ keep, const int* __restrict__ scan,
                                                               const double* __restrict__ wq, const double* __restrict__ wp,
                                                               int64_t candidate0, double* __restrict__ points,
                                                               double* __restrict__ pointing, int64_t* __restrict__ candidate,
                                                               int64_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == m) count[0] = scan[m];
    if (i >= m || !keep[i]) return;
    const int64_t s = scan[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        points[3 * s + c] = wq[3 * i + c];
        pointing[3 * s + c] = wp[3 * i + c];
    }
    candidate[s] = candidate0 + i;
}

template <int K>
static int launch_pointing_search_k(int k, unsigned blocks, hipStream_t st, const PtGeom& g, const int64_t* voxels, const double* jitter,
                                    int64_t m, int64_t n, const GridWs& w, int early, double hi2, const PtOut& o) {
    if constexpr (K > 1) {
        if (k != K) return launch_pointing_search_k<K - 1>(k, blocks, st, g, voxels, jitter, m, n, w, early, hi2, o);
    }
    hipLaunchKernelGGL(pointing_search_kernel<K>, dim3(blocks), dim3(256), 0, st, g, voxels, jitter, m, n, w.params, w.start, w.sx, w.sy,
                       w.sz, w.sidx, early, hi2, o);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

static int launch_pointing_brute(const PtGeom& g, const int64_t* voxels, const double* jitter, int64_t m, int64_t n, int k, const PtWs& w,
                                 const PtOut& o, hipStream_t st) {
    for (int64_t i0 = 0; i0 < m; i0 += PT_BRUTE_CHUNK) {
        const int64_t i1 = i0 + PT_BRUTE_CHUNK < m ? i0 + PT_BRUTE_CHUNK : m;
        const unsigned blocks = (unsigned)((i1 - i0 + 255) / 256);
        hipLaunchKernelGGL(pointing_queries_kernel, dim3(blocks), dim3(256), 0, st, g, voxels, jitter, i0, i1, w.wq);
        SAPCU_CHECK_LAUNCH();
        const int rc = launch_knn_outer(w.p64, n, w.wq + 3 * i0, i1 - i0, k, w.bidx, w.bdist, nullptr, st);
        if (rc != SAPCU_OK) return rc;
        hipLaunchKernelGGL(pointing_table_kernel, dim3(blocks), dim3(256), 0, st, i0, i1, k, w.bidx, w.bdist, o);
        SAPCU_CHECK_LAUNCH();
    }
    return SAPCU_OK;
}

int launch_pointing_samples(const float* surface, int64_t n, const int64_t* voxels, int64_t nv, const PtGeom& g, const double* jitter, int k,
                            double lo, double hi, double cell_size, int64_t candidate0, uint8_t* keep, double* d1, int32_t* idx,
                            double* points, double* pointing, int64_t* candidate, int64_t* count, void* ws, int64_t* info,
                            hipStream_t st) {
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (nv == 0) return SAPCU_OK;
    const int64_t m = nv * g.sub3;
    const PtWs w = pt_ws_layout(ws, n, m, k);
    const PtOut o{surface, lo, hi, keep, d1, idx, w.flags, w.wq, w.wp};
    hipLaunchKernelGGL(pointing_widen_kernel, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, st, surface, 3 * n, w.p64);
    SAPCU_CHECK_LAUNCH();
    SAPCU_CHECK_HIP(hipMemsetAsync(w.flags + m, 0, sizeof(int), st));    // the scan's last entry: the total
    bool brute = cell_size == 0.0 && n < KNN_GRID_MIN_N;
    int rc;
    if (!brute) {
        GridParams hp;
        rc = launch_grid_setup(w.p64, n, PT_CELL_POP, cell_size, w.grid, &hp, st);
        if (rc != SAPCU_OK) return rc;
        brute = hp.fallback != 0;
        if (!brute) {
            if (info) {
                info[0] = 1;
                info[1] = hp.gx;
                info[2] = hp.gy;
                info[3] = hp.gz;
            }
            rc = launch_grid_sort(w.p64, n, w.grid, hp, st);
            if (rc != SAPCU_OK) return rc;
            const int early = !d1 && !idx;
            const double hi2 = hi >= 0.0 ? hi * hi : -1.0;               // band_hi < 0 keeps nothing: every bound clears it
            rc = launch_pointing_search_k<PT_MAX_K>(k, (unsigned)((m + 255) / 256), st, g, voxels, jitter, m, n, w.grid, early, hi2, o);
            if (rc != SAPCU_OK) return rc;
        }
    }
    if (brute) {
        rc = launch_pointing_brute(g, voxels, jitter, m, n, k, w, o, st);
        if (rc != SAPCU_OK) return rc;
    }
    rc = launch_exclusive_scan_int(w.flags, m + 1, w.tile_sums, st);
    if (rc != SAPCU_OK) return rc;
    hipLaunchKernelGGL(pointing_scatter_kernel, dim3((unsigned)((m + 1 + 255) / 256)), dim3(256), 0, st, m, keep, w.flags, w.wq, w.wp,
                       candidate0, points, pointing, candidate, count);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

static bool pt_sizes_ok(int64_t n, int64_t nv, int sub, int k) {
    if (n < 1 || n > (1LL << 29) || nv < 0 || sub < 1 || sub > 1024 || k < 1 || k > PT_MAX_K) return false;
    const int64_t sub3 = (int64_t)sub * sub * sub;
    return nv <= ((1LL << 31) - 64) / sub3;
}

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

static bool pt_finite(double v) { return v - v == 0.0; }

extern "C" {

int64_t sapcu_pointing_workspace_bytes(int64_t n, int64_t nv, int sub, int k) {
    if (!pt_sizes_ok(n, nv, sub, k)) return -1;
    return (int64_t)pt_ws_layout(nullptr, n, nv * sub * sub * sub, k).bytes;
}

int sapcu_pointing_samples_f32(const float* surface, int64_t n, const int64_t* voxels, int64_t nv, double origin, double step, int count,
                               int sub, double step2, double half2, const double* jitter, int k, double band_lo, double band_hi,
                               double cell_size, int64_t candidate0, uint8_t* keep_out, double* d1_out, int32_t* idx_out,
                               double* points_out, double* pointing_out, int64_t* candidate_out, int64_t* count_out, void* workspace,
                               int64_t workspace_bytes, int64_t* info_host, void* stream) {
    SAPCU_CHECK_ARG(pt_sizes_ok(n, nv, sub, k),
                    "pointing_samples: need 1 <= n <= 2^29, nv >= 0, 1 <= sub <= 1024, nv * sub^3 <= 2^31 - 64, 1 <= k <= %d "
                    "(n=%lld nv=%lld sub=%d k=%d)", PT_MAX_K, (long long)n, (long long)nv, sub, k);
    SAPCU_CHECK_ARG(k <= n, "pointing_samples: need k <= n (n=%lld k=%d)", (long long)n, k);
    SAPCU_CHECK_ARG(count >= 1 && count <= (1 << 20), "pointing_samples: need 1 <= count <= 2^20 (count=%d)", count);
    SAPCU_CHECK_ARG(pt_finite(origin) && pt_finite(step) && pt_finite(step2) && pt_finite(half2),
                    "pointing_samples: origin, step, step2 and half2 must be finite");
    SAPCU_CHECK_ARG(band_lo == band_lo && band_hi == band_hi, "pointing_samples: a NaN band end");
    SAPCU_CHECK_ARG(cell_size >= 0.0 && cell_size < 1e300, "pointing_samples: cell_size must be finite and >= 0");
    SAPCU_CHECK_ARG(candidate0 >= 0, "pointing_samples: candidate0 must be >= 0");
    SAPCU_CHECK_ARG(surface && (nv == 0 || (voxels && keep_out && points_out && pointing_out && candidate_out && count_out)),
                    "pointing_samples: null pointer");                      // no voxel: nothing is written
    SAPCU_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "pointing_samples: the workspace must be 8-byte aligned (f64 tables)");
    const int sub3 = sub * sub * sub;
    const int64_t need = (int64_t)pt_ws_layout(nullptr, n, nv * sub3, k).bytes;
    SAPCU_CHECK_ARG(nv == 0 || (workspace && workspace_bytes >= need), "pointing_samples: workspace of %lld bytes, need %lld",
                    (long long)workspace_bytes, (long long)need);
    const PtGeom g{origin, step, step2, half2, count, sub, sub3};
    return launch_pointing_samples(surface, n, voxels, nv, g, jitter, k, band_lo, band_hi, cell_size, candidate0, keep_out, d1_out,
                                   idx_out, points_out, pointing_out, candidate_out, count_out, workspace, info_host,
                                   (hipStream_t)stream);
}

}  // extern "C"
