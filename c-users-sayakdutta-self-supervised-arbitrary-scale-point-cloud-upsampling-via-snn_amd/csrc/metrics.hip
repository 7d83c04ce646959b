// Exact nearest neighbour of every query in ANOTHER cloud on the cell grid of knn_grid.hip: the distance vectors behind Chamfer,
// Hausdorff, precision / recall and F-score (sapcu_amd/metrics.py).  Replaces the two sklearn NearestNeighbors(n_neighbors=1)
// queries per cloud pair of the reference's external/Meta-PU_evaluation/evaluation_code/evaluation_cd.py.
//
// nn_cross_kernel, one query per lane:
//   * the grid is built over the cloud by knn_grid.hip's launchers (bounding box, counting sort into the cell-ordered SoA copy);
//   * the queries are counting-sorted by the (clamped) cell of the CLOUD's grid they fall in, with the same launchers;
//   * a cell with c queries gets ceil(c / 64) wavefronts (knn_grid.h: launch_grid_query_waves scans those counts, grid_wave_chunk
//     finds wave w's (cell, chunk); the launch is grid_query_wave_bound, the waves beyond the total exit);
//   * all lanes of a wave share one cell, so grid_shell_walk (knn_grid.h), its ranges start[..] and its loop bounds are
//     wave-uniform.  A range is read 64 points at a time, coalesced, into the wave's own LDS slab; every point is then
//     read back by all lanes at once (one address: an LDS broadcast) and tested against each lane's own query.  A lane keeps
//     (best d, best index) in registers and compares on the key (d, index): candidates arrive in cell order;
//   * the squared distance is ((q-p)_x^2 + (q-p)_y^2) + (q-p)_z^2 in separately rounded f64 operations, the output sqrt_cr of it,
//     the lowest index among equal distances: bit for bit knn_outer.hip at k = 1;
//   * after shell r each lane evaluates the walk's stop rule for its own position against its own best; the wave leaves when
//     every lane is satisfied.  A lane that was satisfied earlier goes on computing: a minimum over more candidates is still
//     the minimum;
//   * the slack covers the queries as well: GridParams.slack is sized to the cloud's coordinates, and a query 1e6 extents outside
//     the box rounds q - face far above it.  nn_cross_setup_kernel adds 1e-11 * (largest |coordinate| of the queries' bounding box);
//   * results go to the queries' original positions with ordinary vector stores.  No float atomics, no scratch.
// Non-finite or huge (|x| > 1e150) coordinates in either set, and n < KNN_GRID_MIN_N with the automatic cell size, run the
// brute-force kernel of knn_outer.hip instead.
#include "common.h"
#include "knn_grid.h"
#include "../../include/sapcu_metrics.h"

namespace sapcu {

// automatic cell edge: emax * sqrt(2 * NN_CROSS_CELL_POP / n), about 2 * NN_CROSS_CELL_POP points in an occupied cell of a surface
// (profiles/metrics_nn.txt: the sweep over 8, 16, 32, 64)
constexpr int NN_CROSS_CELL_POP = 16;
constexpr int NN_CROSS_WAVES = 4;

struct CrossWs {
    GridWs g;                // the cloud's grid
    GridWs q;                // the queries in the cloud's cells (q.params = g.params; q.partials = their own bounding box)
    int* wstart;             // [cells + 1]: wavefronts per cell, then exclusive prefix sums
    int64_t* brute_idx;      // [nq] indices of the brute-force route when the caller wants none (shares q.sx: no grid then)
    size_t bytes;
};

static CrossWs cross_ws_layout(void* base, int64_t n, int64_t nq) {
    const int64_t cap = grid_cell_cap(n);
    CrossWs w;
    w.g = grid_ws_layout(base, n);
    WsCarver c(base ? (char*)base + w.g.bytes : nullptr);
    w.q = grid_query_ws_layout(c, cap, nq, w.g.params);
    w.wstart = c.take<int>(cap + 1);
    w.brute_idx = (int64_t*)w.q.sx;
    w.bytes = w.g.bytes + c.bytes();
    return w;
}

// one wavefront: the queries' bad flag and magnitude into the cloud's grid parameters
__global__ __launch_bounds__(64) void nn_cross_setup_kernel(const double* __restrict__ qpartials, GridParams* __restrict__ prm) {
    double amax, bad = 0.0;
    grid_partials_fold(qpartials, &amax, &bad);
    if (threadIdx.x != 0) return;
    if (bad != 0.0) {
        prm->fallback = 1;
        return;
    }
    prm->slack = __dadd_rn(prm->slack, __dmul_rn(1e-11, amax));
}

struct __align__(16) CrossPt {
    double x, y, z;
    int idx, pad;
};

struct CrossBest {
    double d;
    int i;
};

// every point of the sorted range [a, b) against every lane's query
__device__ __forceinline__ void cross_scan_range(CrossBest& B, int a, int b, double qx, double qy, double qz,
                                                 const double* __restrict__ sx, const double* __restrict__ sy,
                                                 const double* __restrict__ sz, const int* __restrict__ sidx, CrossPt* slab, int lane) {
    for (int off = a; off < b; off += 64) {
        const int j = off + lane;
        CrossPt mine{0.0, 0.0, 0.0, 0x7fffffff, 0};
        if (j < b) {
            mine.x = sx[j];
            mine.y = sy[j];
            mine.z = sz[j];
            mine.idx = sidx[j];
        }
        __builtin_amdgcn_wave_barrier();
        slab[lane] = mine;
        __builtin_amdgcn_wave_barrier();
        const int cnt = min(64, b - off);                                   // wave-uniform
#pragma unroll 4
        for (int t = 0; t < cnt; ++t) {
            const CrossPt p = slab[t];                                      // one address for the whole wave: a broadcast
            const double d = dist2_rn(qx, qy, qz, p.x, p.y, p.z);
            if (d < B.d || (d == B.d && p.idx < B.i)) {
                B.d = d;
                B.i = p.idx;
            }
        }
    }
}

__global__ __launch_bounds__(256) void nn_cross_kernel(const GridParams* __restrict__ prm, const int* __restrict__ start,
                                                       const double* __restrict__ sx, const double* __restrict__ sy,
                                                       const double* __restrict__ sz, const int* __restrict__ sidx,
                                                       const int* __restrict__ qstart, const int* __restrict__ wstart,
                                                       const double* __restrict__ qsx, const double* __restrict__ qsy,
                                                       const double* __restrict__ qsz, const int* __restrict__ qsidx, int cells,
                                                       double* __restrict__ dist_out, int64_t* __restrict__ idx_out) {
    __shared__ CrossPt slabs[NN_CROSS_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t w = (int64_t)blockIdx.x * NN_CROSS_WAVES + wave;
    int cell, qa, qb;
    if (!grid_wave_chunk(w, wstart, qstart, cells, &cell, &qa, &qb)) return;
    const bool valid = qa + lane < qb;
    const int j = valid ? qa + lane : qa;                                   // a spare lane repeats the chunk's first query
    const double qx = qsx[j], qy = qsy[j], qz = qsz[j];
    const GridParams p = *prm;
    const int cx = cell % p.gx, cy = (cell / p.gx) % p.gy, cz = cell / (p.gx * p.gy);
    const double INF = __builtin_huge_val();
    CrossBest B{INF, 0x7fffffff};
    CrossPt* slab = slabs[wave];
    grid_shell_walk(
        p, start, cx, cy, cz, qx, qy, qz, p.slack,
        [&](int a, int b) { cross_scan_range(B, a, b, qx, qy, qz, sx, sy, sz, sidx, slab, lane); },
        [&](double bnd) { return __ballot(!grid_bound_clears(bnd, B.d)) == 0ull; });       // every lane's bound clears its best
    if (valid) {
        const int o = qsidx[j];
        dist_out[o] = sqrt_cr(B.d);
        if (idx_out) idx_out[o] = B.i;
    }
}

int launch_nn_cross(const double* cloud, int64_t n, const double* queries, int64_t nq, double cell_size, double* dist, int64_t* idx,
                    void* ws, int64_t* info, hipStream_t st) {
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (nq == 0) return SAPCU_OK;
    const CrossWs w = cross_ws_layout(ws, n, nq);
    int64_t* bidx = idx ? idx : w.brute_idx;
    if (cell_size == 0.0 && n < KNN_GRID_MIN_N) return launch_knn_outer(cloud, n, queries, nq, 1, bidx, dist, nullptr, st);
    int rc = launch_grid_params(cloud, n, NN_CROSS_CELL_POP, cell_size, w.g, st);
    if (rc != SAPCU_OK) return rc;
    rc = launch_grid_bbox(queries, nq, w.q.partials, st);
    if (rc != SAPCU_OK) return rc;
    hipLaunchKernelGGL(nn_cross_setup_kernel, dim3(1), dim3(64), 0, st, w.q.partials, w.g.params);
    SAPCU_CHECK_LAUNCH();
    GridParams hp;
    SAPCU_CHECK_HIP(hipMemcpyAsync(&hp, w.g.params, sizeof(hp), hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    if (hp.fallback) return launch_knn_outer(cloud, n, queries, nq, 1, bidx, dist, nullptr, st);
    if (info) {
        info[0] = 1;
        info[1] = hp.gx;
        info[2] = hp.gy;
        info[3] = hp.gz;
    }
    rc = launch_grid_sort(cloud, n, w.g, hp, st);
    if (rc != SAPCU_OK) return rc;
    rc = launch_grid_sort(queries, nq, w.q, hp, st);                        // the cloud's parameters: the cloud's cells
    if (rc != SAPCU_OK) return rc;
    const int64_t cells = (int64_t)hp.gx * hp.gy * hp.gz;
    rc = launch_grid_query_waves(w.q.start, cells, w.wstart, w.q.tile_sums, st);
    if (rc != SAPCU_OK) return rc;
    const int64_t grid = (grid_query_wave_bound(nq, cells) + NN_CROSS_WAVES - 1) / NN_CROSS_WAVES;
    hipLaunchKernelGGL(nn_cross_kernel, dim3((unsigned)grid), dim3(256), 0, st, w.g.params, w.g.start, w.g.sx, w.g.sy, w.g.sz, w.g.sidx,
                       w.q.start, w.wstart, w.q.sx, w.q.sy, w.q.sz, w.q.sidx, (int)cells, dist, idx);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

extern "C" {

int64_t sapcu_nn_cross_workspace_bytes(int64_t n, int64_t nq) {
    if (n < 1 || n > (1LL << 29) || nq < 0 || nq > (1LL << 31) - 64) return -1;
    return (int64_t)cross_ws_layout(nullptr, n, nq).bytes;
}

int sapcu_nn_cross_grid_f64(const double* cloud, int64_t n, const double* queries, int64_t nq, double cell_size, double* dist_out,
                            int64_t* idx_out, void* workspace, int64_t workspace_bytes, int64_t* info_host, void* stream) {
    SAPCU_CHECK_ARG(n >= 1 && n <= (1LL << 29), "nn_cross_grid: need 1 <= n <= 2^29 (n=%lld)", (long long)n);
    SAPCU_CHECK_ARG(nq >= 0 && nq <= (1LL << 31) - 64, "nn_cross_grid: need 0 <= nq <= 2^31 - 64 (nq=%lld)", (long long)nq);
    SAPCU_CHECK_ARG(cloud && ((queries && dist_out) || nq == 0), "nn_cross_grid: null pointer");      // no query: nothing is written
    SAPCU_CHECK_ARG(cell_size >= 0.0 && cell_size < 1e300, "nn_cross_grid: cell_size must be finite and >= 0");
    SAPCU_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "nn_cross_grid: the workspace must be 8-byte aligned (f64 tables)");
    const int64_t need = (int64_t)cross_ws_layout(nullptr, n, nq).bytes;
    SAPCU_CHECK_ARG(workspace && workspace_bytes >= need, "nn_cross_grid: workspace of %lld bytes, need %lld",
                    (long long)workspace_bytes, (long long)need);
    return launch_nn_cross(cloud, n, queries, nq, cell_size, dist_out, idx_out, workspace, info_host, (hipStream_t)stream);
}

}  // extern "C"
