// Exact kNN of a point set against itself on a uniform cell grid, and the outlier filter's statistics in numpy's
// summation order.  Replaces the brute-force kNN-30 + the two np.mean of the reference's generation.py:176-183.
//
// kNN (knn_self_grid_kernel):
//   * the grid is built on the device: bounding box (block partials, one finishing thread), cell keys
//     key = (cz*gy + cy)*gx + cx with c = floor((p - origin) / h) clamped to the grid, counting sort (integer atomics
//     for the counts, a three-kernel exclusive scan, integer atomics for the slots) into a cell-ordered SoA copy
//     x|y|z plus the original indices.  The order inside a cell is arbitrary: the (distance, index) keys decide;
//   * one query per wavefront (4 per 256-thread workgroup).  The running top-k is the keyed WaveTopK of wave_ops.h, a sorted
//     list spread over the lanes (entry p in lane p, k <= 64); candidates arrive in cell order, not index order, so
//     a candidate is compared on the key (d, i) — a point at the k-th distance with a lower index still enters;
//   * the search is grid_shell_walk (knn_grid.h: the shells, the lower bound after each and the stop rule), with GridParams.slack
//     as the margin, against the current k-th squared distance;
//   * the squared distance is ((q-p)_x^2 + (q-p)_y^2) + (q-p)_z^2 in separately rounded f64 operations, the output
//     distance sqrt_cr of it (dist2_rn): bit for bit the arithmetic and the order of knn_outer.hip;
//   * non-finite or huge (|x| > 1e150) coordinates, and n < KNN_GRID_MIN_N with the automatic cell size, run the
//     brute-force kernel of knn_outer.hip instead (the launcher reads the grid parameters back: one stream sync).
//
// Statistics (outlier_stats_kernel, outlier_keep_kernel): numpy 2.x np.mean of a C-contiguous f64 [n,kk] table —
//   * the row mean is the pairwise leaf of kk <= 128 values (np_leaf_sum, wave_ops.h) over kk;
//   * the global sum is the flattened table cut into chunks of `bufsize` elements (np.getbufsize()), each summed by
//     numpy's recursive pairwise sum (wave_ops.h: plan, leaves, fold); the chunk sums are added in sequence from 0.0 by
//     the caller (sapcu_amd/generation.py), since they may come from several ranks.
#include "common.h"
#include "knn_grid.h"

namespace sapcu {

// ------------------------------------------------------------------------------------------------------ grid build
__global__ __launch_bounds__(256) void grid_bbox_kernel(const double* __restrict__ pts, int64_t n, double* __restrict__ partials) {
    const double INF = __builtin_huge_val();
    double lx = INF, ly = INF, lz = INF, hx = -INF, hy = -INF, hz = -INF, bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double x = pts[i * 3 + 0], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
        if (!(fabs(x) <= 1e150 && fabs(y) <= 1e150 && fabs(z) <= 1e150)) bad = 1.0;    // NaN, inf, or a square that could overflow
        lx = fmin(lx, x);
        ly = fmin(ly, y);
        lz = fmin(lz, z);
        hx = fmax(hx, x);
        hy = fmax(hy, y);
        hz = fmax(hz, z);
    }
    lx = wave_min(lx);
    ly = wave_min(ly);
    lz = wave_min(lz);
    hx = wave_max(hx);
    hy = wave_max(hy);
    hz = wave_max(hz);
    bad = wave_max(bad);
    __shared__ double red[4][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave][0] = lx;
        red[wave][1] = ly;
        red[wave][2] = lz;
        red[wave][3] = hx;
        red[wave][4] = hy;
        red[wave][5] = hz;
        red[wave][6] = bad;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int c = threadIdx.x;
        double v = red[0][c];
        for (int w = 1; w < 4; ++w) v = c < 3 ? fmin(v, red[w][c]) : fmax(v, red[w][c]);
        partials[blockIdx.x * 8 + c] = v;
    }
}

// one thread: the bounding box, the cell edge (given or automatic) and the grid dimensions, at most `cap` cells
__global__ void grid_setup_kernel(const double* __restrict__ partials, int k, int64_t n, double cell_size, int64_t cap,
                                  GridParams* __restrict__ prm) {
    if (threadIdx.x != 0) return;
    const double INF = __builtin_huge_val();
    double lx = INF, ly = INF, lz = INF, hx = -INF, hy = -INF, hz = -INF, bad = 0.0;
    for (int b = 0; b < KNN_GRID_BBOX_BLOCKS; ++b) {
        const double* q = partials + b * 8;
        lx = fmin(lx, q[0]);
        ly = fmin(ly, q[1]);
        lz = fmin(lz, q[2]);
        hx = fmax(hx, q[3]);
        hy = fmax(hy, q[4]);
        hz = fmax(hz, q[5]);
        bad = fmax(bad, q[6]);
    }
    GridParams p;
    p.fallback = bad != 0.0;
    p.ox = lx;
    p.oy = ly;
    p.oz = lz;
    p.gx = p.gy = p.gz = 1;
    p.h = 1.0;
    p.slack = 0.0;
    if (!p.fallback) {
        const double ex = hx - lx, ey = hy - ly, ez = hz - lz;
        const double emax = fmax(ex, fmax(ey, ez));
        // surfaces: about 2k points per cell face of (longest extent)^2 / n — the k nearest then mostly lie in shell 1
        double h = cell_size > 0.0 ? cell_size : emax * sqrt(2.0 * k / (double)n);
        if (!(emax > 0.0)) h = 1.0;                                  // every point equal: one cell
        h = fmax(h, emax * 1e-9);                                    // floor(extent / h) stays far inside int range
        double gx, gy, gz;
        for (;;) {
            gx = floor(ex / h) + 1.0;
            gy = floor(ey / h) + 1.0;
            gz = floor(ez / h) + 1.0;
            if (gx * gy * gz <= (double)cap) break;
            h *= 1.125;
        }
        p.h = h;
        p.gx = (int)gx;
        p.gy = (int)gy;
        p.gz = (int)gz;
        const double amax = fmax(fmax(fmax(fabs(lx), fabs(hx)), fmax(fabs(ly), fabs(hy))), fmax(fabs(lz), fabs(hz)));
        p.slack = 1e-11 * (amax + emax + h);
    }
    *prm = p;
}

__global__ __launch_bounds__(256) void grid_count_kernel(const double* __restrict__ pts, int64_t n, const GridParams* __restrict__ prm,
                                                         int* __restrict__ count, int* __restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const GridParams p = *prm;
    const int cx = grid_coord(pts[i * 3 + 0], p.ox, p.h, p.gx);
    const int cy = grid_coord(pts[i * 3 + 1], p.oy, p.h, p.gy);
    const int cz = grid_coord(pts[i * 3 + 2], p.oz, p.h, p.gz);
    const int c = (cz * p.gy + cy) * p.gx + cx;
    key[i] = c;
    atomicAdd(&count[c], 1);
}

// exclusive scan of the int counts in tiles of SCAN_TILE: per-tile sums, a one-workgroup scan of those, per-tile apply
__global__ __launch_bounds__(256) void scan_tile_sum_kernel(const int* __restrict__ a, int64_t m, int* __restrict__ tile_sums) {
    __shared__ int red4[4];
    const int64_t b = (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x * 4;
    int s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (b + j < m) s += a[b + j];
    int total;
    block_excl_scan<4>(s, red4, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void scan_tile_offsets_kernel(int* __restrict__ tile_sums, int64_t tiles) {
    __shared__ int red4[4];
    int carry = 0;
    for (int64_t base = 0; base < tiles; base += 256) {
        const int64_t t = base + threadIdx.x;
        const int v = t < tiles ? tile_sums[t] : 0;
        int total;
        const int ex = block_excl_scan<4>(v, red4, &total);
        if (t < tiles) tile_sums[t] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(256) void scan_apply_kernel(int* __restrict__ a, int64_t m, const int* __restrict__ tile_off) {
    __shared__ int red4[4];
    const int64_t b = (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x * 4;
    int v0 = b + 0 < m ? a[b + 0] : 0;
    int v1 = b + 1 < m ? a[b + 1] : 0;
    int v2 = b + 2 < m ? a[b + 2] : 0;
    int v3 = b + 3 < m ? a[b + 3] : 0;
    int total;
    const int run = block_excl_scan<4>(v0 + v1 + v2 + v3, red4, &total) + tile_off[blockIdx.x];
    if (b + 0 < m) a[b + 0] = run;
    if (b + 1 < m) a[b + 1] = run + v0;
    if (b + 2 < m) a[b + 2] = run + v0 + v1;
    if (b + 3 < m) a[b + 3] = run + v0 + v1 + v2;
}

__global__ __launch_bounds__(256) void grid_scatter_kernel(const double* __restrict__ pts, int64_t n, const int* __restrict__ key,
                                                           int* __restrict__ cursor, double* __restrict__ sx, double* __restrict__ sy,
                                                           double* __restrict__ sz, int* __restrict__ sidx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int slot = atomicAdd(&cursor[key[i]], 1);
    sx[slot] = pts[i * 3 + 0];
    sy[slot] = pts[i * 3 + 1];
    sz[slot] = pts[i * 3 + 2];
    sidx[slot] = (int)i;
}

// --------------------------------------------------------------------------------------------------------- search
// every point of the sorted range [a, b) against the list
__device__ __forceinline__ void grid_scan_range(WaveTopK<false, true>& L, int a, int b, double qx, double qy, double qz,
                                                const double* __restrict__ sx, const double* __restrict__ sy,
                                                const double* __restrict__ sz, const int* __restrict__ sidx, int lane) {
    for (int off = a; off < b; off += 64) {
        const int j = off + lane;
        double d = __builtin_huge_val();
        int pi = 0x7fffffff;
        if (j < b) {
            d = dist2_rn(qx, qy, qz, sx[j], sy[j], sz[j]);
            pi = sidx[j];
        }
        L.offer(d, pi);
    }
}

__global__ __launch_bounds__(256) void knn_self_grid_kernel(const double* __restrict__ pts, int64_t row0, int64_t row1, int k,
                                                            const GridParams* __restrict__ prm, const int* __restrict__ start,
                                                            const double* __restrict__ sx, const double* __restrict__ sy,
                                                            const double* __restrict__ sz, const int* __restrict__ sidx,
                                                            int64_t* __restrict__ idx_out, double* __restrict__ dist_out) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = row0 + (int64_t)blockIdx.x * KNN_GRID_WAVES + (threadIdx.x >> 6);
    if (qi >= row1) return;                                            // wave-uniform
    const GridParams p = *prm;
    const double qx = pts[qi * 3 + 0], qy = pts[qi * 3 + 1], qz = pts[qi * 3 + 2];
    const int cx = grid_coord(qx, p.ox, p.h, p.gx);
    const int cy = grid_coord(qy, p.oy, p.h, p.gy);
    const int cz = grid_coord(qz, p.oz, p.h, p.gz);
    WaveTopK<false, true> L(k);
    grid_shell_walk(
        p, start, cx, cy, cz, qx, qy, qz, p.slack,
        [&](int a, int b) { grid_scan_range(L, a, b, qx, qy, qz, sx, sy, sz, sidx, lane); },
        [&](double bnd) { return grid_bound_clears(bnd, L.tau); });                      // against the k-th squared distance
    if (lane < k) {
        const int64_t o = (qi - row0) * k + lane;
        idx_out[o] = L.i[0];
        dist_out[o] = sqrt_cr(L.d[0]);
    }
}

// exclusive scan of a[0..m) in place; tile_sums: ceil(m / SCAN_TILE) ints of scratch
int launch_exclusive_scan_int(int* a, int64_t m, int* tile_sums, hipStream_t st) {
    if (m <= 0) return SAPCU_OK;
    const int64_t tiles = (m + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL(scan_tile_sum_kernel, dim3((unsigned)tiles), dim3(256), 0, st, a, m, tile_sums);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_tile_offsets_kernel, dim3(1), dim3(256), 0, st, tile_sums, tiles);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)tiles), dim3(256), 0, st, a, m, tile_sums);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

// the bounding-box partials of any point array: [KNN_GRID_BBOX_BLOCKS][8] = min xyz, max xyz, bad flag
int launch_grid_bbox(const double* pts, int64_t n, double* partials, hipStream_t st) {
    hipLaunchKernelGGL(grid_bbox_kernel, dim3(KNN_GRID_BBOX_BLOCKS), dim3(256), 0, st, pts, n, partials);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

// the grid's parameters on the device only (w.params), nothing read back
int launch_grid_params(const double* pts, int64_t n, int k, double cell_size, const GridWs& w, hipStream_t st) {
    const int rc = launch_grid_bbox(pts, n, w.partials, st);
    if (rc != SAPCU_OK) return rc;
    hipLaunchKernelGGL(grid_setup_kernel, dim3(1), dim3(64), 0, st, w.partials, k, n, cell_size, grid_cell_cap(n), w.params);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

// the grid's parameters on the device and in *hp (one stream sync); hp->fallback: nothing else may be built
int launch_grid_setup(const double* pts, int64_t n, int k, double cell_size, const GridWs& w, GridParams* hp, hipStream_t st) {
    const int rc = launch_grid_params(pts, n, k, cell_size, w, st);
    if (rc != SAPCU_OK) return rc;
    SAPCU_CHECK_HIP(hipMemcpyAsync(hp, w.params, sizeof(*hp), hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    return SAPCU_OK;
}

// counting sort of the points into the cell-ordered copy w.sx|sy|sz|sidx, w.start = first sorted slot of each cell
int launch_grid_sort(const double* pts, int64_t n, const GridWs& w, const GridParams& hp, hipStream_t st) {
    const int64_t cells = (int64_t)hp.gx * hp.gy * hp.gz;
    const int64_t m = cells + 1;
    const unsigned nb = (unsigned)((n + 255) / 256);
    SAPCU_CHECK_HIP(hipMemsetAsync(w.start, 0, sizeof(int) * m, st));
    hipLaunchKernelGGL(grid_count_kernel, dim3(nb), dim3(256), 0, st, pts, n, w.params, w.start, w.key);
    SAPCU_CHECK_LAUNCH();
    const int rc = launch_exclusive_scan_int(w.start, m, w.tile_sums, st);
    if (rc != SAPCU_OK) return rc;
    SAPCU_CHECK_HIP(hipMemcpyAsync(w.cursor, w.start, sizeof(int) * cells, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(grid_scatter_kernel, dim3(nb), dim3(256), 0, st, pts, n, w.key, w.cursor, w.sx, w.sy, w.sz, w.sidx);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

// wavefronts per cell: ceil(queries / 64); entry `cells` (the scan's total) starts at 0
__global__ __launch_bounds__(256) void grid_query_waves_kernel(const int* __restrict__ qstart, int64_t cells, int* __restrict__ wstart) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > cells) return;
    wstart[c] = c < cells ? (qstart[c + 1] - qstart[c] + 63) >> 6 : 0;
}

int launch_grid_query_waves(const int* qstart, int64_t cells, int* wstart, int* tile_sums, hipStream_t st) {
    hipLaunchKernelGGL(grid_query_waves_kernel, dim3((unsigned)((cells + 1 + 255) / 256)), dim3(256), 0, st, qstart, cells, wstart);
    SAPCU_CHECK_LAUNCH();
    return launch_exclusive_scan_int(wstart, cells + 1, tile_sums, st);
}

int launch_knn_self_grid(const double* pts, int64_t n, int64_t row0, int64_t row1, int k, double cell_size, int64_t* idx,
                         double* dist, void* ws, int64_t ws_bytes, int64_t* info, hipStream_t st) {
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    const int64_t rows = row1 - row0;
    if (rows == 0) return SAPCU_OK;
    if (cell_size == 0.0 && n < KNN_GRID_MIN_N)
        return launch_knn_outer(pts, n, pts + row0 * 3, rows, k, idx, dist, nullptr, st);
    GridWs w = grid_ws_layout(ws, n);
    SAPCU_CHECK_ARG(ws && (int64_t)w.bytes <= ws_bytes, "knn_self_grid: workspace of %lld bytes, need %lld",
                    (long long)ws_bytes, (long long)w.bytes);
    GridParams hp;
    int rc = launch_grid_setup(pts, n, k, cell_size, w, &hp, st);
    if (rc != SAPCU_OK) return rc;
    if (hp.fallback)
        return launch_knn_outer(pts, n, pts + row0 * 3, rows, k, idx, dist, nullptr, st);
    if (info) {
        info[0] = 1;
        info[1] = hp.gx;
        info[2] = hp.gy;
        info[3] = hp.gz;
    }
    rc = launch_grid_sort(pts, n, w, hp, st);
    if (rc != SAPCU_OK) return rc;
    const int64_t grid = (rows + KNN_GRID_WAVES - 1) / KNN_GRID_WAVES;
    hipLaunchKernelGGL(knn_self_grid_kernel, dim3((unsigned)grid), dim3(256), 0, st, pts, row0, row1, k, w.params, w.start,
                       w.sx, w.sy, w.sz, w.sidx, idx, dist);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

// ----------------------------------------------------------------------------------------------------- statistics
// 64-thread workgroups.  Blocks [0, nchunks): the pairwise sum of one `bufsize`-element chunk of the flattened table (lane 0
// lays the leaves out in LDS, the lanes sum them, lane 0 folds them back up the tree with an LDS stack); the blocks after
// those: the row means, one row per thread.
__global__ __launch_bounds__(64) void outlier_stats_kernel(const double* __restrict__ dist, int64_t rows, int kk, int64_t bufsize,
                                                          int64_t nchunks, double* __restrict__ row_mean, double* __restrict__ chunk_sum) {
    if ((int64_t)blockIdx.x >= nchunks) {
        const int64_t r = ((int64_t)blockIdx.x - nchunks) * 64 + threadIdx.x;
        if (r < rows) row_mean[r] = __ddiv_rn(np_leaf_sum(dist + r * kk, kk), (double)kk);
        return;
    }
    __shared__ int leaf_o[STATS_MAX_LEAVES], leaf_l[STATS_MAX_LEAVES];
    __shared__ double leaf_s[STATS_MAX_LEAVES];
    __shared__ int st_o[64], st_l[64], st_e[64];
    __shared__ double vs[64];
    __shared__ int nleaves;
    const int64_t total = rows * (int64_t)kk;
    const int64_t c0 = (int64_t)blockIdx.x * bufsize;
    const int len = (int)((total - c0) < bufsize ? (total - c0) : bufsize);
    const double* a = dist + c0;
    if (threadIdx.x == 0) nleaves = np_pairwise_plan<STATS_MAX_LEAVES>(len, leaf_o, leaf_l, st_o, st_l);
    __syncthreads();
    const int nl = nleaves;
    for (int j = threadIdx.x; j < nl; j += 64) leaf_s[j] = np_leaf_sum(a + leaf_o[j], leaf_l[j]);
    __syncthreads();
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = np_pairwise_fold<double, STATS_MAX_LEAVES>(len, leaf_s, st_l, st_e, vs);
}

__global__ __launch_bounds__(256) void outlier_keep_kernel(const double* __restrict__ row_mean, int64_t rows, double mean,
                                                           double threshold, uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    keep[i] = row_mean[i] < __dmul_rn(mean, threshold) ? 1 : 0;
}

int launch_outlier_stats(const double* dist, int64_t rows, int kk, int64_t bufsize, double* row_mean, double* chunk_sum,
                         hipStream_t st) {
    if (rows == 0) return SAPCU_OK;
    const int64_t nchunks = (rows * kk + bufsize - 1) / bufsize;
    const int64_t rblocks = (rows + 63) / 64;
    hipLaunchKernelGGL(outlier_stats_kernel, dim3((unsigned)(nchunks + rblocks)), dim3(64), 0, st, dist, rows, kk, bufsize, nchunks,
                       row_mean, chunk_sum);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int launch_outlier_keep(const double* row_mean, int64_t rows, double mean, double threshold, uint8_t* keep, hipStream_t st) {
    if (rows == 0) return SAPCU_OK;
    hipLaunchKernelGGL(outlier_keep_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, row_mean, rows, mean, threshold,
                       keep);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

extern "C" {

int64_t sapcu_knn_grid_workspace_bytes(int64_t n) { return n < 1 ? -1 : (int64_t)grid_ws_layout(nullptr, n).bytes; }

int sapcu_knn_self_grid_f64(const double* pts, int64_t n, int64_t row0, int64_t row1, int k, double cell_size, int64_t* idx_out,
                            double* dist_out, void* workspace, int64_t workspace_bytes, int64_t* info_host, void* stream) {
    SAPCU_CHECK_ARG(pts && ((idx_out && dist_out) || row1 == row0), "knn_self_grid: null pointer");     // an empty range writes nothing
    SAPCU_CHECK_ARG(n >= 1 && n <= (1LL << 29), "knn_self_grid: need 1 <= n <= 2^29 (n=%lld)", (long long)n);
    SAPCU_CHECK_ARG(k >= 1 && k <= 64 && k <= n, "knn_self_grid: need 1 <= k <= min(64, n) (n=%lld k=%d)", (long long)n, k);
    SAPCU_CHECK_ARG(0 <= row0 && row0 <= row1 && row1 <= n, "knn_self_grid: bad row range [%lld, %lld) of %lld",
                    (long long)row0, (long long)row1, (long long)n);
    SAPCU_CHECK_ARG(cell_size >= 0.0 && cell_size < 1e300, "knn_self_grid: cell_size must be finite and >= 0");
    SAPCU_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "knn_self_grid: the workspace must be 8-byte aligned (f64 tables)");
    return launch_knn_self_grid(pts, n, row0, row1, k, cell_size, idx_out, dist_out, workspace, workspace_bytes, info_host,
                                (hipStream_t)stream);
}

int sapcu_outlier_stats_f64(const double* dist, int64_t rows, int kk, int64_t bufsize, double* row_mean_out, double* chunk_sum_out,
                            void* stream) {
    SAPCU_CHECK_ARG(rows >= 0 && kk >= 1 && kk <= 128, "outlier_stats: need rows >= 0 and 1 <= kk <= 128");
    SAPCU_CHECK_ARG(bufsize >= 1 && bufsize <= STATS_MAX_BUFSIZE, "outlier_stats: bufsize must be in 1..%lld (got %lld)",
                    (long long)STATS_MAX_BUFSIZE, (long long)bufsize);
    SAPCU_CHECK_ARG(rows == 0 || (dist && row_mean_out && chunk_sum_out), "outlier_stats: null pointer");
    return launch_outlier_stats(dist, rows, kk, bufsize, row_mean_out, chunk_sum_out, (hipStream_t)stream);
}

int sapcu_outlier_keep_f64(const double* row_mean, int64_t rows, double mean, double threshold, uint8_t* keep_out, void* stream) {
    SAPCU_CHECK_ARG(rows >= 0 && (rows == 0 || (row_mean && keep_out)), "outlier_keep: bad argument");
    return launch_outlier_keep(row_mean, rows, mean, threshold, keep_out, (hipStream_t)stream);
}

}  // extern "C"
