// The device cell grid of knn_grid.hip, for the translation units that search it: parameters, workspace layout, the build, the
// int exclusive scan, and what every search on the grid shares — the Chebyshev shell walk with its stop rule (grid_shell_walk), the
// table of queries counted into another set's grid (grid_query_ws_layout .. grid_wave_chunk) and the fold of bounding-box partials
// (grid_partials_fold).  Kernels live in knn_grid.hip; a kernel is launched from the file that defines it.
#pragma once
#include "common.h"
#include "wave_ops.h"

namespace sapcu {

constexpr int KNN_GRID_WAVES = 4;
constexpr int KNN_GRID_BBOX_BLOCKS = 256;
constexpr int64_t KNN_GRID_MIN_N = 4096;     // below this (automatic cell size) the brute force costs less than a grid build
constexpr int SCAN_TILE = 1024;              // 256 threads x 4 counts
constexpr int STATS_MAX_LEAVES = 512;        // a chunk of <= STATS_MAX_BUFSIZE elements has <= 129 pairwise leaves
constexpr int64_t STATS_MAX_BUFSIZE = 16384;

struct GridParams {
    double ox, oy, oz;       // origin = bounding-box minimum
    double h;                // cell edge
    double slack;            // absolute margin on the face distances (>> the rounding of keys and faces)
    int gx, gy, gz;
    int fallback;            // 1: brute force (non-finite / huge coordinates)
};

static inline int64_t grid_cell_cap(int64_t n) { return 2 * n + 64; }

struct GridWs {
    double* partials;        // [KNN_GRID_BBOX_BLOCKS][8]: min xyz, max xyz, bad flag
    GridParams* params;
    int* start;              // [cells + 1]: counts, then exclusive prefix sums
    int* cursor;             // [cells]
    int* tile_sums;          // [ceil((cells + 1) / SCAN_TILE)]
    int* key;                // [n]
    double* sx;              // [n] each, cell order
    double* sy;
    double* sz;
    int* sidx;               // [n] original index of each sorted point
    size_t bytes;            // what the layout call that made this table carved (grid_ws_layout: the parameter block included)
};

// the table of nq queries counted into ANOTHER set's grid of at most `cap` cells, whose parameters it shares (partials: the queries'
// own bounding box): everything launch_grid_sort writes
static GridWs grid_query_ws_layout(WsCarver& c, int64_t cap, int64_t nq, GridParams* params) {
    const size_t before = c.bytes();
    GridWs w;
    w.partials = c.take<double>(8 * KNN_GRID_BBOX_BLOCKS);
    w.params = params;
    w.start = c.take<int>(cap + 1);
    w.cursor = c.take<int>(cap);
    w.tile_sums = c.take<int>((cap + 1 + SCAN_TILE - 1) / SCAN_TILE);
    w.key = c.take<int>(nq);
    w.sx = c.take<double>(nq);
    w.sy = c.take<double>(nq);
    w.sz = c.take<double>(nq);
    w.sidx = c.take<int>(nq);
    w.bytes = c.bytes() - before;
    return w;
}

// the grid over n points: its parameter block and the points' own table
static GridWs grid_ws_layout(void* base, int64_t n) {
    WsCarver c(base);
    GridParams* params = c.take<GridParams>(1);
    GridWs w = grid_query_ws_layout(c, grid_cell_cap(n), n, params);
    w.bytes = c.bytes();
    return w;
}

// launch bound of a search that gives a cell with c queries ceil(c / 64) wavefronts: >= the sum over the cells, nothing is read back
static inline int64_t grid_query_wave_bound(int64_t nq, int64_t cells) { return (nq + 63) / 64 + (cells < nq ? cells : nq); }

__device__ __forceinline__ int grid_coord(double v, double o, double h, int g) {
    const double t = floor(__ddiv_rn(__dsub_rn(v, o), h));
    return t < 0.0 ? 0 : (t >= (double)(g - 1) ? g - 1 : (int)t);
}

// wavefront w of such a search: its cell and its chunk [qa, qb) of the queries sorted into that cell (at most 64 of them are the
// wave's: qa + lane < qb).  wstart is launch_grid_query_waves' scan, searched for wstart[cell] <= w < wstart[cell + 1]; false for
// a wave beyond the last (cell, chunk).  Wave-uniform.
__device__ __forceinline__ bool grid_wave_chunk(int64_t w, const int* __restrict__ wstart, const int* __restrict__ qstart, int cells,
                                                int* cell, int* qa, int* qb) {
    if (w >= (int64_t)wstart[cells]) return false;
    int lo = 0, hi = cells;                                                 // wstart[lo] <= w < wstart[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)wstart[mid] <= w) lo = mid; else hi = mid;
    }
    *cell = lo;
    *qa = qstart[lo] + ((int)w - wstart[lo]) * 64;
    *qb = qstart[lo + 1];
    return true;
}

// The stop rule's comparison: the lower bound `bnd` on the distance of everything unvisited (margins already taken off) is
// positive and its square, shrunk by 1 - 1e-9 for what is relative in the rounding of the distances, is STRICTLY above `best` — a
// candidate whose rounded squared distance ties `best` cannot be skipped.
__device__ __forceinline__ bool grid_bound_clears(double bnd, double best) {
    return bnd > 0.0 && __dmul_rn(__dmul_rn(bnd, bnd), 1.0 - 1e-9) > best;
}

// The search around a query at q whose (clamped) cell is (cx, cy, cz): Chebyshev shells r = 0, 1, 2, ... of cells.  A shell row whose
// y or z offset is +-r is ONE contiguous range of the sorted points (the cells of a row are consecutive keys); the other rows
// contribute their two end cells.  scan(a, b) gets every sorted range [a, b) of shell r.  After shell r the distance from q to the
// faces of the visited block [c-r, c+r]^3 bounds every point in an unvisited cell from below (a side at the grid's edge has nothing
// beyond it, and a clamped cell needs nothing more: a face plane still bounds everything beyond it); stop(bnd) gets that bound less
// `margin` — at least GridParams.slack, far above the rounding of the cell keys and of the faces — and says whether to leave,
// normally grid_bound_clears against the caller's running best.  Correct for any cell size.
// With one query per wavefront, or 64 queries of one cell (the cell coordinates, and so every loop bound and range, are then
// wave-uniform), stop must be wave-uniform: it does its own __ballot.  One query per thread may pass a per-thread rule.
// "The whole grid is visited" is the integer test on the cell coordinates: wave-uniform by construction, and for finite
// coordinates the same as bnd == +inf, since every open side contributes a finite term.  Non-finite and |x| > 1e150 input never
// reaches a grid kernel (GridParams.fallback), and the voxel centres of dense_seeds_dev.hip are finite.
template <typename Scan, typename Stop>
__device__ __forceinline__ void grid_shell_walk(const GridParams& p, const int* __restrict__ start, int cx, int cy, int cz, double qx,
                                                double qy, double qz, double margin, Scan scan, Stop stop) {
    const int rmax = max(max(p.gx, p.gy), p.gz);
    for (int r = 0; r <= rmax; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, p.gz - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, p.gy - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, p.gx - 1);
        for (int z = z0; z <= z1; ++z) {
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * p.gy + y) * p.gx;
                if (z == cz - r || z == cz + r || y == cy - r || y == cy + r) {        // a face row of the shell: its whole x range
                    scan(start[row + x0], start[row + x1 + 1]);
                } else {                                                            // an inner row: its two end cells
                    if (cx - r >= 0) scan(start[row + cx - r], start[row + cx - r + 1]);
                    if (cx + r < p.gx) scan(start[row + cx + r], start[row + cx + r + 1]);
                }
            }
        }
        double bnd = __builtin_huge_val();
        if (cx - r > 0) bnd = fmin(bnd, __dsub_rn(qx, __dadd_rn(p.ox, __dmul_rn((double)(cx - r), p.h))));
        if (cx + r < p.gx - 1) bnd = fmin(bnd, __dsub_rn(__dadd_rn(p.ox, __dmul_rn((double)(cx + r + 1), p.h)), qx));
        if (cy - r > 0) bnd = fmin(bnd, __dsub_rn(qy, __dadd_rn(p.oy, __dmul_rn((double)(cy - r), p.h))));
        if (cy + r < p.gy - 1) bnd = fmin(bnd, __dsub_rn(__dadd_rn(p.oy, __dmul_rn((double)(cy + r + 1), p.h)), qy));
        if (cz - r > 0) bnd = fmin(bnd, __dsub_rn(qz, __dadd_rn(p.oz, __dmul_rn((double)(cz - r), p.h))));
        if (cz + r < p.gz - 1) bnd = fmin(bnd, __dsub_rn(__dadd_rn(p.oz, __dmul_rn((double)(cz + r + 1), p.h)), qz));
        if (cx - r <= 0 && cx + r >= p.gx - 1 && cy - r <= 0 && cy + r >= p.gy - 1 && cz - r <= 0 && cz + r >= p.gz - 1)
            break;                                                           // the whole grid is visited
        if (stop(__dsub_rn(bnd, margin))) break;
    }
}

// one wavefront (every lane ends with the result): the bad flag of a point set's bounding-box partials folded into *bad, and the
// largest |coordinate| of its box into *amax — what a search adds to the slack, times 1e-11, for a set whose coordinates meet the
// grid's in a subtraction.  amax NULL (a literal at the call: the branch folds away): the bad flag alone.  Maxima: any order.
__device__ __forceinline__ void grid_partials_fold(const double* __restrict__ partials, double* amax, double* bad) {
    double a = 0.0, f = 0.0;
    for (int b = threadIdx.x & 63; b < KNN_GRID_BBOX_BLOCKS; b += 64) {
        const double* q = partials + b * 8;
        f = fmax(f, q[6]);
        if (!amax) continue;
        for (int c = 0; c < 6; ++c)
            if (fabs(q[c]) <= 1e150) a = fmax(a, fabs(q[c]));               // a block without points holds +-inf
    }
    if (amax) *amax = wave_max(a);
    *bad = fmax(*bad, wave_max(f));
}

int launch_exclusive_scan_int(int* a, int64_t m, int* tile_sums, hipStream_t st);
int launch_grid_bbox(const double* pts, int64_t n, double* partials, hipStream_t st);
int launch_grid_params(const double* pts, int64_t n, int k, double cell_size, const GridWs& w, hipStream_t st);
int launch_grid_setup(const double* pts, int64_t n, int k, double cell_size, const GridWs& w, GridParams* hp, hipStream_t st);
int launch_grid_sort(const double* pts, int64_t n, const GridWs& w, const GridParams& hp, hipStream_t st);
// wstart[0 .. cells] = the exclusive scan of ceil(queries of the cell / 64), from the sorted queries' qstart (tile_sums: the scan's)
int launch_grid_query_waves(const int* qstart, int64_t cells, int* wstart, int* tile_sums, hipStream_t st);

}  // namespace sapcu
