// The device cell grid of knn_grid.hip, for the translation units that search it: parameters, workspace layout, the build and
// the int exclusive scan (kernels live in knn_grid.hip; a kernel is launched from the file that defines it).
#pragma once
#include "common.h"

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
    size_t bytes;
};

static GridWs grid_ws_layout(void* base, int64_t n) {
    const int64_t cap = grid_cell_cap(n);
    const int64_t tiles = (cap + 1 + SCAN_TILE - 1) / SCAN_TILE;
    WsCarver c(base);
    GridWs w;
    w.partials = c.take<double>(8 * KNN_GRID_BBOX_BLOCKS);
    w.params = c.take<GridParams>(1);
    w.start = c.take<int>(cap + 1);
    w.cursor = c.take<int>(cap);
    w.tile_sums = c.take<int>(tiles);
    w.key = c.take<int>(n);
    w.sx = c.take<double>(n);
    w.sy = c.take<double>(n);
    w.sz = c.take<double>(n);
    w.sidx = c.take<int>(n);
    w.bytes = c.bytes();
    return w;
}

__device__ __forceinline__ int grid_coord(double v, double o, double h, int g) {
    const double t = floor(__ddiv_rn(__dsub_rn(v, o), h));
    return t < 0.0 ? 0 : (t >= (double)(g - 1) ? g - 1 : (int)t);
}

int launch_exclusive_scan_int(int* a, int64_t m, int* tile_sums, hipStream_t st);
int launch_grid_bbox(const double* pts, int64_t n, double* partials, hipStream_t st);
int launch_grid_params(const double* pts, int64_t n, int k, double cell_size, const GridWs& w, hipStream_t st);
int launch_grid_setup(const double* pts, int64_t n, int k, double cell_size, const GridWs& w, GridParams* hp, hipStream_t st);
int launch_grid_sort(const double* pts, int64_t n, const GridWs& w, const GridParams& hp, hipStream_t st);

}  // namespace sapcu
