// Seed generation on the device: the voxel flood of dense_seeds.cpp (the reference's dense.cpp:175-252), level-synchronous, with
// the seeds left in HBM.  Same seeds, same order, same 6-decimal values as sapcu_dense_seeds_host, bit for bit.
//
// Per level (a frontier of m voxel keys in the host's queue order):
//   1. seeds_eval_kernel — one voxel per thread.  The 11 nearest of the n+1 points (the cloud plus the reference's all-zero point)
//      by grid_shell_walk (knn_grid.h) on knn_grid.hip's cell grid, compared on (squared distance, index) keys; the squared
//      distance is ((q-p)_x^2 + (q-p)_y^2) + (q-p)_z^2 in separately rounded f64 — the host's (0 + dx^2) + dy^2 + dz^2 (0 + a = a,
//      (p-q)^2 = (q-p)^2 exactly).  The ten nearest in DESCENDING key order are the host heap's pop order: near[0..7] the fan,
//      near[8], near[9] (the two nearest) the shared edge; fewer than 10 points leave zeros behind the ones found.  Then
//      closest_on_triangle and dist in the operation order of dense_seeds.cpp (no contraction: -ffp-contract=off, no fma written
//      here; IEEE divide, correctly rounded sqrt).  A voxel whose 10th and 11th nearest tie exactly (the host's heap keeps whichever
//      its k-d traversal met first) or whose x index lies outside the 6-decimal table is put on a list: the host's own
//      fan_distance recomputes it (dense_seeds_host.h) before the bookkeeping runs;
//   2. the reference's sequential FIFO bookkeeping, in parallel.  Candidate j = 6*i + d (neighbour d of frontier voxel i, order
//      +x -x +y -y +z -z, only if voxel i expands: not (best > 0.015)) has the sequence number base + j, its position in the host's
//      queue; the initial candidates (the points' voxels) have their point index.  seeds_insert_kernel: an open-addressing table
//      keyed by voxel key keeps the MINIMUM sequence number ever seen (atomicCAS claims the slot, atomicMin the number — integer
//      atomics, so the outcome does not depend on slot placement or timing).  seeds_flag_kernel: a candidate wins iff the table
//      holds its own number (the host's `met.insert(key)` returned true for exactly that push); band voxels (0.011 <= best <=
//      0.015) are flagged in the same array.  One exclusive scan (knn_grid.hip's three kernels) of [band flags | win flags] gives
//      both the seed slots and the next frontier's slots, in queue order; seeds_scatter_kernel writes them.
// The eval kernel runs on a fixed grid and reads the frontier size on the device, so ONE read-back per level (after the eval:
// frontier size, flagged count, error bits, seeds so far) is all the host needs to size the level's other launches.
//
// Voxel keys, their % and / decomposition and the neighbour keys are the host's `int` arithmetic, keys that leave the grid included.
#include <cmath>
#include <vector>

#include "common.h"
#include "knn_grid.h"
#include "dense_seeds_host.h"
#include "../../include/sapcu_seeds.h"

namespace sapcu {

constexpr int SEED_NN = 11;                     // the ten of the fan + the one that shows a tie at the boundary
constexpr int SEED_EMPTY = (int)0x80000000;     // free table slot (never a voxel key: checked)
constexpr int SEED_MAX_BOX = 1000;              // boxsize = round(1/cell): keys up to 2*boxsize^3 stay inside int
constexpr int SEED_TAB = 3 * SEED_MAX_BOX + 1;  // 6-decimal centre values for the indices -boxsize .. 2*boxsize
constexpr int SEED_MAX_PROBE = 4096;            // a probe sequence this long in a table at most half full of counted keys: full
constexpr int64_t SEED_MAX_N = 1LL << 28;       // n + 6 * max_voxels sequence numbers stay below 2^31
enum { C_M = 0, C_NFLAG = 1, C_ERR = 2, C_USED = 3, C_SEEDS = 4, C_WORDS = 8 };

struct SeedWs {
    double* pts;          // [n+1][3]: the cloud + the all-zero point
    GridWs grid;          // of n+1 points
    double* tab;          // [SEED_TAB]
    int* ctrl;            // [C_WORDS]
    int* ikey;            // [n] the points' voxel keys
    int* front[2];        // [max_voxels] each
    double* best;         // [max_voxels]
    double* x6;           // [max_voxels] 6-decimal x of a voxel outside the table (written by the host)
    int* flagged;         // [max_voxels] frontier positions handed to the host
    int* flags;           // [max(7 * max_voxels, n) + 1]
    int* tile_sums;
    int* tkey;            // [slots]
    int* tseq;            // [slots]
    int64_t slots, nflags;
    size_t bytes;
};

static int64_t seed_slots(int64_t maxv) {
    int64_t s = 1024;
    while (s < 2 * maxv) s <<= 1;
    return s;
}

static SeedWs seed_ws_layout(void* base, int64_t n, int64_t maxv) {
    WsCarver c(base);
    SeedWs w;
    w.slots = seed_slots(maxv);
    w.nflags = (7 * maxv > n ? 7 * maxv : n) + 1;
    w.pts = c.take<double>(3 * (n + 1));
    w.grid = grid_ws_layout(c.take<char>((int64_t)grid_ws_layout(nullptr, n + 1).bytes), n + 1);
    w.tab = c.take<double>(SEED_TAB);
    w.ctrl = c.take<int>(C_WORDS);
    w.ikey = c.take<int>(n);
    w.front[0] = c.take<int>(maxv);
    w.front[1] = c.take<int>(maxv);
    w.best = c.take<double>(maxv);
    w.x6 = c.take<double>(maxv);
    w.flagged = c.take<int>(maxv);
    w.flags = c.take<int>(w.nflags);
    w.tile_sums = c.take<int>((w.nflags + SCAN_TILE - 1) / SCAN_TILE);
    w.tkey = c.take<int>(w.slots);
    w.tseq = c.take<int>(w.slots);
    w.bytes = c.bytes();
    return w;
}

// ------------------------------------------------------------------------------------------------------------ table
__device__ __forceinline__ unsigned seed_hash(int key) {
    unsigned h = (unsigned)key * 0x9E3779B1u;
    return h ^ (h >> 15);
}

__global__ __launch_bounds__(256) void seeds_init_kernel(int* __restrict__ tkey, int* __restrict__ tseq, int64_t slots,
                                                         int* __restrict__ ctrl) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < slots) {
        tkey[i] = SEED_EMPTY;
        tseq[i] = 0x7fffffff;
    }
    if (i < C_WORDS) ctrl[i] = 0;
}

// keep min(seq) for `key`; a table that cannot take the key sets the error bit, never writes outside [0, mask]
__device__ __forceinline__ void seed_insert(int* tkey, int* tseq, unsigned mask, int key, int seq, int* ctrl, int maxv) {
    if (key == SEED_EMPTY || __atomic_load_n(&ctrl[C_ERR], __ATOMIC_RELAXED) != 0) {
        atomicOr(&ctrl[C_ERR], 1);
        return;
    }
    unsigned s = seed_hash(key) & mask;
    for (int probe = 0; probe < SEED_MAX_PROBE; ++probe, s = (s + 1) & mask) {
        const int prev = atomicCAS(&tkey[s], SEED_EMPTY, key);
        if (prev == SEED_EMPTY && atomicAdd(&ctrl[C_USED], 1) >= maxv) atomicOr(&ctrl[C_ERR], 1);
        if (prev == SEED_EMPTY || prev == key) {
            atomicMin(&tseq[s], seq);
            return;
        }
    }
    atomicOr(&ctrl[C_ERR], 1);
}

__device__ __forceinline__ int seed_lookup(const int* tkey, const int* tseq, unsigned mask, int key) {
    unsigned s = seed_hash(key) & mask;
    for (int probe = 0; probe < SEED_MAX_PROBE; ++probe, s = (s + 1) & mask) {
        const int k = tkey[s];
        if (k == key) return tseq[s];
        if (k == SEED_EMPTY) break;
    }
    return -1;                                   // only after an error bit: no candidate has this number
}

// ------------------------------------------------------------------------------------------------------ fan distance
struct D3 {
    double x, y, z;
};
__device__ __forceinline__ D3 d3sub(const D3& a, const D3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 d3add(const D3& a, const D3& b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 d3mul(const D3& a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ D3 d3div(const D3& a, double s) { return {__ddiv_rn(a.x, s), __ddiv_rn(a.y, s), __ddiv_rn(a.z, s)}; }
__device__ __forceinline__ double d3dot(const D3& a, const D3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 d3cross(const D3& a, const D3& b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double d3dist(const D3& a, const D3& b) {
    return sqrt_cr((a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y) + (a.z - b.z) * (a.z - b.z));
}

// dense_seeds.cpp closest_on_triangle, operation for operation
__device__ D3 seed_closest_on_triangle(const D3& a, const D3& b, const D3& c, const D3& p) {
    const D3 ab = d3sub(b, a), ac = d3sub(c, a), bc = d3sub(c, b);
    const double snom = d3dot(d3sub(p, a), ab), sdenom = d3dot(d3sub(p, b), d3sub(a, b));
    const double tnom = d3dot(d3sub(p, a), ac), tdenom = d3dot(d3sub(p, c), d3sub(a, c));
    if (snom <= 0.0 && tnom <= 0.0) return a;
    const double unom = d3dot(d3sub(p, b), bc), udenom = d3dot(d3sub(p, c), d3sub(b, c));
    if (sdenom <= 0.0 && unom <= 0.0) return b;
    if (tdenom <= 0.0 && udenom <= 0.0) return c;
    const D3 n = d3cross(d3sub(b, a), d3sub(c, a));
    const double vc = d3dot(n, d3cross(d3sub(a, p), d3sub(b, p)));
    if (vc <= 0.0 && snom >= 0.0 && sdenom >= 0.0) return d3add(a, d3div(d3mul(ab, snom), snom + sdenom));
    const double va = d3dot(n, d3cross(d3sub(b, p), d3sub(c, p)));
    if (va <= 0.0 && unom >= 0.0 && udenom >= 0.0) return d3add(b, d3div(d3mul(bc, unom), unom + udenom));
    const double vb = d3dot(n, d3cross(d3sub(c, p), d3sub(a, p)));
    if (vb <= 0.0 && tnom >= 0.0 && tdenom >= 0.0) return d3add(a, d3div(d3mul(ac, tnom), tnom + tdenom));
    const double u = __ddiv_rn(va, va + vb + vc);
    const double w2 = __ddiv_rn(vb, va + vb + vc);
    const double w3 = 1.0 - u - w2;
    return d3add(d3add(d3mul(a, u), d3mul(b, w2)), d3mul(c, w3));
}

// the running 11 nearest of one thread, ascending on (d, i), in registers (every index below is a compile-time constant)
struct SeedList {
    double d[SEED_NN];
    int i[SEED_NN];
};

__device__ __forceinline__ bool seed_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

__device__ __forceinline__ void seed_scan_range(SeedList& L, int a, int b, double qx, double qy, double qz,
                                                const double* __restrict__ sx, const double* __restrict__ sy,
                                                const double* __restrict__ sz, const int* __restrict__ sidx) {
    for (int j = a; j < b; ++j) {
        const double dx = qx - sx[j], dy = qy - sy[j], dz = qz - sz[j];
        const double cd = (dx * dx + dy * dy) + dz * dz;
        const int ci = sidx[j];
        if (!seed_less(cd, ci, L.d[SEED_NN - 1], L.i[SEED_NN - 1])) continue;
#pragma unroll
        for (int p = SEED_NN - 1; p >= 0; --p) {                    // downwards: entry p-1 is still the old one
            const bool below_prev = p > 0 && seed_less(cd, ci, L.d[p > 0 ? p - 1 : 0], L.i[p > 0 ? p - 1 : 0]);
            const bool below_cur = seed_less(cd, ci, L.d[p], L.i[p]);
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

struct SeedGeom {
    double cell;
    int boxsize;
    int npts;            // n + 1
};

__device__ __forceinline__ void seed_voxel_xyz(int key, int boxsize, int& x, int& y, int& z) {
    int t = key;
    z = t % boxsize;
    t /= boxsize;
    y = t % boxsize;
    t /= boxsize;
    x = t;
}

__global__ __launch_bounds__(256) void seeds_eval_kernel(const int* __restrict__ front, int* __restrict__ ctrl, SeedGeom g,
                                                         const double* __restrict__ pts, const GridParams* __restrict__ prm,
                                                         const int* __restrict__ start, const double* __restrict__ sx,
                                                         const double* __restrict__ sy, const double* __restrict__ sz,
                                                         const int* __restrict__ sidx, double* __restrict__ best_out,
                                                         int* __restrict__ flagged) {
    const int m = ctrl[C_M];
    const GridParams p = *prm;
    const double INF = __builtin_huge_val();
    for (int64_t vi = (int64_t)blockIdx.x * 256 + threadIdx.x; vi < m; vi += (int64_t)gridDim.x * 256) {
        int x, y, z;
        seed_voxel_xyz(front[vi], g.boxsize, x, y, z);
        const double qx = x * g.cell + 0.5 * g.cell - 0.5;
        const double qy = y * g.cell + 0.5 * g.cell - 0.5;
        const double qz = z * g.cell + 0.5 * g.cell - 0.5;
        const int cx = grid_coord(qx, p.ox, p.h, p.gx);
        const int cy = grid_coord(qy, p.oy, p.h, p.gy);
        const int cz = grid_coord(qz, p.oz, p.h, p.gz);
        SeedList L;
#pragma unroll
        for (int q = 0; q < SEED_NN; ++q) {
            L.d[q] = INF;
            L.i[q] = 0x7fffffff;
        }
        grid_shell_walk(                                                // one voxel per thread: a per-thread stop rule
            p, start, cx, cy, cz, qx, qy, qz, p.slack,
            [&](int a, int b) { seed_scan_range(L, a, b, qx, qy, qz, sx, sy, sz, sidx); },
            [&](double bnd) { return grid_bound_clears(bnd, L.d[SEED_NN - 1]); });
        // host recomputation: a tie at the boundary of the ten, or no table entry for x
        const bool tie = g.npts >= SEED_NN && L.d[SEED_NN - 2] == L.d[SEED_NN - 1];
        const bool off_table = x < -g.boxsize || x > 2 * g.boxsize;
        if (tie || off_table) flagged[atomicAdd(&ctrl[C_NFLAG], 1)] = (int)vi;   // at most m <= max_voxels entries
        // near[c] = the c-th pop of the host's heap: entry cnt-1-c of the list, zeros behind the cnt points found
        const int cnt = g.npts < 10 ? g.npts : 10;
        const D3 centre{qx, qy, qz};
        D3 e[2];
#pragma unroll
        for (int c = 8; c < 10; ++c) {
            int pi = -1;
#pragma unroll
            for (int q = 0; q < 10; ++q)
                if (q == cnt - 1 - c) pi = L.i[q];
            e[c - 8] = pi >= 0 ? D3{pts[3 * (int64_t)pi], pts[3 * (int64_t)pi + 1], pts[3 * (int64_t)pi + 2]} : D3{0.0, 0.0, 0.0};
        }
        double best = 99999999999999.0;
        for (int c = 0; c < 8; ++c) {
            int pi = -1;
#pragma unroll
            for (int q = 0; q < 10; ++q)
                if (q == cnt - 1 - c) pi = L.i[q];
            const D3 a = pi >= 0 ? D3{pts[3 * (int64_t)pi], pts[3 * (int64_t)pi + 1], pts[3 * (int64_t)pi + 2]} : D3{0.0, 0.0, 0.0};
            const double d = d3dist(seed_closest_on_triangle(a, e[0], e[1], centre), centre);
            if (d < best) best = d;
        }
        best_out[vi] = best;
    }
}

// -------------------------------------------------------------------------------------------------------- bookkeeping
__device__ __forceinline__ bool seed_in_band(double best) { return best >= 0.0110 && best <= 0.0150; }
__device__ __forceinline__ bool seed_expands(double best) { return !(best > 0.0150); }     // NaN expands, as on the host

__device__ __forceinline__ int seed_neighbour_key(int key, int boxsize, int d) {
    int x, y, z;
    seed_voxel_xyz(key, boxsize, x, y, z);
    const int s = (d & 1) ? -1 : 1, axis = d >> 1;
    return (x + (axis == 0 ? s : 0)) * boxsize * boxsize + (y + (axis == 1 ? s : 0)) * boxsize + (z + (axis == 2 ? s : 0));
}

__global__ __launch_bounds__(256) void seeds_insert_initial_kernel(const int* __restrict__ ikey, int n, int* tkey, int* tseq,
                                                                   unsigned mask, int* ctrl, int maxv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) seed_insert(tkey, tseq, mask, ikey[i], i, ctrl, maxv);
}

__global__ __launch_bounds__(256) void seeds_flag_initial_kernel(const int* __restrict__ ikey, int n, const int* __restrict__ tkey,
                                                                 const int* __restrict__ tseq, unsigned mask, int* __restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = seed_lookup(tkey, tseq, mask, ikey[i]) == i ? 1 : 0;
    if (i == n) flags[i] = 0;
}

__global__ __launch_bounds__(256) void seeds_scatter_initial_kernel(const int* __restrict__ ikey, int n, const int* __restrict__ scan,
                                                                    int* __restrict__ front, int* __restrict__ ctrl, int maxv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && scan[i + 1] - scan[i] == 1 && scan[i] < maxv) front[scan[i]] = ikey[i];
    if (i == n) {
        const int total = scan[n];
        if (total > maxv) atomicOr(&ctrl[C_ERR], 1);
        ctrl[C_M] = total > maxv ? maxv : total;
    }
}

__global__ __launch_bounds__(256) void seeds_insert_kernel(const int* __restrict__ front, const double* __restrict__ best, int m,
                                                           int base, int boxsize, int* tkey, int* tseq, unsigned mask, int* ctrl,
                                                           int maxv) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= 6 * (int64_t)m) return;
    const int i = (int)(j / 6), d = (int)(j % 6);
    if (!seed_expands(best[i])) return;
    seed_insert(tkey, tseq, mask, seed_neighbour_key(front[i], boxsize, d), base + (int)j, ctrl, maxv);
}

// flags[0, m): band voxels; flags[m, 7m): winning candidates; flags[7m] = 0 (its scan value is the total)
__global__ __launch_bounds__(256) void seeds_flag_kernel(const int* __restrict__ front, const double* __restrict__ best, int m,
                                                         int base, int boxsize, const int* __restrict__ tkey,
                                                         const int* __restrict__ tseq, unsigned mask, int* __restrict__ flags,
                                                         int* __restrict__ ctrl) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) ctrl[C_NFLAG] = 0;
    if (t < m) {
        flags[t] = seed_in_band(best[t]) ? 1 : 0;
    } else if (t < 7 * (int64_t)m) {
        const int64_t j = t - m;
        const int i = (int)(j / 6), d = (int)(j % 6);
        int won = 0;
        if (seed_expands(best[i])) won = seed_lookup(tkey, tseq, mask, seed_neighbour_key(front[i], boxsize, d)) == base + (int)j;
        flags[t] = won;
    } else if (t == 7 * (int64_t)m) {
        flags[t] = 0;
    }
}

__global__ __launch_bounds__(256) void seeds_scatter_kernel(const int* __restrict__ front, int m, int boxsize, const int* __restrict__ scan,
                                                            const double* __restrict__ tab, const double* __restrict__ x6,
                                                            int seed_base, double* __restrict__ seeds, int64_t capacity,
                                                            int* __restrict__ next, int* __restrict__ ctrl, int maxv) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < m) {
        if (scan[t + 1] - scan[t] == 1) {
            const int64_t pos = (int64_t)seed_base + scan[t];
            if (pos < capacity) {
                int x, y, z;
                seed_voxel_xyz(front[t], boxsize, x, y, z);                 // |y|, |z| < boxsize: always inside the table
                seeds[3 * pos + 0] = (x < -boxsize || x > 2 * boxsize) ? x6[t] : tab[x + boxsize];
                seeds[3 * pos + 1] = tab[y + boxsize];
                seeds[3 * pos + 2] = tab[z + boxsize];
            }
        }
    } else if (t < 7 * (int64_t)m) {
        if (scan[t + 1] - scan[t] == 1) {
            const int pos = scan[t] - scan[m];
            const int64_t j = t - m;
            if (pos < maxv) next[pos] = seed_neighbour_key(front[j / 6], boxsize, (int)(j % 6));
        }
    } else if (t == 7 * (int64_t)m) {
        const int total = scan[7 * (int64_t)m] - scan[m];
        if (total > maxv) atomicOr(&ctrl[C_ERR], 1);
        ctrl[C_M] = total > maxv ? maxv : total;
        ctrl[C_SEEDS] = seed_base + scan[m];
    }
}

// ---------------------------------------------------------------------------------------------------------- launcher
struct HostFanGuard {
    sapcu_seeds::HostFan* f = nullptr;
    ~HostFanGuard() {
        if (f) sapcu_seeds::host_fan_destroy(f);
    }
};

static int launch_dense_seeds(const double* cloud, int64_t n, double cell, int boxsize, double* seeds, int64_t capacity,
                              int64_t maxv, int64_t* count_host, int64_t* stats, const SeedWs& w, hipStream_t st) {
    // the cloud on the host: validation, the points' voxel keys in the host's own arithmetic, the tie path
    std::vector<double> hc((size_t)n * 3);
    SAPCU_CHECK_HIP(hipMemcpyAsync(hc.data(), cloud, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    std::vector<int> ikey((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const double x = hc[3 * i], y = hc[3 * i + 1], z = hc[3 * i + 2];
        SAPCU_CHECK_ARG(std::isfinite(x) && std::isfinite(y) && std::isfinite(z), "dense_seeds: point %lld is not finite", (long long)i);
        const double kd = std::floor(((x + 0.5) / cell)) * boxsize * boxsize + std::floor(((y + 0.5) / cell)) * boxsize +
                          std::floor(((z + 0.5) / cell));
        SAPCU_CHECK_ARG(std::fabs(kd) <= 2e9, "dense_seeds: the voxel key of point %lld does not fit an int", (long long)i);
        ikey[i] = (int)kd;
    }
    std::vector<double> tab(SEED_TAB, 0.0);
    for (int t = -boxsize; t <= 2 * boxsize; ++t) tab[t + boxsize] = sapcu_seeds::host_six_decimals(t * cell + 0.5 * cell - 0.5);

    SAPCU_CHECK_HIP(hipMemcpyAsync(w.pts, cloud, sizeof(double) * 3 * n, hipMemcpyDeviceToDevice, st));
    SAPCU_CHECK_HIP(hipMemsetAsync(w.pts + 3 * n, 0, sizeof(double) * 3, st));
    SAPCU_CHECK_HIP(hipMemcpyAsync(w.tab, tab.data(), sizeof(double) * SEED_TAB, hipMemcpyHostToDevice, st));
    SAPCU_CHECK_HIP(hipMemcpyAsync(w.ikey, ikey.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    GridParams hp;
    int rc = launch_grid_setup(w.pts, n + 1, SEED_NN, 0.0, w.grid, &hp, st);      // synchronises: tab and ikey are uploaded
    if (rc != SAPCU_OK) return rc;
    SAPCU_CHECK_ARG(!hp.fallback, "dense_seeds: coordinates too large for the cell grid");
    rc = launch_grid_sort(w.pts, n + 1, w.grid, hp, st);
    if (rc != SAPCU_OK) return rc;

    const unsigned mask = (unsigned)(w.slots - 1);
    const int mv = (int)maxv, ni = (int)n;
    hipLaunchKernelGGL(seeds_init_kernel, dim3((unsigned)((w.slots + 255) / 256)), dim3(256), 0, st, w.tkey, w.tseq, w.slots, w.ctrl);
    SAPCU_CHECK_LAUNCH();
    const unsigned nb1 = (unsigned)((n + 1 + 255) / 256);
    hipLaunchKernelGGL(seeds_insert_initial_kernel, dim3(nb1), dim3(256), 0, st, w.ikey, ni, w.tkey, w.tseq, mask, w.ctrl, mv);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(seeds_flag_initial_kernel, dim3(nb1), dim3(256), 0, st, w.ikey, ni, w.tkey, w.tseq, mask, w.flags);
    SAPCU_CHECK_LAUNCH();
    rc = launch_exclusive_scan_int(w.flags, n + 1, w.tile_sums, st);
    if (rc != SAPCU_OK) return rc;
    hipLaunchKernelGGL(seeds_scatter_initial_kernel, dim3(nb1), dim3(256), 0, st, w.ikey, ni, w.flags, w.front[0], w.ctrl, mv);
    SAPCU_CHECK_LAUNCH();

    const SeedGeom g{cell, boxsize, (int)(n + 1)};
    const int64_t eval_blocks_max = (int64_t)device_cu_count() * 8;
    const unsigned eval_blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((maxv + 255) / 256, eval_blocks_max));
    HostFanGuard fan;
    std::vector<int> hflag, hfront;
    std::vector<double> hbest, hx6;
    int64_t levels = 0, evaluated = 0, redone = 0, base = n;
    int cur = 0, ctrl[C_WORDS];
    for (;;) {
        hipLaunchKernelGGL(seeds_eval_kernel, dim3(eval_blocks), dim3(256), 0, st, w.front[cur], w.ctrl, g, w.pts, w.grid.params,
                           w.grid.start, w.grid.sx, w.grid.sy, w.grid.sz, w.grid.sidx, w.best, w.flagged);
        SAPCU_CHECK_LAUNCH();
        SAPCU_CHECK_HIP(hipMemcpyAsync(ctrl, w.ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, st));
        SAPCU_CHECK_HIP(hipStreamSynchronize(st));
        const int m = ctrl[C_M];
        if (ctrl[C_ERR] || m == 0) break;
        ++levels;
        evaluated += m;
        if (ctrl[C_NFLAG] > 0) {                       // the host's own fan distance for the flagged voxels of this level
            const int nf = ctrl[C_NFLAG];
            redone += nf;
            if (!fan.f) fan.f = sapcu_seeds::host_fan_create(hc.data(), n);
            hflag.resize(nf);
            hfront.resize(m);
            hbest.resize(m);
            hx6.assign(m, 0.0);
            SAPCU_CHECK_HIP(hipMemcpyAsync(hflag.data(), w.flagged, sizeof(int) * nf, hipMemcpyDeviceToHost, st));
            SAPCU_CHECK_HIP(hipMemcpyAsync(hfront.data(), w.front[cur], sizeof(int) * m, hipMemcpyDeviceToHost, st));
            SAPCU_CHECK_HIP(hipMemcpyAsync(hbest.data(), w.best, sizeof(double) * m, hipMemcpyDeviceToHost, st));
            SAPCU_CHECK_HIP(hipStreamSynchronize(st));
            for (int f = 0; f < nf; ++f) {
                const int vi = hflag[f];
                int t = hfront[vi];
                const int z = t % boxsize;
                t /= boxsize;
                const int y = t % boxsize;
                t /= boxsize;
                const int x = t;
                const double cx = x * cell + 0.5 * cell - 0.5;
                hbest[vi] = sapcu_seeds::host_fan_distance(fan.f, cx, y * cell + 0.5 * cell - 0.5, z * cell + 0.5 * cell - 0.5);
                hx6[vi] = sapcu_seeds::host_six_decimals(cx);
            }
            SAPCU_CHECK_HIP(hipMemcpyAsync(w.best, hbest.data(), sizeof(double) * m, hipMemcpyHostToDevice, st));
            SAPCU_CHECK_HIP(hipMemcpyAsync(w.x6, hx6.data(), sizeof(double) * m, hipMemcpyHostToDevice, st));
            SAPCU_CHECK_HIP(hipStreamSynchronize(st));            // the host vectors are reused by the next level
        }
        const unsigned nb6 = (unsigned)((6 * (int64_t)m + 255) / 256), nb7 = (unsigned)((7 * (int64_t)m + 1 + 255) / 256);
        hipLaunchKernelGGL(seeds_insert_kernel, dim3(nb6), dim3(256), 0, st, w.front[cur], w.best, m, (int)base, boxsize, w.tkey,
                           w.tseq, mask, w.ctrl, mv);
        SAPCU_CHECK_LAUNCH();
        hipLaunchKernelGGL(seeds_flag_kernel, dim3(nb7), dim3(256), 0, st, w.front[cur], w.best, m, (int)base, boxsize, w.tkey,
                           w.tseq, mask, w.flags, w.ctrl);
        SAPCU_CHECK_LAUNCH();
        rc = launch_exclusive_scan_int(w.flags, 7 * (int64_t)m + 1, w.tile_sums, st);
        if (rc != SAPCU_OK) return rc;
        hipLaunchKernelGGL(seeds_scatter_kernel, dim3(nb7), dim3(256), 0, st, w.front[cur], m, boxsize, w.flags, w.tab, w.x6,
                           ctrl[C_SEEDS], seeds, capacity, w.front[cur ^ 1], w.ctrl, mv);
        SAPCU_CHECK_LAUNCH();
        base += 6 * (int64_t)m;
        cur ^= 1;
    }
    *count_host = ctrl[C_SEEDS];
    if (stats) {
        stats[0] = levels;
        stats[1] = evaluated;
        stats[2] = redone;
        stats[3] = w.slots;
    }
    if (ctrl[C_ERR]) {
        set_error("dense_seeds: more than max_voxels = %lld distinct voxels", (long long)maxv);
        return SAPCU_ERR_WORKSPACE;
    }
    if (ctrl[C_SEEDS] > capacity) {
        set_error("dense_seeds: %d seeds, capacity %lld", ctrl[C_SEEDS], (long long)capacity);
        return SAPCU_ERR_WORKSPACE;
    }
    return SAPCU_OK;
}

static bool seed_box(double cell, int* boxsize) {
    if (!(cell > 0.0)) return false;
    const double b = std::round(1 / cell);
    if (!(b >= 1.0 && b <= (double)SEED_MAX_BOX)) return false;
    *boxsize = (int)b;
    return true;
}

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

extern "C" {

int64_t sapcu_dense_seeds_workspace_bytes(int64_t n, int64_t max_voxels) {
    if (n < 1 || n > SEED_MAX_N || max_voxels < 1 || max_voxels > SEED_MAX_N) return -1;
    return (int64_t)seed_ws_layout(nullptr, n, max_voxels).bytes;
}

int sapcu_dense_seeds_f64(const double* cloud_dev, int64_t n, double cell, double* seeds_out_dev, int64_t capacity,
                          int64_t max_voxels, int64_t* count_host, int64_t* stats_host, void* workspace,
                          int64_t workspace_bytes, void* stream) {
    SAPCU_CHECK_ARG(cloud_dev && count_host && workspace, "dense_seeds: null pointer");
    SAPCU_CHECK_ARG(n >= 1 && n <= SEED_MAX_N, "dense_seeds: need 1 <= n <= 2^28 (n=%lld)", (long long)n);
    SAPCU_CHECK_ARG(max_voxels >= 1 && max_voxels <= SEED_MAX_N, "dense_seeds: need 1 <= max_voxels <= 2^28 (got %lld)",
                    (long long)max_voxels);
    SAPCU_CHECK_ARG(capacity >= 0 && (capacity == 0 || seeds_out_dev), "dense_seeds: capacity %lld without a seed buffer",
                    (long long)capacity);
    int boxsize = 0;
    SAPCU_CHECK_ARG(seed_box(cell, &boxsize), "dense_seeds: need cell > 0 with round(1/cell) in 1..%d (cell=%g)", SEED_MAX_BOX, cell);
    SAPCU_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "dense_seeds: the workspace must be 8-byte aligned (f64 tables)");
    const SeedWs w = seed_ws_layout(workspace, n, max_voxels);
    SAPCU_CHECK_ARG((int64_t)w.bytes <= workspace_bytes, "dense_seeds: workspace of %lld bytes, need %lld",
                    (long long)workspace_bytes, (long long)w.bytes);
    *count_host = 0;
    if (stats_host) stats_host[0] = stats_host[1] = stats_host[2] = stats_host[3] = 0;
    return launch_dense_seeds(cloud_dev, n, cell, boxsize, seeds_out_dev, capacity, max_voxels, count_host, stats_host, w,
                              (hipStream_t)stream);
}

}  // extern "C"
