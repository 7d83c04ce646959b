// Poisson-disk selection and the exact-count subsample of a cloud (csrc/sapcu_poisson.h: the definition, the two paths, the margin
// of the cell edge and its derivation; tests/poisson_ref.py restates the definition in numpy).
//
// Resident path (pd_resident_kernel): one work group per batch entry, everything of the entry in LDS, synchronous rounds between
// work-group barriers, the bisection inside the launch.  Grid path (pd_grid_*): the cell sort of knn_grid.h per radius, one launch
// per round (state_in -> state_out, so a round reads what the round before left), chunks of rounds between read-backs.
#include <math.h>

#include <vector>

#include "common.h"
#include "knn_grid.h"
#include "sapcu_poisson.h"

namespace sapcu {

constexpr int PD_THREADS = 1024;
constexpr int PD_WAVES = PD_THREADS / 64;
constexpr int PD_SCRATCH_BYTES = 512;
static_assert(SAPCU_PD_RESIDENT_CELLS <= 4 * PD_THREADS, "the cell scan takes four cells per thread");
static_assert(SAPCU_PD_RESIDENT_CELLS <= 4096 && SAPCU_PD_RESIDENT_MAX <= 8192, "a cell key has 12 bits, a row 13");

// states of a candidate; PD_FRESH marks a decision of the running round, which the round's readers take as undecided
constexpr int PD_UNDECIDED = 0, PD_ACCEPTED = 1, PD_REJECTED = 2, PD_FRESH = 4, PD_STATE_MASK = 7;
constexpr int PD_KEY_SHIFT = 3, PD_KEY_MASK = 4095, PD_ROW_SHIFT = 15, PD_SORT_ROW_BITS = 13;
constexpr int PD_CSTART_INTS = SAPCU_PD_RESIDENT_CELLS + 64;          // cells + 1 entries, the next region 16-byte aligned
static_assert(4 * PD_CSTART_INTS >= SAPCU_PD_RESIDENT_MAX, "the kept flags of the compaction lie over the cell table");

static size_t pd_resident_lds_bytes(int64_t C) { return (size_t)16 * C + 4 * PD_CSTART_INTS + PD_SCRATCH_BYTES; }

// the smallest cell edge whose 27 neighbouring cells hold every conflict at the squared radius r2 (sapcu_poisson.h)
__host__ __device__ static inline double pd_cover(float r2) { return sqrt((double)r2 + 0x1p-140) * (1.0 + 0x1p-20); }

__device__ __forceinline__ float pd_dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// ---------------------------------------------------------------------------------------------------------- resident
// (the block scan and the block extremes are wave_ops.h's, over PD_WAVES wavefronts; their scratch is L.scr)
// One sorted slot is a float4 {x, y, z, word}: a candidate costs its reader ONE LDS read.  word = state in bits 0..2, the cell key
// in bits 3..14, the row (= priority) from bit 15 up; only the slot's owner writes it, a 32-bit store.
struct PdLds {
    float4* pt;                 // [C]: the slots, ordered by (cell key, row)
    int* cstart;                // [cells + 1]: counts, then the first slot of each cell, entry `cells` = C
    int* scr;                   // PD_SCRATCH_BYTES
    unsigned* sortbuf;          // [C rounded up to a power of two] the keys being sorted: aliases pt, dead before pt is filled
    uint8_t* kept;              // [C] in row order: aliases cstart, valid only after the last round
};

__device__ __forceinline__ int pd_word(const float4& p) { return __float_as_int(p.w); }
__device__ __forceinline__ void pd_set_word(float4* slot, int word) { reinterpret_cast<int*>(slot)[3] = word; }

struct PdBox {
    float lx, ly, lz, hx, hy, hz;
};

struct PdGrid {
    double h;
    int gx, gy, gz;
};

// the grid of the radius whose square is r2 over the box: edge >= pd_cover(r2), at most SAPCU_PD_RESIDENT_CELLS cells
__device__ __forceinline__ PdGrid pd_resident_grid(const PdBox& bx, float r2) {
    const double ex = (double)bx.hx - (double)bx.lx, ey = (double)bx.hy - (double)bx.ly, ez = (double)bx.hz - (double)bx.lz;
    const double emax = fmax(ex, fmax(ey, ez));
    PdGrid g;
    g.gx = g.gy = g.gz = 1;
    g.h = 1.0;
    if (!(emax > 0.0)) return g;                                       // every point equal: one cell
    double h = pd_cover(r2);
    const double floor_h = emax * (1.0 / SAPCU_PD_RESIDENT_CELLS);     // an axis of more cells than the cap cannot fit anyway
    if (!(h >= floor_h)) h = floor_h;                                  // also a NaN radius: nothing conflicts, any edge serves
    for (int it = 0; it < 256; ++it) {
        const double gx = floor(ex / h) + 1.0, gy = floor(ey / h) + 1.0, gz = floor(ez / h) + 1.0;
        if (gx * gy * gz <= (double)SAPCU_PD_RESIDENT_CELLS) {
            g.h = h;
            g.gx = (int)gx;
            g.gy = (int)gy;
            g.gz = (int)gz;
            return g;
        }
        h *= 1.125;
    }
    g.h = __builtin_huge_val();                                        // not reached (1.125^256 > 2^43): one cell is always right
    return g;
}

__device__ __forceinline__ int pd_cell(float v, float o, double h, int g) {
    const double t = floor(((double)v - (double)o) / h);
    return t < 0.0 ? 0 : (t >= (double)(g - 1) ? g - 1 : (int)t);
}

// select(P, r) of one entry by the whole work group: the states are left in L.pt, the number kept is returned to every thread.
// The slots of a cell are in ROW order (a bitonic sort of key << 13 | row): greedy keeps low rows, so a scan meets the accepted
// candidates of a cell first and a rejection is found after a few candidates even where a cell holds the whole cloud.
__device__ int pd_resident_select(const float* __restrict__ P, int C, int n2, const PdBox& bx, float r, const PdLds& L, int* rounds) {
    const int tid = threadIdx.x;
    const float r2 = __fmul_rn(r, r);
    const PdGrid g = pd_resident_grid(bx, r2);
    const int cells = g.gx * g.gy * g.gz;
    for (int c = tid; c <= cells; c += PD_THREADS) L.cstart[c] = 0;
    __syncthreads();
    for (int i = tid; i < n2; i += PD_THREADS) {
        unsigned comp = 0xffffffffu;                                     // padding sorts behind every slot
        if (i < C) {
            const int cx = pd_cell(P[i * 3 + 0], bx.lx, g.h, g.gx);
            const int cy = pd_cell(P[i * 3 + 1], bx.ly, g.h, g.gy);
            const int cz = pd_cell(P[i * 3 + 2], bx.lz, g.h, g.gz);
            const int key = (cz * g.gy + cy) * g.gx + cx;
            atomicAdd(&L.cstart[key], 1);
            comp = (unsigned)key << PD_SORT_ROW_BITS | (unsigned)i;
        }
        L.sortbuf[i] = comp;
    }
    __syncthreads();
    {
        int v[4], s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = tid * 4 + j;
            v[j] = c < cells ? L.cstart[c] : 0;
            s += v[j];
        }
        int total;
        int run = block_excl_scan<PD_WAVES>(s, L.scr, &total);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = tid * 4 + j;
            if (c < cells) L.cstart[c] = run;
            run += v[j];
        }
        if (tid == 0) L.cstart[cells] = total;                           // = C
    }
    for (int k = 2; k <= n2; k <<= 1) {                                  // bitonic sort, ascending; n2 is a power of two
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = tid; i < n2; i += PD_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned a = L.sortbuf[i], b = L.sortbuf[l];
                    if ((a > b) == ((i & k) == 0)) {
                        L.sortbuf[i] = b;
                        L.sortbuf[l] = a;
                    }
                }
            }
        }
    }
    __syncthreads();
    // sortbuf lies over the first slots: the chunks of PD_THREADS slots are filled from the last one down, so that the slots of
    // chunk k (bytes from 16 k PD_THREADS) only cover keys of chunks >= 4 k, which are consumed; its own keys are read before the barrier
    for (int k = (C - 1) / PD_THREADS; k >= 0; --k) {
        const int s = tid + k * PD_THREADS;
        const unsigned comp = s < C ? L.sortbuf[s] : 0u;
        __syncthreads();
        if (s < C) {
            const int row = (int)(comp & ((1u << PD_SORT_ROW_BITS) - 1)), key = (int)(comp >> PD_SORT_ROW_BITS);
            L.pt[s] = make_float4(P[row * 3 + 0], P[row * 3 + 1], P[row * 3 + 2],
                                  __int_as_float(row << PD_ROW_SHIFT | key << PD_KEY_SHIFT | PD_UNDECIDED));
        }
    }
    __syncthreads();

    int done_rounds = 0;
    for (int round = 0; round < C; ++round) {
        int pending = 0;
#pragma unroll 1
        for (int s = tid; s < C; s += PD_THREADS) {
            const float4 p = L.pt[s];
            const int word = pd_word(p);
            if ((word & PD_STATE_MASK) != PD_UNDECIDED) continue;
            const int me = word >> PD_ROW_SHIFT, cell = (word >> PD_KEY_SHIFT) & PD_KEY_MASK;
            const int cx = cell % g.gx, cyz = cell / g.gx, cy = cyz % g.gy, cz = cyz / g.gy;
            const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.gx - 1);
            bool hit = false, wait = false, stop = false;
            for (int zz = max(cz - 1, 0); zz <= min(cz + 1, g.gz - 1) && !stop; ++zz) {
                for (int yy = max(cy - 1, 0); yy <= min(cy + 1, g.gy - 1) && !stop; ++yy) {
                    const int row = (zz * g.gy + yy) * g.gx;               // the cells of a row are consecutive: one slot range
                    const int a = L.cstart[row + x0], b = L.cstart[row + x1 + 1];
                    for (int t = a; t < b; ++t) {
                        const float4 q = L.pt[t];
                        const int other = pd_word(q), st = other & PD_STATE_MASK;
                        if ((other >> PD_ROW_SHIFT) >= me || st == PD_REJECTED) continue;
                        if (wait && st != PD_ACCEPTED) continue;           // already waiting: only an accepted candidate matters
                        if (!(pd_dist2(p.x, p.y, p.z, q.x, q.y, q.z) < r2)) continue;
                        if (st == PD_ACCEPTED) {
                            hit = stop = true;
                            break;
                        }
                        wait = true;                                       // undecided, or decided only in this round
                        if (round == 0) {                                  // nothing is accepted yet: no rejection to look for
                            stop = true;
                            break;
                        }
                    }
                }
            }
            if (hit) pd_set_word(&L.pt[s], word | PD_REJECTED | PD_FRESH);
            else if (!wait) pd_set_word(&L.pt[s], word | PD_ACCEPTED | PD_FRESH);
            else pending = 1;
        }
        ++done_rounds;
        __syncthreads();
        for (int s = tid; s < C; s += PD_THREADS) {
            const int word = pd_word(L.pt[s]);
            if (word & PD_FRESH) pd_set_word(&L.pt[s], word & ~PD_FRESH);
        }
        if (!__syncthreads_or(pending)) break;
    }
    *rounds += done_rounds;
    int mine = 0;
    for (int s = tid; s < C; s += PD_THREADS) mine += (pd_word(L.pt[s]) & PD_STATE_MASK) == PD_ACCEPTED;
    int total;
    block_excl_scan<PD_WAVES>(mine, L.scr, &total);
    return total;
}

// steps < 0: select at radius_in[entry] -> keep_out, count_out, rounds_out.  steps >= 0: subsample to n -> idx_out, radius_out,
// count_out, rounds_out.  Dynamic LDS: pd_resident_lds_bytes(C).
__global__ __launch_bounds__(PD_THREADS) void pd_resident_kernel(const float* __restrict__ points, int C, const float* __restrict__ radius_in,
                                                                 int n, int steps, uint8_t* __restrict__ keep_out,
                                                                 int32_t* __restrict__ idx_out, float* __restrict__ radius_out,
                                                                 int32_t* __restrict__ count_out, int32_t* __restrict__ rounds_out) {
    extern __shared__ __align__(16) unsigned char pd_lds[];
    PdLds L;
    L.pt = reinterpret_cast<float4*>(pd_lds);
    L.cstart = reinterpret_cast<int*>(L.pt + C);
    L.scr = L.cstart + PD_CSTART_INTS;
    L.sortbuf = reinterpret_cast<unsigned*>(pd_lds);
    L.kept = reinterpret_cast<uint8_t*>(L.cstart);
    const int tid = threadIdx.x;
    const int64_t e = blockIdx.x;
    const float* __restrict__ P = points + e * C * 3;
    int n2 = 1;
    while (n2 < C) n2 <<= 1;

    // the bounding box, and whether every coordinate is finite
    const float INF = __builtin_huge_valf();
    float lx = INF, ly = INF, lz = INF, hx = -INF, hy = -INF, hz = -INF, bad = 0.f;
    for (int i = tid; i < C; i += PD_THREADS) {
        const float x = P[i * 3 + 0], y = P[i * 3 + 1], z = P[i * 3 + 2];
        if (!(fabsf(x) < INF && fabsf(y) < INF && fabsf(z) < INF)) bad = 1.f;
        lx = fminf(lx, x);
        ly = fminf(ly, y);
        lz = fminf(lz, z);
        hx = fmaxf(hx, x);
        hy = fmaxf(hy, y);
        hz = fmaxf(hz, z);
    }
    float* fscr = reinterpret_cast<float*>(L.scr);
    lx = block_min<PD_WAVES>(lx, fscr);
    ly = block_min<PD_WAVES>(ly, fscr);
    lz = block_min<PD_WAVES>(lz, fscr);
    hx = block_max<PD_WAVES>(hx, fscr);
    hy = block_max<PD_WAVES>(hy, fscr);
    hz = block_max<PD_WAVES>(hz, fscr);
    bad = block_max<PD_WAVES>(bad, fscr);
    const PdBox bx{lx, ly, lz, hx, hy, hz};

    if (bad != 0.f) {                                                    // a box that is not finite keeps nothing (uniform branch)
        if (steps < 0)
            for (int i = tid; i < C; i += PD_THREADS) keep_out[e * C + i] = 0;
        else
            for (int i = tid; i < n; i += PD_THREADS) idx_out[e * n + i] = -1;
        if (tid == 0) {
            count_out[e] = 0;
            rounds_out[e] = 0;
            if (steps >= 0) radius_out[e] = 0.f;
        }
        return;
    }

    int rounds = 0;
    float r;
    if (steps < 0) {
        r = radius_in[e];
    } else {
        const float ex = __fsub_rn(bx.hx, bx.lx), ey = __fsub_rn(bx.hy, bx.ly), ez = __fsub_rn(bx.hz, bx.lz);
        float lo = 0.f;
        float hi = (float)sqrt_cr((double)__fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez)));
        for (int s = 0; s < steps; ++s) {
            const float mid = __fmul_rn(0.5f, __fadd_rn(lo, hi));
            if (pd_resident_select(P, C, n2, bx, mid, L, &rounds) >= n) lo = mid; else hi = mid;
        }
        r = lo;
    }
    const int count = pd_resident_select(P, C, n2, bx, r, L, &rounds);
    if (tid == 0) {
        count_out[e] = count;
        rounds_out[e] = rounds;
        if (steps >= 0) radius_out[e] = r;
    }
    if (steps < 0) {
        for (int s = tid; s < C; s += PD_THREADS) {
            const int word = pd_word(L.pt[s]);
            keep_out[e * C + (word >> PD_ROW_SHIFT)] = (word & PD_STATE_MASK) == PD_ACCEPTED;
        }
        return;
    }
    // the first n kept rows in ascending order: the flags in row order (over the cell table, which is done), then a scan
    for (int s = tid; s < C; s += PD_THREADS) {
        const int word = pd_word(L.pt[s]);
        L.kept[word >> PD_ROW_SHIFT] = (word & PD_STATE_MASK) == PD_ACCEPTED;
    }
    __syncthreads();
    const int per = (C + PD_THREADS - 1) / PD_THREADS, first = tid * per;
    int mine = 0;
    for (int i = first; i < min(first + per, C); ++i) mine += L.kept[i];
    int total;
    int pos = block_excl_scan<PD_WAVES>(mine, L.scr, &total);
    for (int i = first; i < min(first + per, C); ++i) {
        if (!L.kept[i]) continue;
        if (pos < n) idx_out[e * n + pos] = i;
        ++pos;
    }
}

// -------------------------------------------------------------------------------------------------------------- grid
__global__ __launch_bounds__(256) void pd_widen_kernel(const float* __restrict__ src, int64_t count, double* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) dst[i] = (double)src[i];
}

// one synchronous round over the sorted slots: state_in is only read, state_out written for every slot; *undecided counts the
// slots the round leaves undecided
__global__ __launch_bounds__(256) void pd_grid_round_kernel(int64_t n, const GridParams* __restrict__ prm, const int* __restrict__ start,
                                                            const int* __restrict__ key, const double* __restrict__ sx,
                                                            const double* __restrict__ sy, const double* __restrict__ sz,
                                                            const int* __restrict__ sidx, float r2, const uint8_t* __restrict__ state_in,
                                                            uint8_t* __restrict__ state_out, int* __restrict__ undecided) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int st = PD_REJECTED;
    if (s < n) {
        st = state_in[s];
        if (st == PD_UNDECIDED) {
            const int gx = prm->gx, gy = prm->gy, gz = prm->gz;
            const int me = sidx[s], cell = key[me];
            const float x = (float)sx[s], y = (float)sy[s], z = (float)sz[s];   // f32 values widened: the conversion back is exact
            const int cx = cell % gx, cyz = cell / gx, cy = cyz % gy, cz = cyz / gy;
            const int x0 = max(cx - 1, 0), x1 = min(cx + 1, gx - 1);
            bool hit = false, wait = false;
            for (int zz = max(cz - 1, 0); zz <= min(cz + 1, gz - 1) && !hit; ++zz) {
                for (int yy = max(cy - 1, 0); yy <= min(cy + 1, gy - 1) && !hit; ++yy) {
                    const int row = (zz * gy + yy) * gx;
                    const int a = start[row + x0], b = start[row + x1 + 1];
                    for (int t = a; t < b; ++t) {
                        if (sidx[t] >= me) continue;
                        if (!(pd_dist2(x, y, z, (float)sx[t], (float)sy[t], (float)sz[t]) < r2)) continue;
                        const int other = state_in[t];
                        if (other == PD_ACCEPTED) {
                            hit = true;
                            break;
                        }
                        if (other != PD_REJECTED) wait = true;
                    }
                }
            }
            st = hit ? PD_REJECTED : (wait ? PD_UNDECIDED : PD_ACCEPTED);
        }
        state_out[s] = (uint8_t)st;
    }
    const unsigned long long left = __ballot(st == PD_UNDECIDED);
    if ((threadIdx.x & 63) == 0 && left) atomicAdd(undecided, __popcll(left));
}

// the states of the sorted slots -> flags in row order (u8 and / or int, either may be NULL) and their number
__global__ __launch_bounds__(256) void pd_grid_finish_kernel(int64_t n, const int* __restrict__ sidx, const uint8_t* __restrict__ state,
                                                             uint8_t* __restrict__ keep8, int* __restrict__ keep32, int* __restrict__ count) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool kept = false;
    if (s < n) {
        kept = state[s] == PD_ACCEPTED;
        if (keep8) keep8[sidx[s]] = kept;
        if (keep32) keep32[sidx[s]] = kept;
    }
    const unsigned long long m = __ballot(kept);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, __popcll(m));
}

__global__ __launch_bounds__(256) void pd_fill_kernel(uint8_t* __restrict__ keep8, int64_t n8, int32_t* __restrict__ idx, int64_t n32) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (keep8 && i < n8) keep8[i] = 0;
    if (idx && i < n32) idx[i] = -1;
}

// scan[0 .. n]: the exclusive scan of the row-order flags (entry n = their number): the first `want` kept rows, ascending
__global__ __launch_bounds__(256) void pd_grid_compact_kernel(int64_t n, const int* __restrict__ scan, int64_t want, int32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int pos = scan[i];
    if (scan[i + 1] != pos && pos < want) idx[pos] = (int32_t)i;
}

struct PdGridWs {
    GridWs grid;
    double* pts;             // [3 C] the entry's coordinates, widened
    uint8_t *state_a, *state_b;   // [C] each, by sorted slot
    uint8_t* keep8;          // [C] by row
    int* keep32;             // [C + 1] by row, then its scan
    int* tile_sums;
    int* undecided;          // [SAPCU_PD_GRID_CHUNK]
    int* count;              // [1]
    size_t bytes;
};

static PdGridWs pd_grid_layout(void* base, int64_t C) {
    PdGridWs w;
    w.grid = grid_ws_layout(base, C);
    WsCarver c(base ? (char*)base + w.grid.bytes : nullptr);
    w.pts = c.take<double>(3 * C);
    w.state_a = c.take<uint8_t>(C);
    w.state_b = c.take<uint8_t>(C);
    w.keep8 = c.take<uint8_t>(C);
    w.keep32 = c.take<int>(C + 1);
    w.tile_sums = c.take<int>((C + 1 + SCAN_TILE - 1) / SCAN_TILE);
    w.undecided = c.take<int>(SAPCU_PD_GRID_CHUNK);
    w.count = c.take<int>(1);
    w.bytes = w.grid.bytes + c.bytes();
    return w;
}

static inline unsigned pd_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// select(P, r) of the entry whose widened coordinates are in w.pts: keep8 / keep32 (either may be NULL) get the flags in row order;
// *bad: the box is not finite, nothing was written.  Synchronises st: once for the grid, once per chunk of rounds, once at the end.
static int pd_grid_select(int64_t C, float r, int chunk, const PdGridWs& w, uint8_t* keep8, int* keep32, int* count, int* rounds,
                          bool* bad, hipStream_t st) {
    const float r2 = r * r;
    const double cover = pd_cover(r2);
    GridParams hp;
    int rc = launch_grid_setup(w.pts, C, 1, cover == cover ? cover : 0.0, w.grid, &hp, st);   // a NaN radius: nothing conflicts, any edge serves
    if (rc != SAPCU_OK) return rc;
    *bad = hp.fallback != 0;
    *count = 0;
    if (*bad) return SAPCU_OK;
    rc = launch_grid_sort(w.pts, C, w.grid, hp, st);
    if (rc != SAPCU_OK) return rc;
    uint8_t *in = w.state_a, *out = w.state_b;
    SAPCU_CHECK_HIP(hipMemsetAsync(in, PD_UNDECIDED, (size_t)C, st));
    int left[SAPCU_PD_GRID_CHUNK];
    bool done = false;
    int ran = 0;
    for (int64_t round = 0; round < C && !done; round += chunk) {
        const int m = (int)(C - round < chunk ? C - round : chunk);
        SAPCU_CHECK_HIP(hipMemsetAsync(w.undecided, 0, sizeof(int) * m, st));
        for (int k = 0; k < m; ++k) {                                       // rounds after the last undecided slot copy the states
            hipLaunchKernelGGL(pd_grid_round_kernel, dim3(pd_blocks(C)), dim3(256), 0, st, C, w.grid.params, w.grid.start, w.grid.key,
                               w.grid.sx, w.grid.sy, w.grid.sz, w.grid.sidx, r2, in, out, w.undecided + k);
            SAPCU_CHECK_LAUNCH();
            uint8_t* t = in;
            in = out;
            out = t;
        }
        SAPCU_CHECK_HIP(hipMemcpyAsync(left, w.undecided, sizeof(int) * m, hipMemcpyDeviceToHost, st));
        SAPCU_CHECK_HIP(hipStreamSynchronize(st));
        for (int k = 0; k < m && !done; ++k) {
            ++ran;
            done = left[k] == 0;
        }
    }
    if (!done) {
        set_error("poisson: %d rounds left candidates undecided", ran);
        return SAPCU_ERR_LIMIT;
    }
    *rounds += ran;
    SAPCU_CHECK_HIP(hipMemsetAsync(w.count, 0, sizeof(int), st));
    hipLaunchKernelGGL(pd_grid_finish_kernel, dim3(pd_blocks(C)), dim3(256), 0, st, C, w.grid.sidx, in, keep8, keep32, w.count);
    SAPCU_CHECK_LAUNCH();
    SAPCU_CHECK_HIP(hipMemcpyAsync(count, w.count, sizeof(int), hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    return SAPCU_OK;
}

static int pd_widen(const float* P, int64_t C, const PdGridWs& w, hipStream_t st) {
    hipLaunchKernelGGL(pd_widen_kernel, dim3(pd_blocks(3 * C)), dim3(256), 0, st, P, 3 * C, w.pts);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

static int pd_select_grid(const float* points, int64_t b, int64_t C, const float* radius, uint8_t* keep_out, int32_t* count_out,
                          int32_t* rounds_out, int chunk, const PdGridWs& w, hipStream_t st) {
    std::vector<float> r(b);
    std::vector<int32_t> count(b, 0), rounds(b, 0);
    SAPCU_CHECK_HIP(hipMemcpyAsync(r.data(), radius, sizeof(float) * b, hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    for (int64_t e = 0; e < b; ++e) {
        int rc = pd_widen(points + e * C * 3, C, w, st);
        if (rc != SAPCU_OK) return rc;
        bool bad = false;
        rc = pd_grid_select(C, r[e], chunk, w, keep_out + e * C, nullptr, &count[e], &rounds[e], &bad, st);
        if (rc != SAPCU_OK) return rc;
        if (bad) {
            hipLaunchKernelGGL(pd_fill_kernel, dim3(pd_blocks(C)), dim3(256), 0, st, keep_out + e * C, C, (int32_t*)nullptr, (int64_t)0);
            SAPCU_CHECK_LAUNCH();
        }
    }
    SAPCU_CHECK_HIP(hipMemcpyAsync(count_out, count.data(), sizeof(int32_t) * b, hipMemcpyHostToDevice, st));
    SAPCU_CHECK_HIP(hipMemcpyAsync(rounds_out, rounds.data(), sizeof(int32_t) * b, hipMemcpyHostToDevice, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    return SAPCU_OK;
}

static int pd_subsample_grid(const float* points, int64_t b, int64_t C, int64_t n, int steps, int32_t* idx_out, float* radius_out,
                             int32_t* count_out, int32_t* rounds_out, const PdGridWs& w, hipStream_t st) {
    std::vector<float> radius(b, 0.f);
    std::vector<int32_t> count(b, 0), rounds(b, 0);
    std::vector<double> part(8 * KNN_GRID_BBOX_BLOCKS);
    for (int64_t e = 0; e < b; ++e) {
        int rc = pd_widen(points + e * C * 3, C, w, st);
        if (rc != SAPCU_OK) return rc;
        rc = launch_grid_bbox(w.pts, C, w.grid.partials, st);
        if (rc != SAPCU_OK) return rc;
        SAPCU_CHECK_HIP(hipMemcpyAsync(part.data(), w.grid.partials, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st));
        SAPCU_CHECK_HIP(hipStreamSynchronize(st));
        double box[7] = {HUGE_VAL, HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL, 0.0};
        for (int k = 0; k < KNN_GRID_BBOX_BLOCKS; ++k)
            for (int c = 0; c < 7; ++c) box[c] = c < 3 ? fmin(box[c], part[k * 8 + c]) : fmax(box[c], part[k * 8 + c]);
        bool bad = box[6] != 0.0;
        int cnt = 0;
        float lo = 0.f;
        if (!bad) {
            const float ex = (float)box[3] - (float)box[0], ey = (float)box[4] - (float)box[1], ez = (float)box[5] - (float)box[2];
            const float d2 = (ex * ex + ey * ey) + ez * ez;
            float hi = sqrtf(d2);
            for (int s = 0; s < steps && !bad; ++s) {
                const float mid = 0.5f * (lo + hi);
                rc = pd_grid_select(C, mid, SAPCU_PD_GRID_CHUNK, w, nullptr, nullptr, &cnt, &rounds[e], &bad, st);
                if (rc != SAPCU_OK) return rc;
                if (cnt >= n) lo = mid; else hi = mid;
            }
            if (!bad) {
                rc = pd_grid_select(C, lo, SAPCU_PD_GRID_CHUNK, w, nullptr, w.keep32, &cnt, &rounds[e], &bad, st);
                if (rc != SAPCU_OK) return rc;
            }
        }
        if (bad) {
            rounds[e] = 0;
            hipLaunchKernelGGL(pd_fill_kernel, dim3(pd_blocks(n)), dim3(256), 0, st, (uint8_t*)nullptr, (int64_t)0, idx_out + e * n, n);
            SAPCU_CHECK_LAUNCH();
            continue;
        }
        radius[e] = lo;
        count[e] = cnt;
        SAPCU_CHECK_HIP(hipMemsetAsync(w.keep32 + C, 0, sizeof(int), st));
        rc = launch_exclusive_scan_int(w.keep32, C + 1, w.tile_sums, st);
        if (rc != SAPCU_OK) return rc;
        hipLaunchKernelGGL(pd_grid_compact_kernel, dim3(pd_blocks(C)), dim3(256), 0, st, C, w.keep32, n, idx_out + e * n);
        SAPCU_CHECK_LAUNCH();
    }
    SAPCU_CHECK_HIP(hipMemcpyAsync(radius_out, radius.data(), sizeof(float) * b, hipMemcpyHostToDevice, st));
    SAPCU_CHECK_HIP(hipMemcpyAsync(count_out, count.data(), sizeof(int32_t) * b, hipMemcpyHostToDevice, st));
    SAPCU_CHECK_HIP(hipMemcpyAsync(rounds_out, rounds.data(), sizeof(int32_t) * b, hipMemcpyHostToDevice, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    return SAPCU_OK;
}

static DeviceOnce pd_resident_once;

static int pd_launch_resident(const float* points, int64_t b, int64_t C, const float* radius, int64_t n, int steps, uint8_t* keep,
                              int32_t* idx, float* radius_out, int32_t* count, int32_t* rounds, hipStream_t st) {
    SAPCU_SET_MAX_LDS(pd_resident_once, pd_resident_kernel, (int)pd_resident_lds_bytes(SAPCU_PD_RESIDENT_MAX));
    hipLaunchKernelGGL(pd_resident_kernel, dim3((unsigned)b), dim3(PD_THREADS), pd_resident_lds_bytes(C), st, points, (int)C, radius, (int)n,
                       steps, keep, idx, radius_out, count, rounds);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

static bool pd_sizes_ok(int64_t b, int64_t C) { return b >= 0 && b <= SAPCU_PD_MAX_B && C >= 1 && C <= SAPCU_PD_MAX_C; }

// the checks both entry points and the test hook share; *w: the layout over the aligned workspace
static int pd_check(const char* who, int64_t b, int64_t C, void* workspace, int64_t workspace_bytes, PdGridWs* w) {
    SAPCU_CHECK_ARG(b >= 0 && b <= SAPCU_PD_MAX_B, "%s: need 0 <= b <= %d (b=%lld)", who, SAPCU_PD_MAX_B, (long long)b);
    SAPCU_CHECK_ARG(C >= 1 && C <= SAPCU_PD_MAX_C, "%s: need 1 <= C <= 2^24 (C=%lld)", who, (long long)C);
    SAPCU_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0, "%s: a NULL or misaligned workspace", who);
    *w = pd_grid_layout(ws_align256(workspace), C);
    if (workspace_bytes < (int64_t)w->bytes + 256) {
        set_error("%s: workspace of %lld bytes, need %lld", who, (long long)workspace_bytes, (long long)w->bytes + 256);
        return SAPCU_ERR_WORKSPACE;
    }
    return SAPCU_OK;
}

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

extern "C" {

int64_t sapcu_poisson_workspace_bytes(int64_t b, int64_t C) {
    if (!pd_sizes_ok(b, C)) return -1;
    return (int64_t)pd_grid_layout(nullptr, C).bytes + 256;
}

int sapcu_poisson_select_f32(const float* points, int64_t b, int64_t C, const float* radius, uint8_t* keep_out, int32_t* count_out,
                             int32_t* rounds_out, void* workspace, int64_t workspace_bytes, void* stream) {
    PdGridWs w;
    const int rc = pd_check("poisson_select", b, C, workspace, workspace_bytes, &w);
    if (rc != SAPCU_OK) return rc;
    SAPCU_CHECK_ARG(points && radius && keep_out && count_out && rounds_out, "poisson_select: null pointer");
    if (b == 0) return SAPCU_OK;
    if (C <= SAPCU_PD_RESIDENT_MAX)
        return pd_launch_resident(points, b, C, radius, 0, -1, keep_out, nullptr, nullptr, count_out, rounds_out, (hipStream_t)stream);
    return pd_select_grid(points, b, C, radius, keep_out, count_out, rounds_out, SAPCU_PD_GRID_CHUNK, w, (hipStream_t)stream);
}

int sapcu_poisson_subsample_f32(const float* points, int64_t b, int64_t C, int64_t n, int steps, int32_t* idx_out, float* radius_out,
                                int32_t* count_out, int32_t* rounds_out, void* workspace, int64_t workspace_bytes, void* stream) {
    PdGridWs w;
    const int rc = pd_check("poisson_subsample", b, C, workspace, workspace_bytes, &w);
    if (rc != SAPCU_OK) return rc;
    SAPCU_CHECK_ARG(n >= 1 && n <= C, "poisson_subsample: need 1 <= n <= C (n=%lld, C=%lld)", (long long)n, (long long)C);
    SAPCU_CHECK_ARG(steps >= 0 && steps <= SAPCU_PD_MAX_STEPS, "poisson_subsample: need 0 <= steps <= %d (steps=%d)", SAPCU_PD_MAX_STEPS, steps);
    SAPCU_CHECK_ARG(points && idx_out && radius_out && count_out && rounds_out, "poisson_subsample: null pointer");
    if (b == 0) return SAPCU_OK;
    if (C <= SAPCU_PD_RESIDENT_MAX)
        return pd_launch_resident(points, b, C, nullptr, n, steps, nullptr, idx_out, radius_out, count_out, rounds_out, (hipStream_t)stream);
    return pd_subsample_grid(points, b, C, n, steps, idx_out, radius_out, count_out, rounds_out, w, (hipStream_t)stream);
}

// test hook: sapcu_poisson_select_f32 on the grid path at any C, one round per chunk
int sapcu_internal_poisson_select_grid(const float* points, int64_t b, int64_t C, const float* radius, uint8_t* keep_out, int32_t* count_out,
                                       int32_t* rounds_out, void* workspace, int64_t workspace_bytes, void* stream) {
    PdGridWs w;
    const int rc = pd_check("poisson_select_grid", b, C, workspace, workspace_bytes, &w);
    if (rc != SAPCU_OK) return rc;
    SAPCU_CHECK_ARG(points && radius && keep_out && count_out && rounds_out, "poisson_select_grid: null pointer");
    if (b == 0) return SAPCU_OK;
    return pd_select_grid(points, b, C, radius, keep_out, count_out, rounds_out, 1, w, (hipStream_t)stream);
}

}  // extern "C"
