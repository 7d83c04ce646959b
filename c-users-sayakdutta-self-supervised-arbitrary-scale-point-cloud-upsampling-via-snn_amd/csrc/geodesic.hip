// Geodesic disks on a triangle mesh: the counts behind the uniformity figure (sapcu_amd/uniformity.py).  Replaces the per-seed
// CGAL Surface_mesh_shortest_path of the reference's evaluation.cpp.  The definition, the stages and the memory contract are in
// csrc/sapcu_geodesic.h, the definition in Python in tests/geodesic_ref.py.  All arithmetic is f64.
//
// Mesh tables (once per call, a few small kernels over half-edges, vertices and targets):
//   * half-edge h = 3 f + k runs from vertex k to vertex k+1 of face f.  geo_edge_insert_kernel claims the slot of the undirected
//     pair (lo, hi) in an open-addressing table with a 64-bit CAS and the pair's slot for its own direction with a 32-bit CAS;
//     a second claim of one direction is the non-manifold verdict.  geo_twin_kernel reads the other direction's slot.
//   * geo_vertex_kernel walks the fan of a vertex from its stored outgoing half-edge (a boundary one where there is one):
//     boundary flag, angle sum, pseudo-source flag.  The walk is bounded by 3 nf steps.
//   * the face -> targets table is a counting sort (atomic counts, a one-block scan, atomic cursors).
// geo_seed_kernel, 64 lanes = one wavefront per work group, work groups striding over the seeds.  Per seed, in LDS:
//   * a ring of QL window slots with a tag per slot (the queue position the slot holds); position p lives in LDS when fewer than
//     QL positions were queued at its push, else in the work group's ring of qg slots in the workspace: a pop finds it by the tag;
//   * a table of H (key, 64-bit distance) slots, key = vertex or nv + target, lowered with ds_min_u64 on the distance's bits
//     (distances are >= 0, so their bit patterns order like the numbers); a key that finds the table full goes to the work group's
//     dense table in the workspace (global 64-bit atomic min), which is +inf before every seed;
//   * counters.  Nothing in LDS or in the workspace is assumed initialised.
//   The lanes take up to 64 queue entries at a time; every entry is processed by one lane; children are pushed with one LDS atomic
//   on the tail.  The order in which lanes lower a distance is not fixed, so which of two windows survives a filter can differ from
//   run to run: the filters only drop windows that cannot carry a shortest path, the minimum is the same up to rounding.
//   The loop ends on "queue empty", on the window cap and on a queue past the workspace ring (header).
#include "common.h"
#include "sapcu_geodesic.h"
#include "wave_ops.h"

namespace sapcu {

constexpr int GEO_QL = SAPCU_GEODESIC_LDS_QUEUE, GEO_H = SAPCU_GEODESIC_LDS_TABLE, GEO_MAXR = SAPCU_GEODESIC_MAX_RADII;
constexpr int GEO_MAX_GROUPS = 512;
constexpr unsigned long long GEO_EMPTY = ~0ull;
constexpr unsigned long long GEO_INF_BITS = 0x7ff0000000000000ull;
constexpr double GEO_TWO_PI = 6.283185307179586476925286766559;
constexpr double GEO_FILTER_SLACK = 1e-12, GEO_EDGE_EPS = 1e-12;

struct GeoWin {        // a queue entry: a window entering the face of half-edge he >= 0, or the pseudo-source vertex -(he + 1)
    int he, pad;
    double sx, sy, lo, hi, sigma;
};

struct GeoCtl {        // device counters, zeroed by the call
    int bad_mesh;      // 1 duplicate direction, 2 zero-area face, 4 index out of range
    int n_boundary, n_pseudo, n_spilled, n_capped, n_overflow, peak;
    int pad;
    unsigned long long windows;
};

struct GeoRadii {
    double r[GEO_MAXR];
};

struct GeoWs {
    GeoCtl* ctl;
    unsigned long long* ekey;      // [tsize] undirected pair
    int* ehe;                      // [2 tsize] half-edge of the (lo -> hi) and of the (hi -> lo) direction
    int* twin;                     // [3 nf]
    int* vhe;                      // [nv]
    unsigned char* pseudo;         // [nv]
    int* fstart;                   // [nf + 1]
    int* fcur;                     // [nf]
    int* tlist;                    // [nq]
    GeoWin* gq;                    // [groups][qg]
    unsigned long long* gmap;      // [groups][nv + nq]
    int64_t tsize, qg, groups;
    size_t bytes;
};

static int64_t geo_groups(int64_t ns) { return ns < GEO_MAX_GROUPS ? (ns < 1 ? 1 : ns) : GEO_MAX_GROUPS; }

// the one layout of the workspace: the sizer calls it on a null base
static GeoWs geo_ws_layout(void* base, int64_t nv, int64_t nf, int64_t nq, int64_t ns) {
    GeoWs w;
    w.tsize = 64;
    while (w.tsize < 6 * nf) w.tsize <<= 1;
    w.qg = nf + 4096;
    w.groups = geo_groups(ns);
    WsCarver c(ws_align256(base));
    w.ctl = c.take<GeoCtl>(1);
    w.ekey = c.take<unsigned long long>(w.tsize);
    w.ehe = c.take<int>(2 * w.tsize);
    w.twin = c.take<int>(3 * nf);
    w.vhe = c.take<int>(nv);
    w.pseudo = c.take<unsigned char>(nv);
    w.fstart = c.take<int>(nf + 1);
    w.fcur = c.take<int>(nf);
    w.tlist = c.take<int>(nq > 0 ? nq : 1);
    w.gq = c.take<GeoWin>(w.groups * w.qg);
    w.gmap = c.take<unsigned long long>(w.groups * (nv + nq));
    w.bytes = c.bytes() + 256;
    return w;
}

static bool geo_sizes_ok(int64_t nv, int64_t nf, int64_t nq, int64_t ns, int64_t nr) {
    return nv >= 1 && nv <= (1 << 24) && nf >= 1 && nf <= (1 << 24) && nq >= 0 && nq <= (1 << 30) && ns >= 0 && ns <= (1 << 24) && nr >= 1 &&
           nr <= GEO_MAXR;
}

__device__ __forceinline__ unsigned long long geo_mix(unsigned long long x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

__device__ __forceinline__ double geo_hypot(double x, double y) { return sqrt(x * x + y * y); }
__device__ __forceinline__ double geo_dist3(const double* a, const double* b) {
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return sqrt((x * x + y * y) + z * z);
}

// ------------------------------------------------------------------------------------------------------- mesh tables
__global__ __launch_bounds__(256) void geo_init_kernel(GeoWs w, int64_t nv, int64_t nf) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < w.tsize; i += step) {
        w.ekey[i] = GEO_EMPTY;
        w.ehe[2 * i] = -1;
        w.ehe[2 * i + 1] = -1;
    }
    for (int64_t i = i0; i < nv; i += step) {
        w.vhe[i] = -1;
        w.pseudo[i] = 0;
    }
    for (int64_t i = i0; i <= nf; i += step) w.fstart[i] = 0;
}

__device__ __forceinline__ int64_t geo_edge_slot(const GeoWs& w, unsigned long long key, bool insert) {
    int64_t slot = (int64_t)(geo_mix(key) & (unsigned long long)(w.tsize - 1));
    for (int64_t probe = 0; probe < w.tsize; ++probe) {            // the table holds at most 3 nf <= tsize / 2 keys
        unsigned long long k = insert ? atomicCAS(&w.ekey[slot], GEO_EMPTY, key) : w.ekey[slot];
        if (k == key || (insert && k == GEO_EMPTY)) return slot;
        if (k == GEO_EMPTY) return -1;
        slot = (slot + 1) & (w.tsize - 1);
    }
    return -1;
}

__global__ __launch_bounds__(256) void geo_edge_insert_kernel(GeoWs w, const double* __restrict__ V, int nv, const int* __restrict__ F, int nf) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int v0 = F[3 * f], v1 = F[3 * f + 1], v2 = F[3 * f + 2];
    if (v0 < 0 || v0 >= nv || v1 < 0 || v1 >= nv || v2 < 0 || v2 >= nv) {
        atomicOr(&w.ctl->bad_mesh, 4);
        return;
    }
    const double* a = V + 3 * (int64_t)v0;
    const double* b = V + 3 * (int64_t)v1;
    const double* c = V + 3 * (int64_t)v2;
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2];
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const double nn = (nx * nx + ny * ny) + nz * nz;
    if (!(nn > 0.0 && nn < __builtin_huge_val())) {
        atomicOr(&w.ctl->bad_mesh, 2);
        return;
    }
    const int vs[4] = {v0, v1, v2, v0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int p = vs[k], q = vs[k + 1];
        const unsigned long long key = p < q ? ((unsigned long long)p << 32 | (unsigned)q) : ((unsigned long long)q << 32 | (unsigned)p);
        const int64_t slot = geo_edge_slot(w, key, true);
        if (slot < 0 || atomicCAS(&w.ehe[2 * slot + (p < q ? 0 : 1)], -1, 3 * f + k) != -1) atomicOr(&w.ctl->bad_mesh, 1);
    }
}

__global__ __launch_bounds__(256) void geo_twin_kernel(GeoWs w, const int* __restrict__ F, int nf) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= 3 * nf) return;
    const int f = h / 3, k = h - 3 * f;
    const int p = F[3 * f + k], q = F[3 * f + (k == 2 ? 0 : k + 1)];
    const unsigned long long key = p < q ? ((unsigned long long)p << 32 | (unsigned)q) : ((unsigned long long)q << 32 | (unsigned)p);
    const int64_t slot = geo_edge_slot(w, key, false);
    w.twin[h] = slot < 0 ? -1 : w.ehe[2 * slot + (p < q ? 1 : 0)];
    w.vhe[p] = h;                                                   // any outgoing half-edge; geo_boundary_kernel has the last word
}

__global__ __launch_bounds__(256) void geo_boundary_kernel(GeoWs w, const int* __restrict__ F, int nf) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= 3 * nf || w.twin[h] >= 0) return;
    w.vhe[F[h]] = h;                                                // F[3 f + k] is the start of h
    atomicAdd(&w.ctl->n_boundary, 1);
}

__global__ __launch_bounds__(256) void geo_vertex_kernel(GeoWs w, const double* __restrict__ V, int nv, const int* __restrict__ F, int nf) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const int h0 = w.vhe[v];
    if (h0 < 0) return;
    bool boundary = w.twin[h0] < 0;
    double sum = 0.0;
    int h = h0;
    for (int step = 0; step < 3 * nf; ++step) {
        const int f = h / 3, k = h - 3 * f;
        const int p = F[3 * f + (k + 1) % 3], q = F[3 * f + (k + 2) % 3];
        const double* a = V + 3 * (int64_t)v;
        const double* b = V + 3 * (int64_t)p;
        const double* c = V + 3 * (int64_t)q;
        const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2];
        const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        sum += atan2(sqrt((nx * nx + ny * ny) + nz * nz), (ux * wx + uy * wy) + uz * wz);
        const int t = w.twin[3 * f + (k + 2) % 3];                  // the half-edge q -> v; its twin leaves v in the next face
        if (t < 0) {
            boundary = true;
            break;
        }
        if (t == h0) break;
        h = t;
    }
    if (boundary || sum >= GEO_TWO_PI - 1e-9) {
        w.pseudo[v] = 1;
        atomicAdd(&w.ctl->n_pseudo, 1);
    }
}

__global__ __launch_bounds__(256) void geo_target_count_kernel(GeoWs w, const int64_t* __restrict__ tface, int nq, int nf) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq) return;
    const int64_t f = tface[t];
    if (f >= 0 && f < nf) atomicAdd(&w.fstart[f + 1], 1);
}

// exclusive scan of the counts in fstart[1 .. nf] in place (fstart[0] = 0), one work group; fcur = the starts
__global__ __launch_bounds__(1024) void geo_scan_kernel(GeoWs w, int nf) {
    __shared__ int scr[16];
    const int tid = threadIdx.x, chunk = (nf + 1023) / 1024;
    const int a = min(nf, tid * chunk), b = min(nf, a + chunk);
    int s = 0;
    for (int i = a; i < b; ++i) s += w.fstart[i + 1];
    int total;
    int run = block_excl_scan<16>(s, scr, &total);                  // targets of the faces before a
    for (int i = a; i < b; ++i) {
        const int c = w.fstart[i + 1];
        w.fcur[i] = run;
        run += c;
        w.fstart[i + 1] = run;
    }
}

__global__ __launch_bounds__(256) void geo_target_fill_kernel(GeoWs w, const int64_t* __restrict__ tface, int nq, int nf) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq) return;
    const int64_t f = tface[t];
    if (f >= 0 && f < nf) w.tlist[atomicAdd(&w.fcur[f], 1)] = t;
}

// ------------------------------------------------------------------------------------------------------- propagation
struct GeoShared {
    GeoWin q[GEO_QL];
    unsigned long long vals[GEO_H];
    int tag[GEO_QL];
    int keys[GEO_H];
    int counts[GEO_MAXR];
    int head, tail, spilled, err;
};

struct GeoSeed {       // what one work group carries through a seed
    GeoShared* S;
    int ql, H;                         // LDS capacities in use
    GeoWin* gq;
    int qg;
    unsigned long long* gmap;
    const double* V;
    const int* F;
    const int* twin;
    const int* vhe;
    const unsigned char* pseudo;
    const int* fstart;
    const int* tlist;
    const double* tpoint;
    int nv, nf;
    double limit;
};

// lower the distance of `key` to val; the value it held before (+inf for a new key)
__device__ __forceinline__ double geo_map_min(const GeoSeed& g, int key, double val) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(val);
    int slot = (int)(geo_mix((unsigned long long)key) & (unsigned long long)(g.H - 1));
    for (int probe = 0; probe < g.H; ++probe) {
        const int k = atomicCAS(&g.S->keys[slot], -1, key);
        if (k == -1 || k == key) return __longlong_as_double((long long)atomicMin(&g.S->vals[slot], bits));
        slot = (slot + 1) & (g.H - 1);
    }
    atomicOr(&g.S->spilled, 1);
    return __longlong_as_double((long long)atomicMin(&g.gmap[key], bits));
}

__device__ __forceinline__ double geo_map_get(const GeoSeed& g, int key) {
    int slot = (int)(geo_mix((unsigned long long)key) & (unsigned long long)(g.H - 1));
    volatile int* keys = g.S->keys;
    volatile unsigned long long* vals = g.S->vals;
    for (int probe = 0; probe < g.H; ++probe) {
        const int k = keys[slot];
        if (k == key) return __longlong_as_double((long long)vals[slot]);
        if (k == -1) return __builtin_huge_val();                   // a hole: the key was never stored (a full table has none)
        slot = (slot + 1) & (g.H - 1);
    }
    return __longlong_as_double((long long)__hip_atomic_load(&g.gmap[key], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

__device__ __forceinline__ void geo_push(const GeoSeed& g, const GeoWin& w) {
    const int pos = atomicAdd(&g.S->tail, 1);
    const int ahead = pos - *(volatile int*)&g.S->head;             // the head stands still while a batch is processed
    if (ahead < g.ql) {
        const int slot = pos % g.ql;
        g.S->q[slot] = w;
        g.S->tag[slot] = pos;
    } else if (ahead < g.qg) {
        atomicOr(&g.S->spilled, 1);
        g.gq[pos % g.qg] = w;
    } else {
        atomicOr(&g.S->err, 2);
    }
}

__device__ __forceinline__ void geo_push_window(const GeoSeed& g, int he, double sx, double sy, double lo, double hi, double sigma) {
    const double near = sx < lo ? geo_hypot(sx - lo, sy) : (sx > hi ? geo_hypot(sx - hi, sy) : -sy);
    if (!(sigma + near <= g.limit)) return;
    geo_push(g, GeoWin{he, 0, sx, sy, lo, hi, sigma});
}

__device__ __forceinline__ void geo_update_vertex(const GeoSeed& g, int v, double val) {
    if (!(val <= g.limit)) return;
    const double old = geo_map_min(g, v, val);
    if (val < old && g.pseudo[v]) geo_push(g, GeoWin{-(v + 1), 0, 0.0, 0.0, 0.0, 0.0, val});
}

// the unfolded frame of half-edge h: a at the origin, b at (L, 0), c at (cx, cy > 0); ex, ey its axes in space
struct GeoFrame {
    int a, b, c;
    double ax, ay, az, exx, exy, exz, eyx, eyy, eyz, L, cx, cy;
};

__device__ __forceinline__ GeoFrame geo_frame(const GeoSeed& g, int h) {
    GeoFrame r;
    const int f = h / 3, k = h - 3 * f;
    r.a = g.F[3 * f + k];
    r.b = g.F[3 * f + (k + 1) % 3];
    r.c = g.F[3 * f + (k + 2) % 3];
    const double* A = g.V + 3 * (int64_t)r.a;
    const double* B = g.V + 3 * (int64_t)r.b;
    const double* C = g.V + 3 * (int64_t)r.c;
    r.ax = A[0], r.ay = A[1], r.az = A[2];
    const double ux = B[0] - r.ax, uy = B[1] - r.ay, uz = B[2] - r.az, wx = C[0] - r.ax, wy = C[1] - r.ay, wz = C[2] - r.az;
    r.L = sqrt((ux * ux + uy * uy) + uz * uz);
    r.exx = ux / r.L, r.exy = uy / r.L, r.exz = uz / r.L;
    r.cx = (wx * r.exx + wy * r.exy) + wz * r.exz;
    const double px = wx - r.cx * r.exx, py = wy - r.cx * r.exy, pz = wz - r.cx * r.exz;
    r.cy = sqrt((px * px + py * py) + pz * pz);
    r.eyx = px / r.cy, r.eyy = py / r.cy, r.eyz = pz / r.cy;
    return r;
}

__device__ __forceinline__ double geo_edge_length(const GeoSeed& g, int h) {
    const int f = h / 3, k = h - 3 * f;
    return geo_dist3(g.V + 3 * (int64_t)g.F[3 * f + k], g.V + 3 * (int64_t)g.F[3 * f + (k + 1) % 3]);
}

// the part [l, r] of a window of the frame `fr` leaves through the far edge from o = (ox, oy) to e = (ex, ey) (the face's own
// direction) into the twin t2, whose frame has e at the origin and o at (L2, 0)
__device__ __forceinline__ void geo_child(const GeoSeed& g, int t2, double ox, double oy, double ex, double ey, double sx, double sy, double l,
                                          double r, double sigma, bool l_at_origin, bool r_at_end) {
    if (t2 < 0) return;
    const double L2 = geo_edge_length(g, t2);
    double ux = ex - ox, uy = ey - oy;
    const double n = geo_hypot(ux, uy);
    ux /= n, uy /= n;
    // a point p of the old frame in the twin's frame: x' = L2 - (p - o).u, y' = -(p - o) x u
    const double qsx = sx - ox, qsy = sy - oy;
    const double s2x = L2 - (qsx * ux + qsy * uy), s2y = -(-uy * qsx + ux * qsy);
    if (!(s2y < 0.0)) return;
    double nl, nr;
    {
        const double qx = l - ox, qy = -oy;
        const double px = L2 - (qx * ux + qy * uy), py = -(-uy * qx + ux * qy), den = py - s2y;
        nl = l_at_origin ? 0.0 : (den <= 0.0 ? px : s2x + (px - s2x) * (-s2y) / den);
    }
    {
        const double qx = r - ox, qy = -oy;
        const double px = L2 - (qx * ux + qy * uy), py = -(-uy * qx + ux * qy), den = py - s2y;
        nr = r_at_end ? L2 : (den <= 0.0 ? px : s2x + (px - s2x) * (-s2y) / den);
    }
    nl = fmin(fmax(nl, 0.0), L2);
    nr = fmin(fmax(nr, 0.0), L2);
    if (!(nr - nl > 0.1 * GEO_EDGE_EPS * L2)) return;
    geo_push_window(g, t2, s2x, s2y, nl, nr, sigma);
}

__device__ __forceinline__ void geo_process_vertex(const GeoSeed& g, int v, double sigma) {
    if (sigma > geo_map_get(g, v)) return;                          // a shorter way to v was found since
    const int h0 = g.vhe[v];
    if (h0 < 0) return;
    const double* A = g.V + 3 * (int64_t)v;
    int h = h0;
    for (int step = 0; step < 3 * g.nf; ++step) {
        const int f = h / 3, k = h - 3 * f;
        const int p = g.F[3 * f + (k + 1) % 3], q = g.F[3 * f + (k + 2) % 3];
        geo_update_vertex(g, p, sigma + geo_dist3(A, g.V + 3 * (int64_t)p));
        geo_update_vertex(g, q, sigma + geo_dist3(A, g.V + 3 * (int64_t)q));
        const int h2 = 3 * f + (k + 1) % 3;                         // p -> q, opposite to v
        const int t2 = g.twin[h2];
        if (t2 >= 0) {
            const GeoFrame fr = geo_frame(g, h2);                   // v is its c
            geo_push_window(g, t2, fr.L - fr.cx, -fr.cy, 0.0, fr.L, sigma);
        }
        const int t = g.twin[3 * f + (k + 2) % 3];
        if (t < 0 || t == h0) break;
        h = t;
    }
}

__device__ __forceinline__ void geo_process_window(const GeoSeed& g, const GeoWin& w) {
    const GeoFrame fr = geo_frame(g, w.he);
    const double sx = w.sx, sy = w.sy, lo = w.lo, hi = w.hi, sigma = w.sigma;
    const double to_lo = geo_hypot(sx - lo, sy), to_hi = geo_hypot(sx - hi, sy);
    if (geo_map_get(g, fr.a) + hi < sigma + to_hi - GEO_FILTER_SLACK) return;
    if (geo_map_get(g, fr.b) + (fr.L - lo) < sigma + to_lo - GEO_FILTER_SLACK) return;
    geo_update_vertex(g, fr.a, sigma + to_lo + lo);
    geo_update_vertex(g, fr.b, sigma + to_hi + (fr.L - hi));
    const double eps = GEO_EDGE_EPS * fr.L;
    const int f = w.he / 3, k = w.he - 3 * f;
    for (int i = g.fstart[f]; i < g.fstart[f + 1]; ++i) {
        const int t = g.tlist[i];
        const double* P = g.tpoint + 3 * (int64_t)t;
        const double px = P[0] - fr.ax, py = P[1] - fr.ay, pz = P[2] - fr.az;
        const double tx = (px * fr.exx + py * fr.exy) + pz * fr.exz, ty = (px * fr.eyx + py * fr.eyy) + pz * fr.eyz;
        const double den = ty - sy;
        if (den > 0.0) {
            const double X = sx + (tx - sx) * (-sy) / den;
            const double val = sigma + geo_hypot(tx - sx, ty - sy);
            if (X >= lo - eps && X <= hi + eps && val <= g.limit) geo_map_min(g, g.nv + t, val);
        }
    }
    const double Xc = sx + (fr.cx - sx) * (-sy) / (fr.cy - sy);
    if (Xc >= lo - eps && Xc <= hi + eps) geo_update_vertex(g, fr.c, sigma + geo_hypot(fr.cx - sx, fr.cy - sy));
    if (Xc < hi)    // through b -> c; the twin's origin is c
        geo_child(g, g.twin[3 * f + (k + 1) % 3], fr.L, 0.0, fr.cx, fr.cy, sx, sy, fmax(lo, Xc), hi, sigma, Xc > lo, false);
    if (Xc > lo)    // through c -> a; the twin's origin is a, its end c
        geo_child(g, g.twin[3 * f + (k + 2) % 3], fr.cx, fr.cy, 0.0, 0.0, sx, sy, lo, fmin(hi, Xc), sigma, false, Xc < hi);
}

__global__ __launch_bounds__(64) void geo_seed_kernel(GeoWs w, const double* __restrict__ V, int nv, const int* __restrict__ F, int nf,
                                                      const double* __restrict__ tpoint, const int64_t* __restrict__ tface, int nq,
                                                      const int64_t* __restrict__ seed_face, const double* __restrict__ seed_bary, int ns,
                                                      GeoRadii radii, int nr, int ql, int H, int qg, long long cap, int64_t* __restrict__ counts_out,
                                                      double* __restrict__ dist_out) {
    __shared__ GeoShared S;
    const int lane = threadIdx.x;
    GeoSeed g;
    g.S = &S;
    g.ql = ql;
    g.H = H;
    g.qg = qg;                                                      // <= w.qg, the stride of the work groups' rings
    g.gq = w.gq + (int64_t)blockIdx.x * w.qg;
    g.gmap = w.gmap + (int64_t)blockIdx.x * ((int64_t)nv + nq);
    g.V = V, g.F = F, g.twin = w.twin, g.vhe = w.vhe, g.pseudo = w.pseudo, g.fstart = w.fstart, g.tlist = w.tlist, g.tpoint = tpoint;
    g.nv = nv, g.nf = nf;
    double rmax = radii.r[0];
#pragma unroll
    for (int j = 1; j < GEO_MAXR; ++j)
        if (j < nr) rmax = radii.r[j];
    g.limit = rmax * (1.0 + 1e-12);
    const int64_t nkeys = (int64_t)nv + nq;
    for (int64_t i = lane; i < nkeys; i += 64) g.gmap[i] = GEO_INF_BITS;
    long long windows = 0;
    int peak = 0, n_spilled = 0, n_capped = 0, n_overflow = 0;

    for (int s = blockIdx.x; s < ns; s += gridDim.x) {
        __syncthreads();
        for (int i = lane; i < ql; i += 64) S.tag[i] = -1;
        for (int i = lane; i < H; i += 64) {
            S.keys[i] = -1;
            S.vals[i] = GEO_INF_BITS;
        }
        if (lane < GEO_MAXR) S.counts[lane] = 0;
        if (lane == 0) S.head = 0, S.tail = 0, S.spilled = 0, S.err = 0;
        __syncthreads();
        const int f0 = (int)seed_face[s];
        const double b0 = seed_bary[3 * (int64_t)s], b1 = seed_bary[3 * (int64_t)s + 1], b2 = seed_bary[3 * (int64_t)s + 2];
        const int i0 = F[3 * f0], i1 = F[3 * f0 + 1], i2 = F[3 * f0 + 2];
        double s3[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) s3[c] = (b0 * V[3 * (int64_t)i0 + c] + b1 * V[3 * (int64_t)i1 + c]) + b2 * V[3 * (int64_t)i2 + c];
        if (lane < 3) {
            const int h = 3 * f0 + lane;
            const int v = F[h];
            geo_update_vertex(g, v, geo_dist3(s3, V + 3 * (int64_t)v));
            const int t2 = w.twin[h];
            if (t2 >= 0) {
                const GeoFrame fr = geo_frame(g, h);
                const double px = s3[0] - fr.ax, py = s3[1] - fr.ay, pz = s3[2] - fr.az;
                const double x = (px * fr.exx + py * fr.exy) + pz * fr.exz, y = (px * fr.eyx + py * fr.eyy) + pz * fr.eyz;
                if (y > 0.0) geo_push_window(g, t2, fr.L - x, -y, 0.0, fr.L, 0.0);
            }
        }
        long long done = 0;
        int err = 0;
        for (;;) {
            __syncthreads();
            const int head = S.head, tail = S.tail;
            err = S.err;
            const int n = min(64, tail - head);
            if (n <= 0 || err) break;
            if (done + n > cap) {
                err = 1;
                break;
            }
            done += n;
            peak = max(peak, tail - head);
            if (lane < n) {
                const int pos = head + lane, slot = pos % ql;
                const GeoWin item = S.tag[slot] == pos ? S.q[slot] : g.gq[pos % g.qg];
                if (item.he < 0)
                    geo_process_vertex(g, -(item.he + 1), item.sigma);
                else
                    geo_process_window(g, item);
            }
            __syncthreads();
            if (lane == 0) S.head = head + n;
        }
        __syncthreads();
        windows += done;
        const int spilled = S.spilled;
        n_spilled += spilled ? 1 : 0;
        n_capped += (err & 1) ? 1 : 0;
        n_overflow += (err & 2) ? 1 : 0;
        // every target: the straight distance in the seed's face, else what the windows and the face's vertices give
        for (int t = lane; t < nq; t += 64) {
            const double* P = tpoint + 3 * (int64_t)t;
            const int64_t f = tface[t];
            double best = __builtin_huge_val();
            const double e = geo_dist3(s3, P);
            if (e <= g.limit && f >= 0 && f < nf) {
                if (f == f0) {
                    best = e;
                } else {
                    best = geo_map_get(g, nv + t);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int v = F[3 * f + k];
                        best = fmin(best, geo_map_get(g, v) + geo_dist3(V + 3 * (int64_t)v, P));
                    }
                }
            }
            if (!(best <= rmax)) best = __builtin_huge_val();
            if (dist_out) dist_out[(int64_t)s * nq + t] = best;
            if (best <= rmax) {
#pragma unroll
                for (int j = 0; j < GEO_MAXR; ++j)
                    if (j < nr && best <= radii.r[j]) atomicAdd(&S.counts[j], 1);
            }
        }
        __syncthreads();
        if (lane < nr) counts_out[(int64_t)s * nr + lane] = S.counts[lane];
        if (spilled) {                                              // the dense table back to +inf (uniform: S.spilled was read after a barrier)
            __syncthreads();
            for (int64_t i = lane; i < nkeys; i += 64) g.gmap[i] = GEO_INF_BITS;
        }
    }
    if (lane == 0) {
        atomicAdd(&w.ctl->windows, (unsigned long long)windows);
        atomicMax(&w.ctl->peak, peak);
        if (n_spilled) atomicAdd(&w.ctl->n_spilled, n_spilled);
        if (n_capped) atomicAdd(&w.ctl->n_capped, n_capped);
        if (n_overflow) atomicAdd(&w.ctl->n_overflow, n_overflow);
    }
}

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

extern "C" {

int64_t sapcu_geodesic_disks_workspace_bytes(int64_t nv, int64_t nf, int64_t nq, int64_t ns, int64_t nr) {
    return geo_sizes_ok(nv, nf, nq, ns, nr) ? (int64_t)geo_ws_layout(nullptr, nv, nf, nq, ns).bytes : -1;
}

// the call; window_cap and queue_limit are the header's constants, or smaller ones from the test hook below
static int geo_disks(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* target_point,
                     const int64_t* target_face, int64_t nq, const int64_t* seed_face, const double* seed_bary, int64_t ns,
                     const double* radii_host, int64_t nr, int64_t* counts_out, double* dist_out, int64_t queue_slots, int64_t window_cap,
                     int64_t queue_limit, void* workspace, int64_t workspace_bytes, int64_t* info_host, void* stream) {
    SAPCU_CHECK_ARG(vertices && faces && radii_host, "geodesic_disks: null pointer (vertices, faces and radii_host are required)");
    SAPCU_CHECK_ARG(geo_sizes_ok(nv, nf, nq, ns, nr),
                    "geodesic_disks: need 1 <= nv, nf <= 2^24, 0 <= nq <= 2^30, 0 <= ns <= 2^24, 1 <= nr <= %d (nv=%lld nf=%lld nq=%lld ns=%lld "
                    "nr=%lld)", GEO_MAXR, (long long)nv, (long long)nf, (long long)nq, (long long)ns, (long long)nr);
    SAPCU_CHECK_ARG(ns == 0 || (seed_face && seed_bary && counts_out), "geodesic_disks: null seed_face, seed_bary or counts_out with ns > 0");
    SAPCU_CHECK_ARG(nq == 0 || (target_point && target_face), "geodesic_disks: null target_point or target_face with nq > 0");
    SAPCU_CHECK_ARG(queue_slots >= 0, "geodesic_disks: queue_slots must be >= 0 (0 = automatic)");
    SAPCU_CHECK_ARG(window_cap >= 1 && window_cap <= SAPCU_GEODESIC_WINDOW_CAP(nf) && queue_limit >= 1 && queue_limit <= nf + 4096,
                    "geodesic_disks: the window cap and the queue limit must be positive and at most the header's");
    GeoRadii radii;
    for (int j = 0; j < GEO_MAXR; ++j) radii.r[j] = 0.0;
    for (int64_t j = 0; j < nr; ++j) {
        const double r = radii_host[j];
        SAPCU_CHECK_ARG(r > 0.0 && r < 1e300 && (j == 0 || r >= radii_host[j - 1]), "geodesic_disks: radii must be finite, positive and ascending");
        radii.r[j] = r;
    }
    const int64_t need = sapcu_geodesic_disks_workspace_bytes(nv, nf, nq, ns, nr);
    SAPCU_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0, "geodesic_disks: the workspace must be non-null and 8-byte aligned");
    SAPCU_CHECK_ARG(workspace_bytes >= need, "geodesic_disks: the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes,
                    (long long)need);
    if (ns == 0) {
        if (info_host)
            for (int i = 0; i < 8; ++i) info_host[i] = 0;
        return SAPCU_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    {   // the seeds' checks, on the host
        int64_t* hf = (int64_t*)malloc((size_t)ns * sizeof(int64_t));
        double* hb = (double*)malloc((size_t)ns * 3 * sizeof(double));
        if (!hf || !hb) {
            free(hf), free(hb);
            set_error("geodesic_disks: no host memory for %lld seeds", (long long)ns);
            return SAPCU_ERR_ARG;
        }
        hipError_t e = hipMemcpyAsync(hf, seed_face, (size_t)ns * sizeof(int64_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hb, seed_bary, (size_t)ns * 3 * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        int64_t bad = -1;
        for (int64_t s = 0; e == hipSuccess && s < ns && bad < 0; ++s) {
            const double a = hb[3 * s], b = hb[3 * s + 1], c = hb[3 * s + 2], sum = (a + b) + c;
            if (!(hf[s] >= 0 && hf[s] < nf && a > 0.0 && b > 0.0 && c > 0.0 && a < 1.0 && b < 1.0 && c < 1.0 && sum >= 1.0 - 1e-9 && sum <= 1.0 + 1e-9))
                bad = s;
        }
        free(hf), free(hb);
        if (e != hipSuccess) {
            set_error("geodesic_disks: copying the seeds failed: %s", hipGetErrorString(e));
            return SAPCU_ERR_HIP;
        }
        SAPCU_CHECK_ARG(bad < 0, "geodesic_disks: seed %lld has a face outside [0, %lld) or weights that are not positive, finite and of sum 1 "
                        "(seeds on edges and vertices are not taken)", (long long)bad, (long long)nf);
    }
    if (info_host)
        for (int i = 0; i < 8; ++i) info_host[i] = 0;
    if (nq == 0) {
        SAPCU_CHECK_HIP(hipMemsetAsync(counts_out, 0, (size_t)ns * nr * sizeof(int64_t), st));
        return SAPCU_OK;
    }
    const GeoWs w = geo_ws_layout(workspace, nv, nf, nq, ns);
    SAPCU_CHECK_HIP(hipMemsetAsync(w.ctl, 0, sizeof(GeoCtl), st));
    const unsigned fb = (unsigned)((nf + 255) / 256), hb3 = (unsigned)((3 * nf + 255) / 256), vb = (unsigned)((nv + 255) / 256),
                   qb = (unsigned)((nq + 255) / 256);
    hipLaunchKernelGGL(geo_init_kernel, dim3(1024), dim3(256), 0, st, w, nv, nf);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(geo_edge_insert_kernel, dim3(fb), dim3(256), 0, st, w, vertices, (int)nv, faces, (int)nf);
    SAPCU_CHECK_LAUNCH();
    GeoCtl hc;
    SAPCU_CHECK_HIP(hipMemcpyAsync(&hc, w.ctl, sizeof(hc), hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    if (hc.bad_mesh) {
        set_error("geodesic_disks: the mesh is refused:%s%s%s", (hc.bad_mesh & 1) ? " an edge is traversed twice in one direction (more than two faces, or two "
                  "faces of opposite orientation);" : "", (hc.bad_mesh & 2) ? " a face has zero area;" : "",
                  (hc.bad_mesh & 4) ? " a face has a vertex index outside [0, nv);" : "");
        return SAPCU_ERR_MESH;
    }
    hipLaunchKernelGGL(geo_twin_kernel, dim3(hb3), dim3(256), 0, st, w, faces, (int)nf);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(geo_boundary_kernel, dim3(hb3), dim3(256), 0, st, w, faces, (int)nf);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(geo_vertex_kernel, dim3(vb), dim3(256), 0, st, w, vertices, (int)nv, faces, (int)nf);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(geo_target_count_kernel, dim3(qb), dim3(256), 0, st, w, target_face, (int)nq, (int)nf);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(geo_scan_kernel, dim3(1), dim3(1024), 0, st, w, (int)nf);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(geo_target_fill_kernel, dim3(qb), dim3(256), 0, st, w, target_face, (int)nq, (int)nf);
    SAPCU_CHECK_LAUNCH();
    int ql = GEO_QL, H = GEO_H;
    const int qg = (int)queue_limit;
    if (ql > qg) ql = qg;                                           // the LDS ring is never longer than the workspace's
    if (queue_slots > 0) {
        if (queue_slots < ql) ql = (int)queue_slots;
        while (H > queue_slots) H >>= 1;
        if (H < 1) H = 1;
    }
    hipLaunchKernelGGL(geo_seed_kernel, dim3((unsigned)w.groups), dim3(64), 0, st, w, vertices, (int)nv, faces, (int)nf, target_point, target_face,
                       (int)nq, seed_face, seed_bary, (int)ns, radii, (int)nr, ql, H, qg, (long long)window_cap, counts_out, dist_out);
    SAPCU_CHECK_LAUNCH();
    SAPCU_CHECK_HIP(hipMemcpyAsync(&hc, w.ctl, sizeof(hc), hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    if (info_host) {
        info_host[0] = (int64_t)hc.windows;
        info_host[1] = hc.peak;
        info_host[2] = hc.n_spilled;
        info_host[3] = hc.n_boundary;
        info_host[4] = hc.n_pseudo;
        info_host[5] = hc.n_capped;
        info_host[6] = hc.n_overflow;
        info_host[7] = w.groups;
    }
    if (hc.n_capped || hc.n_overflow) {
        set_error("geodesic_disks: %d seeds reached the cap of %lld windows, %d outgrew the workspace queue of %lld slots", hc.n_capped,
                  (long long)window_cap, hc.n_overflow, (long long)queue_limit);
        return SAPCU_ERR_LIMIT;
    }
    return SAPCU_OK;
}

int sapcu_geodesic_disks_f64(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* target_point,
                             const int64_t* target_face, int64_t nq, const int64_t* seed_face, const double* seed_bary, int64_t ns,
                             const double* radii_host, int64_t nr, int64_t* counts_out, double* dist_out, int64_t queue_slots,
                             void* workspace, int64_t workspace_bytes, int64_t* info_host, void* stream) {
    return geo_disks(vertices, nv, faces, nf, target_point, target_face, nq, seed_face, seed_bary, ns, radii_host, nr, counts_out, dist_out,
                     queue_slots, SAPCU_GEODESIC_WINDOW_CAP(nf), nf + 4096, workspace, workspace_bytes, info_host, stream);
}

// test hook in no header: the same call with a smaller window cap and a shorter workspace queue, so that the two bounded ends of
// the loop (SAPCU_ERR_LIMIT) can be reached on a small mesh: tests/test_gpu_uniformity.py
int sapcu_internal_geodesic_disks_limited(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* target_point,
                                          const int64_t* target_face, int64_t nq, const int64_t* seed_face, const double* seed_bary,
                                          int64_t ns, const double* radii_host, int64_t nr, int64_t* counts_out, double* dist_out,
                                          int64_t queue_slots, int64_t window_cap, int64_t queue_limit, void* workspace,
                                          int64_t workspace_bytes, int64_t* info_host, void* stream) {
    return geo_disks(vertices, nv, faces, nf, target_point, target_face, nq, seed_face, seed_bary, ns, radii_host, nr, counts_out, dist_out,
                     queue_slots, window_cap, queue_limit, workspace, workspace_bytes, info_host, stream);
}

}  // extern "C"
