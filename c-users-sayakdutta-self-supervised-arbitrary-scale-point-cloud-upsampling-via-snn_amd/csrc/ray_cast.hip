// Where every ray first meets a triangle mesh (t, face, hit point), and the fused step of fd's ray sampler (sapcu_amd/ray.py).
// Replaces the embree intersector the reference's scripts/sample_mesh-rd.py calls through trimesh.  The definition (Moeller-Trumbore
// in a fixed operation order, two-sided, lowest face index among equal t, skipped faces) is stated in include/sapcu_ray.h and, in
// numpy, in tests/ray_ref.py.
//
// ray_face_test: one (ray, face) pair.  e1 and e2 depend on the face alone, so they are computed once while the face is loaded
// (the same two subtractions); everything else is the definition's operations in its order, the hit a conjunction of comparisons
// (a NaN fails them all), the best kept on the key (t, face).
//
// ray_brute_kernel, the definition on the device and the oracle of the grid route: one ray per lane; a wavefront gathers 64 faces at
// a time (skipped faces flagged while loading) into its own LDS slab and reads them back one face at a time, all lanes at one
// address: a broadcast (mesh_common.h: mesh_slab_scan, shared with mesh_dist.hip).
//
// ray_grid_kernel, on the centroid grid of mesh_dist.hip (mesh_common.h: the same centroids, radii r_f, oversize list, largest
// in-grid radius R):
//   * a hit is attributed to a face whose triangle the computed point P = o + t*d lies within `slack` of (sapcu_ray.h states what
//     that rests on), so the face's centroid lies within r_f + slack <= R + slack of P, for every in-grid face;
//   * ray_clip_kernel clips every ray to the vertices' box dilated by R + 2 * slack, per axis (slabs): outside [t0, t1] P leaves the
//     box along some axis, where no triangle is within slack of it.  The quotients are rounded at the magnitude of box and origin,
//     which one of the two slacks pays for.  A ray that misses the box, a zero direction (det is then +-0 for every face) and a
//     t_max that is negative or NaN have no piece at all: a miss without a search;
//   * the clipped segment is cut into np pieces of at most RAY_PIECE_CELLS cell edges (largest component); for a piece [ta, tb]
//     the box of its two end points, dilated by R + slack, contains the centroid of every in-grid face hit at a t in [ta, tb]; the
//     cell coordinates are monotone in the coordinate, so the block of cells between the box's corners holds them all.  A wavefront
//     visits the union block of its lanes' boxes;
//   * after the pieces before ta every face that could be hit at t <= ta has been tested, so a lane whose best t is strictly below
//     ta less the slack (in units of |d|: slack / largest |component of d|) is finished; best only falls and ta only grows, so a
//     finished lane stays finished.  A finished lane still tests the faces its wavefront loads: testing more faces moves a lane's
//     best towards the brute-force result, never away;
//   * slack = GridParams.slack of the centroids' grid plus 1e-11 * (largest |coordinate| of the vertices) plus 1e-11 * (largest
//     |coordinate| of the origins), as in mesh_dist.hip: s = o - a is rounded at these magnitudes;
//   * the rays are counting-sorted by the (clamped) cell of their clipped origin o + t0*d and taken 64 at a time in that order;
//     results go to the rays' original positions with ordinary vector stores.  No float atomics, no scratch.
// The brute-force kernel runs instead for non-finite or huge (|x| > 1e150) coordinates in vertices, origins or directions, for a
// non-zero direction component below 1e-150, when more than 1 / RAY_OVERSIZE_SHARE_DIV of the faces are oversize, and, with the
// automatic cell size, for nf < RAY_GRID_MIN_FACES and for rays longer than about an eighth of the grid on average.
#include "mesh_common.h"
#include "../../include/sapcu_ray.h"

namespace sapcu {

// profiles/ray_cast.txt: the grid wins from 1280 faces on for the sampler's rays and loses at 320; populations 2 .. 8
// and pieces of 1 .. 8 cell edges time alike for short rays
constexpr int RAY_CELL_POP = 4;
constexpr int64_t RAY_GRID_MIN_FACES = 1280;
constexpr double RAY_OVERSIZE_MULT = 2.0;
constexpr int64_t RAY_OVERSIZE_SHARE_DIV = 4;
constexpr double RAY_PIECE_CELLS = 2.0;
constexpr int RAY_MAX_PIECES = 1 << 20;
// automatic cell size: the grid only while the rays are short, on average at most max(2, largest grid dimension / 16) pieces per
// ray, about an eighth of the mesh's extent; rays that cross the whole mesh make a wavefront's lanes part ways and its union blocks
// grow, and brute force wins at every size measured (profiles/ray_cast.txt)
constexpr int RAY_AUTO_MIN_PIECES = 2;
constexpr int RAY_AUTO_GRID_DIV = 16;
constexpr int RAY_ROUTE_AUTO = 0, RAY_ROUTE_BRUTE = 1, RAY_ROUTE_GRID = 2;
constexpr double RAY_COS_1RAD = 0.5403023058681398;

struct RayCtl {
    MeshCtl m;
    double lo[3], hi[3];         // the vertices' bounding box
    unsigned long long pieces;   // pieces of all rays
    int weird;                   // a non-zero direction component below 1e-150
    int pad;
};

struct RayWs {
    GridWs g;                    // the grid over the faces' centroids
    GridWs q;                    // the rays in that grid's cells, by clipped origin (q.params = g.params, q.partials: the origins' box)
    double* vpartials;           // [KNN_GRID_BBOX_BLOCKS][8] bounding box of the vertices
    double* dpartials;           // the same of the directions (the bad flag alone is used)
    double* centroid;            // [nf, 3]
    double* radius;              // [nf]
    int* olist;                  // [nf]
    double* corg;                // [nq, 3] clipped origins
    double* t0;                  // [nq]
    double* t1;                  // [nq]
    int* np;                     // [nq] pieces (0: no search)
    RayCtl* ctl;
    size_t bytes;
};

static RayWs ray_ws_layout(void* base, int64_t nf, int64_t nq) {
    RayWs w;
    w.g = grid_ws_layout(base, nf);
    WsCarver c(base ? (char*)base + w.g.bytes : nullptr);
    w.q = grid_query_ws_layout(c, grid_cell_cap(nf), nq, w.g.params);
    w.vpartials = c.take<double>(8 * KNN_GRID_BBOX_BLOCKS);
    w.dpartials = c.take<double>(8 * KNN_GRID_BBOX_BLOCKS);
    w.centroid = c.take<double>(3 * nf);
    w.radius = c.take<double>(nf);
    w.olist = c.take<int>(nf);
    w.corg = c.take<double>(3 * nq);
    w.t0 = c.take<double>(nq);
    w.t1 = c.take<double>(nq);
    w.np = c.take<int>(nq);
    w.ctl = c.take<RayCtl>(1);
    w.bytes = w.g.bytes + c.bytes();
    return w;
}

// the sampler's own tables in front of the cast's workspace
struct FdRayWs {
    double* tmax;                // [n]
    double* t;                   // [n]
    int64_t* face;               // [n]
    void* cast;
    size_t bytes;
};

static FdRayWs fd_ray_ws_layout(void* base, int64_t nf, int64_t n) {
    WsCarver c(base);
    FdRayWs w;
    w.tmax = c.take<double>(n);
    w.t = c.take<double>(n);
    w.face = c.take<int64_t>(n);
    w.cast = base ? (char*)base + c.bytes() : nullptr;
    w.bytes = c.bytes() + ray_ws_layout(nullptr, nf, n).bytes;
    return w;
}

// ------------------------------------------------------------------------------------------------------ arithmetic
struct __align__(16) RayFace {
    double ax, ay, az, e1x, e1y, e1z, e2x, e2y, e2z;
    int idx, pad;                // idx < 0: skipped (or a spare slot of the slab)
};

struct RayBest {
    double t;                    // +inf beside f = -1: no hit yet
    int f;
};

struct Ray {
    double ox, oy, oz, dx, dy, dz, tmax;
};

__device__ __forceinline__ RayFace ray_load_face(int f, const double* __restrict__ vertices, int64_t nv, const int32_t* __restrict__ faces) {
    const MeshFace m = mesh_load_face(f, vertices, nv, faces);
    RayFace r;
    r.ax = m.ax;
    r.ay = m.ay;
    r.az = m.az;
    r.e1x = __dsub_rn(m.bx, m.ax);
    r.e1y = __dsub_rn(m.by, m.ay);
    r.e1z = __dsub_rn(m.bz, m.az);
    r.e2x = __dsub_rn(m.cx, m.ax);
    r.e2y = __dsub_rn(m.cy, m.ay);
    r.e2z = __dsub_rn(m.cz, m.az);
    r.idx = m.idx;
    r.pad = 0;
    return r;
}

__device__ __forceinline__ Ray ray_load(int64_t i, const double* __restrict__ origins, const double* __restrict__ dirs,
                                        const double* __restrict__ t_max) {
    Ray r;
    r.ox = origins[i * 3 + 0];
    r.oy = origins[i * 3 + 1];
    r.oz = origins[i * 3 + 2];
    r.dx = dirs[i * 3 + 0];
    r.dy = dirs[i * 3 + 1];
    r.dz = dirs[i * 3 + 2];
    r.tmax = t_max ? t_max[i] : __builtin_huge_val();
    return r;
}

// one face against one ray: the definition of include/sapcu_ray.h
__device__ __forceinline__ void ray_face_test(RayBest& B, const RayFace& m, const Ray& r) {
    const double hx = __dsub_rn(__dmul_rn(r.dy, m.e2z), __dmul_rn(r.dz, m.e2y));
    const double hy = __dsub_rn(__dmul_rn(r.dz, m.e2x), __dmul_rn(r.dx, m.e2z));
    const double hz = __dsub_rn(__dmul_rn(r.dx, m.e2y), __dmul_rn(r.dy, m.e2x));
    const double det = mesh_dot(m.e1x, m.e1y, m.e1z, hx, hy, hz);
    const double inv = __ddiv_rn(1.0, det);
    const double sx = __dsub_rn(r.ox, m.ax), sy = __dsub_rn(r.oy, m.ay), sz = __dsub_rn(r.oz, m.az);
    const double u = __dmul_rn(inv, mesh_dot(sx, sy, sz, hx, hy, hz));
    const double qx = __dsub_rn(__dmul_rn(sy, m.e1z), __dmul_rn(sz, m.e1y));
    const double qy = __dsub_rn(__dmul_rn(sz, m.e1x), __dmul_rn(sx, m.e1z));
    const double qz = __dsub_rn(__dmul_rn(sx, m.e1y), __dmul_rn(sy, m.e1x));
    const double v = __dmul_rn(inv, mesh_dot(r.dx, r.dy, r.dz, qx, qy, qz));
    const double t = __dmul_rn(inv, mesh_dot(m.e2x, m.e2y, m.e2z, qx, qy, qz));
    const bool hit = det != 0.0 && fabs(det) < __builtin_huge_val() && u >= 0.0 && u <= 1.0 && v >= 0.0 && __dadd_rn(u, v) <= 1.0 &&
                     t >= 0.0 && t <= r.tmax;
    // B.f starts at -1 beside t = +inf: an overflowed t never enters
    if (hit && (t < B.t || (t == B.t && m.idx < B.f))) {
        B.t = t;
        B.f = m.idx;
    }
}

// the faces order[a..b) (order NULL: the faces a..b themselves) against every lane's ray
__device__ __forceinline__ void ray_scan_range(RayBest& B, int a, int b, const int* __restrict__ order, const double* __restrict__ vertices,
                                               int64_t nv, const int32_t* __restrict__ faces, const Ray& r, RayFace* slab, int lane) {
    mesh_slab_scan(
        a, b, slab, lane, [&](int j) { return ray_load_face(order ? order[j] : j, vertices, nv, faces); },
        [&](const RayFace& m) { ray_face_test(B, m, r); });
}

__device__ __forceinline__ void ray_store(const RayBest& B, const Ray& r, int64_t o, double* __restrict__ t_out, int64_t* __restrict__ face_out,
                                          double* __restrict__ hit_out) {
    const double nan = __builtin_nan("");
    const bool hit = B.f >= 0;
    t_out[o] = B.t;
    if (face_out) face_out[o] = B.f;
    if (hit_out) {
        hit_out[o * 3 + 0] = hit ? __dadd_rn(r.ox, __dmul_rn(B.t, r.dx)) : nan;
        hit_out[o * 3 + 1] = hit ? __dadd_rn(r.oy, __dmul_rn(B.t, r.dy)) : nan;
        hit_out[o * 3 + 2] = hit ? __dadd_rn(r.oz, __dmul_rn(B.t, r.dz)) : nan;
    }
}

// --------------------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void ray_brute_kernel(const double* __restrict__ vertices, int64_t nv, const int32_t* __restrict__ faces,
                                                        int nf, const double* __restrict__ origins, const double* __restrict__ dirs,
                                                        const double* __restrict__ t_max, int64_t nq, double* __restrict__ t_out,
                                                        int64_t* __restrict__ face_out, double* __restrict__ hit_out) {
    __shared__ RayFace slabs[MESH_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t q0 = ((int64_t)blockIdx.x * MESH_WAVES + wave) * 64;
    if (q0 >= nq) return;                                                   // wave-uniform
    const bool valid = q0 + lane < nq;
    const int64_t i = valid ? q0 + lane : q0;                               // a spare lane repeats the chunk's first ray
    const Ray r = ray_load(i, origins, dirs, t_max);
    RayBest B{__builtin_huge_val(), -1};
    ray_scan_range(B, 0, nf, nullptr, vertices, nv, faces, r, slabs[wave], lane);
    if (valid) ray_store(B, r, i, t_out, face_out, hit_out);
}

// one wavefront: the bad flags of vertices, origins and directions, the vertices' box and the magnitudes into the slack
__global__ __launch_bounds__(64) void ray_setup_kernel(const double* __restrict__ vpartials, const double* __restrict__ opartials,
                                                       const double* __restrict__ dpartials, GridParams* __restrict__ prm,
                                                       RayCtl* __restrict__ ctl) {
    const double INF = __builtin_huge_val();
    double amax_v, amax_o, bad = 0.0;
    grid_partials_fold(vpartials, &amax_v, &bad);
    grid_partials_fold(opartials, &amax_o, &bad);
    grid_partials_fold(dpartials, nullptr, &bad);                            // the directions: the bad flag alone
    double lo[3] = {INF, INF, INF}, hi[3] = {-INF, -INF, -INF};
    for (int b = threadIdx.x; b < KNN_GRID_BBOX_BLOCKS; b += 64) {
        const double* v = vpartials + b * 8;
        for (int c = 0; c < 3; ++c) {
            lo[c] = fmin(lo[c], v[c]);
            hi[c] = fmax(hi[c], v[3 + c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = wave_min(lo[c]);
        hi[c] = wave_max(hi[c]);
    }
    if (threadIdx.x != 0) return;
    if (bad != 0.0) {
        prm->fallback = 1;
        return;
    }
    for (int c = 0; c < 3; ++c) {
        ctl->lo[c] = lo[c];
        ctl->hi[c] = hi[c];
    }
    prm->slack = __dadd_rn(prm->slack, __dadd_rn(__dmul_rn(1e-11, amax_v), __dmul_rn(1e-11, amax_o)));
}

// every ray against the dilated box: [t0, t1], the clipped origin, the number of pieces (0: no search)
__global__ __launch_bounds__(256) void ray_clip_kernel(const double* __restrict__ origins, const double* __restrict__ dirs,
                                                       const double* __restrict__ t_max, int64_t nq, const GridParams* __restrict__ prm,
                                                       double piece_cells, RayCtl* __restrict__ ctl, double* __restrict__ corg,
                                                       double* __restrict__ t0_out, double* __restrict__ t1_out, int* __restrict__ np_out) {
    if (prm->fallback) return;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i0 < nq;
    const int64_t i = valid ? i0 : nq - 1;                                  // a spare lane repeats the last ray and stores nothing
    const Ray r = ray_load(i, origins, dirs, t_max);
    const double R = __longlong_as_double((long long)ctl->m.rbits);
    const double margin = R + 2.0 * prm->slack;
    const double o[3] = {r.ox, r.oy, r.oz}, d[3] = {r.dx, r.dy, r.dz};
    double t0 = 0.0, t1 = r.tmax;
    bool miss = !(r.tmax >= 0.0) || (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0);
    bool weird = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double lo = ctl->lo[c] - margin, hi = ctl->hi[c] + margin;
        if (d[c] == 0.0) {
            if (!(o[c] >= lo && o[c] <= hi)) miss = true;
        } else {
            if (fabs(d[c]) < 1e-150) weird = true;
            const double ta = (lo - o[c]) / d[c], tb = (hi - o[c]) / d[c];
            t0 = fmax(t0, fmin(ta, tb));
            t1 = fmin(t1, fmax(ta, tb));
        }
    }
    if (weird && valid) atomicOr(&ctl->weird, 1);
    if (!(t0 <= t1) || !(t1 < __builtin_huge_val())) miss = true;
    int np = 0;
    double cx = ctl->lo[0], cy = ctl->lo[1], cz = ctl->lo[2];
    if (!miss && !weird) {
        const double span = t1 - t0;
        const double len = fmax(fmax(fabs(span * d[0]), fabs(span * d[1])), fabs(span * d[2]));
        const double want = ceil(len / (piece_cells * prm->h));
        np = want >= (double)RAY_MAX_PIECES ? RAY_MAX_PIECES : (want >= 1.0 ? (int)want : 1);
        cx = o[0] + t0 * d[0];
        cy = o[1] + t0 * d[1];
        cz = o[2] + t0 * d[2];
    }
    const int sum = wave_sum(valid ? np : 0);                                     // the wavefront's pieces: one integer atomic
    if (valid) {
        corg[i * 3 + 0] = cx;
        corg[i * 3 + 1] = cy;
        corg[i * 3 + 2] = cz;
        t0_out[i] = miss ? 0.0 : t0;
        t1_out[i] = miss ? 0.0 : t1;
        np_out[i] = np;
    }
    if ((threadIdx.x & 63) == 0 && sum > 0) atomicAdd(&ctl->pieces, (unsigned long long)sum);
}

__global__ __launch_bounds__(256) void ray_grid_kernel(const GridParams* __restrict__ prm, const int* __restrict__ start,
                                                       const int* __restrict__ fsidx, const int* __restrict__ olist, int n_over, double R,
                                                       const double* __restrict__ vertices, int64_t nv, const int32_t* __restrict__ faces,
                                                       const double* __restrict__ origins, const double* __restrict__ dirs,
                                                       const double* __restrict__ t_max, const int* __restrict__ qsidx,
                                                       const double* __restrict__ t0s, const double* __restrict__ t1s,
                                                       const int* __restrict__ nps, int64_t nq, double* __restrict__ t_out,
                                                       int64_t* __restrict__ face_out, double* __restrict__ hit_out) {
    __shared__ RayFace slabs[MESH_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t q0 = ((int64_t)blockIdx.x * MESH_WAVES + wave) * 64;
    if (q0 >= nq) return;                                                   // wave-uniform
    const bool valid = q0 + lane < nq;
    const int64_t i = qsidx[valid ? q0 + lane : q0];                        // a spare lane repeats the chunk's first ray
    const Ray r = ray_load(i, origins, dirs, t_max);
    const double t0 = t0s[i], t1 = t1s[i];
    const int np = nps[i];
    const GridParams p = *prm;
    RayBest B{__builtin_huge_val(), -1};
    RayFace* slab = slabs[wave];
    ray_scan_range(B, 0, n_over, olist, vertices, nv, faces, r, slab, lane);
    const double margin = __dadd_rn(R, p.slack);
    const double dmax = fmax(fmax(fabs(r.dx), fabs(r.dy)), fabs(r.dz));
    const double tslack = np > 0 ? p.slack / dmax : 0.0;
    const double span = t1 - t0;
    const int kmax = wave_max_uniform(np);
    double ta = t0;
    for (int k = 0; k < kmax; ++k) {
        const double tb = k + 1 >= np ? t1 : t0 + span * ((double)(k + 1) / (double)np);
        const bool active = k < np && !(B.t < ta - tslack);
        if (__ballot(active) == 0ull) break;                                // every lane is finished, for good
        int x0 = 0x7fffffff, y0 = 0x7fffffff, z0 = 0x7fffffff, x1 = -1, y1 = -1, z1 = -1;
        if (active) {
            const double ax = r.ox + ta * r.dx, ay = r.oy + ta * r.dy, az = r.oz + ta * r.dz;
            const double bx = r.ox + tb * r.dx, by = r.oy + tb * r.dy, bz = r.oz + tb * r.dz;
            x0 = grid_coord(fmin(ax, bx) - margin, p.ox, p.h, p.gx);
            x1 = grid_coord(fmax(ax, bx) + margin, p.ox, p.h, p.gx);
            y0 = grid_coord(fmin(ay, by) - margin, p.oy, p.h, p.gy);
            y1 = grid_coord(fmax(ay, by) + margin, p.oy, p.h, p.gy);
            z0 = grid_coord(fmin(az, bz) - margin, p.oz, p.h, p.gz);
            z1 = grid_coord(fmax(az, bz) + margin, p.oz, p.h, p.gz);
        }
        const int X0 = wave_min_uniform(x0), Y0 = wave_min_uniform(y0), Z0 = wave_min_uniform(z0);
        const int X1 = wave_max_uniform(x1), Y1 = wave_max_uniform(y1), Z1 = wave_max_uniform(z1);
        for (int z = Z0; z <= Z1; ++z) {
            for (int y = Y0; y <= Y1; ++y) {
                const int row = (z * p.gy + y) * p.gx;
                ray_scan_range(B, start[row + X0], start[row + X1 + 1], fsidx, vertices, nv, faces, r, slab, lane);
            }
        }
        ta = tb;
    }
    if (valid) ray_store(B, r, i, t_out, face_out, hit_out);
}

// the sampler's rays: dir = g / |g|, len, p = surf + len * dir; written as origin p, direction -dir, t_max = len * (1 + 2^-20)
__global__ __launch_bounds__(256) void fd_rays_kernel(const double* __restrict__ surf, const double* __restrict__ g, const double* __restrict__ w,
                                                      int64_t n, double* __restrict__ points, double* __restrict__ normals,
                                                      double* __restrict__ lens, double* __restrict__ tmax) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double gx = g[i * 3 + 0], gy = g[i * 3 + 1], gz = g[i * 3 + 2];
    const double s = __ddiv_rn(1.0, sqrt_cr(mesh_dot(gx, gy, gz, gx, gy, gz)));
    const double dx = __dmul_rn(gx, s), dy = __dmul_rn(gy, s), dz = __dmul_rn(gz, s);
    const double len = __dadd_rn(__dmul_rn(w[i], 0.027), 0.003);
    points[i * 3 + 0] = __dadd_rn(surf[i * 3 + 0], __dmul_rn(len, dx));
    points[i * 3 + 1] = __dadd_rn(surf[i * 3 + 1], __dmul_rn(len, dy));
    points[i * 3 + 2] = __dadd_rn(surf[i * 3 + 2], __dmul_rn(len, dz));
    normals[i * 3 + 0] = -dx;
    normals[i * 3 + 1] = -dy;
    normals[i * 3 + 2] = -dz;
    lens[i] = len;
    tmax[i] = __dmul_rn(len, 1.0 + 0x1p-20);
}

// the two keep tests: the first face hit is the sampled face, and its unit normal makes less than 1 rad with dir (= -normals)
__global__ __launch_bounds__(256) void fd_keep_kernel(const double* __restrict__ vertices, int64_t nv, const int32_t* __restrict__ faces,
                                                      int64_t nf, const int64_t* __restrict__ sface, const int64_t* __restrict__ hit_face,
                                                      const double* __restrict__ normals, int64_t n, uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t f = sface[i];
    bool k = f >= 0 && f < nf && hit_face[i] == f;
    if (k) {
        const RayFace m = ray_load_face((int)f, vertices, nv, faces);
        const double nx = __dsub_rn(__dmul_rn(m.e1y, m.e2z), __dmul_rn(m.e1z, m.e2y));
        const double ny = __dsub_rn(__dmul_rn(m.e1z, m.e2x), __dmul_rn(m.e1x, m.e2z));
        const double nz = __dsub_rn(__dmul_rn(m.e1x, m.e2y), __dmul_rn(m.e1y, m.e2x));
        const double s = __ddiv_rn(1.0, sqrt_cr(mesh_dot(nx, ny, nz, nx, ny, nz)));
        const double c = mesh_dot(__dmul_rn(nx, s), __dmul_rn(ny, s), __dmul_rn(nz, s), -normals[i * 3 + 0], -normals[i * 3 + 1],
                                  -normals[i * 3 + 2]);
        k = m.idx >= 0 && c > RAY_COS_1RAD;
    }
    keep[i] = k ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------- launchers
static int launch_ray_brute(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* origins, const double* dirs,
                            const double* t_max, int64_t nq, double* t, int64_t* face, double* hit, hipStream_t st) {
    const int64_t grid = (nq + 64 * MESH_WAVES - 1) / (64 * MESH_WAVES);
    hipLaunchKernelGGL(ray_brute_kernel, dim3((unsigned)grid), dim3(256), 0, st, vertices, nv, faces, (int)nf, origins, dirs, t_max, nq, t,
                       face, hit);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

static int launch_ray_mesh(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* origins, const double* dirs,
                           const double* t_max, int64_t nq, double cell_size, double oversize_mult, int cell_pop, double piece_cells,
                           int route, double* t, int64_t* face, double* hit, void* ws, int64_t* info, hipStream_t st) {
    if (info) info[0] = info[1] = info[2] = info[3] = info[4] = info[5] = 0;
    if (nq == 0) return SAPCU_OK;
    const RayWs w = ray_ws_layout(ws, nf, nq);
    RayCtl hc;
    memset(&hc, 0, sizeof(hc));
    if (route == RAY_ROUTE_BRUTE || (route == RAY_ROUTE_AUTO && cell_size == 0.0 && nf < RAY_GRID_MIN_FACES))
        return mesh_brute_route(vertices, nv, faces, nf, &w.ctl->m, info, st,
                                [&] { return launch_ray_brute(vertices, nv, faces, nf, origins, dirs, t_max, nq, t, face, hit, st); });
    SAPCU_CHECK_HIP(hipMemsetAsync(w.ctl, 0, sizeof(RayCtl), st));
    int rc = launch_grid_bbox(vertices, nv, w.vpartials, st);
    if (rc != SAPCU_OK) return rc;
    rc = launch_grid_bbox(origins, nq, w.q.partials, st);
    if (rc != SAPCU_OK) return rc;
    rc = launch_grid_bbox(dirs, nq, w.dpartials, st);
    if (rc != SAPCU_OK) return rc;
    rc = launch_mesh_prep(vertices, nv, faces, nf, w.centroid, w.radius, &w.ctl->m, st);
    if (rc != SAPCU_OK) return rc;
    rc = launch_grid_params(w.centroid, nf, cell_pop, cell_size, w.g, st);
    if (rc != SAPCU_OK) return rc;
    hipLaunchKernelGGL(ray_setup_kernel, dim3(1), dim3(64), 0, st, w.vpartials, w.q.partials, w.dpartials, w.g.params, w.ctl);
    SAPCU_CHECK_LAUNCH();
    rc = launch_mesh_classify(w.radius, nf, w.g.params, oversize_mult, w.olist, &w.ctl->m, st);
    if (rc != SAPCU_OK) return rc;
    hipLaunchKernelGGL(ray_clip_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, origins, dirs, t_max, nq, w.g.params, piece_cells,
                       w.ctl, w.corg, w.t0, w.t1, w.np);
    SAPCU_CHECK_LAUNCH();
    GridParams hp;
    SAPCU_CHECK_HIP(hipMemcpyAsync(&hp, w.g.params, sizeof(hp), hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipMemcpyAsync(&hc, w.ctl, sizeof(hc), hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    if (info) info[5] = hc.m.n_skip;
    if (hp.fallback || hc.weird) return launch_ray_brute(vertices, nv, faces, nf, origins, dirs, t_max, nq, t, face, hit, st);
    if (info) info[4] = hc.m.n_over;
    if ((int64_t)hc.m.n_over * RAY_OVERSIZE_SHARE_DIV > nf)
        return launch_ray_brute(vertices, nv, faces, nf, origins, dirs, t_max, nq, t, face, hit, st);
    const int gmax = hp.gx > hp.gy ? (hp.gx > hp.gz ? hp.gx : hp.gz) : (hp.gy > hp.gz ? hp.gy : hp.gz);
    const unsigned long long allowed = (unsigned long long)(gmax > RAY_AUTO_MIN_PIECES * RAY_AUTO_GRID_DIV ? gmax : RAY_AUTO_MIN_PIECES * RAY_AUTO_GRID_DIV);
    if (route == RAY_ROUTE_AUTO && cell_size == 0.0 && hc.pieces * RAY_AUTO_GRID_DIV > allowed * (unsigned long long)nq)
        return launch_ray_brute(vertices, nv, faces, nf, origins, dirs, t_max, nq, t, face, hit, st);   // long rays
    if (info) {
        info[0] = 1;
        info[1] = hp.gx;
        info[2] = hp.gy;
        info[3] = hp.gz;
    }
    double R;
    memcpy(&R, &hc.m.rbits, sizeof(R));
    rc = launch_grid_sort(w.centroid, nf, w.g, hp, st);
    if (rc != SAPCU_OK) return rc;
    rc = launch_grid_sort(w.corg, nq, w.q, hp, st);                         // the faces' parameters: the faces' cells
    if (rc != SAPCU_OK) return rc;
    const int64_t grid = (nq + 64 * MESH_WAVES - 1) / (64 * MESH_WAVES);
    hipLaunchKernelGGL(ray_grid_kernel, dim3((unsigned)grid), dim3(256), 0, st, w.g.params, w.g.start, w.g.sidx, w.olist, hc.m.n_over, R,
                       vertices, nv, faces, origins, dirs, t_max, w.q.sidx, w.t0, w.t1, w.np, nq, t, face, hit);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

extern "C" {

int64_t sapcu_ray_mesh_workspace_bytes(int64_t nv, int64_t nf, int64_t nq) {
    return mesh_sizes_ok(nv, nf, nq) ? (int64_t)ray_ws_layout(nullptr, nf, nq).bytes : -1;
}

int sapcu_ray_mesh_f64(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* origins, const double* dirs,
                       const double* t_max, int64_t nq, double cell_size, double* t_out, int64_t* face_out, double* hit_out,
                       void* workspace, int64_t workspace_bytes, int64_t* info_host, void* stream) {
    const int rc = mesh_args_check("ray_mesh", "n", vertices, nv, faces, nf, origins && dirs && t_out, nq, cell_size, workspace, workspace_bytes,
                                   sapcu_ray_mesh_workspace_bytes(nv, nf, nq));
    if (rc != SAPCU_OK) return rc;
    return launch_ray_mesh(vertices, nv, faces, nf, origins, dirs, t_max, nq, cell_size, RAY_OVERSIZE_MULT, RAY_CELL_POP, RAY_PIECE_CELLS,
                           RAY_ROUTE_AUTO, t_out, face_out, hit_out, workspace, info_host, (hipStream_t)stream);
}

int64_t sapcu_ray_fd_samples_workspace_bytes(int64_t nv, int64_t nf, int64_t n) {
    return mesh_sizes_ok(nv, nf, n) ? (int64_t)fd_ray_ws_layout(nullptr, nf, n).bytes : -1;
}

int sapcu_ray_fd_samples_f64(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* surf, const int64_t* sface,
                             const double* g, const double* w, int64_t n, double cell_size, double* points_out, double* normals_out,
                             double* lens_out, uint8_t* keep_out, void* workspace, int64_t workspace_bytes, int64_t* info_host,
                             void* stream) {
    const int rc = mesh_args_check("ray_fd_samples", "n", vertices, nv, faces, nf,
                                   surf && sface && g && w && points_out && normals_out && lens_out && keep_out, n, cell_size, workspace,
                                   workspace_bytes, sapcu_ray_fd_samples_workspace_bytes(nv, nf, n));
    if (rc != SAPCU_OK) return rc;
    if (info_host) info_host[0] = info_host[1] = info_host[2] = info_host[3] = info_host[4] = info_host[5] = 0;
    if (n == 0) return SAPCU_OK;
    hipStream_t st = (hipStream_t)stream;
    const FdRayWs fw = fd_ray_ws_layout(workspace, nf, n);
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(fd_rays_kernel, dim3(nb), dim3(256), 0, st, surf, g, w, n, points_out, normals_out, lens_out, fw.tmax);
    SAPCU_CHECK_LAUNCH();
    const int rc2 = launch_ray_mesh(vertices, nv, faces, nf, points_out, normals_out, fw.tmax, n, cell_size, RAY_OVERSIZE_MULT, RAY_CELL_POP,
                                    RAY_PIECE_CELLS, RAY_ROUTE_AUTO, fw.t, fw.face, nullptr, fw.cast, info_host, st);
    if (rc2 != SAPCU_OK) return rc2;
    hipLaunchKernelGGL(fd_keep_kernel, dim3(nb), dim3(256), 0, st, vertices, nv, faces, nf, sface, fw.face, normals_out, n, keep_out);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

// test and measurement hook in no header: sapcu_ray_mesh_f64 with the oversize cap (in cell edges), the cell population and the piece
// length (in cell edges) given, and the route: 0 automatic, 1 brute force whatever the sizes, 2 the grid whatever the face count and the
// rays' length (the fallbacks for coordinates and oversize faces still apply)
int sapcu_internal_ray_mesh_tuned(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* origins,
                                  const double* dirs, const double* t_max, int64_t nq, double cell_size, double oversize_mult, int cell_pop,
                                  double piece_cells, int route, double* t_out, int64_t* face_out, double* hit_out, void* workspace,
                                  int64_t workspace_bytes, int64_t* info_host, void* stream) {
    const int rc = mesh_args_check("ray_mesh_tuned", "n", vertices, nv, faces, nf, origins && dirs && t_out, nq, cell_size, workspace,
                                   workspace_bytes, sapcu_ray_mesh_workspace_bytes(nv, nf, nq));
    if (rc != SAPCU_OK) return rc;
    SAPCU_CHECK_ARG(oversize_mult > 0.0 && oversize_mult < 1e300 && cell_pop >= 1 && cell_pop <= 4096 && piece_cells >= 0.125 &&
                        piece_cells <= 1024.0 && route >= 0 && route <= 2,
                    "ray_mesh_tuned: need a positive finite oversize cap, 1 <= cell population <= 4096, 1/8 <= piece length <= 1024 and a "
                    "route in 0..2");
    return launch_ray_mesh(vertices, nv, faces, nf, origins, dirs, t_max, nq, cell_size, oversize_mult, cell_pop, piece_cells, route,
                           t_out, face_out, hit_out, workspace, info_host, (hipStream_t)stream);
}

}  // extern "C"
