// Distance from every query to a triangle mesh, the nearest face and the closest surface point: the distance vector behind P2F
// (sapcu_amd/mesh.py).  Replaces the CGAL AABB-tree query of the reference's external/Meta-PU_evaluation/evaluation_code/evaluation.cpp.
// The definition (Ericson's closest point in a fixed operation order, lowest face index among bit-equal d2, skipped faces) is stated
// in include/sapcu_mesh.h and, in numpy, in tests/mesh_ref.py.
//
// mesh_face_test: one (query, face) pair.  The seven regions diverge between lanes, so they are predicates and selects; each of the
// four quotients is needed in exactly one region, so numerator and denominator are selected by region and ONE division is issued
// (1 / den of region 7 included): value-identical to the definition.  The closest point is selected, never blended (a + 0 * e could
// turn a -0.0 into +0.0).
//
// mesh_brute_kernel, the definition on the device and the oracle of the grid route: one query per lane; a wavefront gathers 64
// faces at a time (three indices, nine coordinates, skipped faces flagged while loading) into its own LDS slab and reads them
// back one face at a time, all lanes at one address: a broadcast.  Each lane keeps (d2, face, q) and compares on the key (d2, face).
//
// mesh_grid_kernel, 64 queries of one cell per wavefront on grid_shell_walk (knn_grid.h: the query table, the walk, the stop rule):
//   * mesh_prep_kernel writes the centroid c' = ((a + b) + c) / 3 of every face and its radius r_f = max |vertex - c'| * (1 + 1e-9);
//     knn_grid.hip's launchers build the cell grid over the centroids and counting-sort the faces into it, then the queries by the
//     (clamped) cell of that grid they fall in; a cell with c queries gets ceil(c / 64) wavefronts;
//   * a triangle is the convex hull of its vertices, so it lies inside the ball of radius max |vertex - c'| around c' for ANY point
//     c': the rounding of the centroid itself costs nothing.  The radius is computed from c' as stored; its rounding (three
//     subtractions, a dot product and a square root: below 1e-15 relative) is covered by the factor 1 + 1e-9;
//   * after shell r every unvisited in-grid face has its centroid in a cell outside the visited block, hence every point of it lies
//     at least bnd - R away, R the largest radius among in-grid faces and bnd the distance to the block's faces: the walk's margin
//     is R + slack, its stop rule runs per lane against the lane's best d2, and the wave leaves when every lane is satisfied;
//   * slack = GridParams.slack of the centroids' grid, 1e-11 * (|centroid|max + extent + h), which covers the rounding of the cell
//     keys and of the block's face planes (about 1e-16 of the same magnitudes), plus 1e-11 * (largest |coordinate| of the vertices)
//     plus 1e-11 * (largest |coordinate| of the queries): q - plane is rounded at the query's magnitude, and the vertices of an
//     in-grid face lie up to R beyond the centroids' box.  The same two terms cover the computed distance of a face against its
//     true one: p - q loses the digits of the coordinates' magnitude, so the error of sqrt(d2) is ABSOLUTE, a few times 1e-16 of
//     max(|vertex|, |query|) for a triangle that is no sliver (tests/test_mesh_host.py measures 2.7e-13 relative on d2 for queries
//     1e-5 magnitudes away), five orders below 1e-11 of it.  The factor 1 - 1e-9 covers what is relative (the final dot product,
//     the squaring of the bound);
//   * faces with r_f > MESH_OVERSIZE_MULT * h are on the oversize list, which every wavefront scans first by brute force (this also
//     seeds its best).  They stay in the grid as well: meeting a face twice changes nothing, the key (d2, face) is the same;
//   * results go to the queries' original positions with ordinary vector stores.  No float atomics (the largest radius is an
//     integer maximum over the bits of non-negative doubles), no scratch.
// The brute-force kernel runs instead for non-finite or huge (|x| > 1e150) coordinates in vertices or queries, when more than
// 1 / MESH_OVERSIZE_SHARE_DIV of the faces are oversize, and for nf < MESH_GRID_MIN_FACES with the automatic cell size.
// The face record with its skip rule, mesh_dot, the slab scan and the counters live in mesh_common.h, which ray_cast.hip shares; it reaches
// mesh_prep_kernel and mesh_classify_kernel through launch_mesh_prep / launch_mesh_classify below.
#include "mesh_common.h"
#include "../../include/sapcu_mesh.h"

namespace sapcu {

// automatic cell edge: emax * sqrt(2 * MESH_CELL_POP / nf), about 2 * MESH_CELL_POP faces in an occupied cell of a surface
// (profiles/mesh_dist.txt: the sweeps of the population, the oversize cap and the automatic threshold)
constexpr int MESH_CELL_POP = 4;
constexpr int64_t MESH_GRID_MIN_FACES = 1280;
constexpr double MESH_OVERSIZE_MULT = 2.0;
constexpr int64_t MESH_OVERSIZE_SHARE_DIV = 4;

struct MeshWs {
    GridWs g;                    // the grid over the faces' centroids
    GridWs q;                    // the queries in that grid's cells (q.params = g.params)
    double* vpartials;           // [KNN_GRID_BBOX_BLOCKS][8] bounding box of the vertices
    int* wstart;                 // [cells + 1]
    double* centroid;            // [nf, 3]
    double* radius;              // [nf]
    int* olist;                  // [nf]
    MeshCtl* ctl;
    size_t bytes;
};

static MeshWs mesh_ws_layout(void* base, int64_t nf, int64_t nq) {
    const int64_t cap = grid_cell_cap(nf);
    MeshWs w;
    w.g = grid_ws_layout(base, nf);
    WsCarver c(base ? (char*)base + w.g.bytes : nullptr);
    w.q = grid_query_ws_layout(c, cap, nq, w.g.params);
    w.vpartials = c.take<double>(8 * KNN_GRID_BBOX_BLOCKS);
    w.wstart = c.take<int>(cap + 1);
    w.centroid = c.take<double>(3 * nf);
    w.radius = c.take<double>(nf);
    w.olist = c.take<int>(nf);
    w.ctl = c.take<MeshCtl>(1);
    w.bytes = w.g.bytes + c.bytes();
    return w;
}

// one face against one query: the definition of include/sapcu_mesh.h
__device__ __forceinline__ void mesh_face_test(MeshBest& B, const MeshFace& m, double px, double py, double pz) {
    const double abx = __dsub_rn(m.bx, m.ax), aby = __dsub_rn(m.by, m.ay), abz = __dsub_rn(m.bz, m.az);
    const double acx = __dsub_rn(m.cx, m.ax), acy = __dsub_rn(m.cy, m.ay), acz = __dsub_rn(m.cz, m.az);
    const double apx = __dsub_rn(px, m.ax), apy = __dsub_rn(py, m.ay), apz = __dsub_rn(pz, m.az);
    const double d1 = mesh_dot(abx, aby, abz, apx, apy, apz);
    const double d2 = mesh_dot(acx, acy, acz, apx, apy, apz);
    const double bpx = __dsub_rn(px, m.bx), bpy = __dsub_rn(py, m.by), bpz = __dsub_rn(pz, m.bz);
    const double d3 = mesh_dot(abx, aby, abz, bpx, bpy, bpz);
    const double d4 = mesh_dot(acx, acy, acz, bpx, bpy, bpz);
    const double cpx = __dsub_rn(px, m.cx), cpy = __dsub_rn(py, m.cy), cpz = __dsub_rn(pz, m.cz);
    const double d5 = mesh_dot(abx, aby, abz, cpx, cpy, cpz);
    const double d6 = mesh_dot(acx, acy, acz, cpx, cpy, cpz);
    const double vc = __dsub_rn(__dmul_rn(d1, d4), __dmul_rn(d3, d2));
    const double vb = __dsub_rn(__dmul_rn(d5, d2), __dmul_rn(d1, d6));
    const double va = __dsub_rn(__dmul_rn(d3, d6), __dmul_rn(d5, d4));
    const double e43 = __dsub_rn(d4, d3), e56 = __dsub_rn(d5, d6);
    const bool r1 = d1 <= 0.0 && d2 <= 0.0;
    const bool r2 = !r1 && d3 >= 0.0 && d4 <= d3;
    const bool r3 = !r1 && !r2 && vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0;
    const bool v123 = r1 || r2 || r3;
    const bool r4 = !v123 && d6 >= 0.0 && d5 <= d6;
    const bool r5 = !v123 && !r4 && vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0;
    const bool r6 = !v123 && !r4 && !r5 && va <= 0.0 && e43 >= 0.0 && e56 >= 0.0;
    // the one quotient: v of region 3, w of regions 5 and 6, 1 / den of region 7 (unused in the vertex regions)
    const double num = r3 ? d1 : (r5 ? d2 : (r6 ? e43 : 1.0));
    const double den = r3 ? __dsub_rn(d1, d3) : (r5 ? __dsub_rn(d2, d6) : (r6 ? __dadd_rn(e43, e56) : __dadd_rn(__dadd_rn(va, vb), vc)));
    const double t = __ddiv_rn(num, den);
    // an edge region: base + t * e
    const double ox = r6 ? m.bx : m.ax, oy = r6 ? m.by : m.ay, oz = r6 ? m.bz : m.az;
    const double ex = r3 ? abx : (r5 ? acx : __dsub_rn(m.cx, m.bx));
    const double ey = r3 ? aby : (r5 ? acy : __dsub_rn(m.cy, m.by));
    const double ez = r3 ? abz : (r5 ? acz : __dsub_rn(m.cz, m.bz));
    const double gx = __dadd_rn(ox, __dmul_rn(t, ex)), gy = __dadd_rn(oy, __dmul_rn(t, ey)), gz = __dadd_rn(oz, __dmul_rn(t, ez));
    // the interior: (a + ab * v) + ac * w
    const double v = __dmul_rn(vb, t), w = __dmul_rn(vc, t);
    const double ix = __dadd_rn(__dadd_rn(m.ax, __dmul_rn(abx, v)), __dmul_rn(acx, w));
    const double iy = __dadd_rn(__dadd_rn(m.ay, __dmul_rn(aby, v)), __dmul_rn(acy, w));
    const double iz = __dadd_rn(__dadd_rn(m.az, __dmul_rn(abz, v)), __dmul_rn(acz, w));
    const bool edge = r3 || r5 || r6;
    const double qx = r1 ? m.ax : (r2 ? m.bx : (r4 ? m.cx : (edge ? gx : ix)));
    const double qy = r1 ? m.ay : (r2 ? m.by : (r4 ? m.cy : (edge ? gy : iy)));
    const double qz = r1 ? m.az : (r2 ? m.bz : (r4 ? m.cz : (edge ? gz : iz)));
    const double rx = __dsub_rn(px, qx), ry = __dsub_rn(py, qy), rz = __dsub_rn(pz, qz);
    const double dd = mesh_dot(rx, ry, rz, rx, ry, rz);
    // B.f starts at -1 beside d = +inf: an infinite (overflowed) d2 never enters, a NaN one neither
    if (dd < B.d || (dd == B.d && m.idx < B.f)) {
        B.d = dd;
        B.f = m.idx;
        B.qx = qx;
        B.qy = qy;
        B.qz = qz;
    }
}

// the faces order[a..b) (order NULL: the faces a..b themselves) against every lane's query
__device__ __forceinline__ void mesh_scan_range(MeshBest& B, int a, int b, const int* __restrict__ order, const double* __restrict__ vertices,
                                                int64_t nv, const int32_t* __restrict__ faces, double px, double py, double pz,
                                                MeshFace* slab, int lane) {
    mesh_slab_scan(
        a, b, slab, lane, [&](int j) { return mesh_load_face(order ? order[j] : j, vertices, nv, faces); },
        [&](const MeshFace& m) { mesh_face_test(B, m, px, py, pz); });
}

__device__ __forceinline__ void mesh_store(const MeshBest& B, int64_t o, double* __restrict__ dist_out, int64_t* __restrict__ face_out,
                                           double* __restrict__ closest_out) {
    const double nan = __builtin_nan("");
    const bool hit = B.f >= 0;
    dist_out[o] = hit ? sqrt_cr(B.d) : nan;
    if (face_out) face_out[o] = B.f;
    if (closest_out) {
        closest_out[o * 3 + 0] = hit ? B.qx : nan;
        closest_out[o * 3 + 1] = hit ? B.qy : nan;
        closest_out[o * 3 + 2] = hit ? B.qz : nan;
    }
}

// --------------------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void mesh_brute_kernel(const double* __restrict__ vertices, int64_t nv, const int32_t* __restrict__ faces,
                                                         int nf, const double* __restrict__ queries, int64_t nq,
                                                         double* __restrict__ dist_out, int64_t* __restrict__ face_out,
                                                         double* __restrict__ closest_out) {
    __shared__ MeshFace slabs[MESH_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t q0 = ((int64_t)blockIdx.x * MESH_WAVES + wave) * 64;
    if (q0 >= nq) return;                                                   // wave-uniform
    const bool valid = q0 + lane < nq;
    const int64_t i = valid ? q0 + lane : q0;                               // a spare lane repeats the chunk's first query
    const double px = queries[i * 3 + 0], py = queries[i * 3 + 1], pz = queries[i * 3 + 2];
    MeshBest B{__builtin_huge_val(), -1, 0.0, 0.0, 0.0};
    mesh_scan_range(B, 0, nf, nullptr, vertices, nv, faces, px, py, pz, slabs[wave], lane);
    if (valid) mesh_store(B, i, dist_out, face_out, closest_out);
}

// centroid and radius of every face, the number of skipped faces.  centroid NULL: the count alone.
__global__ __launch_bounds__(256) void mesh_prep_kernel(const double* __restrict__ vertices, int64_t nv, const int32_t* __restrict__ faces,
                                                        int nf, double* __restrict__ centroid, double* __restrict__ radius,
                                                        MeshCtl* __restrict__ ctl) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int32_t* t = faces + (int64_t)f * 3;
    const int64_t i0 = t[0], i1 = t[1], i2 = t[2];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) {   // skipped: a point of the mesh's box, radius 0
        atomicAdd(&ctl->n_skip, 1);
        if (centroid) {
            centroid[(int64_t)f * 3 + 0] = vertices[0];
            centroid[(int64_t)f * 3 + 1] = vertices[1];
            centroid[(int64_t)f * 3 + 2] = vertices[2];
            radius[f] = 0.0;
        }
        return;
    }
    const MeshFace m = mesh_load_face(f, vertices, nv, faces);
    if (m.idx < 0) atomicAdd(&ctl->n_skip, 1);
    if (!centroid) return;
    const double gx = __ddiv_rn(__dadd_rn(__dadd_rn(m.ax, m.bx), m.cx), 3.0);
    const double gy = __ddiv_rn(__dadd_rn(__dadd_rn(m.ay, m.by), m.cy), 3.0);
    const double gz = __ddiv_rn(__dadd_rn(__dadd_rn(m.az, m.bz), m.cz), 3.0);
    const double ux = __dsub_rn(m.ax, gx), uy = __dsub_rn(m.ay, gy), uz = __dsub_rn(m.az, gz);
    const double vx = __dsub_rn(m.bx, gx), vy = __dsub_rn(m.by, gy), vz = __dsub_rn(m.bz, gz);
    const double wx = __dsub_rn(m.cx, gx), wy = __dsub_rn(m.cy, gy), wz = __dsub_rn(m.cz, gz);
    const double r2 = fmax(fmax(mesh_dot(ux, uy, uz, ux, uy, uz), mesh_dot(vx, vy, vz, vx, vy, vz)), mesh_dot(wx, wy, wz, wx, wy, wz));
    centroid[(int64_t)f * 3 + 0] = gx;
    centroid[(int64_t)f * 3 + 1] = gy;
    centroid[(int64_t)f * 3 + 2] = gz;
    radius[f] = __dmul_rn(sqrt(r2), 1.0 + 1e-9);
}

// one wavefront: the bad flags and magnitudes of the vertices and of the queries into the centroid grid's parameters (maxima: any order)
__global__ __launch_bounds__(64) void mesh_setup_kernel(const double* __restrict__ vpartials, const double* __restrict__ qpartials,
                                                        GridParams* __restrict__ prm) {
    double amax_v, amax_q, bad = 0.0;
    grid_partials_fold(vpartials, &amax_v, &bad);
    grid_partials_fold(qpartials, &amax_q, &bad);
    if (threadIdx.x != 0) return;
    if (bad != 0.0) {
        prm->fallback = 1;
        return;
    }
    prm->slack = __dadd_rn(prm->slack, __dadd_rn(__dmul_rn(1e-11, amax_v), __dmul_rn(1e-11, amax_q)));
}

// the oversize list (radius above MESH_OVERSIZE_MULT cell edges) and the largest radius of the other faces
__global__ __launch_bounds__(256) void mesh_classify_kernel(const double* __restrict__ radius, int nf, const GridParams* __restrict__ prm,
                                                            double mult, int* __restrict__ olist, MeshCtl* __restrict__ ctl) {
    if (prm->fallback) return;
    const int f = blockIdx.x * 256 + threadIdx.x;
    const double cap = __dmul_rn(mult, prm->h);
    double r = 0.0;
    if (f < nf) {
        r = radius[f];
        if (!(r <= cap)) {
            olist[atomicAdd(&ctl->n_over, 1)] = f;                          // at most nf entries
            r = 0.0;
        }
    }
    r = wave_max(r);
    if ((threadIdx.x & 63) == 0 && r > 0.0) atomicMax(&ctl->rbits, (unsigned long long)__double_as_longlong(r));
}

__global__ __launch_bounds__(256) void mesh_grid_kernel(const GridParams* __restrict__ prm, const int* __restrict__ start,
                                                        const int* __restrict__ fsidx, const int* __restrict__ olist, int n_over, double R,
                                                        const double* __restrict__ vertices, int64_t nv, const int32_t* __restrict__ faces,
                                                        const int* __restrict__ qstart, const int* __restrict__ wstart,
                                                        const double* __restrict__ qsx, const double* __restrict__ qsy,
                                                        const double* __restrict__ qsz, const int* __restrict__ qsidx, int cells,
                                                        double* __restrict__ dist_out, int64_t* __restrict__ face_out,
                                                        double* __restrict__ closest_out) {
    __shared__ MeshFace slabs[MESH_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t w = (int64_t)blockIdx.x * MESH_WAVES + wave;
    int cell, qa, qb;
    if (!grid_wave_chunk(w, wstart, qstart, cells, &cell, &qa, &qb)) return;
    const bool valid = qa + lane < qb;
    const int j = valid ? qa + lane : qa;                                   // a spare lane repeats the chunk's first query
    const double px = qsx[j], py = qsy[j], pz = qsz[j];
    const GridParams p = *prm;
    const int cx = cell % p.gx, cy = (cell / p.gx) % p.gy, cz = cell / (p.gx * p.gy);
    const double INF = __builtin_huge_val();
    MeshBest B{INF, -1, 0.0, 0.0, 0.0};
    MeshFace* slab = slabs[wave];
    mesh_scan_range(B, 0, n_over, olist, vertices, nv, faces, px, py, pz, slab, lane);
    grid_shell_walk(
        p, start, cx, cy, cz, px, py, pz, __dadd_rn(R, p.slack),                           // a face reaches R from its centroid
        [&](int a, int b) { mesh_scan_range(B, a, b, fsidx, vertices, nv, faces, px, py, pz, slab, lane); },
        [&](double bnd) { return __ballot(!grid_bound_clears(bnd, B.d)) == 0ull; });       // every lane's bound clears its best
    if (valid) mesh_store(B, qsidx[j], dist_out, face_out, closest_out);
}

// ------------------------------------------------------------------------------------------------------- launchers
static int launch_mesh_brute(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* queries, int64_t nq,
                             double* dist, int64_t* face, double* closest, hipStream_t st) {
    const int64_t grid = (nq + 64 * MESH_WAVES - 1) / (64 * MESH_WAVES);
    hipLaunchKernelGGL(mesh_brute_kernel, dim3((unsigned)grid), dim3(256), 0, st, vertices, nv, faces, (int)nf, queries, nq, dist, face,
                       closest);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

// the two face passes for the other translation units (mesh_common.h)
int launch_mesh_prep(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, double* centroid, double* radius, MeshCtl* ctl,
                     hipStream_t st) {
    hipLaunchKernelGGL(mesh_prep_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, vertices, nv, faces, (int)nf, centroid, radius,
                       ctl);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int launch_mesh_classify(const double* radius, int64_t nf, const GridParams* prm, double mult, int* olist, MeshCtl* ctl, hipStream_t st) {
    hipLaunchKernelGGL(mesh_classify_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, radius, (int)nf, prm, mult, olist, ctl);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int launch_point_mesh(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* queries, int64_t nq,
                      double cell_size, double oversize_mult, int cell_pop, bool force_brute, double* dist, int64_t* face, double* closest,
                      void* ws, int64_t* info, hipStream_t st) {
    if (info) info[0] = info[1] = info[2] = info[3] = info[4] = info[5] = 0;
    if (nq == 0) return SAPCU_OK;
    const MeshWs w = mesh_ws_layout(ws, nf, nq);
    const unsigned fblocks = (unsigned)((nf + 255) / 256);
    MeshCtl hc{0ull, 0, 0};
    if (force_brute || (cell_size == 0.0 && nf < MESH_GRID_MIN_FACES))
        return mesh_brute_route(vertices, nv, faces, nf, w.ctl, info, st,
                                [&] { return launch_mesh_brute(vertices, nv, faces, nf, queries, nq, dist, face, closest, st); });
    SAPCU_CHECK_HIP(hipMemsetAsync(w.ctl, 0, sizeof(MeshCtl), st));
    int rc = launch_grid_bbox(vertices, nv, w.vpartials, st);
    if (rc != SAPCU_OK) return rc;
    rc = launch_grid_bbox(queries, nq, w.q.partials, st);
    if (rc != SAPCU_OK) return rc;
    hipLaunchKernelGGL(mesh_prep_kernel, dim3(fblocks), dim3(256), 0, st, vertices, nv, faces, (int)nf, w.centroid, w.radius, w.ctl);
    SAPCU_CHECK_LAUNCH();
    rc = launch_grid_params(w.centroid, nf, cell_pop, cell_size, w.g, st);
    if (rc != SAPCU_OK) return rc;
    hipLaunchKernelGGL(mesh_setup_kernel, dim3(1), dim3(64), 0, st, w.vpartials, w.q.partials, w.g.params);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_classify_kernel, dim3(fblocks), dim3(256), 0, st, w.radius, (int)nf, w.g.params, oversize_mult, w.olist, w.ctl);
    SAPCU_CHECK_LAUNCH();
    GridParams hp;
    SAPCU_CHECK_HIP(hipMemcpyAsync(&hp, w.g.params, sizeof(hp), hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipMemcpyAsync(&hc, w.ctl, sizeof(hc), hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    if (info) info[5] = hc.n_skip;
    if (hp.fallback) return launch_mesh_brute(vertices, nv, faces, nf, queries, nq, dist, face, closest, st);
    if (info) info[4] = hc.n_over;
    if ((int64_t)hc.n_over * MESH_OVERSIZE_SHARE_DIV > nf)
        return launch_mesh_brute(vertices, nv, faces, nf, queries, nq, dist, face, closest, st);
    if (info) {
        info[0] = 1;
        info[1] = hp.gx;
        info[2] = hp.gy;
        info[3] = hp.gz;
    }
    double R;
    memcpy(&R, &hc.rbits, sizeof(R));
    rc = launch_grid_sort(w.centroid, nf, w.g, hp, st);
    if (rc != SAPCU_OK) return rc;
    rc = launch_grid_sort(queries, nq, w.q, hp, st);                        // the faces' parameters: the faces' cells
    if (rc != SAPCU_OK) return rc;
    const int64_t cells = (int64_t)hp.gx * hp.gy * hp.gz;
    rc = launch_grid_query_waves(w.q.start, cells, w.wstart, w.q.tile_sums, st);
    if (rc != SAPCU_OK) return rc;
    const int64_t grid = (grid_query_wave_bound(nq, cells) + MESH_WAVES - 1) / MESH_WAVES;
    hipLaunchKernelGGL(mesh_grid_kernel, dim3((unsigned)grid), dim3(256), 0, st, w.g.params, w.g.start, w.g.sidx, w.olist, hc.n_over, R,
                       vertices, nv, faces, w.q.start, w.wstart, w.q.sx, w.q.sy, w.q.sz, w.q.sidx, (int)cells, dist, face, closest);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

extern "C" {

int64_t sapcu_point_mesh_workspace_bytes(int64_t nv, int64_t nf, int64_t nq) {
    return mesh_sizes_ok(nv, nf, nq) ? (int64_t)mesh_ws_layout(nullptr, nf, nq).bytes : -1;
}

int sapcu_point_mesh_f64(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* queries, int64_t nq,
                         double cell_size, double* dist_out, int64_t* face_out, double* closest_out, void* workspace,
                         int64_t workspace_bytes, int64_t* info_host, void* stream) {
    const int rc = mesh_args_check("point_mesh", "nq", vertices, nv, faces, nf, queries && dist_out, nq, cell_size, workspace, workspace_bytes,
                                   sapcu_point_mesh_workspace_bytes(nv, nf, nq));
    if (rc != SAPCU_OK) return rc;
    return launch_point_mesh(vertices, nv, faces, nf, queries, nq, cell_size, MESH_OVERSIZE_MULT, MESH_CELL_POP, false, dist_out,
                             face_out, closest_out, workspace, info_host, (hipStream_t)stream);
}

// test and measurement hook in no header: the same call with the oversize cap (in cell edges) and the cell population given, or
// (force_brute != 0) on the brute-force route whatever the sizes
int sapcu_internal_point_mesh_tuned(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* queries, int64_t nq,
                                    double cell_size, double oversize_mult, int cell_pop, int force_brute, double* dist_out,
                                    int64_t* face_out, double* closest_out, void* workspace, int64_t workspace_bytes, int64_t* info_host, void* stream) {
    const int rc = mesh_args_check("point_mesh_tuned", "nq", vertices, nv, faces, nf, queries && dist_out, nq, cell_size, workspace,
                                   workspace_bytes, sapcu_point_mesh_workspace_bytes(nv, nf, nq));
    if (rc != SAPCU_OK) return rc;
    SAPCU_CHECK_ARG(oversize_mult > 0.0 && oversize_mult < 1e300 && cell_pop >= 1 && cell_pop <= 4096,
                    "point_mesh_tuned: need a positive finite oversize cap and 1 <= cell population <= 4096");
    return launch_point_mesh(vertices, nv, faces, nf, queries, nq, cell_size, oversize_mult, cell_pop, force_brute != 0, dist_out, face_out,
                             closest_out, workspace, info_host, (hipStream_t)stream);
}

}  // extern "C"
