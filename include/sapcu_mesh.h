/*
 * sapcu_mesh.h — the distance from every query point to a triangle mesh on the device, with the nearest face and the closest
 * surface point: the distance vector behind P2F, the point-to-surface figure of an upsampler (sapcu_amd/mesh.py; the quantity the
 * reference's external/Meta-PU_evaluation/evaluation_code/evaluation.cpp computes with a CGAL AABB tree on the host).
 *
 * Part of libsapcu_hip.so; the conventions and status codes of sapcu.h apply (device pointers unless named *_host, the caller owns
 * every buffer, 0 on success, sapcu_last_error() for the text).  SAPCU_ABI_VERSION is unchanged: these entry points are additions.
 *
 * Definition (tests/mesh_ref.py states it in numpy).  Every operation is one separately rounded f64 operation.
 *   dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z.  For a query p and a face (a, b, c), the first matching region wins:
 *     1. ab = b - a, ac = c - a, ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap); d1 <= 0 and d2 <= 0:          q = a
 *     2. bp = p - b, d3 = dot(ab, bp), d4 = dot(ac, bp); d3 >= 0 and d4 <= d3:                                 q = b
 *     3. vc = d1*d4 - d3*d2; vc <= 0 and d1 >= 0 and d3 <= 0:   v = d1 / (d1 - d3),                            q = a + v*ab
 *     4. cp = p - c, d5 = dot(ab, cp), d6 = dot(ac, cp); d6 >= 0 and d5 <= d6:                                 q = c
 *     5. vb = d5*d2 - d1*d6; vb <= 0 and d2 >= 0 and d6 <= 0:   w = d2 / (d2 - d6),                            q = a + w*ac
 *     6. va = d3*d6 - d5*d4; va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
 *                                                w = (d4 - d3) / ((d4 - d3) + (d5 - d6)),                      q = b + w*(c - b)
 *     7. otherwise: den = 1 / ((va + vb) + vc), v = vb*den, w = vc*den,                                        q = (a + ab*v) + ac*w
 *   r = p - q, d2 = dot(r, r).  The result of a query is the face with the smallest d2, the LOWEST FACE INDEX among faces with
 *   bit-equal d2: dist_out = the correctly rounded square root of that d2, face_out = that face, closest_out = that face's q.
 *   Skipped faces take part in nothing: a face with a vertex index outside [0, nv), and a face whose normal n = ab x ac
 *   (ab.y*ac.z - ab.z*ac.y, ...) has dot(n, n) == 0 or not finite (zero area, collinear, repeated vertex: region 7 of a collinear
 *   triangle can return a point outside the segment and a distance below the true one).  A query that no face gives a finite d2
 *   for (a NaN query, every face skipped) gets dist NaN, face -1 and q NaN.
 *   Near-degenerate slivers get whatever the arithmetic above gives: the reference decides them with exact predicates, this code
 *   does not.  The equality of the two routes below rests on the computed distance of a face lying within 1e-11 of the largest
 *   |coordinate| of vertices and queries (absolute) plus 1e-9 (relative) of its true distance, which the arithmetic keeps by
 *   five orders of magnitude for triangles that are not such slivers.
 *
 * How it runs (csrc/mesh_dist.hip).  Brute force: one query per lane, the faces through a per-wavefront LDS slab, every lane
 * against every face.  Grid: the faces are binned by centroid into the cell grid of csrc/knn_grid.hip, the queries sorted by the
 * cell of that grid they fall in (clamped), Chebyshev shells around it until every lane's distance to the faces of the visited
 * block, less the largest radius of an in-grid face and a slack for the rounding at the vertices' and the queries' magnitude, is
 * strictly above its best.  Faces whose radius exceeds two cell edges are on an oversize list that every wavefront
 * scans first.  dist_out, face_out and closest_out of the grid route are BIT FOR BIT those of the brute-force route, for every
 * cell_size.  cell_size 0 = automatic: brute force below 1280 faces, else a cell edge for about 8 faces per occupied cell.
 * The brute-force route also runs, whatever cell_size says, for a non-finite or |x| > 1e150 coordinate in the vertices or the
 * queries, and when more than a quarter of the faces are oversize.
 *
 * Memory contract (as sapcu.h; checked under guard bands by tests/test_gpu_mesh.py):
 *   - vertices [nv,3] f64, faces [nf,3] int32 and queries [nq,3] f64 are only read; dist_out [nq] f64, face_out [nq] int64 (may be
 *     NULL) and closest_out [nq,3] f64 (may be NULL) are written in full, nothing else; nothing is written beyond the
 *     workspace_bytes the sizer returned for the same (nv, nf, nq);
 *   - the workspace needs NO initialisation and 8-byte alignment (f64 tables inside);
 *   - nq == 0 launches nothing and writes nothing (queries and dist_out may then be NULL);
 *   - refused before anything is launched, with SAPCU_ERR_ARG: a NULL vertices or faces, a NULL queries or dist_out with nq > 0,
 *     nv < 1 or nv > 2^31 - 1, nf < 1 or nf > 2^29, nq < 0 or nq > 2^31 - 64, cell_size negative, NaN or >= 1e300, a NULL
 *     workspace, one shorter than the sizer's bytes or not 8-byte aligned;
 *   - `stream` is synchronised once when the grid is asked for or info_host is given (grid parameters and counters are read
 *     back together), not at all on the automatic brute-force route with a NULL info_host.
 *
 * info_host (HOST int64[6], may be NULL) = {route: 0 brute force, 1 grid; gx, gy, gz; faces on the oversize list; faces skipped}.
 */
#ifndef SAPCU_MESH_H
#define SAPCU_MESH_H

#include "sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for a mesh of nv vertices and nf faces and nq queries; -1 for sizes the search would refuse. */
int64_t sapcu_point_mesh_workspace_bytes(int64_t nv, int64_t nf, int64_t nq);

int sapcu_point_mesh_f64(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* queries, int64_t nq,
                         double cell_size, double* dist_out, int64_t* face_out, double* closest_out, void* workspace,
                         int64_t workspace_bytes, int64_t* info_host, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_MESH_H */
