/*
 * sapcu_ray.h — where a ray first meets a triangle mesh, on the device: the parameter t, the face and the hit point of every ray,
 * and the fused step of fd's ray sampler (sapcu_amd/ray.py).  fd predicts a distance ALONG a direction (Generator3D6 moves a seed to
 * p + n*d); its ground truth against a mesh is a ray-mesh intersection, which the reference's scripts/sample_mesh-rd.py takes from
 * trimesh's embree intersector on the host.
 *
 * Part of libsapcu_hip.so; the conventions and status codes of sapcu.h apply (device pointers unless named *_host, the caller owns
 * every buffer, 0 on success, sapcu_last_error() for the text).  SAPCU_ABI_VERSION is unchanged: these entry points are additions.
 *
 * Definition (tests/ray_ref.py states it in numpy).  Every operation is one separately rounded f64 operation.
 *   dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z, cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x), as in
 *   sapcu_mesh.h.  A ray is an origin o, a direction d and a t_max >= 0; d need not be unit, t is in units of |d|, t_max may be +inf.
 *   For a face (a, b, c), Moeller-Trumbore in this order:
 *     1. e1 = b - a, e2 = c - a, h = cross(d, e2), det = dot(e1, h)
 *     2. inv = 1 / det, s = o - a, u = inv * dot(s, h)
 *     3. q = cross(s, e1), v = inv * dot(d, q), t = inv * dot(e2, q)
 *   The face is HIT iff det != 0 and det is finite, u >= 0 and u <= 1, v >= 0 and u + v <= 1, t >= 0 and t <= t_max.  A NaN anywhere
 *   makes a miss (every comparison is false), so does a t that overflowed to +inf, the value a miss reports.  Two-sided: no back-face
 *   culling.  Skipped faces take part in nothing and are counted: a face with a vertex index outside [0, nv), and a face whose normal
 *   n = cross(e1, e2) has dot(n, n) == 0 or not finite (the rule of sapcu_mesh.h).
 *   The result of a ray is the hit with the smallest t, the LOWEST FACE INDEX among faces with equal t: t_out = that t,
 *   face_out = that face, hit_out = o + t*d per component.  A ray that hits nothing gets t = +inf, face = -1, hit = NaN.
 *   A ray through a shared edge or vertex may hit both faces or neither: Moeller-Trumbore is not watertight there, and no exact
 *   predicates are used.  The equality of the two routes below rests on the computed hit point o + t*d lying within 1e-11 of the
 *   largest |coordinate| of vertices and origins of the face it is attributed to, which the arithmetic keeps by orders of magnitude
 *   unless the ray runs within about 1e-5 rad of the face's plane or the face is a sliver.
 *
 * How it runs (csrc/ray_cast.hip).  Brute force: one ray per lane, the faces through a per-wavefront LDS slab, every lane against
 * every face.  Grid: the faces are binned by centroid into the cell grid of csrc/knn_grid.hip exactly as for sapcu_point_mesh_f64;
 * every ray is clipped to the vertices' bounding box dilated by the largest radius R of an in-grid face plus a slack (a ray that
 * misses the box is a miss without a search, which is what makes t_max = +inf legal), the rays are sorted by the cell of their clipped
 * origin, and a wavefront walks its 64 clipped segments front to back in pieces of a few cell edges, visiting for each piece the
 * block of cells that covers the pieces' boxes dilated by R + slack, until every lane's best t is strictly below the start of its
 * next piece less the slack.  Faces whose radius exceeds two cell edges are on an oversize list that every wavefront scans first.
 * t_out, face_out and hit_out of the grid route are BIT FOR BIT those of the brute-force route, for every cell_size.
 * cell_size 0 = automatic: brute force below 1280 faces and for rays whose clipped segments are on average longer than four cell
 * edges and than an eighth of the grid (rays that cross the mesh, for which brute force is the faster route), else a cell edge for
 * about 8 faces per occupied cell.  The brute-force route also runs, whatever cell_size says, for a non-finite or |x| > 1e150
 * coordinate in vertices, origins or directions, for a non-zero direction component below 1e-150 in magnitude, and when more than
 * a quarter of the faces are oversize.
 *
 * Memory contract (as sapcu.h; checked under guard bands by tests/test_gpu_ray.py):
 *   - vertices [nv,3] f64, faces [nf,3] int32, origins [nq,3] f64, dirs [nq,3] f64 and t_max [nq] f64 (may be NULL: +inf for every
 *     ray) are only read; t_out [nq] f64, face_out [nq] int64 (may be NULL) and hit_out [nq,3] f64 (may be NULL) are written in
 *     full, nothing else; nothing is written beyond the workspace_bytes the sizer returned for the same (nv, nf, nq);
 *   - the workspace needs NO initialisation and 8-byte alignment (f64 tables inside);
 *   - nq == 0 launches nothing and writes nothing (origins, dirs and t_out may then be NULL);
 *   - refused before anything is launched, with SAPCU_ERR_ARG: a NULL vertices or faces, a NULL origins, dirs or t_out with nq > 0,
 *     nv < 1 or nv > 2^31 - 1, nf < 1 or nf > 2^29, nq < 0 or nq > 2^31 - 64, cell_size negative, NaN or >= 1e300, a NULL
 *     workspace, one shorter than the sizer's bytes or not 8-byte aligned;
 *   - `stream` is synchronised once when the grid is asked for or info_host is given (grid parameters and counters are read
 *     back together), not at all on the automatic brute-force route with a NULL info_host.
 *
 * info_host (HOST int64[6], may be NULL) = {route: 0 brute force, 1 grid; gx, gy, gz; faces on the oversize list; faces skipped}.
 *
 * sapcu_ray_fd_samples_f64: the sampler of scripts/sample_mesh-rd.py with the draws as inputs, n samples in one call.  surf [n,3]
 * f64 is a point on the face sface [n] int64 of the mesh, g [n,3] f64 a Gaussian triple, w [n] f64 uniform in [0, 1).  In f64:
 *   dir = g * (1 / sqrt(dot(g, g))), len = w*0.027 + 0.003, p = surf + len*dir; the ray from p along -dir with
 *   t_max = len * (1 + 2^-20) is cast as above; the sample is KEPT iff the first face hit is sface and dot(n, dir) > cos(1) =
 *   0.5403023058681398, n = cross(e1, e2) * (1 / sqrt(dot(cross(e1, e2), cross(e1, e2)))) of that face (square roots correctly
 *   rounded).  The reference tests arccos(dot) < 1; the cosine is compared instead because no device acos is correctly rounded.
 *   points_out [n,3] = p, normals_out [n,3] = -dir, lens_out [n] = len (all f64) and keep_out [n] uint8 (1 kept, 0 dropped) are
 *   written in full for every sample, kept or not.  One launch before the cast and one after it.  The contract above applies with
 *   n for nq; every pointer is required (n == 0: nothing is launched); an sface outside [0, nf) or a skipped face is never kept.
 */
#ifndef SAPCU_RAY_H
#define SAPCU_RAY_H

#include "sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for a mesh of nv vertices and nf faces and nq rays; -1 for sizes the cast would refuse. */
int64_t sapcu_ray_mesh_workspace_bytes(int64_t nv, int64_t nf, int64_t nq);

int sapcu_ray_mesh_f64(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* origins, const double* dirs,
                       const double* t_max, int64_t nq, double cell_size, double* t_out, int64_t* face_out, double* hit_out,
                       void* workspace, int64_t workspace_bytes, int64_t* info_host, void* stream);

/* Bytes of workspace for n samples against a mesh of nv vertices and nf faces; -1 for sizes the sampler would refuse. */
int64_t sapcu_ray_fd_samples_workspace_bytes(int64_t nv, int64_t nf, int64_t n);

int sapcu_ray_fd_samples_f64(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, const double* surf, const int64_t* sface,
                             const double* g, const double* w, int64_t n, double cell_size, double* points_out, double* normals_out,
                             double* lens_out, uint8_t* keep_out, void* workspace, int64_t workspace_bytes, int64_t* info_host,
                             void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_RAY_H */
