/*
 * sapcu_surface.h — area-weighted sampling of triangle meshes on the device: what the reference's fn/datacore.py
 * PU1KMeshDataset._sample_points_from_mesh (:122-184) computes per sample in numpy, i.e. the step of PU1KMeshDataset.__getitem__
 * that comes BEFORE what sapcu_data.h covers (sapcu_amd/surface.py is the Python layer, sapcu_amd.data.MeshSurfacePatches the loader).
 *
 * Part of libsapcu_hip.so; the conventions and status codes of sapcu.h apply (device pointers, the caller owns every buffer, 0 on
 * success, sapcu_last_error() for the text).  SAPCU_ABI_VERSION is unchanged: these entry points are additions.
 *
 * Meshes are stored ragged: vertices f32 [total_vertices,3] and faces int32 [total_faces,3] (indices LOCAL to their mesh) of all S
 * meshes one after the other, vert_off / face_off int64 [S+1] the first row of every mesh (off[0] = 0, off[S] = the total).
 *
 * Semantics; every operation is one separately rounded f32 operation unless f64 is named.
 *   Per face (sapcu_surface_tables_f32):
 *     e1 = v1 - v0, e2 = v2 - v0;  c = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x);
 *     len = sqrtf((c.x^2 + c.y^2) + c.z^2), correctly rounded;  normal = c / max(len, 1e-8f);  area = 0.5f * len.
 *   Per mesh:
 *     area_sum = numpy's f32 `areas.sum()`: the pairwise sum of every 8192-element chunk (numpy's ufunc buffer) — fewer than 8
 *       values in sequence from 0; a leaf of at most 128 values with eight accumulators over its first n - n%8 values, combined as
 *       ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the rest added in order; above 128 values split at n/2 rounded down to a multiple of
 *       8 — and the chunk sums added in sequence from 0 (a mesh of at most 8192 faces is one pairwise sum);
 *     denom = area_sum + 1e-8f;  p[i] = (double)(area[i] / denom);
 *     cdf[i] = (...((p[0] + p[1]) + p[2]) ... + p[i]), a SEQUENTIAL f64 running sum;  prob_sum = cdf[F-1];
 *     cdf_out[i] = cdf[i] / prob_sum, an f64 division.
 *   Per sample point (sapcu_surface_sample_f32) of batch entry e (mesh m = mesh_idx[e]) with draws u (f64), r1, r2 (f32):
 *     face = the number of entries of mesh m's cdf slice that are <= u (numpy's searchsorted(side='right'), the rule of the legacy
 *       RandomState.choice), clamped to the mesh's last face; a face of zero area repeats its predecessor's cdf entry and is
 *       therefore never selected;
 *     s = sqrtf(r1) (correctly rounded), a = 1 - s, b = s * (1 - r2), w = s * r2;
 *     point = (a v0 + b v1) + w v2 per component;  normal = that face's row of face_normals;  face_out = the face, local to its mesh.
 * Coordinates and draws are expected to be finite (anything else gives unspecified values, never an access outside a buffer).
 *
 * Memory contract (as sapcu.h; checked under guard bands by tests/test_gpu_surface.py):
 *   - vertices, vert_off, faces, face_off, face_normals, cdf, mesh_idx [b] int64, u [b,n] f64, r1 [b,n], r2 [b,n] are only read;
 *     every output that is passed is written in full — face_normals_out [total_faces,3], cdf_out [total_faces] f64, area_sum_out [S]
 *     (the sum BEFORE + 1e-8f), prob_sum_out [S] f64; points_out [b,n,3], normals_out [b,n,3], face_out [b,n] int32 — and nothing else;
 *   - the workspace of sapcu_surface_tables_f32 (the face areas and the mesh sums) needs NO initialisation and 4-byte alignment;
 *     sapcu_surface_sample_f32 has no workspace;
 *   - S == 0 (tables, sample) or b == 0 (sample) launches nothing and writes nothing;
 *   - refused before anything is launched, with SAPCU_ERR_ARG: S < 0 or S > 2^20; total_faces outside 1..2^29; total_vertices
 *     outside 1..2^31-1; a NULL vertices, vert_off, faces, face_off, face_normals_out or cdf_out (tables; area_sum_out and
 *     prob_sum_out are optional); a NULL, short or misaligned workspace; n outside 1..4096; b outside 0..2^20; a NULL vertices,
 *     vert_off, faces, face_off, face_normals, cdf, mesh_idx, u, r1, r2, points_out or normals_out (sample; face_out is optional);
 *   - INDEX VALUES (the offsets, the faces' vertex indices, mesh_idx) are validated by the caller (sapcu_amd.surface does it and
 *     raises ValueError): neither entry point reads device memory on the host or synchronises `stream`, so both can be captured
 *     into a graph.  The kernels stay memory-safe on bad values: a face with a vertex index outside its mesh, or outside every
 *     mesh's face range, counts as area 0 and normal 0 (the sampler, should it meet one, writes a NaN point); a mesh whose offsets
 *     are not ascending inside [0, total] counts as empty (area_sum 0, prob_sum NaN, every batch entry that names it skipped); a
 *     batch entry whose mesh_idx is outside [0,S) is skipped whole (none of its output rows is written).
 * No float atomics: every result is the same bit pattern on every run.
 */
#ifndef SAPCU_SURFACE_H
#define SAPCU_SURFACE_H

#include "sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for the tables of S meshes with total_faces faces in all; -1 for sizes the call would refuse. */
int64_t sapcu_surface_tables_workspace_bytes(int64_t n_meshes, int64_t total_faces);

/* The per-mesh constants of the sampler: run once per data set (three launches, one workgroup per mesh for the two serial chains). */
int sapcu_surface_tables_f32(
    const float* vertices, const int64_t* vert_off, int64_t total_vertices,   /* [total_vertices,3], [S+1] */
    const int32_t* faces, const int64_t* face_off, int64_t total_faces,       /* [total_faces,3] local indices, [S+1] */
    int64_t n_meshes,
    float* face_normals_out,                         /* [total_faces,3] */
    double* cdf_out,                                 /* [total_faces]: every mesh's slice ends in 1.0 */
    float* area_sum_out,                             /* [S] or NULL */
    double* prob_sum_out,                            /* [S] or NULL */
    void* workspace, int64_t workspace_bytes,
    void* stream);

/* n surface points of each of b batch entries: one launch, no workspace, no host read-back.  points_out / normals_out have the
 * shape of sapcu_train_patches_f32's clouds / normals with n_samples = b. */
int sapcu_surface_sample_f32(
    const float* vertices, const int64_t* vert_off, int64_t total_vertices,
    const int32_t* faces, const int64_t* face_off, int64_t total_faces,
    const float* face_normals, const double* cdf,    /* the outputs of sapcu_surface_tables_f32 */
    int64_t n_meshes,
    const int64_t* mesh_idx, int64_t b,              /* the mesh of every batch entry (repeats allowed) */
    int n,
    const double* u,                                 /* [b,n] in [0,1): selects the face */
    const float* r1, const float* r2,                /* [b,n] in [0,1]: the position inside the face */
    float* points_out,                               /* [b,n,3] */
    float* normals_out,                              /* [b,n,3] */
    int32_t* face_out,                               /* [b,n] or NULL */
    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_SURFACE_H */
