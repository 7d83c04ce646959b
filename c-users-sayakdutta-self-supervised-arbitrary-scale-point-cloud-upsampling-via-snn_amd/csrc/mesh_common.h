// What the translation units that work on triangle meshes share (mesh_dist.hip: the distance to a mesh; ray_cast.hip: ray casting):
// the face record with its skip rule, the dot product in the definition's order, the counters of a call, and the launchers of the two
// face passes that live in mesh_dist.hip (a kernel is launched from the file that defines it).
#pragma once
#include "common.h"
#include "knn_grid.h"

namespace sapcu {

constexpr int MESH_WAVES = 4;

struct MeshCtl {
    unsigned long long rbits;    // bits of the largest radius among in-grid faces
    int n_over;                  // faces on the oversize list
    int n_skip;                  // skipped faces
};

__device__ __forceinline__ double mesh_dot(double ux, double uy, double uz, double vx, double vy, double vz) {
    return __dadd_rn(__dadd_rn(__dmul_rn(ux, vx), __dmul_rn(uy, vy)), __dmul_rn(uz, vz));
}

struct __align__(16) MeshFace {
    double ax, ay, az, bx, by, bz, cx, cy, cz;
    int idx, pad;                // idx < 0: skipped (or a spare slot of the slab)
};

struct MeshBest {
    double d;
    int f;
    double qx, qy, qz;
};

// the face's record; idx = f, or -1 when the face is skipped (an index out of range, dot(n, n) zero or not finite)
__device__ __forceinline__ MeshFace mesh_load_face(int f, const double* __restrict__ vertices, int64_t nv, const int32_t* __restrict__ faces) {
    MeshFace m{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1, 0};
    const int32_t* t = faces + (int64_t)f * 3;
    const int64_t i0 = t[0], i1 = t[1], i2 = t[2];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) return m;
    m.ax = vertices[i0 * 3 + 0];
    m.ay = vertices[i0 * 3 + 1];
    m.az = vertices[i0 * 3 + 2];
    m.bx = vertices[i1 * 3 + 0];
    m.by = vertices[i1 * 3 + 1];
    m.bz = vertices[i1 * 3 + 2];
    m.cx = vertices[i2 * 3 + 0];
    m.cy = vertices[i2 * 3 + 1];
    m.cz = vertices[i2 * 3 + 2];
    const double abx = __dsub_rn(m.bx, m.ax), aby = __dsub_rn(m.by, m.ay), abz = __dsub_rn(m.bz, m.az);
    const double acx = __dsub_rn(m.cx, m.ax), acy = __dsub_rn(m.cy, m.ay), acz = __dsub_rn(m.cz, m.az);
    const double nx = __dsub_rn(__dmul_rn(aby, acz), __dmul_rn(abz, acy));
    const double ny = __dsub_rn(__dmul_rn(abz, acx), __dmul_rn(abx, acz));
    const double nz = __dsub_rn(__dmul_rn(abx, acy), __dmul_rn(aby, acx));
    const double nn = mesh_dot(nx, ny, nz, nx, ny, nz);
    if (nn > 0.0 && nn < __builtin_huge_val()) m.idx = f;
    return m;
}

// mesh_dist.hip: centroid c' = ((a + b) + c) / 3 and radius r_f = max |vertex - c'| * (1 + 1e-9) of every face, the skipped faces
// counted into ctl->n_skip (centroid NULL: the count alone); the oversize list (radius above mult cell edges of prm) with its length in
// ctl->n_over, and the bits of the largest radius of the other faces in ctl->rbits.  *ctl is zeroed by the caller.
int launch_mesh_prep(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, double* centroid, double* radius, MeshCtl* ctl,
                     hipStream_t st);
int launch_mesh_classify(const double* radius, int64_t nf, const GridParams* prm, double mult, int* olist, MeshCtl* ctl, hipStream_t st);

}  // namespace sapcu
