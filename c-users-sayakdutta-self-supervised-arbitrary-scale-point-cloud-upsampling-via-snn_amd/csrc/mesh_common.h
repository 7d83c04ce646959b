// What the translation units that work on triangle meshes share (mesh_dist.hip: the distance to a mesh; ray_cast.hip: ray casting):
// the face record with its skip rule, the dot product in the definition's order, the counters of a call, the per-wave LDS slab scan
// of a range of faces, the argument checks and the brute-force route of the entry points, and the
// launchers of the two face passes that live in mesh_dist.hip (a kernel is launched from the file that defines it).
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

// The records load(j), j in [a, b), against every lane's query: a wavefront gathers 64 records at a time into its own LDS slab (one per
// lane, coalesced) and reads them back one at a time, all lanes at one address: a broadcast.  test(rec) runs in every lane for every
// record with idx >= 0; a skipped face costs one wave-uniform branch.
template <typename Rec, typename Load, typename Test>
__device__ __forceinline__ void mesh_slab_scan(int a, int b, Rec* slab, int lane, Load load, Test test) {
    for (int off = a; off < b; off += 64) {
        const int j = off + lane;
        Rec mine{};
        mine.idx = -1;
        if (j < b) mine = load(j);
        __builtin_amdgcn_wave_barrier();
        slab[lane] = mine;
        __builtin_amdgcn_wave_barrier();
        const int cnt = min(64, b - off);                                   // wave-uniform
#pragma unroll 2
        for (int t = 0; t < cnt; ++t) {
            const Rec m = slab[t];
            if (m.idx < 0) continue;                                        // wave-uniform
            test(m);
        }
    }
}

// ------------------------------------------------------------------------------------------------------- host side
static inline bool mesh_sizes_ok(int64_t nv, int64_t nf, int64_t nq) {
    return nv >= 1 && nv <= (1LL << 31) - 1 && nf >= 1 && nf <= (1LL << 29) && nq >= 0 && nq <= (1LL << 31) - 64;
}

// the argument checks of every entry point that takes a mesh and `nq` queries or rays (named `qname` in the messages); `need`: the
// entry point's workspace size, read only once the sizes are in range
static int mesh_args_check(const char* who, const char* qname, const void* vertices, int64_t nv, const void* faces, int64_t nf,
                           bool rest_given, int64_t nq, double cell_size, void* workspace, int64_t workspace_bytes, int64_t need) {
    SAPCU_CHECK_ARG(nv >= 1 && nv <= (1LL << 31) - 1, "%s: need 1 <= nv <= 2^31 - 1 (nv=%lld)", who, (long long)nv);
    SAPCU_CHECK_ARG(nf >= 1 && nf <= (1LL << 29), "%s: need 1 <= nf <= 2^29 (nf=%lld)", who, (long long)nf);
    SAPCU_CHECK_ARG(nq >= 0 && nq <= (1LL << 31) - 64, "%s: need 0 <= %s <= 2^31 - 64 (%s=%lld)", who, qname, qname, (long long)nq);
    SAPCU_CHECK_ARG(vertices && faces && (rest_given || nq == 0), "%s: null pointer", who);       // no query: nothing is written
    SAPCU_CHECK_ARG(cell_size >= 0.0 && cell_size < 1e300, "%s: cell_size must be finite and >= 0", who);
    SAPCU_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "%s: the workspace must be 8-byte aligned (f64 tables)", who);
    SAPCU_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace of %lld bytes, need %lld", who, (long long)workspace_bytes,
                    (long long)need);
    return SAPCU_OK;
}

// mesh_dist.hip: centroid c' = ((a + b) + c) / 3 and radius r_f = max |vertex - c'| * (1 + 1e-9) of every face, the skipped faces
// counted into ctl->n_skip (centroid NULL: the count alone); the oversize list (radius above mult cell edges of prm) with its length in
// ctl->n_over, and the bits of the largest radius of the other faces in ctl->rbits.  *ctl is zeroed by the caller.
int launch_mesh_prep(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, double* centroid, double* radius, MeshCtl* ctl,
                     hipStream_t st);
int launch_mesh_classify(const double* radius, int64_t nf, const GridParams* prm, double mult, int* olist, MeshCtl* ctl, hipStream_t st);

// a call that goes straight to brute force, launched by brute(): the skipped faces are counted into info[5] (the face pass without
// centroids, one read-back of *ctl) only for a caller who asks
template <typename Brute>
static int mesh_brute_route(const double* vertices, int64_t nv, const int32_t* faces, int64_t nf, MeshCtl* ctl, int64_t* info, hipStream_t st,
                            Brute brute) {
    if (info) {
        SAPCU_CHECK_HIP(hipMemsetAsync(ctl, 0, sizeof(MeshCtl), st));
        const int rc = launch_mesh_prep(vertices, nv, faces, nf, nullptr, nullptr, ctl, st);
        if (rc != SAPCU_OK) return rc;
    }
    const int rc = brute();
    if (rc != SAPCU_OK || !info) return rc;
    MeshCtl hc;
    SAPCU_CHECK_HIP(hipMemcpyAsync(&hc, ctl, sizeof(hc), hipMemcpyDeviceToHost, st));
    SAPCU_CHECK_HIP(hipStreamSynchronize(st));
    info[5] = hc.n_skip;
    return SAPCU_OK;
}

}  // namespace sapcu
