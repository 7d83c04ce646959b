// Area-weighted sampling of triangle meshes (include/sapcu_surface.h): the face normals, the cumulative distribution of the face
// areas, and n surface points with their face normals per batch entry.
//
// Replaces the per-sample host work of the reference's fn/datacore.py:122-184 (numpy: np.cross, np.linalg.norm, ndarray.sum,
// RandomState.choice = cumsum + searchsorted).  Every value equals numpy's bit for bit, so the two sums keep numpy's order.
//
// Tables, once per data set (gfx950), three launches on the caller's stream, no host read-back:
//   * faces, one face per lane: the mesh of the face by a binary search of face_off, nine gathered coordinates, normal and area.
//     Bound by the gathers (36 B read, 16 B written per face).
//   * area sum, one 128-thread workgroup per mesh: numpy's pairwise tree over every 8192-element chunk, the chunk sums added in
//     sequence.  A full chunk's tree is perfect (64 leaves of 128 values): one leaf per lane with eight accumulators, then six
//     levels of neighbour pairs through LDS.  The last, shorter chunk: lane 0 lays its leaves (64..128 values each) out in LDS, one
//     leaf per lane, lane 0 folds them back up the tree with an LDS stack (leaf, plan and fold: wave_ops.h, in f32).
//   * cdf, one 256-thread workgroup per mesh: 1024-face tiles of p = (double)(area / denom) go coalesced into LDS, lane 0 runs the
//     dependent f64 add chain through the tile in place, all threads store the running sums; a second pass divides by the last one
//     (every thread re-reads what it wrote itself).  Bound by the F-step add chain: 15 ns per face, and keeping the next LDS reads
//     and the next tile's global loads in flight under the adds did not move it.
// Sampler, per batch, one launch: one lane per (entry, point) — an upper-bound binary search in the mesh's cdf slice (log2 F
// dependent f64 loads, L2 hits), three face indices, nine coordinates and the normal gathered, 11 f32 operations and one root.
// No scratch, no atomics.
#include "common.h"
#include "wave_ops.h"
#include "../../include/sapcu_surface.h"

namespace sapcu {

constexpr int SS_MAX_N = 4096;
constexpr int64_t SS_MAX_B = 1LL << 20;
constexpr int64_t SS_MAX_MESHES = 1LL << 20;
constexpr int64_t SS_MAX_FACES = 1LL << 29;
constexpr int64_t SS_MAX_VERTICES = 0x7fffffffLL;
constexpr int SS_CHUNK = 8192;          // numpy's default ufunc buffer: ndarray.sum() adds the pairwise sums of such chunks in sequence
constexpr int SS_MAX_LEAVES = 128;      // a leaf of a split node holds at least 64 values
constexpr int SS_STACK = 32;            // a chunk's tree is 7 levels deep
constexpr int SS_CDF_TILE = 1024;

struct SsMeshes {
    const float* vertices;      // [total_vertices,3]
    const int64_t* vert_off;    // [S+1]
    int64_t total_vertices;
    const int32_t* faces;       // [total_faces,3], indices local to the mesh
    const int64_t* face_off;    // [S+1]
    int64_t total_faces;
    int64_t S;
};

struct SsRange {
    int64_t first, count;       // count 0: offsets that are not ascending inside [0, total]
};

__device__ __forceinline__ SsRange ss_range(const int64_t* __restrict__ off, int64_t m, int64_t total) {
    const int64_t o = off[m], e = off[m + 1];
    if (o < 0 || e < o || e > total) return SsRange{0, 0};
    return SsRange{o, e - o};
}

// the correctly rounded f32 square root (train_patches.hip's tp_sqrtf: __fsqrt_rn is the approximate instruction)
__device__ __forceinline__ float ss_sqrtf(float x) { return (float)sqrt_cr((double)x); }

// ---------------------------------------------------------------------------------------------------------------- faces
__global__ __launch_bounds__(256) void ss_face_kernel(SsMeshes ms, float* __restrict__ normals_out, float* __restrict__ area) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ms.total_faces) return;
    int64_t lo = 0, hi = ms.S;                                   // the number of meshes that end at or before face f
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ms.face_off[mid + 1] <= f) lo = mid + 1;
        else hi = mid;
    }
    const int64_t m = lo < ms.S ? lo : ms.S - 1;
    const SsRange fr = ss_range(ms.face_off, m, ms.total_faces);
    const SsRange vr = ss_range(ms.vert_off, m, ms.total_vertices);
    const int64_t i0 = ms.faces[f * 3 + 0], i1 = ms.faces[f * 3 + 1], i2 = ms.faces[f * 3 + 2];
    const bool ok = f >= fr.first && f < fr.first + fr.count && i0 >= 0 && i0 < vr.count && i1 >= 0 && i1 < vr.count && i2 >= 0 &&
                    i2 < vr.count;
    float nx = 0.f, ny = 0.f, nz = 0.f, a = 0.f;                 // a face outside its mesh: area 0, normal 0
    if (ok) {
        const float* v0 = ms.vertices + (vr.first + i0) * 3;
        const float* v1 = ms.vertices + (vr.first + i1) * 3;
        const float* v2 = ms.vertices + (vr.first + i2) * 3;
        const float ax = __fsub_rn(v1[0], v0[0]), ay = __fsub_rn(v1[1], v0[1]), az = __fsub_rn(v1[2], v0[2]);
        const float bx = __fsub_rn(v2[0], v0[0]), by = __fsub_rn(v2[1], v0[1]), bz = __fsub_rn(v2[2], v0[2]);
        const float cx = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
        const float cy = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
        const float cz = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
        const float len = ss_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(cx, cx), __fmul_rn(cy, cy)), __fmul_rn(cz, cz)));
        const float den = fmaxf(len, 1e-8f);
        nx = __fdiv_rn(cx, den);
        ny = __fdiv_rn(cy, den);
        nz = __fdiv_rn(cz, den);
        a = __fmul_rn(0.5f, len);
    }
    normals_out[f * 3 + 0] = nx;
    normals_out[f * 3 + 1] = ny;
    normals_out[f * 3 + 2] = nz;
    area[f] = a;
}

// ------------------------------------------------------------------------------------------------------------- area sum
__global__ __launch_bounds__(128) void ss_area_sum_kernel(const int64_t* __restrict__ face_off, int64_t total_faces,
                                                          const float* __restrict__ area, float* __restrict__ sums) {
    __shared__ int leaf_o[SS_MAX_LEAVES], leaf_l[SS_MAX_LEAVES];
    __shared__ float leaf_s[SS_MAX_LEAVES];
    __shared__ int st_o[SS_STACK], st_l[SS_STACK], st_e[SS_STACK];
    __shared__ float vs[SS_STACK];
    __shared__ int nleaves;
    const int64_t m = blockIdx.x;
    const SsRange fr = ss_range(face_off, m, total_faces);       // block-uniform
    const int tid = threadIdx.x;
    const int count = (int)fr.count;                             // <= 2^29: the loops below count in 32 bits
    float total = 0.f;                                           // lane 0's: the chunk sums in sequence
    for (int c0 = 0; c0 < count; c0 += SS_CHUNK) {
        const int len = min(count - c0, SS_CHUNK);
        const float* a = area + fr.first + c0;
        if (len == SS_CHUNK) {                                   // (block-uniform) a full chunk's tree is perfect: 64 leaves of 128 values,
            if (tid < 64) leaf_s[tid] = np_leaf_sum(a + tid * 128, 128);      // neighbours added pair by pair, level by level
            __syncthreads();
            for (int s = 1; s < 64; s <<= 1) {
                if (tid < 64 && (tid & (2 * s - 1)) == 0) leaf_s[tid] = __fadd_rn(leaf_s[tid], leaf_s[tid + s]);   // tid + s is idle at this level
                __syncthreads();
            }
            if (tid == 0) total = __fadd_rn(total, leaf_s[0]);
            __syncthreads();                                     // leaf_s is rewritten by the next chunk
            continue;
        }
        if (tid == 0) nleaves = np_pairwise_plan<SS_MAX_LEAVES>(len, leaf_o, leaf_l, st_o, st_l);
        __syncthreads();
        const int nl = nleaves;
        for (int j = tid; j < nl; j += 128) leaf_s[j] = np_leaf_sum(a + leaf_o[j], leaf_l[j]);
        __syncthreads();
        if (tid == 0) total = __fadd_rn(total, np_pairwise_fold<float, SS_MAX_LEAVES>(len, leaf_s, st_l, st_e, vs));
        // (lane 0 rewrites the leaf table only after the next barrier-free stretch of its own: the other lanes read it between the
        //  two barriers above, and wait at the first one of the next chunk)
    }
    if (tid == 0) sums[m] = total;
}

// ------------------------------------------------------------------------------------------------------------------ cdf
__global__ __launch_bounds__(256) void ss_cdf_kernel(const int64_t* __restrict__ face_off, int64_t total_faces,
                                                     const float* __restrict__ area, const float* __restrict__ sums,
                                                     double* __restrict__ cdf_out, float* __restrict__ area_sum_out,
                                                     double* __restrict__ prob_sum_out) {
    __shared__ double p[SS_CDF_TILE];
    __shared__ double last;
    const int64_t m = blockIdx.x;
    const SsRange fr = ss_range(face_off, m, total_faces);       // block-uniform
    const int tid = threadIdx.x;
    const float total = sums[m];
    const float denom = __fadd_rn(total, 1e-8f);
    const float* a = area + fr.first;
    double* cdf = cdf_out + fr.first;
    double carry = 0.0;                                          // lane 0's: the running sum at the end of the previous tile
    const int count = (int)fr.count;                             // <= 2^29: the loops below count in 32 bits
    for (int base = 0; base < count; base += SS_CDF_TILE) {
        const int cnt = min(count - base, SS_CDF_TILE);
        for (int i = tid; i < cnt; i += 256) p[i] = (double)__fdiv_rn(a[base + i], denom);
        __syncthreads();
        if (tid == 0) {                                          // the serial chain: ((p0 + p1) + p2) + ... (numpy's cumsum)
            double run = carry;
            int i = 0;
            if (base == 0) run = p[i++];                         // cumsum starts from p[0] itself
#pragma unroll 8
            for (; i < cnt; ++i) {
                run = __dadd_rn(run, p[i]);
                p[i] = run;
            }
            carry = run;
        }
        __syncthreads();
        for (int i = tid; i < cnt; i += 256) cdf[base + i] = p[i];
        __syncthreads();                                         // the next tile overwrites p
    }
    if (tid == 0) last = count > 0 ? carry : __builtin_nan("");
    __syncthreads();
    const double prob_sum = last;
    for (int i = tid; i < count; i += 256) cdf[i] = __ddiv_rn(cdf[i], prob_sum);       // thread tid wrote these rows itself
    if (tid == 0) {
        if (prob_sum_out) prob_sum_out[m] = prob_sum;
        if (area_sum_out) area_sum_out[m] = total;
    }
}

// -------------------------------------------------------------------------------------------------------------- sampler
__global__ __launch_bounds__(256) void ss_sample_kernel(SsMeshes ms, const float* __restrict__ face_normals,
                                                        const double* __restrict__ cdf, const int64_t* __restrict__ mesh_idx,
                                                        int64_t b, int n, const double* __restrict__ u, const float* __restrict__ r1,
                                                        const float* __restrict__ r2, float* __restrict__ points_out,
                                                        float* __restrict__ normals_out, int32_t* __restrict__ face_out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= b * n) return;
    const int64_t e = t / n;
    const int64_t m = mesh_idx[e];
    if (m < 0 || m >= ms.S) return;                              // a bad mesh index: nothing of this entry is written
    const SsRange fr = ss_range(ms.face_off, m, ms.total_faces);
    const SsRange vr = ss_range(ms.vert_off, m, ms.total_vertices);
    if (fr.count < 1) return;                                    // an empty mesh: skipped like a bad index
    const double* c = cdf + fr.first;
    const double uu = u[t];
    int64_t lo = 0, hi = fr.count;                               // the number of cdf entries <= u
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (c[mid] <= uu) lo = mid + 1;
        else hi = mid;
    }
    const int64_t face = lo < fr.count ? lo : fr.count - 1;
    const int64_t f = fr.first + face;
    const int64_t i0 = ms.faces[f * 3 + 0], i1 = ms.faces[f * 3 + 1], i2 = ms.faces[f * 3 + 2];
    const bool ok = i0 >= 0 && i0 < vr.count && i1 >= 0 && i1 < vr.count && i2 >= 0 && i2 < vr.count;
    float px = __builtin_nanf(""), py = px, pz = px;
    if (ok) {
        const float* v0 = ms.vertices + (vr.first + i0) * 3;
        const float* v1 = ms.vertices + (vr.first + i1) * 3;
        const float* v2 = ms.vertices + (vr.first + i2) * 3;
        const float q = r2[t];
        const float s = ss_sqrtf(r1[t]);
        const float wa = __fsub_rn(1.0f, s);
        const float wb = __fmul_rn(s, __fsub_rn(1.0f, q));
        const float wc = __fmul_rn(s, q);
        px = __fadd_rn(__fadd_rn(__fmul_rn(wa, v0[0]), __fmul_rn(wb, v1[0])), __fmul_rn(wc, v2[0]));
        py = __fadd_rn(__fadd_rn(__fmul_rn(wa, v0[1]), __fmul_rn(wb, v1[1])), __fmul_rn(wc, v2[1]));
        pz = __fadd_rn(__fadd_rn(__fmul_rn(wa, v0[2]), __fmul_rn(wb, v1[2])), __fmul_rn(wc, v2[2]));
    }
    points_out[t * 3 + 0] = px;
    points_out[t * 3 + 1] = py;
    points_out[t * 3 + 2] = pz;
    const float* nr = face_normals + f * 3;
    normals_out[t * 3 + 0] = nr[0];
    normals_out[t * 3 + 1] = nr[1];
    normals_out[t * 3 + 2] = nr[2];
    if (face_out) face_out[t] = (int32_t)face;
}

// the workspace of sapcu_surface_tables_f32: sizer (null base) and carver in one
struct SsWorkspace {
    float* area;    // [total_faces]
    float* sums;    // [S]
};
static size_t ss_layout(void* base, int64_t n_meshes, int64_t total_faces, SsWorkspace* w) {
    WsCarver c(base, 4);
    w->area = c.take<float>(total_faces);
    w->sums = c.take<float>(n_meshes);
    return c.bytes();
}
static bool ss_sizes_ok(int64_t n_meshes, int64_t total_faces) {
    return n_meshes >= 0 && n_meshes <= SS_MAX_MESHES && total_faces >= 1 && total_faces <= SS_MAX_FACES;
}

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

extern "C" {

int64_t sapcu_surface_tables_workspace_bytes(int64_t n_meshes, int64_t total_faces) {
    if (!ss_sizes_ok(n_meshes, total_faces)) return -1;
    SsWorkspace w;
    return (int64_t)ss_layout(nullptr, n_meshes, total_faces, &w);
}

int sapcu_surface_tables_f32(const float* vertices, const int64_t* vert_off, int64_t total_vertices, const int32_t* faces,
                             const int64_t* face_off, int64_t total_faces, int64_t n_meshes, float* face_normals_out, double* cdf_out,
                             float* area_sum_out, double* prob_sum_out, void* workspace, int64_t workspace_bytes, void* stream) {
    SAPCU_CHECK_ARG(n_meshes >= 0 && n_meshes <= SS_MAX_MESHES, "surface_tables: need 0 <= n_meshes <= 2^20 (%lld)", (long long)n_meshes);
    SAPCU_CHECK_ARG(total_faces >= 1 && total_faces <= SS_MAX_FACES, "surface_tables: need 1 <= total_faces <= 2^29 (%lld)",
                    (long long)total_faces);
    SAPCU_CHECK_ARG(total_vertices >= 1 && total_vertices <= SS_MAX_VERTICES, "surface_tables: need 1 <= total_vertices < 2^31 (%lld)",
                    (long long)total_vertices);
    SAPCU_CHECK_ARG(vertices && vert_off && faces && face_off && face_normals_out && cdf_out, "surface_tables: null pointer");
    SsWorkspace w;
    const int64_t need = (int64_t)ss_layout(workspace, n_meshes, total_faces, &w);
    SAPCU_CHECK_ARG(workspace && ((uintptr_t)workspace & 3) == 0 && workspace_bytes >= need,
                    "surface_tables: workspace of %lld bytes at a 4-byte aligned address, need %lld", (long long)workspace_bytes,
                    (long long)need);
    if (n_meshes == 0) return SAPCU_OK;
    hipStream_t st = (hipStream_t)stream;
    const SsMeshes ms{vertices, vert_off, total_vertices, faces, face_off, total_faces, n_meshes};
    hipLaunchKernelGGL(ss_face_kernel, dim3((unsigned)((total_faces + 255) / 256)), dim3(256), 0, st, ms, face_normals_out, w.area);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(ss_area_sum_kernel, dim3((unsigned)n_meshes), dim3(128), 0, st, face_off, total_faces, (const float*)w.area, w.sums);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(ss_cdf_kernel, dim3((unsigned)n_meshes), dim3(256), 0, st, face_off, total_faces, (const float*)w.area,
                       (const float*)w.sums, cdf_out, area_sum_out, prob_sum_out);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int sapcu_surface_sample_f32(const float* vertices, const int64_t* vert_off, int64_t total_vertices, const int32_t* faces,
                             const int64_t* face_off, int64_t total_faces, const float* face_normals, const double* cdf, int64_t n_meshes,
                             const int64_t* mesh_idx, int64_t b, int n, const double* u, const float* r1, const float* r2,
                             float* points_out, float* normals_out, int32_t* face_out, void* stream) {
    SAPCU_CHECK_ARG(n_meshes >= 0 && n_meshes <= SS_MAX_MESHES, "surface_sample: need 0 <= n_meshes <= 2^20 (%lld)", (long long)n_meshes);
    SAPCU_CHECK_ARG(total_faces >= 1 && total_faces <= SS_MAX_FACES, "surface_sample: need 1 <= total_faces <= 2^29 (%lld)",
                    (long long)total_faces);
    SAPCU_CHECK_ARG(total_vertices >= 1 && total_vertices <= SS_MAX_VERTICES, "surface_sample: need 1 <= total_vertices < 2^31 (%lld)",
                    (long long)total_vertices);
    SAPCU_CHECK_ARG(n >= 1 && n <= SS_MAX_N, "surface_sample: need 1 <= n <= %d (n=%d)", SS_MAX_N, n);
    SAPCU_CHECK_ARG(b >= 0 && b <= SS_MAX_B, "surface_sample: need 0 <= b <= 2^20 (b=%lld)", (long long)b);
    SAPCU_CHECK_ARG(vertices && vert_off && faces && face_off && face_normals && cdf && mesh_idx && u && r1 && r2 && points_out &&
                        normals_out,
                    "surface_sample: null pointer");
    if (b == 0 || n_meshes == 0) return SAPCU_OK;
    const SsMeshes ms{vertices, vert_off, total_vertices, faces, face_off, total_faces, n_meshes};
    const int64_t blocks = (b * n + 255) / 256;                  // <= 2^24
    hipLaunchKernelGGL(ss_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ms, face_normals, cdf, mesh_idx, b, n,
                       u, r1, r2, points_out, normals_out, face_out);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

}  // extern "C"
