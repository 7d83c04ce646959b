// Training samples of fd and fn from raw cloud pairs (include/sapcu_data.h): augmentation, normalisation, the distance of every
// point to the denser cloud, and the k nearest cloud points of every patch centre.
//
// Replaces the per-sample host work of the reference's fd/datacore.py:91-149 and fn/datacore.py:201-258 (numpy + two cKDTree builds).
//
// Three kernels per batch (gfx950), all on the caller's stream, no host read-back:
//   * prepare, one 256-thread workgroup per batch entry: the augmented cloud sits in LDS as an f32 SoA tile (n <= 4096: 48 KiB);
//     lanes 0..2 run the three serial centroid chains (row 0 + row 1 + ...: the order numpy's mean(axis=0) adds in), the block takes
//     the largest squared radius (sqrtf is monotone, so sqrtf(max) = max(sqrtf)), then cloud, dense and normals are written;
//     centroid and radius go to the workspace for the distance kernel.  Bound by the latency of the n-step add chain.
//   * nearest-dense, one workgroup per (entry, 64 cloud points): one query per lane, the four waves each scan a quarter of every
//     1024-point LDS tile of the dense cloud (transformed while it is loaded, the same operations as prepare's dense_out), and the
//     four partial minima are combined through LDS (a minimum does not depend on the order).  f64 VALU.
//   * neighbours, one workgroup per (entry, 8 centres): the entry's normalised cloud in LDS (f32 SoA, 12 n bytes of dynamic LDS), one
//     centre per wave at a time;
//     the k-list is WaveTopK in arrival order (wave_ops.h) — a sorted list spread over the lanes, the first 64-point slab sorted by
//     a bitonic network on (distance, index), later candidates in ascending index against the k-th distance with strict '<'.  f64 VALU.
// No scratch, no atomics.
#include "common.h"
#include "wave_ops.h"
#include "../../include/sapcu_data.h"

namespace sapcu {

constexpr int TP_MAX_N = 4096;
constexpr int TP_MAX_G = 65536;
constexpr int TP_MAX_K = 128;
constexpr int TP_CENTRES_PER_WG = 8;
constexpr int TP_DENSE_TILE = 1024;

struct TpAug {
    const float* rot;      // [b,9] or null
    const float* scale;    // [b] or null
    const float* jitter;   // [b,n,3] or null
};

struct TpPoint {
    float x, y, z;
};

// The correctly rounded f32 square root numpy takes.  (HIP's __fsqrt_rn is the hardware's approximate v_sqrt_f32, an ulp off for
// about one argument in seven.)  Through f64: common.h's correctly rounded f64 root, then one more rounding — innocuous for a
// square root, 53 >= 2 * 24 + 2 bits.
__device__ __forceinline__ float tp_sqrtf(float x) { return (float)sqrt_cr((double)x); }

__device__ __forceinline__ TpPoint tp_rotate(TpPoint p, const float* __restrict__ r) {
    TpPoint o;
    o.x = __fadd_rn(__fadd_rn(__fmul_rn(p.x, r[0]), __fmul_rn(p.y, r[1])), __fmul_rn(p.z, r[2]));
    o.y = __fadd_rn(__fadd_rn(__fmul_rn(p.x, r[3]), __fmul_rn(p.y, r[4])), __fmul_rn(p.z, r[5]));
    o.z = __fadd_rn(__fadd_rn(__fmul_rn(p.x, r[6]), __fmul_rn(p.y, r[7])), __fmul_rn(p.z, r[8]));
    return o;
}

// rotation and scale of one cloud or dense point of batch entry bi (jitter is the cloud's alone)
__device__ __forceinline__ TpPoint tp_augment(TpPoint p, const TpAug& a, int64_t bi) {
    if (a.rot) p = tp_rotate(p, a.rot + bi * 9);
    if (a.scale) {
        const float s = a.scale[bi];
        p.x = __fmul_rn(p.x, s);
        p.y = __fmul_rn(p.y, s);
        p.z = __fmul_rn(p.z, s);
    }
    return p;
}

// centre on the cloud's centroid, divide by its radius when that is > 0   (st = {cx, cy, cz, radius})
__device__ __forceinline__ TpPoint tp_normalise(TpPoint p, const float* __restrict__ st) {
    p.x = __fsub_rn(p.x, st[0]);
    p.y = __fsub_rn(p.y, st[1]);
    p.z = __fsub_rn(p.z, st[2]);
    const float r = st[3];
    if (r > 0.f) {
        p.x = __fdiv_rn(p.x, r);
        p.y = __fdiv_rn(p.y, r);
        p.z = __fdiv_rn(p.z, r);
    }
    return p;
}

// a normal of batch entry bi: rotated, then n / (|n| + 1e-8)
__device__ __forceinline__ TpPoint tp_normal(const float* __restrict__ nrm, const TpAug& a, int64_t bi) {
    TpPoint p{nrm[0], nrm[1], nrm[2]};
    if (a.rot) p = tp_rotate(p, a.rot + bi * 9);
    const float len = tp_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y)), __fmul_rn(p.z, p.z)));
    const float den = __fadd_rn(len, 1e-8f);
    return TpPoint{__fdiv_rn(p.x, den), __fdiv_rn(p.y, den), __fdiv_rn(p.z, den)};
}

// ------------------------------------------------------------------------------------------------------------ prepare
__global__ __launch_bounds__(256) void tp_prepare_kernel(const float* __restrict__ clouds, int64_t n_samples, int n,
                                                         const float* __restrict__ dense, int g, const float* __restrict__ normals,
                                                         const int64_t* __restrict__ sample_idx, TpAug aug,
                                                         float* __restrict__ cloud_out, float* __restrict__ dense_out,
                                                         float* __restrict__ normals_out, float* __restrict__ stats) {
    __shared__ float tile[3][TP_MAX_N];
    __shared__ float st[4];
    __shared__ float wmax[4];
    const int64_t bi = blockIdx.x;
    const int64_t s = sample_idx[bi];
    if (s < 0 || s >= n_samples) return;                         // (block-uniform) a bad sample index: nothing of this entry is written
    const int tid = threadIdx.x;
    const float* src = clouds + s * n * 3;
    for (int p = tid; p < n; p += 256) {
        TpPoint q = tp_augment(TpPoint{src[p * 3 + 0], src[p * 3 + 1], src[p * 3 + 2]}, aug, bi);
        if (aug.jitter) {
            const float* j = aug.jitter + (bi * n + p) * 3;
            q.x = __fadd_rn(q.x, j[0]);
            q.y = __fadd_rn(q.y, j[1]);
            q.z = __fadd_rn(q.z, j[2]);
        }
        tile[0][p] = q.x;
        tile[1][p] = q.y;
        tile[2][p] = q.z;
    }
    __syncthreads();
    if (tid < 3) {                                               // the serial chains: row 0, + row 1, + ... (numpy's order), then / n
        const float* a = tile[tid];
        float sum = a[0];
        for (int i = 1; i < n; ++i) sum = __fadd_rn(sum, a[i]);
        st[tid] = __fdiv_rn(sum, (float)n);
    }
    __syncthreads();
    float m = 0.f;                                               // squared radii are >= 0
    for (int p = tid; p < n; p += 256) {
        const float x = __fsub_rn(tile[0][p], st[0]), y = __fsub_rn(tile[1][p], st[1]), z = __fsub_rn(tile[2][p], st[2]);
        tile[0][p] = x;
        tile[1][p] = y;
        tile[2][p] = z;
        m = fmaxf(m, __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
    }
    m = wave_max(m);
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) st[3] = tp_sqrtf(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
    __syncthreads();
    const float r = st[3];
    if (tid < 4) stats[bi * 4 + tid] = st[tid];
    float* co = cloud_out + bi * n * 3;
    for (int p = tid; p < n; p += 256) {
        float x = tile[0][p], y = tile[1][p], z = tile[2][p];
        if (r > 0.f) {
            x = __fdiv_rn(x, r);
            y = __fdiv_rn(y, r);
            z = __fdiv_rn(z, r);
        }
        co[p * 3 + 0] = x;
        co[p * 3 + 1] = y;
        co[p * 3 + 2] = z;
    }
    if (dense_out) {
        const float* d = dense + s * g * 3;
        float* o = dense_out + bi * g * 3;
        for (int p = tid; p < g; p += 256) {
            const TpPoint q = tp_normalise(tp_augment(TpPoint{d[p * 3 + 0], d[p * 3 + 1], d[p * 3 + 2]}, aug, bi), st);
            o[p * 3 + 0] = q.x;
            o[p * 3 + 1] = q.y;
            o[p * 3 + 2] = q.z;
        }
    }
    if (normals_out) {
        const float* nr = normals + s * n * 3;
        float* o = normals_out + bi * n * 3;
        for (int p = tid; p < n; p += 256) {
            const TpPoint q = tp_normal(nr + p * 3, aug, bi);
            o[p * 3 + 0] = q.x;
            o[p * 3 + 1] = q.y;
            o[p * 3 + 2] = q.z;
        }
    }
}

// ------------------------------------------------------------------------------------------------------ nearest dense
__global__ __launch_bounds__(256) void tp_len_kernel(const float* __restrict__ dense, int64_t n_samples, int g,
                                                     const int64_t* __restrict__ sample_idx, TpAug aug,
                                                     const float* __restrict__ cloud_out, int n, const float* __restrict__ stats,
                                                     int slabs, float* __restrict__ len_out) {
    __shared__ float tile[3][TP_DENSE_TILE];
    __shared__ double part[4][64];
    __shared__ float st[4];
    const int64_t bi = blockIdx.x / slabs;
    const int slab = blockIdx.x % slabs;
    const int64_t s = sample_idx[bi];
    if (s < 0 || s >= n_samples) return;                         // block-uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 4) st[tid] = stats[bi * 4 + tid];
    const int qi = slab * 64 + lane;
    const bool valid = qi < n;
    const float* q3 = cloud_out + (bi * n + (valid ? qi : 0)) * 3;
    const double qx = q3[0], qy = q3[1], qz = q3[2];
    const float* d = dense + s * g * 3;
    double best = __builtin_huge_val();
    for (int base = 0; base < g; base += TP_DENSE_TILE) {
        const int cnt = min(g - base, TP_DENSE_TILE);
        __syncthreads();                                         // (also orders st[] before its first use)
        for (int p = tid; p < cnt; p += 256) {
            const float* d3 = d + (int64_t)(base + p) * 3;
            const TpPoint t = tp_normalise(tp_augment(TpPoint{d3[0], d3[1], d3[2]}, aug, bi), st);
            tile[0][p] = t.x;
            tile[1][p] = t.y;
            tile[2][p] = t.z;
        }
        __syncthreads();
        const int quarter = (cnt + 3) >> 2;
        const int j0 = wave * quarter, j1 = min(j0 + quarter, cnt);
        double other = best;                                     // two chains: a minimum does not depend on the order
        int j = j0;
#pragma unroll 4
        for (; j + 1 < j1; j += 2) {
            best = fmin(best, dist2_rn(qx, qy, qz, tile[0][j], tile[1][j], tile[2][j]));
            other = fmin(other, dist2_rn(qx, qy, qz, tile[0][j + 1], tile[1][j + 1], tile[2][j + 1]));
        }
        if (j < j1) best = fmin(best, dist2_rn(qx, qy, qz, tile[0][j], tile[1][j], tile[2][j]));
        best = fmin(best, other);
    }
    part[wave][lane] = best;
    __syncthreads();
    if (wave == 0 && valid) {
        const double m = fmin(fmin(part[0][lane], part[1][lane]), fmin(part[2][lane], part[3][lane]));
        len_out[bi * n + qi] = (float)sqrt_cr(m);
    }
}

// ---------------------------------------------------------------------------------------------------------- neighbours
// TWO = the list needs the second slot per lane (k > 64); fd's k = 32 and fn's k = 12 run the one-slot instance.
template <bool TWO>
__global__ __launch_bounds__(256) void tp_knn_kernel(const float* __restrict__ cloud_out, int n, const float* __restrict__ normals,
                                                     int64_t n_samples, const int64_t* __restrict__ sample_idx, TpAug aug,
                                                     const int32_t* __restrict__ centres, int pc, int k, int slabs,
                                                     float* __restrict__ patches_out, int32_t* __restrict__ idx_out,
                                                     float* __restrict__ patch_normals_out) {
    extern __shared__ float tp_cloud_tile[];                     // [3][n], sized by the launch: a small cloud leaves the CU to 8 workgroups
    float* const tile[3] = {tp_cloud_tile, tp_cloud_tile + n, tp_cloud_tile + 2 * n};
    const int64_t bi = blockIdx.x / slabs;
    const int slab = blockIdx.x % slabs;
    const int64_t s = sample_idx[bi];
    if (s < 0 || s >= n_samples) return;                         // block-uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* c = cloud_out + bi * n * 3;
    for (int p = tid; p < n; p += 256) {
        tile[0][p] = c[p * 3 + 0];
        tile[1][p] = c[p * 3 + 1];
        tile[2][p] = c[p * 3 + 2];
    }
    __syncthreads();                                             // the only barrier: from here on every wave runs on its own
    const double INF = __builtin_huge_val();
    for (int cw = wave; cw < TP_CENTRES_PER_WG; cw += 4) {
        const int ci = slab * TP_CENTRES_PER_WG + cw;
        if (ci >= pc) break;                                     // wave-uniform
        const int centre = centres ? centres[bi * pc + ci] : ci;
        if (centre < 0 || centre >= n) continue;                 // a bad centre: its rows are not written (wave-uniform)
        const double qx = tile[0][centre], qy = tile[1][centre], qz = tile[2][centre];
        WaveTopK<TWO> top(k);
        for (int off = 0; off < n; off += 64) {
            const int j = off + lane;
            const double d = j < n ? dist2_rn(qx, qy, qz, tile[0][j], tile[1][j], tile[2][j]) : INF;
            if (off == 0) top.first_slab(d, j < n ? j : 0x7fffffff);      // lanes past the cloud: INF, last
            else top.offer(d, off);
        }
        const int64_t row = (bi * pc + ci) * k;
#pragma unroll
        for (int slot = 0; slot < top.SLOTS; ++slot) {
            const int p = lane + 64 * slot;
            if (p >= k) continue;
            const int i = top.i[slot];
            const bool ok = i >= 0 && i < n;                     // (a non-finite cloud can leave entries empty: NaN rows, index -1)
            if (idx_out) idx_out[row + p] = ok ? i : -1;
            float* o = patches_out + (row + p) * 3;
            const float nanv = __builtin_nanf("");
            o[0] = ok ? tile[0][i] : nanv;
            o[1] = ok ? tile[1][i] : nanv;
            o[2] = ok ? tile[2][i] : nanv;
        }
        if (patch_normals_out && lane == 0) {
            const TpPoint q = tp_normal(normals + (s * n + centre) * 3, aug, bi);
            float* o = patch_normals_out + (bi * pc + ci) * 3;
            o[0] = q.x;
            o[1] = q.y;
            o[2] = q.z;
        }
    }
}

static int64_t tp_workspace_bytes(int64_t b) { return b * 4 * (int64_t)sizeof(float); }

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

extern "C" {

int64_t sapcu_train_patches_workspace_bytes(int64_t b) {
    if (b < 0 || b > (1LL << 20)) return -1;
    return tp_workspace_bytes(b);
}

int sapcu_train_patches_f32(const float* clouds, int64_t n_samples, int n, const float* dense, int g, const float* normals,
                            const int64_t* sample_idx, int64_t b, const float* rot, const float* scale, const float* jitter,
                            const int32_t* centres, int pc, int k, float* patches_out, int32_t* idx_out, float* cloud_out,
                            float* dense_out, float* len_out, float* normals_out, float* patch_normals_out, void* workspace,
                            int64_t workspace_bytes, void* stream) {
    SAPCU_CHECK_ARG(n >= 1 && n <= TP_MAX_N, "train_patches: need 1 <= n <= %d (n=%d)", TP_MAX_N, n);
    SAPCU_CHECK_ARG(g >= 0 && g <= TP_MAX_G, "train_patches: need 0 <= g <= %d (g=%d)", TP_MAX_G, g);
    SAPCU_CHECK_ARG(k >= 1 && k <= n && k <= TP_MAX_K, "train_patches: need 1 <= k <= min(n, %d) (k=%d, n=%d)", TP_MAX_K, k, n);
    SAPCU_CHECK_ARG(pc >= 1 && pc <= (1 << 20), "train_patches: need 1 <= pc <= 2^20 (pc=%d)", pc);
    SAPCU_CHECK_ARG(centres || pc == n, "train_patches: without centres every point is one (pc=%d, n=%d)", pc, n);
    SAPCU_CHECK_ARG(n_samples >= 1, "train_patches: need n_samples >= 1 (%lld)", (long long)n_samples);
    SAPCU_CHECK_ARG(b >= 0 && b <= (1LL << 20), "train_patches: need 0 <= b <= 2^20 (b=%lld)", (long long)b);
    SAPCU_CHECK_ARG((dense != nullptr) == (g > 0), "train_patches: dense and g > 0 go together (g=%d)", g);
    SAPCU_CHECK_ARG(dense || (!dense_out && !len_out), "train_patches: dense_out / len_out need dense");
    SAPCU_CHECK_ARG(normals || (!normals_out && !patch_normals_out), "train_patches: normals_out / patch_normals_out need normals");
    const int slabs = (pc + TP_CENTRES_PER_WG - 1) / TP_CENTRES_PER_WG;
    SAPCU_CHECK_ARG(b * slabs < (1LL << 31), "train_patches: b * ceil(pc / %d) must stay below 2^31", TP_CENTRES_PER_WG);
    if (b == 0) return SAPCU_OK;
    SAPCU_CHECK_ARG(clouds && sample_idx && patches_out && cloud_out, "train_patches: null pointer");
    SAPCU_CHECK_ARG(workspace && ((uintptr_t)workspace & 3) == 0 && workspace_bytes >= tp_workspace_bytes(b),
                    "train_patches: workspace of %lld bytes at a 4-byte aligned address, need %lld", (long long)workspace_bytes,
                    (long long)tp_workspace_bytes(b));
    hipStream_t st = (hipStream_t)stream;
    const TpAug aug{rot, scale, jitter};
    float* stats = (float*)workspace;
    hipLaunchKernelGGL(tp_prepare_kernel, dim3((unsigned)b), dim3(256), 0, st, clouds, n_samples, n, dense, g, normals, sample_idx, aug,
                       cloud_out, dense_out, normals_out, stats);
    SAPCU_CHECK_LAUNCH();
    if (len_out) {
        const int qslabs = (n + 63) / 64;
        hipLaunchKernelGGL(tp_len_kernel, dim3((unsigned)(b * qslabs)), dim3(256), 0, st, dense, n_samples, g, sample_idx, aug,
                           (const float*)cloud_out, n, (const float*)stats, qslabs, len_out);
        SAPCU_CHECK_LAUNCH();
    }
    const unsigned tile_bytes = 3u * (unsigned)n * (unsigned)sizeof(float);       // <= 48 KiB: inside the default dynamic-LDS limit
    if (k > 64)
        hipLaunchKernelGGL(tp_knn_kernel<true>, dim3((unsigned)(b * slabs)), dim3(256), tile_bytes, st, (const float*)cloud_out, n, normals,
                           n_samples, sample_idx, aug, centres, pc, k, slabs, patches_out, idx_out, patch_normals_out);
    else
        hipLaunchKernelGGL(tp_knn_kernel<false>, dim3((unsigned)(b * slabs)), dim3(256), tile_bytes, st, (const float*)cloud_out, n, normals,
                           n_samples, sample_idx, aug, centres, pc, k, slabs, patches_out, idx_out, patch_normals_out);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

}  // extern "C"
