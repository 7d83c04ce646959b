// The factored EdgeConv training op of fd's blocks 1-3 (include/sapcu_fd_edgeconv.h).
//
// The convolution over the graph feature [x_n - x_i | x_n] with W = [W1 | W2] is  y[i, j] = s[n(i, j)] - a[i]  with a = x W1^T,
// b = x W2^T, s = a + b (fd_encoder.hip:8 uses the same identity for inference).  a and b come from one point-level GEMM; the
// kernels here gather rows of ab = [a | b] and never write y or any other [patches * m * kk, .] tensor:
//   forward   ec_stats_partial_kernel + ec_final_kernel<0>   f64 column sums of y, y^2 over all edge rows -> mean / var / invstd
//             ec_max_fwd_kernel                              BatchNorm-apply + LeakyReLU + max + first arg-max, y on the fly
//   backward  ec_gz_partial_kernel + ec_final_kernel<1>      gz at the arg-max row of every (point, channel) -> workspace
//                                                            [patches * m, ch], and the column sums  sum gz, sum gz * y_hat
//             ec_bwd_kernel                                  dy = gamma * invstd * (gz - sum gz / R - y_hat * sum gz y_hat / R)
//                                                            reduced straight to grad_s (over a point's incoming edges, from
//                                                            the inverse neighbour table in LDS) and grad_a (over its own).
// All the sources of a destination p share s[p], so  sum y_hat  over them is  invstd * (deg (s[p] - mean) - sum a[source])  and
// sum over a point's own edges is  invstd * (sum s[nbr] - cnt (a[i] + mean)):  the backward gathers rows of a, gz and arg-max,
// it does not evaluate y per edge.  No float atomics: column sums go through per-workgroup f64 partials (fold_groups,
// train_common.h) added in ascending workgroup order, every destination's sources are visited in ascending edge order
// (inverse_table_build, train_common.h).
//
// Tiling: a workgroup owns 64 channels (one lane each, so every gathered row is one coalesced 256-byte read) — s and a of a
// whole patch at block 3 (100 x 512 x 4 B each) stay in L2, LDS holds only the backward's inverse table.
#include "common.h"
#include "ops.h"
#include "train_common.h"
#include "../../include/sapcu_fd_edgeconv.h"

namespace sapcu {

constexpr int EC_STAT_PTS = 16;        // points per workgroup of the statistics pass (each walks its kk neighbours)
constexpr int EC_GZ_PTS = 64;          // points per workgroup of the backward's arg-max pass

// y of edge (pt, neighbour nb) in channel c: s[nb] - a[pt], s = a + b formed in f32; 0 for an index outside the patch
__device__ __forceinline__ float ec_edge_y(const float* __restrict__ patch_ab, int nb, int m, int ch, int c, float a_i) {
    if (nb < 0 || nb >= m) return 0.f;
    const float* row = patch_ab + (int64_t)nb * 2 * ch;
    return __fsub_rn(__fadd_rn(row[c], row[ch + c]), a_i);
}

// grid (ceil(pts / 16), ceil(ch / 64)); thread (g = tid >> 6, lane) walks points g, g + 4, .. of its block in channel lane
__global__ __launch_bounds__(256) void ec_stats_partial_kernel(const float* __restrict__ ab, const int32_t* __restrict__ idx, int64_t pts,
                                                               int m, int kk, int ch, double* __restrict__ partial /*[gridDim.x][2][ch]*/,
                                                               int* __restrict__ bad) {
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const bool live = c < ch;
    double s[2] = {0.0, 0.0};
    for (int q = g; q < EC_STAT_PTS; q += 4) {
        const int64_t pt = (int64_t)blockIdx.x * EC_STAT_PTS + q;
        if (pt >= pts) break;
        const float* pab = ab + (pt / m) * m * 2 * (int64_t)ch;
        const int32_t* ip = idx + pt * kk;
        const float a_i = live ? ab[pt * 2 * ch + c] : 0.f;
        int nbad = 0;
        for (int j = 0; j < kk; ++j) {
            const int nb = ip[j];
            nbad += (nb < 0 || nb >= m) ? 1 : 0;
            const float y = live ? ec_edge_y(pab, nb, m, ch, c, a_i) : 0.f;
            s[0] += (double)y;
            s[1] += (double)y * (double)y;
        }
        if (bad && blockIdx.y == 0 && lane == 0 && nbad) atomicAdd(bad, nbad);
    }
    fold_groups(s);
    if (g == 0 && live) {
        partial[((int64_t)blockIdx.x * 2 + 0) * ch + c] = s[0];
        partial[((int64_t)blockIdx.x * 2 + 1) * ch + c] = s[1];
    }
}

// grid ceil(ch / 64): 64 channels x 4 groups; group g adds partials g, g + 4, .. in ascending order, the groups combine in the order
// 0..3.  MODE 0: mean / var / invstd over `rows` edge rows (the formulas of bn_stats_kernel).  MODE 1: the two sums as f64 for
// ec_bwd_kernel, and grad_beta = sum gz, grad_gamma = sum gz * y_hat.
template <int MODE>
__global__ __launch_bounds__(256) void ec_final_kernel(const double* __restrict__ partial, int64_t nb, int ch, int64_t rows, float eps,
                                                       float* __restrict__ o0, float* __restrict__ o1, float* __restrict__ o2,
                                                       double* __restrict__ sums /*[2][ch]*/) {
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const bool live = c < ch;
    double t[2] = {0.0, 0.0};
    if (live) {
        for (int64_t b = g; b < nb; b += 4) {
            t[0] += partial[(b * 2 + 0) * ch + c];
            t[1] += partial[(b * 2 + 1) * ch + c];
        }
    }
    fold_groups(t);
    if (g != 0 || !live) return;
    if (MODE == 0) {
        const BnStats s = bn_batch_stats(t[0], t[1], rows, eps);  // as sapcu_fd_bn_stats
        o0[c] = (float)s.mu;
        o1[c] = (float)s.var;
        o2[c] = s.invstd;
    } else {
        sums[c] = t[0];
        sums[ch + c] = t[1];
        o0[c] = (float)t[1];                                     // grad_gamma
        o1[c] = (float)t[0];                                     // grad_beta
    }
}

// one thread per (point, channel); the compare of bn_lrelu_max_fwd_kernel: ties go to the FIRST neighbour, a NaN is the result
__global__ __launch_bounds__(256) void ec_max_fwd_kernel(const float* __restrict__ ab, const int32_t* __restrict__ idx, int64_t pts, int m,
                                                         int kk, int ch, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ out, int32_t* __restrict__ arg) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= pts * ch) return;
    const int c = (int)(t % ch);
    const int64_t pt = t / ch;
    const float* pab = ab + (pt / m) * m * 2 * (int64_t)ch;
    const int32_t* ip = idx + pt * kk;
    const float a_i = ab[pt * 2 * ch + c];
    const float mu = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
    float mx = bn_lrelu(ec_edge_y(pab, ip[0], m, ch, c, a_i), mu, is, ga, be);
    int am = 0;
    for (int j = 1; j < kk; ++j) {
        const float v = bn_lrelu(ec_edge_y(pab, ip[j], m, ch, c, a_i), mu, is, ga, be);
        if (v > mx || (v != v && mx == mx)) { mx = v; am = j; }
    }
    out[t] = mx;
    arg[t] = am;
}

// grid (ceil(pts / 64), ceil(ch / 64)); thread (g, lane) walks points g, g + 4, .. of its block: gz of the arg-max row
// (grad_out times LeakyReLU's slope at its z, bn_lrelu_max_bwd_kernel) -> gzv [pts, ch], and the f64 partial sums of gz and
// gz * y_hat (col_partial_kernel<1>'s arithmetic).  Every other row of the dense gz is 0 and adds nothing.
__global__ __launch_bounds__(256) void ec_gz_partial_kernel(const float* __restrict__ ab, const int32_t* __restrict__ idx,
                                                            const float* __restrict__ gout, const int32_t* __restrict__ arg, int64_t pts,
                                                            int m, int kk, int ch, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ gzv,
                                                            double* __restrict__ partial /*[gridDim.x][2][ch]*/) {
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const bool live = c < ch;
    double s[2] = {0.0, 0.0};
    if (live) {
        const float mu = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
        for (int q = g; q < EC_GZ_PTS; q += 4) {
            const int64_t pt = (int64_t)blockIdx.x * EC_GZ_PTS + q;
            if (pt >= pts) break;
            const int ar = arg[pt * ch + c];
            float gz = 0.f, yh = 0.f;
            if (ar >= 0 && ar < kk) {
                const float y = ec_edge_y(ab + (pt / m) * m * 2 * (int64_t)ch, idx[pt * kk + ar], m, ch, c, ab[pt * 2 * ch + c]);
                const float z = bn_z(y, mu, is, ga, be);
                const float go = gout[pt * ch + c];
                gz = z > 0.f ? go : go * 0.2f;
                yh = (y - mu) * is;
            }
            gzv[pt * ch + c] = gz;
            s[0] += (double)gz;
            s[1] += (double)gz * (double)yh;
        }
    }
    fold_groups(s);
    if (g == 0 && live) {
        partial[((int64_t)blockIdx.x * 2 + 0) * ch + c] = s[0];
        partial[((int64_t)blockIdx.x * 2 + 1) * ch + c] = s[1];
    }
}

// grid (patches, ceil(ch / 64)): the inverse neighbour table of the patch in LDS (edge_feature_bwd_kernel's, the list entries
// packed as centre << 16 | rank), then wave w takes points w, w + 4, .. and lane l channel blockIdx.y * 64 + l.
__global__ __launch_bounds__(256) void ec_bwd_kernel(const float* __restrict__ ab, const int32_t* __restrict__ idx,
                                                     const float* __restrict__ gzv, const int32_t* __restrict__ arg, int m, int kk, int ch,
                                                     int64_t rows, const double* __restrict__ sums, const float* __restrict__ mean,
                                                     const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                     float* __restrict__ grad_ab, int* __restrict__ bad) {
    extern __shared__ unsigned char ec_smem[];
    const int gr = m * kk;
    const InverseTable tab(ec_smem, gr);                        // the list entries are the edges, packed
    const int* dst = tab.dst;
    const int* lst = tab.lst;
    const int* off = tab.off;
    const int64_t g = blockIdx.x;
    const int tid = threadIdx.x;
    const int nbad = inverse_table_build(tab, m, gr, [&](int e) { return idx[g * gr + e]; }, [&](int e) { return ((e / kk) << 16) | (e % kk); });
    if (nbad && blockIdx.y == 0) atomicAdd(bad, nbad);
    const int lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.y * 64 + lane;
    if (c >= ch) return;
    const float mu = mean[c], is = invstd[c], k = gamma[c] * is;
    const float m1 = (float)(sums[c] / (double)rows), m2 = (float)(sums[ch + c] / (double)rows);   // as bn_train_bwd_apply_kernel
    const float* pab = ab + g * m * 2 * (int64_t)ch;
    const float* gzb = gzv + g * m * (int64_t)ch;
    const int32_t* argb = arg + g * m * (int64_t)ch;
    float* ob = grad_ab + g * m * 2 * (int64_t)ch;
    for (int p = wave; p < m; p += 4) {
        const float a_p = pab[(int64_t)p * 2 * ch + c];
        const float s_p = __fadd_rn(a_p, pab[(int64_t)p * 2 * ch + ch + c]);
        // grad_s[p]: the edges that point at p, ascending
        float G = 0.f, A = 0.f;
        const int w0 = off[p], w1 = off[p + 1];
        for (int w = w0; w < w1; ++w) {
            const int pk = lst[w];
            const int i = pk >> 16, j = pk & 0xffff;
            A += pab[(int64_t)i * 2 * ch + c];
            G += argb[(int64_t)i * ch + c] == j ? gzb[(int64_t)i * ch + c] : 0.f;
        }
        const float deg = (float)(w1 - w0);
        const float gs = k * (G - deg * m1 - m2 * (is * (deg * (s_p - mu) - A)));
        // grad_a[p] = - sum over p's own valid edges
        float S = 0.f;
        int cnt = 0;
        for (int j = 0; j < kk; ++j) {
            const int d = dst[p * kk + j];
            if (d >= 0) {
                S += __fadd_rn(pab[(int64_t)d * 2 * ch + c], pab[(int64_t)d * 2 * ch + ch + c]);
                ++cnt;
            }
        }
        const int ar = argb[(int64_t)p * ch + c];
        const float gv = (ar >= 0 && ar < kk && dst[p * kk + ar] >= 0) ? gzb[(int64_t)p * ch + c] : 0.f;
        const float n = (float)cnt;
        const float ga = -k * (gv - n * m1 - m2 * (is * (S - n * (a_p + mu))));
        ob[(int64_t)p * 2 * ch + c] = gs + ga;
        ob[(int64_t)p * 2 * ch + ch + c] = gs;
    }
}

struct EcStatsWs {
    double* partial;         // [point blocks][2][ch]
    size_t bytes;
};
static int64_t ec_blocks(int64_t pts, int per) { return (pts + per - 1) / per; }
static EcStatsWs ec_stats_ws_layout(void* base, int64_t pts, int ch) {
    WsCarver c(base, sizeof(double));
    EcStatsWs w;
    w.partial = c.take<double>(ec_blocks(pts, EC_STAT_PTS) * 2 * (int64_t)ch);
    w.bytes = c.bytes();
    return w;
}
struct EcBwdWs {
    double* partial;         // [point blocks][2][ch]
    double* sums;            // [2][ch]
    float* gzv;              // [pts][ch]
    size_t bytes;
};
static EcBwdWs ec_bwd_ws_layout(void* base, int64_t pts, int ch) {
    WsCarver c(base, sizeof(double));
    EcBwdWs w;
    w.partial = c.take<double>(ec_blocks(pts, EC_GZ_PTS) * 2 * (int64_t)ch);
    w.sums = c.take<double>(2 * (int64_t)ch);
    w.gzv = c.take<float>(pts * (int64_t)ch);
    w.bytes = c.bytes();
    return w;
}

// shapes every entry point accepts: the grids fit, the inverse table fits 64 KiB of LDS (so m * kk < 8192 and the packed list
// entries hold), the flat indices fit int64 with room
static bool ec_shape_ok(int64_t patches, int m, int kk, int ch, int64_t min_patches) {
    if (patches < min_patches || m < 1 || kk < 1 || ch < 1 || ch > (1 << 20) || patches >= 0x7fffffffLL) return false;
    if ((int64_t)m * kk > 16384 || inverse_table_bytes(m, (int64_t)m * kk) > 64 * 1024) return false;
    const int64_t pts = patches * m;
    return (pts * ch + 255) / 256 < 0x7fffffffLL && ec_blocks(pts, EC_STAT_PTS) < 0x7fffffffLL;
}

}  // namespace sapcu

using namespace sapcu;

extern "C" {

int64_t sapcu_fd_edgeconv_stats_workspace_bytes(int64_t patches, int m, int kk, int channels) {
    if (!ec_shape_ok(patches, m, kk, channels, 1)) return -1;
    return (int64_t)ec_stats_ws_layout(nullptr, patches * m, channels).bytes;
}

int sapcu_fd_edgeconv_stats(const float* ab, const int32_t* idx, int64_t patches, int m, int kk, int channels, float eps,
                            float* mean_out, float* var_out, float* invstd_out, int* bad_count, void* workspace,
                            int64_t workspace_bytes, void* stream) {
    SAPCU_CHECK_ARG(ab && idx && mean_out && var_out && invstd_out && workspace, "fd_edgeconv_stats: null pointer");
    SAPCU_CHECK_ARG(ec_shape_ok(patches, m, kk, channels, 1),
                    "fd_edgeconv_stats: bad shape (patches >= 1, and a patch of %d points x %d neighbours must fit the backward's LDS)", m, kk);
    SAPCU_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "fd_edgeconv_stats: workspace must be 8-byte aligned");
    const int64_t need = sapcu_fd_edgeconv_stats_workspace_bytes(patches, m, kk, channels);
    if (workspace_bytes < need) {
        set_error("fd_edgeconv_stats: workspace of %lld bytes, need %lld", (long long)workspace_bytes, (long long)need);
        return SAPCU_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t pts = patches * m;
    const EcStatsWs L = ec_stats_ws_layout(workspace, pts, channels);
    const int64_t nb = ec_blocks(pts, EC_STAT_PTS);
    const unsigned tiles = (unsigned)((channels + 63) / 64);
    if (bad_count) { const int zrc = zero_count(bad_count, st); if (zrc != SAPCU_OK) return zrc; }
    hipLaunchKernelGGL(ec_stats_partial_kernel, dim3((unsigned)nb, tiles), dim3(256), 0, st, ab, idx, pts, m, kk, channels, L.partial,
                       bad_count);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(ec_final_kernel<0>, dim3(tiles), dim3(256), 0, st, L.partial, nb, channels, pts * kk, eps, mean_out, var_out,
                       invstd_out, (double*)nullptr);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int sapcu_fd_edgeconv_max_forward(const float* ab, const int32_t* idx, int64_t patches, int m, int kk, int channels, const float* mean,
                                  const float* invstd, const float* gamma, const float* beta, float* out, int32_t* argmax_out,
                                  void* stream) {
    SAPCU_CHECK_ARG(ab && idx && mean && invstd && gamma && beta && out && argmax_out, "fd_edgeconv_max_forward: null pointer");
    SAPCU_CHECK_ARG(ec_shape_ok(patches, m, kk, channels, 0),
                    "fd_edgeconv_max_forward: bad shape (a patch of %d points x %d neighbours must fit the backward's LDS)", m, kk);
    const int64_t pts = patches * m;
    if (pts == 0) return SAPCU_OK;
    hipLaunchKernelGGL(ec_max_fwd_kernel, dim3((unsigned)((pts * channels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ab, idx, pts, m,
                       kk, channels, mean, invstd, gamma, beta, out, argmax_out);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int64_t sapcu_fd_edgeconv_backward_workspace_bytes(int64_t patches, int m, int kk, int channels) {
    if (!ec_shape_ok(patches, m, kk, channels, 1)) return -1;
    return (int64_t)ec_bwd_ws_layout(nullptr, patches * m, channels).bytes;
}

int sapcu_fd_edgeconv_backward(const float* ab, const int32_t* idx, const float* grad_out, const int32_t* argmax, int64_t patches, int m,
                               int kk, int channels, const float* mean, const float* invstd, const float* gamma, const float* beta,
                               float* grad_ab, float* grad_gamma, float* grad_beta, int* bad_count, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    SAPCU_CHECK_ARG(ab && idx && grad_out && argmax && mean && invstd && gamma && beta && grad_ab && grad_gamma && grad_beta && bad_count &&
                        workspace, "fd_edgeconv_backward: null pointer (bad_count is required)");
    SAPCU_CHECK_ARG(ec_shape_ok(patches, m, kk, channels, 1),
                    "fd_edgeconv_backward: bad shape (patches >= 1, and a patch of %d points x %d neighbours must fit 64 KiB of LDS)", m, kk);
    SAPCU_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "fd_edgeconv_backward: workspace must be 8-byte aligned");
    const int64_t need = sapcu_fd_edgeconv_backward_workspace_bytes(patches, m, kk, channels);
    if (workspace_bytes < need) {
        set_error("fd_edgeconv_backward: workspace of %lld bytes, need %lld", (long long)workspace_bytes, (long long)need);
        return SAPCU_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t pts = patches * m;
    const EcBwdWs L = ec_bwd_ws_layout(workspace, pts, channels);
    const int64_t nb = ec_blocks(pts, EC_GZ_PTS);
    const unsigned tiles = (unsigned)((channels + 63) / 64);
    { const int zrc = zero_count(bad_count, st); if (zrc != SAPCU_OK) return zrc; }
    hipLaunchKernelGGL(ec_gz_partial_kernel, dim3((unsigned)nb, tiles), dim3(256), 0, st, ab, idx, grad_out, argmax, pts, m, kk, channels,
                       mean, invstd, gamma, beta, L.gzv, L.partial);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(ec_final_kernel<1>, dim3(tiles), dim3(256), 0, st, L.partial, nb, channels, pts * kk, 0.f, grad_gamma, grad_beta,
                       (float*)nullptr, L.sums);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(ec_bwd_kernel, dim3((unsigned)patches, tiles), dim3(256), inverse_table_bytes(m, (int64_t)m * kk), st, ab, idx, L.gzv, argmax,
                       m, kk, channels, pts * kk, L.sums, mean, invstd, gamma, grad_ab, bad_count);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

}  // extern "C"
