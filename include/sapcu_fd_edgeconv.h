/*
 * sapcu_fd_edgeconv.h — the FACTORED EdgeConv training op of fd's blocks 1-3: convolution over the graph feature [x_n - x_i | x_n]
 * -> BatchNorm (batch statistics) -> LeakyReLU(0.2) -> max over the kk neighbours, without the [patches * m * kk, .] edge tensors.
 *
 * With W = [W1 | W2] the convolution of an edge (centre i, neighbour n) is  y = W1 (x_n - x_i) + W2 x_n = s[n] - a[i],  where
 * a = x W1^T and b = x W2^T come out of ONE point-level GEMM of x against the stacked [W1 ; W2] and s = a + b is formed in f32.
 * The entry points below take that GEMM's output  ab [patches * m, 2 * channels] = [a | b]  and the neighbour table and never
 * write y: the statistics, the max and the whole BatchNorm backward are evaluated from gathered rows of ab.  The backward returns
 * grad_ab = [grad_s + grad_a | grad_s], the gradient of the stacked GEMM's output; dW and dx are then one point-level weight
 * gradient and one point-level GEMM (sapcu.h).  sapcu_amd/fd_train.py (edgeconv_factored) composes them.
 *
 * Part of libsapcu_hip.so; the conventions and status codes of sapcu.h apply.  SAPCU_ABI_VERSION is unchanged: these entry points
 * are additions.  The per-element arithmetic after y is that of sapcu_fd_bn_stats / sapcu_fd_bn_lrelu_max_forward
 * (sapcu_fd_train.h), the BatchNorm backward that of sapcu_bn_train_backward over all patches * m * kk edge rows.  Every reduction
 * runs in a fixed order and there are no float atomics: the same call gives the same bits every time.
 *
 * Memory contract:
 *   - inputs are only read; each output is written over exactly its extent (grad_ab: all 2 * channels columns of every row);
 *   - a workspace needs NO initialisation and 8-byte alignment; a NULL required pointer, a misaligned workspace, channels < 1,
 *     m < 1, kk < 1, patches < 0 or a patch whose inverse table (2 * m * kk + m + 1 ints) exceeds 64 KiB of LDS return
 *     SAPCU_ERR_ARG, fewer workspace bytes than the sizer returns for the same shape SAPCU_ERR_WORKSPACE, both before anything is
 *     launched; the sizers return -1 for a shape the calls refuse;
 *   - an index outside [0, m): that edge's y is 0 (as with a zero feature row — it still counts in the statistics), it gets no
 *     gradient, and bad_count (device int, zeroed by the call) counts it.  bad_count may be NULL in sapcu_fd_edgeconv_stats and is
 *     required in the backward.  An argmax entry outside [0, kk) selects no row.
 */
#ifndef SAPCU_FD_EDGECONV_H
#define SAPCU_FD_EDGECONV_H

#include "sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batch statistics of y over all patches * m * kk edge rows (f64 sums in a fixed order; the final formulas of
 * sapcu_fd_bn_stats): mean, biased variance, 1 / sqrt(var + eps) per channel.  patches >= 1. */
int64_t sapcu_fd_edgeconv_stats_workspace_bytes(int64_t patches, int m, int kk, int channels);
int sapcu_fd_edgeconv_stats(const float* ab, const int32_t* idx, int64_t patches, int m, int kk, int channels, float eps,
                            float* mean_out, float* var_out, float* invstd_out, int* bad_count, void* workspace,
                            int64_t workspace_bytes, void* stream);

/* ---- out[i, c] = max over the kk neighbours of LeakyReLU_0.2((y - mean) * invstd * gamma + beta), out [patches * m, channels];
 * argmax_out int32 = the FIRST neighbour rank that attains it; a NaN among the kk values is the result (torch.max(dim)). */
int sapcu_fd_edgeconv_max_forward(const float* ab, const int32_t* idx, int64_t patches, int m, int kk, int channels, const float* mean,
                                  const float* invstd, const float* gamma, const float* beta, float* out, int32_t* argmax_out,
                                  void* stream);

/* ---- the backward of max, LeakyReLU, BatchNorm and the gather in one: grad_out [patches * m, channels] ->
 * grad_ab [patches * m, 2 * channels] = [grad_s + grad_a | grad_s] with grad_s[p] = sum of dy over the edges whose neighbour is p
 * (ascending edge order, one workgroup per patch and column tile) and grad_a[i] = - sum_j dy[i, j]; grad_gamma, grad_beta
 * [channels].  patches >= 1. */
int64_t sapcu_fd_edgeconv_backward_workspace_bytes(int64_t patches, int m, int kk, int channels);
int sapcu_fd_edgeconv_backward(const float* ab, const int32_t* idx, const float* grad_out, const int32_t* argmax, int64_t patches, int m,
                               int kk, int channels, const float* mean, const float* invstd, const float* gamma, const float* beta,
                               float* grad_ab, float* grad_gamma, float* grad_beta, int* bad_count, void* workspace,
                               int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_FD_EDGECONV_H */
