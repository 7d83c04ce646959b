/*
 * sapcu_fd_train.h — the training ops of fd (the distance network): the single-step LIF / EIF neuron with detached carried state,
 * the EdgeConv graph feature, BatchNorm statistics, and BatchNorm-apply + LeakyReLU(0.2) + max over the neighbours in one pass,
 * each with its backward.  sapcu_amd/fd_train.py composes them, with the GEMM / weight-gradient / BatchNorm-backward / kNN entry
 * points of sapcu.h, into the training forward of EnhancedSNNDistanceEstimation (the reference's fd/snn_coder.py:392-492).
 *
 * Part of libsapcu_hip.so; the conventions and status codes of sapcu.h apply (device pointers, the caller owns every buffer, 0 on
 * success, sapcu_last_error() for the text).  SAPCU_ABI_VERSION is unchanged: these entry points are additions.
 *
 * Tensors are dense [rows, channels] f32, channel last, unless a pitch (ldx, ld_grad: floats between rows, >= the width) is named.
 * Every reduction runs in a fixed order and there are no float atomics: the same call gives the same bits every time.
 *
 * The neuron step (fd/snn_coder.py:94-155 LIF, :198-275 EIF, `self.training`).  The encoder detaches the neuron state between time
 * steps (:438-442, :467-471), so a step is a function of x and the raw per-channel parameters with the carried state as constants:
 *     forward:  membrane' = membrane * decay * (1 - refractory) + x * (refractory <= 0) [+ delta_T * exp(clamp((membrane - theta_rh) /
 *               (delta_T + 1e-6), +-5))],  u = membrane' - threshold,  spike = (u > 0), then the reference's state update;
 *     backward: d spike / d u is the soft surrogate's derivative on clamp(u, +-10); threshold_adapt and refractory_decay take no part;
 *               threshold_base is reached only when the carried state is NULL (the step whose threshold IS threshold_base);
 *               a raw parameter outside its clamp, and an exponent argument outside +-5, get zero (torch.clamp).
 *   The refractory gate is evaluated: with hard spikes `refractory` is exactly 0 until a neuron's first spike.
 *   force_spikes (may be NULL): the spike values to use instead of (u > 0) for spikes_out and the new state (teacher forcing of
 *   the parity tests); preact_out (may be NULL) receives u either way.
 *
 * Memory contract (as sapcu.h; checked under guard bands by tests/test_gpu_fd_train.py):
 *   - inputs are only read; each output is written over exactly its extent, nothing else;
 *   - a workspace needs NO initialisation, 8-byte alignment (4 for the neuron step), and at least the bytes its sizer returns for
 *     the same shape — fewer bytes, a NULL required pointer, a carried state given in part, an EIF step without delta_T / theta_rh,
 *     out_channels < 2 * channels, a pitch below the width, or a patch whose inverse table (2 * m * kk + m + 1 ints) exceeds
 *     64 KiB of LDS return SAPCU_ERR_ARG before anything is launched;
 *   - bad_count (device int) is zeroed and then counts the neighbour indices outside [0, m): the forward writes zeros for such
 *     an edge, the backward gives it no gradient.  A step whose count is not 0 must be failed by the caller.
 */
#ifndef SAPCU_FD_TRAIN_H
#define SAPCU_FD_TRAIN_H

#include "sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- single-step neuron.  eif = 0: LIF (delta_T, theta_rh and their gradients may be NULL), 1: EIF.
 * membrane_in / threshold_in / refractory_in: all three [rows, channels], or all NULL = the first step (0, threshold_base, 0). */
int sapcu_fd_neuron_step_forward(const float* x, int64_t rows, int channels, int eif, const float* membrane_decay,
                                 const float* threshold_adapt, const float* refractory_decay, const float* threshold_base,
                                 const float* delta_T, const float* theta_rh, const float* membrane_in, const float* threshold_in,
                                 const float* refractory_in, const float* force_spikes, float* spikes_out, float* membrane_out,
                                 float* threshold_out, float* refractory_out, float* preact_out, void* stream);

/* bytes of workspace of the backward (the per-workgroup partial column sums); -1 for a shape it would refuse */
int64_t sapcu_fd_neuron_step_workspace_bytes(int64_t rows, int channels);

/* grad_x [rows, channels]; grad_membrane_decay, grad_threshold_base (zeros when a carried state is given), grad_delta_T,
 * grad_theta_rh [channels] (the last two EIF only).  Recomputes the forward from x and the carried state. */
int sapcu_fd_neuron_step_backward(const float* x, const float* grad_spikes, int64_t rows, int channels, int eif,
                                  const float* membrane_decay, const float* threshold_base, const float* delta_T, const float* theta_rh,
                                  const float* membrane_in, const float* threshold_in, const float* refractory_in, float* grad_x,
                                  float* grad_membrane_decay, float* grad_threshold_base, float* grad_delta_T, float* grad_theta_rh,
                                  void* workspace, int64_t workspace_bytes, void* stream);

/* ---- EdgeConv graph feature (get_graph_feature, fd/snn_coder.py:52-68).  x [patches * m, ldx], idx int32 [patches, m, kk] in-patch
 * neighbours -> out [patches * m * kk, out_channels]: columns [0, channels) = x[nbr] - x[centre], [channels, 2 channels) = x[nbr]
 * (the neighbour, not the centre), [2 channels, out_channels) = 0 (padding for a GEMM that steps its reduction axis by 32).
 * bad_count may be NULL in the forward. */
int sapcu_fd_edge_feature_forward(const float* x, int ldx, const int32_t* idx, int64_t patches, int m, int kk, int channels,
                                  int out_channels, float* out, int* bad_count, void* stream);

/* grad_x [patches * m, ld_grad] (columns [0, channels) of every row are stored, no zeroing needed): one workgroup per patch, every
 * destination summed over its sources in ascending source order.  bad_count is required. */
int sapcu_fd_edge_feature_backward(const float* grad_out, const int32_t* idx, int64_t patches, int m, int kk, int channels,
                                   int out_channels, float* grad_x, int ld_grad, int* bad_count, void* stream);

/* ---- BatchNorm statistics only (the f64 fixed-order column sums of sapcu_bn_train_forward, no activation written):
 * mean, biased variance, 1 / sqrt(var + eps) per channel of y [rows, channels], rows >= 1. */
int64_t sapcu_fd_bn_stats_workspace_bytes(int64_t rows, int channels);
int sapcu_fd_bn_stats(const float* y, int64_t rows, int channels, float eps, float* mean_out, float* var_out, float* invstd_out,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- out[g, c] = max over the kk rows of group g of LeakyReLU_0.2((y - mean) * invstd * gamma + beta), y [groups * kk, channels];
 * argmax_out int32 [groups, channels] = the FIRST row that attains it (torch.max(dim)); a NaN among the rows is the result (the
 * first one), as torch.max propagates it.  kk = 1: BatchNorm-apply + LeakyReLU. */
int sapcu_fd_bn_lrelu_max_forward(const float* y, int64_t groups, int kk, int channels, const float* mean, const float* invstd,
                                  const float* gamma, const float* beta, float* out, int32_t* argmax_out, void* stream);

/* grad_z [groups * kk, channels], dense: the arg-max row takes grad_out times LeakyReLU's slope, every other row 0 — the grad_z
 * that sapcu_bn_train_backward (sapcu.h) takes. */
int sapcu_fd_bn_lrelu_max_backward(const float* y, const float* grad_out, const int32_t* argmax, int64_t groups, int kk, int channels,
                                   const float* mean, const float* invstd, const float* gamma, const float* beta, float* grad_z,
                                   void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_FD_TRAIN_H */
