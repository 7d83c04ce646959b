// Training ops of fd (include/sapcu_fd_train.h): the single-step LIF / EIF neuron with detached carried state, the EdgeConv graph
// feature, and BatchNorm-apply + LeakyReLU(0.2) + max over the neighbours in one pass — forward and backward.
//
// /root/reference/fd/snn_coder.py in `self.training` mode.  The encoder detaches its neuron state between time steps
// (:438-442, :467-471), so every step is ONE neuron step whose carried state (membrane, threshold, refractory) is a constant of
// the gradient: unlike fn's T-step self-loop (train_ops.hip) nothing flows backwards through the state, threshold_adapt and
// refractory_decay take no part in any derivative, and threshold_base is reached only through the step that starts from it.
// The refractory gate is live: with hard spikes `refractory` is exactly 0 until a neuron's first spike.
//
// No float atomics: column sums go through per-workgroup partials (fold_groups, train_common.h) added in ascending workgroup order,
// the EdgeConv backward sums every destination's sources in ascending source order (inverse_table_build, train_common.h).  All
// tensors are dense [rows, channels] f32, channel last, except where a pitch is named.
#include "common.h"
#include "ops.h"
#include "train_common.h"
#include "../../include/sapcu_fd_train.h"

namespace sapcu {

constexpr int NS_ROWS_PER_WG = 64;     // 4 row slabs of 16 rows x 64 channels per 256-thread workgroup
constexpr int NS_Q = 4;                // parameter gradients per channel: membrane_decay, threshold_base, delta_T, theta_rh

struct StepP {                         // clamped parameters (train_common.h; the clamp masks are applied by neuron_step_reduce_kernel)
    float decay, adapt, rdecay, theta0, dT, rh;
};

__device__ __forceinline__ StepP load_step_params(const float* md, const float* ta, const float* rd, const float* tb, const float* dT,
                                                  const float* rh, bool eif, int c) {
    StepP p;
    p.decay = clamp_membrane_decay(md[c]).v;
    p.adapt = ta ? clamp_threshold_adapt(ta[c]).v : 0.f;
    p.rdecay = rd ? clamp_refractory_decay(rd[c]).v : 0.f;
    p.theta0 = tb[c];
    p.dT = eif ? clamp_delta_T(dT[c]).v : 0.f;
    p.rh = eif ? clamp_theta_rh(rh[c]).v : 0.f;
    return p;
}

struct StepV {                         // what one step computes before the spike
    float gate, arg, e, mm, u;         // (r <= 0), the clamped exponent argument and exp of it (EIF), integrated membrane, mm - th
    bool arg_in;
};

// fd/snn_coder.py:133-135 (LIF) and :245-255 (EIF), every operator rounded on its own in the reference's order
template <bool EIF>
__device__ __forceinline__ StepV step_integrate(float x, float m, float th, float r, const StepP& p) {
    StepV v;
    v.arg = 0.f; v.e = 0.f; v.arg_in = false;
    float ex = 0.f;
    if (EIF) {
        const float raw = __fdiv_rn(__fsub_rn(m, p.rh), __fadd_rn(p.dT, 1e-6f));
        v.arg_in = raw >= -5.0f && raw <= 5.0f;
        v.arg = fminf(fmaxf(raw, -5.0f), 5.0f);
        v.e = expf(v.arg);
        ex = __fmul_rn(p.dT, v.e);
    }
    v.gate = r <= 0.f ? 1.f : 0.f;
    v.mm = __fadd_rn(__fmul_rn(__fmul_rn(m, p.decay), __fsub_rn(1.0f, r)), __fmul_rn(x, v.gate));
    if (EIF) v.mm = __fadd_rn(v.mm, ex);
    v.u = __fsub_rn(v.mm, th);
    return v;
}

template <bool EIF>
__global__ __launch_bounds__(256) void neuron_step_fwd_kernel(const float* __restrict__ x, int64_t rows, int ch, const float* md,
                                                              const float* ta, const float* rd, const float* tb, const float* dT,
                                                              const float* rh, const float* __restrict__ m_in,
                                                              const float* __restrict__ th_in, const float* __restrict__ r_in,
                                                              const float* __restrict__ force, float* __restrict__ spikes,
                                                              float* __restrict__ m_out, float* __restrict__ th_out,
                                                              float* __restrict__ r_out, float* __restrict__ pre_out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * ch) return;
    const StepP p = load_step_params(md, ta, rd, tb, dT, rh, EIF, (int)(t % ch));
    const float m = m_in ? m_in[t] : 0.f, th = th_in ? th_in[t] : p.theta0, r = r_in ? r_in[t] : 0.f;
    const StepV v = step_integrate<EIF>(x[t], m, th, r, p);
    const float sp = force ? force[t] : (v.u > 0.f ? 1.f : 0.f);
    spikes[t] = sp;
    m_out[t] = __fmul_rn(v.mm, __fsub_rn(1.0f, sp));
    r_out[t] = __fadd_rn(__fmul_rn(r, p.rdecay), sp);
    const float th1 = __fadd_rn(th, __fmul_rn(p.adapt, sp));
    th_out[t] = __fadd_rn(p.theta0, __fmul_rn(__fsub_rn(th1, p.theta0), 0.95f));
    if (pre_out) pre_out[t] = v.u;
}

// grid: (ceil(rows / 64), ceil(ch / 64)); thread (slab = tid >> 6, lane = tid & 63) walks rows slab*16 .. +16 of its column.
// The forward is recomputed; the spike's own value takes no part (the state it feeds is detached).
template <bool EIF>
__global__ __launch_bounds__(256) void neuron_step_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gout, int64_t rows,
                                                              int ch, const float* md, const float* tb, const float* dT, const float* rh,
                                                              const float* __restrict__ m_in, const float* __restrict__ th_in,
                                                              const float* __restrict__ r_in, float* __restrict__ gx,
                                                              float* __restrict__ partial /*[gridDim.x][NS_Q][ch]*/) {
    const int lane = threadIdx.x & 63, slab = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const bool live = c < ch;
    float g[NS_Q] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const StepP p = load_step_params(md, nullptr, nullptr, tb, dT, rh, EIF, c);
        const int64_t row0 = (int64_t)blockIdx.x * NS_ROWS_PER_WG + slab * 16;
        for (int i = 0; i < 16; ++i) {
            const int64_t row = row0 + i;
            if (row >= rows) break;
            const int64_t t = row * ch + c;
            const float m = m_in ? m_in[t] : 0.f, th = th_in ? th_in[t] : p.theta0, r = r_in ? r_in[t] : 0.f;
            const StepV v = step_integrate<EIF>(x[t], m, th, r, p);
            const float a_u = gout[t] * surrogate_grad(v.u);      // u = mm - th: d mm = a_u, d th = -a_u
            gx[t] = a_u * v.gate;
            g[0] += a_u * m * (1.0f - r);                              // mm = m*decay*(1-r) + ...
            if (!th_in) g[1] -= a_u;                                   // the threshold IS threshold_base on the first step only
            if (EIF) {                                                 // ex = dT * exp(clamp((m - rh) / (dT + 1e-6), +-5))
                const float den = __fadd_rn(p.dT, 1e-6f);
                const float a_arg = v.arg_in ? a_u * p.dT * v.e : 0.f;
                g[2] += a_u * v.e - a_arg * (m - p.rh) / (den * den);
                g[3] -= a_arg / den;
            }
        }
    }
    fold_groups(g);
    if (slab == 0 && live) {
#pragma unroll
        for (int q = 0; q < NS_Q; ++q) partial[((int64_t)blockIdx.x * NS_Q + q) * ch + c] = g[q];
    }
}

// one thread per channel adds the workgroups' partials in ascending order and applies the clamp masks of the raw parameters
__global__ __launch_bounds__(256) void neuron_step_reduce_kernel(const float* __restrict__ partial, int64_t nblocks, int ch, int eif,
                                                                 const float* md, const float* dT, const float* rh,
                                                                 float* __restrict__ g_md, float* __restrict__ g_tb,
                                                                 float* __restrict__ g_dT, float* __restrict__ g_rh) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ch) return;
    float s[NS_Q] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t b = 0; b < nblocks; ++b)
#pragma unroll
        for (int q = 0; q < NS_Q; ++q) s[q] += partial[(b * NS_Q + q) * ch + c];
    g_md[c] = clamp_membrane_decay(md[c]).in ? s[0] : 0.f;
    g_tb[c] = s[1];
    if (eif) {
        g_dT[c] = clamp_delta_T(dT[c]).in ? s[2] : 0.f;
        g_rh[c] = clamp_theta_rh(rh[c]).in ? s[3] : 0.f;
    }
}

struct NeuronStepWs {
    float* partial;          // [row blocks][NS_Q][ch]
    size_t bytes;
};
static int64_t ns_blocks(int64_t rows) { return (rows + NS_ROWS_PER_WG - 1) / NS_ROWS_PER_WG; }
static NeuronStepWs neuron_step_ws_layout(void* base, int64_t rows, int ch) {
    WsCarver c(base, sizeof(float));
    NeuronStepWs w;
    const int64_t nb = ns_blocks(rows);
    w.partial = c.take<float>((nb > 0 ? nb : 1) * NS_Q * (int64_t)ch);
    w.bytes = c.bytes();
    return w;
}

// ---- EdgeConv graph feature (get_graph_feature, fd/snn_coder.py:52-68): out[(p,i,j), :] = [x[nbr] - x[i] | x[nbr] | 0 ...]
// one thread per (edge row, output column); an index outside its patch writes zeros and is counted
__global__ __launch_bounds__(256) void edge_feature_fwd_kernel(const float* __restrict__ x, int ldx, const int32_t* __restrict__ idx,
                                                               int64_t edges, int m, int kk, int c, int oc, float* __restrict__ out,
                                                               int* __restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= edges * oc) return;
    const int64_t e = t / oc;
    const int col = (int)(t - e * oc);
    const int64_t pt = e / kk;
    const int64_t patch = pt / m;
    const int nb = idx[e];
    const bool ok = nb >= 0 && nb < m;
    if (!ok && col == 0 && bad) atomicAdd(bad, 1);
    float v = 0.f;
    if (ok && col < 2 * c) {
        const int cc = col < c ? col : col - c;
        const float xn = x[(patch * m + nb) * ldx + cc];
        v = col < c ? __fsub_rn(xn, x[pt * ldx + cc]) : xn;
    }
    out[t] = v;
}

// one workgroup per patch: the inverse neighbour table (train_common.h: destination t's edges in ascending edge order), then every
// (point, channel) is summed by one thread — first minus its own kk edges' difference halves, then its listed edges — and STORED.
__global__ __launch_bounds__(256) void edge_feature_bwd_kernel(const float* __restrict__ gout, const int32_t* __restrict__ idx, int m,
                                                               int kk, int c, int oc, float* __restrict__ gx, int ldg,
                                                               int* __restrict__ bad) {
    extern __shared__ unsigned char ef_smem[];
    const int gr = m * kk;
    const InverseTable tab(ef_smem, gr);                        // the list entries are the edges
    const int* dst = tab.dst;
    const int* lst = tab.lst;
    const int* off = tab.off;
    const int64_t g = blockIdx.x;
    const int tid = threadIdx.x;
    const int nbad = inverse_table_build(tab, m, gr, [&](int e) { return idx[g * gr + e]; }, [](int e) { return e; });
    if (nbad) atomicAdd(bad, nbad);
    const float* gb = gout + g * gr * (int64_t)oc;
    float* ob = gx + g * m * (int64_t)ldg;
    for (int64_t q = tid; q < (int64_t)m * c; q += 256) {
        const int t = (int)(q / c), cc = (int)(q - (int64_t)t * c);
        float s = 0.f;
        for (int j = 0; j < kk; ++j)
            if (dst[t * kk + j] >= 0) s = __fsub_rn(s, gb[(int64_t)(t * kk + j) * oc + cc]);
        for (int w = off[t]; w < off[t + 1]; ++w) {
            const float* ge = gb + (int64_t)lst[w] * oc;
            s = __fadd_rn(s, __fadd_rn(ge[cc], ge[c + cc]));
        }
        ob[(int64_t)t * ldg + cc] = s;
    }
}

// ---- BatchNorm statistics of a [rows, ch] tensor from the f64 fixed-order column sums of train_ops.hip
__global__ __launch_bounds__(256) void bn_stats_kernel(const double* __restrict__ sums, int64_t rows, int ch, float eps,
                                                       float* __restrict__ mean_out, float* __restrict__ var_out,
                                                       float* __restrict__ invstd_out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ch) return;
    const BnStats s = bn_batch_stats(sums[c], sums[ch + c], rows, eps);      // as sapcu_bn_train_forward
    mean_out[c] = (float)s.mu;
    var_out[c] = (float)s.var;
    invstd_out[c] = s.invstd;
}

// one thread per (group, channel): max over the kk rows of the group of LeakyReLU(BN(y)); ties go to the FIRST row, and a NaN among
// the rows is the result (the first one), as torch.max(dim) propagates it
__global__ __launch_bounds__(256) void bn_lrelu_max_fwd_kernel(const float* __restrict__ y, int64_t groups, int kk, int ch,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* __restrict__ out, int32_t* __restrict__ arg) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= groups * ch) return;
    const int c = (int)(t % ch);
    const int64_t g = t / ch;
    const float mu = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
    const float* p = y + g * kk * ch + c;
    float mx = bn_lrelu(p[0], mu, is, ga, be);
    int am = 0;
    for (int j = 1; j < kk; ++j) {
        const float v = bn_lrelu(p[(int64_t)j * ch], mu, is, ga, be);
        if (v > mx || (v != v && mx == mx)) { mx = v; am = j; }
    }
    out[t] = mx;
    arg[t] = am;
}

// dense grad_z [groups*kk, ch]: the arg-max row takes grad_out times LeakyReLU's slope at its z, every other row 0
__global__ __launch_bounds__(256) void bn_lrelu_max_bwd_kernel(const float* __restrict__ y, const float* __restrict__ gout,
                                                               const int32_t* __restrict__ arg, int64_t groups, int kk, int ch,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* __restrict__ gz) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= groups * kk * ch) return;
    const int c = (int)(t % ch);
    const int64_t row = t / ch;
    const int64_t g = row / kk;
    const int j = (int)(row - g * kk);
    float v = 0.f;
    if (arg[g * ch + c] == j) {
        const float z = bn_z(y[t], mean[c], invstd[c], gamma[c], beta[c]);
        v = z > 0.f ? gout[g * ch + c] : gout[g * ch + c] * 0.2f;
    }
    gz[t] = v;
}

}  // namespace sapcu

using namespace sapcu;

extern "C" {

int64_t sapcu_fd_neuron_step_workspace_bytes(int64_t rows, int channels) {
    if (rows < 0 || channels < 1 || ns_blocks(rows) >= 0x7fffffffLL) return -1;
    return (int64_t)neuron_step_ws_layout(nullptr, rows, channels).bytes;
}

int sapcu_fd_neuron_step_forward(const float* x, int64_t rows, int channels, int eif, const float* membrane_decay,
                                 const float* threshold_adapt, const float* refractory_decay, const float* threshold_base,
                                 const float* delta_T, const float* theta_rh, const float* membrane_in, const float* threshold_in,
                                 const float* refractory_in, const float* force_spikes, float* spikes_out, float* membrane_out,
                                 float* threshold_out, float* refractory_out, float* preact_out, void* stream) {
    SAPCU_CHECK_ARG(x && membrane_decay && threshold_adapt && refractory_decay && threshold_base && spikes_out && membrane_out &&
                        threshold_out && refractory_out, "fd_neuron_step_forward: null pointer");
    SAPCU_CHECK_ARG(!eif || (delta_T && theta_rh), "fd_neuron_step_forward: an EIF step needs delta_T and theta_rh");
    SAPCU_CHECK_ARG((membrane_in != nullptr) == (threshold_in != nullptr) && (membrane_in != nullptr) == (refractory_in != nullptr),
                    "fd_neuron_step_forward: the carried state is three tensors or none");
    SAPCU_CHECK_ARG(rows >= 0 && channels >= 1 && (rows * channels + 255) / 256 < 0x7fffffffLL, "fd_neuron_step_forward: bad shape");
    const int64_t total = rows * channels;
    if (total == 0) return SAPCU_OK;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (eif)
        hipLaunchKernelGGL(neuron_step_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, rows, channels, membrane_decay,
                           threshold_adapt, refractory_decay, threshold_base, delta_T, theta_rh, membrane_in, threshold_in, refractory_in,
                           force_spikes, spikes_out, membrane_out, threshold_out, refractory_out, preact_out);
    else
        hipLaunchKernelGGL(neuron_step_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, rows, channels, membrane_decay,
                           threshold_adapt, refractory_decay, threshold_base, delta_T, theta_rh, membrane_in, threshold_in, refractory_in,
                           force_spikes, spikes_out, membrane_out, threshold_out, refractory_out, preact_out);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int sapcu_fd_neuron_step_backward(const float* x, const float* grad_spikes, int64_t rows, int channels, int eif,
                                  const float* membrane_decay, const float* threshold_base, const float* delta_T, const float* theta_rh,
                                  const float* membrane_in, const float* threshold_in, const float* refractory_in, float* grad_x,
                                  float* grad_membrane_decay, float* grad_threshold_base, float* grad_delta_T, float* grad_theta_rh,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    SAPCU_CHECK_ARG(x && grad_spikes && membrane_decay && threshold_base && grad_x && grad_membrane_decay && grad_threshold_base &&
                        workspace, "fd_neuron_step_backward: null pointer");
    SAPCU_CHECK_ARG(!eif || (delta_T && theta_rh && grad_delta_T && grad_theta_rh),
                    "fd_neuron_step_backward: an EIF step needs delta_T, theta_rh and their gradient buffers");
    SAPCU_CHECK_ARG((membrane_in != nullptr) == (threshold_in != nullptr) && (membrane_in != nullptr) == (refractory_in != nullptr),
                    "fd_neuron_step_backward: the carried state is three tensors or none");
    SAPCU_CHECK_ARG(rows >= 0 && channels >= 1 && ns_blocks(rows) < 0x7fffffffLL, "fd_neuron_step_backward: bad shape");
    SAPCU_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "fd_neuron_step_backward: workspace must be 4-byte aligned");
    SAPCU_CHECK_ARG(workspace_bytes >= sapcu_fd_neuron_step_workspace_bytes(rows, channels),
                    "fd_neuron_step_backward: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
                    (long long)sapcu_fd_neuron_step_workspace_bytes(rows, channels));
    hipStream_t st = (hipStream_t)stream;
    const NeuronStepWs L = neuron_step_ws_layout(workspace, rows, channels);
    const int64_t nb = ns_blocks(rows);
    if (nb > 0) {
        const dim3 grid((unsigned)nb, (unsigned)((channels + 63) / 64));
        if (eif)
            hipLaunchKernelGGL(neuron_step_bwd_kernel<true>, grid, dim3(256), 0, st, x, grad_spikes, rows, channels, membrane_decay,
                               threshold_base, delta_T, theta_rh, membrane_in, threshold_in, refractory_in, grad_x, L.partial);
        else
            hipLaunchKernelGGL(neuron_step_bwd_kernel<false>, grid, dim3(256), 0, st, x, grad_spikes, rows, channels, membrane_decay,
                               threshold_base, delta_T, theta_rh, membrane_in, threshold_in, refractory_in, grad_x, L.partial);
        SAPCU_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(neuron_step_reduce_kernel, dim3((unsigned)((channels + 255) / 256)), dim3(256), 0, st, L.partial, nb, channels,
                       eif ? 1 : 0, membrane_decay, delta_T, theta_rh, grad_membrane_decay, grad_threshold_base, grad_delta_T,
                       grad_theta_rh);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

static int edge_feature_args_ok(int64_t patches, int m, int kk, int c, int oc) {
    return patches >= 0 && m >= 1 && kk >= 1 && c >= 1 && oc >= 2 * c && patches < 0x7fffffffLL &&
           ((patches * m * kk * oc + 255) / 256) < 0x7fffffffLL;
}

int sapcu_fd_edge_feature_forward(const float* x, int ldx, const int32_t* idx, int64_t patches, int m, int kk, int channels,
                                  int out_channels, float* out, int* bad_count, void* stream) {
    SAPCU_CHECK_ARG(x && idx && out, "fd_edge_feature_forward: null pointer");
    SAPCU_CHECK_ARG(edge_feature_args_ok(patches, m, kk, channels, out_channels) && ldx >= channels,
                    "fd_edge_feature_forward: bad shape (need out_channels >= 2 channels, ldx >= channels)");
    if (bad_count) { const int zrc = zero_count(bad_count, (hipStream_t)stream); if (zrc != SAPCU_OK) return zrc; }
    const int64_t edges = patches * m * kk;
    if (edges == 0) return SAPCU_OK;
    hipLaunchKernelGGL(edge_feature_fwd_kernel, dim3((unsigned)((edges * out_channels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                       ldx, idx, edges, m, kk, channels, out_channels, out, bad_count);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int sapcu_fd_edge_feature_backward(const float* grad_out, const int32_t* idx, int64_t patches, int m, int kk, int channels,
                                   int out_channels, float* grad_x, int ld_grad, int* bad_count, void* stream) {
    SAPCU_CHECK_ARG(grad_out && idx && grad_x && bad_count, "fd_edge_feature_backward: null pointer (bad_count is required)");
    SAPCU_CHECK_ARG(edge_feature_args_ok(patches, m, kk, channels, out_channels) && ld_grad >= channels,
                    "fd_edge_feature_backward: bad shape (need out_channels >= 2 channels, ld_grad >= channels)");
    const size_t lds = inverse_table_bytes(m, (int64_t)m * kk);
    SAPCU_CHECK_ARG(lds <= 64 * 1024, "fd_edge_feature_backward: patch too large (%d points x %d neighbours)", m, kk);
    { const int zrc = zero_count(bad_count, (hipStream_t)stream); if (zrc != SAPCU_OK) return zrc; }
    if (patches == 0) return SAPCU_OK;
    hipLaunchKernelGGL(edge_feature_bwd_kernel, dim3((unsigned)patches), dim3(256), lds, (hipStream_t)stream, grad_out, idx, m, kk,
                       channels, out_channels, grad_x, ld_grad, bad_count);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int64_t sapcu_fd_bn_stats_workspace_bytes(int64_t rows, int channels) {
    if (rows < 1 || channels < 1) return -1;
    return train_column_sums_bytes(rows, channels);
}

int sapcu_fd_bn_stats(const float* y, int64_t rows, int channels, float eps, float* mean_out, float* var_out, float* invstd_out,
                      void* workspace, int64_t workspace_bytes, void* stream) {
    SAPCU_CHECK_ARG(y && mean_out && var_out && invstd_out && workspace && rows >= 1 && channels >= 1, "fd_bn_stats: bad argument");
    SAPCU_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "fd_bn_stats: workspace must be 8-byte aligned");
    SAPCU_CHECK_ARG(workspace_bytes >= sapcu_fd_bn_stats_workspace_bytes(rows, channels), "fd_bn_stats: workspace of %lld bytes, need %lld",
                    (long long)workspace_bytes, (long long)sapcu_fd_bn_stats_workspace_bytes(rows, channels));
    double* sums = nullptr;
    const int rc = column_sums(0, y, nullptr, rows, channels, nullptr, nullptr, workspace, &sums, (hipStream_t)stream);
    if (rc != SAPCU_OK) return rc;
    hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)((channels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sums, rows, channels,
                       eps, mean_out, var_out, invstd_out);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int sapcu_fd_bn_lrelu_max_forward(const float* y, int64_t groups, int kk, int channels, const float* mean, const float* invstd,
                                  const float* gamma, const float* beta, float* out, int32_t* argmax_out, void* stream) {
    SAPCU_CHECK_ARG(y && mean && invstd && gamma && beta && out && argmax_out, "fd_bn_lrelu_max_forward: null pointer");
    SAPCU_CHECK_ARG(groups >= 0 && kk >= 1 && channels >= 1 && (groups * channels + 255) / 256 < 0x7fffffffLL,
                    "fd_bn_lrelu_max_forward: bad shape");
    if (groups == 0) return SAPCU_OK;
    hipLaunchKernelGGL(bn_lrelu_max_fwd_kernel, dim3((unsigned)((groups * channels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y,
                       groups, kk, channels, mean, invstd, gamma, beta, out, argmax_out);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int sapcu_fd_bn_lrelu_max_backward(const float* y, const float* grad_out, const int32_t* argmax, int64_t groups, int kk, int channels,
                                   const float* mean, const float* invstd, const float* gamma, const float* beta, float* grad_z,
                                   void* stream) {
    SAPCU_CHECK_ARG(y && grad_out && argmax && mean && invstd && gamma && beta && grad_z, "fd_bn_lrelu_max_backward: null pointer");
    SAPCU_CHECK_ARG(groups >= 0 && kk >= 1 && channels >= 1 && (groups * kk * channels + 255) / 256 < 0x7fffffffLL,
                    "fd_bn_lrelu_max_backward: bad shape");
    if (groups == 0) return SAPCU_OK;
    hipLaunchKernelGGL(bn_lrelu_max_bwd_kernel, dim3((unsigned)((groups * kk * channels + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       y, grad_out, argmax, groups, kk, channels, mean, invstd, gamma, beta, grad_z);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

}  // extern "C"
