// What the training translation units share (train_ops.hip: fn's ops; fd_train_ops.hip, fd_edgeconv_ops.hip: fd's; train_bf16.hip:
// the bf16 GEMMs): the four-group column fold, the per-group inverse neighbour table in LDS with its byte count, the surrogate
// derivative, the clamp range of every raw neuron parameter, the batch statistics, BatchNorm-apply + LeakyReLU, and the launcher of
// the slab sum that lives in train_bf16.hip (a kernel is launched from the file that defines it).  Device functions are
// __device__ __forceinline__, host helpers static inline.
#pragma once
#include "common.h"

namespace sapcu {

// ---- the 4 row-lanes x 64 channels fold.  A 256-thread workgroup is 64 channels (lane = tid & 63) x 4 groups (g = tid >> 6), every
// thread holds Q running sums of its channel: group 0's v[] becomes ((g0 + g1) + g2) + g3 of each, the other groups' v[] stay.
// Every thread of the workgroup calls it (it synchronises); what is done with the sums stays in the kernel.
// (colsum_kernel in train_bf16.hip adds (p0 + p1) + (p2 + p3): a different sum, not this one.)
template <int Q, typename T>
__device__ __forceinline__ void fold_groups(T (&v)[Q]) {
    __shared__ T red[4][Q][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < Q; ++q) red[g][q][lane] = v[q];
    __syncthreads();
    if (g != 0) return;
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = ((red[0][q][lane] + red[1][q][lane]) + red[2][q][lane]) + red[3][q][lane];
}

// ---- the inverse table of a group: gr index entries (a patch's m kk edge rows) point into gs destinations (its m points); the
// table lists, per destination, its entries in ascending entry order, so that one thread can sum a destination's sources in a fixed
// order and STORE the sum — no float atomics.  It lives in the caller's dynamic LDS, inverse_table_bytes(gs, gr) of it.
static inline size_t inverse_table_bytes(int64_t gs, int64_t gr) { return ((size_t)2 * gr + gs + 1) * sizeof(int); }

struct InverseTable {
    int* dst;        // [gr] local destination of each entry (-1: outside [0, gs))
    int* lst;        // [gr] what entry_of gave for the entries, ordered by (destination, entry)
    int* off;        // [gs + 1] start of each destination's list
    __device__ __forceinline__ InverseTable(void* lds, int gr) : dst(reinterpret_cast<int*>(lds)), lst(dst + gr), off(lst + gr) {}
};

// dst_of(e): the local destination of entry e (anything outside [0, gs) is skipped); entry_of(e): what the list stores for e.
// Every thread of the 256-thread workgroup calls it; the table is complete on return.  -> this thread's count of skipped entries
// (each entry is counted by one thread), for the caller's own rule of adding it to its bad-index counter.
template <typename DstOf, typename EntryOf>
__device__ __forceinline__ int inverse_table_build(const InverseTable& tab, int gs, int gr, DstOf dst_of, EntryOf entry_of) {
    const int tid = threadIdx.x;
    int nbad = 0;
    for (int e = tid; e < gr; e += 256) {
        const int64_t v = dst_of(e);
        const bool ok = v >= 0 && v < gs;
        tab.dst[e] = ok ? (int)v : -1;
        nbad += ok ? 0 : 1;
    }
    __syncthreads();
    for (int t = tid; t < gs; t += 256) {                       // count
        int n = 0;
        for (int e = 0; e < gr; ++e) n += tab.dst[e] == t;
        tab.off[t + 1] = n;
    }
    __syncthreads();
    if (tid == 0) {                                             // exclusive prefix (gs <= a few hundred)
        tab.off[0] = 0;
        for (int t = 0; t < gs; ++t) tab.off[t + 1] += tab.off[t];
    }
    __syncthreads();
    for (int t = tid; t < gs; t += 256) {                       // fill, ascending entry order
        int w = tab.off[t];
        for (int e = 0; e < gr; ++e)
            if (tab.dst[e] == t) tab.lst[w++] = entry_of(e);
    }
    __syncthreads();
    return nbad;
}

// ---- derivative of the soft surrogate 0.5 N(u) + 0.5 sigmoid(10 u) on clamp(u, +-10) (fn/snn_coder.py:148-151,
// fd/snn_coder.py:143-155); the forward value of a spike is the hard threshold
__device__ __forceinline__ float surrogate_grad(float u) {
    if (!(u >= -10.0f && u <= 10.0f)) return 0.f;              // torch.clamp passes the gradient on [min, max] only
    const float gauss = expf(-0.5f * u * u) * 0.3989422804014327f;
    const float sg = 1.0f / (1.0f + expf(-10.0f * u));
    return 0.5f * (-u * gauss) + 0.5f * (10.0f * sg * (1.0f - sg));
}

// ---- the clamp of every raw neuron parameter: the value the neuron uses, and whether the raw value lies in [lo, hi] (torch.clamp
// passes the gradient there and nowhere else)
struct Clamped {
    float v;
    bool in;
};
__device__ __forceinline__ Clamped clamp_to(float raw, float lo, float hi) { return Clamped{fminf(fmaxf(raw, lo), hi), raw >= lo && raw <= hi}; }
__device__ __forceinline__ Clamped clamp_membrane_decay(float raw) { return clamp_to(raw, 0.1f, 0.99f); }
__device__ __forceinline__ Clamped clamp_threshold_adapt(float raw) { return clamp_to(raw, 0.001f, 0.1f); }
__device__ __forceinline__ Clamped clamp_refractory_decay(float raw) { return clamp_to(raw, 0.1f, 0.95f); }
__device__ __forceinline__ Clamped clamp_delta_T(float raw) { return clamp_to(raw, 0.1f, 5.0f); }
__device__ __forceinline__ Clamped clamp_theta_rh(float raw) { return clamp_to(raw, 0.1f, 2.0f); }

// ---- BatchNorm in training mode: the statistics of a channel from its f64 sums over `rows` values (biased variance: what the
// normalisation uses), and z = gamma * y_hat + beta with LeakyReLU(0.2) behind it
struct BnStats {
    double mu, var;
    float invstd;
};
__device__ __forceinline__ BnStats bn_batch_stats(double sum, double sum_sq, int64_t rows, float eps) {
    BnStats s;
    s.mu = sum / (double)rows;
    s.var = sum_sq / (double)rows - s.mu * s.mu;
    if (s.var < 0.0) s.var = 0.0;
    s.invstd = (float)(1.0 / sqrt(s.var + (double)eps));
    return s;
}
__device__ __forceinline__ float bn_z(float y, float mu, float is, float ga, float be) { return (y - mu) * is * ga + be; }
__device__ __forceinline__ float bn_lrelu(float y, float mu, float is, float ga, float be) {
    const float z = bn_z(y, mu, is, ga, be);
    return z > 0.f ? z : z * 0.2f;
}

// ---- out[i] = sum over slabs (ascending, plain f32 adds) of part[s][i], i < count: the last pass of both weight gradients
// (train_bf16.hip)
int launch_slab_sum(const float* part, int slabs, int64_t count, float* out, hipStream_t st);

}  // namespace sapcu
