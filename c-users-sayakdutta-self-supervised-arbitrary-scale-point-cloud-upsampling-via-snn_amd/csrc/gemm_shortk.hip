// Short-K split-f16 GEMM with a neuron epilogue (fn fc1: K = 64; fn conv_final: K = 192), f32-layout A:
//
//   C[r, n] = LIF_T( A[r, k] . W[n, k]^T / 16 + bias[n] ),   k in {64, 128, 192}
//
// Same arithmetic as gemm_sf16_kernel, bit for bit (the tests compare the two with torch.equal): operands split as split8 does,
// weights from the pre-split x16 planes, v_mfma_f32_32x32x16_f16 into one f32 accumulator per output in the order a_lo.w_hi,
// a_hi.w_lo, a_hi.w_hi per k32 step (each over both k16 halves), k32 ascending; then x 1/16, + bias, the T-step neuron loop.
//
// At these depths the matrix work is a small fraction of the neuron loop (K = 64: one tenth), so gemm_sf16_kernel's split into
// MFMA producers and epilogue consumers leaves half the waves at the barriers.  Here EVERY wave does both jobs:
//   * a workgroup owns one group of 32 RT rows.  It splits the group's A panel ONCE into LDS (hi | lo planes, 16-byte chunks
//     XOR-swizzled by (row >> 1) & 7 inside every 128-byte block as in gemm_sf16.hip: conflict-free ds_read_b128 fragments) and
//     meets at ONE barrier;
//   * from there on the waves are independent.  A wave walks the 32-column tiles w, w + nw, ...: for each it owns all 32 RT rows
//     (RT accumulators of 16 registers; its W fragments go global -> registers, L2 hits, 4 K / (32 RT) bytes per output element),
//     runs its MFMAs, then the neuron loop on the accumulators where they are — eight elements (four packed pairs) of one
//     channel at a time — and stores.  Waves of one SIMD are in different phases, so one wave's MFMAs and W loads run under
//     another's neuron arithmetic without any scheduling in the source.
//   * EPI_LIF_MAX with whole patches in the row group (RT = 3: 96 rows = two patches of 48): a lane holds one column of all 96
//     rows, so the max over a patch's points is a max over the lane's own registers and one exchange between the two lane
//     halves; pooled[patch, col] is written directly — no key buffer, no atomics, no memset, no decode launch.
#include "common.h"
#include "gemm_epi.h"

namespace sapcu {

typedef _Float16 sk_half8 __attribute__((ext_vector_type(8)));

constexpr int SK_MAX_WAVES = 8;

__device__ __forceinline__ int sk_chunk_offset(int row, int chunk, int k) {      // bytes inside one plane
    return row * (k * 2) + (((chunk & ~7) | ((chunk & 7) ^ ((row >> 1) & 7))) * 16);
}

template <int EPI, int RT>
__global__ __launch_bounds__(SK_MAX_WAVES * 64, 4) void gemm_shortk_kernel(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sk_smem[];
    constexpr int RG = 32 * RT;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int nw = blockDim.x >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const int K = g.k;
    const int plane_bytes = RG * K * 2;
    const int64_t row0 = (int64_t)blockIdx.x * RG;

    // ---- the group's A panel: f32 rows -> hi | lo planes in LDS, once (rows past r repeat row r - 1: they feed masked outputs only)
    {
        const int cpr = K >> 3;                      // 8-float chunks per row
        const int total = RG * cpr;
        float amax = 0.f;
        for (int c = tid; c < total; c += blockDim.x) {
            const int row = c / cpr, ch = c - row * cpr;
            int64_t grow = row0 + row;
            if (grow >= g.r) grow = g.r - 1;
            const float* ap = g.a + grow * g.lda + ch * 8;
            const float4 x0 = ld4(ap), x1 = ld4(ap + 4);
            const float xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
            sk_half8 hi, lo;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const _Float16 hh = (_Float16)xs[i];
                hi[i] = hh;
                lo[i] = (_Float16)(xs[i] - (float)hh);
                amax = fmaxf(amax, fabsf(xs[i]));
            }
            const int off = sk_chunk_offset(row, ch, K);
            *reinterpret_cast<sk_half8*>(sk_smem + off) = hi;
            *reinterpret_cast<sk_half8*>(sk_smem + plane_bytes + off) = lo;
        }
        if (amax > 65504.0f && g.ovf) atomicAdd(g.ovf, 1);
    }
    __syncthreads();

    const int nct = (g.n + 31) >> 5;
    const int nk = K >> 6;
    for (int ct = wave; ct < nct; ct += nw) {
        const int col = ct * 32 + r32;
        const bool col_ok = col < g.n;
        const int cc = col_ok ? col : g.n - 1;
        const _Float16* wp[2] = {g.w16_hi + (int64_t)cc * K + h * 8, g.w16_lo + (int64_t)cc * K + h * 8};
        f32x16 acc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[rt][e] = 0.f;

        sk_half8 wa[2][2], wb[2][2];                 // [plane][k16 half] of an even / odd k32 step
        auto load_w = [&](sk_half8 (&w)[2][2], int k32) {
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int t = 0; t < 2; ++t) w[p][t] = *reinterpret_cast<const sk_half8*>(wp[p] + k32 * 32 + t * 16);
        };
        auto step = [&](const sk_half8 (&w)[2][2], int k32) {
            auto product = [&](int a_plane, int w_plane) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const sk_half8 a = *reinterpret_cast<const sk_half8*>(
                            sk_smem + a_plane * plane_bytes + sk_chunk_offset(rt * 32 + r32, (2 * k32 + t) * 2 + h, K));
                        acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, w[w_plane][t], acc[rt], 0, 0, 0);
                    }
            };
            product(1, 0);      // a_lo . w_hi
            product(0, 1);      // a_hi . w_lo
            product(0, 0);      // a_hi . w_hi
        };
        load_w(wa, 0);
        for (int kt = 0; kt < nk; ++kt) {
            load_w(wb, 2 * kt + 1);
            step(wa, 2 * kt);
            if (kt + 1 < nk) load_w(wa, 2 * kt + 2);
            step(wb, 2 * kt + 1);
        }

        // ---- epilogue on the accumulators: acc[rt][e] = row 32 rt + 8 (e >> 2) + 4 h + (e & 3), column col
        const float bias = g.bias ? g.bias[cc] : 0.f;
        const NeuronP np = load_lif(g.lif, g.n, cc);
        // lane offsets inside a row block of sixteen: rows + 4 h, this column (f32 elements / halves of a split row, gemm_epi.h)
        const int off_f32 = 4 * h * g.ldc + col;
        const int off_hi = 8 * h * g.ldc + split_hi_index(g.ldc, col), off_lo = 8 * h * g.ldc + split_lo_index(g.ldc, col);
        float pmax[2] = {-INFINITY, -INFINITY};      // EPI_LIF_MAX, RT = 3: rows 0..47 | 48..95
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int64_t grow = row0 + rt * 32 + half * 16;     // the eight elements lie in rows grow .. grow + 15
                if (grow >= g.r) continue;                            // (wave-uniform)
                __builtin_amdgcn_sched_barrier(0);                    // one group's live set at a time
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = __fadd_rn(__fmul_rn(acc[rt][half * 8 + e], 0.0625f), bias);   // undo W x 16
                lif_selfloop_n<8>(v, np, g.lif_T);
                if (EPI == EPI_LIF_MAX) {
                    float best = v[0];
#pragma unroll
                    for (int e = 1; e < 8; ++e) best = fmaxf(best, v[e]);
                    const int pi = (rt * 2 + half) >= 3 ? 1 : 0;      // (static after unrolling)
                    pmax[pi] = fmaxf(pmax[pi], best);
                } else {
                    // uniform row pointers + one 32-bit lane offset: nothing per element for the compiler to precompute and spill
                    const int left = (g.r - grow) < 16 ? (int)(g.r - grow) : 16;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int lr = 8 * (e >> 2) + (e & 3);        // + 4 h: the row inside the sixteen
                        float* rowp = g.c + (grow + lr) * g.ldc;
                        if (!col_ok || lr + 4 * h >= left) continue;
                        if (g.c_split) {
                            _Float16* rp = reinterpret_cast<_Float16*>(rowp);
                            const _Float16 hi = (_Float16)v[e];
                            rp[off_hi] = hi;
                            rp[off_lo] = (_Float16)(v[e] - (float)hi);
                        } else {
                            rowp[off_f32] = v[e];
                        }
                    }
                }
            }
        }
        if (EPI == EPI_LIF_MAX) {
            // the other lane half holds the patch's other rows of this column
            pmax[0] = fmaxf(pmax[0], __shfl_xor(pmax[0], 32));
            pmax[1] = fmaxf(pmax[1], __shfl_xor(pmax[1], 32));
            float* op = g.max_out + (int64_t)blockIdx.x * 2 * g.ldc;  // (uniform) half h writes patch h of the group
            const int left = (g.r - row0) < RG ? (int)(g.r - row0) : RG;
            if (col_ok && h * 48 < left) op[h * g.ldc + col] = h ? pmax[1] : pmax[0];
        }
    }
}

bool gemm_shortk_ok(const GemmArgs& g) {
    if (g.a_split || !g.w16_hi || !g.w16_lo || !g.lif || g.lif_T < 1) return false;
    if (g.k < 64 || g.k > 192 || g.k % 64 != 0) return false;
    if (g.r >= ((int64_t)1 << 31) * 32) return false;                 // one workgroup per row group
    if (g.epi == EPI_LIF) return true;
    // the register max needs whole patches in a row group: two patches of 48 rows in 96
    return g.epi == EPI_LIF_MAX && g.max_out && g.max_m == 48 && g.r % 48 == 0;
}

template <int EPI, int RT>
static int launch_shortk_t(const GemmArgs& g, hipStream_t st) {
    static DeviceOnce lds_once;
    constexpr int RG = 32 * RT;
    SAPCU_SET_MAX_LDS(lds_once, (&gemm_shortk_kernel<EPI, RT>), RG * 192 * 4);
    const int nct = (g.n + 31) / 32;
    const int nw = nct < SK_MAX_WAVES ? nct : SK_MAX_WAVES;
    const int64_t groups = (g.r + RG - 1) / RG;
    hipLaunchKernelGGL((gemm_shortk_kernel<EPI, RT>), dim3((unsigned)groups), dim3(nw * 64), (size_t)RG * g.k * 4, st, g);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

int launch_gemm_shortk(const GemmArgs& g, hipStream_t st) {
    if (g.r == 0 || g.n == 0) return SAPCU_OK;
    SAPCU_CHECK_ARG(gemm_shortk_ok(g), "gemm_shortk: shape or epilogue not served (k=%d epi=%d)", g.k, g.epi);
    SAPCU_CHECK_ARG(g.lda % 4 == 0 && ((uintptr_t)g.a & 15) == 0 && ((uintptr_t)g.w16_hi & 15) == 0 && ((uintptr_t)g.w16_lo & 15) == 0,
                    "gemm_shortk: operands must be 16-byte aligned (lda=%d)", g.lda);
    if (g.epi == EPI_LIF_MAX) return launch_shortk_t<EPI_LIF_MAX, 3>(g, st);
    return launch_shortk_t<EPI_LIF, 2>(g, st);
}

}  // namespace sapcu
