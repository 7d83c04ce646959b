// Test-only shim over the five GEMM launchers (tests/test_gpu_gemm_epilogues.py): no kernels of its own.  One extern "C" entry takes
// flat scalars and pointers, fills a sapcu::GemmArgs — compiled against csrc/common.h, so the struct cannot drift from the library's
// — and calls the launcher or the predicate asked for.  Built as a small shared library linked against libsapcu_hip.so, whose
// launchers it leaves undefined.
#include "common.h"
#include "ops.h"

using namespace sapcu;

extern "C" {

// what: 0 launch_gemm, 1 launch_gemm_sf16, 2 launch_gemm_sf16_ring, 3 launch_gemm_sf16_bt, 4 launch_gemm_shortk (-> status);
//       5 gemm_sf16_bt_ok, 6 gemm_shortk_ok, 7 gemm_sf16_ring_accepts (-> 0 / 1)
int gemm_probe(int what, const float* a, long long r, int k, int lda, const float* w, int n, const float* bias, float* c, int ldc, int epi,
               const float* lif, int lif_T, const float* resid, int ldr, float* c2, const float* q, const float* kf, int ldq, const void* tab,
               const void* w16_hi, const void* w16_lo, int* ovf, int a_split, int c_split, int c2_split, unsigned* max_keys, int max_m,
               float* max_out, void* stream) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.a = a;
    g.r = r;
    g.k = k;
    g.lda = lda;
    g.w = w;
    g.n = n;
    g.bias = bias;
    g.c = c;
    g.ldc = ldc;
    g.epi = epi;
    g.lif = lif;
    g.lif_T = lif_T;
    g.resid = resid;
    g.ldr = ldr;
    g.c2 = c2;
    g.q = q;
    g.kf = kf;
    g.ldq = ldq;
    g.tab = (const int2*)tab;
    g.w16_hi = (const _Float16*)w16_hi;
    g.w16_lo = (const _Float16*)w16_lo;
    g.ovf = ovf;
    g.a_split = a_split;
    g.c_split = c_split;
    g.c2_split = c2_split;
    g.max_keys = max_keys;
    g.max_m = max_m;
    g.max_out = max_out;
    hipStream_t st = (hipStream_t)stream;
    const char* why = nullptr;
    switch (what) {
        case 0: return launch_gemm(g, st);
        case 1: return launch_gemm_sf16(g, st);
        case 2: return launch_gemm_sf16_ring(g, st);
        case 3: return launch_gemm_sf16_bt(g, st);
        case 4: return launch_gemm_shortk(g, st);
        case 5: return gemm_sf16_bt_ok(g) ? 1 : 0;
        case 6: return gemm_shortk_ok(g) ? 1 : 0;
        case 7: return gemm_sf16_ring_accepts(g, &why) ? 1 : 0;
        default: return -1;
    }
}

int gemm_probe_split_weights(const float* w, long long count, void* hi, void* lo, int* ovf, void* stream) {
    return launch_split_weights(w, count, hi, lo, ovf, (hipStream_t)stream);
}

int gemm_probe_to_split_rows(const float* in, long long rows, int k, int ld_in, float* out, int ld_out, void* stream) {
    return launch_to_split_rows(in, rows, k, ld_in, out, ld_out, (hipStream_t)stream);
}

int gemm_probe_edge_table(const int* idx, long long rows, int m, int kk, void* tab, void* stream) {
    return launch_edge_table(idx, rows, m, kk, (int2*)tab, (hipStream_t)stream);
}

int gemm_probe_decode_max_keys(const unsigned* keys, long long count, float* out, void* stream) {
    return launch_decode_max_keys(keys, count, out, (hipStream_t)stream);
}

}  // extern "C"
