// Entropic optimal transport (Sinkhorn) between two clouds without the n x m cost matrix: the potentials, and the row statistics of
// the plan, behind sapcu_amd/sinkhorn.py (include/sapcu_sinkhorn.h states the definition; tests/sinkhorn_ref.py is it in numpy).
//
// sk_softmin_kernel<P>, one row per lane, one column chunk per wavefront:
//   * a half-step is, for every row i, -eps * log sum_j exp(h_j - C_ij / eps): n * m independent (distance, exp) pairs and O(n + m)
//     memory when the cost is recomputed per pair;
//   * the columns are cut into `split` contiguous chunks of whole tiles (sk_split: a function of the row and column counts only);
//     wave w of a workgroup takes chunk blockIdx.y * 4 + w of the 64 rows of blockIdx.x.  A chunk is read 64 columns at a time,
//     coalesced, into the wave's own LDS slab as {x, y, z, h}; every column is then read back by all lanes at once (one address: an
//     LDS broadcast, two ds_read_b128) and met with each lane's own row;
//   * s = (dx^2 + dy^2) + dz^2 in separately rounded operations (the Makefile's -ffp-contract=off), C = s / 2 or sqrt(s);
//     the exponent is h - (C / eps) with the quotient rounded before the subtraction, as the definition writes it: the quotient is
//     fma(C, inv_hi, C * inv_lo) with inv_hi + inv_lo = 1 / eps to twice the working precision (the host splits it), which is the
//     correctly rounded C / eps but for ties no input meets: no division per pair.  The order matters: rounding h - C / eps once
//     instead is as accurate, but the definition's f / eps - C / eps cancels exactly where f = C (one column, equal clouds), and a
//     once-rounded form leaves the quotient's rounding error there, which 1 / eps then magnifies in the plan;
//   * the log-sum-exp is online: a running maximum M and the sum S of exp(. - M).  Each pair costs ONE exp: e = exp(-|a - M|) either
//     rescales S (a new maximum) or is added to it, the addition compensated (sk_online).  M starts at -inf: then a - M = +inf,
//     e = 0 and S = 0 * 0 + 1 — no exp(-inf - (-inf)) is ever formed.  Terms that underflow against the maximum add 0;
//   * the wave stores its (M, S) to the workspace with ordinary stores; a chunk without columns stores (-inf, 0).
// sk_merge_kernel, one row per thread: the partials of a row in chunk order 0, 1, .. by the same rule (a -inf partial is skipped),
// then -eps * (M + log S), optionally damped ((old + new) / 2, the symmetric problem), optionally the next half-step's
// h = log w + value / eps_next.  No float atomics anywhere: every sum has one fixed order, so two runs agree bit for bit, and every
// workspace word that is read was written before in the same call.
// sk_stats_kernel<P>: the same tiling and chunks for r_i = sum_j P_ij and c_i = sum_j P_ij C_ij; sk_sum_kernel adds the partials in
// chunk order.  exp and log are OCML's f64 routines (gfx950 has no f64 transcendental instruction: polynomials on the f64 VALU).
#include <math.h>

#include "common.h"
#include "../../include/sapcu_sinkhorn.h"

namespace sapcu {

constexpr int SK_TILE = 64;               // columns per LDS tile = lanes of a wavefront
constexpr int SK_WAVES = 4;               // column chunks per workgroup
constexpr int SK_MIN_COLS = 128;          // no chunk is planned shorter than this
constexpr int SK_TARGET_WAVES = 4096;     // 16 wavefronts for each of 256 CUs
constexpr int SK_MAX_SPLIT = 64;
constexpr int64_t SK_MAX_POINTS = 1LL << 24;
constexpr int64_t SK_MAX_STEPS = 1LL << 20;

// number of column chunks for `rows` rows against `cols` columns: enough wavefronts to fill the device, no chunk below SK_MIN_COLS
static int sk_split(int64_t rows, int64_t cols) {
    const int64_t groups = (rows + 63) / 64;
    int64_t k = (SK_TARGET_WAVES + groups - 1) / groups;
    const int64_t by_cols = (cols + SK_MIN_COLS - 1) / SK_MIN_COLS;
    if (k > by_cols) k = by_cols;
    if (k > SK_MAX_SPLIT) k = SK_MAX_SPLIT;
    return k < 1 ? 1 : (int)k;
}

// columns per chunk: ceil(cols / split) rounded up to whole tiles
static int64_t sk_chunk(int64_t cols, int split) {
    const int64_t c = (cols + split - 1) / split;
    return (c + SK_TILE - 1) / SK_TILE * SK_TILE;
}

struct SkWs {
    double* hx;        // [n] h of the x side
    double* hy;        // [m] h of the y side
    double* pa;        // [split * rows] partial maxima (statistics: partial r)
    double* pb;        // [split * rows] partial sums (statistics: partial c)
    size_t bytes;
};

static SkWs sk_ws_layout(void* base, int64_t n, int64_t m) {
    const int64_t pn = (int64_t)sk_split(n, m) * n, pm = (int64_t)sk_split(m, n) * m;
    const int64_t parts = pn > pm ? pn : pm;
    WsCarver c(base, 8);
    SkWs w;
    w.hx = c.take<double>(n);
    w.hy = c.take<double>(m);
    w.pa = c.take<double>(parts);
    w.pb = c.take<double>(parts);
    w.bytes = c.bytes();
    return w;
}

struct __align__(16) SkCol {
    double x, y, z, h;
};

struct SkInv {          // 1 / eps as an unevaluated sum hi + lo
    double hi, lo;
};

static SkInv sk_inverse(double eps) {
    SkInv v;
    v.hi = 1.0 / eps;
    v.lo = fma(-v.hi, eps, 1.0) / eps;
    return v;
}

template <int P>
__device__ __forceinline__ double sk_cost(double qx, double qy, double qz, const SkCol& c) {
    const double dx = __dsub_rn(qx, c.x);
    const double dy = __dsub_rn(qy, c.y);
    const double dz = __dsub_rn(qz, c.z);
    double s = __dmul_rn(dx, dx);
    s = __dadd_rn(s, __dmul_rn(dy, dy));
    s = __dadd_rn(s, __dmul_rn(dz, dz));
    return P == 2 ? __dmul_rn(0.5, s) : sqrt(s);             // sqrt(0) = 0: duplicated points
}

// one more term with exponent a into the running (M, S + c): S + c holds the sum of exp(. - M), c what the additions to S rounded
// away.  Without c a row of nearly equal terms (a single column on the other side, equal clouds) loses the same sign of half an ulp
// in every addition once S has grown, log S comes out a few ulps high in every iteration alike, and the potentials drift along the
// iteration's neutral direction (a constant added to f and taken from g) by eps times that, iteration after iteration.
// The addition is compensated where it is the common case: no new maximum, S >= 1 >= e, so (S - t) + e is its exact error.
__device__ __forceinline__ void sk_online(double& M, double& S, double& c, double a) {
    const double d = __dsub_rn(a, M);
    const double e = exp(-fabs(d));
    const bool up = d > 0.0;
    const double t = up ? __fma_rn(S, e, 1.0) : __dadd_rn(S, e);
    c = up ? __dmul_rn(c, e) : __dadd_rn(c, __dadd_rn(__dsub_rn(S, t), e));
    S = t;
    M = up ? a : M;
}

// the same for a partial (exponent a, sum w) of any size against S: the branch-free exact error of an addition
__device__ __forceinline__ void sk_online_partial(double& M, double& S, double& c, double a, double w) {
    const double d = __dsub_rn(a, M);
    const double e = exp(-fabs(d));
    const bool up = d > 0.0;
    const double x = up ? __dmul_rn(S, e) : S, y = up ? w : __dmul_rn(w, e);
    const double t = __dadd_rn(x, y);
    const double yy = __dsub_rn(t, x);
    const double err = __dadd_rn(__dsub_rn(x, __dsub_rn(t, yy)), __dsub_rn(y, yy));
    c = __dadd_rn(up ? __dmul_rn(c, e) : c, err);
    S = t;
    M = up ? a : M;
}

// one tile of the wave's chunk into its slab; -> the number of columns in it
__device__ __forceinline__ int sk_load_tile(SkCol* slab, const double* __restrict__ cols, const double* __restrict__ h, int64_t off,
                                            int64_t c1, int lane) {
    const int64_t j = off + lane;
    SkCol mine{0.0, 0.0, 0.0, 0.0};
    if (j < c1) {
        mine.x = cols[3 * j];
        mine.y = cols[3 * j + 1];
        mine.z = cols[3 * j + 2];
        mine.h = h[j];
    }
    __builtin_amdgcn_wave_barrier();
    slab[lane] = mine;
    __builtin_amdgcn_wave_barrier();
    const int64_t left = c1 - off;
    return left < SK_TILE ? (int)left : SK_TILE;              // wave-uniform
}

template <int P>
__global__ __launch_bounds__(256) void sk_softmin_kernel(const double* __restrict__ rows, int64_t n, const double* __restrict__ cols,
                                                         const double* __restrict__ h, int64_t m, int split, int64_t chunk,
                                                         double inv_hi, double inv_lo, double* __restrict__ pm,
                                                         double* __restrict__ ps) {
    __shared__ SkCol slabs[SK_WAVES][SK_TILE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.y * SK_WAVES + wave;
    if (k >= split) return;                                   // wave-uniform; no workgroup barrier below
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const bool valid = i < n;
    const int64_t ii = valid ? i : n - 1;                     // a spare lane repeats the last row
    const double qx = rows[3 * ii], qy = rows[3 * ii + 1], qz = rows[3 * ii + 2];
    const int64_t c0 = (int64_t)k * chunk;
    const int64_t c1 = c0 + chunk < m ? c0 + chunk : m;
    SkCol* slab = slabs[wave];
    double M = -__builtin_huge_val(), S = 0.0, comp = 0.0;
    for (int64_t off = c0; off < c1; off += SK_TILE) {
        const int cnt = sk_load_tile(slab, cols, h, off, c1, lane);
#pragma unroll 2
        for (int t = 0; t < cnt; ++t) {
            const SkCol c = slab[t];                          // one address for the whole wave: a broadcast
            const double C = sk_cost<P>(qx, qy, qz, c);
            const double a = __dsub_rn(c.h, __fma_rn(C, inv_hi, __dmul_rn(C, inv_lo)));       // h - (C / eps), the quotient rounded first
            sk_online(M, S, comp, a);
        }
    }
    if (valid) {
        pm[(int64_t)k * n + i] = M;
        ps[(int64_t)k * n + i] = __dadd_rn(S, comp);
    }
}

__global__ __launch_bounds__(256) void sk_merge_kernel(const double* __restrict__ pm, const double* __restrict__ ps, int64_t n, int split,
                                                       double eps, int damped, double* __restrict__ out, double* __restrict__ hnext,
                                                       double eps_next) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double M = -__builtin_huge_val(), S = 0.0, comp = 0.0;
    for (int k = 0; k < split; ++k) {
        const double mk = pm[(int64_t)k * n + i];
        if (mk == -__builtin_huge_val()) continue;            // a chunk without columns
        sk_online_partial(M, S, comp, mk, ps[(int64_t)k * n + i]);
    }
    double v = __dmul_rn(-eps, __dadd_rn(M, log(__dadd_rn(S, comp))));
    if (damped) v = __dmul_rn(0.5, __dadd_rn(out[i], v));
    out[i] = v;
    if (hnext) hnext[i] = __dadd_rn(-log((double)n), __ddiv_rn(v, eps_next));        // log w with the log that meets it again: see sk_h_kernel
}

// pot (may be null) = 0 and h = log w: the start f = g = 0;  or, with src, h = log w + src / eps.  log w = log(1 / count) is taken as
// -log(count) with the device's own log: the half-step that reads h ends in log S, and where S = count (equal clouds, a single
// column, the fixed point of a uniform problem) the two cancel exactly.  A host log that rounds the other way leaves one ulp of
// log(count) there in every iteration, which the iteration does not damp: adding a constant to f and taking it from g is its one
// neutral direction, so the potentials would drift by eps * ulp per iteration.
__global__ __launch_bounds__(256) void sk_h_kernel(const double* __restrict__ src, int64_t count, double eps,
                                                   double* __restrict__ zero_out, double* __restrict__ h) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    if (zero_out) zero_out[i] = 0.0;
    const double log_w = -log((double)count);
    h[i] = src ? __dadd_rn(log_w, __ddiv_rn(src[i], eps)) : log_w;
}

template <int P>
__global__ __launch_bounds__(256) void sk_stats_kernel(const double* __restrict__ rows, int64_t n, const double* __restrict__ cols,
                                                       const double* __restrict__ f, const double* __restrict__ g, int64_t m, int split,
                                                       int64_t chunk, double inv_hi, double inv_lo, double ab, double* __restrict__ pr,
                                                       double* __restrict__ pc) {
    __shared__ SkCol slabs[SK_WAVES][SK_TILE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.y * SK_WAVES + wave;
    if (k >= split) return;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const bool valid = i < n;
    const int64_t ii = valid ? i : n - 1;
    const double qx = rows[3 * ii], qy = rows[3 * ii + 1], qz = rows[3 * ii + 2], fi = f[ii];
    const int64_t c0 = (int64_t)k * chunk;
    const int64_t c1 = c0 + chunk < m ? c0 + chunk : m;
    SkCol* slab = slabs[wave];
    double r = 0.0, cs = 0.0;
    for (int64_t off = c0; off < c1; off += SK_TILE) {
        const int cnt = sk_load_tile(slab, cols, g, off, c1, lane);            // the slab's h slot carries g_j
#pragma unroll 2
        for (int t = 0; t < cnt; ++t) {
            const SkCol c = slab[t];
            const double C = sk_cost<P>(qx, qy, qz, c);
            const double u = __dsub_rn(__dadd_rn(fi, c.h), C);                 // (f_i + g_j) - C_ij
            const double pij = __dmul_rn(ab, exp(__fma_rn(u, inv_hi, __dmul_rn(u, inv_lo))));
            r = __dadd_rn(r, pij);
            cs = __dadd_rn(cs, __dmul_rn(pij, C));
        }
    }
    if (valid) {
        pr[(int64_t)k * n + i] = r;
        pc[(int64_t)k * n + i] = cs;
    }
}

__global__ __launch_bounds__(256) void sk_sum_kernel(const double* __restrict__ pr, const double* __restrict__ pc, int64_t n, int split,
                                                     double* __restrict__ r_out, double* __restrict__ c_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double r = 0.0, c = 0.0;
    for (int k = 0; k < split; ++k) {
        r = __dadd_rn(r, pr[(int64_t)k * n + i]);
        c = __dadd_rn(c, pc[(int64_t)k * n + i]);
    }
    r_out[i] = r;
    c_out[i] = c;
}

static dim3 sk_grid(int64_t rows, int split) { return dim3((unsigned)((rows + 63) / 64), (unsigned)((split + SK_WAVES - 1) / SK_WAVES)); }
static dim3 sk_rows256(int64_t rows) { return dim3((unsigned)((rows + 255) / 256)); }

// out = softmin over `cols` with the h already in `h` (damped: out = (out + softmin) / 2); hnext as sk_merge_kernel
static int launch_softmin(const double* rows, int64_t n, const double* cols, const double* h, int64_t m, int p, double eps, int split,
                          int damped, double* out, double* hnext, double eps_next, const SkWs& w, hipStream_t st) {
    const SkInv inv = sk_inverse(eps);
    const int64_t chunk = sk_chunk(m, split);
    if (p == 2)
        hipLaunchKernelGGL(sk_softmin_kernel<2>, sk_grid(n, split), dim3(256), 0, st, rows, n, cols, h, m, split, chunk, inv.hi, inv.lo,
                           w.pa, w.pb);
    else
        hipLaunchKernelGGL(sk_softmin_kernel<1>, sk_grid(n, split), dim3(256), 0, st, rows, n, cols, h, m, split, chunk, inv.hi, inv.lo,
                           w.pa, w.pb);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(sk_merge_kernel, sk_rows256(n), dim3(256), 0, st, w.pa, w.pb, n, split, eps, damped, out, hnext, eps_next);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

static int launch_h(const double* src, int64_t count, double eps, double* zero_out, double* h, hipStream_t st) {
    hipLaunchKernelGGL(sk_h_kernel, sk_rows256(count), dim3(256), 0, st, src, count, eps, zero_out, h);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

static int launch_sinkhorn(const double* x, int64_t n, const double* y, int64_t m, int p, const double* sched, int64_t n_sched, double eps,
                           int64_t iters, double* f, double* g, const SkWs& w, hipStream_t st) {
    const int64_t total = n_sched + iters;
    auto eps_of = [&](int64_t it) { return it < n_sched ? sched[it] : eps; };
    int rc;
    if (!y) {                                                                  // OT(a, a): f <- (f + softmin(f)) / 2
        if ((rc = launch_h(nullptr, n, 1.0, f, w.hx, st)) != SAPCU_OK) return rc;
        const int split = sk_split(n, n);
        for (int64_t it = 0; it < total; ++it) {
            const double e = eps_of(it), en = it + 1 < total ? eps_of(it + 1) : e;
            if ((rc = launch_softmin(x, n, x, w.hx, n, p, e, split, 1, f, w.hx, en, w, st)) != SAPCU_OK) return rc;
        }
        return SAPCU_OK;
    }
    if ((rc = launch_h(nullptr, n, 1.0, f, w.hx, st)) != SAPCU_OK) return rc;
    if ((rc = launch_h(nullptr, m, 1.0, g, w.hy, st)) != SAPCU_OK) return rc;
    const int split_f = sk_split(n, m), split_g = sk_split(m, n);
    for (int64_t it = 0; it < total; ++it) {
        const double e = eps_of(it), en = it + 1 < total ? eps_of(it + 1) : e;
        if ((rc = launch_softmin(x, n, y, w.hy, m, p, e, split_f, 0, f, w.hx, e, w, st)) != SAPCU_OK) return rc;
        if ((rc = launch_softmin(y, m, x, w.hx, n, p, e, split_g, 0, g, w.hy, en, w, st)) != SAPCU_OK) return rc;
    }
    return SAPCU_OK;
}

static bool sk_positive(double v) { return v > 0.0 && v < __builtin_huge_val(); }        // false for NaN

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

#define SK_CHECK_SIZES(what)                                                                                                         \
    SAPCU_CHECK_ARG(n >= 1 && n <= SK_MAX_POINTS && m >= 1 && m <= SK_MAX_POINTS, what ": need 1 <= n, m <= 2^24 (n=%lld, m=%lld)", \
                    (long long)n, (long long)m)
#define SK_CHECK_WS(what)                                                                                              \
    SAPCU_CHECK_ARG(((uintptr_t)workspace & 7) == 0, what ": the workspace must be 8-byte aligned (f64 tables)");      \
    const int64_t need = (int64_t)sk_ws_layout(nullptr, n, m).bytes;                                                   \
    SAPCU_CHECK_ARG(workspace && workspace_bytes >= need, what ": workspace of %lld bytes, need %lld", (long long)workspace_bytes, \
                    (long long)need)

extern "C" {

int64_t sapcu_sinkhorn_workspace_bytes(int64_t n, int64_t m) {
    if (n < 1 || n > SK_MAX_POINTS || m < 1 || m > SK_MAX_POINTS) return -1;
    return (int64_t)sk_ws_layout(nullptr, n, m).bytes;
}

int sapcu_softmin_f64(const double* x, int64_t n, const double* y, int64_t m, const double* pot_y, int p, double eps, double* out,
                      void* workspace, int64_t workspace_bytes, void* stream) {
    SK_CHECK_SIZES("softmin");
    SAPCU_CHECK_ARG(x && y && pot_y && out, "softmin: null pointer");
    SAPCU_CHECK_ARG(p == 1 || p == 2, "softmin: p must be 1 or 2 (p=%d)", p);
    SAPCU_CHECK_ARG(sk_positive(eps), "softmin: eps must be finite and > 0");
    SK_CHECK_WS("softmin");
    const SkWs w = sk_ws_layout(workspace, n, m);
    hipStream_t st = (hipStream_t)stream;
    const int rc = launch_h(pot_y, m, eps, nullptr, w.hy, st);
    if (rc != SAPCU_OK) return rc;
    return launch_softmin(x, n, y, w.hy, m, p, eps, sk_split(n, m), 0, out, nullptr, 1.0, w, st);
}

int sapcu_sinkhorn_f64(const double* x, int64_t n, const double* y, int64_t m, int p, const double* eps_schedule_host, int64_t n_schedule,
                       double eps, int64_t iters, double* f_out, double* g_out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!y) m = n;
    SK_CHECK_SIZES("sinkhorn");
    SAPCU_CHECK_ARG(x && f_out && (g_out || !y), "sinkhorn: null pointer");
    SAPCU_CHECK_ARG(p == 1 || p == 2, "sinkhorn: p must be 1 or 2 (p=%d)", p);
    SAPCU_CHECK_ARG(iters >= 0 && n_schedule >= 0 && iters <= SK_MAX_STEPS && n_schedule <= SK_MAX_STEPS && n_schedule + iters <= SK_MAX_STEPS,
                    "sinkhorn: need iters >= 0, n_schedule >= 0 and at most 2^20 iterations in all");
    SAPCU_CHECK_ARG(eps_schedule_host || n_schedule == 0, "sinkhorn: null schedule");
    SAPCU_CHECK_ARG(sk_positive(eps), "sinkhorn: eps must be finite and > 0");
    for (int64_t k = 0; k < n_schedule; ++k)
        SAPCU_CHECK_ARG(sk_positive(eps_schedule_host[k]), "sinkhorn: schedule entry %lld must be finite and > 0", (long long)k);
    SK_CHECK_WS("sinkhorn");
    return launch_sinkhorn(x, n, y, m, p, eps_schedule_host, n_schedule, eps, iters, f_out, g_out, sk_ws_layout(workspace, n, m),
                           (hipStream_t)stream);
}

int sapcu_plan_stats_f64(const double* x, int64_t n, const double* y, int64_t m, const double* f, const double* g, int p, double eps,
                         double* r_out, double* c_out, void* workspace, int64_t workspace_bytes, void* stream) {
    SK_CHECK_SIZES("plan_stats");
    SAPCU_CHECK_ARG(x && y && f && g && r_out && c_out, "plan_stats: null pointer");
    SAPCU_CHECK_ARG(p == 1 || p == 2, "plan_stats: p must be 1 or 2 (p=%d)", p);
    SAPCU_CHECK_ARG(sk_positive(eps), "plan_stats: eps must be finite and > 0");
    SK_CHECK_WS("plan_stats");
    const SkWs w = sk_ws_layout(workspace, n, m);
    hipStream_t st = (hipStream_t)stream;
    const SkInv inv = sk_inverse(eps);
    const int split = sk_split(n, m);
    const int64_t chunk = sk_chunk(m, split);
    const double ab = (1.0 / (double)n) * (1.0 / (double)m);
    if (p == 2)
        hipLaunchKernelGGL(sk_stats_kernel<2>, sk_grid(n, split), dim3(256), 0, st, x, n, y, f, g, m, split, chunk, inv.hi, inv.lo, ab, w.pa,
                           w.pb);
    else
        hipLaunchKernelGGL(sk_stats_kernel<1>, sk_grid(n, split), dim3(256), 0, st, x, n, y, f, g, m, split, chunk, inv.hi, inv.lo, ab, w.pa,
                           w.pb);
    SAPCU_CHECK_LAUNCH();
    hipLaunchKernelGGL(sk_sum_kernel, sk_rows256(n), dim3(256), 0, st, w.pa, w.pb, n, split, r_out, c_out);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}

// test hooks (no header).  {SK_TILE, SK_MIN_COLS, split, chunk} of `rows` rows against `cols` columns
int sapcu_internal_sinkhorn_split(int64_t rows, int64_t cols, int64_t* out_host) {
    SAPCU_CHECK_ARG(rows >= 1 && cols >= 1 && out_host, "sinkhorn_split: bad argument");
    const int split = sk_split(rows, cols);
    out_host[0] = SK_TILE;
    out_host[1] = SK_MIN_COLS;
    out_host[2] = split;
    out_host[3] = sk_chunk(cols, split);
    return SAPCU_OK;
}

// sapcu_softmin_f64 with the number of column chunks given (1..SK_MAX_SPLIT): chunks beyond the last column are empty.
// The workspace holds m + 2 * split * n doubles.
int sapcu_internal_softmin_split_f64(const double* x, int64_t n, const double* y, int64_t m, const double* pot_y, int p, double eps,
                                     int split, double* out, void* workspace, int64_t workspace_bytes, void* stream) {
    SK_CHECK_SIZES("softmin_split");
    SAPCU_CHECK_ARG(x && y && pot_y && out && (p == 1 || p == 2) && sk_positive(eps) && split >= 1 && split <= SK_MAX_SPLIT,
                    "softmin_split: bad argument");
    const int64_t need = (m + 2 * (int64_t)split * n) * 8;
    SAPCU_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= need, "softmin_split: workspace");
    SkWs w;
    w.hx = nullptr;
    w.hy = (double*)workspace;
    w.pa = w.hy + m;
    w.pb = w.pa + (int64_t)split * n;
    w.bytes = (size_t)need;
    hipStream_t st = (hipStream_t)stream;
    const int rc = launch_h(pot_y, m, eps, nullptr, w.hy, st);
    if (rc != SAPCU_OK) return rc;
    return launch_softmin(x, n, y, w.hy, m, p, eps, split, 0, out, nullptr, 1.0, w, st);
}

}  // extern "C"
