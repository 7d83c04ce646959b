// The building blocks of csrc/wave_ops.h, each behind a thin kernel, swept against a plain host reference written here.
//
// Four sections, one line each on stdout: "<name>: cases N, mismatches M" (then the first mismatch's parameters); the exit status is
// non-zero if any M is.  tests/test_gpu_wave_ops.py builds this file (hipcc -O3 -ffp-contract=off -I csrc), runs it once and asserts M == 0 and N == the
// count it computes itself.  Every comparison is == on bits or integers.
//
//   arrival-order list   WaveTopK<false> at k = 1..64 and WaveTopK<true> at k = 1..128 (the two-slot type's read_tau branches on k),
//                        one wave a case, first_slab then offer(d, off) as tp_knn_kernel calls them, n candidates from NSET(k)
//                        (n < k included), seven distance patterns; reference: std::stable_sort over the finite distances, the
//                        first k, then empty entries (+inf, NONE); every entry's distance bits and index, and tau, are compared;
//   keyed list           WaveTopK<false, true> at k = 1..64, the same patterns under shuffled indices, offered as consecutive
//                        ranges of 0..150 candidates whose last slab is padded with (+inf, INT_MAX) lanes as grid_scan_range pads;
//                        reference: std::sort by (distance, index) over the distances that are not NaN; tau_i is compared too;
//   block collectives    block_excl_scan<W> twice on one scratch, block_min / block_max on int, float, double, the wave folds;
//   numpy sum            np_leaf_sum at n = 0..128, plan + leaves + fold against the recursive definition, one guard case.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <type_traits>
#include <vector>

#include "wave_ops.h"

using namespace sapcu;

#define HIP_OK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__);     \
            std::exit(2);                                                                          \
        }                                                                                          \
    } while (0)

static const double INF = std::numeric_limits<double>::infinity();
static const int IMAX = 0x7fffffff;

template <typename T>
struct Dev {      // a device array with its host copy
    std::vector<T> h;
    T* d = nullptr;
    explicit Dev(size_t n = 0) : h(n) {}
    void up() {
        HIP_OK(hipMalloc(&d, std::max<size_t>(h.size(), 1) * sizeof(T)));
        HIP_OK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    void down() { HIP_OK(hipMemcpy(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost)); }
    ~Dev() {
        if (d) (void)hipFree(d);
    }
};

struct Report {
    const char* name;
    long cases = 0, mismatches = 0;
    std::string first;
    void miss(const std::string& what) {
        if (!mismatches++) first = what;
    }
    bool print() const {
        std::printf("%s: cases %ld, mismatches %ld\n", name, cases, mismatches);
        if (mismatches) std::printf("  first mismatch: %s\n", first.c_str());
        return mismatches == 0;
    }
};

static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}
template <typename... A>
static std::string fmt(const char* f, A... a) {
    char buf[512];
    std::snprintf(buf, sizeof buf, f, a...);
    return buf;
}

// ============================================================================================================== the k-lists
static std::vector<int> nset(int k) {
    std::vector<int> v = {1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, k - 1, k, k + 1};
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    v.erase(std::remove_if(v.begin(), v.end(), [](int n) { return n < 1; }), v.end());
    return v;
}

constexpr int PATTERNS = 7;
static std::vector<double> pattern(int p, int n, std::mt19937_64& rng) {
    std::vector<double> d(n);
    auto four = [&] {
        double vals[4];
        for (double& v : vals) v = (double)(rng() % 1000) / 8.0;
        for (int j = 0; j < n; ++j) d[j] = vals[rng() % 4];
    };
    switch (p) {
    case 1:                                              // a permutation of 0..n-1
        for (int j = 0; j < n; ++j) d[j] = j;
        std::shuffle(d.begin(), d.end(), rng);
        break;
    case 2:                                              // all equal
        for (int j = 0; j < n; ++j) d[j] = 3.0;
        break;
    case 3:                                              // four values
        four();
        break;
    case 4:                                              // strictly descending: every candidate enters at position 0
        for (int j = 0; j < n; ++j) d[j] = n - 1 - j;
        break;
    case 5:                                              // strictly ascending
        for (int j = 0; j < n; ++j) d[j] = j;
        break;
    case 6:                                              // every value four times, shuffled
        for (int j = 0; j < n; ++j) d[j] = j / 4;
        std::shuffle(d.begin(), d.end(), rng);
        break;
    default: {                                           // four values; NaN at three and +inf at three other positions among the
        four();                                          // first 64, and the same again past position 64 (as many as fit)
        for (int lo = 0; lo < 128 && lo < n; lo += 64) {
            const int hi = lo == 0 ? std::min(n, 64) : n;
            std::vector<int> pos;
            for (int j = lo; j < hi; ++j) pos.push_back(j);
            std::shuffle(pos.begin(), pos.end(), rng);
            for (int t = 0; t < 6 && t < (int)pos.size(); ++t) d[pos[t]] = t < 3 ? std::numeric_limits<double>::quiet_NaN() : INF;
        }
    }
    }
    return d;
}

struct ListCase {
    int k, n, pat;
    int64_t off;      // first candidate of the case in the stream
    int slabs;        // keyed: 64-lane slabs of the padded stream
};

template <bool TWO>
__global__ __launch_bounds__(64) void arrival_kernel(const ListCase* __restrict__ cases, const double* __restrict__ dist,
                                                     double* __restrict__ out_d, int* __restrict__ out_i, double* __restrict__ out_tau) {
    const ListCase c = cases[blockIdx.x];
    const int lane = threadIdx.x;
    WaveTopK<TWO> top(c.k);
    for (int off = 0; off < c.n; off += 64) {
        const int j = off + lane;
        const double d = j < c.n ? dist[c.off + j] : __builtin_huge_val();
        if (off == 0) top.first_slab(d, j < c.n ? j : 0x7fffffff);
        else top.offer(d, off);
    }
#pragma unroll
    for (int s = 0; s < top.SLOTS; ++s) {
        out_d[(int64_t)blockIdx.x * 128 + 64 * s + lane] = top.d[s];
        out_i[(int64_t)blockIdx.x * 128 + 64 * s + lane] = top.i[s];
    }
    if (lane == 0) out_tau[blockIdx.x] = top.tau;
}

__global__ __launch_bounds__(64) void keyed_kernel(const ListCase* __restrict__ cases, const double* __restrict__ dist,
                                                   const int* __restrict__ index, double* __restrict__ out_d, int* __restrict__ out_i,
                                                   double* __restrict__ out_tau, int* __restrict__ out_tau_i, double inf) {
    const ListCase c = cases[blockIdx.x];
    const int lane = threadIdx.x;
    WaveTopK<false, true> top(c.k);
    // The constructor's value again, from a kernel argument.  In THIS kernel the threshold stays wave-uniform from the start, and
    // hipcc 6.x for gfx950 then builds +inf with one 64-bit scalar move whose literal the assembler cuts to its lower 32 bits: the
    // list would start with tau = 0.0 and take nothing but zero distances.  (No kernel of the library holds such a move: checked
    // in the assembly of every csrc/*.hip when this probe was written.)
    top.tau = inf;
    for (int s = 0; s < c.slabs; ++s) top.offer(dist[c.off + 64 * s + lane], index[c.off + 64 * s + lane]);
    out_d[(int64_t)blockIdx.x * 64 + lane] = top.d[0];
    out_i[(int64_t)blockIdx.x * 64 + lane] = top.i[0];
    if (lane == 0) {
        out_tau[blockIdx.x] = top.tau;
        out_tau_i[blockIdx.x] = top.tau_i;
    }
}

template <bool TWO>
static void arrival_sweep(Report& rep, std::mt19937_64& rng) {
    const int kmax = TWO ? 128 : 64;
    std::vector<ListCase> cases;
    Dev<double> dist;
    for (int k = 1; k <= kmax; ++k)
        for (int n : nset(k))
            for (int p = 1; p <= PATTERNS; ++p) {
                cases.push_back({k, n, p, (int64_t)dist.h.size(), 0});
                const std::vector<double> d = pattern(p, n, rng);
                dist.h.insert(dist.h.end(), d.begin(), d.end());
            }
    Dev<ListCase> dc(cases.size());
    dc.h = cases;
    Dev<double> od(cases.size() * 128), otau(cases.size());
    Dev<int> oi(cases.size() * 128);
    dc.up(), dist.up(), od.up(), oi.up(), otau.up();
    hipLaunchKernelGGL(arrival_kernel<TWO>, dim3((unsigned)cases.size()), dim3(64), 0, 0, dc.d, dist.d, od.d, oi.d, otau.d);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    od.down(), oi.down(), otau.down();
    for (size_t c = 0; c < cases.size(); ++c) {
        const ListCase& cs = cases[c];
        const double* d = dist.h.data() + cs.off;
        std::vector<int> order;
        for (int j = 0; j < cs.n; ++j)
            if (std::isfinite(d[j])) order.push_back(j);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return d[a] < d[b]; });
        ++rep.cases;
        bool bad = false;
        for (int p = 0; p < cs.k && !bad; ++p) {
            const double rd = p < (int)order.size() ? d[order[p]] : INF;
            const int ri = p < (int)order.size() ? order[p] : -1;
            if (bits(od.h[c * 128 + p]) != bits(rd) || oi.h[c * 128 + p] != ri) {
                bad = true;
                rep.miss(fmt("slots %d k %d n %d pattern %d entry %d: (%.17g, %d), expected (%.17g, %d)", TWO ? 2 : 1, cs.k, cs.n, cs.pat, p,
                             od.h[c * 128 + p], oi.h[c * 128 + p], rd, ri));
            }
        }
        const double rtau = cs.k <= (int)order.size() ? d[order[cs.k - 1]] : INF;
        if (!bad && bits(otau.h[c]) != bits(rtau))
            rep.miss(fmt("slots %d k %d n %d pattern %d tau %.17g, expected %.17g", TWO ? 2 : 1, cs.k, cs.n, cs.pat, otau.h[c], rtau));
    }
}

static void keyed_sweep(Report& rep, std::mt19937_64& rng) {
    std::vector<ListCase> cases;
    std::vector<std::vector<std::pair<double, int>>> cands;      // per case: (distance, index) in arrival order
    Dev<double> dist;
    Dev<int> index;
    for (int k = 1; k <= 64; ++k)
        for (int n : nset(k))
            for (int p = 1; p <= PATTERNS; ++p) {
                const std::vector<double> d = pattern(p, n, rng);
                std::vector<int> id(n);
                for (int j = 0; j < n; ++j) id[j] = j;
                std::shuffle(id.begin(), id.end(), rng);
                ListCase cs{k, n, p, (int64_t)dist.h.size(), 0};
                std::vector<std::pair<double, int>> cd;
                for (int j = 0; j < n;) {                                  // consecutive ranges of 0..150 candidates, each padded to whole slabs
                    const int len = std::min<int>(n - j, (int)(rng() % 151));
                    for (int t = 0; t < len; ++t) {
                        dist.h.push_back(d[j + t]);
                        index.h.push_back(id[j + t]);
                        cd.push_back({d[j + t], id[j + t]});
                    }
                    for (int t = len; t % 64; ++t) {
                        dist.h.push_back(INF);
                        index.h.push_back(IMAX);
                    }
                    j += len;
                }
                cs.slabs = (int)((dist.h.size() - cs.off) / 64);
                cases.push_back(cs);
                cands.push_back(cd);
            }
    Dev<ListCase> dc(cases.size());
    dc.h = cases;
    Dev<double> od(cases.size() * 64), otau(cases.size());
    Dev<int> oi(cases.size() * 64), otaui(cases.size());
    dc.up(), dist.up(), index.up(), od.up(), oi.up(), otau.up(), otaui.up();
    hipLaunchKernelGGL(keyed_kernel, dim3((unsigned)cases.size()), dim3(64), 0, 0, dc.d, dist.d, index.d, od.d, oi.d, otau.d, otaui.d, INF);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    od.down(), oi.down(), otau.down(), otaui.down();
    for (size_t c = 0; c < cases.size(); ++c) {
        const ListCase& cs = cases[c];
        std::vector<std::pair<double, int>> ref;
        for (const auto& e : cands[c])
            if (!std::isnan(e.first)) ref.push_back(e);
        std::sort(ref.begin(), ref.end());
        ref.resize(std::max<size_t>(ref.size(), cs.k), {INF, IMAX});
        ++rep.cases;
        bool bad = false;
        for (int p = 0; p < cs.k && !bad; ++p)
            if (bits(od.h[c * 64 + p]) != bits(ref[p].first) || oi.h[c * 64 + p] != ref[p].second) {
                bad = true;
                rep.miss(fmt("k %d n %d pattern %d entry %d: (%.17g, %d), expected (%.17g, %d)", cs.k, cs.n, cs.pat, p, od.h[c * 64 + p],
                             oi.h[c * 64 + p], ref[p].first, ref[p].second));
            }
        if (!bad && (bits(otau.h[c]) != bits(ref[cs.k - 1].first) || otaui.h[c] != ref[cs.k - 1].second))
            rep.miss(fmt("k %d n %d pattern %d tau (%.17g, %d), expected (%.17g, %d)", cs.k, cs.n, cs.pat, otau.h[c], otaui.h[c],
                         ref[cs.k - 1].first, ref[cs.k - 1].second));
    }
}

// ======================================================================================================== block collectives
template <int W>
__global__ __launch_bounds__(64 * W) void scan_kernel(const int* __restrict__ v, int* __restrict__ res, int* __restrict__ tot) {
    __shared__ int scr[W];
    const int t = threadIdx.x;
    int total;
    res[t] = block_excl_scan<W>(v[t], scr, &total);
    tot[t] = total;
    res[64 * W + t] = block_excl_scan<W>(v[64 * W + t], scr, &total);      // the same scratch at once: "free again on return"
    tot[64 * W + t] = total;
}

template <int W>
static void scan_sweep(Report& rep, std::mt19937_64& rng) {
    const int T = 64 * W;
    for (int input = 0; input < 5; ++input) {
        Dev<int> v(2 * T), res(2 * T), tot(2 * T);
        for (int call = 0; call < 2; ++call)
            for (int t = 0; t < T; ++t) {
                int x = 0;
                if (input == 1) x = 1;
                if (input == 2) x = (int)(rng() % 1001);
                if (input == 3) x = (t & 63) == 0 ? 1 + t : 0;           // one non-zero at the first lane of each wave
                if (input == 4) x = (t & 63) == 63 ? 1 + t : 0;          // ... at the last
                v.h[call * T + t] = call == 0 ? x : (input == 2 ? (int)(rng() % 1001) : 2 * x);
            }
        v.up(), res.up(), tot.up();
        hipLaunchKernelGGL(scan_kernel<W>, dim3(1), dim3(T), 0, 0, v.d, res.d, tot.d);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        res.down(), tot.down();
        ++rep.cases;
        bool bad = false;
        for (int call = 0; call < 2 && !bad; ++call) {
            int sum = 0;
            for (int t = 0; t < T; ++t) sum += v.h[call * T + t];
            int run = 0;
            for (int t = 0; t < T && !bad; ++t) {
                if (res.h[call * T + t] != run || tot.h[call * T + t] != sum) {
                    bad = true;
                    rep.miss(fmt("block_excl_scan<%d> input %d call %d thread %d: %d total %d, expected %d total %d", W, input, call, t,
                                 res.h[call * T + t], tot.h[call * T + t], run, sum));
                }
                run += v.h[call * T + t];
            }
        }
    }
}

template <int W, typename T, bool MAX>
__global__ __launch_bounds__(64 * W) void extreme_kernel(const T* __restrict__ v, T* __restrict__ res) {
    __shared__ T scr[W];
    const int t = threadIdx.x;
    res[t] = MAX ? block_max<W>(v[t], scr) : block_min<W>(v[t], scr);
    res[64 * W + t] = MAX ? block_max<W>(v[64 * W + t], scr) : block_min<W>(v[64 * W + t], scr);
}

template <typename T>
static bool same(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// kinds: 0 = a finite extreme; 1 (float, double) = an infinite one, the opposite infinity among the other values
template <int W, typename T, bool MAX>
static void extreme_sweep(Report& rep, std::mt19937_64& rng, const char* tname) {
    const int N = 64 * W;
    const int kinds = std::numeric_limits<T>::has_infinity ? 2 : 1;
    const int places[4] = {0, 63, N - 64, N - 1};                        // lanes 0 and 63 of the first and of the last wave
    for (int kind = 0; kind < kinds; ++kind)
        for (int pl = 0; pl < 4; ++pl) {
            Dev<T> v(2 * N), res(2 * N);
            T want[2];
            for (int call = 0; call < 2; ++call) {
                for (int t = 0; t < N; ++t) v.h[call * N + t] = (T)((int)(rng() % 2001) - 1000) / (T)(std::is_integral<T>::value ? 1 : 8);
                T ext = (T)(MAX ? 5000 + call : -5000 - call);
                if (kind == 1) {
                    ext = MAX ? std::numeric_limits<T>::infinity() : -std::numeric_limits<T>::infinity();
                    v.h[call * N + (places[pl] + 17) % N] = -ext;
                }
                v.h[call * N + places[pl]] = ext;
                want[call] = ext;
            }
            v.up(), res.up();
            hipLaunchKernelGGL((extreme_kernel<W, T, MAX>), dim3(1), dim3(N), 0, 0, v.d, res.d);
            HIP_OK(hipGetLastError());
            HIP_OK(hipDeviceSynchronize());
            res.down();
            ++rep.cases;
            for (int t = 0; t < 2 * N; ++t)
                if (!same(res.h[t], want[t / N])) {
                    rep.miss(fmt("block_%s<%d, %s> kind %d extreme at thread %d, call %d thread %d: %.9g, expected %.9g", MAX ? "max" : "min", W,
                                 tname, kind, places[pl], t / N, t % N, (double)res.h[t], (double)want[t / N]));
                    break;
                }
        }
}

template <int W>
static void extremes_of_width(Report& rep, std::mt19937_64& rng) {
    extreme_sweep<W, int, false>(rep, rng, "int");
    extreme_sweep<W, int, true>(rep, rng, "int");
    extreme_sweep<W, float, false>(rep, rng, "float");
    extreme_sweep<W, float, true>(rep, rng, "float");
    extreme_sweep<W, double, false>(rep, rng, "double");
    extreme_sweep<W, double, true>(rep, rng, "double");
}

// fold: 0 wave_min, 1 wave_max, 2 wave_sum, 3 wave_min_uniform, 4 wave_max_uniform; one wave a case (64 cases a launch)
__global__ __launch_bounds__(64) void fold_kernel(int fold, const int* __restrict__ v, int* __restrict__ res) {
    const int x = v[blockIdx.x * 64 + threadIdx.x];
    int r;
    switch (fold) {
    case 0: r = wave_min(x); break;
    case 1: r = wave_max(x); break;
    case 2: r = wave_sum(x); break;
    case 3: r = wave_min_uniform(x); break;
    default: r = wave_max_uniform(x); break;
    }
    res[blockIdx.x * 64 + threadIdx.x] = r;
}

static void fold_sweep(Report& rep, std::mt19937_64& rng) {
    static const char* names[5] = {"wave_min", "wave_max", "wave_sum", "wave_min_uniform", "wave_max_uniform"};
    for (int fold = 0; fold < 5; ++fold) {
        Dev<int> v(64 * 64), res(64 * 64);
        std::vector<int> want(64);
        for (int c = 0; c < 64; ++c) {                                  // case c: the extreme (the one large term) at lane c
            const bool mx = fold == 1 || fold == 4;
            for (int l = 0; l < 64; ++l) v.h[c * 64 + l] = (int)(rng() % 2001) - 1000;
            v.h[c * 64 + c] = mx ? 100000 + c : -100000 - c;
            int w = fold == 2 ? 0 : v.h[c * 64 + c];
            if (fold == 2)
                for (int l = 0; l < 64; ++l) w += v.h[c * 64 + l];
            want[c] = w;
        }
        v.up(), res.up();
        hipLaunchKernelGGL(fold_kernel, dim3(64), dim3(64), 0, 0, fold, v.d, res.d);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        res.down();
        for (int c = 0; c < 64; ++c) {
            ++rep.cases;
            for (int l = 0; l < 64; ++l)
                if (res.h[c * 64 + l] != want[c]) {
                    rep.miss(fmt("%s, the large term at lane %d: lane %d holds %d, expected %d", names[fold], c, l, res.h[c * 64 + l], want[c]));
                    break;
                }
        }
    }
}

// ================================================================================================================ numpy's sum
template <typename T>
static T ref_leaf(const T* a, int n) {
    if (n < 8) {
        T res = 0;
        for (int i = 0; i < n; ++i) res = res + a[i];
        return res;
    }
    T r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + a[i];
    return res;
}
// the recursive definition; leaves: (offset, length) of every leaf, left to right
template <typename T>
static T ref_pairwise(const T* a, int o, int n, std::vector<std::pair<int, int>>& leaves) {
    if (n <= 128) {
        leaves.push_back({o, n});
        return ref_leaf(a + o, n);
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    const T l = ref_pairwise(a, o, n2, leaves);
    const T r = ref_pairwise(a, o + n2, n - n2, leaves);
    return l + r;
}

template <typename T>
static std::vector<T> spread_values(int n, std::mt19937_64& rng) {      // a wide exponent spread: the order of additions shows
    std::vector<T> a(n);
    for (T& x : a) {
        const double m = 1.0 + (double)(rng() % (1 << 20)) / (1 << 20);
        x = (T)std::ldexp((rng() & 1) ? m : -m, (int)(rng() % 41) - 20);
    }
    return a;
}

template <typename T>
__global__ void leaf_kernel(const T* __restrict__ a, T* __restrict__ res, int cases) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < cases) res[n] = np_leaf_sum(a, n);
}

constexpr int NP_STACK = 32;      // the tree of 16384 values is 8 levels deep
template <typename T, int ML>
__global__ __launch_bounds__(64) void pairwise_kernel(const T* __restrict__ a, const int* __restrict__ lens, T* __restrict__ res,
                                                      int* __restrict__ nl_out, int* __restrict__ leaves_out) {
    __shared__ int leaf_o[ML], leaf_l[ML], st_a[NP_STACK], st_b[NP_STACK], nl_s;
    __shared__ T leaf_s[ML], vs[NP_STACK];
    const int len = lens[blockIdx.x];
    if (threadIdx.x == 0) nl_s = np_pairwise_plan<ML>(len, leaf_o, leaf_l, st_a, st_b);
    __syncthreads();
    const int nl = nl_s;
    for (int l = threadIdx.x; l < nl; l += 64) {
        leaf_s[l] = np_leaf_sum(a + leaf_o[l], leaf_l[l]);
        leaves_out[((int64_t)blockIdx.x * ML + l) * 2 + 0] = leaf_o[l];
        leaves_out[((int64_t)blockIdx.x * ML + l) * 2 + 1] = leaf_l[l];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        res[blockIdx.x] = np_pairwise_fold<T, ML>(len, leaf_s, st_a, st_b, vs);
        nl_out[blockIdx.x] = nl;
    }
}

static std::vector<int> pairwise_lengths() {
    std::vector<int> v;
    for (int n = 0; n <= 1100; ++n) v.push_back(n);
    for (int n = 8185; n <= 8200; ++n) v.push_back(n);
    for (int n = 16377; n <= 16384; ++n) v.push_back(n);
    return v;
}

template <typename T>
static void leaf_sweep(Report& rep, std::mt19937_64& rng, const char* tname) {
    Dev<T> a(128), res(129);
    a.h = spread_values<T>(128, rng);
    a.up(), res.up();
    hipLaunchKernelGGL(leaf_kernel<T>, dim3(3), dim3(64), 0, 0, a.d, res.d, 129);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    res.down();
    for (int n = 0; n <= 128; ++n) {
        ++rep.cases;
        const T want = ref_leaf(a.h.data(), n);
        if (!same(res.h[n], want)) rep.miss(fmt("np_leaf_sum<%s> n %d: %.17g, expected %.17g", tname, n, (double)res.h[n], (double)want));
    }
}

// A run of more than ML leaves is outside the plan's contract (its callers bound the length): the plan must then stop at ML leaves,
// the first ML of the definition, and the fold must still end; its value is not compared.
template <typename T, int ML>
static void pairwise_sweep(Report& rep, std::mt19937_64& rng, const char* tname) {
    const std::vector<int> lens = pairwise_lengths();
    Dev<T> a(16384), res(lens.size());
    Dev<int> dl(lens.size()), nl(lens.size()), leaves(lens.size() * ML * 2);
    a.h = spread_values<T>(16384, rng);
    dl.h = lens;
    std::fill(leaves.h.begin(), leaves.h.end(), -7);
    a.up(), res.up(), dl.up(), nl.up(), leaves.up();
    hipLaunchKernelGGL((pairwise_kernel<T, ML>), dim3((unsigned)lens.size()), dim3(64), 0, 0, a.d, dl.d, res.d, nl.d, leaves.d);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    res.down(), nl.down(), leaves.down();
    for (size_t c = 0; c < lens.size(); ++c) {
        ++rep.cases;
        std::vector<std::pair<int, int>> rl;
        const T want = ref_pairwise(a.h.data(), 0, lens[c], rl);
        const int rn = std::min<int>((int)rl.size(), ML);
        if (nl.h[c] != rn) {
            rep.miss(fmt("np_pairwise_plan<%d> (%s) length %d: %d leaves, expected %d", ML, tname, lens[c], nl.h[c], rn));
            continue;
        }
        bool bad = false;
        for (int l = 0; l < rn && !bad; ++l)
            if (leaves.h[(c * ML + l) * 2] != rl[l].first || leaves.h[(c * ML + l) * 2 + 1] != rl[l].second) {
                bad = true;
                rep.miss(fmt("np_pairwise_plan<%d> (%s) length %d leaf %d: (%d, %d), expected (%d, %d)", ML, tname, lens[c], l,
                             leaves.h[(c * ML + l) * 2], leaves.h[(c * ML + l) * 2 + 1], rl[l].first, rl[l].second));
            }
        if (!bad && (int)rl.size() <= ML && !same(res.h[c], want))
            rep.miss(fmt("np_pairwise_fold<%s, %d> length %d: %.17g, expected %.17g", tname, ML, lens[c], (double)res.h[c], (double)want));
    }
}

// the guard case, entirely in bounds: MAX_LEAVES = 4 against the 8 leaves of 1000 values, every array between canaries
constexpr int CANARY = 0x5ca1ab1e;
struct GuardArrays {
    int c0, leaf_o[4], c1, leaf_l[4], c2, st_a[NP_STACK], c3, st_b[NP_STACK], c4;
    double c5, leaf_s[4], c6, vs[NP_STACK], c7;
    int nl, done;
};
__global__ void guard_kernel(GuardArrays* g) {
    if (threadIdx.x != 0) return;
    g->nl = np_pairwise_plan<4>(1000, g->leaf_o, g->leaf_l, g->st_a, g->st_b);
    g->leaf_s[0] = np_pairwise_fold<double, 4>(1000, g->leaf_s, g->st_a, g->st_b, g->vs);
    g->done = 1;
}
static void guard_case(Report& rep) {
    Dev<GuardArrays> g(1);
    std::memset(&g.h[0], 0, sizeof(GuardArrays));
    GuardArrays& a = g.h[0];
    a.c0 = a.c1 = a.c2 = a.c3 = a.c4 = CANARY;
    a.c5 = a.c6 = a.c7 = 12345.0;
    g.up();
    hipLaunchKernelGGL(guard_kernel, dim3(1), dim3(64), 0, 0, g.d);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    g.down();
    ++rep.cases;
    const bool canaries = a.c0 == CANARY && a.c1 == CANARY && a.c2 == CANARY && a.c3 == CANARY && a.c4 == CANARY && a.c5 == 12345.0 &&
                          a.c6 == 12345.0 && a.c7 == 12345.0;
    if (a.nl != 4 || !canaries || a.done != 1)
        rep.miss(fmt("guard case MAX_LEAVES 4, length 1000: plan returned %d (expected 4), canaries %s, fold %s", a.nl,
                     canaries ? "intact" : "DAMAGED", a.done == 1 ? "ended" : "did not end"));
}

int main() {
    int devices = 0;
    HIP_OK(hipGetDeviceCount(&devices));
    if (devices < 1) {
        std::printf("no GPU\n");
        return 2;
    }
    std::mt19937_64 rng(20240607);
    bool ok = true;

    Report arrival{"arrival-order list"};
    arrival_sweep<false>(arrival, rng);
    arrival_sweep<true>(arrival, rng);
    ok &= arrival.print();

    Report keyed{"keyed list"};
    keyed_sweep(keyed, rng);
    ok &= keyed.print();

    Report block{"block collectives"};
    scan_sweep<1>(block, rng), scan_sweep<2>(block, rng), scan_sweep<4>(block, rng), scan_sweep<8>(block, rng), scan_sweep<16>(block, rng);
    extremes_of_width<1>(block, rng), extremes_of_width<2>(block, rng), extremes_of_width<4>(block, rng), extremes_of_width<8>(block, rng),
        extremes_of_width<16>(block, rng);
    fold_sweep(block, rng);
    ok &= block.print();

    Report np{"numpy sum"};
    leaf_sweep<float>(np, rng, "float"), leaf_sweep<double>(np, rng, "double");
    pairwise_sweep<float, 64>(np, rng, "float"), pairwise_sweep<float, 512>(np, rng, "float");
    pairwise_sweep<double, 64>(np, rng, "double"), pairwise_sweep<double, 512>(np, rng, "double");
    guard_case(np);
    ok &= np.print();
    return ok ? 0 : 1;
}
