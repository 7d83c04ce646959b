// What a wavefront or a work group of the geometry kernels does as a unit: cross-lane moves, wave folds, the block scan and
// extremes, the sorted k-list spread over a wave's lanes (WaveTopK), the f64 squared distance in the definition's order, and
// numpy's pairwise sum.  Every piece carries an exactness contract (a tie rule, or numpy's summation order) that its users assert
// bit for bit.  No kernels, no host code.  Work groups are one-dimensional: a lane is threadIdx.x & 63, a wave threadIdx.x >> 6.
#pragma once
#include "common.h"

namespace sapcu {

// ------------------------------------------------------------------------------------------------------ cross-lane moves
// Cross-lane moves without the LDS crossbar: ds_bpermute (what __shfl compiles to) has ~100 cycles of
// latency and an insertion chains ~15 of them; a wave-uniform source lane is a v_readlane, and "take the
// value of lane-1" is one DPP move (wave_shr:1, lane 0 keeps its own).
__device__ __forceinline__ int wave_shr1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ double wave_shr1(double v) {
    return __hiloint2double(wave_shr1(__double2hiint(v)), wave_shr1(__double2loint(v)));
}
__device__ __forceinline__ double wave_readlane(double v, int lane_uniform) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane_uniform),
                            __builtin_amdgcn_readlane(__double2loint(v), lane_uniform));
}

// ------------------------------------------------------------------------------------------------------------ wave folds
__device__ __forceinline__ int lane_min(int a, int b) { return min(a, b); }
__device__ __forceinline__ float lane_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double lane_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ int lane_max(int a, int b) { return max(a, b); }
__device__ __forceinline__ float lane_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double lane_max(double a, double b) { return fmax(a, b); }

// the 64-lane butterfly (int, float, double): every lane ends with the result
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = lane_min(v, __shfl_xor(v, o));
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = lane_max(v, __shfl_xor(v, o));
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the result in a scalar register, for loop bounds
__device__ __forceinline__ int wave_min_uniform(int v) { return __builtin_amdgcn_readfirstlane(wave_min(v)); }
__device__ __forceinline__ int wave_max_uniform(int v) { return __builtin_amdgcn_readfirstlane(wave_max(v)); }

// ----------------------------------------------------------------------------------------------------- block collectives
// exclusive scan of one int per thread over a work group of WAVES wavefronts, the sum of all in *total; scr: WAVES ints, free
// again on return (two barriers)
template <int WAVES>
__device__ __forceinline__ int block_excl_scan(int v, int* scr, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) scr[wave] = x;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int t = scr[w];
        if (w < wave) off += t;
        tot += t;
    }
    __syncthreads();
    *total = tot;
    return off + x - v;
}

// the minimum / maximum of one value per thread over the work group, in every thread; scr: WAVES values, free again on return
template <int WAVES, typename T>
__device__ __forceinline__ T block_min(T v, T* scr) {
    v = wave_min(v);
    if ((threadIdx.x & 63) == 0) scr[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = scr[0];
    for (int w = 1; w < WAVES; ++w) r = lane_min(r, scr[w]);
    __syncthreads();
    return r;
}
template <int WAVES, typename T>
__device__ __forceinline__ T block_max(T v, T* scr) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) scr[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = scr[0];
    for (int w = 1; w < WAVES; ++w) r = lane_max(r, scr[w]);
    __syncthreads();
    return r;
}

// -------------------------------------------------------------------------------------------------------------- distance
// the f64 squared distance in the definition's order, ((dx*dx) + (dy*dy)) + (dz*dz) with separately rounded operations: the reduced
// distance sklearn accumulates — no FMA contraction, or neighbour indices would differ in the last ulp
__device__ __forceinline__ double dist2_rn(double qx, double qy, double qz, double px, double py, double pz) {
    const double dx = __dsub_rn(qx, px);
    const double dy = __dsub_rn(qy, py);
    const double dz = __dsub_rn(qz, pz);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// ------------------------------------------------------------------------------------------------ the lane-spread k-list
// The k nearest candidates of one wavefront's query as a sorted list spread over the lanes: entry p in lane p % 64, slot p / 64
// (TWO: the second slot, for 64 < k <= 128; the one-slot insertion is a third shorter).  An insertion is one ballot + popcount
// (the position) and one lane shift — no LDS, no divergence beyond the wave-uniform candidate loop.  The result is the ascending
// (distance, index) order of a stable sort; how a candidate is ordered against the list is the second choice:
//   * arrival order (KEYED false): strict '<' against the k-th distance, position = the number of entries <= the candidate.
//     Correct ONLY when candidates are offered in ascending index — an entry at the candidate's distance then has a lower index.
//     offer() takes the index of lane 0's candidate, lane l holds the candidate of index + l.  No index compare anywhere;
//   * keyed: the lexicographic (distance, index) compare, the k-th entry's index carried along; any arrival order.  offer() takes
//     each lane's own index.
// (knn_outer.hip keeps the arrival-order insertion written out, for its speed there: a change of the rule belongs in both.)
// A lane without a candidate offers distance +inf (keyed: index INT_MAX).
// NON-FINITE CANDIDATES (arrival order; the rule of include/sapcu.h and DESIGN section 2): a candidate whose squared distance is
// NaN or +inf is not a candidate.  The list holds the finite ones in (distance, index) order, then empty entries (+inf, NONE); a
// kernel writes an empty entry as index -1, distance +inf and a NaN row, and loads nothing through it.  offer() keeps the rule for
// nothing (NaN < tau and +inf < tau are false); first_slab() turns such a lane into a lane without a candidate before its
// network, whose compare is no order once a NaN is in it.  The keyed list orders whatever is not NaN: there a +inf distance with
// a real index stands behind the finite entries and in front of the empty ones; its user (knn_grid.hip) never offers one, the
// grid is not built over non-finite coordinates.
template <bool TWO, bool KEYED = false>
struct WaveTopK {
    static_assert(!(TWO && KEYED), "the keyed list has no user beyond k = 64");
    static constexpr int SLOTS = TWO ? 2 : 1;
    static constexpr int NONE = KEYED ? 0x7fffffff : -1;       // index of an empty entry (keyed: it has to order last)
    double d[SLOTS];       // this lane's entries (squared distance, point index)
    int i[SLOTS];
    double tau;            // entry k-1 (wave-uniform)
    int tau_i;             // keyed only
    int k;

    __device__ __forceinline__ explicit WaveTopK(int k_) : tau(__builtin_huge_val()), tau_i(0x7fffffff), k(k_) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            d[s] = __builtin_huge_val();
            i[s] = NONE;
        }
    }

    // the candidate (cd, ci) enters: it orders before entry k-1
    __device__ __forceinline__ bool enters(double cd, int ci) const {
        if constexpr (KEYED) return cd < tau || (cd == tau && ci < tau_i);
        else return cd < tau;
    }
    // the entry (ed, ei) stays in front of the candidate (cd, ci)
    static __device__ __forceinline__ bool stays(double ed, int ei, double cd, int ci) {
        if constexpr (KEYED) return ed < cd || (ed == cd && ei < ci);
        else return ed <= cd;
    }
    __device__ __forceinline__ void read_tau() {
        const int kl = (k - 1) & 63;
        if constexpr (TWO) tau = k <= 64 ? wave_readlane(d[0], kl) : wave_readlane(d[1], kl);
        else tau = wave_readlane(d[0], kl);
        if constexpr (KEYED) tau_i = __builtin_amdgcn_readlane(i[0], kl);
    }

    // The first 64 candidates into the EMPTY list without 64 serial insertions (every one of them passes an empty list's threshold):
    // a bitonic network on (distance, index) keys sorts them across the lanes.  si: this lane's index, INT_MAX without a candidate.
    __device__ __forceinline__ void first_slab(double cd, int si) {
        const int lane = threadIdx.x & 63;
        if (!(cd < __builtin_huge_val())) {       // NaN or +inf: no candidate (once per query; the network needs a total order)
            cd = __builtin_huge_val();
            si = 0x7fffffff;
        }
#pragma unroll
        for (int kb = 2; kb <= 64; kb <<= 1) {
#pragma unroll
            for (int jb = kb >> 1; jb > 0; jb >>= 1) {
                const double od = __shfl_xor(cd, jb);
                const int oi = __shfl_xor(si, jb);
                const bool own_less = cd < od || (cd == od && si < oi);
                const bool want_less = ((lane & jb) == 0) == ((lane & kb) == 0);     // lower lane of an ascending pair
                if (own_less != want_less) {
                    cd = od;
                    si = oi;
                }
            }
        }
        d[0] = cd;
        i[0] = si == 0x7fffffff ? NONE : si;
        if (!TWO || k <= 64) read_tau();       // k <= 64: the list is full (+inf while fewer than k candidates); else entry k-1 is empty
    }

    // one candidate per lane against the list.  (It works on a copy: the optimiser then sees registers, not stores through `this`,
    // and the slot update becomes selects instead of branches on the exec mask.)
    __device__ __forceinline__ void offer(double cand, int idx) {
        WaveTopK L = *this;
        const int lane = threadIdx.x & 63;
        unsigned long long mask = __ballot(L.enters(cand, idx));      // (arrival order ignores the index)
        while (mask) {
            const int src = __builtin_ctzll(mask);
            mask &= mask - 1;
            const double cd = wave_readlane(cand, src);
            const int ci = KEYED ? __builtin_amdgcn_readlane(idx, src) : idx + src;
            if (!L.enters(cd, ci)) continue;                          // an earlier candidate of this slab has lowered the threshold
            int pos = __popcll(__ballot(stays(L.d[0], L.i[0], cd, ci)));
            if constexpr (TWO) pos += __popcll(__ballot(stays(L.d[1], L.i[1], cd, ci)));
            // entries at positions >= pos move up by one, the last drops out
            const double u0d = wave_shr1(L.d[0]);
            const int u0i = wave_shr1(L.i[0]);
            double l63d = 0.0;                                      // entry 63 moves into the second slot's lane 0
            int l63i = 0;
            if constexpr (TWO) {
                l63d = wave_readlane(L.d[0], 63);
                l63i = __builtin_amdgcn_readlane(L.i[0], 63);
            }
            if (lane == pos) {
                L.d[0] = cd;
                L.i[0] = ci;
            } else if (lane > pos) {
                L.d[0] = u0d;
                L.i[0] = u0i;
            }
            if constexpr (TWO) {
                double u1d = wave_shr1(L.d[1]);
                int u1i = wave_shr1(L.i[1]);
                if (lane == 0) {
                    u1d = l63d;
                    u1i = l63i;
                }
                if (lane + 64 == pos) {
                    L.d[1] = cd;
                    L.i[1] = ci;
                } else if (lane + 64 > pos) {
                    L.d[1] = u1d;
                    L.i[1] = u1i;
                }
            }
            L.read_tau();
        }
        *this = L;
    }
};

// ----------------------------------------------------------------------------------------------------- numpy's pairwise sum
// numpy adds a contiguous run of n values as a tree: a run of more than 128 splits at n/2 rounded down to a multiple of 8, a leaf
// (n <= 128) is summed with eight accumulators.  A kernel gives every leaf to a lane: one lane lays the leaves out
// (np_pairwise_plan), the lanes sum them (np_leaf_sum), one lane folds the sums back up the tree (np_pairwise_fold); the LDS arrays
// are the kernel's.  f32 and f64.
__device__ __forceinline__ float np_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double np_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ int np_split(int l) {
    const int n2 = l / 2;
    return n2 - n2 % 8;
}

// the leaf: 8 accumulators over the first n - n%8 values, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the rest added in order;
// fewer than 8: a plain sum from 0
template <typename T>
__device__ __forceinline__ T np_leaf_sum(const T* __restrict__ a, int n) {
    if (n < 8) {
        T res = 0;
        for (int i = 0; i < n; ++i) res = np_add(res, a[i]);
        return res;
    }
    T r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 = np_add(r0, a[i + 0]);
        r1 = np_add(r1, a[i + 1]);
        r2 = np_add(r2, a[i + 2]);
        r3 = np_add(r3, a[i + 3]);
        r4 = np_add(r4, a[i + 4]);
        r5 = np_add(r5, a[i + 5]);
        r6 = np_add(r6, a[i + 6]);
        r7 = np_add(r7, a[i + 7]);
    }
    T res = np_add(np_add(np_add(r0, r1), np_add(r2, r3)), np_add(np_add(r4, r5), np_add(r6, r7)));
    for (; i < n; ++i) res = np_add(res, a[i]);
    return res;
}

// ONE lane: the leaves of a run of len values, left to right, into leaf_o / leaf_l (offset, length; at most MAX_LEAVES); returns
// their number.  st_o / st_l: a stack as deep as the tree.
template <int MAX_LEAVES>
__device__ __forceinline__ int np_pairwise_plan(int len, int* leaf_o, int* leaf_l, int* st_o, int* st_l) {
    int sp = 0, nl = 0;
    st_o[sp] = 0;
    st_l[sp] = len;
    ++sp;
    while (sp > 0 && nl < MAX_LEAVES) {
        --sp;
        const int o = st_o[sp], l = st_l[sp];
        if (l <= 128) {
            leaf_o[nl] = o;
            leaf_l[nl] = l;
            ++nl;
        } else {
            const int n2 = np_split(l);
            st_o[sp] = o + n2;                 // the right half pushed first: the left one is popped (and numbered) first
            st_l[sp] = l - n2;
            ++sp;
            st_o[sp] = o;
            st_l[sp] = n2;
            ++sp;
        }
    }
    return nl;
}

// ONE lane: the leaf sums leaf_s (in the plan's order) folded back up the tree of a run of len values.  Post-order: a node is
// pushed unexpanded (e = 0); popped, an inner node goes back expanded (e = 1) under its two halves.  st_l / st_e / vs: stacks as
// deep as the tree.
template <typename T, int MAX_LEAVES>
__device__ __forceinline__ T np_pairwise_fold(int len, const T* leaf_s, int* st_l, int* st_e, T* vs) {
    int sp = 0, vsp = 0, leaf = 0;
    st_l[sp] = len;
    st_e[sp] = 0;
    ++sp;
    while (sp > 0) {
        --sp;
        const int l = st_l[sp];
        if (st_e[sp]) {
            const T rhs = vs[--vsp];
            const T lhs = vs[--vsp];
            vs[vsp++] = np_add(lhs, rhs);
        } else if (l <= 128) {
            vs[vsp++] = leaf_s[leaf < MAX_LEAVES ? leaf : MAX_LEAVES - 1];
            ++leaf;
        } else {
            const int n2 = np_split(l);
            st_l[sp] = l;
            st_e[sp] = 1;
            ++sp;
            st_l[sp] = l - n2;
            st_e[sp] = 0;
            ++sp;
            st_l[sp] = n2;
            st_e[sp] = 0;
            ++sp;
        }
    }
    return vs[0];
}

}  // namespace sapcu
