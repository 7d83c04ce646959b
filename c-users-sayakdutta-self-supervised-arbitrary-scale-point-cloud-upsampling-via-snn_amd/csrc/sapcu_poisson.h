/*
 * sapcu_poisson.h — Poisson-disk selection: the blue-noise subset of a cloud whose points keep a distance r from each other, and the
 * exact-count subsample that a bisection on r gives (sapcu_amd/poisson.py; the kind of cloud the PU-GAN / PU1K protocol trains and
 * evaluates on, "poisson_256" / "poisson_1024").  csrc/poisson.hip; tests/poisson_ref.py states the definition in numpy.
 *
 * Part of libsapcu_hip.so; the conventions and status codes of include/sapcu.h apply (device pointers, the caller owns every
 * buffer, 0 on success, sapcu_last_error() for the text).  SAPCU_ABI_VERSION is unchanged: these entry points are additions.  The
 * header lies beside its source, and its table in sapcu_amd/_lib.py beside TABLES, as csrc/sapcu_geodesic.h does and for its reason.
 *
 * Definition.  All arithmetic is f32, every operation rounded once (the library is built with -ffp-contract=off).
 *   select(P, r): P f32 [C,3], the row index is the priority (row 0 first); r2 = r * r; for i = 0 .. C-1
 *       keep[i]  <=>  no j < i has keep[j] and d2(i,j) < r2,    d2 = (dx*dx + dy*dy) + dz*dz,  dx = P[i,0] - P[j,0], dy, dz likewise.
 *     The comparison is strict: a pair at exactly r keeps both, r = 0 keeps every row (duplicates included), any r > 0 drops the
 *     later of two equal rows.  count = sum(keep).
 *   subsample(P, n, steps), 1 <= n <= C: e = max - min per axis, hi = sqrtf((ex*ex + ey*ey) + ez*ez), lo = 0; `steps` times
 *       mid = 0.5f * (lo + hi);  count(select(P, mid)) >= n ? lo = mid : hi = mid;
 *     then r = lo, keep = select(P, r), idx = the first n kept rows in ascending order.  count(select(P, 0)) = C >= n, so count >= n.
 *
 * How it runs.  The parallel form of select gives the same set: a candidate is accepted once every lower row within r is rejected,
 * rejected once one of them is accepted, undecided until then.  A decision depends only on final decisions of lower rows, and every
 * round decides at least the lowest undecided row, so at most C rounds.  Both paths run SYNCHRONOUS rounds — a round reads the
 * states the round before left — so `rounds` is a property of the input too (tests/poisson_ref.py select_rounds), not of scheduling.
 * Which path runs is chosen by C alone:
 *   - resident, C <= SAPCU_PD_RESIDENT_MAX: one work group of 1024 threads per batch entry.  Per candidate one 16-byte slot
 *     {x, y, z, state | cell | row} in LDS, the slots ordered by (cell, row) by a bitonic sort, and the cell table (4 bytes per
 *     cell, at most SAPCU_PD_RESIDENT_CELLS cells): 16 C + 16.75 KiB, 144.75 KiB at C = 8192; the coordinates sit in LDS, so a
 *     candidate costs its reader one LDS read.  Rounds are separated by work-group barriers, the whole bisection (the grid is
 *     rebuilt for every radius) runs inside the one launch: no read-back, no atomics outside LDS, no workspace use, capturable
 *     into a graph.
 *   - grid, larger C (and sapcu_internal_poisson_select_grid at any C): entries one after another; per radius the cell sort of
 *     knn_grid.h on the coordinates widened to f64, then one launch per round; the launches are enqueued in chunks of
 *     SAPCU_PD_GRID_CHUNK rounds and the per-round undecided counts are read back after each chunk, one synchronisation per chunk;
 *     the bisection runs on the host side of the entry point, one more synchronisation per step.  NOT capturable into a graph.
 *
 * The grid is only an accelerator; the distance test is the f32 expression above on both paths.  The cell edge h is at least
 *       cover(r2) = sqrt((double)r2 + 2^-140) * (1 + 2^-20)              (f64; r2 is the f32 product the test compares against)
 *   and is enlarged (times 1.125 until it fits) so that the cell count stays within its cap.  Derivation of the margin: when
 *   d2 < r2 holds in f32, each of fl(dx*dx) <= d2 up to the two additions' roundings, and dx = fl(x_i - x_j); four roundings of
 *   2^-24 relative, plus 2^-149 absolute each where a product or sum is subnormal, bound the true |x_i - x_j| by
 *   sqrt(r2 (1 + 2^-21) + 2^-146) < cover(r2) / (1 + 2^-21).  The cell of x is floor((x - o) / h) in f64, clamped to the grid:
 *   x - o is exact or rounded at 2^-53 relative, the quotient likewise, and the quotient is below 2^24 cells, so two computed
 *   quotients whose true values differ by less than 1 - 2^-22 differ by less than 1 and their floors by at most 1 (clamping is
 *   monotone).  Hence every conflict of a point lies in the 27 cells around its own.
 *
 * Memory contract (checked under guard bands by tests/test_gpu_poisson.py):
 *   - points [b,C,3] f32 and radius [b] f32 are only read; keep u8 [b,C] (0 / 1), idx i32 [b,n], radius_out f32 [b], count i32 [b]
 *     and rounds i32 [b] (select: the rounds of the one selection; subsample: summed over its steps + 1 selections) are written in
 *     full, nothing else; nothing is written beyond the sizer's bytes; the workspace needs NO initialisation, 8-byte alignment;
 *   - an entry whose bounding box is not finite (a NaN or infinite coordinate) keeps nothing: keep = 0, idx = -1, count = 0,
 *     rounds = 0, radius_out = 0; the other entries are unaffected;
 *   - b == 0 launches and writes nothing;
 *   - refused before anything is launched: SAPCU_ERR_ARG for a NULL pointer, b outside [0, SAPCU_PD_MAX_B], C outside
 *     [1, SAPCU_PD_MAX_C], n < 1, n > C, steps outside [0, SAPCU_PD_MAX_STEPS], a misaligned workspace; SAPCU_ERR_WORKSPACE for
 *     fewer bytes than the sizer's.  A radius that is negative or NaN selects as r2 = r * r says (NaN keeps everything); the
 *     Python layer refuses both.
 */
#ifndef SAPCU_POISSON_H
#define SAPCU_POISSON_H

#include "../../include/sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAPCU_PD_RESIDENT_MAX 8192
#define SAPCU_PD_RESIDENT_CELLS 4096
#define SAPCU_PD_GRID_CHUNK 8
#define SAPCU_PD_MAX_C (1 << 24)
#define SAPCU_PD_MAX_B 65535
#define SAPCU_PD_MAX_STEPS 64

/* Bytes of workspace for either entry point (one layout: the grid path's); -1 for sizes the calls would refuse. */
int64_t sapcu_poisson_workspace_bytes(int64_t b, int64_t C);

int sapcu_poisson_select_f32(const float* points, int64_t b, int64_t C, const float* radius, uint8_t* keep_out, int32_t* count_out,
                             int32_t* rounds_out, void* workspace, int64_t workspace_bytes, void* stream);

int sapcu_poisson_subsample_f32(const float* points, int64_t b, int64_t C, int64_t n, int steps, int32_t* idx_out, float* radius_out,
                                int32_t* count_out, int32_t* rounds_out, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_POISSON_H */
