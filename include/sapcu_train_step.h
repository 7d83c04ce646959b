/*
 * sapcu_train_step.h — what a training step captured as a HIP graph needs beside the training ops: a host decision moved onto the
 * device.  sapcu_amd/fd_trainer.py (GraphedTrainStep) decides on the device whether a batch is skipped (non-finite loss or gradient,
 * a neighbour index outside its patch) and, when it is, puts the parameters and the optimiser's state back from shadow copies and
 * zero-fills the gradients — in ONE launch over a table of tensors instead of a `where` / `masked_fill_` node per tensor.
 *
 * Part of libsapcu_hip.so; the conventions and status codes of sapcu.h apply (0 on success, sapcu_last_error() for the text).
 * SAPCU_ABI_VERSION is unchanged: this entry point is an addition.  The call neither synchronises nor allocates nor copies to the
 * host, and it is one kernel node on `stream`: it can be captured.
 *
 * Memory contract:
 *   - flag, dst, src and nbytes are DEVICE arrays: one int, and `count` pointers / pointers / byte counts.  They are read by the
 *     kernel when it runs, not by the call: a captured launch sees whatever the tables hold at replay;
 *   - *flag == 0: nothing is written.  *flag != 0: for every i < count the nbytes[i] bytes at dst[i] become a copy of the bytes at
 *     src[i], or zero bytes when src[i] is NULL (src itself may be NULL: every entry is zero-filled); nothing else is written;
 *   - dst[i] and src[i] need 4-byte alignment only and nbytes[i] % 4 == 0 (trailing 1-3 bytes would be left alone); nbytes[i] == 0
 *     and a NULL dst[i] are legal entries that write nothing; a tensor and its source must not overlap, two dst may not either;
 *   - the grid is (blocks_per_tensor, count): every tensor is walked by blocks_per_tensor workgroups of 256 lanes in 16-byte chunks
 *     (vector stores; up to three 4-byte words before the first and after the last aligned chunk), whatever its size;
 *   - count < 1, blocks_per_tensor < 1 or > 65535, count > 65535, or a NULL flag, dst or nbytes return SAPCU_ERR_ARG before
 *     anything is launched.
 * No atomics, no LDS, no scratch; the result does not depend on blocks_per_tensor.
 */
#ifndef SAPCU_TRAIN_STEP_H
#define SAPCU_TRAIN_STEP_H

#include "sapcu.h"

#ifdef __cplusplus
extern "C" {
#endif

int sapcu_multi_select(const int* flag, void* const* dst, const void* const* src, const int64_t* nbytes, int count,
                       int blocks_per_tensor, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAPCU_TRAIN_STEP_H */
