// The device side of a graphed training step's skip decision (include/sapcu_train_step.h): when *flag is set, every tensor of a
// device table becomes a copy of its source (the shadow taken before optimizer.step()) or, with a NULL source, zero bytes (a
// gradient).  One launch, grid (blocks_per_tensor, count); with the flag clear every workgroup leaves after one uniform load.
//
// A tensor is walked in 16-byte chunks from the first 16-byte boundary of ITS destination; the up to three 4-byte words before
// that boundary and after the last whole chunk are written by the first lanes of the tensor's first workgroup.  The source of a
// chunk is read as one 16-byte load when it is aligned like the destination and as four words when it is not.
//
// Also here: zero_count (common.h), how the training ops zero a bad_count slot on a stream that is being captured.
#include "common.h"
#include "../../include/sapcu_train_step.h"

namespace sapcu {

constexpr int MS_THREADS = 256;

__global__ __launch_bounds__(MS_THREADS) void multi_select_kernel(const int* __restrict__ flag, void* const* __restrict__ dst,
                                                                  const void* const* __restrict__ src,
                                                                  const int64_t* __restrict__ nbytes) {
    if (*flag == 0) return;
    const int t = blockIdx.y;
    char* d = (char*)dst[t];
    const char* s = src ? (const char*)src[t] : nullptr;
    const int64_t n = nbytes[t] & ~(int64_t)3;
    if (d == nullptr || n <= 0) return;
    int64_t head = (int64_t)((16 - ((uintptr_t)d & 15)) & 15);           // bytes up to the first 16-byte boundary: 0, 4, 8 or 12
    if (head > n) head = n;
    const int64_t chunks = (n - head) >> 4;
    const int64_t tail0 = head + (chunks << 4);                           // first byte after the last whole chunk
    if (blockIdx.x == 0) {
        const int64_t hw = head >> 2, tw = (n - tail0) >> 2;              // <= 3 words each
        if ((int64_t)threadIdx.x < hw) {
            const int64_t o = (int64_t)threadIdx.x << 2;
            *(uint32_t*)(d + o) = s ? *(const uint32_t*)(s + o) : 0u;
        } else if ((int64_t)threadIdx.x - hw < tw) {
            const int64_t o = tail0 + (((int64_t)threadIdx.x - hw) << 2);
            *(uint32_t*)(d + o) = s ? *(const uint32_t*)(s + o) : 0u;
        }
    }
    const bool wide = s != nullptr && (((uintptr_t)(s + head)) & 15) == 0;
    const int64_t stride = (int64_t)gridDim.x * MS_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; i < chunks; i += stride) {
        const int64_t o = head + (i << 4);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (wide) {
            v = *(const uint4*)(s + o);
        } else if (s) {
            const uint32_t* w = (const uint32_t*)(s + o);
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *(uint4*)(d + o) = v;
    }
}

__global__ void zero_count_kernel(int* __restrict__ p) {
    if (threadIdx.x == 0) *p = 0;
}

int zero_count(int* p, hipStream_t st) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &capturing) != hipSuccess) {
        (void)hipGetLastError();                                          // a refused query must not stick to the next launch check
    } else if (capturing == hipStreamCaptureStatusActive) {
        hipLaunchKernelGGL(zero_count_kernel, dim3(1), dim3(64), 0, st, p);
        SAPCU_CHECK_LAUNCH();
        return SAPCU_OK;
    }
    SAPCU_CHECK_HIP(hipMemsetAsync(p, 0, sizeof(int), st));
    return SAPCU_OK;
}

}  // namespace sapcu

using namespace sapcu;

int sapcu_multi_select(const int* flag, void* const* dst, const void* const* src, const int64_t* nbytes, int count,
                       int blocks_per_tensor, void* stream) {
    SAPCU_CHECK_ARG(flag && dst && nbytes, "multi_select: null flag, dst or nbytes table");
    SAPCU_CHECK_ARG(count >= 1 && count <= 65535, "multi_select: count %d outside [1, 65535]", count);
    SAPCU_CHECK_ARG(blocks_per_tensor >= 1 && blocks_per_tensor <= 65535, "multi_select: blocks_per_tensor %d outside [1, 65535]",
                    blocks_per_tensor);
    hipLaunchKernelGGL(multi_select_kernel, dim3((unsigned)blocks_per_tensor, (unsigned)count), dim3(MS_THREADS), 0, (hipStream_t)stream,
                       flag, dst, src, nbytes);
    SAPCU_CHECK_LAUNCH();
    return SAPCU_OK;
}
