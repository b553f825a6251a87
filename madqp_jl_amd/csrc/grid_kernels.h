// The __global__ form of the kernel bodies in vec_kernels.inc and kkt_kernels.inc, and of the kernels written beside
// them (vec_kernels.hip, kkt.hip, dist.hip): TPB threads per block, a grid-stride loop over at most MADQP_MAX_BLOCKS
// blocks, one partial sum per block.  (batch_wg.inc defines the workgroup-stride form of the same names itself.)
#pragma once
#include <algorithm>

#include "common.h"

#define TPB 256
#define MADQP_MAX_BLOCKS 1024
#define MQ_KERNEL __global__ __launch_bounds__(TPB) void
#define MQ_BLOCK blockIdx.x
#define GRID_STRIDE(i, len) \
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < (len); i += (int64_t)gridDim.x * TPB)

static inline int grid_for(int64_t len) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((len + TPB - 1) / TPB, MADQP_MAX_BLOCKS));
}

// LAUNCH: kern over len entries on the stream of `ctx` (a madqp_ctx* in scope); returns from the caller if the launch fails
#define LAUNCH(kern, len, ...)                                                             \
    do {                                                                                        \
        hipLaunchKernelGGL(kern, dim3(grid_for(len)), dim3(TPB), 0, ctx->stream, __VA_ARGS__);  \
        LAUNCH_CHECK(ctx);                                                                      \
    } while (0)
