// The second half of every split-K gradient (csrc/dcn_bwd.hip, csrc/heads_bwd.hip): out[i] = the sum over S partial slices of n floats,
// added in split order from 0.f -- a fixed order, so the result is bit-identical from run to run.
// TAPS_LAST: the partials are [tap][rows][cols] as the matrix-core kernels leave them (9 taps), out is the reference's [rows][cols][tap].
#pragma once
#include "common.h"

template <bool TAPS_LAST>
__global__ void h3d_split_sum_kernel(const float *__restrict__ part, float *__restrict__ out, size_t n, int S, int rows, int cols)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
    for (int s = 0; s < S; ++s) v += part[(size_t)s * n + i];
    if constexpr (TAPS_LAST) {
        const int c = (int)(i % cols), r = (int)((i / cols) % rows), t = (int)(i / ((size_t)cols * rows));
        out[((size_t)r * cols + c) * 9 + t] = v;
    } else {
        out[i] = v;
    }
}

// rows > 0: TAPS_LAST, n = 9 * rows * cols
static inline int h3d_split_sum(const float *part, float *out, size_t n, int S, hipStream_t st, int rows = 0, int cols = 0)
{
    const dim3 grid((unsigned)((n + 255) / 256));
    if (rows) return h3d_launch({"h3d_split_sum_kernel", true}, h3d_split_sum_kernel<true>, grid, dim3(256), 0, st, part, out, n, S, rows, cols);
    return h3d_launch({"h3d_split_sum_kernel", false}, h3d_split_sum_kernel<false>, grid, dim3(256), 0, st, part, out, n, S, rows, cols);
}
