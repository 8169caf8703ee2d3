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

// The same blocked sum formed inside a kernel, by every workgroup that needs the total (csrc/bn.hip: a second stage that also consumes
// it): S slots of n floats, G = ceil(S / 64) <= 64 chains; chain g adds the slots g, g + G, g + 2G, ... in ascending order from 0.f (at
// most 64 terms), then the G chain sums are added in order.  The workgroup is `lanes` x `workers` threads; a lane owns the four floats at
// column `col` of every slot (`active` = false: zeros), the workers share the chains.  s_chain holds 64 * lanes entries, s_tot `lanes`.
// Every thread of the workgroup calls it; every worker of a lane gets the lane's total.  The order depends on S alone.
static __device__ __forceinline__ f32x4 h3d_chain_sum4(const float *__restrict__ part, size_t n, int S, size_t col, bool active, int lane,
                                                       int lanes, int worker, int workers, f32x4 *s_chain, f32x4 *s_tot)
{
    const int G = (S + 63) / 64;
    for (int g = worker; g < G; g += workers) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (active)
            for (int s = g; s < S; s += G) v += *reinterpret_cast<const f32x4 *>(part + (size_t)s * n + col);
        s_chain[g * lanes + lane] = v;
    }
    __syncthreads();
    if (worker == 0) {
        f32x4 t = s_chain[lane];
        for (int g = 1; g < G; ++g) t += s_chain[g * lanes + lane];
        s_tot[lane] = t;
    }
    __syncthreads();
    return s_tot[lane];
}

// rows > 0: TAPS_LAST, n = 9 * rows * cols
static inline int h3d_split_sum(const float *part, float *out, size_t n, int S, hipStream_t st, int rows = 0, int cols = 0)
{
    const dim3 grid((unsigned)((n + 255) / 256));
    if (rows) return h3d_launch({"h3d_split_sum_kernel", true}, h3d_split_sum_kernel<true>, grid, dim3(256), 0, st, part, out, n, S, rows, cols);
    return h3d_launch({"h3d_split_sum_kernel", false}, h3d_split_sum_kernel<false>, grid, dim3(256), 0, st, part, out, n, S, rows, cols);
}
