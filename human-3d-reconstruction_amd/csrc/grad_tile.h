// Device and host pieces shared by the fp32 matrix-core gradient kernels (csrc/heads_bwd.hip, dcn_bwd.hip, conv_bwd.hip): the 4 x 32
// pixel tile and its halo in LDS, the C/D layout of v_mfma_f32_32x32x2_f32, one tap of the gather-form 3x3 contraction, the filter image
// that contraction reads, the K = pixels (grad_W) contraction of a wave and its partial stores, and the split of the pixels.  Everything
// here is force-inlined into its call site and keeps that site's operations and their order: the kernels' sums stay bit-identical.
#pragma once
#include "common.h"
#include <algorithm>

// ---- the pixel tile ------------------------------------------------------------------------------------------------------------
constexpr int GT_TH = 4, GT_TW = 32;              // pixel tile of a workgroup (4 waves, one row each)
constexpr int GT_IH = GT_TH + 2, GT_IW = GT_TW + 2;
constexpr int GT_PS = 64 + 4;                     // floats per halo pixel (padded: the 16-byte B-fragment reads stay conflict-free)

// nv 16-byte vectors (channels c0 .. c0 + 4 nv - 1) of the ih x iw halo pixels whose first is (hy0, hx0) -> LDS, zero outside the
// H x W image.  src is NHWC with channel stride cs; block = 256; the LDS rows keep the pitch GT_IW whatever iw is.
__device__ __forceinline__ void gt_stage_halo(float *s_halo, const float *__restrict__ src, int cs, int c0, int b, int H, int W, int hy0,
                                              int hx0, int ih, int iw, int nv, int tid)
{
    for (int i = tid; i < ih * iw * nv; i += 256) {
        const int v = i % nv, pix = i / nv;
        const int iy = pix / iw, ix = pix - iy * iw;
        const int gy = hy0 + iy, gx = hx0 + ix;
        f32x4 val = {0.f, 0.f, 0.f, 0.f};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W)
            val = *reinterpret_cast<const f32x4 *>(src + ((size_t)(b * H + gy) * W + gx) * cs + c0 + v * 4);
        *reinterpret_cast<f32x4 *>(s_halo + (pix + iy * (GT_IW - iw)) * GT_PS + v * 4) = val;
    }
}

// ---- the C/D layout ------------------------------------------------------------------------------------------------------------
// A 32 x 32 accumulator of v_mfma_f32_32x32x2_f32: lane = column (lane & 31); register e of the lane holds row
// (e & 3) + 8 (e >> 2) + 4 (lane >> 5), so registers 4g .. 4g + 3 are the four consecutive rows from 8 g + 4 (lane >> 5).
__device__ __forceinline__ int gt_row(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }
__device__ __forceinline__ int gt_row4(int g, int half) { return 8 * g + 4 * half; }

template <int N>
__device__ __forceinline__ void gt_zero(f32x16 (&a)[N])
{
#pragma unroll
    for (int m = 0; m < N; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) a[m][e] = 0.f;
}
template <int N>
__device__ __forceinline__ void gt_add(f32x16 (&acc)[N], const f32x16 (&part)[N])
{
#pragma unroll
    for (int m = 0; m < N; ++m) acc[m] += part[m];
}
// a chain of the K = pixels contractions ends: its sums join acc (`add`: not before the first chain) and part starts over
template <int N>
__device__ __forceinline__ void gt_chain_next(f32x16 (&acc)[N], f32x16 (&part)[N], bool add)
{
#pragma unroll
    for (int m = 0; m < N; ++m) {
        acc[m] = add ? acc[m] + part[m] : acc[m];
#pragma unroll
        for (int e = 0; e < 16; ++e) part[m][e] = 0.f;
    }
}
// ... the same for the [2][3] accumulators of a grad_W wave
template <int M, int N>
__device__ __forceinline__ void gt_zero(f32x16 (&a)[M][N])
{
#pragma unroll
    for (int m = 0; m < M; ++m) gt_zero(a[m]);
}
template <int M, int N>
__device__ __forceinline__ void gt_add(f32x16 (&acc)[M][N], const f32x16 (&part)[M][N])
{
#pragma unroll
    for (int m = 0; m < M; ++m) gt_add(acc[m], part[m]);
}
template <int M, int N>
__device__ __forceinline__ void gt_chain_next(f32x16 (&acc)[M][N], f32x16 (&part)[M][N], bool add)
{
#pragma unroll
    for (int m = 0; m < M; ++m) gt_chain_next(acc[m], part[m], add);
}

// acc (rows r0 .. r0 + 31, the lane's column c) -> rows row0 + r0 .. of the row-major [.][C] matrix p; BOUND: only the rows r < R
template <bool BOUND>
__device__ __forceinline__ void gt_store_column(float *p, size_t row0, const f32x16 &acc, int r0, int R, int C, int c, int half)
{
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = r0 + gt_row(e, half);
        if (!BOUND || r < R) p[(row0 + r) * C + c] = acc[e];
    }
}

// ---- the gather-form 3x3 contraction (grad of the input of a convolution) ------------------------------------------------------------
// acc[m] += sum over ng (<= 8) groups of 8 K channels of  A[m*32 + row][k] . B[pixel][k]  for ONE tap: two 32-row tiles, 32 pixels, a
// fresh fmaf chain of 8 ng terms that joins acc afterwards.  A operand: 16-byte loads ap[k8 * 2 M] (and + 32) of a filter image
// [tap][k8][half][M][4] (a lane's operand of four consecutive K steps; slot `half` of step s of group k8 is K channel k8*8 + half*4 + s).
// B operand: 16 bytes per group at bp, the lane's halo pixel.
__device__ __forceinline__ void gt_tap_mfma(f32x16 (&acc)[2], const f32x4 *__restrict__ ap, int M, const float *bp, int ng)
{
    f32x16 part[2];
    gt_zero(part);
#pragma unroll
    for (int k8 = 0; k8 < 8; ++k8) {
        if (k8 < ng) {
            const f32x4 a0 = ap[(size_t)k8 * 2 * M], a1 = ap[(size_t)k8 * 2 * M + 32];
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(bp + k8 * 8);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], bv[s], part[0], 0, 0, 0);
                part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], bv[s], part[1], 0, 0, 0);
            }
        }
    }
    gt_add(acc, part);
}

// element i of that filter image for the gather form, wf[t][k8][half][c][s] (c < Cpad) = W[k8*8 + half*4 + s][c][t] of the filters
// W[Cout][C][taps], zero for c >= C; `flip`: tap taps - 1 - t (the stride-1 kernel that walks the halo in tap order)
__device__ __forceinline__ float gt_filter_image(const float *__restrict__ w, int i, int C, int Cout, int Cpad, int taps, bool flip)
{
    const int s = i & 3;
    int r = i >> 2;
    const int c = r % Cpad; r /= Cpad;
    const int half = r & 1; r >>= 1;
    const int kg = Cout / 8;
    const int k8 = r % kg, t = r / kg;
    return c < C ? w[((size_t)(k8 * 8 + half * 4 + s) * C + c) * taps + (flip ? taps - 1 - t : t)] : 0.f;
}

// ---- the K = pixels contraction (grad of the filters) --------------------------------------------------------------------------------
// A group of 8 pixels is 4 MFMA steps; slot `half` of step s holds pixel P + 4 half + s for both operands: av[m][s] the lane's row of
// A tile m, bv[j][s] its column of B tile j.  part[m][j] += A_m^T B_j for the tiles with on(m, j).
template <typename On>
__device__ __forceinline__ void gt_gw_step(f32x16 (&part)[2][3], const float (&av)[2][4], const float (&bv)[3][4], On on)
{
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int m = 0; m < 2; ++m)
                if (on(m, j)) part[m][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][s], bv[j][s], part[m][j], 0, 0, 0);
}

// One wave's contraction over the pixels [q_begin, q_end) with operands it fetches itself: fetch(q, ok, s, av, bv) fills slot s of
// both operands for pixel q (ok: q < q_end; zeros otherwise).  The second A tile only with `two`.  Summation order: CHAIN > 0: chains of
// CHAIN pixels, the chain sums added in pixel order; CHAIN == 0: a single chain.
template <int CHAIN, typename Fetch>
__device__ __forceinline__ void gt_gw_pixels(f32x16 (&acc)[2][3], int q_begin, int q_end, int half, bool two, Fetch fetch)
{
    gt_zero(acc);
    f32x16 part[2][3];
    f32x16 (&dst)[2][3] = CHAIN ? part : acc;
    for (int P = q_begin; P < q_end; P += 8) {
        if constexpr (CHAIN > 0) {
            if ((P - q_begin) % CHAIN == 0) gt_chain_next(acc, part, P > q_begin);
        }
        float av[2][4], bv[3][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int q = P + 4 * half + s;
            fetch(q, q < q_end, s, av, bv);
        }
        gt_gw_step(dst, av, bv, [&](int m, int) { return m == 0 || two; });
    }
    if constexpr (CHAIN > 0) gt_add(acc, part);
}

// ---- the split of the pixels ---------------------------------------------------------------------------------------------------
// S splits of L pixels (a multiple of 8) each, at least split_pixels pixels per split and at most split_max splits
static inline void h3d_split_plan(int NPX, int split_pixels, int split_max, int *S, int *L)
{
    const int s = std::min(split_max, cdiv(NPX, split_pixels));
    *L = cdiv(cdiv(NPX, s), 8) * 8;
    *S = cdiv(NPX, *L);
}
// the pixels [begin, end) of split sp
struct GtRange { int begin, end; };
__device__ __forceinline__ GtRange gt_split_range(int sp, int L, int NPX) { return {sp * L, std::min(NPX, sp * L + L)}; }
