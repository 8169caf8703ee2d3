// Modulated deformable convolution (DCNv2) BACKWARD on gfx950: the gradients of csrc/dcn.hip's operator.
//
// Reference being replaced (DCNv2/src/cuda/): dcn_v2_cuda.cu:175-336 (host function: per image, columns = W^T grad_output by Sgemm,
// col2im_coord, col2im, im2col + Sgemm for grad_weight, Sgemv for grad_bias) and dcn_v2_im2col_cuda.cu:56-123, 197-327 (gradient /
// coordinate weights, the three kernels).  With col[b,c,t,p] = mask * bilinear(x[b,c], pos(t,p) + offset) and G = grad_output:
//   grad_bias[co]      = sum_{b,p} G
//   grad_weight[co,c,t]= sum_{b,p} G[b,co,p] col[b,c,t,p]
//   gcol[b,c,t,p]      = sum_co weight[co,c,t] G[b,co,p]
//   grad_input        += gcol * mask * corner weight, at the (up to) four corners inside the image
//   grad_mask[b,g,t,p] = sum_{c in g} gcol * bilinear(x[b,c])
//   grad_offset        = sum_{c in g} gcol * mask * d bilinear / d(h | w)      (floor convention: right-hand derivative at integers)
// Neither `col` nor `gcol` exists in memory here: both are produced and consumed inside one kernel.
//
// Two levels.  GENERAL (any kernel size / stride / pad / dilation / deformable_group / channel count): fp32 FMA, LDS-tiled.
// MODEL CONFIGURATION (3x3 s1 p1 d1 dg1, C % 16 == 0): both contractions on v_mfma_f32_32x32x2_f32 (exact fmaf chains, the
// arithmetic H3D_DCN_F32_MFMA selects in the forward), sampling in the same kernel.  The K = pixels contraction of grad_weight, its
// partial stores and the C/D layout are csrc/grad_tile.h's, shared with csrc/heads_bwd.hip and csrc/conv_bwd.hip.
//
// Reproducibility: grad_offset, grad_mask, grad_weight and grad_bias are sums in a fixed order (bit-identical from run to run);
// grad_input is a scatter by float atomic adds to global memory (the order of the adds, hence the last bits, varies).
#include "common.h"
#include "dcn_sample.h"
#include "grad_tile.h"
#include "split_sum.h"
#include <algorithm>

struct DcnBwdArgs {
    const float *in, *w, *off, *mask, *go;
    float *gin, *goff, *gmask;
    float *part;        // grad_weight partials (split-K), see the launchers
    const float *xn;    // fast path: input in NHWC
    const float *wp;    // fast path: filters packed for the gcol MFMA
    int B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, dg, Ho, Wo;
    int S, L;           // grad_weight: number of pixel splits, pixels per split
};

// The sample of one (pixel, tap) with what the gradients need on top of the forward's `Sample`: the fractional parts.
struct SampleG {
    Sample s;
    float lh, lw, hh, hw;
};
__device__ __forceinline__ SampleG make_sample_g(float h_im, float w_im, float mask, int H, int W)
{
    SampleG g;
    g.s = make_sample(h_im, w_im, mask, H, W);
    g.lh = h_im - floorf(h_im);
    g.lw = w_im - floorf(w_im);
    g.hh = 1.f - g.lh;
    g.hw = 1.f - g.lw;
    return g;
}
// d bilinear / dh and / dw from the four corner values (zero for corners outside): dcn_v2_im2col_cuda.cu:86-123
__device__ __forceinline__ float coord_h(const SampleG &g, float v1, float v2, float v3, float v4) { return g.hw * (v3 - v1) + g.lw * (v4 - v2); }
__device__ __forceinline__ float coord_w(const SampleG &g, float v1, float v2, float v3, float v4) { return g.hh * (v2 - v1) + g.lh * (v4 - v3); }

// ================================================================================================================================
// grad_bias: one workgroup per output channel, fixed-order tree.
__global__ __launch_bounds__(256) void dcn_bwd_bias_kernel(const float *__restrict__ go, float *__restrict__ gb, int B, int Cout, int HoWo)
{
    __shared__ float s[256];
    const int co = blockIdx.x;
    float a = 0.f;
    for (int b = 0; b < B; ++b) {
        const float *p = go + ((size_t)b * Cout + co) * HoWo;
        for (int n = threadIdx.x; n < HoWo; n += 256) a += p[n];
    }
    s[threadIdx.x] = a;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) gb[co] = s[0];
}

// ================================================================================================================================
// GENERAL, data gradients.  Workgroup = 64 output pixels of one image, ALL channels: for every (group, tap) the sampling geometry is
// computed once per pixel; gcol for 16 channels x 64 pixels comes from an LDS-tiled contraction over Cout (thread = pixel x 4 channels,
// so gcol stays in registers), is scattered to grad_input and folded into the per-pixel grad_offset / grad_mask sums, which are reduced
// over the four waves in a fixed order (no atomics).
__global__ __launch_bounds__(256) void dcn_bwd_data_kernel(DcnBwdArgs a)
{
    constexpr int TP = 64, CC = 16, KO = 16;
    __shared__ float s_g[KO][TP];
    __shared__ float s_w[KO][CC];
    __shared__ float s_red[4][3][TP];
    const int tid = threadIdx.x, p = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, n = blockIdx.x * TP + p;
    const int HoWo = a.Ho * a.Wo, HW = a.H * a.W, khw = a.kh * a.kw, cpg = a.C / a.dg;
    const bool valid = n < HoWo;
    const int oh = valid ? n / a.Wo : 0, ow = valid ? n - oh * a.Wo : 0;
    const bool want_om = a.goff || a.gmask;
    for (int g = 0; g < a.dg; ++g) {
        for (int t = 0; t < khw; ++t) {
            const int i = t / a.kw, jj = t - i * a.kw;
            float m = 0.f, d_h = 0.f, d_w = 0.f;
            if (valid) {
                d_h = a.off[((size_t)(b * a.dg + g) * 2 * khw + 2 * t) * HoWo + n];
                d_w = a.off[((size_t)(b * a.dg + g) * 2 * khw + 2 * t + 1) * HoWo + n];
                m = a.mask[((size_t)(b * a.dg + g) * khw + t) * HoWo + n];
            }
            const SampleG sg = make_sample_g((float)(oh * a.sh - a.ph + i * a.dh) + d_h, (float)(ow * a.sw - a.pw + jj * a.dw) + d_w, m, a.H, a.W);
            const bool live = valid && sg.s.inside;
            float am = 0.f, ah = 0.f, aw = 0.f;
            const int cend = (g + 1) * cpg;
            for (int c0 = g * cpg; c0 < cend; c0 += CC) {
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
                for (int co0 = 0; co0 < a.Cout; co0 += KO) {
                    __syncthreads();
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int co = co0 + wv + 4 * j;
                        s_g[wv + 4 * j][p] = (co < a.Cout && valid) ? a.go[((size_t)b * a.Cout + co) * HoWo + n] : 0.f;
                    }
                    {
                        const int co = co0 + (tid >> 4), c = c0 + (tid & 15);
                        s_w[tid >> 4][tid & 15] = (co < a.Cout && c < cend) ? a.w[((size_t)co * a.C + c) * khw + t] : 0.f;
                    }
                    __syncthreads();
#pragma unroll
                    for (int k = 0; k < KO; ++k) {
                        const float gv = s_g[k][p];
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] = fmaf(s_w[k][wv * 4 + e], gv, acc[e]);
                    }
                }
                if (live) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = c0 + wv * 4 + e;
                        if (c >= cend) continue;
                        const size_t base = ((size_t)b * a.C + c) * HW;
                        const float gc = acc[e];
                        if (want_om) {
                            const float *im = a.in + base;
                            const float v1 = sg.s.off[0] >= 0 ? im[sg.s.off[0]] : 0.f;
                            const float v2 = sg.s.off[1] >= 0 ? im[sg.s.off[1]] : 0.f;
                            const float v3 = sg.s.off[2] >= 0 ? im[sg.s.off[2]] : 0.f;
                            const float v4 = sg.s.off[3] >= 0 ? im[sg.s.off[3]] : 0.f;
                            am = fmaf(gc, sg.s.w[0] * v1 + sg.s.w[1] * v2 + sg.s.w[2] * v3 + sg.s.w[3] * v4, am);
                            ah = fmaf(gc * m, coord_h(sg, v1, v2, v3, v4), ah);
                            aw = fmaf(gc * m, coord_w(sg, v1, v2, v3, v4), aw);
                        }
                        if (a.gin) {
                            const float gm = gc * m;
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (sg.s.off[k] >= 0) unsafeAtomicAdd(a.gin + base + sg.s.off[k], sg.s.w[k] * gm);
                        }
                    }
                }
            }
            if (want_om) {
                s_red[wv][0][p] = am; s_red[wv][1][p] = ah; s_red[wv][2][p] = aw;
                __syncthreads();
                if (wv == 0 && valid) {
                    const float rm = (s_red[0][0][p] + s_red[1][0][p]) + (s_red[2][0][p] + s_red[3][0][p]);
                    const float rh = (s_red[0][1][p] + s_red[1][1][p]) + (s_red[2][1][p] + s_red[3][1][p]);
                    const float rw = (s_red[0][2][p] + s_red[1][2][p]) + (s_red[2][2][p] + s_red[3][2][p]);
                    if (a.gmask) a.gmask[((size_t)(b * a.dg + g) * khw + t) * HoWo + n] = rm;
                    if (a.goff) {
                        a.goff[((size_t)(b * a.dg + g) * 2 * khw + 2 * t) * HoWo + n] = rh;
                        a.goff[((size_t)(b * a.dg + g) * 2 * khw + 2 * t + 1) * HoWo + n] = rw;
                    }
                }
                // (s_red is written again only after the two barriers of the next contraction step)
            }
        }
    }
}

// ================================================================================================================================
// GENERAL, grad_weight.  Workgroup = 64 output channels x 64 filter elements k = (c, tap), one split of the B*Ho*Wo pixels walked 16 at
// a time: sampled columns and grad_output meet in LDS.  Partials [S][Cout][K] go to the workspace and are summed in split order (csrc/split_sum.h).
__global__ __launch_bounds__(256) void dcn_bwd_weight_kernel(DcnBwdArgs a)
{
    constexpr int TK = 64, TC = 64, PC = 16;
    __shared__ float s_col[PC][TK + 4];
    __shared__ float s_gg[PC][TC + 4];
    const int tid = threadIdx.x;
    const int k0 = blockIdx.x * TK, co0 = blockIdx.y * TC, sp = blockIdx.z;
    const int HoWo = a.Ho * a.Wo, khw = a.kh * a.kw, K = a.C * khw, cpg = a.C / a.dg;
    const long long NPX = (long long)a.B * HoWo;
    const long long q_begin = (long long)sp * a.L, q_end = std::min<long long>(NPX, q_begin + a.L);
    const int tk = tid & 15, tc = tid >> 4;
    const int pl = tid & 15;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (long long q0 = q_begin; q0 < q_end; q0 += PC) {
        const long long gp = q0 + pl;
        const bool valid = gp < q_end;
        const int b = valid ? (int)(gp / HoWo) : 0;
        const int n = valid ? (int)(gp - (long long)b * HoWo) : 0;
        const int oh = n / a.Wo, ow = n - oh * a.Wo;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kl = (tid >> 4) + 16 * j, k = k0 + kl;
            float val = 0.f;
            if (valid && k < K) {
                const int c = k / khw, t = k - c * khw;
                const int i = t / a.kw, jj = t - i * a.kw;
                const int g = c / cpg;
                const float d_h = a.off[((size_t)(b * a.dg + g) * 2 * khw + 2 * t) * HoWo + n];
                const float d_w = a.off[((size_t)(b * a.dg + g) * 2 * khw + 2 * t + 1) * HoWo + n];
                const float m = a.mask[((size_t)(b * a.dg + g) * khw + t) * HoWo + n];
                const Sample s = make_sample((float)(oh * a.sh - a.ph + i * a.dh) + d_h, (float)(ow * a.sw - a.pw + jj * a.dw) + d_w, m, a.H, a.W);
                if (s.inside) {
                    const float *im = a.in + ((size_t)b * a.C + c) * a.H * a.W;
                    const float v1 = s.off[0] >= 0 ? im[s.off[0]] : 0.f;
                    const float v2 = s.off[1] >= 0 ? im[s.off[1]] : 0.f;
                    const float v3 = s.off[2] >= 0 ? im[s.off[2]] : 0.f;
                    const float v4 = s.off[3] >= 0 ? im[s.off[3]] : 0.f;
                    val = (s.w[0] * v1 + s.w[1] * v2 + s.w[2] * v3 + s.w[3] * v4) * m;
                }
            }
            s_col[pl][kl] = val;
            const int co = co0 + kl;
            s_gg[pl][kl] = (valid && co < a.Cout) ? a.go[((size_t)b * a.Cout + co) * HoWo + n] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PC; ++q) {
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = s_gg[q][tc * 4 + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = s_col[q][tk * 4 + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = co0 + tc * 4 + i;
        if (co >= a.Cout) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + tk * 4 + j;
            if (k < K) a.part[((size_t)sp * a.Cout + co) * K + k] = acc[i][j];
        }
    }
}

// ================================================================================================================================
// MODEL CONFIGURATION (3x3 s1 p1 d1 dg1, C % 16 == 0), data gradients on the matrix cores.
//
// Filters packed for the A operand: wp[t][ct][co8][half][c32][s] = w[co8*8 + half*4 + s][ct*32 + c32][t] (zero beyond Cout / C): a
// lane reads 16 bytes = its operand of four consecutive 32x32x2 steps, 1 KiB per wave and load.
__global__ void dcn_bwd_wpack_kernel(const float *__restrict__ w, float *__restrict__ wp, int Cout, int C, int CT, int CO8)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)9 * CT * CO8 * 256;
    if (i >= total) return;
    const int s = (int)(i & 3), c32 = (int)((i >> 2) & 31), half = (int)((i >> 7) & 1);
    size_t r = i >> 8;
    const int co8 = (int)(r % CO8); r /= CO8;
    const int ct = (int)(r % CT);
    const int t = (int)(r / CT);
    const int co = co8 * 8 + half * 4 + s, c = ct * 32 + c32;
    wp[i] = (co < Cout && c < C) ? w[((size_t)co * C + c) * 9 + t] : 0.f;
}

// Workgroup = 32 consecutive output pixels of one image x ALL channels.  grad_output of the tile sits in LDS in the B-operand order
// ([co8][half][pixel][s]); a work item is (tap, slot): the wave computes gcol for 32 channels x 32 pixels per channel tile of its slot
// (K = Cout on v_mfma_f32_32x32x2_f32), and the C/D layout hands every lane ONE pixel and 4 runs of 4 consecutive channels of it -- the
// sampling layout: geometry once per (lane, tap), corner values as 16-byte reads of the NHWC copy of the input, grad_input scattered with
// float atomics to the NCHW tensor (lanes = consecutive pixels: neighbouring addresses), grad_offset / grad_mask summed over the
// lane's channels, the two lane halves (one shuffle) and, in slot order, over the slots: no atomics, fixed order.
__global__ __launch_bounds__(256) void dcn_bwd_data_mfma_kernel(DcnBwdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    const int CO8 = (a.Cout + 7) >> 3, CT = (a.C + 31) >> 5, NS = CT < 4 ? CT : 4;
    float *s_g = s_dyn;                          // [CO8][2][32][4]
    float *s_part = s_dyn + (size_t)CO8 * 256;   // [9][4][3][32]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, p = lane & 31, half = lane >> 5;
    const int b = blockIdx.y, n0 = blockIdx.x * 32, HW = a.H * a.W;
    for (int idx = tid; idx < CO8 * 256; idx += 256) {
        const int co = idx >> 5, pp = idx & 31;
        const float v = (co < a.Cout && n0 + pp < HW) ? a.go[((size_t)b * a.Cout + co) * HW + n0 + pp] : 0.f;
        s_g[(((co >> 3) * 2 + ((co >> 2) & 1)) * 32 + pp) * 4 + (co & 3)] = v;
    }
    __syncthreads();
    const int n = n0 + p;
    const bool valid = n < HW;
    const int oh = valid ? n / a.W : 0, ow = valid ? n - oh * a.W : 0;
    const bool want_om = a.goff || a.gmask;
    for (int q = wv; q < 9 * NS; q += 4) {
        const int t = q / NS, sl = q - t * NS;
        const int i = t / 3, jj = t - 3 * i;
        float m = 0.f, d_h = 0.f, d_w = 0.f;
        if (valid) {
            d_h = a.off[((size_t)b * 18 + 2 * t) * HW + n];
            d_w = a.off[((size_t)b * 18 + 2 * t + 1) * HW + n];
            m = a.mask[((size_t)b * 9 + t) * HW + n];
        }
        const SampleG sg = make_sample_g((float)(oh - 1 + i) + d_h, (float)(ow - 1 + jj) + d_w, m, a.H, a.W);
        const bool live = valid && sg.s.inside;
        float am = 0.f, ah = 0.f, aw = 0.f;
        for (int ct = sl; ct < CT; ct += NS) {
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            const f32x4 *wa = reinterpret_cast<const f32x4 *>(a.wp) + ((size_t)(t * CT + ct) * CO8 * 2 + half) * 32 + p;
            const f32x4 *gb = reinterpret_cast<const f32x4 *>(s_g) + half * 32 + p;
            for (int co8 = 0; co8 < CO8; ++co8) {
                const f32x4 a4 = wa[(size_t)co8 * 64], b4 = gb[co8 * 64];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[0], b4[0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[1], b4[1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[2], b4[2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[3], b4[3], acc, 0, 0, 0);
            }
            if (live) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = ct * 32 + gt_row4(r, half);
                    if (c >= a.C) continue;                            // (C % 16 == 0: a run of 4 is inside or outside as a whole)
                    f32x4 v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        v[k] = (want_om && sg.s.off[k] >= 0) ? *reinterpret_cast<const f32x4 *>(a.xn + ((size_t)b * HW + sg.s.off[k]) * a.C + c)
                                                             : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float gc = acc[4 * r + e];
                        if (want_om) {
                            am = fmaf(gc, sg.s.w[0] * v[0][e] + sg.s.w[1] * v[1][e] + sg.s.w[2] * v[2][e] + sg.s.w[3] * v[3][e], am);
                            ah = fmaf(gc * m, coord_h(sg, v[0][e], v[1][e], v[2][e], v[3][e]), ah);
                            aw = fmaf(gc * m, coord_w(sg, v[0][e], v[1][e], v[2][e], v[3][e]), aw);
                        }
                        if (a.gin) {
                            const float gm = gc * m;
                            float *dst = a.gin + ((size_t)b * a.C + c + e) * HW;
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (sg.s.off[k] >= 0) unsafeAtomicAdd(dst + sg.s.off[k], sg.s.w[k] * gm);
                        }
                    }
                }
            }
        }
        if (want_om) {
            am += __shfl_xor(am, 32); ah += __shfl_xor(ah, 32); aw += __shfl_xor(aw, 32);
            if (half == 0) {
                s_part[((t * 4 + sl) * 3 + 0) * 32 + p] = am;
                s_part[((t * 4 + sl) * 3 + 1) * 32 + p] = ah;
                s_part[((t * 4 + sl) * 3 + 2) * 32 + p] = aw;
            }
        }
    }
    if (!want_om) return;
    __syncthreads();
    for (int idx = tid; idx < 9 * 32; idx += 256) {
        const int t = idx >> 5, pp = idx & 31;
        if (n0 + pp >= HW) continue;
        float r[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float v = s_part[((t * 4 + 0) * 3 + j) * 32 + pp];
            for (int sl = 1; sl < NS; ++sl) v += s_part[((t * 4 + sl) * 3 + j) * 32 + pp];
            r[j] = v;
        }
        if (a.gmask) a.gmask[((size_t)b * 9 + t) * HW + n0 + pp] = r[0];
        if (a.goff) {
            a.goff[((size_t)b * 18 + 2 * t) * HW + n0 + pp] = r[1];
            a.goff[((size_t)b * 18 + 2 * t + 1) * HW + n0 + pp] = r[2];
        }
    }
}

// MODEL CONFIGURATION, grad_weight on the matrix cores: D[co][c] += G[co][pixel] col[pixel][c] per tap, K = pixels.  Workgroup = 3 waves
// = the 3 kernel rows (3 taps each) x one tile of 32 input channels x up to 64 output channels x one split of the pixels of one image.
// A lane IS an input channel (column of the B operand) for the two pixel slots of a step: it samples col itself from the NHWC copy of the
// input (32 lanes = 128 contiguous bytes per corner), so nothing is staged: gt_gw_pixels as a single chain with the sampling as its B
// fetch.  Partials [split][tap][Cout][C] go to the workspace.
__global__ __launch_bounds__(192) void dcn_bwd_weight_mfma_kernel(DcnBwdArgs a)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l32 = lane & 31, half = lane >> 5;
    const int HW = a.H * a.W, SP = a.S / a.B;
    const int c = blockIdx.x * 32 + l32;
    const int cot0 = blockIdx.y * 2, COT = (a.Cout + 31) >> 5;
    const bool two = cot0 + 1 < COT;
    const int b = blockIdx.z / SP, chunk = blockIdx.z - b * SP;
    const auto [p_begin, p_end] = gt_split_range(chunk, a.L, HW);
    const bool c_ok = c < a.C;
    f32x16 acc[2][3];
    const int co_a0 = cot0 * 32 + l32, co_a1 = co_a0 + 32;
    gt_gw_pixels<0>(acc, p_begin, p_end, half, two, [&](int px, bool ok, int s, float (&av)[2][4], float (&bv)[3][4]) {
        av[0][s] = (ok && co_a0 < a.Cout) ? a.go[((size_t)b * a.Cout + co_a0) * HW + px] : 0.f;
        av[1][s] = (ok && two && co_a1 < a.Cout) ? a.go[((size_t)b * a.Cout + co_a1) * HW + px] : 0.f;
        const int oh = ok ? px / a.W : 0, ow = ok ? px - oh * a.W : 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int t = 3 * wv + j;
            float val = 0.f;
            if (ok) {
                const float d_h = a.off[((size_t)b * 18 + 2 * t) * HW + px];
                const float d_w = a.off[((size_t)b * 18 + 2 * t + 1) * HW + px];
                const float m = a.mask[((size_t)b * 9 + t) * HW + px];
                const Sample sm = make_sample((float)(oh - 1 + wv) + d_h, (float)(ow - 1 + j) + d_w, m, a.H, a.W);
                if (sm.inside && c_ok) {
                    const float *xb = a.xn + (size_t)b * HW * a.C + c;
                    const float v1 = sm.off[0] >= 0 ? xb[(size_t)sm.off[0] * a.C] : 0.f;
                    const float v2 = sm.off[1] >= 0 ? xb[(size_t)sm.off[1] * a.C] : 0.f;
                    const float v3 = sm.off[2] >= 0 ? xb[(size_t)sm.off[2] * a.C] : 0.f;
                    const float v4 = sm.off[3] >= 0 ? xb[(size_t)sm.off[3] * a.C] : 0.f;
                    val = (sm.w[0] * v1 + sm.w[1] * v2 + sm.w[2] * v3 + sm.w[3] * v4) * m;
                }
            }
            bv[j][s] = val;
        }
    });
    if (!c_ok) return;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (m == 1 && !two) break;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            gt_store_column<true>(a.part, ((size_t)blockIdx.z * 9 + 3 * wv + j) * a.Cout, acc[m][j], (cot0 + m) * 32, a.Cout, a.C, c, half);
    }
}

// ================================================================================================================================
// Host side.
struct BwdPlan {
    bool fast;
    int Ho, Wo;
    int Sg; long long Lg;       // general grad_weight: splits of the B*Ho*Wo pixels, pixels per split (multiple of 16)
    int SP, Lf;                 // fast grad_weight: splits per image, pixels per split (multiple of 8)
    // workspace: the general partials [Sg][Cout][K] at offset 0, or (overlaid) the matrix-core path's NHWC input, packed filters and partials
    size_t xn, wp, part_f, total;
};

static bool bwd_plan(BwdPlan &pl, int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int dg)
{
    pl.Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1;
    pl.Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
    if (pl.Ho <= 0 || pl.Wo <= 0) return false;
    const long long NPX = (long long)B * pl.Ho * pl.Wo;
    const long long K = (long long)C * kh * kw;
    const long long tiles = ((K + 63) / 64) * ((Cout + 63) / 64);
    long long Sg = std::min<long long>(std::max<long long>((512 + tiles - 1) / tiles, 1), std::max<long long>(NPX / 256, 1));
    Sg = std::min<long long>(Sg, 64);
    pl.Lg = ((NPX + Sg - 1) / Sg + 15) / 16 * 16;
    pl.Sg = (int)((NPX + pl.Lg - 1) / pl.Lg);
    h3d_ws_layout general, mfma;
    general.take((size_t)pl.Sg * Cout * K * 4);
    // the matrix-core kernels: the model's configuration; the tile of grad_output (Cout rounded up to 8, x 32 pixels) must fit in LDS
    pl.fast = kh == 3 && kw == 3 && sh == 1 && sw == 1 && ph == 1 && pw == 1 && dh == 1 && dw == 1 && dg == 1 && C % 16 == 0 && Cout <= 1024 &&
              H <= 32767 && W <= 32767;
    pl.xn = pl.wp = pl.part_f = 0;
    pl.SP = 1; pl.Lf = 8;
    if (pl.fast) {
        const int HW = H * W, CT = (C + 31) / 32, COB = (Cout + 63) / 64, CO8 = (Cout + 7) / 8;
        long long SP = std::min<long long>(std::max<long long>((1024 + (long long)CT * COB * B - 1) / ((long long)CT * COB * B), 1), std::max(HW / 512, 1));
        pl.Lf = (int)(((HW + SP - 1) / SP + 7) / 8 * 8);
        pl.SP = (HW + pl.Lf - 1) / pl.Lf;
        pl.xn = mfma.take((size_t)B * HW * C * 4);
        pl.wp = mfma.take((size_t)9 * CT * CO8 * 256 * 4);
        pl.part_f = mfma.take((size_t)B * pl.SP * 9 * Cout * C * 4);
    }
    pl.total = std::max(general.total, mfma.total);
    return true;
}

static int bwd_check(const char *what, int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int dg)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || Cout <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || ph < 0 || pw < 0 || dh <= 0 || dw <= 0)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: non-positive dimension", what);
    if (dg <= 0 || C % dg) H3D_FAIL(H3D_ERR_SHAPE, "%s: channels %d not divisible by deformable_group %d", what, C, dg);
    return H3D_OK;
}

extern "C" int h3d_dcn_v2_backward_workspace_bytes(int B, int C, int H, int W, int Cout, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                                   int pad_h, int pad_w, int dilation_h, int dilation_w, int deformable_group, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "dcn_v2_backward_workspace_bytes: null pointer");
    *bytes = 0;
    int rc = bwd_check("dcn_v2_backward", B, C, H, W, Cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group);
    if (rc != H3D_OK) return rc;
    BwdPlan pl;
    if (!bwd_plan(pl, B, C, H, W, Cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group))
        H3D_FAIL(H3D_ERR_SHAPE, "dcn_v2_backward: empty output %dx%d", pl.Ho, pl.Wo);
    *bytes = pl.total;
    return H3D_OK;
}

static int dcn_v2_backward_impl(bool allow_fast, const float *input, const float *weight, const float *bias, const float *offset, const float *mask,
                                const float *grad_output, float *grad_input, float *grad_offset, float *grad_mask, float *grad_weight,
                                float *grad_bias, int B, int C, int H, int W, int Cout, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                int pad_h, int pad_w, int dilation_h, int dilation_w, int deformable_group, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    (void)bias;      // (the gradients do not depend on it; kept for the reference's operand order, may be NULL)
    if (!input || !weight || !offset || !mask || !grad_output) H3D_FAIL(H3D_ERR_ARG, "dcn_v2_backward: null pointer");
    int rc = bwd_check("dcn_v2_backward", B, C, H, W, Cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group);
    if (rc != H3D_OK) return rc;
    BwdPlan pl;
    if (!bwd_plan(pl, B, C, H, W, Cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group))
        H3D_FAIL(H3D_ERR_SHAPE, "dcn_v2_backward: empty output %dx%d", pl.Ho, pl.Wo);
    const bool data = grad_input || grad_offset || grad_mask;
    const bool fast = allow_fast && pl.fast;
    const bool need_ws = grad_weight || (fast && data);
    if (need_ws && (!workspace || workspace_bytes < pl.total))
        H3D_FAIL(H3D_ERR_ARG, "dcn_v2_backward: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, pl.total);
    hipStream_t st = (hipStream_t)stream;
    const int HoWo = pl.Ho * pl.Wo;
    DcnBwdArgs a = {};
    a.in = input; a.w = weight; a.off = offset; a.mask = mask; a.go = grad_output;
    a.gin = grad_input; a.goff = grad_offset; a.gmask = grad_mask;
    a.B = B; a.C = C; a.H = H; a.W = W; a.Cout = Cout; a.kh = kernel_h; a.kw = kernel_w; a.sh = stride_h; a.sw = stride_w;
    a.ph = pad_h; a.pw = pad_w; a.dh = dilation_h; a.dw = dilation_w; a.dg = deformable_group; a.Ho = pl.Ho; a.Wo = pl.Wo;
    if (grad_input && hipMemsetAsync(grad_input, 0, (size_t)B * C * H * W * 4, st) != hipSuccess) H3D_FAIL(H3D_ERR_LAUNCH, "dcn_v2_backward: memset");
    if (grad_bias) H3D_TRY(h3d_launch({"dcn_bwd_bias_kernel"}, dcn_bwd_bias_kernel, dim3(Cout), dim3(256), 0, st, grad_output, grad_bias, B, Cout, HoWo));
    if (!fast) {
        if (data) H3D_TRY(h3d_launch({"dcn_bwd_data_kernel"}, dcn_bwd_data_kernel, dim3(cdiv(HoWo, 64), B), dim3(256), 0, st, a));
        if (grad_weight) {
            const int K = C * kernel_h * kernel_w;
            a.part = pl.Sg == 1 ? grad_weight : (float *)workspace;
            a.S = pl.Sg; a.L = (int)std::min<long long>(pl.Lg, 0x7fffffff);
            if (pl.Lg > 0x7fffffff) H3D_FAIL(H3D_ERR_SHAPE, "dcn_v2_backward: %lld pixels per split", pl.Lg);
            H3D_TRY(h3d_launch({"dcn_bwd_weight_kernel"}, dcn_bwd_weight_kernel, dim3(cdiv(K, 64), cdiv(Cout, 64), pl.Sg), dim3(256), 0, st, a));
            if (pl.Sg > 1) H3D_TRY(h3d_split_sum((const float *)workspace, grad_weight, (size_t)Cout * K, pl.Sg, st));
        }
        return H3D_OK;
    }
    const int CT = (C + 31) / 32, CO8 = (Cout + 7) / 8;
    char *ws = (char *)workspace;
    float *xn = (float *)(ws + pl.xn), *wp = (float *)(ws + pl.wp), *part = (float *)(ws + pl.part_f);
    a.xn = xn; a.wp = wp; a.part = part;
    if (grad_weight || grad_offset || grad_mask)        // (grad_input alone needs no input values)
        H3D_TRY(h3d_nchw_f32_to_nhwc(input, xn, H3D_F32, B, C, H, W, C, stream));
    if (data) {
        const size_t wtotal = (size_t)9 * CT * CO8 * 256;
        H3D_TRY(h3d_launch({"dcn_bwd_wpack_kernel"}, dcn_bwd_wpack_kernel, dim3((unsigned)((wtotal + 255) / 256)), dim3(256), 0, st, weight, wp, Cout, C, CT, CO8));
        const size_t lds = ((size_t)CO8 * 256 + 9 * 4 * 3 * 32) * 4;
        if (lds > 48 * 1024 &&
            hipFuncSetAttribute((const void *)dcn_bwd_data_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            H3D_FAIL(H3D_ERR_LAUNCH, "dcn_v2_backward: %zu bytes of LDS", lds);
        H3D_TRY(h3d_launch({"dcn_bwd_data_mfma_kernel"}, dcn_bwd_data_mfma_kernel, dim3(cdiv(H * W, 32), B), dim3(256), lds, st, a));
    }
    if (grad_weight) {
        a.S = B * pl.SP; a.L = pl.Lf;
        H3D_TRY(h3d_launch({"dcn_bwd_weight_mfma_kernel"}, dcn_bwd_weight_mfma_kernel, dim3(CT, cdiv(Cout, 64), B * pl.SP), dim3(192), 0, st, a));
        H3D_TRY(h3d_split_sum(part, grad_weight, (size_t)9 * Cout * C, B * pl.SP, st, Cout, C));      // [tap][co][c] -> the reference's [co][c][tap]
    }
    return H3D_OK;
}

extern "C" int h3d_dcn_v2_backward(const float *input, const float *weight, const float *bias, const float *offset, const float *mask,
                                   const float *grad_output, float *grad_input, float *grad_offset, float *grad_mask, float *grad_weight,
                                   float *grad_bias, int B, int C, int H, int W, int Cout, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                   int pad_h, int pad_w, int dilation_h, int dilation_w, int deformable_group, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    return dcn_v2_backward_impl(true, input, weight, bias, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight, grad_bias, B, C, H,
                                W, Cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group, workspace,
                                workspace_bytes, stream);
}

// The general kernels on ANY configuration, the model's included (the correctness anchor the matrix-core kernels are tested and timed against).
extern "C" int h3d_dcn_v2_backward_general(const float *input, const float *weight, const float *bias, const float *offset, const float *mask,
                                           const float *grad_output, float *grad_input, float *grad_offset, float *grad_mask, float *grad_weight,
                                           float *grad_bias, int B, int C, int H, int W, int Cout, int kernel_h, int kernel_w, int stride_h,
                                           int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, int deformable_group, void *workspace,
                                           size_t workspace_bytes, void *stream)
{
    return dcn_v2_backward_impl(false, input, weight, bias, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight, grad_bias, B, C, H,
                                W, Cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group, workspace,
                                workspace_bytes, stream);
}
