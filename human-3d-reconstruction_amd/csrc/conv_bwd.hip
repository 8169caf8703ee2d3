// Plain convolution BACKWARD on gfx950: the gradients of H3D_OP_CONV's operator  y = act(conv2d(x, W, b) + res)  (act = ReLU or the
// identity, groups = 1; BatchNorm stays folded into W, b).  With g = dL/dy:
//     gg = g * [y > 0]  (ReLU; gradient 0 where y <= 0, torch.relu's)  or  gg = g
//     grad_res = gg            grad_b[o] = sum_px gg[o,px]
//     grad_W[o,c,t] = sum_px gg[o,px] x[c, px*s + t*d - p]
//     grad_x[c,q]   = sum_{o,t} W[o,c,t] gg[o,(q + p - t*d)/s]      over the terms where the division is exact and in range
// fp32 storage and accumulation.  No float atomics: every output is a sum in a fixed order, bit-identical from run to run whichever
// other outputs are requested, and overwritten, never accumulated into.
//
//   1. conv_bwd_gate_kernel    gg in NHWC (into grad_res when the caller wants it, else into the workspace; skipped without ReLU when
//                              neither grad_res nor grad_b is wanted: gg is grad_y itself) and, in the same pass, the per-channel sums
//                              of a chunk of pixels: thread = 4 channels x one pixel phase, chains of CB_CHAIN pixels, the phases meet in
//                              a fixed tree through LDS; h3d_split_sum_kernel adds the chunks.
//   2. grad_x, gather form     matrix cores (3x3 s1 p1, 3x3 s2 p1, 1x1 s1 p0; C, Cout % 16 == 0): csrc/grad_tile.h's tile, halo and tap
//                              contraction (the ones of heads_bwd_gy_kernel) for any Cout -> C.  Workgroup = 4 x 32 input pixels
//                              (stride 2: of ONE parity class of the input pixel, which has 1, 2, 2 or 4 live taps), wave = one
//                              row, 64 channels of grad_x; 64 channels of the gg halo at a time
//                              through LDS.  The workgroup that owns a tile writes it.   General: one thread per element, fp32 FMA.
//   3. grad_W, split-K         K = the B*Ho*Wo pixels in splits of at least CB_SPLIT_PIXELS.  Matrix cores: workgroup = 3 waves x 3
//                              output tiles of 64 x 32 each (3x3: the nine taps of 32 input channels; 1x1: nine tiles of 32 input
//                              channels); per chain of 32 pixels gg and the x rows of every tap go through LDS as 16-byte NHWC rows.
//                              Partials to the workspace, h3d_split_sum_kernel sums them in split order.   General: thread = one
//                              filter element of one split.
// Summation order: tap sums are chains of at most 64 terms added afterwards; the K = pixels contractions are chains of CB_CHAIN pixels,
// the chain sums added in pixel order, then the splits.  The C/D layout, the K = pixels step and the split plan are csrc/grad_tile.h's too.
#include "common.h"
#include "grad_tile.h"
#include "split_sum.h"
#include <algorithm>

constexpr int CB_SPLIT_PIXELS = 512;             // pixels per split of the K = pixels contractions, at least (tests/conv_grad_ref.py mirrors it)
constexpr int CB_SPLIT_MAX = 256;                // splits, at most
constexpr int CB_CHAIN = 32;                     // pixels per fmaf chain of the K = pixels contractions
constexpr int CB_GP = 64 + 8, CB_XP = 32 + 8;    // grad_W: floats per staged gg / x pixel (4 * pitch = 32 mod 64: the two lane halves use disjoint banks)
constexpr int CB_SLOTS = 9;                      // grad_W: output tiles of a workgroup
constexpr int CB_BIAS_CHAINS = 4;                // grad_b: chains per thread and chunk

struct ConvBwdArgs {
    const float *x, *w, *y, *gy;
    const float *gg;        // NHWC [B*Ho*Wo][gg_cs]: the gated gradient
    float *gdst;            // where the gate kernel stores gg (contiguous [.][Cout]) or null
    float *gx;              // NHWC [B,H,W,C] or null
    float *wf;              // [taps][Cout/8][2][Cpad][4]: wf[t][k8][half][c][s] = W[k8*8 + half*4 + s][c][t], zero for c >= C
    float *p_w, *p_b;       // partials: [S][taps][Cout][C] (matrix cores, 3x3), [S][Cout][C][taps] (otherwise); [Sb][Cout]
    int x_cs, y_cs, gy_cs, gg_cs;
    int B, C, H, W, Cout, Ho, Wo;
    int kh, kw, sh, sw, ph, pw, dh, dw;
    int relu, Cpad;
    int tiles_x, tiles_y;
    int NPX, S, L;
    int CG, CGT, P;         // grad_b: channel groups, groups per pass of a workgroup, pixel phases
};

// ---- 1. the gate and the bias sums ---------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void conv_bwd_gate_kernel(ConvBwdArgs a)
{
    __shared__ float s_sum[256 * V];
    const int tid = threadIdx.x;
    const int phase = tid / a.CGT, g0 = tid - phase * a.CGT;
    const bool active = phase < a.P;
    const int chunk = a.P * CB_CHAIN * CB_BIAS_CHAINS;
    const int q0 = blockIdx.x * chunk, q1 = std::min(a.NPX, q0 + chunk);
    float tot[V];
#pragma unroll
    for (int i = 0; i < V; ++i) tot[i] = 0.f;
    if (active) {
        for (int g = g0; g < a.CG; g += a.CGT) {
#pragma unroll
            for (int i = 0; i < V; ++i) tot[i] = 0.f;
            for (int qc = q0 + phase; qc < q1; qc += a.P * CB_CHAIN) {
                float part[V];
#pragma unroll
                for (int i = 0; i < V; ++i) part[i] = 0.f;
                const int qe = std::min(q1, qc + a.P * CB_CHAIN);
                for (int q = qc; q < qe; q += a.P) {
                    float gv[V];
                    if constexpr (V == 4) {
                        const f32x4 t = *reinterpret_cast<const f32x4 *>(a.gy + (size_t)q * a.gy_cs + g * 4);
#pragma unroll
                        for (int i = 0; i < 4; ++i) gv[i] = t[i];
                        if (a.relu) {
                            const f32x4 yv = *reinterpret_cast<const f32x4 *>(a.y + (size_t)q * a.y_cs + g * 4);
#pragma unroll
                            for (int i = 0; i < 4; ++i) gv[i] = yv[i] > 0.f ? gv[i] : 0.f;
                        }
                        if (a.gdst) {
                            const f32x4 o = {gv[0], gv[1], gv[2], gv[3]};
                            *reinterpret_cast<f32x4 *>(a.gdst + (size_t)q * a.Cout + g * 4) = o;
                        }
                    } else {
                        gv[0] = a.gy[(size_t)q * a.gy_cs + g];
                        if (a.relu) gv[0] = a.y[(size_t)q * a.y_cs + g] > 0.f ? gv[0] : 0.f;
                        if (a.gdst) a.gdst[(size_t)q * a.Cout + g] = gv[0];
                    }
#pragma unroll
                    for (int i = 0; i < V; ++i) part[i] += gv[i];
                }
#pragma unroll
                for (int i = 0; i < V; ++i) tot[i] += part[i];
            }
            if (a.P == 1 && a.p_b) {
#pragma unroll
                for (int i = 0; i < V; ++i) a.p_b[(size_t)blockIdx.x * a.Cout + g * V + i] = tot[i];
            }
        }
    }
    if (a.P > 1 && a.p_b) {          // (CGT == CG: the loop above ran once)
        if (active) {
#pragma unroll
            for (int i = 0; i < V; ++i) s_sum[tid * V + i] = tot[i];
        }
        int top = 1;
        while (top < a.P) top <<= 1;
        for (int h = top >> 1; h >= 1; h >>= 1) {          // a fixed tree over the phases: phase p takes phase p + h
            __syncthreads();
            if (active && phase < h && phase + h < a.P) {
#pragma unroll
                for (int i = 0; i < V; ++i) s_sum[tid * V + i] += s_sum[(tid + h * a.CGT) * V + i];
            }
        }
        if (tid < a.CG) {                                  // (phase 0: its own sums)
#pragma unroll
            for (int i = 0; i < V; ++i) a.p_b[(size_t)blockIdx.x * a.Cout + tid * V + i] = s_sum[tid * V + i];
        }
    }
}

// ---- 2. grad_x ----------------------------------------------------------------------------------------------------------------------
__global__ void conv_bwd_pack_kernel(const float *__restrict__ w, float *__restrict__ wf, int C, int Cout, int Cpad, int taps)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = taps * Cout * Cpad;
    if (i >= n) return;
    wf[i] = gt_filter_image(w, i, C, Cout, Cpad, taps, false);
}

// Matrix cores.  grid = (B * tiles, Cpad / 64, parity classes); block = 256.
__global__ __launch_bounds__(256) void conv_bwd_gx_kernel(ConvBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_halo[GT_IH * GT_IW * GT_PS];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, l32 = lane & 31, half = lane >> 5;
    const int s = a.sh, k = a.kh;
    const int py = s == 2 ? (int)(blockIdx.z >> 1) : 0, px = s == 2 ? (int)(blockIdx.z & 1) : 0;
    const int Hc = s == 2 ? (a.H - py + 1) / 2 : a.H, Wc = s == 2 ? (a.W - px + 1) / 2 : a.W;     // the class's pixel grid
    const int tiles = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / tiles, t_ = blockIdx.x - b * tiles;
    const int tyi = t_ / a.tiles_x, txi = t_ - tyi * a.tiles_x;
    const int i0 = tyi * GT_TH, j0 = txi * GT_TW;
    if (i0 >= Hc || j0 >= Wc) return;
    // the gg halo of the tile: rows hy0 .. hy0 + ih - 1, columns hx0 .. hx0 + iw - 1
    const int org = (k == 3 && s == 1) ? 1 : 0;
    const int ih = (k == 3) ? (s == 1 ? GT_IH : GT_TH + 1) : GT_TH, iw = (k == 3) ? (s == 1 ? GT_IW : GT_TW + 1) : GT_TW;
    const int hy0 = i0 - org, hx0 = j0 - org;
    const int m0 = blockIdx.y * 64;
    const int kg_total = a.Cout / 8;
    f32x16 acc[2];
    gt_zero(acc);
    const int nch = (a.Cout + 63) / 64;
    for (int ch = 0; ch < nch; ++ch) {
        const int ng = std::min(8, kg_total - ch * 8);            // groups of 8 gg channels in this chunk
        if (ch) __syncthreads();
        gt_stage_halo(s_halo, a.gg, a.gg_cs, ch * 64, b, a.Ho, a.Wo, hy0, hx0, ih, iw, ng * 2, tid);
        __syncthreads();
        f32x16 part[2];
        gt_zero(part);
#pragma unroll 1
        for (int t = 0; t < k * k; ++t) {
            const int ty = t / k, tx = t - k * ty;
            int dyh = 0, dxh = 0;
            if (k == 3) {
                if (s == 1) { dyh = 2 - ty; dxh = 2 - tx; }
                else {
                    if (((py + 1 - ty) & 1) || ((px + 1 - tx) & 1)) continue;       // no output pixel meets this class through this tap
                    dyh = (py + 1 - ty) / 2; dxh = (px + 1 - tx) / 2;
                }
            }
            const float *bp = s_halo + ((wv + dyh) * GT_IW + l32 + dxh) * GT_PS + half * 4;
            const f32x4 *ap = reinterpret_cast<const f32x4 *>(a.wf) + ((size_t)(t * kg_total + ch * 8) * 2 + half) * a.Cpad + m0 + l32;
            gt_tap_mfma(part, ap, a.Cpad, bp, ng);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[m] = ch ? acc[m] + part[m] : part[m];
    }
    const int qy = s * (i0 + wv) + py, qx = s * (j0 + l32) + px;
    if (i0 + wv < Hc && j0 + l32 < Wc && qy < a.H && qx < a.W) {
        float *dst = a.gx + (((size_t)b * a.H + qy) * a.W + qx) * a.C;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = m0 + m * 32 + gt_row4(g, half);
                if (c < a.C) {
                    const f32x4 v = {acc[m][4 * g], acc[m][4 * g + 1], acc[m][4 * g + 2], acc[m][4 * g + 3]};
                    *reinterpret_cast<f32x4 *>(dst + c) = v;
                }
            }
    }
}

// General: thread = one element of grad_x.
__global__ __launch_bounds__(256) void conv_bwd_gx_general_kernel(ConvBwdArgs a)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)a.B * a.H * a.W * a.C) return;
    const int c = (int)(i % a.C);
    size_t r = i / a.C;
    const int qx = (int)(r % a.W); r /= a.W;
    const int qy = (int)(r % a.H);
    const int b = (int)(r / a.H);
    const int taps = a.kh * a.kw;
    float acc = 0.f;
    for (int ty = 0; ty < a.kh; ++ty) {
        const int ny = qy + a.ph - ty * a.dh;
        if (ny < 0 || ny % a.sh) continue;
        const int oy = ny / a.sh;
        if (oy >= a.Ho) continue;
        for (int tx = 0; tx < a.kw; ++tx) {
            const int nx = qx + a.pw - tx * a.dw;
            if (nx < 0 || nx % a.sw) continue;
            const int ox = nx / a.sw;
            if (ox >= a.Wo) continue;
            const float *gp = a.gg + ((size_t)(b * a.Ho + oy) * a.Wo + ox) * a.gg_cs;
            const float *wp = a.w + (size_t)c * taps + ty * a.kw + tx;
            for (int o0 = 0; o0 < a.Cout; o0 += 64) {
                float part = 0.f;
                const int o1 = std::min(a.Cout, o0 + 64);
                for (int o = o0; o < o1; ++o) part = fmaf(wp[(size_t)o * a.C * taps], gp[o], part);
                acc += part;
            }
        }
    }
    a.gx[i] = acc;
}

// ---- 3. grad_W ----------------------------------------------------------------------------------------------------------------------
// Matrix cores.  D[o][c] += gg[px][o] x[px*s + tap - p][c], K = pixels.  grid = (input-channel tiles, Cout / 64, splits); block = 192:
// wave w owns slots 3w .. 3w + 2.  3x3: slot = tap, every slot the same 32 input channels; 1x1: slot j = input channels 32 (9 bx + j) ...
// A group of 8 pixels is 4 MFMA steps; slot `half` of step u holds pixel P + 4 half + u for both operands.
__global__ __launch_bounds__(192) void conv_bwd_gw_kernel(ConvBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_g[CB_CHAIN * CB_GP];
    __shared__ __attribute__((aligned(16))) float s_x[CB_SLOTS * CB_CHAIN * CB_XP];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l32 = lane & 31, half = lane >> 5;
    const bool k3 = a.kh == 3;
    const int o0 = blockIdx.y * 64, sp = blockIdx.z;
    const int HWo = a.Ho * a.Wo;
    const auto [q_begin, q_end] = gt_split_range(sp, a.L, a.NPX);
    const int cbase = k3 ? blockIdx.x * 32 : blockIdx.x * 32 * CB_SLOTS;      // first input channel of slot 0
    f32x16 acc[2][3], part[2][3];
    bool live[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) live[j] = k3 || cbase + (3 * wv + j) * 32 < a.C;
    gt_zero(acc);
    for (int Q = q_begin; Q < q_end; Q += CB_CHAIN) {
        if (Q > q_begin) __syncthreads();
        for (int i = tid; i < CB_CHAIN * 16; i += 192) {
            const int v = i & 15, p = i >> 4;
            const int q = Q + p, o = o0 + v * 4;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (q < q_end && o < a.Cout) val = *reinterpret_cast<const f32x4 *>(a.gg + (size_t)q * a.gg_cs + o);
            *reinterpret_cast<f32x4 *>(s_g + p * CB_GP + v * 4) = val;
        }
        for (int i = tid; i < CB_SLOTS * CB_CHAIN * 8; i += 192) {
            const int v = i & 7, p = (i >> 3) & (CB_CHAIN - 1), j = i >> 8;
            const int q = Q + p;
            const int c = cbase + (k3 ? 0 : j * 32) + v * 4;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (q < q_end && c < a.C) {
                const int b = q / HWo, n = q - b * HWo;
                const int oy = n / a.Wo, ox = n - oy * a.Wo;
                const int ty = k3 ? j / 3 : 0, tx = k3 ? j - 3 * ty : 0;
                const int iy = oy * a.sh + ty - a.ph, ix = ox * a.sw + tx - a.pw;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                    val = *reinterpret_cast<const f32x4 *>(a.x + ((size_t)(b * a.H + iy) * a.W + ix) * a.x_cs + c);
            }
            *reinterpret_cast<f32x4 *>(s_x + (j * CB_CHAIN + p) * CB_XP + v * 4) = val;
        }
        __syncthreads();
        gt_zero(part);
#pragma unroll
        for (int g = 0; g < CB_CHAIN / 8; ++g) {
            float av[2][4], bv[3][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = g * 8 + 4 * half + u;
                av[0][u] = s_g[p * CB_GP + l32];
                av[1][u] = s_g[p * CB_GP + 32 + l32];
#pragma unroll
                for (int j = 0; j < 3; ++j) bv[j][u] = s_x[((3 * wv + j) * CB_CHAIN + p) * CB_XP + l32];
            }
            gt_gw_step(part, av, bv, [&](int, int j) { return live[j]; });
        }
        gt_add(acc, part);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int slot = 3 * wv + j;
        const int c = cbase + (k3 ? 0 : slot * 32) + l32;
        if (c >= a.C) continue;
        const size_t tile = k3 ? (size_t)sp * 9 + slot : sp;          // [split][tap][Cout][C] or [split][Cout][C]
#pragma unroll
        for (int m = 0; m < 2; ++m) gt_store_column<true>(a.p_w, tile * a.Cout, acc[m][j], o0 + m * 32, a.Cout, a.C, c, half);
    }
}

// General: thread = one element [o][c][tap] of one split's partial.  grid = (elements / 256, splits).
__global__ __launch_bounds__(256) void conv_bwd_gw_general_kernel(ConvBwdArgs a)
{
    const int taps = a.kh * a.kw;
    const int n = a.Cout * a.C * taps;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int t = e % taps, c = (e / taps) % a.C, o = e / (taps * a.C);
    const int ty = t / a.kw, tx = t - ty * a.kw;
    const int sp = blockIdx.y;
    const int HWo = a.Ho * a.Wo;
    const auto [q_begin, q_end] = gt_split_range(sp, a.L, a.NPX);
    float acc = 0.f;
    for (int q0 = q_begin; q0 < q_end; q0 += CB_CHAIN) {
        float part = 0.f;
        const int q1 = std::min(q_end, q0 + CB_CHAIN);
        for (int q = q0; q < q1; ++q) {
            const int b = q / HWo, r = q - b * HWo;
            const int oy = r / a.Wo, ox = r - oy * a.Wo;
            const int iy = oy * a.sh + ty * a.dh - a.ph, ix = ox * a.sw + tx * a.dw - a.pw;
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                part = fmaf(a.gg[(size_t)q * a.gg_cs + o], a.x[((size_t)(b * a.H + iy) * a.W + ix) * a.x_cs + c], part);
        }
        acc += part;
    }
    a.p_w[(size_t)sp * n + e] = acc;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct CbPlan {
    int Ho, Wo, NPX, S, L, taps, Cpad;
    int V, CG, CGT, P, Sb;
    bool mfma;
    size_t gg, wf, p_w, p_b, total;
};

static bool cb_mfma_takes(int C, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw)
{
    if (dh != 1 || dw != 1 || kh != kw || sh != sw || ph != pw) return false;
    if (C % 16 || Cout % 16 || C > H3D_CONV_BWD_MFMA_CMAX || Cout > H3D_CONV_BWD_MFMA_CMAX) return false;
    return (kh == 3 && ph == 1 && (sh == 1 || sh == 2)) || (kh == 1 && ph == 0 && sh == 1);
}

static int cb_plan(CbPlan &pl, const char *what, int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                   int dh, int dw, int flags)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || Cout <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: non-positive dimension (B %d, C %d, H %d, W %d, Cout %d)", what, B, C, H, W, Cout);
    if (kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0 || ph < 0 || pw < 0)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: kernel %d x %d, stride %d x %d, padding %d x %d, dilation %d x %d", what, kh, kw, sh, sw, ph, pw, dh, dw);
    if (kh > 64 || kw > 64) H3D_FAIL(H3D_ERR_SHAPE, "%s: kernel %d x %d (at most 64 x 64)", what, kh, kw);
    const long long eh = (long long)H + 2 * ph - ((long long)dh * (kh - 1) + 1), ew = (long long)W + 2 * pw - ((long long)dw * (kw - 1) + 1);
    if (eh < 0 || ew < 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: the kernel does not fit the padded input (%d x %d)", what, H, W);
    pl.Ho = (int)(eh / sh) + 1;
    pl.Wo = (int)(ew / sw) + 1;
    const long long lim = 0x7fffffffLL / 256;
    if ((long long)B * H * W > lim || (long long)B * pl.Ho * pl.Wo > lim) H3D_FAIL(H3D_ERR_SHAPE, "%s: %lld pixels", what, (long long)B * H * W);
    if ((long long)C * Cout * kh * kw > lim) H3D_FAIL(H3D_ERR_SHAPE, "%s: %lld filter elements", what, (long long)C * Cout * kh * kw);
    if (flags & ~H3D_CONV_BWD_RELU) H3D_FAIL(H3D_ERR_ARG, "%s: unknown flags %#x", what, flags);
    pl.NPX = B * pl.Ho * pl.Wo;
    pl.taps = kh * kw;
    h3d_split_plan(pl.NPX, CB_SPLIT_PIXELS, CB_SPLIT_MAX, &pl.S, &pl.L);
    pl.mfma = cb_mfma_takes(C, Cout, kh, kw, sh, sw, ph, pw, dh, dw);
    pl.Cpad = cdiv(C, 64) * 64;
    pl.V = Cout % 4 ? 1 : 4;
    pl.CG = Cout / pl.V;
    pl.CGT = std::min(pl.CG, 256);
    pl.P = 256 / pl.CGT;
    pl.Sb = cdiv(pl.NPX, pl.P * CB_CHAIN * CB_BIAS_CHAINS);
    h3d_ws_layout ws;
    pl.gg = ws.take((flags & H3D_CONV_BWD_RELU) ? (size_t)pl.NPX * Cout * 4 : 0);
    pl.wf = ws.take(pl.mfma ? (size_t)pl.taps * Cout * pl.Cpad * 4 : 0);
    pl.p_w = ws.take((size_t)pl.S * pl.taps * Cout * C * 4);
    pl.p_b = ws.take((size_t)pl.Sb * Cout * 4);
    pl.total = ws.total;
    return H3D_OK;
}

extern "C" int h3d_conv2d_backward_workspace_bytes(int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                                                   int dh, int dw, int flags, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "conv2d_backward_workspace_bytes: null pointer");
    *bytes = 0;
    CbPlan pl;
    H3D_TRY(cb_plan(pl, "conv2d_backward_workspace_bytes", B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, flags));
    *bytes = pl.total;
    return H3D_OK;
}

static int cb_run(bool general, const float *x, int x_cs, const float *weight, const float *y, int y_cs, const float *grad_y, int gy_cs,
                  float *grad_x, float *grad_res, float *grad_weight, float *grad_bias, int B, int C, int H, int W, int Cout, int kh, int kw,
                  int sh, int sw, int ph, int pw, int dh, int dw, int flags, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = general ? "conv2d_backward_general" : "conv2d_backward";
    CbPlan pl;
    H3D_TRY(cb_plan(pl, what, B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, flags));
    const bool relu = (flags & H3D_CONV_BWD_RELU) != 0;
    if (x_cs < C || x_cs % 4) H3D_FAIL(H3D_ERR_SHAPE, "%s: x channel stride %d (>= %d channels, a multiple of 4)", what, x_cs, C);
    if (gy_cs < Cout || gy_cs % 4) H3D_FAIL(H3D_ERR_SHAPE, "%s: grad_y channel stride %d (>= %d channels, a multiple of 4)", what, gy_cs, Cout);
    if (relu && (y_cs < Cout || y_cs % 4)) H3D_FAIL(H3D_ERR_SHAPE, "%s: y channel stride %d (>= %d channels, a multiple of 4)", what, y_cs, Cout);
    if (!x || !weight || !grad_y) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", what);
    if (relu && !y) H3D_FAIL(H3D_ERR_ARG, "%s: H3D_CONV_BWD_RELU needs the saved output y", what);
    if (((uintptr_t)x | (uintptr_t)grad_y | (uintptr_t)grad_x | (uintptr_t)grad_res | (relu ? (uintptr_t)y : 0)) & 15)
        H3D_FAIL(H3D_ERR_ARG, "%s: x / y / grad_y / grad_x / grad_res must be 16-byte aligned", what);
    if (((uintptr_t)weight | (uintptr_t)grad_weight | (uintptr_t)grad_bias) & 3)
        H3D_FAIL(H3D_ERR_ARG, "%s: weight / grad_weight / grad_bias must be 4-byte aligned", what);
    if (!grad_x && !grad_res && !grad_weight && !grad_bias) return H3D_OK;
    if (!workspace || workspace_bytes < pl.total || ((uintptr_t)workspace & 255))
        H3D_FAIL(H3D_ERR_ARG, "%s: workspace of %zu bytes, %zu needed (256-byte aligned)", what, workspace ? workspace_bytes : (size_t)0, pl.total);
    hipStream_t st = (hipStream_t)stream;
    const bool mfma = pl.mfma && !general;
    char *ws = (char *)workspace;
    ConvBwdArgs a = {};
    a.x = x; a.w = weight; a.y = y; a.gy = grad_y;
    a.gx = grad_x; a.wf = (float *)(ws + pl.wf); a.p_w = (float *)(ws + pl.p_w);
    a.x_cs = x_cs; a.y_cs = y_cs; a.gy_cs = gy_cs;
    a.B = B; a.C = C; a.H = H; a.W = W; a.Cout = Cout; a.Ho = pl.Ho; a.Wo = pl.Wo;
    a.kh = kh; a.kw = kw; a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw; a.dh = dh; a.dw = dw;
    a.relu = relu; a.Cpad = pl.Cpad;
    a.NPX = pl.NPX; a.S = pl.S; a.L = pl.L;
    a.CG = pl.CG; a.CGT = pl.CGT; a.P = pl.P;
    // 1. gg: materialised once where it is gated or asked for; grad_y itself otherwise
    const bool need_gg = grad_x || grad_weight;
    a.gdst = grad_res ? grad_res : (relu && need_gg) ? (float *)(ws + pl.gg) : nullptr;
    a.p_b = grad_bias ? (float *)(ws + pl.p_b) : nullptr;
    if (a.gdst || a.p_b) {
        if (pl.V == 4) H3D_TRY(h3d_launch({"conv_bwd_gate_kernel", 4}, conv_bwd_gate_kernel<4>, dim3(pl.Sb), dim3(256), 0, st, a));
        else H3D_TRY(h3d_launch({"conv_bwd_gate_kernel", 1}, conv_bwd_gate_kernel<1>, dim3(pl.Sb), dim3(256), 0, st, a));
        if (grad_bias) H3D_TRY(h3d_split_sum(a.p_b, grad_bias, Cout, pl.Sb, st));
    }
    if (a.gdst) { a.gg = a.gdst; a.gg_cs = Cout; }
    else { a.gg = grad_y; a.gg_cs = gy_cs; }
    // 2. grad_x
    if (grad_x) {
        if (mfma) {
            const int n = pl.taps * Cout * pl.Cpad;
            H3D_TRY(h3d_launch({"conv_bwd_pack_kernel"}, conv_bwd_pack_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, weight, a.wf, C, Cout, pl.Cpad, pl.taps));
            a.tiles_y = cdiv(cdiv(H, sh), GT_TH);
            a.tiles_x = cdiv(cdiv(W, sh), GT_TW);
            const dim3 grid(B * a.tiles_x * a.tiles_y, pl.Cpad / 64, sh == 2 ? 4 : 1);
            H3D_TRY(h3d_launch({"conv_bwd_gx_kernel"}, conv_bwd_gx_kernel, grid, dim3(256), 0, st, a));
        } else {
            const size_t n = (size_t)B * H * W * C;
            H3D_TRY(h3d_launch({"conv_bwd_gx_general_kernel"}, conv_bwd_gx_general_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a));
        }
    }
    // 3. grad_W
    if (grad_weight) {
        const size_t n = (size_t)pl.taps * Cout * C;
        if (mfma) {
            const dim3 grid(kh == 3 ? cdiv(C, 32) : cdiv(C, 32 * CB_SLOTS), cdiv(Cout, 64), pl.S);
            H3D_TRY(h3d_launch({"conv_bwd_gw_kernel"}, conv_bwd_gw_kernel, grid, dim3(192), 0, st, a));
            if (kh == 3) H3D_TRY(h3d_split_sum(a.p_w, grad_weight, n, pl.S, st, Cout, C));        // [tap][o][c] -> the reference's [o][c][tap]
            else H3D_TRY(h3d_split_sum(a.p_w, grad_weight, n, pl.S, st));
        } else {
            H3D_TRY(h3d_launch({"conv_bwd_gw_general_kernel"}, conv_bwd_gw_general_kernel, dim3((unsigned)((n + 255) / 256), pl.S), dim3(256), 0, st, a));
            H3D_TRY(h3d_split_sum(a.p_w, grad_weight, n, pl.S, st));
        }
    }
    return H3D_OK;
}

extern "C" int h3d_conv2d_backward(const float *x, int x_cs, const float *weight, const float *y, int y_cs, const float *grad_y, int gy_cs,
                                   float *grad_x, float *grad_res, float *grad_weight, float *grad_bias, int B, int C, int H, int W, int Cout,
                                   int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int flags, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    return cb_run(false, x, x_cs, weight, y, y_cs, grad_y, gy_cs, grad_x, grad_res, grad_weight, grad_bias, B, C, H, W, Cout, kh, kw, sh, sw,
                  ph, pw, dh, dw, flags, workspace, workspace_bytes, stream);
}

extern "C" int h3d_conv2d_backward_general(const float *x, int x_cs, const float *weight, const float *y, int y_cs, const float *grad_y,
                                           int gy_cs, float *grad_x, float *grad_res, float *grad_weight, float *grad_bias, int B, int C, int H,
                                           int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int flags,
                                           void *workspace, size_t workspace_bytes, void *stream)
{
    return cb_run(true, x, x_cs, weight, y, y_cs, grad_y, gy_cs, grad_x, grad_res, grad_weight, grad_bias, B, C, H, W, Cout, kh, kw, sh, sw,
                  ph, pw, dh, dw, flags, workspace, workspace_bytes, stream);
}
