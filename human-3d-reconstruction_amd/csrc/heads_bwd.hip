// Output heads BACKWARD on gfx950: the gradients of csrc/heads.hip's operator (reference models/model.py:451-464, 485-489),
//     z = W2 relu(conv3x3(y, W1) + b1) + b2      per head,
// at the parameters of every head and at the feature map y.  With pre = conv3x3(y, W1) + b1, h = relu(pre), gz = dL/dz:
//     gb2 = sum_px gz                      gW2[k,o]   = sum_px gz[k,px] h[o,px]
//     gh  = (W2^T gz) * [pre > 0]          gb1        = sum_px gh
//     gW1[o,c,t] = sum_px gh[o,px] y[c,px+t]   (zero padding)
//     gy[c,q]    = sum_{o,t} W1[o,c,t] gh[o,q-t],  summed over the heads
// ReLU convention: gradient 0 where pre <= 0 (torch.relu's).
//
// fp32 storage, fp32 accumulation, every contraction on v_mfma_f32_32x32x2_f32 (exact fmaf chains).  No float atomics: every output
// is a sum in a fixed order and bit-identical from run to run, whichever other outputs are requested.
//
// Per head, in head order (the workspace buffers are reused from head to head):
//   1. heads_bwd_pack_kernel   W1 -> the A-operand images of the recompute (rows = o) and of the gather-form gy (rows = c, taps flipped)
//   2. heads_bwd_gh_kernel     workgroup = 4 x 32 pixel tile, wave = one row of it.  The 64-channel halo tile of y sits in LDS (the
//                              forward's tile); per slab of 64 intermediate channels: pre on the matrix cores, W2^T gz on the matrix
//                              cores into a second accumulator set of the SAME C/D layout (lane = pixel), gate, and gh / h leave as
//                              16-byte NHWC stores to the workspace.
//   3. heads_bwd_gy_kernel     the same tile and the same contraction (heads_bwd_conv), 3x3 over gh with the flipped filters, head_conv -> 64,
//                              64 channels of gh halo at a time through LDS.  The one workgroup that owns a pixel tile writes (first
//                              live head) or load-add-stores (later heads) grad_feat.
//   4. heads_bwd_w1_kernel / heads_bwd_w2_kernel / heads_bwd_bias_kernel   K = pixels: one split of the B*H*W pixels per workgroup,
//                              partials to the workspace, then h3d_split_sum_kernel (csrc/split_sum.h) sums them in split order.
// The tile, its halo, the tap and K = pixels contractions, the C/D layout and the split plan are csrc/grad_tile.h's, shared with
// csrc/conv_bwd.hip and csrc/dcn_bwd.hip.
#include "common.h"
#include "grad_tile.h"
#include "split_sum.h"
#include <algorithm>

constexpr int HB_SPLIT_PIXELS = 512;              // pixels per split of the K = pixels contractions, at least
constexpr int HB_SPLIT_MAX = 64;                  // splits, at most
constexpr int HB_CMAX = 96;
constexpr int HB_CHAIN = 32;                      // pixels per fmaf chain of the K = pixels contractions (chain sums are added in order)

struct HeadsBwdArgs {
    const float *feat;      // NHWC [B,H,W,in_cs], 64 channels used
    const float *w1, *b1, *w2, *gz;
    float *w1p;             // [9][8][2][hc][4]:     w1p[t][k8][half][o][s] = W1[o][k8*8 + half*4 + s][t]
    float *w1f;             // [9][hc/8][2][64][4]:  w1f[t][o8][half][c][s] = W1[o8*8 + half*4 + s][c][8 - t]
    float *gh, *hh;         // [B*H*W][hc]
    float *gy;              // [B*H*W][64] or null
    float *p_w1, *p_w2, *p_b1, *p_b2;   // partials: [S][9][hc][64], [S][C][hc], [S][hc], [S][C]
    int gy_add, want_gh, want_h;
    int in_cs, B, H, W, hc, C;
    int tiles_x, tiles_y;
    int NPX, S, L;
};

__global__ void heads_bwd_pack_kernel(const float *__restrict__ w1, float *__restrict__ w1p, float *__restrict__ w1f, int hc)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = 576 * hc;
    if (i >= n) return;
    const int s = i & 3;
    int r = i >> 2;
    const int o = r % hc; r /= hc;
    const int half = r & 1; r >>= 1;
    const int k8 = r & 7, t = r >> 3;
    w1p[i] = w1[((size_t)o * 64 + k8 * 8 + half * 4 + s) * 9 + t];
    w1f[i] = gt_filter_image(w1, i, 64, hc, 64, 9, true);
}

// acc[m] += sum over the 9 taps and 64 K channels of  A[m*32 + row][k, tap] . halo[pixel + tap][k]   (two 32-row tiles, 32 pixels).
// A operand: a packed image wp[tap][k8][half][M][4] at rows m0 + {0, 32} + l32 (gt_tap_mfma).  B operand: the lane's halo pixel.
// Summation order: one fmaf chain of 64 terms per tap, the nine tap sums added in tap order -- a single chain of 576 terms carries about
// twice the rounding error of the blocked sums a CPU convolution makes, which is what the gradients are measured against.
__device__ __forceinline__ void heads_bwd_conv(f32x16 (&acc)[2], const float *__restrict__ wp, int M, int m0, int kg_total, int kg0,
                                               const float *s_halo, int row, int l32, int half)
{
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3, dx = t - 3 * dy;
        const float *bp = s_halo + ((row + dy) * GT_IW + l32 + dx) * GT_PS + half * 4;
        const f32x4 *ap = reinterpret_cast<const f32x4 *>(wp) + ((size_t)(t * kg_total + kg0) * 2 + half) * M + m0 + l32;
        gt_tap_mfma(acc, ap, M, bp, 8);
    }
}

__global__ __launch_bounds__(256) void heads_bwd_gh_kernel(HeadsBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_halo[GT_IH * GT_IW * GT_PS];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, l32 = lane & 31, half = lane >> 5;
    const int tiles = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int oy0 = ty * GT_TH, ox0 = tx * GT_TW;
    gt_stage_halo(s_halo, a.feat, a.in_cs, 0, b, a.H, a.W, oy0 - 1, ox0 - 1, GT_IH, GT_IW, 16, tid);
    __syncthreads();
    const int oy = oy0 + wv, ox = ox0 + l32;
    const bool valid = oy < a.H && ox < a.W;
    const size_t HW = (size_t)a.H * a.W;
    const size_t pix = ((size_t)b * a.H + oy) * a.W + ox;
    const float *gzp = a.gz + (size_t)b * a.C * HW + (size_t)oy * a.W + ox;
    const int k2n = (a.C + 1) >> 1;
    for (int sl = 0; sl < a.hc / 64; ++sl) {
        f32x16 acc[2], acc2[2];
        gt_zero(acc);
        gt_zero(acc2);
        heads_bwd_conv(acc, a.w1p, a.hc, sl * 64, 8, 0, s_halo, wv, l32, half);
        // W2^T gz: rows = o, K = the head's channels (slot `half` of step k2 is channel 2 k2 + half), columns = pixels
        const float *w2p = a.w2 + sl * 64 + l32;
        for (int k2 = 0; k2 < k2n; ++k2) {
            const int k = 2 * k2 + half;
            const bool kok = k < a.C;
            const float a0 = kok ? w2p[(size_t)k * a.hc] : 0.f, a1 = kok ? w2p[(size_t)k * a.hc + 32] : 0.f;
            const float bv = (kok && valid) ? gzp[(size_t)k * HW] : 0.f;
            acc2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc2[0], 0, 0, 0);
            acc2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc2[1], 0, 0, 0);
        }
        if (valid) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int o = sl * 64 + m * 32 + gt_row4(g, half);
                    const f32x4 b1v = *reinterpret_cast<const f32x4 *>(a.b1 + o);
                    f32x4 gv, hv;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float pre = acc[m][4 * g + i] + b1v[i];
                        const bool on = pre > 0.f;
                        hv[i] = on ? pre : 0.f;
                        gv[i] = on ? acc2[m][4 * g + i] : 0.f;
                    }
                    if (a.want_gh) *reinterpret_cast<f32x4 *>(a.gh + pix * a.hc + o) = gv;
                    if (a.want_h) *reinterpret_cast<f32x4 *>(a.hh + pix * a.hc + o) = hv;
                }
        }
    }
}

__global__ __launch_bounds__(256) void heads_bwd_gy_kernel(HeadsBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_halo[GT_IH * GT_IW * GT_PS];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, l32 = lane & 31, half = lane >> 5;
    const int tiles = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int oy0 = ty * GT_TH, ox0 = tx * GT_TW;
    // per 64-channel chunk of gh its own sum (nine tap sums, see heads_bwd_conv), the chunk sums added in chunk order
    f32x16 acc[2];
    gt_zero(acc);
    for (int ch = 0; ch < a.hc / 64; ++ch) {
        if (ch) __syncthreads();
        gt_stage_halo(s_halo, a.gh, a.hc, ch * 64, b, a.H, a.W, oy0 - 1, ox0 - 1, GT_IH, GT_IW, 16, tid);
        __syncthreads();
        f32x16 part[2];
        gt_zero(part);
        heads_bwd_conv(part, a.w1f, 64, 0, a.hc / 8, ch * 8, s_halo, wv, l32, half);
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[m] = ch ? acc[m] + part[m] : part[m];
    }
    const int oy = oy0 + wv, ox = ox0 + l32;
    if (oy < a.H && ox < a.W) {
        float *dst = a.gy + (((size_t)b * a.H + oy) * a.W + ox) * 64;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 *p = reinterpret_cast<f32x4 *>(dst + m * 32 + gt_row4(g, half));
                f32x4 v = {acc[m][4 * g], acc[m][4 * g + 1], acc[m][4 * g + 2], acc[m][4 * g + 3]};
                if (a.gy_add) { const f32x4 old = *p; v = old + v; }
                *p = v;
            }
    }
}

// gW1 partials: D[o][c] += gh[px][o] y[px + tap][c] per tap, K = pixels.  Workgroup = 3 waves = the 3 kernel rows (3 taps each) x one
// tile of 32 input channels x 64 intermediate channels x one split of the pixels: gt_gw_pixels with both operands from global memory.
__global__ __launch_bounds__(192) void heads_bwd_w1_kernel(HeadsBwdArgs a)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l32 = lane & 31, half = lane >> 5;
    const int c = blockIdx.x * 32 + l32, o0 = blockIdx.y * 64, sp = blockIdx.z;
    const int HW = a.H * a.W;
    const auto [q_begin, q_end] = gt_split_range(sp, a.L, a.NPX);
    f32x16 acc[2][3];
    // (summation order: chains of HB_CHAIN pixels, the chain sums added in pixel order)
    gt_gw_pixels<HB_CHAIN>(acc, q_begin, q_end, half, true, [&](int q, bool ok, int s, float (&av)[2][4], float (&bv)[3][4]) {
        const float *gp = a.gh + (size_t)q * a.hc + o0 + l32;
        av[0][s] = ok ? gp[0] : 0.f;
        av[1][s] = ok ? gp[32] : 0.f;
        const int b = ok ? q / HW : 0, n = ok ? q - b * HW : 0;
        const int y = n / a.W, x = n - y * a.W;
        const int yy = y + wv - 1;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int xx = x + j - 1;
            bv[j][s] = (ok && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) ? a.feat[((size_t)(b * a.H + yy) * a.W + xx) * a.in_cs + c] : 0.f;
        }
    });
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            gt_store_column<false>(a.p_w1, ((size_t)sp * 9 + (3 * wv + j)) * a.hc, acc[m][j], o0 + m * 32, a.hc, 64, c, half);
}

// gW2 partials: D[k][o] += gz[k][px] h[px][o], K = pixels.  One wave = all (up to 96) channels k x 32 intermediate channels x one split.
__global__ __launch_bounds__(64) void heads_bwd_w2_kernel(HeadsBwdArgs a)
{
    const int lane = threadIdx.x, l32 = lane & 31, half = lane >> 5;
    const int o = blockIdx.x * 32 + l32, sp = blockIdx.y;
    const int HW = a.H * a.W;
    const auto [q_begin, q_end] = gt_split_range(sp, a.L, a.NPX);
    const int mt = (a.C + 31) >> 5;
    f32x16 acc[3], part[3];
    gt_zero(acc);
    for (int P = q_begin; P < q_end; P += 8) {
        if ((P - q_begin) % HB_CHAIN == 0) gt_chain_next(acc, part, P > q_begin);
        float av[3][4], bv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int q = P + 4 * half + s;
            const bool ok = q < q_end;
            bv[s] = ok ? a.hh[(size_t)q * a.hc + o] : 0.f;
            const int b = ok ? q / HW : 0, n = ok ? q - b * HW : 0;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int k = m * 32 + l32;
                av[m][s] = (ok && k < a.C) ? a.gz[((size_t)b * a.C + k) * HW + n] : 0.f;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][s], bv[s], part[0], 0, 0, 0);
            if (mt > 1) part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][s], bv[s], part[1], 0, 0, 0);
            if (mt > 2) part[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2][s], bv[s], part[2], 0, 0, 0);
        }
    }
    gt_add(acc, part);
#pragma unroll
    for (int m = 0; m < 3; ++m) gt_store_column<true>(a.p_w2, (size_t)sp * a.C, acc[m], m * 32, a.C, a.hc, o, half);
}

// gb1 / gb2 partials of one split: gb1 thread = intermediate channel, pixels in order (chains of HB_CHAIN); gb2 wave = channel, lanes stride over the
// pixels and meet in a fixed butterfly.
__global__ __launch_bounds__(256) void heads_bwd_bias_kernel(HeadsBwdArgs a, int want_b1, int want_b2)
{
    const int tid = threadIdx.x, sp = blockIdx.x;
    const int HW = a.H * a.W;
    const auto [q_begin, q_end] = gt_split_range(sp, a.L, a.NPX);
    if (want_b1 && tid < a.hc) {
        float v = 0.f;
        for (int q0 = q_begin; q0 < q_end; q0 += HB_CHAIN) {
            float c = 0.f;
            const int q1 = std::min(q_end, q0 + HB_CHAIN);
            for (int q = q0; q < q1; ++q) c += a.gh[(size_t)q * a.hc + tid];
            v += c;
        }
        a.p_b1[(size_t)sp * a.hc + tid] = v;
    }
    if (want_b2) {
        const int wv = tid >> 6, lane = tid & 63;
        for (int k = wv; k < a.C; k += 4) {
            float v = 0.f;
            for (int q = q_begin + lane; q < q_end; q += 64) {
                const int b = q / HW, n = q - b * HW;
                v += a.gz[((size_t)b * a.C + k) * HW + n];
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
            if (lane == 0) a.p_b2[(size_t)sp * a.C + k] = v;
        }
    }
}

// the splits of the K = pixels contractions and the workspace: the two packed images of W1, gh, h, the four sets of partials
struct HbPlan {
    int NPX, S, L;
    size_t w1p, w1f, gh, hh, p_w1, p_w2, p_b1, p_b2, total;
};

static int hb_check(const char *what, int B, int H, int W, int head_conv, int nheads)
{
    if (B <= 0 || H <= 0 || W <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: non-positive dimension %d x %d x %d", what, B, H, W);
    if ((long long)B * H * W > 0x7fffffffLL / 256) H3D_FAIL(H3D_ERR_SHAPE, "%s: %lld pixels", what, (long long)B * H * W);
    if (head_conv <= 0 || head_conv % 64 || head_conv > 256)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: head_conv %d must be a multiple of 64, at most 256", what, head_conv);
    if (nheads < 0 || nheads > H3D_HEADS_MAX) H3D_FAIL(H3D_ERR_SHAPE, "%s: %d heads (max %d)", what, nheads, H3D_HEADS_MAX);
    return H3D_OK;
}

static void hb_plan(HbPlan &pl, int B, int H, int W, int hc)
{
    pl.NPX = B * H * W;
    h3d_split_plan(pl.NPX, HB_SPLIT_PIXELS, HB_SPLIT_MAX, &pl.S, &pl.L);
    h3d_ws_layout ws;
    pl.w1p = ws.take((size_t)576 * hc * 4);
    pl.w1f = ws.take((size_t)576 * hc * 4);
    pl.gh = ws.take((size_t)pl.NPX * hc * 4);
    pl.hh = ws.take((size_t)pl.NPX * hc * 4);
    pl.p_w1 = ws.take((size_t)pl.S * 576 * hc * 4);
    pl.p_w2 = ws.take((size_t)pl.S * HB_CMAX * hc * 4);
    pl.p_b1 = ws.take((size_t)pl.S * hc * 4);
    pl.p_b2 = ws.take((size_t)pl.S * HB_CMAX * 4);
    pl.total = ws.total;
}

extern "C" int h3d_heads_backward_workspace_bytes(int B, int H, int W, int head_conv, int nheads, const int *C, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "heads_backward_workspace_bytes: null pointer");
    *bytes = 0;
    int rc = hb_check("heads_backward_workspace_bytes", B, H, W, head_conv, nheads);
    if (rc != H3D_OK) return rc;
    if (nheads > 0 && !C) H3D_FAIL(H3D_ERR_ARG, "heads_backward_workspace_bytes: null pointer");
    for (int i = 0; i < nheads; ++i)
        if (C[i] < 1 || C[i] > HB_CMAX)
            H3D_FAIL(H3D_ERR_UNSUPPORTED, "heads_backward_workspace_bytes: head %d has %d channels (1 to %d)", i, C[i], HB_CMAX);
    HbPlan pl;
    hb_plan(pl, B, H, W, head_conv);
    *bytes = pl.total;
    return H3D_OK;
}

extern "C" int h3d_heads_backward(const float *feat, int in_cs, int B, int H, int W, int head_conv, int nheads, const h3d_heads_bwd_head *heads,
                                  float *grad_feat, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!feat || !heads) H3D_FAIL(H3D_ERR_ARG, "heads_backward: null pointer");
    int rc = hb_check("heads_backward", B, H, W, head_conv, nheads);
    if (rc != H3D_OK) return rc;
    if (in_cs < 64 || in_cs % 4) H3D_FAIL(H3D_ERR_SHAPE, "heads_backward: input must have 64 channels (channel stride %d, a multiple of 4)", in_cs);
    if (((uintptr_t)feat | (uintptr_t)grad_feat) & 15) H3D_FAIL(H3D_ERR_ARG, "heads_backward: feat / grad_feat must be 16-byte aligned");
    bool live = false;
    for (int i = 0; i < nheads; ++i) {
        const h3d_heads_bwd_head &h = heads[i];
        if (h.C < 1 || h.C > HB_CMAX) H3D_FAIL(H3D_ERR_UNSUPPORTED, "heads_backward: head %d has %d channels (1 to %d)", i, h.C, HB_CMAX);
        if (!h.grad_out) continue;
        if (!h.w1 || !h.b1 || !h.w2) H3D_FAIL(H3D_ERR_ARG, "heads_backward: head %d null pointer", i);
        if (((uintptr_t)h.b1) & 15) H3D_FAIL(H3D_ERR_ARG, "heads_backward: head %d b1 must be 16-byte aligned", i);
        live = true;
    }
    HbPlan pl;
    hb_plan(pl, B, H, W, head_conv);
    if (live && (!workspace || workspace_bytes < pl.total))
        H3D_FAIL(H3D_ERR_ARG, "heads_backward: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, pl.total);
    hipStream_t st = (hipStream_t)stream;
    if (!live) {
        if (grad_feat && hipMemsetAsync(grad_feat, 0, (size_t)pl.NPX * 64 * 4, st) != hipSuccess) H3D_FAIL(H3D_ERR_LAUNCH, "heads_backward: memset");
        return H3D_OK;
    }
    HeadsBwdArgs a = {};
    char *ws = (char *)workspace;
    a.w1p = (float *)(ws + pl.w1p); a.w1f = (float *)(ws + pl.w1f);
    a.gh = (float *)(ws + pl.gh); a.hh = (float *)(ws + pl.hh);
    a.p_w1 = (float *)(ws + pl.p_w1); a.p_w2 = (float *)(ws + pl.p_w2);
    a.p_b1 = (float *)(ws + pl.p_b1); a.p_b2 = (float *)(ws + pl.p_b2);
    a.feat = feat; a.in_cs = in_cs; a.B = B; a.H = H; a.W = W; a.hc = head_conv;
    a.tiles_x = cdiv(W, GT_TW); a.tiles_y = cdiv(H, GT_TH);
    a.NPX = pl.NPX; a.S = pl.S; a.L = pl.L;
    a.gy = grad_feat;
    const int hc = head_conv;
    const dim3 tile_grid(B * a.tiles_x * a.tiles_y);
    bool first = true;
    for (int i = 0; i < nheads; ++i) {
        const h3d_heads_bwd_head &h = heads[i];
        if (!h.grad_out) continue;
        a.w1 = h.w1; a.b1 = h.b1; a.w2 = h.w2; a.gz = h.grad_out; a.C = h.C;
        a.want_gh = grad_feat || h.grad_w1 || h.grad_b1;
        a.want_h = h.grad_w2 != nullptr;
        if (a.want_gh || a.want_h) {
            H3D_TRY(h3d_launch({"heads_bwd_pack_kernel"}, heads_bwd_pack_kernel, dim3(cdiv(576 * hc, 256)), dim3(256), 0, st, h.w1, a.w1p, a.w1f, hc));
            H3D_TRY(h3d_launch({"heads_bwd_gh_kernel"}, heads_bwd_gh_kernel, tile_grid, dim3(256), 0, st, a));
        }
        if (grad_feat) {
            a.gy_add = first ? 0 : 1;
            H3D_TRY(h3d_launch({"heads_bwd_gy_kernel"}, heads_bwd_gy_kernel, tile_grid, dim3(256), 0, st, a));
            first = false;
        }
        if (h.grad_w1) {
            H3D_TRY(h3d_launch({"heads_bwd_w1_kernel"}, heads_bwd_w1_kernel, dim3(2, hc / 64, pl.S), dim3(192), 0, st, a));
            H3D_TRY(h3d_split_sum(a.p_w1, h.grad_w1, (size_t)576 * hc, pl.S, st, hc, 64));       // [tap][o][c] -> the reference's [o][c][tap]
        }
        if (h.grad_w2) {
            H3D_TRY(h3d_launch({"heads_bwd_w2_kernel"}, heads_bwd_w2_kernel, dim3(hc / 32, pl.S), dim3(64), 0, st, a));
            H3D_TRY(h3d_split_sum(a.p_w2, h.grad_w2, (size_t)h.C * hc, pl.S, st));
        }
        if (h.grad_b1 || h.grad_b2) {
            H3D_TRY(h3d_launch({"heads_bwd_bias_kernel"}, heads_bwd_bias_kernel, dim3(pl.S), dim3(256), 0, st, a, h.grad_b1 ? 1 : 0, h.grad_b2 ? 1 : 0));
            if (h.grad_b1) H3D_TRY(h3d_split_sum(a.p_b1, h.grad_b1, hc, pl.S, st));
            if (h.grad_b2) H3D_TRY(h3d_split_sum(a.p_b2, h.grad_b2, h.C, pl.S, st));
        }
    }
    return H3D_OK;
}
