// Backward of the two DLA-34 operators that had none (include/h3d.h section 2d): Tree.downsample's 2x2 max-pool (H3D_OP_MAXPOOL) and
// IDAUp's depthwise ConvTranspose2d(k = 2f, s = f, p = f/2) + skip add (H3D_OP_UPADD).  fp32 NHWC with a channel stride, no float atomics:
// every output element is written once, as a sum in a fixed order.
#include "common.h"
#include "split_sum.h"

#include <algorithm>
#include <math.h>

// ---- max-pool -------------------------------------------------------------------------------------------------------------------------
// thread = one 2x2 window x 4 channels: four 16-byte loads of x, one of grad_y, four 16-byte stores.  The windows cover ceil(H/2) x
// ceil(W/2), so the last row / column of an odd H / W belongs to a window without an output pixel and gets 0.
// Tie rule = torch's CPU max_pool2d: scan (0,0), (0,1), (1,0), (1,1) from -inf, move on `v > m || isnan(v)`: the first of equal maxima.
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float *__restrict__ x, const float *__restrict__ gy, float *__restrict__ gx,
                                                           int B, int C, int H, int W, int x_cs, int gy_cs, int gx_cs)
{
    const int vpc = C / 4, Hc = (H + 1) / 2, Wc = (W + 1) / 2, Ho = H / 2, Wo = W / 2;
    const size_t total = (size_t)B * Hc * Wc * vpc;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int v = (int)(i % vpc);
    const size_t p = i / vpc;
    const int wx = (int)(p % Wc);
    const size_t q = p / Wc;
    const int wy = (int)(q % Hc), b = (int)(q / Hc);
    const int iy = 2 * wy, ix = 2 * wx;
    const bool full = wy < Ho && wx < Wo;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 o[4] = {zero, zero, zero, zero};
    if (full) {
        f32x4 xv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            xv[j] = *reinterpret_cast<const f32x4 *>(x + (((size_t)b * H + iy + (j >> 1)) * W + ix + (j & 1)) * x_cs + 4 * v);
        const f32x4 g = *reinterpret_cast<const f32x4 *>(gy + (((size_t)b * Ho + wy) * Wo + wx) * gy_cs + 4 * v);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            float m = -INFINITY;
            int at = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float val = xv[j][n];
                if (val > m || isnan(val)) { m = val; at = j; }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j][n] = at == j ? g[n] : 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = iy + (j >> 1), xx = ix + (j & 1);
        if (y < H && xx < W) *reinterpret_cast<f32x4 *>(gx + (((size_t)b * H + y) * W + xx) * gx_cs + 4 * v) = o[j];
    }
}

static int check_cs(const char *what, const char *name, int cs, int C)
{
    if (cs < C || cs % 4) H3D_FAIL(H3D_ERR_SHAPE, "%s: %s channel stride %d (>= %d channels, a multiple of 4)", what, name, cs, C);
    return H3D_OK;
}

extern "C" int h3d_maxpool2_backward(const float *x, int x_cs, const float *grad_y, int gy_cs, float *grad_x, int gx_cs, int B, int C, int H,
                                     int W, void *stream)
{
    const char *what = "maxpool2_backward";
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: non-positive dimension (B %d, C %d, H %d, W %d)", what, B, C, H, W);
    if (C % 4) H3D_FAIL(H3D_ERR_SHAPE, "%s: C = %d is no multiple of 4", what, C);
    if ((long long)B * H * W > 0x7fffffffLL / 4) H3D_FAIL(H3D_ERR_SHAPE, "%s: %lld pixels", what, (long long)B * H * W);
    H3D_TRY(check_cs(what, "x", x_cs, C));
    H3D_TRY(check_cs(what, "grad_y", gy_cs, C));
    H3D_TRY(check_cs(what, "grad_x", gx_cs, C));
    const bool has_out = H >= 2 && W >= 2;         // (otherwise grad_y has no element and is not read)
    if (!x || (has_out && !grad_y)) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", what);
    if (((uintptr_t)x | (uintptr_t)grad_y | (uintptr_t)grad_x) & 15) H3D_FAIL(H3D_ERR_ARG, "%s: x / grad_y / grad_x must be 16-byte aligned", what);
    if (!grad_x) return H3D_OK;
    const size_t total = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
    return h3d_launch({"maxpool2_bwd_kernel"}, maxpool2_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                      grad_y, grad_x, B, C, H, W, x_cs, gy_cs, gx_cs);
}

// ---- up-sample + add --------------------------------------------------------------------------------------------------------------------
// y[oy,ox,c] = skip[oy,ox,c] + sum_{ki,kj} w[ki,kj,c] x[iy,ix,c] over oy = iy f - p + ki, ox = ix f - p + kj (k = 2f taps a side, p = f/2), so
//     grad_x[iy,ix,c]  = sum_{ki,kj} w[ki,kj,c] gy[iy f - p + ki, ix f - p + kj, c]
//     grad_w[ki,kj,c]  = sum_{b,iy,ix} x[b,iy,ix,c] gy[b, iy f - p + ki, ix f - p + kj, c]
// and grad_skip = gy.  Workgroup = TH x TW input pixels x CS channels of one image.  It stages the (TH + 1) f x (TW + 1) f window of grad_y
// that these pixels' taps cover (out-of-range positions as exact zeros) into LDS once and forms from it
//   - grad_x: item = (pixel, 4 channels, one of R groups of 2f / R kernel rows); an fmaf chain over the group's taps in (ki, kj) order; with
//     R > 1 the group sums meet in LDS and are added in group order.  R = 1, 2, 16 for f = 2, 4, 8: chains of 16, 32, 16 terms;
//   - its grad_w partial: item = (tap, 4 channels), an fmaf chain over the tile's in-range pixels in row-major order (at most 64 terms),
//     stored to slot (b, tile) of the workspace.  h3d_split_sum_kernel adds the slots (below).
// LDS pixels are CS + 4 floats apart (upadd_kernel's skew, csrc/conv.hip): neighbouring pixels of a wave read taps f pixels apart, and at a
// pitch of CS floats (128 B) every second one would sit on the same banks.
template <int F> struct UpBwd;
template <> struct UpBwd<2> { static constexpr int TH = 8, TW = 8, CS = 32; };
template <> struct UpBwd<4> { static constexpr int TH = 4, TW = 4, CS = 32; };
template <> struct UpBwd<8> { static constexpr int TH = 2, TW = 2, CS = 16; };

struct UpBwdArgs {
    const float *x, *w, *gy;
    float *gx, *pw;
    int x_cs, gy_cs, gx_cs;
    int B, C, H, W, tiles_x;
};

static __device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c)
{
    return f32x4{fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w)};
}

template <int F>
__global__ __launch_bounds__(256) void up_bwd_kernel(UpBwdArgs a)
{
    using K = UpBwd<F>;
    constexpr int TH = K::TH, TW = K::TW, CS = K::CS, V = CS / 4, PP = CS + 4, WH = (TH + 1) * F, WW = (TW + 1) * F, KK = 2 * F, P = F / 2;
    constexpr int ITEMS = TH * TW * V;
    constexpr int R = ITEMS >= 256 ? 1 : 256 / ITEMS;
    static_assert((ITEMS * R) % 256 == 0 && KK % R == 0, "grad_x items fill whole passes of the workgroup");
    __shared__ __attribute__((aligned(16))) float s_g[WH * WW * PP];
    __shared__ __attribute__((aligned(16))) float s_x[TH * TW * CS];
    __shared__ __attribute__((aligned(16))) float s_p[R > 1 ? R * ITEMS * 4 : 4];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
    const int c0 = blockIdx.y * CS, b = blockIdx.z;
    const int iy0 = tyi * TH, ix0 = txi * TW;
    const int Ho = a.H * F, Wo = a.W * F;
    const int oy0 = iy0 * F - P, ox0 = ix0 * F - P;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < WH * WW * V; i += 256) {
        const int v = i % V, px = i / V, wx = px % WW, wy = px / WW;
        const int oy = oy0 + wy, ox = ox0 + wx, c = c0 + 4 * v;
        f32x4 g = zero;
        if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo && c < a.C)
            g = *reinterpret_cast<const f32x4 *>(a.gy + (((size_t)b * Ho + oy) * Wo + ox) * a.gy_cs + c);
        *reinterpret_cast<f32x4 *>(s_g + px * PP + 4 * v) = g;
    }
    if (a.pw) {
        for (int i = tid; i < ITEMS; i += 256) {
            const int v = i % V, px = i / V, tx = px % TW, ty = px / TW;
            const int iy = iy0 + ty, ix = ix0 + tx, c = c0 + 4 * v;
            f32x4 xv = zero;
            if (iy < a.H && ix < a.W && c < a.C) xv = *reinterpret_cast<const f32x4 *>(a.x + (((size_t)b * a.H + iy) * a.W + ix) * a.x_cs + c);
            *reinterpret_cast<f32x4 *>(s_x + px * CS + 4 * v) = xv;
        }
    }
    __syncthreads();
    if (a.gx) {
        for (int i0 = 0; i0 < ITEMS * R; i0 += 256) {
            const int i = i0 + tid;
            const int it = i % ITEMS, r = i / ITEMS;
            const int v = it % V, px = it / V, tx = px % TW, ty = px / TW;
            const int c = c0 + 4 * v;
            f32x4 acc = zero;
            if (c < a.C) {
                for (int ki = r * (KK / R); ki < (r + 1) * (KK / R); ++ki) {
                    const float *wrow = a.w + (size_t)ki * KK * a.C + c;
                    const float *grow = s_g + ((ty * F + ki) * WW + tx * F) * PP + 4 * v;
#pragma unroll
                    for (int kj = 0; kj < KK; ++kj)
                        acc = fma4(*reinterpret_cast<const f32x4 *>(wrow + (size_t)kj * a.C), *reinterpret_cast<const f32x4 *>(grow + kj * PP), acc);
                }
            }
            if constexpr (R == 1) {
                const int iy = iy0 + ty, ix = ix0 + tx;
                if (iy < a.H && ix < a.W && c < a.C) *reinterpret_cast<f32x4 *>(a.gx + (((size_t)b * a.H + iy) * a.W + ix) * a.gx_cs + c) = acc;
            } else {
                *reinterpret_cast<f32x4 *>(s_p + (r * ITEMS + it) * 4) = acc;
            }
        }
        if constexpr (R > 1) {
            __syncthreads();
            if (tid < ITEMS) {
                const int v = tid % V, px = tid / V, tx = px % TW, ty = px / TW;
                const int iy = iy0 + ty, ix = ix0 + tx, c = c0 + 4 * v;
                f32x4 acc = *reinterpret_cast<const f32x4 *>(s_p + tid * 4);
                for (int r = 1; r < R; ++r) acc += *reinterpret_cast<const f32x4 *>(s_p + (r * ITEMS + tid) * 4);
                if (iy < a.H && ix < a.W && c < a.C) *reinterpret_cast<f32x4 *>(a.gx + (((size_t)b * a.H + iy) * a.W + ix) * a.gx_cs + c) = acc;
            }
        }
    }
    if (a.pw) {
        float *dst = a.pw + ((size_t)b * gridDim.x + tile) * (KK * KK) * a.C;
        const int th = min(TH, a.H - iy0), tw = min(TW, a.W - ix0);
        for (int i = tid; i < KK * KK * V; i += 256) {
            const int v = i % V, t = i / V, kj = t % KK, ki = t / KK;
            const int c = c0 + 4 * v;
            if (c >= a.C) continue;
            f32x4 acc = zero;
            for (int ty = 0; ty < th; ++ty)
                for (int tx = 0; tx < tw; ++tx)
                    acc = fma4(*reinterpret_cast<const f32x4 *>(s_x + (ty * TW + tx) * CS + 4 * v),
                               *reinterpret_cast<const f32x4 *>(s_g + ((ty * F + ki) * WW + tx * F + kj) * PP + 4 * v), acc);
            *reinterpret_cast<f32x4 *>(dst + (size_t)t * a.C + c) = acc;
        }
    }
}

// grad_w: S = B * tiles workgroup slots of n = k k C floats.  G = ceil(S / 64) chains: chain g adds the slots g, g + G, g + 2G, ... in
// ascending order (at most 64 terms; rows = ceil(S / G); the slots the last row lacks are zeroed), then the chain sums are added in order.
struct UpPlan {
    int TH, TW, CS, tiles_x, tiles_y, S, G, rows;
    size_t n, part, chains, total;
};

static int up_plan(UpPlan &pl, const char *what, int B, int C, int H, int W, int f)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: non-positive dimension (B %d, C %d, H %d, W %d)", what, B, C, H, W);
    if (f != 2 && f != 4 && f != 8) H3D_FAIL(H3D_ERR_SHAPE, "%s: f = %d (2, 4 or 8)", what, f);
    if (C % 4) H3D_FAIL(H3D_ERR_SHAPE, "%s: C = %d is no multiple of 4", what, C);
    if ((long long)B * H * W * f * f > 0x7fffffffLL / 4) H3D_FAIL(H3D_ERR_SHAPE, "%s: %lld output pixels", what, (long long)B * H * W * f * f);
    if (B > 65535) H3D_FAIL(H3D_ERR_SHAPE, "%s: B = %d (at most 65535)", what, B);
    pl.TH = pl.TW = f == 2 ? UpBwd<2>::TH : f == 4 ? UpBwd<4>::TH : UpBwd<8>::TH;
    pl.CS = f == 2 ? UpBwd<2>::CS : f == 4 ? UpBwd<4>::CS : UpBwd<8>::CS;
    pl.tiles_x = cdiv(W, pl.TW);
    pl.tiles_y = cdiv(H, pl.TH);
    if (cdiv(C, pl.CS) > 65535) H3D_FAIL(H3D_ERR_SHAPE, "%s: C = %d", what, C);
    pl.S = B * pl.tiles_x * pl.tiles_y;
    pl.G = cdiv(pl.S, 64);
    pl.rows = cdiv(pl.S, pl.G);
    pl.n = (size_t)4 * f * f * C;
    h3d_ws_layout ws;
    pl.part = ws.take((size_t)pl.rows * pl.G * pl.n * 4);
    pl.chains = ws.take(pl.G > 1 ? (size_t)pl.G * pl.n * 4 : 0);
    pl.total = ws.total;
    return H3D_OK;
}

extern "C" int h3d_upsample_backward_workspace_bytes(int B, int C, int H, int W, int f, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "upsample_backward_workspace_bytes: null pointer");
    *bytes = 0;
    UpPlan pl;
    H3D_TRY(up_plan(pl, "upsample_backward_workspace_bytes", B, C, H, W, f));
    *bytes = pl.total;
    return H3D_OK;
}

extern "C" int h3d_upsample_backward(const float *x, int x_cs, const float *w, const float *grad_y, int gy_cs, float *grad_x, int gx_cs,
                                     float *grad_w, int B, int C, int H, int W, int f, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "upsample_backward";
    UpPlan pl;
    H3D_TRY(up_plan(pl, what, B, C, H, W, f));
    H3D_TRY(check_cs(what, "x", x_cs, C));
    H3D_TRY(check_cs(what, "grad_y", gy_cs, C));
    H3D_TRY(check_cs(what, "grad_x", gx_cs, C));
    if (!x || !w || !grad_y) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", what);
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)grad_y | (uintptr_t)grad_x) & 15)
        H3D_FAIL(H3D_ERR_ARG, "%s: x / w / grad_y / grad_x must be 16-byte aligned", what);
    if ((uintptr_t)grad_w & 3) H3D_FAIL(H3D_ERR_ARG, "%s: grad_w must be 4-byte aligned", what);
    if (!grad_x && !grad_w) return H3D_OK;
    if (grad_w && (!workspace || workspace_bytes < pl.total || ((uintptr_t)workspace & 255)))
        H3D_FAIL(H3D_ERR_ARG, "%s: workspace of %zu bytes, %zu needed (256-byte aligned)", what, workspace ? workspace_bytes : (size_t)0, pl.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    UpBwdArgs a = {};
    a.x = x; a.w = w; a.gy = grad_y; a.gx = grad_x;
    a.pw = grad_w ? (float *)(ws + pl.part) : nullptr;
    a.x_cs = x_cs; a.gy_cs = gy_cs; a.gx_cs = gx_cs;
    a.B = B; a.C = C; a.H = H; a.W = W; a.tiles_x = pl.tiles_x;
    const dim3 grid(pl.tiles_x * pl.tiles_y, cdiv(C, pl.CS), B);
    if (f == 2) H3D_TRY(h3d_launch({"up_bwd_kernel", 2}, up_bwd_kernel<2>, grid, dim3(256), 0, st, a));
    else if (f == 4) H3D_TRY(h3d_launch({"up_bwd_kernel", 4}, up_bwd_kernel<4>, grid, dim3(256), 0, st, a));
    else H3D_TRY(h3d_launch({"up_bwd_kernel", 8}, up_bwd_kernel<8>, grid, dim3(256), 0, st, a));
    if (grad_w) {
        if (pl.G == 1) return h3d_split_sum(a.pw, grad_w, pl.n, pl.S, st);
        const size_t tail = (size_t)pl.rows * pl.G - pl.S;
        if (tail && hipMemsetAsync(a.pw + (size_t)pl.S * pl.n, 0, tail * pl.n * 4, st) != hipSuccess)
            H3D_FAIL(H3D_ERR_LAUNCH, "%s: hipMemsetAsync failed", what);
        float *chains = (float *)(ws + pl.chains);
        H3D_TRY(h3d_split_sum(a.pw, chains, (size_t)pl.G * pl.n, pl.rows, st));
        H3D_TRY(h3d_split_sum(chains, grad_w, pl.n, pl.G, st));
    }
    return H3D_OK;
}
