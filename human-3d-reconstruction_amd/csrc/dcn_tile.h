// Device and launch pieces shared by the tiled DeformConv generations (csrc/dcn2.hip, dcn3.hip, dcn4.hip, dcn5.hip): the LDS-DMA of a
// filter stage, the range-checked corner load, the tap broadcast, the bilinear geometry of a sample, the tap-at-a-time form of pass 2
// (samples whose corners left the apron), and the launchers' argument checks, argument fill, epilogue choice and workgroup-width
// ladder.  The SE<> sample traits stay in dcn_traits.h.  Everything here is force-inlined into its call site and keeps that site's
// operations and their order.  (The batched pass 2 of dcn3 / dcn5 and dcn4's pass 2 stay written out in their kernels: DESIGN.md.)
#pragma once
#include "common.h"
#include "epilogue.h"
#include "dcn_traits.h"
#include <type_traits>

// ---- device ------------------------------------------------------------------------------------------------------------------

// PIECES KiB pieces of a stage-major filter image -> LDS at `dst`: linear copy (lane offsets lane16 = l * 16) starting at byte `src`
// of the buffer (`base`, `bytes`); piece p is issued by wave p % 8
template <int PIECES>
__device__ __forceinline__ void dcn_lds_dma(const char *base, int bytes, char *dst, int src, int lane16, int wv)
{
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, bytes, 0x00020000);
#pragma unroll
    for (int j = 0; j < (PIECES + 7) / 8; ++j) {
        const int p = wv + 8 * j;
        if (p < PIECES)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(dst + p * 1024), 16, lane16, src + p * 1024, 0, 0);
    }
}

// 16 bytes at byte offset voff (+ soff, the stage's channel offset) of image `img`; an offset beyond `bytes` (corner outside the
// image, idle thread) reads as zero
__device__ __forceinline__ u32x4 dcn_corner16(const char *img, int bytes, int voff, int soff)
{
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)img, 0, bytes, 0x00020000);
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0));
}

// raw (dh, dw, mask logit) of `tap` for pixel r of the wave: they live in the phase-A accumulators of the lane half that owns the tap
// (h = 0: taps 0..4, h = 1: 5..8) and are broadcast to both halves
struct DcnTapOffset { float d_h, d_w, d_m; };
__device__ __forceinline__ DcnTapOffset dcn_tap_offset(const f32x16 &aoffs, int tap, int r)
{
    const int src = (tap < 5) ? r : r + 32, u = (tap < 5) ? tap : tap - 5;
    DcnTapOffset o;
    o.d_h = __shfl(aoffs[3 * u], src); o.d_w = __shfl(aoffs[3 * u + 1], src); o.d_m = __shfl(aoffs[3 * u + 2], src);
    return o;
}

// the four bilinear weights hh*hw, hh*lw, lh*hw, lh*lw of a sample at (h_im, w_im) whose low corner is (fh, fw) = floor of both
__device__ __forceinline__ void dcn_bilinear_w(float h_im, float w_im, float fh, float fw, float (&w4)[4])
{
    const float lh = h_im - fh, lw = w_im - fw;
    const float hh = 1.f - lh, hw = 1.f - lw;
    w4[0] = hh * hw; w4[1] = hh * lw; w4[2] = lh * hw; w4[3] = lh * lw;
}

// a sample gathered from global memory: its weights and which of its corners (hl + (k >> 1), wl + (k & 1)) lie inside the image (bit k)
struct DcnFar { float w[4]; int ok; };
__device__ __forceinline__ DcnFar dcn_far(float h_im, float w_im, int hl, int wl, int H, int W)
{
    DcnFar s;
    dcn_bilinear_w(h_im, w_im, (float)hl, (float)wl, s.w);
    s.ok = (hl >= 0 && wl >= 0 ? 1 : 0) | (hl >= 0 && wl + 1 <= W - 1 ? 2 : 0) |
           (hl + 1 <= H - 1 && wl >= 0 ? 4 : 0) | (hl + 1 <= H - 1 && wl + 1 <= W - 1 ? 8 : 0);
    return s;
}

// Tap-at-a-time pass 2, one (pixel, tap): when the sample at (h_im, w_im) is inside the image and its corners leave the HH x HH apron,
// fb = its NK 16-channel fragments blended from global memory and true is returned; otherwise fb is left alone.  mask() is the
// sample's modulation, corner(kk, y, x) the fragment of channel group kk at image pixel (y, x) -- both only evaluated for such a sample.
template <typename X, int HH, int NK, typename Mask, typename Corner>
__device__ __forceinline__ bool dcn_far_gather(typename X::frag (&fb)[NK], bool live, float h_im, float w_im, int hy0, int hx0, int H, int W,
                                               Mask mask, Corner corner)
{
    if (!(live && h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W)) return false;
    const int hl = (int)floorf(h_im), wl = (int)floorf(w_im);
    const int ry = hl - hy0, rx = wl - hx0;
    if (ry >= 0 && ry + 1 < HH && rx >= 0 && rx + 1 < HH) return false;      // done from the apron
    const DcnFar s = dcn_far(h_im, w_im, hl, wl, H, W);
    const typename X::geo g = X::make_geo(s.w, mask());
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) {
        typename X::frag v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = ((s.ok >> k) & 1) ? corner(kk, hl + (k >> 1), wl + (k & 1)) : X::zero();
        fb[kk] = X::blend(v, g);
    }
    return true;
}

// the epilogue's view of a DeformConv launch (no residual)
template <typename A>
__device__ __forceinline__ EpiArgs dcn_epi_args(const A &a)
{
    EpiArgs e;
    e.bias = a.bias; e.res = nullptr; e.out = a.out; e.Ho = a.H; e.Wo = a.W; e.Cout = a.Cout;
    e.out_cs = a.out_cs; e.res_cs = 0; e.relu = a.relu; e.out_mode = a.out_mode;
    return e;
}

// ---- host --------------------------------------------------------------------------------------------------------------------

// the fields every generation's argument struct takes straight from the op (filters, offsets and switches stay with their launcher)
template <typename A>
static inline void dcn_fill_args(const h3d_op &op, A &a)
{
    a.in = (const char *)op.in; a.bias = op.bias; a.out = (char *)op.out;
    a.B = op.B; a.H = op.H; a.W = op.W; a.in_cs = op.in_cs;
    a.Cout = op.Cout; a.out_cs = op.out_cs; a.relu = op.relu; a.out_mode = op.out_mode;
    a.tiles_x = a.tiles_y = 0;
}

// Argument checks of the 3x3 DeformConv ops with `es`-byte elements (0: the op's dtype has no kernel).  om_rows: op.in2 holds the
// [B,H,W,in2_cs] offset / mask rows of H3D_OP_DCN (what = "dcn"); otherwise it holds the offset filters of a fused op.
static inline int dcn_check_op(const h3d_op &op, const char *what, int es, bool om_rows)
{
    if (!op.in || !op.w || !op.bias || !op.out || !op.in2) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", what);
    if (!es) H3D_FAIL(H3D_ERR_DTYPE, "%s: dtype %d", what, op.dtype);
    if (op.ksize != 3 || op.stride != 1 || op.Ho != op.H || op.Wo != op.W)
        H3D_FAIL(H3D_ERR_UNSUPPORTED, om_rows ? "%s op: network path covers 3x3 s1 p1 d1 dg1 only (k=%d s=%d)" : "%s: covers 3x3 s1 p1 d1 dg1 only (k=%d s=%d)",
                 what, op.ksize, op.stride);
    if (om_rows) {
        if (op.Cin % 16 || op.in_cs % (16 / es) || op.Cin > op.in_cs || op.in2_cs < 28 || op.in2_cs % 4)
            H3D_FAIL(H3D_ERR_SHAPE, "%s: Cin=%d (stride %d) must be a multiple of 16; offset stride %d must be a multiple of 4, >= 28",
                     what, op.Cin, op.in_cs, op.in2_cs);
    } else if (op.Cin % 16 || op.in_cs % (16 / es) || op.Cin > op.in_cs) {
        H3D_FAIL(H3D_ERR_SHAPE, "%s: Cin=%d (stride %d) must be a multiple of 16", what, op.Cin, op.in_cs);
    }
    if (op.H > 32767 || op.W > 32767) H3D_FAIL(H3D_ERR_SHAPE, "%s: image larger than 32767", what);
    if (op.wrows < ((op.Cout + 127) / 128) * 128)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: packed weight rows %d < Cout %d padded to 128", what, op.wrows, op.Cout);
    if (op.out_mode != H3D_OUT_NCHW_F32 && (op.out_cs % 4 || op.Cout > op.out_cs))
        H3D_FAIL(H3D_ERR_SHAPE, "%s: out channel stride %d", what, op.out_cs);
    return H3D_OK;
}

// the kernels' EPI parameter for a launch: 2 LDS-transposed (where the variant has it: `lds_ok`), 1 lean NHWC, 0 general
template <typename A>
static inline int dcn_epi_mode(const A &a, bool lds_ok)
{
    const bool lean = a.out_mode == H3D_OUT_NHWC && a.Cout % 4 == 0 && ((uintptr_t)a.bias & 15) == 0;
    return (lds_ok && lean && a.Cout % 8 == 0 && a.out_cs % 8 == 0 && ((uintptr_t)a.out & 15) == 0) ? 2 : lean ? 1 : 0;
}
// ... as a constant: f(std::integral_constant<int, EPI>); only the modes the variant has are instantiated
template <bool LDS_OK, typename A, typename F>
static inline int dcn_by_epi(const A &a, F f)
{
    return h3d_by_values(f, h3d_epi_vals<LDS_OK>{}, dcn_epi_mode(a, LDS_OK));
}

// the workgroup-width ladder: f(std::integral_constant<int, MT>) for MT = 1 (Cout <= 32), 2 (`mt2`) or 4 32-channel tiles per
// workgroup; MAXMT = 2 where a launcher has no 128-channel variant (only the rungs up to MAXMT are instantiated)
template <int MAXMT = 4, typename F>
static inline int dcn_by_mt(int Cout, bool mt2, F f)
{
    if (Cout <= 32) return f(std::integral_constant<int, 1>{});
    if constexpr (MAXMT >= 4) {
        if (!mt2) return f(std::integral_constant<int, 4>{});
    }
    return f(std::integral_constant<int, 2>{});
}
