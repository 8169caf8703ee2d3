// Network-path modulated deformable convolution, second generation (replaces dcn.hip's
// dcn_kernel in the plan; that one stays as the simple reference implementation for tests).
//
// Reference semantics: DCNv2/src/cuda/dcn_v2_im2col_cuda.cu:25-54 (bilinear, zero corners),
// :125-195 (positions, (>-1,<H) gate, val*mask), dcn_v2_cuda.cu:124-164 (bias + W.columns).
//
// What changed against generation one (profiles/r01_v1: 97 TFLOP/s, VALU- and L1-gather-bound):
//  * the input tile + a MARGIN-pixel apron is staged ONCE per channel chunk in LDS, zero outside
//    the image, so the 36 corner reads per output pixel hit LDS (256 B/clk/CU) instead of the
//    vector L1 (64 B/clk/CU); samples whose corners leave the apron take a per-lane global path;
//  * in bf16 mode the tile is converted to fp16 while staging and the 4-corner blend runs as
//    v_pk_fma_f16 (2 channels per instruction, no bf16 unpack/pack): fp16 carries 11 significant
//    bits, so the sampled operand is MORE precise than a bf16-rounded sample, and the f16 MFMA
//    runs at the bf16 rate.  Weights of DCN layers are packed as fp16 by the host;
//  * each lane blends exactly the 8 channels its MFMA B-fragment needs, for its own pixel, so the
//    sampled tile never goes back to LDS and a tap costs no barrier: 2 barriers per chunk.
//  * f32 (parity) mode keeps the reference's float operation order (sum of 4 products, then *mask).
#include "common.h"
#include "epilogue.h"
#include "dcn_tile.h"

struct Dcn2Args {
    const char *in;
    const char *w;     // [rows][9][Cin] of S (fp16 in bf16 mode, fp32 in f32 mode)
    const float *bias;
    const float *om;   // [B,H,W,om_cs] fp32: 0..17 offsets (2t = dh, 2t+1 = dw), 18..26 mask logits
    char *out;
    int B, H, W, Cin, in_cs, om_cs;
    int Cout, out_cs, relu, out_mode;
    int tiles_x, tiles_y;
    int dbg;   // ablation switches for profiling (h3d_op.reserved & H3D_TUNE_DCN_ABLATE_MASK): 1 = stage only chunk 0, 2 = no gather/blend, 4 = no MFMA
    int mask_final;   // om[18..26] is the mask itself, not its logit (operator boundary h3d_dcn_v2_forward_ws; H3D_OPF_DCN_MASK_FINAL)
    const unsigned *wmax;   // H3D_F16X3 (the operator's fp32 fast path): bit pattern of max |filter|, written by the pack kernels (csrc/dcn.hip)
    const unsigned *amax;   // H3D_F16X3 behind H3D_OPF_DCN_ACT_MAXIMA: [0] max |x|, [1] max |mask| over finite elements (csrc/dcn.hip), the activation scale's source
};

template <typename T, int MT, int CK, int MARGIN, int NT_>
struct Dcn2Cfg {
    static constexpr int ES = sizeof(T);
    static constexpr int SS = SE<T>::SS;
    static constexpr int HH = 16 + 2 + 2 * MARGIN;      // halo height = width
    static constexpr int SBH = CK * SS + 16;            // halo pixel stride (bytes)
    static constexpr int RBH = ((HH * SBH + 255) / 256) * 256;   // 256 B-aligned rows: the 2-row x 16-px gather of a
                                                                 // 16-lane ds_read_b128 group then covers 16 distinct 16-B slots
    static constexpr int WB = 9 * CK * SS + 16;
    static constexpr int BN = 32 * MT;
    static constexpr int NT = NT_;                      // N-tiles (2 rows x 16 px) per wave
    static constexpr int WAVES = 8 / NT_;               // 16 tile rows = WAVES * NT * 2
    static constexpr int THREADS = 64 * WAVES;
    static constexpr int VPP = CK * SS / 16;            // 16-byte vectors of S per pixel
    static constexpr int LDS_H = HH * RBH;
    static constexpr int LDS = LDS_H + BN * WB;
};


template <typename T, int MT, int CK, int MARGIN, int NT_>
__global__ __launch_bounds__(512 / NT_) void dcn2_kernel(Dcn2Args a)
{
    using C = Dcn2Cfg<T, MT, CK, MARGIN, NT_>;
    using X = SE<T>;
    constexpr int ES = C::ES, SS = C::SS, NT = C::NT;
    __shared__ __attribute__((aligned(16))) char smem[C::LDS];
    char *s_h = smem;
    char *s_w = smem + C::LDS_H;

    const int tid = threadIdx.x;
    const int wv = tid >> 6, l = tid & 63, r = l & 31, h = l >> 5;
    const int tiles = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / tiles;
    const int t = blockIdx.x - b * tiles;
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int oy0 = ty * 16, ox0 = tx * 16;
    const int hy0 = oy0 - 1 - MARGIN, hx0 = ox0 - 1 - MARGIN;   // image coords of halo pixel (0,0)
    const int cout0 = blockIdx.y * C::BN;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.f;

    const char *img = a.in + (size_t)b * a.H * a.W * a.in_cs * ES;
    const int aoff = r * C::WB + 8 * h * SS;
    // f16x3 (round 5): `w` is the operator's plain fp32 pack; the filters are scaled by a power of two and split into (hi | lo) fp16 terms by
    // the thread that stages them (as the activations of every f16x3 kernel are).  The scale puts max |w| into [2^13, 2^14) -- the rule of
    // engine.x3_exp, evaluated here from the maximum the pack kernel left behind the bias -- so that lo terms are normal fp16 numbers
    // whatever the magnitude of the caller's filters; the accumulators are multiplied by its inverse (exact).
    [[maybe_unused]] float wsc = 1.f, wun = 1.f;
    if constexpr (std::is_same_v<T, x3_t>) {
        const float m = __uint_as_float(*a.wmax);
        int k = 14;
        if (m > 0.f && m < __builtin_inff()) (void)frexpf(m, &k);
        const int e = min(60, max(-60, 14 - k));
        wsc = ldexpf(1.f, e);
        wun = ldexpf(1.f, -e);
    }
    // ... and the activations by a second power of two (dcn_act_exp), folded into the mask of every sample: the blend runs in fp32 on the
    // unconverted apron, so the blended sample comes out scaled and is split without a clamp (a NaN or an infinity stays non-finite);
    // the accumulators are multiplied by the inverse after wun (two exact steps)
    [[maybe_unused]] float xsc = 1.f, xun = 1.f;
    if constexpr (std::is_same_v<T, x3_t>) {
        if (a.amax) {
            const int e = dcn_act_exp(a.amax[0], a.amax[1]);
            xsc = ldexpf(1.f, e);
            xun = ldexpf(1.f, -e);
        }
    }
    [[maybe_unused]] auto store_w = [&](char *dst_row_tap, int v, u32x4 raw) {      // one 16-byte vector of a staged filter row -> LDS
        if constexpr (std::is_same_v<T, x3_t>) {
#pragma unroll
            for (int i = 0; i < 4; ++i) raw[i] = __float_as_uint(__uint_as_float(raw[i]) * wsc);
            x3_store4(dst_row_tap + (v >> 1) * 32, v & 1, raw);
        } else {
            *reinterpret_cast<u32x4 *>(dst_row_tap + v * 16) = raw;
        }
    };

    // ---- sampling geometry of every (pixel, tap) of this lane, ONCE per workgroup: the reference's
    //      float arithmetic (im2col.cu:163-185).  Kept in registers: boff = LDS byte offset of corner
    //      (h_low, w_low) inside the staged apron, geo = the four blend coefficients (x mask).
    //      A sample failing the (>-1, <H) gate gets zero coefficients.  A sample whose corners leave
    //      the apron ALSO gets zero coefficients here and raises `slow`: pass 2 adds it back.
    int boff[NT][9];
    typename X::geo geo[NT][9];
    int oyx[NT];
    bool slow = false;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int oy = oy0 + wv * (2 * NT) + n * 2 + (r >> 4), ox = ox0 + (r & 15);
        const bool live = (oy < a.H && ox < a.W);
        oyx[n] = live ? ((oy << 16) | ox) : -1;
        const float *omp = a.om + ((size_t)(b * a.H + (live ? oy : 0)) * a.W + (live ? ox : 0)) * a.om_cs;
        float omv[28];
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const f32x4 v = (H3D_DBG(a) & 16) ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4 *>(omp + 4 * q);   // om_cs >= 28, 16-byte aligned rows
            omv[4 * q] = v[0]; omv[4 * q + 1] = v[1]; omv[4 * q + 2] = v[2]; omv[4 * q + 3] = v[3];
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ti = tap / 3, tj = tap - ti * 3;
            const float h_im = (float)(oy - 1 + ti) + omv[2 * tap];
            const float w_im = (float)(ox - 1 + tj) + omv[2 * tap + 1];
            const bool inside = live && (h_im > -1.f && w_im > -1.f && h_im < (float)a.H && w_im < (float)a.W);
            typename X::geo g = X::zero_geo();
            // a sample with zero coefficients still reads its four corners: point it at the undeformed tap, inside the apron and inside
            // this pixel's own 4x4 neighbourhood, so that a non-finite pixel elsewhere in the tile cannot reach this output through 0 * v
            int off = 8 * h * SS + (oy - 1 + ti - hy0) * C::RBH + (ox - 1 + tj - hx0) * C::SBH;
            if (!inside && live && a.mask_final) {
                const float w0[4] = {0.f, 0.f, 0.f, 0.f};
                g = X::make_geo(w0, omv[18 + tap]);        // the reference's `val * mask` with val = 0 (im2col.cu:178): NaN for a NaN / inf mask
            }
            if (inside) {
                const int hl = (int)floorf(h_im), wl = (int)floorf(w_im);
                const int ry = hl - hy0, rx = wl - hx0;
                if (ry >= 0 && ry + 1 < C::HH && rx >= 0 && rx + 1 < C::HH) {
                    float w4[4];
                    dcn_bilinear_w(h_im, w_im, (float)hl, (float)wl, w4);
                    g = X::make_geo(w4, (a.mask_final ? omv[18 + tap] : dcn2_sigmoid(omv[18 + tap])) * xsc);
                    off = 8 * h * SS + ry * C::RBH + rx * C::SBH;
                } else {
                    slow = true;
                }
            }
            boff[n][tap] = off;
            geo[n][tap] = g;
        }
    }

    // ================= pass 1: every sample whose 2x2 corners lie in the apron (branch-free) ==========
    // Software pipeline over channel chunks: chunk c+1's global loads (apron tile + weight slab) are in
    // flight in registers while chunk c is gathered/contracted; converted to S when written to LDS.
    constexpr int WV = 9 * C::VPP;
    constexpr int NH = C::HH * C::HH * C::VPP, NW = C::BN * WV;
    constexpr int NV = (NH + NW + C::THREADS - 1) / C::THREADS;
    u32x4 stg[NV];
    auto load_stage = [&](int c0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = tid + j * C::THREADS;
            u32x4 val = {0u, 0u, 0u, 0u};
            if (i < NH) {
                const int v = i % C::VPP, pix = i / C::VPP;
                const int iy = pix / C::HH, ix = pix - iy * C::HH;
                const int gy = hy0 + iy, gx = hx0 + ix;
                if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
                    val = *reinterpret_cast<const u32x4 *>(img + ((size_t)(gy * a.W + gx) * a.in_cs + c0) * ES + v * 16);
            } else if (i < NH + NW) {
                const int q0 = i - NH;
                const int row = q0 / WV, q = q0 - row * WV;
                const int tap = q / C::VPP, v = q - tap * C::VPP;
                val = *reinterpret_cast<const u32x4 *>(a.w + (((size_t)(cout0 + row) * 9 + tap) * a.Cin + c0) * SS + v * 16);
            }
            stg[j] = val;
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = tid + j * C::THREADS;
            if (i < NH) {
                const int v = i % C::VPP, pix = i / C::VPP;
                const int iy = pix / C::HH, ix = pix - iy * C::HH;
                // (f16x3 with an activation scale: the apron stays unconverted fp32 -- the scale is applied in the blend -- and unclamped)
                *reinterpret_cast<u32x4 *>(s_h + iy * C::RBH + ix * C::SBH + v * 16) =
                    (std::is_same_v<T, x3_t> && a.amax) ? stg[j] : X::convert16(stg[j]);
            } else if (i < NH + NW) {
                const int q0 = i - NH;
                const int row = q0 / WV, q = q0 - row * WV;
                const int tap = q / C::VPP, v = q - tap * C::VPP;
                store_w(s_w + row * C::WB + tap * CK * SS, v, stg[j]);
            }
        }
    };
    load_stage(0);
    for (int c0 = 0; c0 < a.Cin; c0 += CK) {
        if (c0) __syncthreads();
        store_stage();
        __syncthreads();
        if (c0 + CK < a.Cin) load_stage(c0 + CK);

#ifndef DCN2_X3_PIPE
#define DCN2_X3_PIPE 1
#endif
        if constexpr (DCN2_X3_PIPE && std::is_same_v<T, x3_t> && CK == 16 && NT == 1) {
            // f16x3: tap t+1 is blended and split BETWEEN the MFMAs of tap t (a wave issues in order; second operand register set), tap
            // t+2's corners requested as soon as t+1 is blended -- csrc/dcn3.hip's phase B schedule, see there
            typename X::frag v[4];
            typename X::bfrag pb[2];
            auto gather = [&](int tap) {
                const char *p00 = s_h + boff[0][tap];
                v[0] = X::lds(p00);
                v[1] = X::lds(p00 + C::SBH);
                v[2] = X::lds(p00 + C::RBH);
                v[3] = X::lds(p00 + C::RBH + C::SBH);
            };
            gather(0);
            {
                const typename X::frag fb0 = X::blend(v, geo[0][0]);
                __builtin_amdgcn_sched_barrier(0);
                gather(1);
                pb[0] = X::prep(fb0);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                typename X::wfrag fa[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) fa[m] = X::lds_w(s_w + aoff + m * 32 * C::WB + tap * CK * SS);
                if (tap + 1 < 9) {
                    const typename X::frag fbn = X::blend(v, geo[0][tap + 1]);
                    if (tap + 2 < 9) gather(tap + 2);
                    pb[(tap + 1) & 1] = X::prep(fbn);
                }
#pragma unroll
                for (int m = 0; m < MT; ++m) X::mma(acc[m][0], fa[m], pb[tap & 1]);
                __builtin_amdgcn_sched_group_barrier(0x100, 2 * MT, 0);
                if (tap + 1 < 9) {
#pragma unroll
                    for (int i = 0; i < 3 * MT; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        if (i == 3 * MT - 1) __builtin_amdgcn_sched_group_barrier(0x002, 24, 0);
                        else __builtin_amdgcn_sched_group_barrier(0x002, 36 / (3 * MT - 1) + 1, 0);
                        if (i == (MT > 1 ? 2 : 1) && tap + 2 < 9) __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
                    }
                } else {
                    __builtin_amdgcn_sched_group_barrier(0x008, 3 * MT, 0);
                }
            }
        } else
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            typename X::frag fb[NT][CK / 16];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const char *p00 = s_h + boff[n][tap];
#pragma unroll
                for (int kk = 0; kk < CK / 16; ++kk) {
                    if (H3D_DBG(a) & 2) { fb[n][kk] = X::lds(p00 + kk * 16 * SS); continue; }
                    typename X::frag v[4];
                    v[0] = X::lds(p00 + kk * 16 * SS);
                    v[1] = X::lds(p00 + C::SBH + kk * 16 * SS);
                    v[2] = X::lds(p00 + C::RBH + kk * 16 * SS);
                    v[3] = X::lds(p00 + C::RBH + C::SBH + kk * 16 * SS);
                    fb[n][kk] = X::blend(v, geo[n][tap]);
                }
            }
#pragma unroll
            for (int kk = 0; kk < CK / 16; ++kk) {
                typename X::wfrag fa[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) fa[m] = X::lds_w(s_w + aoff + m * 32 * C::WB + (tap * CK + kk * 16) * SS);
                if constexpr (!std::is_same_v<T, x3_t>) {
                    if (H3D_DBG(a) & 4) {
#pragma unroll
                        for (int m = 0; m < MT; ++m)
#pragma unroll
                            for (int n = 0; n < NT; ++n) { X::keep(fa[m]); X::keep(fb[n][kk]); }
                        continue;
                    }
                }
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const typename X::bfrag pb = X::prep(fb[n][kk]);      // (f16x3: the blended fp32 sample split into fp16 terms, once for all M-tiles)
#pragma unroll
                    for (int m = 0; m < MT; ++m) X::mma(acc[m][n], fa[m], pb);
                }
            }
        }
    }

    // ================= pass 2 (rare): samples whose corners left the apron, gathered from global ======
    // Compact rolled loops; geometry is recomputed from the offsets so pass 1 carries no slow-path code.
    if (!(H3D_DBG(a) & 8) && __syncthreads_or(slow ? 1 : 0)) {
        for (int c0 = 0; c0 < a.Cin; c0 += CK) {
            __syncthreads();
            constexpr int WV = 9 * C::VPP;
            for (int i = tid; i < C::BN * WV; i += C::THREADS) {
                const int row = i / WV, q = i - row * WV;
                const int tap = q / C::VPP, v = q - tap * C::VPP;
                store_w(s_w + row * C::WB + tap * CK * SS, v, *reinterpret_cast<const u32x4 *>(
                    a.w + (((size_t)(cout0 + row) * 9 + tap) * a.Cin + c0) * SS + v * 16));
            }
            __syncthreads();
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
                const int ti = tap / 3, tj = tap - ti * 3;
                typename X::frag fb[NT][CK / 16];
                bool any = false;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
#pragma unroll
                    for (int kk = 0; kk < CK / 16; ++kk) fb[n][kk] = X::zero();
                    if (oyx[n] < 0) continue;
                    const int oy = oyx[n] >> 16, ox = oyx[n] & 0xffff;
                    const float *omp = a.om + ((size_t)(b * a.H + oy) * a.W + ox) * a.om_cs;
                    const float h_im = (float)(oy - 1 + ti) + omp[2 * tap];
                    const float w_im = (float)(ox - 1 + tj) + omp[2 * tap + 1];
                    any |= dcn_far_gather<X, C::HH>(fb[n], true, h_im, w_im, hy0, hx0, a.H, a.W,
                        [&] { return (a.mask_final ? omp[18 + tap] : dcn2_sigmoid(omp[18 + tap])) * xsc; },
                        [&](int kk, int y, int x) { return X::global8(img + ((size_t)(y * a.W + x) * a.in_cs + c0 + kk * 16 + 8 * h) * ES); });
                }
                if (!__any(any)) continue;          // wave-uniform: no lane of this wave has a slow sample at this tap
#pragma unroll
                for (int kk = 0; kk < CK / 16; ++kk) {
                    typename X::wfrag fa[MT];
#pragma unroll
                    for (int m = 0; m < MT; ++m) fa[m] = X::lds_w(s_w + aoff + m * 32 * C::WB + (tap * CK + kk * 16) * SS);
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        // (corners straight from memory: the split clamps -- unless the activations are scaled, which bounds the sample)
                        const typename X::bfrag pb = (std::is_same_v<T, x3_t> && a.amax) ? X::prep(fb[n][kk]) : X::prep_raw(fb[n][kk]);
#pragma unroll
                        for (int m = 0; m < MT; ++m) X::mma(acc[m][n], fa[m], pb);
                    }
                }
            }
        }
    }
    if constexpr (std::is_same_v<T, x3_t>) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[m][n][i] = acc[m][n][i] * wun * xun;
    }
    const EpiArgs e = dcn_epi_args(a);
    tile_epilogue<typename StoreT<T>::type, MT, NT>(acc, e, b, oy0, ox0, cout0, wv, r, h);
}

template <typename T, int MT, int CK, int MARGIN, int NT_>
static int launch_dcn2_cfg(const Dcn2Args &a0, hipStream_t st)
{
    using C = Dcn2Cfg<T, MT, CK, MARGIN, NT_>;
    static_assert(C::LDS <= 160 * 1024, "LDS budget");
    Dcn2Args a = a0;
    a.tiles_x = cdiv(a.W, 16);
    a.tiles_y = cdiv(a.H, 16);
    dim3 grid(a.B * a.tiles_x * a.tiles_y, cdiv(a.Cout, C::BN));
    return h3d_launch({"dcn2_kernel", h3d_tag<T>{}, MT, CK, MARGIN, NT_},
                      dcn2_kernel<T, MT, CK, MARGIN, NT_>, grid, dim3(C::THREADS), 0, st, a);
}

int h3d_launch_dcn2(const h3d_op &op, hipStream_t st)
{
    if (const int rc = dcn_check_op(op, "dcn", op.dtype == H3D_BF16 ? 2 : 4, true)) return rc;
    if ((long)op.H * op.W > (1L << 30)) H3D_FAIL(H3D_ERR_SHAPE, "dcn: image too large");
    Dcn2Args a;
    dcn_fill_args(op, a);
    a.w = (const char *)op.w; a.om = (const float *)op.in2; a.Cin = op.Cin; a.om_cs = op.in2_cs;
    a.dbg = op.reserved & H3D_TUNE_DCN_ABLATE_MASK;
    a.mask_final = (op.reserved & H3D_OPF_DCN_MASK_FINAL) ? 1 : 0;
    a.wmax = nullptr;
    a.amax = nullptr;
    if (op.dtype == H3D_BF16) {
        if (op.Cin % 32 == 0 && op.Cout <= 64) {
            if (op.Cout <= 32) return launch_dcn2_cfg<bf16_t, 1, 32, 2, 2>(a, st);
            return launch_dcn2_cfg<bf16_t, 2, 32, 2, 1>(a, st);      // 8 waves x (32 px x 64 ch)
        }
        if (op.Cout <= 32) return launch_dcn2_cfg<bf16_t, 1, 16, 2, 2>(a, st);
        if (op.Cout <= 64) return launch_dcn2_cfg<bf16_t, 2, 16, 2, 2>(a, st);
        return launch_dcn2_cfg<bf16_t, 4, 16, 2, 1>(a, st);      // 8 waves x (32 px x 128 ch)
    }
    if (op.dtype == H3D_F32) {
        if (op.Cout <= 32) return launch_dcn2_cfg<float, 1, 16, 2, 1>(a, st);
        return launch_dcn2_cfg<float, 2, 16, 2, 1>(a, st);
    }
    if (op.dtype == H3D_F16X3 && (op.reserved & H3D_OPF_DCN_RAW_PACK)) {
        // (H3D_OPF_DCN_RAW_PACK: set by the operator entry points of csrc/dcn.hip -- a network plan's f16x3 DeformConvs are H3D_OP_DCN_FUSED[_STREAM]
        //  with pre-split filters and h3d_op.wexp; an H3D_OP_DCN of that kind has no kernel and fails below as before)
        // the operator's fp32 fast path on the fp16 matrix cores: fp32 tensors and the plain fp32 filter pack of H3D_F32, every product as
        // three fp16 MFMAs on split operands (csrc/common.h ET<x3_t>).  bias[wrows] holds the bit pattern of max |filter| (see Dcn2Args)
        a.wmax = (const unsigned *)(op.bias + op.wrows);
        // H3D_OPF_DCN_ACT_MAXIMA: the two activation maxima follow the [B,H,W,in2_cs] offset / mask rows (csrc/dcn.hip)
        if (op.reserved & H3D_OPF_DCN_ACT_MAXIMA) a.amax = (const unsigned *)((const float *)op.in2 + (size_t)op.B * op.H * op.W * op.in2_cs);
        if (op.Cout <= 32) return launch_dcn2_cfg<x3_t, 1, 16, 2, 1>(a, st);
        return launch_dcn2_cfg<x3_t, 2, 16, 2, 1>(a, st);
    }
    H3D_FAIL(H3D_ERR_DTYPE, "dcn: dtype %d", op.dtype);
}
