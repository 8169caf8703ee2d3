// Deformable PS-ROI pooling forward on gfx950 (reference: DCNv2/src/cuda/dcn_v2_psroi_pooling_cuda.cu:58-146, 271-341).
//
// The op is a gather: R * C * P^2 * spp^2 bilinear samples with next to no arithmetic.  Everything about a sample except the
// channel it reads -- position, the in-map gate, the clamped corner offset and the two fractions -- depends on (roi, class, ph, pw)
// only, so it is computed once per workgroup into LDS and reused by every channel of the class (the reference recomputes it for
// every output element).
//
//   psroi_kernel   one workgroup iteration = (roi n, class k, tile t).  Tile t is 256 groups of four consecutive output elements
//                  of the class's contiguous [C/ncls, P, P] slab, one group per thread, group starts aligned to four elements of
//                  the whole output so the results leave as 16-byte stores.  Stage 1 writes the sample table
//                  [P*P bins][spp^2 samples] (16 B per sample: corner offset, fx, fy, flags) to LDS, one thread per sample; stage 2
//                  walks the table for the thread's four elements.  Lanes hold consecutive elements, i.e. neighbouring bins of one
//                  channel plane, so at every gather instruction neighbouring lanes read neighbouring pixels of the same rows.  A
//                  table larger than PSROI_LDS_SAMPLES is walked in chunks of whole sample columns (sample order, and so the
//                  summation order, stays the reference's).
//   masked mode    the DCNPooling second pass: offsets are channels 0/1 of the fully-connected output [R,3,P,P] (roi stride
//                  3*P*P), and the result is multiplied by sigmoid(channel 2) -- chunk + cat + sigmoid + pool + mul in one launch.
//
// The sample geometry is csrc/psroi_geom.h's (shared with the backward, csrc/psroi_bwd.hip).  Compiled with -ffp-contract=off: every
// geometry operation is one IEEE fp32 operation in the reference's order, so sample positions and counts match an fp32 restatement
// exactly.  Guards come before any address is formed: a roi whose batch index is not finite or truncates outside [0, B) yields
// 0 / count 0; non-finite coordinates follow the reference's arithmetic (infinite samples fail the gate, NaN ones are clamped to 0
// by fmaxf / fminf), so every corner address is inside its channel plane.
#include "common.h"
#include "psroi_geom.h"
#include "psroi_check.h"

constexpr int PSROI_THREADS = 256;
constexpr int PSROI_LDS_SAMPLES = 2048;   // 32 KiB of sample table per workgroup at most

struct PsroiArgs {
    const float *input, *bbox, *trans;
    float *out, *count;                   // count == nullptr in masked mode
    int B, C, H, W;
    int P, part, spp, S2c;                // S2c = samples per table chunk (a multiple of 1 .. spp*spp)
    int cpc, ncls, ntiles, no_trans;
    long long trans_stride;               // floats per roi in `trans`
    long long total;                      // R * ncls * ntiles workgroup iterations
    float scale, trans_std;
    int vec;                              // out / count are 16-byte aligned
};

template <bool MASKED>
__global__ __launch_bounds__(PSROI_THREADS) void psroi_kernel(PsroiArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int4 *tab = reinterpret_cast<int4 *>(smem);                         // [P*P][S2c]
    float *s_mul = reinterpret_cast<float *>(smem + (size_t)a.P * a.P * a.S2c * sizeof(int4));  // [P*P], masked mode
    const int tid = threadIdx.x, P = a.P, P2 = a.P * a.P, S2 = a.spp * a.spp, HW = a.H * a.W;
    const long long slab = (long long)a.cpc * P2;

    for (long long it = blockIdx.x; it < a.total; it += gridDim.x) {
        const int t = (int)(it % a.ntiles);
        const long long nk = it / a.ntiles;
        const int k = (int)(nk % a.ncls);
        const long long n = nk / a.ncls;

        // ---- roi geometry (uniform over the workgroup): csrc/psroi_geom.h
        const PsroiRoi geo = psroi_roi(a.bbox + n * 5, a.B, a.scale, P, a.spp);
        const bool bvalid = geo.valid;
        const int b = geo.b;
        const float *tr = a.trans + n * a.trans_stride;

        // ---- this thread's four output elements
        const long long slab_lo = n * a.C * (long long)P2 + (long long)k * slab, slab_hi = slab_lo + slab;
        const long long g = ((slab_lo >> 2) + (long long)t * PSROI_THREADS + tid) << 2;
        const long long roi_base = n * a.C * (long long)P2;
        int bin[4];
        bool in[4];
        const float *plane[4];
        float sum[4];
        int cnt[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long e = g + j;
            in[j] = bvalid && e >= slab_lo && e < slab_hi;
            const long long r = in[j] ? e - roi_base : (long long)k * slab;
            const int ctop = (int)(r / P2);
            bin[j] = (int)(r - (long long)ctop * P2);
            plane[j] = a.input + ((long long)b * a.C + ctop) * HW;       // in bounds: b < B, ctop < C
            sum[j] = 0.f;
            cnt[j] = 0;
        }

        for (int s0 = 0; s0 < S2; s0 += a.S2c) {
            __syncthreads();                                            // the previous chunk / iteration is read
            if (bvalid) {
                for (int i = tid; i < P2 * a.S2c; i += PSROI_THREADS) {
                    const int bi = i / a.S2c, s = s0 + (i - bi * a.S2c);
                    int4 ent = make_int4(0, 0, 0, 0);                   // flags 0: not a sample (last chunk) or gated out
                    if (s < S2) {
                        const int ih = s / a.spp, iw = s - ih * a.spp;
                        const int ph = bi / P, pw = bi - ph * P;
                        const int part_h = psroi_part(ph, P, a.part), part_w = psroi_part(pw, P, a.part);
                        float trans_x = 0.f, trans_y = 0.f;
                        if (!a.no_trans) {
                            const float *tk = tr + (long long)(2 * k) * a.part * a.part + part_h * a.part + part_w;
                            trans_x = tk[0] * a.trans_std;
                            trans_y = tk[a.part * a.part] * a.trans_std;
                        }
                        const PsroiSample sm = psroi_sample(geo, ph, pw, ih, iw, trans_x, trans_y, a.H, a.W);
                        if (sm.flags) ent = make_int4(sm.y * a.W + sm.x, __float_as_int(sm.fx), __float_as_int(sm.fy), sm.flags);
                    }
                    tab[i] = ent;
                    if (MASKED && s0 == 0 && i - bi * a.S2c == 0) {
                        const float m = tr[2 * P2 + bi];
                        s_mul[bi] = 1.f / (1.f + expf(-m));
                    }
                }
            }
            __syncthreads();
            if (!bvalid) continue;
            const int ns = min(a.S2c, S2 - s0);
            for (int sl = 0; sl < ns; ++sl) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int4 ent = tab[bin[j] * a.S2c + sl];
                    const int ok = in[j] ? ent.w : 0;
                    const float *p = plane[j] + (ok ? ent.x : 0);
                    const int dx = (ok >> 1) & 1, dy = (ok & 4) ? a.W : 0;
                    const float v11 = p[0], v21 = p[dx], v12 = p[dy], v22 = p[dy + dx];
                    const float fx = __int_as_float(ent.y), fy = __int_as_float(ent.z);
                    const float val = (1.f - fx) * (1.f - fy) * v11 + (1.f - fx) * fy * v12 + fx * (1.f - fy) * v21 + fx * fy * v22;
                    sum[j] += (ok & 1) ? val : 0.f;
                    cnt[j] += ok & 1;
                }
            }
        }

        // ---- epilogue: mean over the valid samples (x sigmoid(mask) in masked mode), 16-byte stores where the group is whole
        float o[4], c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = cnt[j] == 0 ? 0.f : sum[j] / (float)cnt[j];
            if (MASKED && in[j]) o[j] = o[j] * s_mul[bin[j]];
            c[j] = (float)cnt[j];
        }
        const bool inside = g >= slab_lo && g + 4 <= slab_hi;
        if (inside && a.vec) {
            *reinterpret_cast<f32x4 *>(a.out + g) = f32x4{o[0], o[1], o[2], o[3]};
            if (!MASKED) *reinterpret_cast<f32x4 *>(a.count + g) = f32x4{c[0], c[1], c[2], c[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long e = g + j;
                if (e >= slab_lo && e < slab_hi) {
                    a.out[e] = o[j];
                    if (!MASKED) a.count[e] = c[j];
                }
            }
        }
    }
}

int psroi_check_limits(const char *what, int P, int part, int spp)
{
    if (P > 45) H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: pooled_size %d > 45 (P*P bins must fit the LDS sample table)", what, P);
    if (spp > 4096 || part > 65535) H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: sample_per_part / part_size out of range", what);
    return H3D_OK;
}

static int psroi_launch(const char *what, const float *input, const float *bbox, const float *trans, float *output, float *count,
                        int B, int C, int H, int W, int R, long long trans_stride, int ncls, int no_trans, float spatial_scale,
                        int P, int part, int spp, float trans_std, void *stream)
{
    if (R == 0) return H3D_OK;                                          // empty output, no launch (reference :308-312)
    H3D_TRY(psroi_check_limits(what, P, part, spp));
    const int P2 = P * P, S2 = spp * spp;
    PsroiArgs a;
    a.input = input; a.bbox = bbox; a.trans = trans; a.out = output; a.count = count;
    a.B = B; a.C = C; a.H = H; a.W = W;
    a.P = P; a.part = part; a.spp = spp;
    a.S2c = (long long)S2 * P2 <= PSROI_LDS_SAMPLES ? S2 : PSROI_LDS_SAMPLES / P2;
    a.cpc = C / ncls; a.ncls = ncls; a.no_trans = no_trans;
    const long long slab = (long long)a.cpc * P2;
    a.ntiles = (int)((slab / 4 + 2 + PSROI_THREADS - 1) / PSROI_THREADS);   // groups touching a slab: at most slab/4 + 2
    a.trans_stride = trans_stride;
    a.total = (long long)R * ncls * a.ntiles;
    a.scale = spatial_scale; a.trans_std = trans_std;
    a.vec = ((uintptr_t)output % 16 == 0) && (count == nullptr || (uintptr_t)count % 16 == 0);
    const size_t lds = (size_t)P2 * a.S2c * sizeof(int4) + (size_t)(P2 + 3) / 4 * 16;
    const int grid = (int)(a.total < (1 << 20) ? a.total : (1 << 20));
    if (count) return h3d_launch({"psroi_kernel", false}, psroi_kernel<false>, dim3(grid), dim3(PSROI_THREADS), lds, (hipStream_t)stream, a);
    return h3d_launch({"psroi_kernel", true}, psroi_kernel<true>, dim3(grid), dim3(PSROI_THREADS), lds, (hipStream_t)stream, a);
}

// the argument checks and their texts, shared with the backward's entry points (csrc/psroi_bwd.hip)
int psroi_check_common(const char *what, int B, int C, int H, int W, int R, int output_dim, int group_size, int P, int part, int spp)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || R < 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: bad shape B=%d C=%d H=%d W=%d R=%d", what, B, C, H, W, R);
    if (H > (1 << 23) || W > (1 << 23) || (long long)H * W > 0x7fffffffLL || B >= (1 << 24))
        H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: input too large", what);
    if (output_dim != C) H3D_FAIL(H3D_ERR_SHAPE, "input channels and output channels must equal");
    if (group_size != 1)
        H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: group_size %d: only group_size == 1 is supported (the reference indexes channel "
                 "(ctop*gs+gh)*gs+gw past the input for any other value)", what, group_size);
    if (P <= 0 || part <= 0 || spp <= 0) H3D_FAIL(H3D_ERR_ARG, "%s: pooled_size, part_size and sample_per_part must be positive", what);
    return H3D_OK;
}

int psroi_check_trans(const char *what, int channels_trans, int output_dim, int *ncls)
{
    if (channels_trans < 2 || channels_trans % 2)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: trans has %d channels, expected an even number >= 2 (2 * num_classes)", what, channels_trans);
    *ncls = channels_trans / 2;
    if (output_dim % *ncls)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: output_dim %d is not a multiple of num_classes %d", what, output_dim, *ncls);
    return H3D_OK;
}

extern "C" int h3d_dcn_v2_psroi_pooling_forward(const float *input, const float *bbox, const float *trans, float *output,
                                                float *output_count, int B, int C, int H, int W, int num_bbox, int channels_trans,
                                                int no_trans, float spatial_scale, int output_dim, int group_size, int pooled_size,
                                                int part_size, int sample_per_part, float trans_std, void *stream)
{
    const char *what = "dcn_v2_psroi_pooling_forward";
    if (!input || !bbox || !output || !output_count || (!no_trans && !trans)) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", what);
    int rc = psroi_check_common(what, B, C, H, W, num_bbox, output_dim, group_size, pooled_size, part_size, sample_per_part);
    if (rc) return rc;
    int ncls = 1;
    if (!no_trans && (rc = psroi_check_trans(what, channels_trans, output_dim, &ncls))) return rc;
    return psroi_launch(what, input, bbox, no_trans ? nullptr : trans, output, output_count, B, C, H, W, num_bbox,
                        no_trans ? 0 : (long long)channels_trans * part_size * part_size, ncls, no_trans ? 1 : 0, spatial_scale,
                        pooled_size, part_size, sample_per_part, trans_std, stream);
}

extern "C" int h3d_dcn_pooling_modulated(const float *input, const float *bbox, const float *offset_mask, float *output, int B, int C,
                                         int H, int W, int num_bbox, float spatial_scale, int output_dim, int group_size,
                                         int pooled_size, int part_size, int sample_per_part, float trans_std, void *stream)
{
    const char *what = "dcn_pooling_modulated";
    if (!input || !bbox || !offset_mask || !output) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", what);
    int rc = psroi_check_common(what, B, C, H, W, num_bbox, output_dim, group_size, pooled_size, part_size, sample_per_part);
    if (rc) return rc;
    if (part_size != pooled_size)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: part_size %d != pooled_size %d (the offsets are [R,2,P,P])", what, part_size, pooled_size);
    return psroi_launch(what, input, bbox, offset_mask, output, nullptr, B, C, H, W, num_bbox,
                        3LL * pooled_size * pooled_size, 1, 0, spatial_scale, pooled_size, part_size, sample_per_part, trans_std,
                        stream);
}
