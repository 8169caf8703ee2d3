// Deformable PS-ROI pooling backward on gfx950 (reference: DCNv2/src/cuda/dcn_v2_psroi_pooling_cuda.cu:148-269, 343-419), and the
// backward of the DCNPooling second pass (h3d_dcn_pooling_modulated) under a template flag.
//
//   psroi_bwd_kernel   one workgroup iteration = (roi n, class k).  The sample geometry is csrc/psroi_geom.h's, the forward's copy.
//     pass 1           every sample of the class once: the bounding box of the valid samples' corners (near corner .. far corner
//                      where the flags admit one) and, in modulated mode, the count per bin (the modulated forward stores none).
//     table            [P*P bins][spp^2 samples] in LDS as in the forward (chunks of whole sample columns when it is larger than
//                      PSROI_BWD_LDS_SAMPLES); an entry also carries the sample's offset inside the bounding box.
//     items            thread i owns (channel group cg = i / P^2, bin = i % P^2) and walks the channels cg, cg + G, ... of the class
//                      in ascending order: lanes are neighbouring bins of one channel plane, as in the forward.
//     grad_input       a scatter by float atomics.  Most samples of a roi share their destination pixels, so a workgroup first
//                      combines the contributions of a tile of channels in LDS ([channels][box rows][box columns], ds_add_f32) and
//                      then flushes one global atomic per touched pixel, lanes along the box's rows.  When the box does not fit the
//                      LDS tile or is sparsely sampled (psroi_bwd_tile_channels: a function of the geometry alone) the samples are
//                      added directly to global memory, the reference's form.
//     grad_trans       no atomics, a fixed order: a thread sums the samples of its element in table order and its elements in channel
//                      order into its own LDS slot; then the bin's G slots are added in order, then the bins of a part cell in
//                      row-major order.  The order depends on the shapes and the geometry only, so the result is bit-identical
//                      from run to run and between streams.  Modulated mode adds channel 2, s (1 - s) sum_c grad_out * pooled.
//
// Compiled with -ffp-contract=off, like psroi.o and for the same reason: a gate, floor or ceil decision that differed from the
// forward's by one rounding would change a gradient by O(1).  Guards before any address is formed, the forward's contract: a roi whose
// batch index is not finite or truncates outside [0, B) contributes nothing; every corner lies inside its channel plane (csrc/psroi_geom.h),
// and every LDS tile offset inside the box that pass 1 measured from the same samples.
#include <limits.h>

#include "common.h"
#include "psroi_geom.h"

#include "psroi_check.h"

constexpr int PSROI_BWD_THREADS = 256;
constexpr int PSROI_BWD_LDS_SAMPLES = 2048;    // 32 KiB of sample table per workgroup at most
constexpr int PSROI_BWD_LDS_BYTES = 65536;     // everything a workgroup holds
constexpr int PSROI_BWD_TILE_FLOATS = 8192;    // the grad_input tile at most (32 KiB)
constexpr int PSROI_BWD_COUNT_MAX = 1 << 20;   // the valid-sample count saturates here (the tile rule compares it with area <= 8192)

struct PsroiBwdArgs {
    const float *input, *bbox, *trans, *grad_out, *count;   // count == nullptr in modulated mode
    float *grad_input, *grad_trans;                          // either may be nullptr: not wanted
    int B, C, H, W;
    int P, part, spp, S2c;                // S2c = samples per table chunk
    int cpc, ncls, no_trans, force_direct;
    int G, NI, cap;                       // channel groups, items = G * P * P, floats of the grad_input tile
    long long trans_stride;               // floats per roi in `trans` and `grad_trans`
    long long total;                      // R * ncls workgroup iterations
    float scale, trans_std;
};

// LDS plan, from the shapes alone: table | 3 x NI accumulators | P*P counts | box | grad_input tile
struct PsroiBwdPlan {
    int S2c, G, NI, cap;
    size_t lds;
};
static inline PsroiBwdPlan psroi_bwd_plan(int P, int spp)
{
    const int P2 = P * P;
    const long long S2 = (long long)spp * spp;
    PsroiBwdPlan p;
    p.S2c = S2 * P2 <= PSROI_BWD_LDS_SAMPLES ? (int)S2 : PSROI_BWD_LDS_SAMPLES / P2;
    p.G = P2 >= PSROI_BWD_THREADS ? 1 : PSROI_BWD_THREADS / P2;
    p.NI = p.G * P2;
    const int fixed = P2 * p.S2c * 16 + 3 * p.NI * 4 + P2 * 4 + 32;      // <= 64,832 bytes at P = 45
    p.cap = (PSROI_BWD_LDS_BYTES - fixed) / 4;
    p.cap = p.cap > PSROI_BWD_TILE_FLOATS ? PSROI_BWD_TILE_FLOATS : p.cap;
    p.lds = (size_t)fixed + (size_t)p.cap * 4;
    return p;
}

// channels per LDS tile of a (roi, class) whose `nvalid` valid samples span `area` pixels; 0 = the direct path.  Per channel the tile
// costs `area` LDS words and at most `area` global atomics where the direct path issues nvalid .. 4 nvalid: a box that is sparsely
// sampled (a roi over a large part of the map) gains nothing from the tile.  nvalid = min(valid samples, PSROI_BWD_COUNT_MAX).
// The channel loop is tiled by this number whether or not the tile is used (grad_input not wanted, force_direct), so the order in
// which grad_trans is summed is a function of the shapes and the geometry alone.
PSROI_HD int psroi_bwd_tile_channels(int area, int nvalid, int cap, int cpc, int G)
{
    if (area > cap || area > 2 * nvalid) return 0;
    int ct = cap / area;
    ct = ct > cpc ? cpc : ct;
    return ct > G ? ct - ct % G : ct;
}

// the translation of bin (ph, pw), times trans_std (tr = the roi's row of `trans`)
PSROI_HD void psroi_bwd_trans(const float *tr, int no_trans, int k, int ph, int pw, int P, int part, float trans_std, float &tx, float &ty)
{
    tx = 0.f; ty = 0.f;
    if (!no_trans) {
        const float *tk = tr + (long long)(2 * k) * part * part + psroi_part(ph, P, part) * part + psroi_part(pw, P, part);
        tx = tk[0] * trans_std;
        ty = tk[part * part] * trans_std;
    }
}

template <bool MASKED>
__global__ __launch_bounds__(PSROI_BWD_THREADS) void psroi_bwd_kernel(PsroiBwdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, P = a.P, P2 = a.P * a.P, S2 = a.spp * a.spp, HW = a.H * a.W, NI = a.NI, G = a.G, T = PSROI_BWD_THREADS;
    int4 *tab = reinterpret_cast<int4 *>(smem);                         // [P*P][S2c]
    float *s_acc = reinterpret_cast<float *>(tab + P2 * a.S2c);         // [3][NI]: d/dx, d/dy, mask sums; a slot has one owner
    int *s_cnt = reinterpret_cast<int *>(s_acc + 3 * NI);               // [P*P] valid samples per bin
    int *s_box = s_cnt + P2;                                            // xmin, ymin, xmax, ymax, valid samples; 8 words
    float *tile = reinterpret_cast<float *>(s_box + 8);                 // [cap]
    const bool want_in = a.grad_input != nullptr, want_tr = a.grad_trans != nullptr;
    const int nchunks = (S2 + a.S2c - 1) / a.S2c;

    for (long long it = blockIdx.x; it < a.total; it += gridDim.x) {
        const int k = (int)(it % a.ncls);
        const long long n = it / a.ncls;
        const PsroiRoi geo = psroi_roi(a.bbox + n * 5, a.B, a.scale, P, a.spp);
        if (!geo.valid) continue;                                       // (uniform) contributes nothing: the outputs were zeroed
        const float *tr = a.trans + n * a.trans_stride;

        __syncthreads();                                                // the previous iteration is read
        for (int i = tid; i < 3 * NI; i += T) s_acc[i] = 0.f;
        for (int i = tid; i < P2; i += T) s_cnt[i] = 0;
        if (tid < 8) s_box[tid] = tid < 2 ? INT_MAX : tid < 4 ? -1 : 0;
        __syncthreads();

        auto sample_of = [&](int bi, int s) {
            const int ih = s / a.spp, iw = s - ih * a.spp, ph = bi / P, pw = bi - ph * P;
            float tx, ty;
            psroi_bwd_trans(tr, a.no_trans, k, ph, pw, P, a.part, a.trans_std, tx, ty);
            return psroi_sample(geo, ph, pw, ih, iw, tx, ty, a.H, a.W);
        };

        // ---- pass 1: the box of the valid samples' corners, the count per bin
        int nmine = 0;                                                  // this thread's valid samples, saturating
        for (long long i = tid; i < (long long)P2 * S2; i += T) {
            const int bi = (int)(i / S2), s = (int)(i - (long long)bi * S2);
            const PsroiSample sm = sample_of(bi, s);
            if (sm.flags) {
                atomicAdd(&s_cnt[bi], 1);
                nmine = min(nmine + 1, PSROI_BWD_COUNT_MAX);
                atomicMin(&s_box[0], sm.x);
                atomicMin(&s_box[1], sm.y);
                atomicMax(&s_box[2], sm.x + ((sm.flags & PSROI_FAR_X) ? 1 : 0));
                atomicMax(&s_box[3], sm.y + ((sm.flags & PSROI_FAR_Y) ? 1 : 0));
            }
        }
        if (nmine) atomicAdd(&s_box[4], nmine);                         // <= 256 * 2^20: no overflow
        __syncthreads();
        const int xmin = s_box[0], ymin = s_box[1], xmax = s_box[2], ymax = s_box[3];
        if (xmax < 0) continue;                                         // (uniform) no valid sample
        const int bw = xmax - xmin + 1, bh = ymax - ymin + 1, area = bw * bh;      // <= H * W
        const int ctile = psroi_bwd_tile_channels(area, min(s_box[4], PSROI_BWD_COUNT_MAX), a.cap, a.cpc, G);
        const bool lds = ctile > 0 && want_in && !a.force_direct;
        const int CT = ctile > 0 ? ctile : a.cpc;

        auto build = [&](int s0) {
            for (int i = tid; i < P2 * a.S2c; i += T) {
                const int bi = i / a.S2c, s = s0 + (i - bi * a.S2c);
                int4 ent = make_int4(0, 0, 0, 0);                       // flags 0: not a sample (last chunk) or gated out
                if (s < S2) {
                    const PsroiSample sm = sample_of(bi, s);
                    if (sm.flags)                                       // box offset < area <= cap <= 8192: inside the tile
                        ent = make_int4(sm.y * a.W + sm.x, __float_as_int(sm.fx), __float_as_int(sm.fy),
                                        sm.flags | (lds ? ((sm.y - ymin) * bw + (sm.x - xmin)) << 3 : 0));
                }
                tab[i] = ent;
            }
        };
        if (nchunks == 1) build(0);

        const float *in_b = a.input + (long long)geo.b * a.C * HW;      // in bounds: b < B
        float *gin_b = want_in ? a.grad_input + (long long)geo.b * a.C * HW : nullptr;

        for (int c0 = 0; c0 < a.cpc; c0 += CT) {
            const int cend = min(c0 + CT, a.cpc);
            if (lds) {
                __syncthreads();                                        // the previous tile is flushed
                for (int i = tid; i < (cend - c0) * area; i += T) tile[i] = 0.f;
            }
            for (int s0 = 0; s0 < S2; s0 += a.S2c) {
                if (nchunks > 1) {
                    __syncthreads();                                    // the previous chunk is read
                    build(s0);
                }
                __syncthreads();
                const int ns = min(a.S2c, S2 - s0);
                for (int i = tid; i < NI; i += T) {
                    const int cg = i / P2, bin = i - cg * P2;
                    float sig = 0.f;
                    if (MASKED) sig = 1.f / (1.f + expf(-tr[2 * P2 + bin]));                  // the forward's expression
                    for (int c = c0 + cg; c < cend; c += G) {
                        const int ctop = k * a.cpc + c;                 // < C
                        const long long e = (n * a.C + ctop) * P2 + bin;
                        const float cntf = MASKED ? (float)s_cnt[bin] : a.count[e];
                        if (cntf <= 0.f) continue;
                        const float go = a.grad_out[e];
                        const float diff_val = (MASKED ? go * sig : go) / cntf;
                        const float *plane = in_b + (long long)ctop * HW;
                        float *gplane = want_in ? gin_b + (long long)ctop * HW : nullptr;
                        float *tl = tile + (c - c0) * area;
                        float ax = 0.f, ay = 0.f, ap = 0.f;
                        for (int sl = 0; sl < ns; ++sl) {
                            const int4 ent = tab[bin * a.S2c + sl];
                            if (!(ent.w & PSROI_VALID)) continue;
                            const float fx = __int_as_float(ent.y), fy = __int_as_float(ent.z);
                            const bool farx = ent.w & PSROI_FAR_X, fary = ent.w & PSROI_FAR_Y;
                            const float q00 = (1.f - fx) * (1.f - fy), q01 = (1.f - fx) * fy, q10 = fx * (1.f - fy), q11 = fx * fy;
                            if (want_in) {
                                // a far corner that does not exist has weight 0 in the reference (it adds 0 to the near one)
                                if (lds) {
                                    float *t = tl + ((ent.w >> 3) & 0x1fff);
                                    unsafeAtomicAdd(t, q00 * diff_val);
                                    if (fary) unsafeAtomicAdd(t + bw, q01 * diff_val);
                                    if (farx) unsafeAtomicAdd(t + 1, q10 * diff_val);
                                    if (farx && fary) unsafeAtomicAdd(t + bw + 1, q11 * diff_val);
                                } else {
                                    float *g = gplane + ent.x;
                                    unsafeAtomicAdd(g, q00 * diff_val);
                                    if (fary) unsafeAtomicAdd(g + a.W, q01 * diff_val);
                                    if (farx) unsafeAtomicAdd(g + 1, q10 * diff_val);
                                    if (farx && fary) unsafeAtomicAdd(g + a.W + 1, q11 * diff_val);
                                }
                            }
                            if (want_tr) {
                                const float *p = plane + ent.x;
                                const int dx = farx ? 1 : 0, dy = fary ? a.W : 0;
                                const float U00 = p[0], U10 = p[dx], U01 = p[dy], U11 = p[dy + dx];
                                float diff_x = (U11 * fy + U10 * (1.f - fy) - U01 * fy - U00 * (1.f - fy)) * a.trans_std * diff_val;
                                diff_x *= geo.roi_w;
                                float diff_y = (U11 * fx + U01 * (1.f - fx) - U10 * fx - U00 * (1.f - fx)) * a.trans_std * diff_val;
                                diff_y *= geo.roi_h;
                                ax += diff_x;
                                ay += diff_y;
                                if (MASKED) ap += q00 * U00 + q01 * U01 + q10 * U10 + q11 * U11;
                            }
                        }
                        if (want_tr) {
                            s_acc[i] += ax;
                            s_acc[NI + i] += ay;
                            if (MASKED) s_acc[2 * NI + i] += go * (ap / cntf);
                        }
                    }
                }
            }
            if (lds) {
                __syncthreads();
                // one global atomic per touched pixel; lanes along the rows of the box
                for (int i = tid; i < (cend - c0) * area; i += T) {
                    const float v = tile[i];
                    if (v != 0.f) {
                        const int cc = i / area, r = i - cc * area, ty = r / bw, tx = r - ty * bw;
                        unsafeAtomicAdd(gin_b + (long long)(k * a.cpc + c0 + cc) * HW + (long long)(ymin + ty) * a.W + (xmin + tx), v);
                    }
                }
            }
        }

        if (want_tr) {
            // ---- the bin's channel groups in order, then the bins of a part cell in row-major order
            __syncthreads();
            for (int bin = tid; bin < P2; bin += T)
                for (int ch = 0; ch < (MASKED ? 3 : 2); ++ch) {
                    float v = 0.f;
                    for (int cg = 0; cg < G; ++cg) v += s_acc[ch * NI + cg * P2 + bin];
                    s_acc[ch * NI + bin] = v;
                }
            __syncthreads();
            const int PP = a.part * a.part;
            float *gt = a.grad_trans + n * a.trans_stride + (long long)(2 * k) * PP;
            for (int bin = tid; bin < P2; bin += T) {
                const int ph = bin / P, pw = bin - ph * P;
                const int qh = psroi_part(ph, P, a.part), qw = psroi_part(pw, P, a.part);
                if (MASKED) {
                    const float s = 1.f / (1.f + expf(-tr[2 * P2 + bin]));
                    gt[2 * P2 + bin] = s * (1.f - s) * s_acc[2 * NI + bin];
                }
                // psroi_part is monotone: a part cell's bins are a rectangle, and its first bin sums it
                if ((ph > 0 && psroi_part(ph - 1, P, a.part) == qh) || (pw > 0 && psroi_part(pw - 1, P, a.part) == qw)) continue;
                float sx = 0.f, sy = 0.f;
                for (int h = ph; h < P && psroi_part(h, P, a.part) == qh; ++h)
                    for (int w = pw; w < P && psroi_part(w, P, a.part) == qw; ++w) {
                        sx += s_acc[h * P + w];
                        sy += s_acc[NI + h * P + w];
                    }
                gt[qh * a.part + qw] = sx;
                gt[PP + qh * a.part + qw] = sy;
            }
        }
    }
}

static int psroi_bwd_launch(const char *what, bool masked, const float *grad_out, const float *input, const float *bbox, const float *trans,
                            const float *count, float *grad_input, float *grad_trans, size_t grad_trans_floats, int B, int C, int H, int W,
                            int R, long long trans_stride, int ncls, int no_trans, float spatial_scale, int P, int part, int spp,
                            float trans_std, int force_direct, void *stream)
{
    if (R > 0) H3D_TRY(psroi_check_limits(what, P, part, spp));      // (as in the forward: no rois, nothing to refuse)
    hipStream_t st = (hipStream_t)stream;
    if ((grad_input && hipMemsetAsync(grad_input, 0, (size_t)B * C * H * W * 4, st) != hipSuccess) ||
        (grad_trans && grad_trans_floats && hipMemsetAsync(grad_trans, 0, grad_trans_floats * 4, st) != hipSuccess))
        H3D_FAIL(H3D_ERR_LAUNCH, "%s: memset", what);
    if (R == 0 || (!grad_input && !grad_trans)) return H3D_OK;          // zeros; no launch
    const PsroiBwdPlan p = psroi_bwd_plan(P, spp);
    PsroiBwdArgs a;
    a.input = input; a.bbox = bbox; a.trans = trans; a.grad_out = grad_out; a.count = count;
    a.grad_input = grad_input; a.grad_trans = grad_trans;
    a.B = B; a.C = C; a.H = H; a.W = W;
    a.P = P; a.part = part; a.spp = spp; a.S2c = p.S2c;
    a.cpc = C / ncls; a.ncls = ncls; a.no_trans = no_trans; a.force_direct = force_direct ? 1 : 0;
    a.G = p.G; a.NI = p.NI; a.cap = p.cap;
    a.trans_stride = trans_stride;
    a.total = (long long)R * ncls;
    a.scale = spatial_scale; a.trans_std = trans_std;
    const int grid = (int)(a.total < (1 << 20) ? a.total : (1 << 20));
    // the tile is allocated only where a workgroup can use it (a.cap still tiles the channel loop)
    const size_t lds = grad_input && !force_direct ? p.lds : p.lds - (size_t)p.cap * 4;
    if (masked) return h3d_launch({"psroi_bwd_kernel", true}, psroi_bwd_kernel<true>, dim3(grid), dim3(PSROI_BWD_THREADS), lds, st, a);
    return h3d_launch({"psroi_bwd_kernel", false}, psroi_bwd_kernel<false>, dim3(grid), dim3(PSROI_BWD_THREADS), lds, st, a);
}

extern "C" int h3d_dcn_v2_psroi_pooling_backward(const float *grad_output, const float *input, const float *bbox, const float *trans,
                                                 const float *output_count, float *grad_input, float *grad_trans, int B, int C, int H,
                                                 int W, int num_bbox, int num_trans, int channels_trans, int no_trans,
                                                 float spatial_scale, int output_dim, int group_size, int pooled_size, int part_size,
                                                 int sample_per_part, float trans_std, int force_direct, void *stream)
{
    const char *what = "dcn_v2_psroi_pooling_backward";
    // (an empty tensor has no address: with no rois only the tensors the outputs are shaped like are needed)
    if (!input || (!no_trans && !trans) || (num_bbox > 0 && (!grad_output || !bbox || !output_count)))
        H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", what);
    int rc = psroi_check_common(what, B, C, H, W, num_bbox, output_dim, group_size, pooled_size, part_size, sample_per_part);
    if (rc) return rc;
    int ncls = 1;
    if (!no_trans && (rc = psroi_check_trans(what, channels_trans, output_dim, &ncls))) return rc;
    if (!no_trans && num_trans < num_bbox) H3D_FAIL(H3D_ERR_SHAPE, "%s: trans has %d rows for %d rois", what, num_trans, num_bbox);
    const long long stride = no_trans ? 0 : (long long)channels_trans * part_size * part_size;
    return psroi_bwd_launch(what, false, grad_output, input, bbox, no_trans ? nullptr : trans, output_count, grad_input,
                            no_trans ? nullptr : grad_trans, no_trans ? 0 : (size_t)num_trans * (size_t)stride, B, C, H, W, num_bbox, stride,
                            ncls, no_trans ? 1 : 0, spatial_scale, pooled_size, part_size, sample_per_part, trans_std, force_direct, stream);
}

extern "C" int h3d_dcn_pooling_modulated_backward(const float *grad_output, const float *input, const float *bbox, const float *offset_mask,
                                                  float *grad_input, float *grad_offset_mask, int B, int C, int H, int W, int num_bbox,
                                                  float spatial_scale, int output_dim, int group_size, int pooled_size, int part_size,
                                                  int sample_per_part, float trans_std, int force_direct, void *stream)
{
    const char *what = "dcn_pooling_modulated_backward";
    if (!input || (num_bbox > 0 && (!grad_output || !bbox || !offset_mask))) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", what);
    int rc = psroi_check_common(what, B, C, H, W, num_bbox, output_dim, group_size, pooled_size, part_size, sample_per_part);
    if (rc) return rc;
    if (part_size != pooled_size)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: part_size %d != pooled_size %d (the offsets are [R,2,P,P])", what, part_size, pooled_size);
    const long long stride = 3LL * pooled_size * pooled_size;
    return psroi_bwd_launch(what, true, grad_output, input, bbox, offset_mask, nullptr, grad_input, grad_offset_mask,
                            (size_t)num_bbox * (size_t)stride, B, C, H, W, num_bbox, stride, 1, 0, spatial_scale, pooled_size, part_size,
                            sample_per_part, trans_std, force_direct, stream);
}

// Which grad_input path the kernel takes for one (roi, class): the same functions, run on the host.  roi = 5 floats, trans_row = the roi's
// [channels_trans, part, part] translations (HOST pointers; trans_row is not read when no_trans).  *path = 0: nothing to add (invalid batch
// index or no valid sample), 1: combined in LDS, 2: added directly.
extern "C" int h3d_psroi_backward_path(const float *roi, const float *trans_row, int B, int C, int H, int W, int channels_trans, int no_trans,
                                       float spatial_scale, int pooled_size, int part_size, int sample_per_part, float trans_std,
                                       int class_id, int force_direct, int *path)
{
    const char *what = "psroi_backward_path";
    if (!roi || !path || (!no_trans && !trans_row)) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", what);
    int rc = psroi_check_common(what, B, C, H, W, 1, C, 1, pooled_size, part_size, sample_per_part);
    if (rc) return rc;
    int ncls = 1;
    if (!no_trans && (rc = psroi_check_trans(what, channels_trans, C, &ncls))) return rc;
    H3D_TRY(psroi_check_limits(what, pooled_size, part_size, sample_per_part));
    if (class_id < 0 || class_id >= ncls) H3D_FAIL(H3D_ERR_ARG, "%s: class %d of %d", what, class_id, ncls);
    const int P = pooled_size, spp = sample_per_part;
    const PsroiBwdPlan p = psroi_bwd_plan(P, spp);
    const PsroiRoi geo = psroi_roi(roi, B, spatial_scale, P, spp);
    *path = 0;
    if (!geo.valid) return H3D_OK;
    int xmin = INT_MAX, ymin = INT_MAX, xmax = -1, ymax = -1;
    long long nvalid = 0;
    for (int ph = 0; ph < P; ++ph)
        for (int pw = 0; pw < P; ++pw) {
            float tx, ty;
            psroi_bwd_trans(trans_row, no_trans, class_id, ph, pw, P, part_size, trans_std, tx, ty);
            for (int ih = 0; ih < spp; ++ih)
                for (int iw = 0; iw < spp; ++iw) {
                    const PsroiSample sm = psroi_sample(geo, ph, pw, ih, iw, tx, ty, H, W);
                    if (!sm.flags) continue;
                    ++nvalid;
                    xmin = sm.x < xmin ? sm.x : xmin;
                    ymin = sm.y < ymin ? sm.y : ymin;
                    const int fx = sm.x + ((sm.flags & PSROI_FAR_X) ? 1 : 0), fy = sm.y + ((sm.flags & PSROI_FAR_Y) ? 1 : 0);
                    xmax = fx > xmax ? fx : xmax;
                    ymax = fy > ymax ? fy : ymax;
                }
        }
    if (xmax < 0) return H3D_OK;
    const int area = (xmax - xmin + 1) * (ymax - ymin + 1);
    const int counted = (int)(nvalid < PSROI_BWD_COUNT_MAX ? nvalid : PSROI_BWD_COUNT_MAX);
    *path = !force_direct && psroi_bwd_tile_channels(area, counted, p.cap, C / ncls, p.G) > 0 ? 1 : 2;
    return H3D_OK;
}
