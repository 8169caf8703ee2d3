// Training input on the GPU: the train branch of the reference's dataset loaders -- COCOHP._get_input (datasets/coco_hp.py:151-212), the
// same block of COCO.__getitem__ (datasets/coco.py:156-198) and color_aug (utils/image.py:200-232) -- for a batch of uint8 frames that may
// differ in size.  The host (h3d_amd/train_input.py) draws c, s, rot, flipped and the colour parameters and hands over one
// h3d_train_image per image: the INVERSE 2x3 map in double (scale and rotation are in it), the mirror flag, where the frame lies, the
// three colour operations in their drawn order and the lighting vector.
//
//   launch 1  train_warp_kernel    the fixed-point bilinear warp of csrc/preprocess.hip (same rounding, constant border 0) with the mirror
//                                  folded into the source read (column w-1-sx: the reference flips the frame and then warps with
//                                  c[0] = w - c[0] - 1; with integer source coordinates the two are the same bytes), the warped pixel
//                                  stored as one dword B | G<<8 | R<<16 in the workspace, and per workgroup the fp64 sum of
//                                  gs = (B*0.114f + G*0.587f) + R*0.299f over its 1024 pixels (x = v / 255.0f per channel: the float32
//                                  restatement of cv2.cvtColor(BGR2GRAY) on float input; parity with cv2 unpinned, like the warp), written
//                                  to the workgroup's own slot.  No atomics.
//   launch 2  train_colour_kernel  sums the image's slots in slot order, gs_mean = (float)(sum / n), and per pixel and channel applies
//                                  brightness x*a | contrast x*a + (float)(gs_mean*(1-a)) | saturation x*a + gs*(1-a) in the drawn order
//                                  (every product and sum one float32 operation), lighting (float)((double)x + light[c]) -- numpy runs
//                                  `float32 image += float64 vector` in the float64 loop and casts once --, then (x - mean[c]) / std[c] to
//                                  CHW fp32: 16-byte stores where the plane size and the output's alignment allow, scalar stores elsewhere.
//   H3D_TRAIN_INPUT_NO_COLOR_AUG   one launch, no workspace: train_plain_kernel = preprocess_kernel + per-image size, offset and mirror.
//
// The fp64 sum is exact up to 2^18 pixels (512 x 512): every non-zero gs is at least 0.114f/255 > 2^-12 and below 2, a float32, hence a
// multiple of 2^-35; every partial sum of up to 2^18 of them is such a multiple below 2^18 + 1 and fits the 53 bits of a double.  The
// order of the additions then cannot matter, and the device's gs_mean is THE correctly rounded mean.  Above 2^18 pixels a sum may round;
// slot order and the order inside a workgroup are fixed, so two runs still give identical bits.
// This file is compiled with -ffp-contract=off: each float step is one IEEE operation.
#include "common.h"

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_PIX = 4;                                  // pixels per thread; in launch 2 consecutive ones: one 16-byte workspace vector
constexpr int AUG_BLOCK_PIX = AUG_THREADS * AUG_PIX;        // pixels per workgroup of launch 1 = pixels per partial-sum slot
constexpr int AUG_COLOUR_ITERS = 4;                         // launch 2: 4096 pixels per workgroup (the slot sum is paid once per workgroup)

// one warped pixel (B, G, R in 0..255): preprocess_kernel's arithmetic, the column mirrored where d.flipped
__device__ __forceinline__ void warp_pixel(const uint8_t *__restrict__ src, const h3d_train_image &d, int x, int y, int (&v)[3])
{
    const double *M = d.minv;
    const int h = d.h, w = d.w, row_bytes = d.row_bytes;
    const int X0 = __double2int_rn((M[1] * y + M[2]) * 1024.0) + 16;
    const int Y0 = __double2int_rn((M[4] * y + M[5]) * 1024.0) + 16;
    const int X = (X0 + __double2int_rn(M[0] * x * 1024.0)) >> 5;
    const int Y = (Y0 + __double2int_rn(M[3] * x * 1024.0)) >> 5;
    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    const bool x0 = sx >= 0 && sx < w, x1 = sx + 1 >= 0 && sx + 1 < w, y0 = sy >= 0 && sy < h, y1 = sy + 1 >= 0 && sy + 1 < h;
    const int c0 = d.flipped ? w - 1 - sx : sx, c1 = d.flipped ? w - 2 - sx : sx + 1;      // in [0, w) wherever x0 / x1 hold
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int p00 = (x0 && y0) ? src[(size_t)sy * row_bytes + c0 * 3 + c] : 0;
        const int p01 = (x1 && y0) ? src[(size_t)sy * row_bytes + c1 * 3 + c] : 0;
        const int p10 = (x0 && y1) ? src[(size_t)(sy + 1) * row_bytes + c0 * 3 + c] : 0;
        const int p11 = (x1 && y1) ? src[(size_t)(sy + 1) * row_bytes + c1 * 3 + c] : 0;
        v[c] = (w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 16384) >> 15;     // 0..255
    }
}

__device__ __forceinline__ float grey(float b, float g, float r) { return (b * 0.114f + g * 0.587f) + r * 0.299f; }

// the sum of one double per thread over the workgroup, in a fixed order: lanes by halving inside a wave, then the waves in index order
__device__ __forceinline__ double block_sum(double v, double *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < AUG_THREADS / 64; ++k) s += lds[k];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(AUG_THREADS) void train_warp_kernel(const uint8_t *__restrict__ images, const h3d_train_image *__restrict__ desc,
                                                                  int res_w, int n, int npad, int nblk, uint32_t *__restrict__ pix,
                                                                  double *__restrict__ partial)
{
    __shared__ double lds[AUG_THREADS / 64];
    const int b = blockIdx.y;
    const h3d_train_image d = desc[b];
    const uint8_t *src = images + d.offset;
    double sum = 0.0;
#pragma unroll
    for (int e = 0; e < AUG_PIX; ++e) {
        // neighbouring lanes take neighbouring pixels (their source taps share cache lines); p < nblk * 1024 <= 2^30 + 2^10
        const int p = blockIdx.x * AUG_BLOCK_PIX + e * AUG_THREADS + threadIdx.x;
        uint32_t packed = 0u;
        if (p < n) {
            int v[3];
            warp_pixel(src, d, p % res_w, p / res_w, v);
            packed = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16;
            sum += (double)grey((float)v[0] / 255.0f, (float)v[1] / 255.0f, (float)v[2] / 255.0f);
        }
        if (p < npad) pix[(size_t)b * npad + p] = packed;                    // the padding of the last vector is written too (zero)
    }
    const double total = block_sum(sum, lds);
    if (threadIdx.x == 0) partial[(size_t)b * nblk + blockIdx.x] = total;
}

__global__ __launch_bounds__(AUG_THREADS) void train_colour_kernel(const uint32_t *__restrict__ pix, const double *__restrict__ partial,
                                                                    const h3d_train_image *__restrict__ desc, const float *__restrict__ mean,
                                                                    const float *__restrict__ stdv, int n, int npad, int nblk, int vec,
                                                                    float *__restrict__ out, float *__restrict__ gs_mean_out)
{
    __shared__ double lds[AUG_THREADS / 64];
    const int b = blockIdx.y;
    double part = 0.0;
    for (int k = threadIdx.x; k < nblk; k += AUG_THREADS) part += partial[(size_t)b * nblk + k];      // slots in slot order per thread
    const float gs_mean = (float)(block_sum(part, lds) / (double)n);
    if (blockIdx.x == 0 && threadIdx.x == 0 && gs_mean_out) gs_mean_out[b] = gs_mean;
    const h3d_train_image &d = desc[b];
    int op[3];
    float a[3], oma[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) op[k] = d.order[k], a[k] = d.alpha[k], oma[k] = d.one_minus_alpha[k];
    const double light[3] = {d.light[0], d.light[1], d.light[2]};
    const float mn[3] = {mean[0], mean[1], mean[2]}, sd[3] = {stdv[0], stdv[1], stdv[2]};
    float *plane = out + (size_t)b * 3 * n;
    for (int it = 0; it < AUG_COLOUR_ITERS; ++it) {
        const int p0 = ((blockIdx.x * AUG_COLOUR_ITERS + it) * AUG_THREADS + threadIdx.x) * AUG_PIX;
        if (p0 >= n) break;
        const u32x4 packed = *reinterpret_cast<const u32x4 *>(pix + (size_t)b * npad + p0);
        float r[3][AUG_PIX];
#pragma unroll
        for (int e = 0; e < AUG_PIX; ++e) {
            float x[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = (float)((packed[e] >> (8 * c)) & 255u) / 255.0f;
            const float gs = grey(x[0], x[1], x[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (op[k] == H3D_TRAIN_BRIGHTNESS) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) x[c] = x[c] * a[k];
                } else if (op[k] == H3D_TRAIN_CONTRAST) {
                    const float m = gs_mean * oma[k];
#pragma unroll
                    for (int c = 0; c < 3; ++c) x[c] = x[c] * a[k] + m;
                } else {
                    const float g = gs * oma[k];
#pragma unroll
                    for (int c = 0; c < 3; ++c) x[c] = x[c] * a[k] + g;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float lit = (float)((double)x[c] + light[c]);
                r[c][e] = (lit - mn[c]) / sd[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float *o = plane + (size_t)c * n + p0;
            if (vec) {                                            // n % 4 == 0 and out 16-byte aligned: p0 + 4 <= n
                *reinterpret_cast<f32x4 *>(o) = f32x4{r[c][0], r[c][1], r[c][2], r[c][3]};
            } else {
#pragma unroll
                for (int e = 0; e < AUG_PIX; ++e)
                    if (p0 + e < n) o[e] = r[c][e];
            }
        }
    }
}

__global__ void train_plain_kernel(const uint8_t *__restrict__ images, const h3d_train_image *__restrict__ desc, const float *__restrict__ mean,
                                   const float *__restrict__ stdv, int res_h, int res_w, float *__restrict__ out)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= res_w) return;
    const h3d_train_image &d = desc[b];
    int v[3];
    warp_pixel(images + d.offset, d, x, y, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float f = (float)v[c] / 255.0f;
        out[(((size_t)b * 3 + c) * res_h + y) * res_w + x] = (f - mean[c]) / stdv[c];
    }
}

bool misaligned(const void *p, size_t a) { return p && ((uintptr_t)p & (a - 1)) != 0; }

// the workspace of one call: the warped pixels (one dword each, every image padded to whole 16-byte vectors), then one fp64 slot per
// workgroup of launch 1.  Nothing with H3D_TRAIN_INPUT_NO_COLOR_AUG.
struct AugLayout : h3d_ws_layout {
    size_t pix = 0, partial = 0;
    int n = 0, npad = 0, nblk = 0;
};
AugLayout aug_layout(int B, int res_h, int res_w, int options)
{
    AugLayout L;
    L.n = res_h * res_w;                                    // <= 32767^2 < 2^30
    L.npad = (L.n + AUG_PIX - 1) / AUG_PIX * AUG_PIX;
    L.nblk = cdiv(L.n, AUG_BLOCK_PIX);
    if (options & H3D_TRAIN_INPUT_NO_COLOR_AUG) return L;
    L.pix = L.take((size_t)B * L.npad * sizeof(uint32_t));
    L.partial = L.take((size_t)B * L.nblk * sizeof(double));
    return L;
}

int aug_check_sizes(const char *who, int B, int res_h, int res_w, int options)
{
    if (options & ~H3D_TRAIN_INPUT_NO_COLOR_AUG) H3D_FAIL(H3D_ERR_ARG, "%s: options 0x%x", who, options);
    if (B <= 0 || B > 32767 || res_h <= 0 || res_h > 32767 || res_w <= 0 || res_w > 32767)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: B = %d, res = %d x %d (each 1..32767)", who, B, res_h, res_w);
    return H3D_OK;
}

}  // namespace

extern "C" int h3d_train_input_workspace_bytes(int B, int res_h, int res_w, int options, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "train_input_workspace_bytes: null pointer");
    H3D_TRY(aug_check_sizes("train_input_workspace_bytes", B, res_h, res_w, options));
    *bytes = aug_layout(B, res_h, res_w, options).total;
    return H3D_OK;
}

extern "C" int h3d_train_input(const uint8_t *images, size_t images_bytes, const struct h3d_train_image *desc,
                               const struct h3d_train_image *desc_dev, int B, const float *mean, const float *stdv, int res_h, int res_w,
                               int options, void *workspace, size_t workspace_bytes, float *out, float *gs_mean_out, void *stream)
{
    const char *who = "train_input";
    H3D_TRY(aug_check_sizes(who, B, res_h, res_w, options));
    if (!images || !desc || !desc_dev || !mean || !stdv || !out) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if (misaligned(desc, 8) || misaligned(desc_dev, 8) || misaligned(mean, 4) || misaligned(stdv, 4) || misaligned(out, 4) || misaligned(gs_mean_out, 4))
        H3D_FAIL(H3D_ERR_ARG, "%s: misaligned pointer", who);
    const bool colour = !(options & H3D_TRAIN_INPUT_NO_COLOR_AUG);
    for (int b = 0; b < B; ++b) {
        const h3d_train_image &d = desc[b];
        if (d.h <= 0 || d.w <= 0 || d.h > 32767 || d.w > 32767 || d.row_bytes < 3 * d.w)
            H3D_FAIL(H3D_ERR_SHAPE, "%s: image %d is %d x %d (row %d bytes); sides 1..32767 (fixed-point warp), rows of at least 3 w bytes", who, b,
                     d.h, d.w, d.row_bytes);
        // the last byte a pixel read may touch: row h-1, column w-1, channel 2 (the padding of the last row need not exist)
        if (d.offset < 0 || (uint64_t)d.offset > images_bytes ||
            (uint64_t)(d.h - 1) * (uint64_t)d.row_bytes + 3u * (uint64_t)d.w > images_bytes - (uint64_t)d.offset)
            H3D_FAIL(H3D_ERR_SHAPE, "%s: image %d (offset %lld, %d rows of %d bytes) leaves the source buffer of %zu bytes", who, b,
                     (long long)d.offset, d.h, d.row_bytes, images_bytes);
        if (d.flipped != 0 && d.flipped != 1) H3D_FAIL(H3D_ERR_ARG, "%s: image %d: flipped = %d", who, b, d.flipped);
        if (colour) {
            int seen = 0;
            for (int k = 0; k < 3; ++k)
                if (d.order[k] >= 0 && d.order[k] < 3) seen |= 1 << d.order[k];
            if (seen != 7)
                H3D_FAIL(H3D_ERR_ARG, "%s: image %d: colour order (%d, %d, %d) is not a permutation of 0, 1, 2", who, b, d.order[0], d.order[1],
                         d.order[2]);
        }
    }
    const AugLayout L = aug_layout(B, res_h, res_w, options);
    hipStream_t st = (hipStream_t)stream;
    if (!colour)
        return h3d_launch({"train_plain_kernel"}, train_plain_kernel, dim3(cdiv(res_w, 128), res_h, B), dim3(128), 0, st, images, desc_dev, mean,
                          stdv, res_h, res_w, out);
    if (!workspace || workspace_bytes < L.total || misaligned(workspace, 256))
        H3D_FAIL(H3D_ERR_ARG, "%s: workspace of %zu bytes (256-byte aligned), %zu needed", who, workspace ? workspace_bytes : (size_t)0, L.total);
    uint32_t *pix = reinterpret_cast<uint32_t *>((char *)workspace + L.pix);
    double *partial = reinterpret_cast<double *>((char *)workspace + L.partial);
    H3D_TRY(h3d_launch({"train_warp_kernel"}, train_warp_kernel, dim3(L.nblk, B), dim3(AUG_THREADS), 0, st, images, desc_dev, res_w, L.n, L.npad,
                       L.nblk, pix, partial));
    const int vec = (L.n % AUG_PIX == 0 && !misaligned(out, 16)) ? 1 : 0;
    return h3d_launch({"train_colour_kernel"}, train_colour_kernel, dim3(cdiv(L.nblk, AUG_COLOUR_ITERS), B), dim3(AUG_THREADS), 0, st,
                      (const uint32_t *)pix, (const double *)partial, desc_dev, mean, stdv, L.n, L.npad, L.nblk, vec, out, gs_mean_out);
}
