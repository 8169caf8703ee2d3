// Multi-tensor Adam (include/h3d.h section 7): one launch steps a whole parameter list.  fp32 storage and arithmetic.
//
// Built with -ffp-contract=off (csrc/Makefile): every step below is ONE IEEE-754 binary32 operation, round to nearest, in this order --
// the project's definition of the step (tests/optim_ref.py is its numpy mirror):
//     g   = grad                      (weight_decay != 0:  g = grad + wd * p)
//     m   = m + (1-b1) * (g - m)
//     v   = v * b2;   v = v + ((1-b2) * g) * g
//     den = sqrt(v) / bc2s + eps
//     p   = p + (-step_size) * (m / den)
// sqrtf and `/` are the correctly rounded forms (hipcc's default for HIP: v_sqrt_f32 / v_rcp_f32 only seed the refinement sequences
// that end in v_div_fixup_f32 and the sqrt fix-up; no -ffast-math, no __fdividef / __frsqrt_rn here), denormals are kept.
//
// The descriptors travel as the kernel argument: H3D_ADAM_CAPACITY of them plus the prefix table of their chunk counts, 3.6 KB of the
// 4 KB a kernel argument may hold -- no table upload, no workspace, nothing to synchronise with between two steps.  A workgroup finds
// its tensor by a binary search of the prefix table (scalar loads out of the argument segment) and steps one chunk of H3D_ADAM_CHUNK
// elements of it: the size-1 biases cost one workgroup each, a 147 456-element filter is spread over 72.
#include "common.h"
#include <math.h>

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_VEC = 4;                                                // floats per 16-byte access
constexpr int ADAM_VPT = H3D_ADAM_CHUNK / (ADAM_THREADS * ADAM_VEC);       // vectors per thread (all loads of a thread are issued before its first store)
static_assert(ADAM_VPT * ADAM_THREADS * ADAM_VEC == H3D_ADAM_CHUNK, "a chunk is a whole number of vectors per thread");

struct AdamBlock {
    h3d_adam_tensor t[H3D_ADAM_CAPACITY];
    int32_t first[H3D_ADAM_CAPACITY + 1];      // first[i] = chunks of the tensors before i; first[count] = the grid
    int32_t count;
};
static_assert(sizeof(AdamBlock) <= 4096, "the descriptor block must fit a kernel argument");

struct AdamScalars {
    float omb1, b2, omb2, bc2s, eps, nss, wd;
};

__device__ __forceinline__ void adam_element(const AdamScalars &s, float &p, float g, float &m, float &v)
{
    if (s.wd != 0.0f) g = g + s.wd * p;
    m = m + s.omb1 * (g - m);
    v = v * s.b2;
    v = v + (s.omb2 * g) * g;
    const float den = sqrtf(v) / s.bc2s + s.eps;
    p = p + s.nss * (m / den);
}

__device__ __forceinline__ void adam_scalar(const AdamScalars &s, float *p, const float *g, float *m, float *v, int64_t e)
{
    float pe = p[e], me = m[e], ve = v[e];
    adam_element(s, pe, g[e], me, ve);
    p[e] = pe;
    m[e] = me;
    v[e] = ve;
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(const AdamBlock blk)
{
    // the tensor of this workgroup: the last i with first[i] <= blockIdx.x (tensors without elements have no chunk and are never found)
    const int wg = blockIdx.x;
    int lo = 0, hi = blk.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk.first[mid] <= wg) lo = mid;
        else hi = mid;
    }
    const h3d_adam_tensor &d = blk.t[lo];
    const AdamScalars s = {d.one_minus_b1, d.b2, d.one_minus_b2, d.bc2_sqrt, d.eps, d.neg_step_size, d.weight_decay};
    float *__restrict__ p = d.param;
    const float *__restrict__ g = d.grad;
    float *__restrict__ m = d.exp_avg;
    float *__restrict__ v = d.exp_avg_sq;
    const int64_t n = d.n;
    const int tid = threadIdx.x;
    // 16-byte accesses where the four bases share their offset inside 16 bytes: `head` elements (0..3) lead up to the first aligned
    // one and belong to chunk 0; chunk c covers [head + c CHUNK, head + (c + 1) CHUNK).  Bases that disagree: 4-byte accesses only.
    const unsigned mis = (unsigned)((uintptr_t)p & 15);
    const bool vec = mis == (unsigned)((uintptr_t)g & 15) && mis == (unsigned)((uintptr_t)m & 15) && mis == (unsigned)((uintptr_t)v & 15);
    const int head = vec ? (int)(((16 - mis) >> 2) & 3) : 0;
    const int64_t c0 = head + (int64_t)(wg - blk.first[lo]) * H3D_ADAM_CHUNK;
    if (!vec) {
#pragma unroll
        for (int k = 0; k < H3D_ADAM_CHUNK / ADAM_THREADS; ++k) {
            const int64_t e = c0 + k * ADAM_THREADS + tid;
            if (e < n) adam_scalar(s, p, g, m, v, e);
        }
        return;
    }
    if (wg == blk.first[lo] && tid < head && tid < n) adam_scalar(s, p, g, m, v, tid);
    f32x4 pv[ADAM_VPT], gv[ADAM_VPT], mv[ADAM_VPT], vv[ADAM_VPT];
#pragma unroll
    for (int j = 0; j < ADAM_VPT; ++j) {
        const int64_t e = c0 + (int64_t)(j * ADAM_THREADS + tid) * ADAM_VEC;
        if (e + ADAM_VEC <= n) {
            pv[j] = *reinterpret_cast<const f32x4 *>(p + e);
            gv[j] = *reinterpret_cast<const f32x4 *>(g + e);
            mv[j] = *reinterpret_cast<const f32x4 *>(m + e);
            vv[j] = *reinterpret_cast<const f32x4 *>(v + e);
        }
    }
#pragma unroll
    for (int j = 0; j < ADAM_VPT; ++j) {
        const int64_t e = c0 + (int64_t)(j * ADAM_THREADS + tid) * ADAM_VEC;
        if (e + ADAM_VEC <= n) {
#pragma unroll
            for (int k = 0; k < ADAM_VEC; ++k) {
                float pe = pv[j][k], me = mv[j][k], ve = vv[j][k];
                adam_element(s, pe, gv[j][k], me, ve);
                pv[j][k] = pe;
                mv[j][k] = me;
                vv[j][k] = ve;
            }
            *reinterpret_cast<f32x4 *>(p + e) = pv[j];
            *reinterpret_cast<f32x4 *>(m + e) = mv[j];
            *reinterpret_cast<f32x4 *>(v + e) = vv[j];
        } else {
            for (int k = 0; k < ADAM_VEC; ++k)           // the tail: fewer than 4 elements, in one thread of the last chunk
                if (e + k < n) adam_scalar(s, p, g, m, v, e + k);
        }
    }
}

// the chunks of one tensor as the kernel cuts them (the same `head` rule)
int64_t adam_chunks(const h3d_adam_tensor &d)
{
    if (d.n <= 0) return 0;
    const unsigned mis = (unsigned)((uintptr_t)d.param & 15);
    const bool vec = mis == (unsigned)((uintptr_t)d.grad & 15) && mis == (unsigned)((uintptr_t)d.exp_avg & 15) &&
                     mis == (unsigned)((uintptr_t)d.exp_avg_sq & 15);
    const int64_t head = vec ? (int64_t)(((16 - mis) >> 2) & 3) : 0;
    const int64_t body = d.n > head ? d.n - head : 0;
    const int64_t c = (body + H3D_ADAM_CHUNK - 1) / H3D_ADAM_CHUNK;
    return c > 0 ? c : 1;                                   // n <= head: chunk 0 steps the head alone
}

bool adam_finite(float x) { return x - x == 0.0f; }

}  // namespace

extern "C" int h3d_adam_step(const h3d_adam_tensor *tensors, int n_tensors, void *stream)
{
    const char *who = "adam_step";
    if (n_tensors < 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: n_tensors = %d", who, n_tensors);
    if (n_tensors == 0) return H3D_OK;
    if (!tensors) H3D_FAIL(H3D_ERR_ARG, "%s: null tensor list", who);
    for (int i = 0; i < n_tensors; ++i) {
        const h3d_adam_tensor &d = tensors[i];
        if (d.n < 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: tensor %d: n = %lld", who, i, (long long)d.n);
        if (d.n > 0 && (!d.param || !d.grad || !d.exp_avg || !d.exp_avg_sq)) H3D_FAIL(H3D_ERR_ARG, "%s: tensor %d: null pointer", who, i);
        if (((uintptr_t)d.param | (uintptr_t)d.grad | (uintptr_t)d.exp_avg | (uintptr_t)d.exp_avg_sq) & 3)
            H3D_FAIL(H3D_ERR_ARG, "%s: tensor %d: misaligned pointer (fp32 needs 4 bytes)", who, i);
        if (!adam_finite(d.one_minus_b1) || !adam_finite(d.b2) || !adam_finite(d.one_minus_b2) || !adam_finite(d.bc2_sqrt) ||
            !adam_finite(d.eps) || !adam_finite(d.neg_step_size) || !adam_finite(d.weight_decay))
            H3D_FAIL(H3D_ERR_ARG, "%s: tensor %d: non-finite scalar", who, i);
        if (d.b2 < 0.0f || d.b2 >= 1.0f || d.eps < 0.0f || d.bc2_sqrt <= 0.0f)
            H3D_FAIL(H3D_ERR_ARG, "%s: tensor %d: scalar out of range (b2 = %g in [0,1), eps = %g >= 0, bc2_sqrt = %g > 0)", who, i, (double)d.b2,
                     (double)d.eps, (double)d.bc2_sqrt);
        if (adam_chunks(d) > 0x7fffffff) H3D_FAIL(H3D_ERR_SHAPE, "%s: tensor %d: n = %lld is more than 2^31 - 1 chunks", who, i, (long long)d.n);
    }
    hipStream_t st = (hipStream_t)stream;
    // one launch per block of descriptors; a block closes when it holds H3D_ADAM_CAPACITY tensors with elements (or a grid's worth of chunks)
    AdamBlock blk = {};
    int64_t chunks = 0;
    auto flush = [&]() -> int {
        if (!blk.count) return H3D_OK;
        blk.first[blk.count] = (int32_t)chunks;
        for (int i = blk.count + 1; i <= H3D_ADAM_CAPACITY; ++i) blk.first[i] = (int32_t)chunks;
        const int rc = h3d_launch({"adam_step_kernel"}, adam_step_kernel, dim3((unsigned)chunks), dim3(ADAM_THREADS), 0, st, blk);
        blk.count = 0;
        chunks = 0;
        return rc;
    };
    for (int i = 0; i < n_tensors; ++i) {
        const int64_t c = adam_chunks(tensors[i]);
        if (!c) continue;
        if (blk.count == H3D_ADAM_CAPACITY || chunks + c > 0x7fffffff) H3D_TRY(flush());
        blk.t[blk.count] = tensors[i];
        blk.first[blk.count] = (int32_t)chunks;
        ++blk.count;
        chunks += c;
    }
    return flush();
}
