// The training / validation losses on gfx950 (reference: /root/reference/src/lib/models/losses.py, trains/trainer.py:29-137).
//
//   loss_partial_kernel   every term of a call in ONE launch: workgroups are dealt to terms by a prefix table (LossArgs::t[].block0).
//                         focal term (_neg_loss, losses.py:42-67): one pass over x and gt with 16-byte loads (scalar head and tail, so any
//                         4-byte aligned pointer and any n work), optional sigmoid + clamp (and store of it) on the way in;
//                         gathered regression terms (RegL1Loss, RegWeightedL1Loss, NormRegL1Loss, RegLoss): one thread per (b, m, c), the
//                         NCHW map read in place.  fp32 per thread -> wave shuffles -> LDS -> one plain 16-byte store per workgroup.
//   loss_finish_kernel    one wave per term sums that term's partials in a fixed order in fp64, selects `num_pos == 0` on the device and
//                         writes {loss, aux0..2}; then the weighted total.  No float atomics anywhere in the forward: bit-reproducible.
//   loss_bwd_dense_kernel focal gradients (elementwise) and the zero fill of the regression gradients, one launch;
//   loss_bwd_scatter_kernel  the regression gradients, atomically added into the zeroed maps -- ordered behind the fill by the launch
//                         boundary.
// Compiled with -ffp-contract=off: the stored `pred` must be the bits of decode.hip's sigmoid_clamp_kernel.
#include "common.h"

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_WAVES = LOSS_THREADS / 64;
constexpr int LOSS_DENSE_MAX_BLOCKS = 2048;   // 8 workgroups of 4 waves per CU: the whole chip resident once
constexpr int LOSS_REG_MAX_BLOCKS = 256;

struct LossTermDev {
    const float *x, *gt;
    float *pred;
    const int64_t *ind;
    const void *mask;
    float *grad;
    long long n;          // elements this launch sweeps for the term
    int B, C, HW, M;
    int kind, flags, mask_type;
    int block0, nblocks;  // the term's workgroups: [block0, block0 + nblocks)
    int index;            // position in the caller's term array (stats / coef slot)
};
struct LossArgs {
    LossTermDev t[H3D_LOSS_MAX_TERMS];
    int n;
};

// ---- 16-byte sweeps over arrays of any 4-byte alignment ---------------------------------------------------------------------------
// The primary array decides the split: `head` scalar elements up to its first 16-byte boundary, nvec vectors, a scalar tail.
struct Sweep {
    long long head, nvec, tail0, n;
};
__device__ __forceinline__ Sweep make_sweep(const void *primary, long long n)
{
    Sweep s;
    s.n = n;
    s.head = (long long)(((16u - (unsigned)((uintptr_t)primary & 15u)) & 15u) >> 2);
    if (s.head > n) s.head = n;
    s.nvec = (n - s.head) >> 2;
    s.tail0 = s.head + 4 * s.nvec;
    return s;
}
__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
__device__ __forceinline__ f32x4 ld4(const float *p, bool al)
{
    if (al) return *reinterpret_cast<const f32x4 *>(p);
    return f32x4{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ void st4(float *p, bool al, f32x4 v)
{
    if (al) {
        *reinterpret_cast<f32x4 *>(p) = v;
    } else {
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
    }
}
// the scalar element (head or tail) thread `tid` of the term's first workgroup owns, or -1
__device__ __forceinline__ long long sweep_scalar(const Sweep &s, int blk, int tid)
{
    if (blk != 0) return -1;
    if (tid < s.head) return tid;
    if (tid >= 32 && s.tail0 + (tid - 32) < s.n) return s.tail0 + (tid - 32);
    return -1;
}

// ---- the terms' arithmetic -----------------------------------------------------------------------------------------------------------
struct Acc3 { float a, b, c; };

__device__ __forceinline__ void focal_fwd(float p, float g, Acc3 &acc)
{
    const bool ispos = g == 1.0f, isneg = g < 1.0f;
    const float q = 1.0f - p;
    const float l = logf(ispos ? p : q);            // one logarithm per element: log(p) at a centre, log(1-p) elsewhere
    float w = 1.0f - g;
    w = w * w;
    w = w * w;
    acc.a += ispos ? l * (q * q) : 0.0f;
    acc.b += isneg ? l * (p * p) * w : 0.0f;
    acc.c += ispos ? 1.0f : 0.0f;
}
// d/dp of the element's term (before the -1/num_pos)
__device__ __forceinline__ float focal_dp(float p, float g)
{
    const bool ispos = g == 1.0f, isneg = g < 1.0f;
    const float q = 1.0f - p;
    const float l = logf(ispos ? p : q);
    float w = 1.0f - g;
    w = w * w;
    w = w * w;
    const float dpos = (q * q) / p - 2.0f * q * l;                   // d/dp log(p) (1-p)^2
    const float dneg = w * (2.0f * p * l - (p * p) / q);             // d/dp log(1-p) p^2 (1-gt)^4
    return ispos ? dpos : isneg ? dneg : 0.0f;
}
// gradient with respect to x of one focal element; s = coef * (-1/num_pos | -1)
__device__ __forceinline__ float focal_bwd(float x, float g, float s, bool from_logits)
{
    if (!from_logits) return s * focal_dp(x, g);
    const float y = sigmoid_plain(x);
    const bool pass = y >= 1e-4f && y <= 1.0f - 1e-4f;              // torch's clamp passes the gradient on the closed interval
    const float p = fminf(fmaxf(y, 1e-4f), 1.0f - 1e-4f);
    return pass ? s * focal_dp(p, g) * (y * (1.0f - y)) : 0.0f;
}

__device__ __forceinline__ float reg_mask(const LossTermDev &t, long long idx, long long bm)
{
    const long long i = t.kind == H3D_LOSS_REG_WEIGHTED_L1 ? idx : bm;
    return t.mask_type == H3D_LOSS_MASK_U8 ? (float)reinterpret_cast<const uint8_t *>(t.mask)[i] : reinterpret_cast<const float *>(t.mask)[i];
}
// element idx = (b M + m) C + c of a regression term: k = its mask, off = its cell in feat (or -1: ind out of range)
__device__ __forceinline__ void reg_locate(const LossTermDev &t, long long idx, int &c, float &k, long long &off)
{
    const long long bm = idx / t.C;
    c = (int)(idx - bm * t.C);
    const long long b = bm / t.M;
    k = reg_mask(t, idx, bm);
    const int64_t ind = t.ind[bm];
    off = (ind >= 0 && ind < t.HW) ? (b * t.C + c) * (long long)t.HW + ind : -1;
}
__device__ __forceinline__ void reg_fwd(const LossTermDev &t, long long idx, Acc3 &acc)
{
    int c;
    float k;
    long long off;
    reg_locate(t, idx, c, k, off);
    if (off < 0) return;
    const float p = t.x[off], tg = t.gt[idx];
    float v;
    if (t.kind == H3D_LOSS_NORM_REG_L1) {
        v = fabsf(p / (tg + 1e-4f) * k - k);
    } else {
        const float d = fabsf(p * k - tg * k);
        v = (t.kind == H3D_LOSS_REG_SL1) ? (d < 1.0f ? 0.5f * d * d : d - 0.5f) : d;
    }
    acc.a += v;
    acc.b += (t.kind != H3D_LOSS_REG_SL1 || c == 0) ? k : 0.0f;
}
__device__ __forceinline__ float sgn(float d) { return d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : 0.0f; }
__device__ __forceinline__ void reg_bwd(const LossTermDev &t, long long idx, float s)
{
    int c;
    float k;
    long long off;
    reg_locate(t, idx, c, k, off);
    if (off < 0 || k == 0.0f) return;
    const float p = t.x[off], tg = t.gt[idx];
    float g;
    if (t.kind == H3D_LOSS_NORM_REG_L1) {
        const float r = tg + 1e-4f;
        g = sgn(p / r * k - k) * (k / r);
    } else {
        const float d = p * k - tg * k;
        g = ((t.kind == H3D_LOSS_REG_SL1 && fabsf(d) < 1.0f) ? d : sgn(d)) * k;
    }
    atomicAdd(t.grad + off, s * g);
}

// the term workgroup `bid` belongs to (wave-uniform scan of the prefix table)
__device__ __forceinline__ int find_term(const LossArgs &a, int bid)
{
    int ti = 0;
    for (int i = 1; i < a.n; ++i)
        if (bid >= a.t[i].block0) ti = i;
    return ti;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOSS_THREADS) void loss_partial_kernel(const LossArgs a, f32x4 *__restrict__ partials)
{
    __shared__ float s_red[LOSS_WAVES][3];
    const int tid = threadIdx.x, bid = blockIdx.x;
    const LossTermDev &t = a.t[find_term(a, bid)];
    const int blk = bid - t.block0;
    Acc3 acc = {0.0f, 0.0f, 0.0f};
    if (t.kind == H3D_LOSS_FOCAL) {
        const bool logits = t.flags & H3D_LOSS_FROM_LOGITS;
        float *pred = logits ? t.pred : nullptr;
        const Sweep s = make_sweep(t.x, t.n);
        const long long i1 = sweep_scalar(s, blk, tid);
        if (i1 >= 0) {
            const float p = logits ? sigmoid_clamp(t.x[i1]) : t.x[i1];
            if (pred) pred[i1] = p;
            focal_fwd(p, t.gt[i1], acc);
        }
        const bool gal = aligned16(t.gt + s.head), pal = pred && aligned16(pred + s.head);
        for (long long v = (long long)blk * LOSS_THREADS + tid; v < s.nvec; v += (long long)t.nblocks * LOSS_THREADS) {
            const long long i = s.head + 4 * v;
            f32x4 p = *reinterpret_cast<const f32x4 *>(t.x + i);
            const f32x4 g = ld4(t.gt + i, gal);
            if (logits) {
#pragma unroll
                for (int j = 0; j < 4; ++j) p[j] = sigmoid_clamp(p[j]);
                if (pred) st4(pred + i, pal, p);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) focal_fwd(p[j], g[j], acc);
        }
    } else {
        for (long long i = (long long)blk * LOSS_THREADS + tid; i < t.n; i += (long long)t.nblocks * LOSS_THREADS) reg_fwd(t, i, acc);
    }
    // workgroup sum in a fixed order: shuffles inside the wave, the four waves through LDS, thread 0 stores
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc.a += __shfl_down(acc.a, off);
        acc.b += __shfl_down(acc.b, off);
        acc.c += __shfl_down(acc.c, off);
    }
    if ((tid & 63) == 0) {
        s_red[tid >> 6][0] = acc.a;
        s_red[tid >> 6][1] = acc.b;
        s_red[tid >> 6][2] = acc.c;
    }
    __syncthreads();
    if (tid == 0) {
        f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int w = 0; w < LOSS_WAVES; ++w) {
            o[0] += s_red[w][0];
            o[1] += s_red[w][1];
            o[2] += s_red[w][2];
        }
        partials[bid] = o;
    }
}

struct LossFinishTerm {
    int kind, block0, nblocks;
    float weight;
};
struct LossFinishArgs {
    LossFinishTerm t[H3D_LOSS_MAX_TERMS];
    int n;
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// one workgroup of H3D_LOSS_MAX_TERMS waves: wave w finishes term w
__global__ __launch_bounds__(64 * H3D_LOSS_MAX_TERMS) void loss_finish_kernel(const LossFinishArgs a, const f32x4 *__restrict__ partials,
                                                                               float *__restrict__ stats)
{
    __shared__ double s_loss[H3D_LOSS_MAX_TERMS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (w < a.n) {
        const LossFinishTerm &t = a.t[w];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = lane; i < t.nblocks; i += 64) {
            const f32x4 p = partials[t.block0 + i];
            s0 += (double)p[0];
            s1 += (double)p[1];
            s2 += (double)p[2];
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        if (lane == 0) {
            double loss;
            if (t.kind == H3D_LOSS_FOCAL)
                loss = s2 == 0.0 ? 0.0 - s1 : -(s0 + s1) / s2;      // the reference's `if num_pos == 0` (losses.py:63-66), on the device
            else
                loss = s0 / (s1 + 1e-4);
            s_loss[w] = loss;
            stats[4 * w + 0] = (float)loss;
            stats[4 * w + 1] = (float)s0;
            stats[4 * w + 2] = (float)s1;
            stats[4 * w + 3] = (float)s2;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int i = 0; i < a.n; ++i) total += (double)a.t[i].weight * s_loss[i];
        stats[4 * a.n] = (float)total;
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOSS_THREADS) void loss_bwd_dense_kernel(const LossArgs a, const float *__restrict__ stats,
                                                                      const float *__restrict__ coef)
{
    const int tid = threadIdx.x, bid = blockIdx.x;
    const LossTermDev &t = a.t[find_term(a, bid)];
    const int blk = bid - t.block0;
    const Sweep s = make_sweep(t.grad, t.n);
    const long long i1 = sweep_scalar(s, blk, tid);
    if (t.kind == H3D_LOSS_FOCAL) {
        const bool logits = t.flags & H3D_LOSS_FROM_LOGITS;
        const float npos = stats[4 * t.index + 3];
        const float sc = npos == 0.0f ? -coef[t.index] : (float)(-(double)coef[t.index] / (double)npos);     // one rounding
        if (i1 >= 0) t.grad[i1] = focal_bwd(t.x[i1], t.gt[i1], sc, logits);
        const bool xal = aligned16(t.x + s.head), gal = aligned16(t.gt + s.head);
        for (long long v = (long long)blk * LOSS_THREADS + tid; v < s.nvec; v += (long long)t.nblocks * LOSS_THREADS) {
            const long long i = s.head + 4 * v;
            const f32x4 x = ld4(t.x + i, xal), g = ld4(t.gt + i, gal);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = focal_bwd(x[j], g[j], sc, logits);
            *reinterpret_cast<f32x4 *>(t.grad + i) = o;
        }
    } else {          // zero fill of a regression term's gradient map
        if (i1 >= 0) t.grad[i1] = 0.0f;
        for (long long v = (long long)blk * LOSS_THREADS + tid; v < s.nvec; v += (long long)t.nblocks * LOSS_THREADS)
            *reinterpret_cast<f32x4 *>(t.grad + s.head + 4 * v) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_bwd_scatter_kernel(const LossArgs a, const float *__restrict__ stats,
                                                                        const float *__restrict__ coef)
{
    const int tid = threadIdx.x, bid = blockIdx.x;
    const LossTermDev &t = a.t[find_term(a, bid)];
    const int blk = bid - t.block0;
    const float sc = (float)((double)coef[t.index] / ((double)stats[4 * t.index + 2] + 1e-4));     // one rounding
    for (long long i = (long long)blk * LOSS_THREADS + tid; i < t.n; i += (long long)t.nblocks * LOSS_THREADS) reg_bwd(t, i, sc);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static bool loss_is_reg(int kind) { return kind >= H3D_LOSS_REG_L1 && kind <= H3D_LOSS_REG_SL1; }

// validates one term; *n = elements of its forward sweep (0: an empty term, whose pointers are not looked at)
static int loss_elems(const h3d_loss_term &t, int i, const char *who, long long *n)
{
    if (t.kind == H3D_LOSS_FOCAL) {
        if (t.n < 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: term %d: n = %lld", who, i, (long long)t.n);
        *n = t.n;
    } else if (loss_is_reg(t.kind)) {
        if (t.B < 0 || t.C < 0 || t.HW < 0 || t.M < 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: term %d: B, C, HW, M = %d, %d, %d, %d", who, i, t.B, t.C, t.HW, t.M);
        if (t.mask_type != H3D_LOSS_MASK_U8 && t.mask_type != H3D_LOSS_MASK_F32) H3D_FAIL(H3D_ERR_ARG, "%s: term %d: mask_type %d", who, i, t.mask_type);
        *n = t.HW == 0 ? 0 : (long long)t.B * t.M * t.C;
    } else {
        H3D_FAIL(H3D_ERR_ARG, "%s: term %d: kind %d", who, i, t.kind);
    }
    if (*n > 0) {
        if (!t.x || !t.gt) H3D_FAIL(H3D_ERR_ARG, "%s: term %d: null pointer", who, i);
        if (loss_is_reg(t.kind) && (!t.ind || !t.mask)) H3D_FAIL(H3D_ERR_ARG, "%s: term %d: null pointer", who, i);
    }
    return H3D_OK;
}
// workgroups of a sweep over n elements: a function of n (and the test flag) only
static int loss_blocks(long long n, bool dense, int flags)
{
    if (n <= 0) return 0;
    const long long per = dense ? 4LL * LOSS_THREADS : LOSS_THREADS;
    long long nb = (n + per - 1) / per;
    const long long cap = (flags & H3D_LOSS_TUNE_GRID8) ? 8 : dense ? LOSS_DENSE_MAX_BLOCKS : LOSS_REG_MAX_BLOCKS;
    return (int)(nb < cap ? nb : cap);
}
static int loss_check_terms(const h3d_loss_term *terms, int n_terms, const char *who)
{
    if (n_terms < 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: n_terms = %d", who, n_terms);
    if (n_terms > 0 && !terms) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if (n_terms > H3D_LOSS_MAX_TERMS) H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: %d terms, at most %d per call", who, n_terms, H3D_LOSS_MAX_TERMS);
    return H3D_OK;
}
static LossTermDev loss_dev_term(const h3d_loss_term &t, int index, long long n, int block0, int nblocks)
{
    LossTermDev d;
    d.x = t.x; d.gt = t.gt; d.pred = t.pred; d.ind = t.ind; d.mask = t.mask; d.grad = t.grad;
    d.n = n;
    d.B = t.B; d.C = t.C; d.HW = t.HW; d.M = t.M;
    d.kind = t.kind; d.flags = t.flags; d.mask_type = t.mask_type;
    d.block0 = block0; d.nblocks = nblocks; d.index = index;
    return d;
}

// the forward's plan: every term keeps its slot (an empty one with nblocks = 0), so that the finish writes all of stats
static int loss_plan(const h3d_loss_term *terms, int n_terms, const char *who, LossArgs *a, int *total)
{
    int rc = loss_check_terms(terms, n_terms, who);
    if (rc != H3D_OK) return rc;
    int nb = 0;
    for (int i = 0; i < n_terms; ++i) {
        long long n;
        rc = loss_elems(terms[i], i, who, &n);
        if (rc != H3D_OK) return rc;
        const int b = loss_blocks(n, terms[i].kind == H3D_LOSS_FOCAL, terms[i].flags);
        if (a) a->t[i] = loss_dev_term(terms[i], i, n, nb, b);
        nb += b;
    }
    if (a) a->n = n_terms;
    *total = nb;
    return H3D_OK;
}

extern "C" int h3d_loss_workspace_bytes(const h3d_loss_term *terms, int n_terms, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "loss_workspace_bytes: null pointer");
    int total;
    const int rc = loss_plan(terms, n_terms, "loss_workspace_bytes", nullptr, &total);
    if (rc != H3D_OK) return rc;
    *bytes = ((size_t)total * sizeof(f32x4) + 255) / 256 * 256;
    return H3D_OK;
}

extern "C" int h3d_loss_forward(const h3d_loss_term *terms, int n_terms, float *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!stats) H3D_FAIL(H3D_ERR_ARG, "loss_forward: null pointer");
    LossArgs a;
    int total;
    const int rc = loss_plan(terms, n_terms, "loss_forward", &a, &total);
    if (rc != H3D_OK) return rc;
    const size_t need = (size_t)total * sizeof(f32x4);
    if (need && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15)))
        H3D_FAIL(H3D_ERR_ARG, "loss_forward: workspace of %zu bytes (16-byte aligned), %zu needed", workspace ? workspace_bytes : (size_t)0, need);
    const hipStream_t st = (hipStream_t)stream;
    if (n_terms == 0) {
        if (hipMemsetAsync(stats, 0, sizeof(float), st) != hipSuccess) H3D_FAIL(H3D_ERR_LAUNCH, "loss_forward: memset failed");
        return H3D_OK;
    }
    // the partial launch sees the non-empty terms only (its prefix table must be strictly increasing)
    LossArgs p;
    p.n = 0;
    LossFinishArgs f;
    f.n = n_terms;
    for (int i = 0; i < n_terms; ++i) {
        if (a.t[i].nblocks) p.t[p.n++] = a.t[i];
        f.t[i] = LossFinishTerm{terms[i].kind, a.t[i].block0, a.t[i].nblocks, terms[i].weight};
    }
    if (total) H3D_TRY(h3d_launch({"loss_partial_kernel"}, loss_partial_kernel, dim3(total), dim3(LOSS_THREADS), 0, st, p, (f32x4 *)workspace));
    return h3d_launch({"loss_finish_kernel"}, loss_finish_kernel, dim3(1), dim3(64 * H3D_LOSS_MAX_TERMS), 0, st, f, (const f32x4 *)workspace, stats);
}

extern "C" int h3d_loss_backward(const h3d_loss_term *terms, int n_terms, const float *stats, const float *coef, void *stream)
{
    int rc = loss_check_terms(terms, n_terms, "loss_backward");
    if (rc != H3D_OK) return rc;
    if (n_terms == 0) return H3D_OK;
    if (!stats || !coef) H3D_FAIL(H3D_ERR_ARG, "loss_backward: null pointer");
    LossArgs dense, scat;
    dense.n = scat.n = 0;
    int nd = 0, ns = 0;
    for (int i = 0; i < n_terms; ++i) {
        long long n;
        rc = loss_elems(terms[i], i, "loss_backward", &n);
        if (rc != H3D_OK) return rc;
        if (!terms[i].grad || n == 0) continue;
        if (terms[i].kind == H3D_LOSS_FOCAL) {
            const int b = loss_blocks(n, true, terms[i].flags);
            dense.t[dense.n++] = loss_dev_term(terms[i], i, n, nd, b);
            nd += b;
        } else {
            const long long cells = (long long)terms[i].B * terms[i].C * terms[i].HW;
            const int bf = loss_blocks(cells, true, terms[i].flags), bs = loss_blocks(n, false, terms[i].flags);
            dense.t[dense.n++] = loss_dev_term(terms[i], i, cells, nd, bf);
            nd += bf;
            scat.t[scat.n++] = loss_dev_term(terms[i], i, n, ns, bs);
            ns += bs;
        }
    }
    const hipStream_t st = (hipStream_t)stream;
    if (nd) H3D_TRY(h3d_launch({"loss_bwd_dense_kernel"}, loss_bwd_dense_kernel, dim3(nd), dim3(LOSS_THREADS), 0, st, dense, stats, coef));
    if (ns) H3D_TRY(h3d_launch({"loss_bwd_scatter_kernel"}, loss_bwd_scatter_kernel, dim3(ns), dim3(LOSS_THREADS), 0, st, scat, stats, coef));
    return H3D_OK;
}
