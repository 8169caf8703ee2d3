// BatchNorm2d with batch statistics (include/h3d.h section 2e): forward (training and evaluation through one entry), the running-statistics
// update, and backward.  fp32 NHWC with a channel stride, 16-byte accesses, no float atomics: every output element is written once, as a
// sum in a fixed order that depends on the shape alone.
//
// Workgroup = 256 threads = V lanes x PPP pixels (V = 1, 2, 4, 8 float4 lanes = 4V channels, the smallest that covers C up to 32;
// PPP = 256 / V).  It owns one chunk of `chunk` consecutive pixels of one group of 4V channels: thread (lane, p) adds the chunk's pixels
// p, p + PPP, ... in order (at most 64 terms), the PPP thread sums meet in a halving tree in LDS.  With S = ceil(N / chunk) > 1 chunks a
// workgroup stores its sums to slot `s` of the workspace and the next launch's workgroups each form the total with h3d_chain_sum4
// (csrc/split_sum.h: chains of at most 64 slots).  S == 1 (N <= 64 PPP: level 5) needs no second stage: one launch does it all.
//   training forward, S > 1:  bn_sum_kernel (sum x) -> bn_sqsum_kernel (mean; sum (x - mean)^2) -> bn_apply_kernel (var, invstd, the
//                             running update and the outputs by chunk 0 of each channel group; y)
//   training forward, S == 1: bn_fused_kernel
//   evaluation forward:       bn_apply_kernel
//   backward:                 bn_bwd_sum_kernel (sum gg, sum gg xhat; grad_res; evaluation's grad_x) -> bn_bwd_apply_kernel (grad_beta,
//                             grad_gamma by chunk 0; training's grad_x)
// The per-channel scalars (mean = sum / N, var, invstd, the running update) are formed in double and rounded once.
#include "common.h"
#include "split_sum.h"

#include <math.h>

struct BnArgs {
    const float *x, *gamma, *beta, *res, *y_in, *gy, *mean_in, *var_in, *invstd_in;
    float *y, *mean_out, *var_out, *invstd_out, *run_mean, *run_var, *gx, *gres, *ggamma, *gbeta;
    float *part_a, *part_b, *stat;                  // workspace: [S][C], [S][C], mean [C] + invstd [C]
    int x_cs, res_cs, y_cs, gy_cs, gx_cs, gres_cs;
    int C, V, logV, chunk, S, training, relu;
    long long N;
    float momentum, eps;
};

struct BnThread {
    int lane, p, PPP, c;
    bool active;
    size_t p0, p1;
};

static __device__ __forceinline__ BnThread bn_thread(const BnArgs &a)
{
    BnThread t;
    t.lane = threadIdx.x & (a.V - 1);
    t.p = threadIdx.x >> a.logV;
    t.PPP = 256 >> a.logV;
    t.c = (blockIdx.y * a.V + t.lane) * 4;
    t.active = t.c < a.C;
    t.p0 = (size_t)blockIdx.x * a.chunk;
    t.p1 = (size_t)min((long long)t.p0 + a.chunk, a.N);
    return t;
}

static __device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
static __device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// the sum over the workgroup's PPP pixel threads, lane by lane: a halving tree (p += p + h for h = PPP / 2 ... 1); every thread gets it
static __device__ __forceinline__ f32x4 bn_block_sum(f32x4 acc, f32x4 *s, int V, int PPP)
{
    const int tid = threadIdx.x;
    s[tid] = acc;
    __syncthreads();
    for (int h = PPP >> 1; h >= 1; h >>= 1) {
        if (tid < h * V) s[tid] += s[tid + h * V];
        __syncthreads();
    }
    const f32x4 r = s[tid & (V - 1)];
    __syncthreads();
    return r;
}

static __device__ __forceinline__ f32x4 bn_chunk_sum(const BnArgs &a, const BnThread &t)
{
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (t.active)
        for (size_t i = t.p0 + t.p; i < t.p1; i += t.PPP) acc += ld4(a.x + i * a.x_cs + t.c);
    return acc;
}

static __device__ __forceinline__ f32x4 bn_chunk_sqsum(const BnArgs &a, const BnThread &t, f32x4 mean)
{
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (t.active)
        for (size_t i = t.p0 + t.p; i < t.p1; i += t.PPP) {
            const f32x4 d = ld4(a.x + i * a.x_cs + t.c) - mean;
            acc += d * d;
        }
    return acc;
}

static __device__ __forceinline__ f32x4 bn_div_n(f32x4 s, long long N)
{
    const double n = (double)N;
    return f32x4{(float)((double)s.x / n), (float)((double)s.y / n), (float)((double)s.z / n), (float)((double)s.w / n)};
}

static __device__ __forceinline__ f32x4 bn_invstd(f32x4 var, float eps)
{
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = (float)(1.0 / sqrt((double)var[j] + (double)eps));
    return r;
}

// the outputs of the statistics and the running update: one thread per lane of chunk 0
static __device__ __forceinline__ void bn_store_stats(const BnArgs &a, const BnThread &t, f32x4 mean, f32x4 var, f32x4 invstd)
{
    if (!(blockIdx.x == 0 && t.p == 0 && t.active)) return;
    if (a.mean_out) st4(a.mean_out + t.c, mean);
    if (a.var_out) st4(a.var_out + t.c, var);
    if (a.invstd_out) st4(a.invstd_out + t.c, invstd);
    const double m = (double)a.momentum, n = (double)a.N;
    if (a.run_mean) {
        const f32x4 r = ld4(a.run_mean + t.c);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (float)((1.0 - m) * (double)r[j] + m * (double)mean[j]);
        st4(a.run_mean + t.c, o);
    }
    if (a.run_var) {
        const f32x4 r = ld4(a.run_var + t.c);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (float)((1.0 - m) * (double)r[j] + m * ((double)var[j] * n / (n - 1.0)));
        st4(a.run_var + t.c, o);
    }
}

// y = act((x - mean) (gamma invstd) + beta + res) over the chunk
static __device__ __forceinline__ void bn_chunk_apply(const BnArgs &a, const BnThread &t, f32x4 mean, f32x4 invstd)
{
    if (!t.active || !a.y) return;
    const f32x4 sc = ld4(a.gamma + t.c) * invstd, be = ld4(a.beta + t.c);
    for (size_t i = t.p0 + t.p; i < t.p1; i += t.PPP) {
        f32x4 v = (ld4(a.x + i * a.x_cs + t.c) - mean) * sc + be;
        if (a.res) v += ld4(a.res + i * a.res_cs + t.c);
        if (a.relu) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.f ? v[j] : (v[j] != v[j] ? v[j] : 0.f);
        }
        st4(a.y + i * a.y_cs + t.c, v);
    }
}

__global__ __launch_bounds__(256) void bn_sum_kernel(BnArgs a)
{
    __shared__ f32x4 s_red[256];
    const BnThread t = bn_thread(a);
    const f32x4 sum = bn_block_sum(bn_chunk_sum(a, t), s_red, a.V, t.PPP);
    if (t.p == 0 && t.active) st4(a.part_a + (size_t)blockIdx.x * a.C + t.c, sum);
}

__global__ __launch_bounds__(256) void bn_sqsum_kernel(BnArgs a)
{
    __shared__ f32x4 s_red[256];
    __shared__ f32x4 s_chain[64 * 8];
    __shared__ f32x4 s_tot[8];
    const BnThread t = bn_thread(a);
    const f32x4 mean = bn_div_n(h3d_chain_sum4(a.part_a, (size_t)a.C, a.S, (size_t)t.c, t.active, t.lane, a.V, t.p, t.PPP, s_chain, s_tot), a.N);
    if (blockIdx.x == 0 && t.p == 0 && t.active) st4(a.stat + t.c, mean);
    const f32x4 sq = bn_block_sum(bn_chunk_sqsum(a, t, mean), s_red, a.V, t.PPP);
    if (t.p == 0 && t.active) st4(a.part_b + (size_t)blockIdx.x * a.C + t.c, sq);
}

__global__ __launch_bounds__(256) void bn_apply_kernel(BnArgs a)
{
    __shared__ f32x4 s_chain[64 * 8];
    __shared__ f32x4 s_tot[8];
    const BnThread t = bn_thread(a);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 mean = zero, var = zero;
    if (a.training) {
        if (t.active) mean = ld4(a.stat + t.c);
        var = bn_div_n(h3d_chain_sum4(a.part_b, (size_t)a.C, a.S, (size_t)t.c, t.active, t.lane, a.V, t.p, t.PPP, s_chain, s_tot), a.N);
    } else if (t.active) {
        mean = ld4(a.mean_in + t.c);
        var = ld4(a.var_in + t.c);
    }
    const f32x4 invstd = bn_invstd(var, a.eps);
    if (a.training) {
        bn_store_stats(a, t, mean, var, invstd);
        if (blockIdx.x == 0 && t.p == 0 && t.active) st4(a.stat + a.C + t.c, invstd);
    } else if (blockIdx.x == 0 && t.p == 0 && t.active && a.invstd_out) {
        st4(a.invstd_out + t.c, invstd);
    }
    bn_chunk_apply(a, t, mean, invstd);
}

// S == 1: the workgroup's chunk is every pixel
__global__ __launch_bounds__(256) void bn_fused_kernel(BnArgs a)
{
    __shared__ f32x4 s_red[256];
    const BnThread t = bn_thread(a);
    const f32x4 mean = bn_div_n(bn_block_sum(bn_chunk_sum(a, t), s_red, a.V, t.PPP), a.N);
    const f32x4 var = bn_div_n(bn_block_sum(bn_chunk_sqsum(a, t, mean), s_red, a.V, t.PPP), a.N);
    const f32x4 invstd = bn_invstd(var, a.eps);
    bn_store_stats(a, t, mean, var, invstd);
    bn_chunk_apply(a, t, mean, invstd);
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------
// gg = grad_y [y > 0] under ReLU (the mask from the saved output, as h3d_conv2d_backward takes it), else grad_y
static __device__ __forceinline__ f32x4 bn_gg(const BnArgs &a, const BnThread &t, size_t i)
{
    f32x4 g = ld4(a.gy + i * a.gy_cs + t.c);
    if (a.relu) {
        const f32x4 y = ld4(a.y_in + i * a.y_cs + t.c);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = y[j] > 0.f ? g[j] : 0.f;
    }
    return g;
}

__global__ __launch_bounds__(256) void bn_bwd_sum_kernel(BnArgs a)
{
    __shared__ f32x4 s_red[256];
    const BnThread t = bn_thread(a);
    f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgx = {0.f, 0.f, 0.f, 0.f};
    if (t.active) {
        const f32x4 mean = ld4(a.mean_in + t.c), invstd = ld4(a.invstd_in + t.c);
        const bool eval_gx = !a.training && a.gx;
        f32x4 sc = invstd;
        if (eval_gx) sc = ld4(a.gamma + t.c) * invstd;
        for (size_t i = t.p0 + t.p; i < t.p1; i += t.PPP) {
            const f32x4 g = bn_gg(a, t, i);
            const f32x4 xh = (ld4(a.x + i * a.x_cs + t.c) - mean) * invstd;
            sg += g;
            sgx += g * xh;
            if (a.gres) st4(a.gres + i * a.gres_cs + t.c, g);
            if (eval_gx) st4(a.gx + i * a.gx_cs + t.c, g * sc);
        }
    }
    sg = bn_block_sum(sg, s_red, a.V, t.PPP);
    sgx = bn_block_sum(sgx, s_red, a.V, t.PPP);
    if (t.p == 0 && t.active) {
        st4(a.part_a + (size_t)blockIdx.x * a.C + t.c, sg);
        st4(a.part_b + (size_t)blockIdx.x * a.C + t.c, sgx);
    }
}

// training: grad_x = gamma invstd (gg - grad_beta / N - xhat grad_gamma / N)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(BnArgs a)
{
    __shared__ f32x4 s_chain[64 * 8];
    __shared__ f32x4 s_tot[8];
    const BnThread t = bn_thread(a);
    const f32x4 gb = h3d_chain_sum4(a.part_a, (size_t)a.C, a.S, (size_t)t.c, t.active, t.lane, a.V, t.p, t.PPP, s_chain, s_tot);
    const f32x4 gg = h3d_chain_sum4(a.part_b, (size_t)a.C, a.S, (size_t)t.c, t.active, t.lane, a.V, t.p, t.PPP, s_chain, s_tot);
    if (!t.active) return;
    if (blockIdx.x == 0 && t.p == 0) {
        if (a.gbeta) st4(a.gbeta + t.c, gb);
        if (a.ggamma) st4(a.ggamma + t.c, gg);
    }
    if (!(a.training && a.gx)) return;
    const f32x4 mean = ld4(a.mean_in + t.c), invstd = ld4(a.invstd_in + t.c), sc = ld4(a.gamma + t.c) * invstd;
    const f32x4 mb = bn_div_n(gb, a.N), mg = bn_div_n(gg, a.N);
    for (size_t i = t.p0 + t.p; i < t.p1; i += t.PPP) {
        const f32x4 g = bn_gg(a, t, i);
        const f32x4 xh = (ld4(a.x + i * a.x_cs + t.c) - mean) * invstd;
        st4(a.gx + i * a.gx_cs + t.c, sc * (g - mb - xh * mg));
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
struct BnPlan {
    int V, logV, PPP, groups, chunk, S;
    long long N;
    size_t part_a, part_b, stat, total;
};

static int bn_plan(BnPlan &pl, const char *what, int B, int C, int H, int W)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: non-positive dimension (B %d, C %d, H %d, W %d)", what, B, C, H, W);
    if (C % 4) H3D_FAIL(H3D_ERR_SHAPE, "%s: C = %d is no multiple of 4", what, C);
    pl.N = (long long)B * H * W;
    if (pl.N > 0x7fffffffLL / 4) H3D_FAIL(H3D_ERR_SHAPE, "%s: %lld pixels", what, pl.N);
    pl.logV = 0;
    while (pl.logV < 3 && (4 << pl.logV) < C) ++pl.logV;
    pl.V = 1 << pl.logV;
    pl.PPP = 256 >> pl.logV;
    pl.groups = cdiv(C, 4 * pl.V);
    if (pl.groups > 65535) H3D_FAIL(H3D_ERR_SHAPE, "%s: C = %d", what, C);
    if (pl.N <= 64LL * pl.PPP) {
        pl.chunk = (int)pl.N;
    } else {
        // chains of 8 .. 64 pixels per thread: as many workgroups as fill the device a few times over, and at most 4096 slots
        long long per = (pl.N * pl.groups + 1024LL * pl.PPP - 1) / (1024LL * pl.PPP);
        per = per < 8 ? 8 : per > 64 ? 64 : per;
        long long chunk = per * pl.PPP;
        if ((pl.N + chunk - 1) / chunk > 4096) chunk = ((pl.N + 4095) / 4096 + pl.PPP - 1) / pl.PPP * pl.PPP;
        pl.chunk = (int)chunk;
    }
    pl.S = (int)((pl.N + pl.chunk - 1) / pl.chunk);
    h3d_ws_layout ws;
    pl.part_a = ws.take((size_t)pl.S * C * 4);
    pl.part_b = ws.take((size_t)pl.S * C * 4);
    pl.stat = ws.take((size_t)2 * C * 4);
    pl.total = ws.total;
    return H3D_OK;
}

static int bn_check_cs(const char *what, const char *name, int cs, int C)
{
    if (cs < C || cs % 4) H3D_FAIL(H3D_ERR_SHAPE, "%s: %s channel stride %d (>= %d channels, a multiple of 4)", what, name, cs, C);
    return H3D_OK;
}

static int bn_check_ws(const char *what, const BnPlan &pl, void *workspace, size_t workspace_bytes)
{
    if (!workspace || workspace_bytes < pl.total || ((uintptr_t)workspace & 255))
        H3D_FAIL(H3D_ERR_ARG, "%s: workspace of %zu bytes, %zu needed (256-byte aligned)", what, workspace ? workspace_bytes : (size_t)0, pl.total);
    return H3D_OK;
}

static void bn_fill(BnArgs &a, const BnPlan &pl, int C, void *workspace)
{
    char *ws = (char *)workspace;
    a.part_a = ws ? (float *)(ws + pl.part_a) : nullptr;
    a.part_b = ws ? (float *)(ws + pl.part_b) : nullptr;
    a.stat = ws ? (float *)(ws + pl.stat) : nullptr;
    a.C = C; a.V = pl.V; a.logV = pl.logV; a.chunk = pl.chunk; a.S = pl.S; a.N = pl.N;
}

extern "C" int h3d_batch_norm_workspace_bytes(int B, int C, int H, int W, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "batch_norm_workspace_bytes: null pointer");
    *bytes = 0;
    BnPlan pl;
    H3D_TRY(bn_plan(pl, "batch_norm_workspace_bytes", B, C, H, W));
    *bytes = pl.total;
    return H3D_OK;
}

extern "C" int h3d_batch_norm_plan(int B, int C, int H, int W, int *chunk, int *slots)
{
    if (!chunk || !slots) H3D_FAIL(H3D_ERR_ARG, "batch_norm_plan: null pointer");
    BnPlan pl;
    H3D_TRY(bn_plan(pl, "batch_norm_plan", B, C, H, W));
    *chunk = pl.chunk;
    *slots = pl.S;
    return H3D_OK;
}

extern "C" int h3d_batch_norm_forward(const float *x, int x_cs, const float *gamma, const float *beta, const float *res, int res_cs, float *y,
                                      int y_cs, float *mean, float *var, float *save_invstd, float *running_mean, float *running_var, int B,
                                      int C, int H, int W, int training, int relu, float momentum, float eps, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    const char *what = "batch_norm_forward";
    BnPlan pl;
    H3D_TRY(bn_plan(pl, what, B, C, H, W));
    H3D_TRY(bn_check_cs(what, "x", x_cs, C));
    if (res) H3D_TRY(bn_check_cs(what, "res", res_cs, C));
    if (y) H3D_TRY(bn_check_cs(what, "y", y_cs, C));
    if (training && pl.N == 1) H3D_FAIL(H3D_ERR_SHAPE, "%s: more than 1 value per channel is needed in training (B %d, H %d, W %d)", what, B, H, W);
    if (!(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f)) H3D_FAIL(H3D_ERR_ARG, "%s: eps %g (>= 0), momentum %g (in [0, 1])", what, eps, momentum);
    if (!x || (y && (!gamma || !beta)) || (!training && (!mean || !var))) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", what);
    if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)res | (uintptr_t)y | (uintptr_t)mean | (uintptr_t)var |
         (uintptr_t)save_invstd | (uintptr_t)running_mean | (uintptr_t)running_var) & 15)
        H3D_FAIL(H3D_ERR_ARG, "%s: every operand must be 16-byte aligned", what);
    if (training && pl.S > 1) H3D_TRY(bn_check_ws(what, pl, workspace, workspace_bytes));
    if (!training && !y && !save_invstd) return H3D_OK;
    if (training && !y && !mean && !var && !save_invstd && !running_mean && !running_var) return H3D_OK;
    hipStream_t st = (hipStream_t)stream;
    BnArgs a = {};
    bn_fill(a, pl, C, training && pl.S > 1 ? workspace : nullptr);
    a.x = x; a.gamma = gamma; a.beta = beta; a.res = res; a.y = y;
    a.x_cs = x_cs; a.res_cs = res_cs; a.y_cs = y_cs;
    a.training = training != 0; a.relu = relu != 0; a.momentum = momentum; a.eps = eps;
    const dim3 grid(pl.S, pl.groups), one(1, pl.groups);
    if (!training) {
        a.mean_in = mean; a.var_in = var; a.invstd_out = save_invstd;
        return h3d_launch({"bn_apply_kernel"}, bn_apply_kernel, y ? grid : one, dim3(256), 0, st, a);
    }
    a.mean_out = mean; a.var_out = var; a.invstd_out = save_invstd; a.run_mean = running_mean; a.run_var = running_var;
    if (pl.S == 1) return h3d_launch({"bn_fused_kernel"}, bn_fused_kernel, grid, dim3(256), 0, st, a);
    H3D_TRY(h3d_launch({"bn_sum_kernel"}, bn_sum_kernel, grid, dim3(256), 0, st, a));
    H3D_TRY(h3d_launch({"bn_sqsum_kernel"}, bn_sqsum_kernel, grid, dim3(256), 0, st, a));
    return h3d_launch({"bn_apply_kernel"}, bn_apply_kernel, y ? grid : one, dim3(256), 0, st, a);
}

extern "C" int h3d_batch_norm_backward(const float *x, int x_cs, const float *y, int y_cs, const float *grad_y, int gy_cs, const float *gamma,
                                       const float *save_mean, const float *save_invstd, float *grad_x, int gx_cs, float *grad_res, int gr_cs,
                                       float *grad_gamma, float *grad_beta, int B, int C, int H, int W, int training, int relu, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    const char *what = "batch_norm_backward";
    BnPlan pl;
    H3D_TRY(bn_plan(pl, what, B, C, H, W));
    H3D_TRY(bn_check_cs(what, "x", x_cs, C));
    H3D_TRY(bn_check_cs(what, "grad_y", gy_cs, C));
    if (relu) H3D_TRY(bn_check_cs(what, "y", y_cs, C));
    if (grad_x) H3D_TRY(bn_check_cs(what, "grad_x", gx_cs, C));
    if (grad_res) H3D_TRY(bn_check_cs(what, "grad_res", gr_cs, C));
    if (!x || !grad_y || !save_mean || !save_invstd || (relu && !y) || (grad_x && !gamma)) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", what);
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)grad_y | (uintptr_t)gamma | (uintptr_t)save_mean | (uintptr_t)save_invstd | (uintptr_t)grad_x |
         (uintptr_t)grad_res | (uintptr_t)grad_gamma | (uintptr_t)grad_beta) & 15)
        H3D_FAIL(H3D_ERR_ARG, "%s: every operand must be 16-byte aligned", what);
    if (!grad_x && !grad_res && !grad_gamma && !grad_beta) return H3D_OK;
    H3D_TRY(bn_check_ws(what, pl, workspace, workspace_bytes));
    hipStream_t st = (hipStream_t)stream;
    BnArgs a = {};
    bn_fill(a, pl, C, workspace);
    a.x = x; a.y_in = relu ? y : nullptr; a.gy = grad_y; a.gamma = gamma; a.mean_in = save_mean; a.invstd_in = save_invstd;
    a.gx = grad_x; a.gres = grad_res; a.ggamma = grad_gamma; a.gbeta = grad_beta;
    a.x_cs = x_cs; a.y_cs = y_cs; a.gy_cs = gy_cs; a.gx_cs = gx_cs; a.gres_cs = gr_cs;
    a.training = training != 0; a.relu = relu != 0;
    const bool train_gx = training && grad_x;
    H3D_TRY(h3d_launch({"bn_bwd_sum_kernel"}, bn_bwd_sum_kernel, dim3(pl.S, pl.groups), dim3(256), 0, st, a));
    if (!train_gx && !grad_gamma && !grad_beta) return H3D_OK;
    return h3d_launch({"bn_bwd_apply_kernel"}, bn_bwd_apply_kernel, dim3(train_gx ? pl.S : 1, pl.groups), dim3(256), 0, st, a);
}
