// The weak-perspective keypoint reprojection loss on the SMPL output (include/h3d.h section 4c; no reference code: the project's own
// definition).
//
//   kp_partial_kernel   one wave per person slot p = b n + m, four per workgroup.  Lane e = 3 k + c (a second round for K > 21) sums
//                       kp3d[p,k,c] = sum_j JW[k,j] joints[p,j,c] + sum_i VW[k,i] verts[p,VI[k,i],c] in that order (the joints from LDS,
//                       the NV vertices gathered in place), forms pred = s kp3d + t_c from the three camera values read in place at
//                       cam_map[b, 0..2, ind[b,m]], and adds m |pred - hps| and m.  fp32 per lane -> wave shuffles -> LDS -> ONE plain
//                       8-byte store per workgroup.
//   kp_finish_kernel    one wave sums the partials in a fixed order in fp64 and writes {loss, l, num}.  No float atomics in the forward.
//   kp_bwd_fill_kernel  zero fill of grad_cam_map and grad_verts (16-byte stores, scalar head and tail);
//   kp_bwd_scatter_kernel  one wave per person slot: lane 2 k + c holds g = coef sign(pred - hps) m; g_s and g_t by wave shuffles and three
//                       atomic adds per slot into the zeroed camera map (two slots may share a pixel) -- ordered behind the fill by the
//                       launch boundary; grad_joints (all of it) and the touched rows of grad_verts (through the inverted table: every row
//                       once per person) by plain stores, each a sum in a fixed order.
// Compiled with -ffp-contract=off: the definition is a sequence of separately rounded products and sums in a stated order.
#include "common.h"

constexpr int KP_THREADS = 256;
constexpr int KP_WAVES = KP_THREADS / 64;
constexpr int KP_FILL_MAX_BLOCKS = 2048;

struct KpFwdArgs {
    const float *joints, *verts, *cam, *hps;
    const int64_t *ind;
    const void *mask;
    const float *jw, *vw;
    const int32_t *vi;
    float *kp3d, *pred;
    int P, max_objs, n, HW, K, NV, V, mask_type;
};

__device__ __forceinline__ float kp_mask(const void *mask, int mask_type, long long i)
{
    return mask_type == H3D_LOSS_MASK_U8 ? (float)reinterpret_cast<const uint8_t *>(mask)[i] : reinterpret_cast<const float *>(mask)[i];
}
__device__ __forceinline__ float kp_wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}
__device__ __forceinline__ float kp_sgn(float d) { return d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : 0.0f; }

__global__ __launch_bounds__(KP_THREADS) void kp_partial_kernel(const KpFwdArgs a, f32x2 *__restrict__ partials)
{
    __shared__ float s_j[KP_WAVES][72];
    __shared__ float s_red[KP_WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int p = blockIdx.x * KP_WAVES + w;          // wave-uniform
    float l = 0.0f, num = 0.0f;
    const bool active = p < a.P;
    if (active) {
        const float *jp = a.joints + (long long)p * 72;
        s_j[w][lane] = jp[lane];
        if (lane < 8) s_j[w][64 + lane] = jp[64 + lane];
    }
    __syncthreads();
    if (active) {
        const int b = p / a.n, m = p - b * a.n;
        const long long slot = (long long)b * a.max_objs + m;
        const int64_t ind = a.ind[slot];
        const bool ok = ind >= 0 && ind < a.HW;
        float s = 0.0f, tx = 0.0f, ty = 0.0f;
        if (ok) {
            const float *cam = a.cam + (long long)b * 3 * a.HW + ind;
            s = cam[0];
            tx = cam[a.HW];
            ty = cam[2 * (long long)a.HW];
        }
        for (int e = lane; e < 3 * a.K; e += 64) {
            const int k = e / 3, c = e - 3 * k;
            float acc = 0.0f;
            const float *jw = a.jw + k * 24;
#pragma unroll 8
            for (int j = 0; j < 24; ++j) acc = acc + jw[j] * s_j[w][3 * j + c];
            for (int i = 0; i < a.NV; ++i) {
                const int v = a.vi[k * a.NV + i];
                if ((unsigned)v < (unsigned)a.V) acc = acc + a.vw[k * a.NV + i] * a.verts[((long long)p * a.V + v) * 3 + c];
            }
            a.kp3d[(long long)p * 3 * a.K + e] = acc;
            if (c < 2) {
                const long long o = slot * 2 * a.K + 2 * k + c;
                float pr = 0.0f;
                if (ok) {
                    pr = s * acc + (c == 0 ? tx : ty);
                    const float mk = kp_mask(a.mask, a.mask_type, o);
                    l += mk * fabsf(pr - a.hps[o]);
                    num += mk;
                }
                a.pred[((long long)p * a.K + k) * 2 + c] = pr;
            }
        }
    }
    l = kp_wave_sum(l);
    num = kp_wave_sum(num);
    if (lane == 0) {
        s_red[w][0] = l;
        s_red[w][1] = num;
    }
    __syncthreads();
    if (tid == 0) {
        f32x2 o = {0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < KP_WAVES; ++i) {
            o[0] += s_red[i][0];
            o[1] += s_red[i][1];
        }
        partials[blockIdx.x] = o;
    }
}

__global__ __launch_bounds__(64) void kp_finish_kernel(const f32x2 *__restrict__ partials, int nparts, float *__restrict__ stats)
{
    const int lane = threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int i = lane; i < nparts; i += 64) {
        const f32x2 v = partials[i];
        s0 += (double)v[0];
        s1 += (double)v[1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off);
        s1 += __shfl_down(s1, off);
    }
    if (lane == 0) {
        stats[0] = (float)(s0 / (s1 + 1e-4));
        stats[1] = (float)s0;
        stats[2] = (float)s1;
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------
// zero fill of n floats at any 4-byte aligned pointer by `nthreads` threads, of which this is thread `t`
__device__ __forceinline__ void kp_fill_zero(float *p, long long n, long long t, long long nthreads)
{
    if (!p || n <= 0) return;
    long long head = (long long)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const long long nvec = (n - head) >> 2, tail0 = head + 4 * nvec;
    if (t < head) p[t] = 0.0f;
    if (t >= 32 && tail0 + (t - 32) < n) p[tail0 + (t - 32)] = 0.0f;      // at most 3 tail elements, owned by threads 32..34
    for (long long v = t; v < nvec; v += nthreads) *reinterpret_cast<f32x4 *>(p + head + 4 * v) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}
__global__ __launch_bounds__(KP_THREADS) void kp_bwd_fill_kernel(float *__restrict__ grad_cam, long long n_cam, float *__restrict__ grad_verts,
                                                                 long long n_verts)
{
    const long long t = (long long)blockIdx.x * KP_THREADS + threadIdx.x, nt = (long long)gridDim.x * KP_THREADS;
    kp_fill_zero(grad_cam, n_cam, t, nt);
    kp_fill_zero(grad_verts, n_verts, t, nt);
}

struct KpBwdArgs {
    const float *kp3d, *pred, *cam, *hps, *stats, *grad_out;
    const int64_t *ind;
    const void *mask;
    const float *jw, *inv_w;
    const int32_t *inv_vertex, *inv_start, *inv_k;
    float *grad_joints, *grad_verts, *grad_cam;
    int P, max_objs, n, HW, K, V, n_touched, mask_type;
};

__global__ __launch_bounds__(KP_THREADS) void kp_bwd_scatter_kernel(const KpBwdArgs a)
{
    __shared__ float s_g[KP_WAVES][2 * H3D_SMPL_KP_MAX_K];       // g_kp3d[k][c], c < 2 (the z component is 0)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int p = blockIdx.x * KP_WAVES + w;                      // wave-uniform
    const bool active = p < a.P;
    const int k = lane >> 1, c = lane & 1;
    int b = 0;
    int64_t ind = -1;
    float s = 0.0f, g = 0.0f, x = 0.0f;
    if (active) {
        const float coef = (float)((double)a.grad_out[0] / ((double)a.stats[2] + 1e-4));      // one rounding
        b = p / a.n;
        const long long slot = (long long)b * a.max_objs + (p - b * a.n);
        ind = a.ind[slot];
        if (ind >= 0 && ind < a.HW) {
            s = a.cam[(long long)b * 3 * a.HW + ind];
            if (k < a.K) {
                const long long o = slot * 2 * a.K + lane;
                const float mk = kp_mask(a.mask, a.mask_type, o);
                const float d = a.pred[(long long)p * 2 * a.K + lane] - a.hps[o];
                g = mk == 0.0f ? 0.0f : coef * kp_sgn(d) * mk;
                x = a.kp3d[((long long)p * a.K + k) * 3 + c];
            }
        } else {
            ind = -1;
        }
    }
    s_g[w][lane] = s * g;
    const float gs = kp_wave_sum(g * x);
    const float gtx = kp_wave_sum(c == 0 ? g : 0.0f);
    const float gty = kp_wave_sum(c == 1 ? g : 0.0f);
    if (lane == 0 && ind >= 0 && a.grad_cam) {
        float *gc = a.grad_cam + (long long)b * 3 * a.HW + ind;
        atomicAdd(gc, gs);
        atomicAdd(gc + a.HW, gtx);
        atomicAdd(gc + 2 * (long long)a.HW, gty);
    }
    __syncthreads();
    if (!active) return;
    if (a.grad_joints) {
        // lane 3 j + cc of 72 (a second round for lanes 0..7): grad_joints[p,j,cc] = sum_k JW[k,j] g_kp3d[p,k,cc], k ascending
        for (int e = lane; e < 72; e += 64) {
            const int j = e / 3, cc = e - 3 * j;
            float acc = 0.0f;
            if (cc < 2)
                for (int kk = 0; kk < a.K; ++kk) acc = acc + a.jw[kk * 24 + j] * s_g[w][2 * kk + cc];
            a.grad_joints[(long long)p * 72 + e] = acc;
        }
    }
    if (a.grad_verts) {
        for (int t = lane; t < a.n_touched; t += 64) {
            const int v = a.inv_vertex[t];
            if ((unsigned)v >= (unsigned)a.V) continue;
            float ax = 0.0f, ay = 0.0f;
            for (int e = a.inv_start[t]; e < a.inv_start[t + 1]; ++e) {
                const int kk = a.inv_k[e];
                if ((unsigned)kk >= (unsigned)a.K) continue;
                const float wt = a.inv_w[e];
                ax = ax + wt * s_g[w][2 * kk];
                ay = ay + wt * s_g[w][2 * kk + 1];
            }
            float *gv = a.grad_verts + ((long long)p * a.V + v) * 3;
            gv[0] = ax;
            gv[1] = ay;
            gv[2] = 0.0f;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static int kp_check_sizes(const char *who, int B, int max_objs, int n, int HW, int K)
{
    if (B <= 0 || max_objs <= 0 || n <= 0 || HW <= 0 || K <= 0)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: B, max_objs, n, HW, K = %d, %d, %d, %d, %d", who, B, max_objs, n, HW, K);
    if (n > max_objs) H3D_FAIL(H3D_ERR_SHAPE, "%s: n = %d > max_objs = %d", who, n, max_objs);
    if ((long long)B * n > 0x7fffffffLL / 96) H3D_FAIL(H3D_ERR_SHAPE, "%s: B n = %lld person slots", who, (long long)B * n);
    if (K > H3D_SMPL_KP_MAX_K) H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: K = %d keypoints, the kernels are built for at most %d", who, K, H3D_SMPL_KP_MAX_K);
    return H3D_OK;
}
static int kp_blocks(int P) { return (P + KP_WAVES - 1) / KP_WAVES; }

struct KpLayout {
    h3d_ws_layout L;
    size_t partials;
};
static KpLayout kp_layout(int P)
{
    KpLayout w;
    w.partials = w.L.take((size_t)kp_blocks(P) * sizeof(f32x2));
    return w;
}

extern "C" int h3d_smpl_kp_loss_workspace_bytes(int B, int n, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "smpl_kp_loss_workspace_bytes: null pointer");
    if (B <= 0 || n <= 0) H3D_FAIL(H3D_ERR_SHAPE, "smpl_kp_loss_workspace_bytes: B, n = %d, %d", B, n);
    if ((long long)B * n > 0x7fffffffLL / 96) H3D_FAIL(H3D_ERR_SHAPE, "smpl_kp_loss_workspace_bytes: B n = %lld person slots", (long long)B * n);
    *bytes = kp_layout(B * n).L.total;
    return H3D_OK;
}

extern "C" int h3d_smpl_kp_loss_forward(const float *joints, const float *verts, const float *cam_map, const int64_t *ind, const float *hps,
                                        const void *hps_mask, int mask_type, const float *joint_w, const int32_t *vert_idx,
                                        const float *vert_w, int B, int max_objs, int n, int HW, int K, int NV, int V, float *kp3d,
                                        float *pred, float *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "smpl_kp_loss_forward";
    H3D_TRY(kp_check_sizes(who, B, max_objs, n, HW, K));
    if (NV < 0 || (NV > 0 && V <= 0)) H3D_FAIL(H3D_ERR_SHAPE, "%s: NV, V = %d, %d", who, NV, V);
    if (NV > H3D_SMPL_KP_MAX_NV) H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: NV = %d vertices per keypoint, the kernels are built for at most %d", who, NV, H3D_SMPL_KP_MAX_NV);
    if (mask_type != H3D_LOSS_MASK_U8 && mask_type != H3D_LOSS_MASK_F32) H3D_FAIL(H3D_ERR_ARG, "%s: mask_type %d", who, mask_type);
    if (!joints || !cam_map || !ind || !hps || !hps_mask || !joint_w || !kp3d || !pred || !stats) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if (NV > 0 && (!verts || !vert_idx || !vert_w)) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer (verts, vert_idx, vert_w with NV > 0)", who);
    const int P = B * n;
    const KpLayout w = kp_layout(P);
    if (!workspace || workspace_bytes < w.L.total || ((uintptr_t)workspace & 7))
        H3D_FAIL(H3D_ERR_ARG, "%s: workspace of %zu bytes (8-byte aligned), %zu needed", who, workspace ? workspace_bytes : (size_t)0, w.L.total);
    KpFwdArgs a;
    a.joints = joints; a.verts = verts; a.cam = cam_map; a.hps = hps; a.ind = ind; a.mask = hps_mask;
    a.jw = joint_w; a.vw = vert_w; a.vi = vert_idx; a.kp3d = kp3d; a.pred = pred;
    a.P = P; a.max_objs = max_objs; a.n = n; a.HW = HW; a.K = K; a.NV = NV; a.V = V; a.mask_type = mask_type;
    const hipStream_t st = (hipStream_t)stream;
    f32x2 *partials = (f32x2 *)((char *)workspace + w.partials);
    H3D_TRY(h3d_launch({"kp_partial_kernel"}, kp_partial_kernel, dim3(kp_blocks(P)), dim3(KP_THREADS), 0, st, a, partials));
    return h3d_launch({"kp_finish_kernel"}, kp_finish_kernel, dim3(1), dim3(64), 0, st, (const f32x2 *)partials, kp_blocks(P), stats);
}

extern "C" int h3d_smpl_kp_loss_backward(const float *kp3d, const float *pred, const float *cam_map, const int64_t *ind, const float *hps,
                                         const void *hps_mask, int mask_type, const float *stats, const float *grad_out,
                                         const float *joint_w, const int32_t *inv_vertex, const int32_t *inv_start, const int32_t *inv_k,
                                         const float *inv_w, int n_touched, int B, int max_objs, int n, int HW, int K, int V,
                                         float *grad_joints, float *grad_verts, float *grad_cam_map, void *stream)
{
    const char *who = "smpl_kp_loss_backward";
    H3D_TRY(kp_check_sizes(who, B, max_objs, n, HW, K));
    if (n_touched < 0 || (grad_verts && V <= 0)) H3D_FAIL(H3D_ERR_SHAPE, "%s: n_touched, V = %d, %d", who, n_touched, V);
    if (n_touched > K * H3D_SMPL_KP_MAX_NV)
        H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: %d touched vertices, at most K x %d = %d", who, n_touched, H3D_SMPL_KP_MAX_NV, K * H3D_SMPL_KP_MAX_NV);
    if (mask_type != H3D_LOSS_MASK_U8 && mask_type != H3D_LOSS_MASK_F32) H3D_FAIL(H3D_ERR_ARG, "%s: mask_type %d", who, mask_type);
    if (!kp3d || !pred || !cam_map || !ind || !hps || !hps_mask || !stats || !grad_out || !joint_w) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if (grad_verts && n_touched > 0 && (!inv_vertex || !inv_start || !inv_k || !inv_w)) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer (inverted table)", who);
    if (!grad_joints && !grad_verts && !grad_cam_map) return H3D_OK;
    const int P = B * n;
    const long long n_cam = grad_cam_map ? (long long)B * 3 * HW : 0, n_verts = grad_verts ? (long long)P * V * 3 : 0;
    const hipStream_t st = (hipStream_t)stream;
    if (n_cam + n_verts > 0) {
        long long nb = (n_cam + n_verts + 4LL * KP_THREADS - 1) / (4LL * KP_THREADS);
        if (nb > KP_FILL_MAX_BLOCKS) nb = KP_FILL_MAX_BLOCKS;
        H3D_TRY(h3d_launch({"kp_bwd_fill_kernel"}, kp_bwd_fill_kernel, dim3((unsigned)nb), dim3(KP_THREADS), 0, st, grad_cam_map, n_cam, grad_verts, n_verts));
    }
    KpBwdArgs a;
    a.kp3d = kp3d; a.pred = pred; a.cam = cam_map; a.hps = hps; a.stats = stats; a.grad_out = grad_out; a.ind = ind; a.mask = hps_mask;
    a.jw = joint_w; a.inv_w = inv_w; a.inv_vertex = inv_vertex; a.inv_start = inv_start; a.inv_k = inv_k;
    a.grad_joints = grad_joints; a.grad_verts = grad_verts; a.grad_cam = grad_cam_map;
    a.P = P; a.max_objs = max_objs; a.n = n; a.HW = HW; a.K = K; a.V = V; a.n_touched = grad_verts ? n_touched : 0; a.mask_type = mask_type;
    return h3d_launch({"kp_bwd_scatter_kernel"}, kp_bwd_scatter_kernel, dim3(kp_blocks(P)), dim3(KP_THREADS), 0, st, a);
}
