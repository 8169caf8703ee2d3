// SMPL 3D supervision (include/h3d.h section 4e; no reference code: the project's own definition): the label
// transform that moves SMPL pose / 3D-joint labels with the augmentation, and one fused loss with three terms -- rotation matrices,
// betas, root-relative 3D joints -- read in place from the `pose` / `shape` head maps.
//
//   sup_labels_kernel       one lane per (image, row, joint): Rodrigues of the label in fp64, the mirror (S R S on the swapped joint), the
//                           in-plane rotation of the root and of the joints, the gated weights; everything rounded to fp32 once.
//   sup_partial_kernel      one wave per slot p = b n + m, four per workgroup.  Lanes j < 24: R[j] = smpl_rodrigues<float> of the head's
//                           theta and the pose term; lanes 32 .. 41: the shape term; lanes j < 24 again: the joint term from the slot's
//                           72 + 72 coordinates in LDS, both roots formed once per wave.  Six fp32 sums per lane -> wave shuffles -> LDS ->
//                           the six values of the workgroup by plain stores.
//   sup_finish_kernel       one wave sums the partials in a fixed order in fp64 and writes stats[9] = {loss, l, num} x 3.
//   sup_bwd_fill_kernel     zero fill of grad_pose_map and grad_shape_map (16-byte stores, scalar head and tail).
//   sup_bwd_scatter_kernel  one wave per slot: the 72 pose gradients (Rodrigues, residual and derivative in fp64, rounded once) and the 10
//                           shape gradients by float atomic adds into the zeroed maps (two slots may share a pixel) -- ordered behind the
//                           fill by the launch boundary; grad_joints by plain stores, the root share by a shuffle tree.
// No float atomics in the forward.  Compiled with -ffp-contract=off: the definition is a sequence of separately rounded products and sums.
#include "smpl_pose.h"

constexpr int SUP_THREADS = 256;
constexpr int SUP_WAVES = SUP_THREADS / 64;
constexpr int SUP_FILL_MAX_BLOCKS = 2048;
constexpr int SUP_SHAPE_LANE = 32;          // lanes 32 .. 41 hold the ten betas

// the mirror's joint permutation: left / right pairs (1,2) (4,5) (7,8) (10,11) (13,14) (16,17) (18,19) (20,21) (22,23)
__device__ __forceinline__ int sup_mirror_joint(int j)
{
    if (j == 0 || j == 3 || j == 6 || j == 9 || j == 12 || j == 15) return j;
    if (j < 18) return (j % 3 == 1) ? j + 1 : j - 1;
    return (j & 1) ? j - 1 : j + 1;
}
__device__ __forceinline__ float sup_wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// ---- labels --------------------------------------------------------------------------------------------------------------------------
struct SupLabelArgs {
    const float *pose, *shape, *joints, *valid, *pose_w, *joints_w;
    const int32_t *num, *flipped;
    const uint8_t *reg_mask;
    const double *rot2;
    float *o_rotmat, *o_pose_w, *o_shape, *o_shape_w, *o_joints, *o_joints_w;
    int B, M, max_objs;
};

__global__ __launch_bounds__(SUP_THREADS) void sup_labels_kernel(const SupLabelArgs a)
{
    const long long t = (long long)blockIdx.x * SUP_THREADS + threadIdx.x;
    if (t >= (long long)a.B * a.max_objs * SMPL_J) return;
    const int j = (int)(t % SMPL_J);
    const long long row = t / SMPL_J;                   // b max_objs + m
    const int m = (int)(row % a.max_objs), b = (int)(row / a.max_objs);
    int lim = a.num[b];
    lim = lim < a.max_objs ? lim : a.max_objs;
    lim = lim < a.M ? lim : a.M;
    const long long src = (long long)b * a.M + m;       // read only when `gate`
    bool gate = m < lim && a.reg_mask[row] != 0;
    float v = 0.0f;
    if (gate) {
        v = a.valid[src];
        gate = v != 0.0f;                               // (a NaN valid passes: the weight is then NaN, as the caller asked)
    }
    const bool flip = a.flipped && a.flipped[b] != 0;
    const int js = flip ? sup_mirror_joint(j) : j;      // the label joint this output joint comes from
    float wp = 0.0f, wj = 0.0f;
    if (gate) {
        wp = a.pose_w ? a.pose_w[src * SMPL_J + js] : v;
        if (a.joints) wj = a.joints_w ? a.joints_w[src * SMPL_J + js] : v;
    }
    double A00 = 1.0, A01 = 0.0, A10 = 0.0, A11 = 1.0;
    if (a.rot2) {
        const double *r = a.rot2 + (long long)b * 4;
        A00 = r[0]; A01 = r[1]; A10 = r[2]; A11 = r[3];
    }
    float R[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (wp != 0.0f) {
        const float *th = a.pose + src * 72 + js * 3;
        const SmplRot<double> r = smpl_rodrigues<double>((double)th[0], (double)th[1], (double)th[2]);
        double Q[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) Q[i] = r.R[i];
        if (flip) { Q[1] = -Q[1]; Q[2] = -Q[2]; Q[3] = -Q[3]; Q[6] = -Q[6]; }          // S R S, S = diag(-1, 1, 1)
        if (j == 0 && a.rot2) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double q0 = Q[c], q1 = Q[3 + c];
                Q[c] = A00 * q0 + A01 * q1;
                Q[3 + c] = A10 * q0 + A11 * q1;
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = (float)Q[i];
    }
    float J[3] = {0.0f, 0.0f, 0.0f};
    if (wj != 0.0f) {
        const float *jp = a.joints + (src * SMPL_J + js) * 3;
        double x = (double)jp[0];
        const double y = (double)jp[1];
        if (flip) x = -x;
        J[0] = (float)(A00 * x + A01 * y);
        J[1] = (float)(A10 * x + A11 * y);
        J[2] = jp[2];
    }
    float *ro = a.o_rotmat + t * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) ro[i] = R[i];
    a.o_pose_w[t] = wp;
    a.o_joints[t * 3] = J[0]; a.o_joints[t * 3 + 1] = J[1]; a.o_joints[t * 3 + 2] = J[2];
    a.o_joints_w[t] = wj;
    if (j < SMPL_NB) a.o_shape[row * SMPL_NB + j] = gate ? a.shape[src * SMPL_NB + j] : 0.0f;
    if (j == SMPL_NB) a.o_shape_w[row] = gate ? v : 0.0f;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------
struct SupArgs {
    const float *pose_map, *shape_map, *joints, *rotmat, *pose_w, *shape, *shape_w, *joints_lab, *joints_w;
    const int64_t *ind;
    int P, max_objs, n, HW;
};

__global__ __launch_bounds__(SUP_THREADS) void sup_partial_kernel(const SupArgs a, float *__restrict__ partials)
{
    __shared__ float s_j[SUP_WAVES][72], s_l[SUP_WAVES][72];
    __shared__ float s_red[SUP_WAVES][6];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int p = blockIdx.x * SUP_WAVES + w;           // wave-uniform
    const bool active = p < a.P;
    int b = 0;
    long long slot = 0;
    int64_t ind = -1;
    if (active) {
        b = p / a.n;
        slot = (long long)b * a.max_objs + (p - b * a.n);
        ind = a.ind[slot];
        if (ind < 0 || ind >= a.HW) ind = -1;
    }
    const bool ok = ind >= 0;                           // wave-uniform
    const bool with_j = ok && a.joints != nullptr;
    if (with_j) {
        const float *jp = a.joints + (long long)p * 72, *lp = a.joints_lab + slot * 72;
        s_j[w][lane] = jp[lane];
        s_l[w][lane] = lp[lane];
        if (lane < 8) {
            s_j[w][64 + lane] = jp[64 + lane];
            s_l[w][64 + lane] = lp[64 + lane];
        }
    }
    __syncthreads();
    float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};        // l_pose, sum wp, l_shape, sum ws, l_j3d, sum wj
    if (ok && lane < SMPL_J) {
        const float wp = a.pose_w[slot * SMPL_J + lane];
        if (wp != 0.0f) {
            const float *tp = a.pose_map + ((long long)b * 72 + lane * 3) * a.HW + ind;
            const SmplRot<float> r = smpl_rodrigues<float>(tp[0], tp[a.HW], tp[2 * (long long)a.HW]);
            const float *lab = a.rotmat + (slot * SMPL_J + lane) * 9;
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const float d = r.R[i] - lab[i];
                acc = acc + d * d;
            }
            v[0] = wp * acc;
            v[1] = wp;
        }
    }
    if (ok && lane >= SUP_SHAPE_LANE && lane < SUP_SHAPE_LANE + SMPL_NB) {
        const int k = lane - SUP_SHAPE_LANE;
        const float ws = a.shape_w[slot];
        if (ws != 0.0f) {
            const float d = a.shape_map[((long long)b * SMPL_NB + k) * a.HW + ind] - a.shape[slot * SMPL_NB + k];
            v[2] = ws * (d * d);
            if (k == 0) v[3] = ws;
        }
    }
    if (with_j) {
        // both roots once per wave: lane c < 3 forms 0.5 (X[1][c] + X[2][c]) of the prediction and of the label
        float rp = 0.0f, rl = 0.0f;
        if (lane < 3) {
            rp = 0.5f * (s_j[w][3 + lane] + s_j[w][6 + lane]);
            rl = 0.5f * (s_l[w][3 + lane] + s_l[w][6 + lane]);
        }
        const float rp0 = __shfl(rp, 0), rp1 = __shfl(rp, 1), rp2 = __shfl(rp, 2);
        const float rl0 = __shfl(rl, 0), rl1 = __shfl(rl, 1), rl2 = __shfl(rl, 2);
        if (lane < SMPL_J) {
            const float wj = a.joints_w[slot * SMPL_J + lane];
            if (wj != 0.0f) {
                const float dx = (s_j[w][3 * lane] - rp0) - (s_l[w][3 * lane] - rl0);
                const float dy = (s_j[w][3 * lane + 1] - rp1) - (s_l[w][3 * lane + 1] - rl1);
                const float dz = (s_j[w][3 * lane + 2] - rp2) - (s_l[w][3 * lane + 2] - rl2);
                v[4] = wj * ((dx * dx + dy * dy) + dz * dz);
                v[5] = wj;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = sup_wave_sum(v[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) s_red[w][i] = v[i];
    }
    __syncthreads();
    if (tid < 6) {
        float o = 0.0f;
#pragma unroll
        for (int i = 0; i < SUP_WAVES; ++i) o += s_red[i][tid];
        partials[(long long)blockIdx.x * 6 + tid] = o;
    }
}

__global__ __launch_bounds__(64) void sup_finish_kernel(const float *__restrict__ partials, int nparts, float *__restrict__ stats)
{
    const int lane = threadIdx.x;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < nparts; i += 64) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += (double)partials[(long long)i * 6 + k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += __shfl_down(s[k], off);
    }
    if (lane == 0) {
        const double per[3] = {9.0, 10.0, 3.0};
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const double l = s[2 * t], num = per[t] * s[2 * t + 1];
            stats[3 * t] = (float)(l / (num + 1e-4));
            stats[3 * t + 1] = (float)l;
            stats[3 * t + 2] = (float)num;
        }
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------
// zero fill of n floats at any 4-byte aligned pointer by `nthreads` threads, of which this is thread `t`
__device__ __forceinline__ void sup_fill_zero(float *p, long long n, long long t, long long nthreads)
{
    if (!p || n <= 0) return;
    long long head = (long long)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const long long nvec = (n - head) >> 2, tail0 = head + 4 * nvec;
    if (t < head) p[t] = 0.0f;
    if (t >= 32 && tail0 + (t - 32) < n) p[tail0 + (t - 32)] = 0.0f;      // at most 3 tail elements, owned by threads 32..34
    for (long long v = t; v < nvec; v += nthreads) *reinterpret_cast<f32x4 *>(p + head + 4 * v) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}
__global__ __launch_bounds__(SUP_THREADS) void sup_bwd_fill_kernel(float *__restrict__ grad_pose, long long n_pose, float *__restrict__ grad_shape,
                                                                   long long n_shape)
{
    const long long t = (long long)blockIdx.x * SUP_THREADS + threadIdx.x, nt = (long long)gridDim.x * SUP_THREADS;
    sup_fill_zero(grad_pose, n_pose, t, nt);
    sup_fill_zero(grad_shape, n_shape, t, nt);
}

struct SupBwdArgs {
    SupArgs f;
    const float *stats, *grad_out;
    float *grad_pose, *grad_shape, *grad_joints;
};

// d(sum_i G[i] R[i]) / d theta for R = smpl_rodrigues<double>(theta): reverse mode through R(x, y, z, sn, oc), (sn, oc)(angle),
// (x, y, z) = theta / angle, angle = ||theta + 1e-8||
__device__ __forceinline__ void sup_rodrigues_vjp(const SmplRot<double> &r, const double (&th)[3], const double (&G)[9], double (&g)[3])
{
    const double x = r.x, y = r.y, z = r.z, sn = r.sn, cs = r.cs, oc = r.oc, inv = r.inv;
    const double s13 = G[1] + G[3], s26 = G[2] + G[6], s57 = G[5] + G[7];
    const double g_sn = (G[3] - G[1]) * z + (G[2] - G[6]) * y + (G[7] - G[5]) * x;
    const double g_oc = G[0] * (-(y * y) - z * z) + s13 * (x * y) + s26 * (x * z) + G[4] * (-(x * x) - z * z) + s57 * (y * z) +
                        G[8] * (-(x * x) - y * y);
    const double g_x = oc * (s13 * y + s26 * z - 2.0 * x * (G[4] + G[8])) + sn * (G[7] - G[5]);
    const double g_y = oc * (s13 * x + s57 * z - 2.0 * y * (G[0] + G[8])) + sn * (G[2] - G[6]);
    const double g_z = oc * (s26 * x + s57 * y - 2.0 * z * (G[0] + G[4])) + sn * (G[3] - G[1]);
    const double g_inv = g_x * th[0] + g_y * th[1] + g_z * th[2];
    const double g_angle = g_sn * cs + g_oc * sn - g_inv * inv * inv;
    g[0] = g_x * inv + g_angle * r.ex * inv;
    g[1] = g_y * inv + g_angle * r.ey * inv;
    g[2] = g_z * inv + g_angle * r.ez * inv;
}

__global__ __launch_bounds__(SUP_THREADS) void sup_bwd_scatter_kernel(const SupBwdArgs a)
{
    __shared__ float s_j[SUP_WAVES][72], s_l[SUP_WAVES][72];
    const SupArgs &f = a.f;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int p = blockIdx.x * SUP_WAVES + w;           // wave-uniform
    const bool active = p < f.P;
    int b = 0;
    long long slot = 0;
    int64_t ind = -1;
    if (active) {
        b = p / f.n;
        slot = (long long)b * f.max_objs + (p - b * f.n);
        ind = f.ind[slot];
        if (ind < 0 || ind >= f.HW) ind = -1;
    }
    const bool ok = ind >= 0;                           // wave-uniform
    const bool want_j = active && a.grad_joints != nullptr;
    const bool with_j = ok && want_j;
    if (with_j) {
        const float *jp = f.joints + (long long)p * 72, *lp = f.joints_lab + slot * 72;
        s_j[w][lane] = jp[lane];
        s_l[w][lane] = lp[lane];
        if (lane < 8) {
            s_j[w][64 + lane] = jp[64 + lane];
            s_l[w][64 + lane] = lp[64 + lane];
        }
    }
    __syncthreads();
    if (!active) return;
    if (ok && a.grad_pose && lane < SMPL_J) {
        const float wp = f.pose_w[slot * SMPL_J + lane];
        if (wp != 0.0f) {
            const float coef = (float)((double)a.grad_out[0] / ((double)a.stats[2] + 1e-4));       // one rounding
            float *gp = a.grad_pose + ((long long)b * 72 + lane * 3) * f.HW + ind;
            const float *tp = f.pose_map + ((long long)b * 72 + lane * 3) * f.HW + ind;
            const double th[3] = {(double)tp[0], (double)tp[f.HW], (double)tp[2 * (long long)f.HW]};
            const SmplRot<double> r = smpl_rodrigues<double>(th[0], th[1], th[2]);
            const float *lab = f.rotmat + (slot * SMPL_J + lane) * 9;
            const double k2 = 2.0 * (double)coef * (double)wp;
            double G[9], g[3];
#pragma unroll
            for (int i = 0; i < 9; ++i) G[i] = k2 * (r.R[i] - (double)lab[i]);
            sup_rodrigues_vjp(r, th, G, g);
            atomicAdd(gp, (float)g[0]);
            atomicAdd(gp + f.HW, (float)g[1]);
            atomicAdd(gp + 2 * (long long)f.HW, (float)g[2]);
        }
    }
    if (ok && a.grad_shape && lane >= SUP_SHAPE_LANE && lane < SUP_SHAPE_LANE + SMPL_NB) {
        const int k = lane - SUP_SHAPE_LANE;
        const float ws = f.shape_w[slot];
        if (ws != 0.0f) {
            const float coef = (float)((double)a.grad_out[1] / ((double)a.stats[5] + 1e-4));
            const long long at = ((long long)b * SMPL_NB + k) * f.HW + ind;
            const float d = f.shape_map[at] - f.shape[slot * SMPL_NB + k];
            atomicAdd(a.grad_shape + at, ((2.0f * coef) * ws) * d);
        }
    }
    if (want_j) {
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        if (with_j) {
            float rp = 0.0f, rl = 0.0f;
            if (lane < 3) {
                rp = 0.5f * (s_j[w][3 + lane] + s_j[w][6 + lane]);
                rl = 0.5f * (s_l[w][3 + lane] + s_l[w][6 + lane]);
            }
            const float rp0 = __shfl(rp, 0), rp1 = __shfl(rp, 1), rp2 = __shfl(rp, 2);
            const float rl0 = __shfl(rl, 0), rl1 = __shfl(rl, 1), rl2 = __shfl(rl, 2);
            if (lane < SMPL_J) {
                const float wj = f.joints_w[slot * SMPL_J + lane];
                if (wj != 0.0f) {
                    const float coef = (float)((double)a.grad_out[2] / ((double)a.stats[8] + 1e-4));
                    const float k2 = (2.0f * coef) * wj;
                    gx = k2 * ((s_j[w][3 * lane] - rp0) - (s_l[w][3 * lane] - rl0));
                    gy = k2 * ((s_j[w][3 * lane + 1] - rp1) - (s_l[w][3 * lane + 1] - rl1));
                    gz = k2 * ((s_j[w][3 * lane + 2] - rp2) - (s_l[w][3 * lane + 2] - rl2));
                }
            }
        }
        // the root share: joints 1 and 2 each receive -0.5 sum_j g_j (the shuffle tree's fixed order; lanes >= 24 hold zeros)
        const float sx = __shfl(sup_wave_sum(gx), 0), sy = __shfl(sup_wave_sum(gy), 0), sz = __shfl(sup_wave_sum(gz), 0);
        if (lane == 1 || lane == 2) {
            gx = gx - 0.5f * sx;
            gy = gy - 0.5f * sy;
            gz = gz - 0.5f * sz;
        }
        if (lane < SMPL_J) {
            float *gj = a.grad_joints + (long long)p * 72 + 3 * lane;
            gj[0] = gx; gj[1] = gy; gj[2] = gz;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static int sup_blocks(int P) { return (P + SUP_WAVES - 1) / SUP_WAVES; }
static bool sup_misaligned(const void *p, unsigned mask) { return ((uintptr_t)p & mask) != 0; }

struct SupLayout {
    h3d_ws_layout L;
    size_t partials;
};
static SupLayout sup_layout(int P)
{
    SupLayout w;
    w.partials = w.L.take((size_t)sup_blocks(P) * 6 * sizeof(float));
    return w;
}

static int sup_check_sizes(const char *who, int B, int max_objs, int n, int HW)
{
    if (B <= 0 || max_objs <= 0 || n <= 0 || HW <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: B, max_objs, n, HW = %d, %d, %d, %d", who, B, max_objs, n, HW);
    if (n > max_objs) H3D_FAIL(H3D_ERR_SHAPE, "%s: n = %d > max_objs = %d", who, n, max_objs);
    if ((long long)B * max_objs > 0x7fffffffLL / 216) H3D_FAIL(H3D_ERR_SHAPE, "%s: B max_objs = %lld label rows", who, (long long)B * max_objs);
    return H3D_OK;
}

extern "C" int h3d_smpl_sup_labels(const float *pose_lab, const float *shape_lab, const float *joints_lab, const float *valid, const float *pose_w,
                                   const float *joints_w, const int32_t *num, const uint8_t *reg_mask, const int32_t *flipped, const double *rot2,
                                   int B, int M, int max_objs, float *smpl_rotmat, float *smpl_pose_w, float *smpl_shape, float *smpl_shape_w,
                                   float *smpl_joints, float *smpl_joints_w, void *stream)
{
    const char *who = "smpl_sup_labels";
    if (B <= 0 || M <= 0 || max_objs <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: B, M, max_objs = %d, %d, %d", who, B, M, max_objs);
    if ((long long)B * max_objs > 0x7fffffffLL / 216 || (long long)B * M > 0x7fffffffLL / 216)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: B max_objs = %lld, B M = %lld label rows", who, (long long)B * max_objs, (long long)B * M);
    if (!pose_lab || !shape_lab || !valid || !num || !reg_mask || !smpl_rotmat || !smpl_pose_w || !smpl_shape || !smpl_shape_w || !smpl_joints ||
        !smpl_joints_w)
        H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if (joints_w && !joints_lab) H3D_FAIL(H3D_ERR_ARG, "%s: joints_w without joints_lab", who);
    for (const void *q : {(const void *)pose_lab, (const void *)shape_lab, (const void *)joints_lab, (const void *)valid, (const void *)pose_w,
                          (const void *)joints_w, (const void *)num, (const void *)flipped, (const void *)smpl_rotmat, (const void *)smpl_pose_w,
                          (const void *)smpl_shape, (const void *)smpl_shape_w, (const void *)smpl_joints, (const void *)smpl_joints_w})
        if (sup_misaligned(q, 3)) H3D_FAIL(H3D_ERR_ARG, "%s: a pointer is not 4-byte aligned", who);
    if (sup_misaligned(rot2, 7)) H3D_FAIL(H3D_ERR_ARG, "%s: rot2 is not 8-byte aligned", who);
    SupLabelArgs a;
    a.pose = pose_lab; a.shape = shape_lab; a.joints = joints_lab; a.valid = valid; a.pose_w = pose_w; a.joints_w = joints_w;
    a.num = num; a.flipped = flipped; a.reg_mask = reg_mask; a.rot2 = rot2;
    a.o_rotmat = smpl_rotmat; a.o_pose_w = smpl_pose_w; a.o_shape = smpl_shape; a.o_shape_w = smpl_shape_w; a.o_joints = smpl_joints;
    a.o_joints_w = smpl_joints_w;
    a.B = B; a.M = M; a.max_objs = max_objs;
    const long long lanes = (long long)B * max_objs * SMPL_J;
    return h3d_launch({"sup_labels_kernel"}, sup_labels_kernel, dim3((unsigned)((lanes + SUP_THREADS - 1) / SUP_THREADS)), dim3(SUP_THREADS), 0,
                      (hipStream_t)stream, a);
}

extern "C" int h3d_smpl_sup_loss_workspace_bytes(int B, int n, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "smpl_sup_loss_workspace_bytes: null pointer");
    if (B <= 0 || n <= 0) H3D_FAIL(H3D_ERR_SHAPE, "smpl_sup_loss_workspace_bytes: B, n = %d, %d", B, n);
    if ((long long)B * n > 0x7fffffffLL / 216) H3D_FAIL(H3D_ERR_SHAPE, "smpl_sup_loss_workspace_bytes: B n = %lld person slots", (long long)B * n);
    *bytes = sup_layout(B * n).L.total;
    return H3D_OK;
}

// the checks both loss entry points share; fills `a`
static int sup_loss_args(const char *who, const float *pose_map, const float *shape_map, const int64_t *ind, const float *joints, const float *rotmat,
                         const float *pose_w, const float *shape, const float *shape_w, const float *joints_lab, const float *joints_w, int B,
                         int max_objs, int n, int HW, SupArgs &a)
{
    H3D_TRY(sup_check_sizes(who, B, max_objs, n, HW));
    if (!pose_map || !shape_map || !ind || !rotmat || !pose_w || !shape || !shape_w) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if (joints && (!joints_lab || !joints_w)) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer (joints_lab, joints_w with joints)", who);
    for (const void *q : {(const void *)pose_map, (const void *)shape_map, (const void *)joints, (const void *)rotmat, (const void *)pose_w,
                          (const void *)shape, (const void *)shape_w, (const void *)joints_lab, (const void *)joints_w})
        if (sup_misaligned(q, 3)) H3D_FAIL(H3D_ERR_ARG, "%s: a pointer is not 4-byte aligned", who);
    if (sup_misaligned(ind, 7)) H3D_FAIL(H3D_ERR_ARG, "%s: ind is not 8-byte aligned", who);
    a.pose_map = pose_map; a.shape_map = shape_map; a.joints = joints; a.rotmat = rotmat; a.pose_w = pose_w; a.shape = shape; a.shape_w = shape_w;
    a.joints_lab = joints_lab; a.joints_w = joints_w; a.ind = ind;
    a.P = B * n; a.max_objs = max_objs; a.n = n; a.HW = HW;
    return H3D_OK;
}

extern "C" int h3d_smpl_sup_loss_forward(const float *pose_map, const float *shape_map, const int64_t *ind, const float *joints,
                                         const float *smpl_rotmat, const float *smpl_pose_w, const float *smpl_shape, const float *smpl_shape_w,
                                         const float *smpl_joints, const float *smpl_joints_w, int B, int max_objs, int n, int HW, float *stats,
                                         void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "smpl_sup_loss_forward";
    SupArgs a;
    H3D_TRY(sup_loss_args(who, pose_map, shape_map, ind, joints, smpl_rotmat, smpl_pose_w, smpl_shape, smpl_shape_w, smpl_joints, smpl_joints_w, B,
                          max_objs, n, HW, a));
    if (!stats || sup_misaligned(stats, 3)) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer (stats) or not 4-byte aligned", who);
    const SupLayout w = sup_layout(a.P);
    if (!workspace || workspace_bytes < w.L.total || sup_misaligned(workspace, 7))
        H3D_FAIL(H3D_ERR_ARG, "%s: workspace of %zu bytes (8-byte aligned), %zu needed", who, workspace ? workspace_bytes : (size_t)0, w.L.total);
    const hipStream_t st = (hipStream_t)stream;
    float *partials = (float *)((char *)workspace + w.partials);
    H3D_TRY(h3d_launch({"sup_partial_kernel"}, sup_partial_kernel, dim3(sup_blocks(a.P)), dim3(SUP_THREADS), 0, st, a, partials));
    return h3d_launch({"sup_finish_kernel"}, sup_finish_kernel, dim3(1), dim3(64), 0, st, (const float *)partials, sup_blocks(a.P), stats);
}

extern "C" int h3d_smpl_sup_loss_backward(const float *pose_map, const float *shape_map, const int64_t *ind, const float *joints,
                                          const float *smpl_rotmat, const float *smpl_pose_w, const float *smpl_shape, const float *smpl_shape_w,
                                          const float *smpl_joints, const float *smpl_joints_w, int B, int max_objs, int n, int HW, const float *stats,
                                          const float *grad_out, float *grad_pose_map, float *grad_shape_map, float *grad_joints, void *stream)
{
    const char *who = "smpl_sup_loss_backward";
    SupBwdArgs a;
    H3D_TRY(sup_loss_args(who, pose_map, shape_map, ind, joints, smpl_rotmat, smpl_pose_w, smpl_shape, smpl_shape_w, smpl_joints, smpl_joints_w, B,
                          max_objs, n, HW, a.f));
    if (!stats || !grad_out) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer (stats, grad_out)", who);
    if (grad_joints && !joints) H3D_FAIL(H3D_ERR_ARG, "%s: grad_joints without joints", who);
    for (const void *q : {(const void *)stats, (const void *)grad_out, (const void *)grad_pose_map, (const void *)grad_shape_map, (const void *)grad_joints})
        if (sup_misaligned(q, 3)) H3D_FAIL(H3D_ERR_ARG, "%s: a pointer is not 4-byte aligned", who);
    if (!grad_pose_map && !grad_shape_map && !grad_joints) return H3D_OK;
    const long long n_pose = grad_pose_map ? (long long)B * 72 * HW : 0, n_shape = grad_shape_map ? (long long)B * SMPL_NB * HW : 0;
    const hipStream_t st = (hipStream_t)stream;
    if (n_pose + n_shape > 0) {
        long long nb = (n_pose + n_shape + 4LL * SUP_THREADS - 1) / (4LL * SUP_THREADS);
        if (nb > SUP_FILL_MAX_BLOCKS) nb = SUP_FILL_MAX_BLOCKS;
        H3D_TRY(h3d_launch({"sup_bwd_fill_kernel"}, sup_bwd_fill_kernel, dim3((unsigned)nb), dim3(SUP_THREADS), 0, st, grad_pose_map, n_pose,
                           grad_shape_map, n_shape));
    }
    a.stats = stats; a.grad_out = grad_out; a.grad_pose = grad_pose_map; a.grad_shape = grad_shape_map; a.grad_joints = grad_joints;
    return h3d_launch({"sup_bwd_scatter_kernel"}, sup_bwd_scatter_kernel, dim3(sup_blocks(a.f.P)), dim3(SUP_THREADS), 0, st, a);
}
