// MPJPE / PA-MPJPE / PVE / PA-PVE on the device (include/h3d.h section 8b; h3d_amd/mesh_eval.py; no reference code:
// the project's own definition).
//
// Built with -ffp-contract=off (csrc/Makefile): after the fp32 loads every floating-point step below is ONE IEEE-754 binary64 operation,
// round to nearest, in the order include/h3d.h section 8b states -- tests/mesh_eval_ref.py restates it with loops,
// mesh_eval.evaluate_numpy is its numpy mirror, and everything here is bit-equal to both (sqrt and / are correctly rounded).
//
//   pointset_errors_kernel  one workgroup of four waves per pair, for every n (one path, so the sum order depends on n alone).  Three passes
//                           over the pair's two point sets, each ending in the block sum of section 8b: the count, the two centroids and
//                           the plain error | the centred second moments and the source variance | the aligned error.  Between the
//                           second and the third every thread runs the same 3 x 3 one-sided Jacobi SVD on the same nine sums (uniform
//                           data, so uniform control flow: nothing to broadcast, no barrier), and thread 0 stores the results.
//   metric_means_kernel     one wave: lane l adds the pairs l, l + 64, ... with count > 0 in ascending order, then the shuffle tree.
// No atomics, nothing waits on another workgroup: two calls give the same bits.
#include "common.h"
#include <math.h>

namespace {

constexpr int PE_THREADS = 256;
constexpr int PE_WAVES = PE_THREADS / 64;
constexpr int PE_MAX_SUMS = 10;
constexpr int PE_MAX_SWEEPS = H3D_MESH_EVAL_MAX_SWEEPS;
constexpr double PE_JACOBI_TOL = 0x1p-50;

struct PointsetArgs {
    const float *pred, *gt, *pred_root, *gt_root;
    const int32_t *pred_idx, *gt_idx;
    const uint8_t *weight;
    double *err, *transform;
    int32_t *count;
    int Np, Ng, n, nr, root_a, root_b;
};

// the block sum of section 8b over K values per thread: shuffle tree inside the wave, the four wave partials in wave order; every
// thread returns with the totals.  `slot` alternates between consecutive calls (the second call's writes cannot overtake the first
// call's reads: a barrier of the second call lies between them and the third call's writes).
template <int K> __device__ __forceinline__ void pe_block_sum(double (&v)[K], double (*s_part)[PE_WAVES][PE_MAX_SUMS], int slot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] = v[k] + __shfl_down(v[k], off);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_part[slot][wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = s_part[slot][0][k];
#pragma unroll
        for (int w = 1; w < PE_WAVES; ++w) t = t + s_part[slot][w][k];
        v[k] = t;
    }
}

__device__ __forceinline__ double pe_norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }
__device__ __forceinline__ double pe_dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the similarity of section 8b from the centred moments M[r][c] = sum y_r x_c and var = sum |x|^2: s, R (row-major); t is the caller's
__device__ void pe_similarity(const double (&Min)[9], double var, double &s, double (&R)[9])
{
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    s = 1.0;
    if (var == 0.0) return;
    // columns: A[c][r] = M[r][c], V[c][r] = V[r][c]
    double A[3][3], V[3][3];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) {
            A[c][r] = Min[3 * r + c];
            V[c][r] = r == c ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < PE_MAX_SWEEPS; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double a = pe_dot3(A[p], A[p]), b = pe_dot3(A[q], A[q]), g = pe_dot3(A[p], A[q]);
            if (fabs(g) <= PE_JACOBI_TOL * fmax(a, b)) continue;
            rotated = true;
            const double h = b - a, g2 = 2.0 * g;
            double t;
            if (fabs(g2) <= fabs(h)) {
                const double r = g2 / h;
                t = r / (1.0 + sqrt(1.0 + r * r));
            } else {
                const double z = h / g2;
                const double u = 1.0 / (fabs(z) + sqrt(1.0 + z * z));
                t = z < 0.0 ? -u : u;
            }
            const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double ap = A[p][r], aq = A[q][r], vp = V[p][r], vq = V[q][r];
                A[p][r] = cs * ap - sn * aq;
                A[q][r] = sn * ap + cs * aq;
                V[p][r] = cs * vp - sn * vq;
                V[q][r] = sn * vp + cs * vq;
            }
        }
        if (!rotated) break;
    }
    // the columns by squared norm, largest first, a tie keeps the lower original column first (three strict compare-exchanges)
    const double nn[3] = {pe_dot3(A[0], A[0]), pe_dot3(A[1], A[1]), pe_dot3(A[2], A[2])};
    int o0 = 0, o1 = 1, o2 = 2;
    double dv = 1.0;
    if (nn[o1] > nn[o0]) { const int x = o0; o0 = o1; o1 = x; dv = -dv; }
    if (nn[o2] > nn[o1]) { const int x = o1; o1 = o2; o2 = x; dv = -dv; }
    if (nn[o1] > nn[o0]) { const int x = o0; o0 = o1; o1 = x; dv = -dv; }
    double c0[3], c1[3], c2[3], V0[3], V1[3], V2[3];
    for (int r = 0; r < 3; ++r) {          // (selects, not indexed registers)
        c0[r] = o0 == 0 ? A[0][r] : o0 == 1 ? A[1][r] : A[2][r];
        c1[r] = o1 == 0 ? A[0][r] : o1 == 1 ? A[1][r] : A[2][r];
        c2[r] = o2 == 0 ? A[0][r] : o2 == 1 ? A[1][r] : A[2][r];
        V0[r] = o0 == 0 ? V[0][r] : o0 == 1 ? V[1][r] : V[2][r];
        V1[r] = o1 == 0 ? V[0][r] : o1 == 1 ? V[1][r] : V[2][r];
        V2[r] = o2 == 0 ? V[0][r] : o2 == 1 ? V[1][r] : V[2][r];
    }
    const double S0 = sqrt(o0 == 0 ? nn[0] : o0 == 1 ? nn[1] : nn[2]);
    const double S1 = sqrt(o1 == 0 ? nn[0] : o1 == 1 ? nn[1] : nn[2]);
    const double S2 = sqrt(o2 == 0 ? nn[0] : o2 == 1 ? nn[1] : nn[2]);
    if (S0 == 0.0) {                       // rank 0: every target point at the centroid
        s = 0.0;
        return;
    }
    double U0[3], U1[3], U2[3];
    for (int r = 0; r < 3; ++r) U0[r] = c0[r] / S0;
    bool have = false;
    if (S1 > 0.0) {
        double u[3];
        for (int r = 0; r < 3; ++r) u[r] = c1[r] / S1;
        const double hh = pe_dot3(u, U0);
        for (int r = 0; r < 3; ++r) u[r] = u[r] - hh * U0[r];
        const double nw = pe_norm3(u[0], u[1], u[2]);
        if (nw >= 0.5) {
            have = true;
            for (int r = 0; r < 3; ++r) U1[r] = u[r] / nw;
        }
    }
    if (!have) {                           // rank 1: the axis U0 has the least of (the first of equals), made perpendicular to U0
        int k = 0;
        if (fabs(U0[1]) < fabs(U0[k])) k = 1;
        if (fabs(U0[2]) < fabs(k == 0 ? U0[0] : U0[1])) k = 2;
        const double uk = k == 0 ? U0[0] : k == 1 ? U0[1] : U0[2];
        double u[3];
        for (int r = 0; r < 3; ++r) u[r] = (r == k ? 1.0 : 0.0) - uk * U0[r];
        const double nw = pe_norm3(u[0], u[1], u[2]);
        for (int r = 0; r < 3; ++r) U1[r] = u[r] / nw;
    }
    U2[0] = U0[1] * U1[2] - U0[2] * U1[1];
    U2[1] = U0[2] * U1[0] - U0[0] * U1[2];
    U2[2] = U0[0] * U1[1] - U0[1] * U1[0];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (U0[r] * V0[c] + U1[r] * V1[c]) + dv * (U2[r] * V2[c]);
    const double d = pe_dot3(c2, U2) < 0.0 ? -dv : dv;
    s = ((S0 + S1) + d * S2) / var;
}

__global__ __launch_bounds__(PE_THREADS) void pointset_errors_kernel(const PointsetArgs a)
{
    __shared__ double s_part[2][PE_WAVES][PE_MAX_SUMS];
    const int pair = blockIdx.x, tid = threadIdx.x, n = a.n;
    const int pi = a.pred_idx[pair], gi = a.gt_idx[pair];
    double *err = a.err + (size_t)pair * 2;
    double *tr = a.transform ? a.transform + (size_t)pair * 13 : nullptr;
    if (pi < 0 || pi >= a.Np || gi < 0 || gi >= a.Ng) {          // workgroup-uniform
        if (tid == 0) {
            err[0] = err[1] = 0.0;
            a.count[pair] = 0;
        }
        if (tr && tid < 13) tr[tid] = 0.0;
        return;
    }
    const float *P = a.pred + (size_t)pi * n * 3, *G = a.gt + (size_t)gi * n * 3;
    const uint8_t *W = a.weight ? a.weight + (size_t)gi * n : nullptr;
    double op[3] = {0.0, 0.0, 0.0}, og[3] = {0.0, 0.0, 0.0};
    if (a.pred_root) {
        const float *rp = a.pred_root + (size_t)pi * a.nr * 3, *rg = a.gt_root + (size_t)gi * a.nr * 3;
        for (int c = 0; c < 3; ++c) {
            op[c] = ((double)rp[3 * a.root_a + c] + (double)rp[3 * a.root_b + c]) * 0.5;
            og[c] = ((double)rg[3 * a.root_a + c] + (double)rg[3 * a.root_b + c]) * 0.5;
        }
    }
    // ---- pass 1: the count, the sums of the points, the plain error ----------------------------------------------------------------------
    double v1[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += PE_THREADS) {
        if (W && !W[i]) continue;
        const double p0 = (double)P[3 * i], p1 = (double)P[3 * i + 1], p2 = (double)P[3 * i + 2];
        const double g0 = (double)G[3 * i], g1 = (double)G[3 * i + 1], g2 = (double)G[3 * i + 2];
        v1[0] = v1[0] + p0;
        v1[1] = v1[1] + p1;
        v1[2] = v1[2] + p2;
        v1[3] = v1[3] + g0;
        v1[4] = v1[4] + g1;
        v1[5] = v1[5] + g2;
        v1[6] = v1[6] + pe_norm3((p0 - op[0]) - (g0 - og[0]), (p1 - op[1]) - (g1 - og[1]), (p2 - op[2]) - (g2 - og[2]));
        v1[7] = v1[7] + 1.0;               // (an integer below 2^53: exact in any order)
    }
    pe_block_sum(v1, s_part, 0);
    const int cnt = (int)v1[7];
    if (cnt == 0) {
        if (tid == 0) {
            err[0] = err[1] = 0.0;
            a.count[pair] = 0;
        }
        if (tr && tid < 13) tr[tid] = 0.0;
        return;
    }
    const double dn = v1[7];
    const double mp[3] = {v1[0] / dn, v1[1] / dn, v1[2] / dn}, mg[3] = {v1[3] / dn, v1[4] / dn, v1[5] / dn};
    const double plain = v1[6] / dn;
    // ---- pass 2: the centred second moments M[r][c] = sum y_r x_c and var = sum |x|^2 ------------------------------------------------------
    double v2[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += PE_THREADS) {
        if (W && !W[i]) continue;
        const double x0 = (double)P[3 * i] - mp[0], x1 = (double)P[3 * i + 1] - mp[1], x2 = (double)P[3 * i + 2] - mp[2];
        const double y0 = (double)G[3 * i] - mg[0], y1 = (double)G[3 * i + 1] - mg[1], y2 = (double)G[3 * i + 2] - mg[2];
        v2[0] = v2[0] + y0 * x0;
        v2[1] = v2[1] + y0 * x1;
        v2[2] = v2[2] + y0 * x2;
        v2[3] = v2[3] + y1 * x0;
        v2[4] = v2[4] + y1 * x1;
        v2[5] = v2[5] + y1 * x2;
        v2[6] = v2[6] + y2 * x0;
        v2[7] = v2[7] + y2 * x1;
        v2[8] = v2[8] + y2 * x2;
        v2[9] = v2[9] + ((x0 * x0 + x1 * x1) + x2 * x2);
    }
    pe_block_sum(v2, s_part, 1);
    // ---- the similarity: every thread, on the same sums ----------------------------------------------------------------------------------------
    double M[9], R[9], s, t[3];
    for (int i = 0; i < 9; ++i) M[i] = v2[i];
    pe_similarity(M, v2[9], s, R);
    for (int r = 0; r < 3; ++r) t[r] = mg[r] - s * ((R[3 * r] * mp[0] + R[3 * r + 1] * mp[1]) + R[3 * r + 2] * mp[2]);
    // ---- pass 3: the aligned error -------------------------------------------------------------------------------------------------------------
    double v3[1] = {0.0};
    for (int i = tid; i < n; i += PE_THREADS) {
        if (W && !W[i]) continue;
        const double p0 = (double)P[3 * i], p1 = (double)P[3 * i + 1], p2 = (double)P[3 * i + 2];
        double d[3];
        for (int r = 0; r < 3; ++r) d[r] = (s * ((R[3 * r] * p0 + R[3 * r + 1] * p1) + R[3 * r + 2] * p2) + t[r]) - (double)G[3 * i + r];
        v3[0] = v3[0] + pe_norm3(d[0], d[1], d[2]);
    }
    pe_block_sum(v3, s_part, 0);
    if (tid == 0) {
        err[0] = plain;
        err[1] = v3[0] / dn;
        a.count[pair] = cnt;
        if (tr) {
            tr[0] = s;
            for (int i = 0; i < 9; ++i) tr[1 + i] = R[i];
            for (int r = 0; r < 3; ++r) tr[10 + r] = t[r];
        }
    }
}

__global__ __launch_bounds__(64) void metric_means_kernel(const double *__restrict__ err, const int32_t *__restrict__ count, int P,
                                                          double *__restrict__ means, int32_t *__restrict__ n_pairs)
{
    const int lane = threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    int c = 0;
    for (int i = lane; i < P; i += 64) {
        if (count[i] <= 0) continue;
        s0 = s0 + err[2 * (size_t)i];
        s1 = s1 + err[2 * (size_t)i + 1];
        ++c;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 = s0 + __shfl_down(s0, off);
        s1 = s1 + __shfl_down(s1, off);
        c += __shfl_down(c, off);
    }
    if (lane == 0) {
        means[0] = c ? s0 / (double)c : 0.0;
        means[1] = c ? s1 / (double)c : 0.0;
        *n_pairs = c;
    }
}

}  // namespace

extern "C" int h3d_pointset_errors(const float *pred, int Np, const float *gt, int Ng, int n, const int32_t *pred_idx, const int32_t *gt_idx,
                                   int P, const uint8_t *weight, const float *pred_root, const float *gt_root, int nr, int root_a, int root_b,
                                   double *err, int32_t *count, double *transform, void *stream)
{
    const char *who = "pointset_errors";
    if (n <= 0 || P < 0 || Np < 0 || Ng < 0) H3D_FAIL(H3D_ERR_ARG, "%s: n = %d, P = %d, Np = %d, Ng = %d", who, n, P, Np, Ng);
    if ((double)n * 3.0 >= 2147483648.0) H3D_FAIL(H3D_ERR_ARG, "%s: n = %d, 3 n must stay below 2^31", who, n);
    if ((pred_root != nullptr) != (gt_root != nullptr)) H3D_FAIL(H3D_ERR_ARG, "%s: one root source without the other", who);
    if (pred_root && (nr <= 0 || root_a < 0 || root_a >= nr || root_b < 0 || root_b >= nr || (double)nr * 3.0 >= 2147483648.0))
        H3D_FAIL(H3D_ERR_ARG, "%s: roots %d and %d of nr = %d", who, root_a, root_b, nr);
    if (P == 0) return H3D_OK;
    if (!pred_idx || !gt_idx || !err || !count) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if ((Np > 0 && !pred) || (Ng > 0 && !gt)) H3D_FAIL(H3D_ERR_ARG, "%s: null point set", who);
    if (((uintptr_t)err | (uintptr_t)transform) & 7) H3D_FAIL(H3D_ERR_ARG, "%s: misaligned pointer (fp64 needs 8 bytes)", who);
    PointsetArgs a;
    a.pred = pred, a.gt = gt, a.pred_root = pred_root, a.gt_root = gt_root, a.pred_idx = pred_idx, a.gt_idx = gt_idx, a.weight = weight;
    a.err = err, a.transform = transform, a.count = count;
    a.Np = Np, a.Ng = Ng, a.n = n, a.nr = nr, a.root_a = root_a, a.root_b = root_b;
    return h3d_launch({"pointset_errors_kernel"}, pointset_errors_kernel, dim3((unsigned)P), dim3(PE_THREADS), 0, (hipStream_t)stream, a);
}

extern "C" int h3d_metric_means(const double *err, const int32_t *count, int P, double *means, int32_t *n_pairs, void *stream)
{
    const char *who = "metric_means";
    if (P < 0) H3D_FAIL(H3D_ERR_ARG, "%s: P = %d", who, P);
    if (!means || !n_pairs || (P > 0 && (!err || !count))) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if (((uintptr_t)err | (uintptr_t)means) & 7) H3D_FAIL(H3D_ERR_ARG, "%s: misaligned pointer (fp64 needs 8 bytes)", who);
    return h3d_launch({"metric_means_kernel"}, metric_means_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, err, count, P, means, n_pairs);
}
