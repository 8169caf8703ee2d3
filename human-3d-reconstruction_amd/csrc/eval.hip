// COCO keypoint (OKS) and box AP evaluation on the device (include/h3d.h section 8; h3d_amd/coco_eval.py).
//
// Built with -ffp-contract=off (csrc/Makefile): every floating-point step below is ONE IEEE-754 binary64 operation, round to nearest,
// in the order include/h3d.h section 8 states -- tests/coco_eval_ref.py restates it with loops, coco_eval.evaluate_numpy is its numpy
// mirror, and everything here but the OKS matrix (exp is the one inexact operation) is bit-equal to both.
//
//   coco_match_kernel       one workgroup of two waves per image: the rounded records, the stable in-image score ranks, the D x G IoU / OKS
//                           matrix (row-major in LDS when it fits, else in global memory), then one lane per (area range, threshold)
//                           runs COCOeval's greedy walk over the detections in score order.  The lanes of one area range read the same
//                           matrix element (an LDS broadcast); lanes of different area ranges read other columns of the SAME row, so a
//                           row-major image keeps the at most four distinct addresses of a step on different banks unless two columns
//                           are 32 apart.
//   coco_npig_kernel        the non-ignored ground truths per (class, area range): an integer count in LDS, one workgroup per cell.
//   coco_accumulate_kernel  one workgroup per (class, area range, maxDet, threshold) row: the flags gathered through the sort
//                           permutation, a chunked block scan of tp / fp with a carried prefix, rc and pr per detection, a maximum
//                           into the bin of the last recall threshold rc reaches (LDS, 64-bit integer maximum: a non-negative double
//                           orders as its bit pattern) and a suffix maximum over the bins.  No global atomics, nothing waits on
//                           another workgroup.
#include "common.h"
#include <math.h>

namespace {

constexpr int MATCH_THREADS = 128;
constexpr int ACC_THREADS = 256;
constexpr int ACC_ITEMS = H3D_COCO_SCAN_CHUNK / ACC_THREADS;
static_assert(ACC_ITEMS * ACC_THREADS == H3D_COCO_SCAN_CHUNK, "a scan chunk is a whole number of items per thread");
static_assert(H3D_COCO_MAX_D <= MATCH_THREADS, "one thread per detection");
constexpr int MAXG = H3D_COCO_MAX_G, MAXD = H3D_COCO_MAX_D, MAXA = H3D_COCO_MAX_A, MAXL = H3D_COCO_MAX_LANES;
constexpr size_t MATCH_LDS_MATRIX_MAX = 96 * 1024;            // bytes of the D x G matrix kept in LDS (beside ~25 KiB of static LDS)

struct MatchArgs {
    const float *dets;
    const int32_t *det_cls, *det_num;
    const double *gt_boxes, *gt_kp, *gt_area;
    const uint8_t *gt_crowd;
    const int32_t *gt_cls, *gt_num;
    const double *area_rng, *iou_thrs, *kp_vars;
    double *ious, *mat;                  // the public matrix (may be NULL) | where the walk reads it when it is not in LDS
    int32_t *dt_match;
    uint8_t *dt_ignore, *gt_ignore;
    double *dt_score;
    int32_t *dt_rank;
    double *dt_box, *dt_area, *dt_kp;
    int det_stride, D, G, kp, round2, max_det, A, T, mat_lds;
};

// float("{:.2f}".format(v)) for finite |v| < 2^20
__device__ __forceinline__ double round2(double v) { return rint(v * 100.0) / 100.0; }

__device__ __forceinline__ double box_iou(const double *d, const double *g, bool crowd)
{
    const double iw = fmin(d[0] + d[2], g[0] + g[2]) - fmax(d[0], g[0]);
    const double ih = fmin(d[1] + d[3], g[1] + g[3]) - fmax(d[1], g[1]);
    if (iw <= 0.0 || ih <= 0.0) return 0.0;
    const double I = iw * ih;
    const double U = crowd ? d[2] * d[3] : d[2] * d[3] + g[2] * g[3] - I;
    return I / U;
}

__device__ __forceinline__ double oks(const double *dk, const double *gk, const double *bb, double area, int k1, const double *vars)
{
    const double den = area + 0x1p-52;
    const double x0 = bb[0] - bb[2], x1 = bb[0] + bb[2] * 2.0, y0 = bb[1] - bb[3], y1 = bb[1] + bb[3] * 2.0;
    double sum = 0.0;
    for (int j = 0; j < 17; ++j) {
        const double xd = dk[2 * j], yd = dk[2 * j + 1];
        double dx, dy;
        if (k1 > 0) {
            if (!(gk[3 * j + 2] > 0.0)) continue;
            dx = xd - gk[3 * j];
            dy = yd - gk[3 * j + 1];
        } else {
            dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1);
            dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
        }
        const double e = (dx * dx + dy * dy) / vars[j] / den / 2.0;
        sum = sum + exp(-e);
    }
    return sum / (double)(k1 > 0 ? k1 : 17);
}

__global__ __launch_bounds__(MATCH_THREADS) void coco_match_kernel(const MatchArgs a)
{
    extern __shared__ double s_mat[];
    __shared__ uint16_t s_gorder[MAXA][MAXG];      // per area range: the ground truths, not-ignored ones first (stable)
    __shared__ uint8_t s_gig[MAXA][MAXG];
    __shared__ int32_t s_gcls[MAXG];
    __shared__ uint8_t s_crowd[MAXG], s_k1[MAXG];
    __shared__ uint32_t s_matched[MAXL][MAXG / 32];
    __shared__ double s_score[MAXD], s_darea[MAXD];
    __shared__ int32_t s_dcls[MAXD], s_crank[MAXD], s_order[MAXD], s_nvalid[MAXA];

    const int n = blockIdx.x, tid = threadIdx.x;
    const int D = a.D, G = a.G, A = a.A, T = a.T;
    const int nd = a.det_num ? min(max(a.det_num[n], 0), D) : D;
    const int ng = min(max(a.gt_num[n], 0), G);
    const size_t nD = (size_t)n * D, nG = (size_t)n * G;

    // ---- the rounded records ------------------------------------------------------------------------------------------------------------
    if (tid < D) {
        const int d = tid;
        double b[4] = {0.0, 0.0, 0.0, 0.0}, sc = 0.0, ar = 0.0;
        if (d < nd) {
            const float *row = a.dets + (nD + d) * a.det_stride;
            b[0] = (double)row[0];
            b[1] = (double)row[1];
            b[2] = (double)row[2] - (double)row[0];
            b[3] = (double)row[3] - (double)row[1];
            sc = (double)row[4];
            if (a.round2) {
                for (int j = 0; j < 4; ++j) b[j] = round2(b[j]);
                sc = round2(sc);
            }
            ar = b[2] * b[3];
            if (a.kp)
                for (int j = 0; j < 34; ++j) {
                    const double v = (double)row[5 + j];
                    a.dt_kp[(nD + d) * 34 + j] = a.round2 ? round2(v) : v;
                }
        } else if (a.kp) {
            for (int j = 0; j < 34; ++j) a.dt_kp[(nD + d) * 34 + j] = 0.0;
        }
        for (int j = 0; j < 4; ++j) a.dt_box[(nD + d) * 4 + j] = b[j];
        a.dt_score[nD + d] = sc;
        a.dt_area[nD + d] = ar;
        s_score[d] = sc;
        s_darea[d] = ar;
        s_dcls[d] = (d < nd && a.det_cls) ? a.det_cls[nD + d] : 0;
    }
    // ---- the ground truths: class, crowd, labelled joints, ignore per area range -------------------------------------------------------------
    for (int g = tid; g < G; g += MATCH_THREADS) {
        bool crowd = false;
        int k1 = 0;
        double area = 0.0;
        if (g < ng) {
            crowd = a.gt_crowd[nG + g] != 0;
            area = a.gt_area[nG + g];
            s_gcls[g] = a.gt_cls[nG + g];
            if (a.kp)
                for (int j = 0; j < 17; ++j) k1 += a.gt_kp[(nG + g) * 51 + 3 * j + 2] > 0.0;
            s_crowd[g] = crowd;
            s_k1[g] = (uint8_t)k1;
        }
        const bool base = crowd || (a.kp && k1 == 0);
        for (int r = 0; r < A; ++r) {
            const bool ig = g < ng && (base || area < a.area_rng[2 * r] || area > a.area_rng[2 * r + 1]);
            a.gt_ignore[((size_t)n * A + r) * G + g] = ig;
            if (g < ng) s_gig[r][g] = ig;
        }
    }
    for (int i = tid; i < MAXL * (MAXG / 32); i += MATCH_THREADS) (&s_matched[0][0])[i] = 0u;
    __syncthreads();

    // ---- stable ranks: over the image (the walk's order) and inside the detection's class (the maxDet cut) -----------------------------------
    if (tid < D) {
        const int d = tid;
        int crank = -1;
        if (d < nd) {
            const double s = s_score[d];
            const int c = s_dcls[d];
            int grank = 0;
            crank = 0;
            for (int o = 0; o < nd; ++o) {
                const bool before = s_score[o] > s || (s_score[o] == s && o < d);
                grank += before;
                crank += before && s_dcls[o] == c;
            }
            s_order[grank] = d;
            s_crank[d] = crank;
        }
        a.dt_rank[nD + d] = crank;
    }
    if (tid < A) {
        int p = 0;
        for (int g = 0; g < ng; ++g)
            if (!s_gig[tid][g]) s_gorder[tid][p++] = (uint16_t)g;
        s_nvalid[tid] = p;
        for (int g = 0; g < ng; ++g)
            if (s_gig[tid][g]) s_gorder[tid][p++] = (uint16_t)g;
    }

    // ---- the matrix (the records of this image were written by this workgroup: visible after the barrier above) ---------------------------
    double *gmat = a.mat ? a.mat + nD * G : nullptr;
    double *pub = a.ious ? a.ious + nD * G : nullptr;
    for (int e = tid; e < D * G; e += MATCH_THREADS) {
        const int d = e / G, g = e - d * G;
        double v = 0.0;
        if (d < nd && g < ng) {
            if (a.kp)
                v = oks(a.dt_kp + (nD + d) * 34, a.gt_kp + (nG + g) * 51, a.gt_boxes + (nG + g) * 4, a.gt_area[nG + g], s_k1[g], a.kp_vars);
            else
                v = box_iou(a.dt_box + (nD + d) * 4, a.gt_boxes + (nG + g) * 4, s_crowd[g] != 0);
        }
        if (a.mat_lds) s_mat[e] = v;
        else gmat[e] = v;
        if (pub && pub != gmat) pub[e] = v;
    }
    __syncthreads();

    // ---- the walk: one lane per (area range, threshold) ---------------------------------------------------------------------------------------
    const int lane = tid;
    if (lane < A * T) {
        const int r = lane / T, t = lane - r * T;
        const double thr = fmin(a.iou_thrs[t], 1.0 - 1e-10);
        const double lo = a.area_rng[2 * r], hi = a.area_rng[2 * r + 1];
        const int nvalid = s_nvalid[r];
        const double *M = a.mat_lds ? s_mat : gmat;
        uint32_t *matched = s_matched[lane];
        const size_t out = (((size_t)n * A + r) * T + t) * D;
        for (int k = 0; k < nd; ++k) {
            const int d = s_order[k];
            int m = -1;
            bool ig = false;
            if (s_crank[d] < a.max_det) {
                const int c = s_dcls[d];
                double best = thr;
                bool mig = false;
                for (int p = 0; p < ng; ++p) {
                    const int g = s_gorder[r][p];
                    if (s_gcls[g] != c) continue;
                    const bool gig = p >= nvalid;
                    if ((matched[g >> 5] >> (g & 31) & 1u) && !s_crowd[g]) continue;
                    if (m >= 0 && !mig && gig) break;
                    const double v = M[d * G + g];
                    if (v < best) continue;
                    best = v;
                    m = g;
                    mig = gig;
                }
                if (m >= 0) {
                    ig = mig;
                    matched[m >> 5] |= 1u << (m & 31);
                } else {
                    ig = s_darea[d] < lo || s_darea[d] > hi;
                }
            }
            a.dt_match[out + d] = m;
            a.dt_ignore[out + d] = ig;
        }
    }
    // the padding rows
    for (int e = tid; e < A * T * (D - nd); e += MATCH_THREADS) {
        const int l = e / (D - nd), d = nd + (e - l * (D - nd));
        a.dt_match[((size_t)n * A * T + l) * D + d] = -1;
        a.dt_ignore[((size_t)n * A * T + l) * D + d] = 0;
    }
}

// ---- accumulate ------------------------------------------------------------------------------------------------------------------------------
struct AccArgs {
    const int64_t *order;
    const int32_t *seg_start, *dt_rank, *dt_match;
    const uint8_t *dt_ignore, *gt_ignore;
    const int32_t *gt_cls, *gt_num;
    const double *rec_thrs;
    int32_t *npig;
    double *precision, *recall;
    int N, D, G, K, A, T, M, R;
    int max_dets[H3D_COCO_MAX_M];
};

__global__ __launch_bounds__(ACC_THREADS) void coco_npig_kernel(const AccArgs a)
{
    __shared__ int s_count;
    const int k = blockIdx.x / a.A, r = blockIdx.x - k * a.A;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    int c = 0;
    const size_t total = (size_t)a.N * a.G;
    for (size_t i = threadIdx.x; i < total; i += ACC_THREADS) {
        const size_t n = i / a.G;
        const int g = (int)(i - n * a.G);
        if (g < a.gt_num[n] && a.gt_cls[i] == k && !a.gt_ignore[(n * a.A + r) * a.G + g]) ++c;
    }
    if (c) atomicAdd(&s_count, c);
    __syncthreads();
    if (threadIdx.x == 0) a.npig[blockIdx.x] = s_count;
}

__global__ __launch_bounds__(ACC_THREADS) void coco_accumulate_kernel(const AccArgs a)
{
    __shared__ unsigned long long s_bins[H3D_COCO_MAX_R];
    __shared__ double s_rec[H3D_COCO_MAX_R];
    __shared__ int s_wave[2][ACC_THREADS / 64][2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int A = a.A, T = a.T, M = a.M, R = a.R, K = a.K, D = a.D;
    int row = blockIdx.x;
    const int t = row % T;
    row /= T;
    const int mi = row % M;
    row /= M;
    const int r = row % A, k = row / A;
    const int maxdet = a.max_dets[mi];
    const int npig = a.npig[k * A + r];
    double *prec = a.precision + (((size_t)t * R * K + k) * A + r) * M + mi;       // element q: prec[q * K * A * M]
    const size_t pstride = (size_t)K * A * M;
    double *rec = a.recall + (((size_t)t * K + k) * A + r) * M + mi;
    if (npig == 0) {
        for (int q = tid; q < R; q += ACC_THREADS) prec[q * pstride] = -1.0;
        if (tid == 0) *rec = -1.0;
        return;
    }
    for (int q = tid; q < R; q += ACC_THREADS) {
        s_bins[q] = 0ull;
        s_rec[q] = a.rec_thrs[q];
    }
    __syncthreads();
    const double dn = (double)npig;
    const int begin = a.seg_start[k], end = a.seg_start[k + 1];
    int carry_tp = 0, carry_fp = 0, buf = 0;
    for (int base = begin; base < end; base += H3D_COCO_SCAN_CHUNK, buf ^= 1) {
        bool inc[ACC_ITEMS];
        int tp[ACC_ITEMS], fp[ACC_ITEMS];
        int stp = 0, sfp = 0;
#pragma unroll
        for (int j = 0; j < ACC_ITEMS; ++j) {
            const int i = base + tid * ACC_ITEMS + j;
            inc[j] = false;
            tp[j] = fp[j] = 0;
            if (i < end) {
                const int64_t e = a.order[i];
                const int rank = a.dt_rank[e];
                if (rank >= 0 && rank < maxdet) {
                    const int64_t n = e / D;
                    const size_t at = ((((size_t)n * A + r) * T + t) * D) + (size_t)(e - n * D);
                    const bool ig = a.dt_ignore[at] != 0, mt = a.dt_match[at] >= 0;
                    inc[j] = true;
                    tp[j] = mt && !ig;
                    fp[j] = !mt && !ig;
                }
            }
            stp += tp[j];
            sfp += fp[j];
        }
        // inclusive scan of the per-thread sums inside the wave, then the waves' totals through LDS
        int itp = stp, ifp = sfp;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int utp = __shfl_up(itp, off), ufp = __shfl_up(ifp, off);
            if (lane >= off) {
                itp += utp;
                ifp += ufp;
            }
        }
        if (lane == 63) {
            s_wave[buf][wave][0] = itp;
            s_wave[buf][wave][1] = ifp;
        }
        __syncthreads();
        int rtp = carry_tp + itp - stp, rfp = carry_fp + ifp - sfp;
#pragma unroll
        for (int w = 0; w < ACC_THREADS / 64; ++w) {
            if (w < wave) {
                rtp += s_wave[buf][w][0];
                rfp += s_wave[buf][w][1];
            }
            carry_tp += s_wave[buf][w][0];
            carry_fp += s_wave[buf][w][1];
        }
#pragma unroll
        for (int j = 0; j < ACC_ITEMS; ++j) {
            rtp += tp[j];
            rfp += fp[j];
            if (inc[j]) {
                const double dtp = (double)rtp, dfp = (double)rfp;
                const double rc = dtp / dn;
                const double pr = dtp / (dfp + dtp + 0x1p-52);
                // the last threshold rc reaches: s_rec[0] = 0 <= rc always holds for COCO's recThrs; a first threshold above rc has no bin
                int lo = -1, hi = R;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_rec[mid] <= rc) lo = mid;
                    else hi = mid;
                }
                if (lo >= 0) atomicMax(&s_bins[lo], (unsigned long long)__double_as_longlong(pr));
            }
        }
        // (s_wave is double-buffered: the next chunk's totals go to the other half, and the barrier of that chunk orders this chunk's reads
        // before the chunk after it writes this half again)
    }
    __syncthreads();
    for (int q = tid; q < R; q += ACC_THREADS) {
        unsigned long long best = 0ull;
        for (int u = q; u < R; ++u) best = s_bins[u] > best ? s_bins[u] : best;
        prec[q * pstride] = __longlong_as_double((long long)best);
    }
    if (tid == 0) *rec = (double)carry_tp / dn;
}

int coco_match_layout(int N, int D, int G, size_t *matrix_bytes, bool *in_lds)
{
    const size_t per = (size_t)D * G * sizeof(double);
    *in_lds = per <= MATCH_LDS_MATRIX_MAX;
    *matrix_bytes = *in_lds ? 0 : h3d_align256(per * (size_t)N);
    return H3D_OK;
}

int coco_check_sizes(const char *who, int N, int D, int G, int A, int T)
{
    if (N < 0 || D < 0 || G < 0 || A <= 0 || T <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: N = %d, D = %d, G = %d, A = %d, T = %d", who, N, D, G, A, T);
    if (D > H3D_COCO_MAX_D) H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: D = %d detections per image, at most %d are ranked", who, D, H3D_COCO_MAX_D);
    if (G > H3D_COCO_MAX_G) H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: G = %d ground truths per image, at most %d are matched", who, G, H3D_COCO_MAX_G);
    if (A > H3D_COCO_MAX_A || A * T > H3D_COCO_MAX_LANES)
        H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: A = %d area ranges (at most %d) x T = %d thresholds, at most %d walks", who, A, H3D_COCO_MAX_A, T, H3D_COCO_MAX_LANES);
    if ((double)N * A * T * (D > 0 ? D : 1) >= 2147483648.0 || (double)N * (G > 0 ? G : 1) * A >= 2147483648.0)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: N A T D = %d * %d * %d * %d and N A G = %d * %d * %d flags must stay below 2^31", who, N, A, T, D, N, A, G);
    return H3D_OK;
}

}  // namespace

extern "C" int h3d_coco_match_workspace_bytes(int N, int D, int G, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "coco_match_workspace_bytes: null pointer");
    H3D_TRY(coco_check_sizes("coco_match_workspace_bytes", N, D, G, 1, 1));
    bool in_lds;
    return coco_match_layout(N, D, G, bytes, &in_lds);
}

extern "C" int h3d_coco_match(const float *dets, int det_stride, const int32_t *det_cls, const int32_t *det_num, const double *gt_boxes,
                              const double *gt_keypoints, const double *gt_area, const uint8_t *gt_iscrowd, const int32_t *gt_cls,
                              const int32_t *gt_num, int N, int D, int G, int iou_type, int flags, int max_det, const double *area_rng, int A,
                              const double *iou_thrs, int T, const double *kp_vars, double *ious, int32_t *dt_match, uint8_t *dt_ignore,
                              uint8_t *gt_ignore, double *dt_score, int32_t *dt_rank, double *dt_box, double *dt_area, double *dt_keypoints,
                              void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "coco_match";
    H3D_TRY(coco_check_sizes(who, N, D, G, A, T));
    if (iou_type != H3D_COCO_BBOX && iou_type != H3D_COCO_KEYPOINTS) H3D_FAIL(H3D_ERR_ARG, "%s: iou_type = %d", who, iou_type);
    if (flags & ~H3D_COCO_ROUND2) H3D_FAIL(H3D_ERR_ARG, "%s: unknown flag bits %#x", who, flags);
    const bool kp = iou_type == H3D_COCO_KEYPOINTS;
    if (det_stride < (kp ? 39 : 5)) H3D_FAIL(H3D_ERR_SHAPE, "%s: det_stride = %d, a row holds at least %d floats", who, det_stride, kp ? 39 : 5);
    if (max_det < 1) H3D_FAIL(H3D_ERR_SHAPE, "%s: max_det = %d", who, max_det);
    if (N == 0) return H3D_OK;
    if (!area_rng || !iou_thrs || !gt_num) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    // (an operand without elements may be NULL)
    if (D > 0 && (!dets || !dt_match || !dt_ignore || !dt_score || !dt_rank || !dt_box || !dt_area)) H3D_FAIL(H3D_ERR_ARG, "%s: null detection operand", who);
    if (G > 0 && (!gt_boxes || !gt_area || !gt_iscrowd || !gt_cls || !gt_ignore)) H3D_FAIL(H3D_ERR_ARG, "%s: null ground-truth operand", who);
    if (kp && (!kp_vars || (D > 0 && !dt_keypoints) || (G > 0 && !gt_keypoints))) H3D_FAIL(H3D_ERR_ARG, "%s: null keypoint operand", who);
    size_t need;
    bool in_lds;
    coco_match_layout(N, D, G, &need, &in_lds);
    if (!in_lds && !ious && (!workspace || workspace_bytes < need))
        H3D_FAIL(H3D_ERR_ARG, "%s: workspace of %zu bytes needed for the matrix (got %zu)", who, need, workspace_bytes);
    if (((uintptr_t)workspace | (uintptr_t)ious | (uintptr_t)dt_score | (uintptr_t)dt_box | (uintptr_t)dt_area | (uintptr_t)dt_keypoints |
         (uintptr_t)gt_boxes | (uintptr_t)gt_keypoints | (uintptr_t)gt_area | (uintptr_t)area_rng | (uintptr_t)iou_thrs | (uintptr_t)kp_vars) & 7)
        H3D_FAIL(H3D_ERR_ARG, "%s: misaligned pointer (fp64 needs 8 bytes)", who);
    MatchArgs a;
    a.dets = dets, a.det_cls = det_cls, a.det_num = det_num;
    a.gt_boxes = gt_boxes, a.gt_kp = gt_keypoints, a.gt_area = gt_area, a.gt_crowd = gt_iscrowd, a.gt_cls = gt_cls, a.gt_num = gt_num;
    a.area_rng = area_rng, a.iou_thrs = iou_thrs, a.kp_vars = kp_vars;
    a.ious = ious, a.mat = in_lds ? nullptr : (ious ? ious : (double *)workspace);
    a.dt_match = dt_match, a.dt_ignore = dt_ignore, a.gt_ignore = gt_ignore, a.dt_score = dt_score, a.dt_rank = dt_rank;
    a.dt_box = dt_box, a.dt_area = dt_area, a.dt_kp = dt_keypoints;
    a.det_stride = det_stride, a.D = D, a.G = G, a.kp = kp, a.round2 = (flags & H3D_COCO_ROUND2) != 0, a.max_det = max_det, a.A = A, a.T = T;
    a.mat_lds = in_lds;
    const size_t lds = in_lds ? (size_t)D * G * sizeof(double) : 0;
    const h3d_kname name{"coco_match_kernel"};
    if (name.dry()) return H3D_OK;
    if (lds > 16 * 1024) {               // (the default limit covers static + dynamic LDS)
        static size_t raised = 0;        // the attribute holds the largest size asked for so far
        if (lds > raised) {
            if (hipFuncSetAttribute((const void *)coco_match_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MATCH_LDS_MATRIX_MAX) != hipSuccess)
                H3D_FAIL(H3D_ERR_LAUNCH, "%s: cannot raise the dynamic LDS limit to %zu bytes", who, MATCH_LDS_MATRIX_MAX);
            raised = MATCH_LDS_MATRIX_MAX;
        }
    }
    return h3d_bind(name, coco_match_kernel).launch(dim3((unsigned)N), dim3(MATCH_THREADS), lds, (hipStream_t)stream, a);
}

extern "C" int h3d_coco_accumulate_workspace_bytes(int K, int A, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "coco_accumulate_workspace_bytes: null pointer");
    if (K <= 0 || A <= 0 || (double)K * A >= 2147483648.0 / 4) H3D_FAIL(H3D_ERR_SHAPE, "coco_accumulate_workspace_bytes: K = %d, A = %d", K, A);
    *bytes = h3d_align256((size_t)K * A * sizeof(int32_t));
    return H3D_OK;
}

extern "C" int h3d_coco_accumulate(const int64_t *order, const int32_t *seg_start, const int32_t *dt_rank, const int32_t *dt_match,
                                   const uint8_t *dt_ignore, const uint8_t *gt_ignore, const int32_t *gt_cls, const int32_t *gt_num, int N, int D,
                                   int G, int K, int A, int T, const int32_t *max_dets, int M, const double *rec_thrs, int R, double *precision,
                                   double *recall, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "coco_accumulate";
    H3D_TRY(coco_check_sizes(who, N, D, G, A, T));
    if (K <= 0 || M <= 0 || R <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: K = %d, M = %d, R = %d", who, K, M, R);
    if (M > H3D_COCO_MAX_M || R > H3D_COCO_MAX_R)
        H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: M = %d maxDets (at most %d), R = %d recall thresholds (at most %d)", who, M, H3D_COCO_MAX_M, R, H3D_COCO_MAX_R);
    if ((double)K * A * M * T >= 2147483648.0 || (double)K * A * M * T * R >= 2147483648.0)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: K A M T R = %d * %d * %d * %d * %d cells, they must stay below 2^31", who, K, A, M, T, R);
    if (!max_dets || !rec_thrs || !precision || !recall || !seg_start || !gt_num) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if (N * D > 0 && (!order || !dt_rank || !dt_match || !dt_ignore)) H3D_FAIL(H3D_ERR_ARG, "%s: null detection operand", who);
    if (N * G > 0 && (!gt_ignore || !gt_cls)) H3D_FAIL(H3D_ERR_ARG, "%s: null ground-truth operand", who);
    size_t need;
    H3D_TRY(h3d_coco_accumulate_workspace_bytes(K, A, &need));
    if (!workspace || workspace_bytes < need) H3D_FAIL(H3D_ERR_ARG, "%s: workspace of %zu bytes needed (got %zu)", who, need, workspace_bytes);
    if (((uintptr_t)workspace & 3) || (((uintptr_t)precision | (uintptr_t)recall | (uintptr_t)rec_thrs | (uintptr_t)order) & 7))
        H3D_FAIL(H3D_ERR_ARG, "%s: misaligned pointer", who);
    AccArgs a;
    a.order = order, a.seg_start = seg_start, a.dt_rank = dt_rank, a.dt_match = dt_match, a.dt_ignore = dt_ignore, a.gt_ignore = gt_ignore;
    a.gt_cls = gt_cls, a.gt_num = gt_num, a.rec_thrs = rec_thrs, a.npig = (int32_t *)workspace, a.precision = precision, a.recall = recall;
    a.N = N, a.D = D, a.G = G, a.K = K, a.A = A, a.T = T, a.M = M, a.R = R;
    for (int i = 0; i < H3D_COCO_MAX_M; ++i) a.max_dets[i] = i < M ? max_dets[i] : 0;
    hipStream_t st = (hipStream_t)stream;
    H3D_TRY(h3d_launch({"coco_npig_kernel"}, coco_npig_kernel, dim3((unsigned)(K * A)), dim3(ACC_THREADS), 0, st, a));
    return h3d_launch({"coco_accumulate_kernel"}, coco_accumulate_kernel, dim3((unsigned)(K * A * M * T)), dim3(ACC_THREADS), 0, st, a);
}
