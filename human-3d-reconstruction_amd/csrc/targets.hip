// Training targets of the multi_pose / ctdet tasks (include/h3d.h section 6): the label half of the reference's dataset items,
// COCOHP._get_label (datasets/coco_hp.py:215-309) and the ctdet block of COCO.__getitem__ (datasets/coco.py:203-248), for a batch.
//
// Two launches, no memset, no atomics, every output element stored exactly once:
//   targets_objects_kernel<POSE>  one wave per (image, object slot), lanes over the joints.  The box path, the radius and every row are
//                                 computed with the reference's types at every step (this file is built with -ffp-contract=off): float32
//                                 where numpy holds float32, float64 for the 2x3 matrix product and gaussian_radius.  The wave also leaves
//                                 one splat slot {x, y, r, cls} per map channel it may draw on (r < 0: nothing) in the workspace, and finds
//                                 its row of the compact gt_det by counting the live objects of its image in front of it (the box path of
//                                 every object of the image again, one lane each: a few dozen flops against a launch of its own).
//   targets_render_kernel         one workgroup per 1024 consecutive pixels of one (image, channel) map.  Wave 0 compacts the channel's
//                                 slots that reach the workgroup's rows into LDS (ballot order = object order); every thread then takes the
//                                 maximum over the splats covering its 4 pixels, exp in float64 rounded to float32, and stores them
//                                 once.  A heat map is a pure maximum over its splats (np.maximum in draw_umich_gaussian), so the gather
//                                 gives what the reference's scatter gives, whatever the object order.
#include "common.h"

#include <math.h>

namespace {

constexpr int TGT_CHUNK = 1024;          // pixels per render workgroup: 256 threads x 4

struct TgtBox { float b0, b1, b2, b3, h, w; };

// affine_transform (utils/image.py:65-68): float64 2x3 times float32 [x, y, 1], one rounding to float32 at the store into bbox / pts
__device__ __forceinline__ float tgt_affine(const double *t, float x, float y)
{
    return (float)(t[0] * (double)x + t[1] * (double)y + t[2]);
}

__device__ __forceinline__ float tgt_clip(float v, float hi) { return fminf(fmaxf(v, 0.0f), hi); }

// xywh -> xyxy, the mirror, trans_output on both corners, the clip, h and w (coco_hp.py:249-261, coco.py:220-228)
__device__ __forceinline__ TgtBox tgt_box(const float *box, const double *t, bool flip, float width, float xmax, float ymax)
{
    float x0 = box[0], y0 = box[1], x1 = box[0] + box[2], y1 = box[1] + box[3];
    if (flip) {
        const float m0 = (width - x1) - 1.0f, m1 = (width - x0) - 1.0f;
        x0 = m0;
        x1 = m1;
    }
    TgtBox r;
    r.b0 = tgt_clip(tgt_affine(t, x0, y0), xmax);
    r.b1 = tgt_clip(tgt_affine(t + 3, x0, y0), ymax);
    r.b2 = tgt_clip(tgt_affine(t, x1, y1), xmax);
    r.b3 = tgt_clip(tgt_affine(t + 3, x1, y1), ymax);
    r.h = r.b3 - r.b1;
    r.w = r.b2 - r.b0;
    return r;
}

// max(0, int(gaussian_radius((ceil(h), ceil(w))))), utils/image.py:97-117 in float64 and in its operation order
__device__ __forceinline__ int tgt_radius(float hf, float wf)
{
    const double mo = 0.7;
    const double height = ceil((double)hf), width = ceil((double)wf);
    const double b1 = height + width;
    const double c1 = width * height * (1 - mo) / (1 + mo);
    const double sq1 = sqrt(b1 * b1 - 4 * c1);
    const double r1 = (b1 + sq1) / 2;
    const double b2 = 2 * (height + width);
    const double c2 = (1 - mo) * width * height;
    const double sq2 = sqrt(b2 * b2 - 16 * c2);
    const double r2 = (b2 + sq2) / 2;
    const double a3 = 4 * mo;
    const double b3 = -2 * mo * (height + width);
    const double c3 = (mo - 1) * width * height;
    const double sq3 = sqrt(b3 * b3 - 4 * a3 * c3);
    const double r3 = (b3 + sq3) / 2;
    const double r = fmin(fmin(r1, r2), r3);
    return max(0, (int)r);
}

struct TgtArgs {
    const float *boxes, *kp;
    const int32_t *cls, *num;
    const double *trans;
    const int32_t *rot_flag, *flipped, *width, *flip_pairs;
    int n_pairs, B, M, J, H, W, C, max_objs;
    float *wh, *reg;
    int64_t *ind;
    uint8_t *reg_mask;
    float *kps;
    uint8_t *kps_mask;
    float *hp_offset;
    int64_t *hp_ind, *hp_mask;
    float *cat_wh;
    uint8_t *cat_mask;
    float *gt_det;
    int32_t *gt_count;
    int4 *list;            // [B][1 + J][max_objs] splat slots {x, y, r, cls}
};

// the gate: (h > 0 and w > 0) or rot != 0 (coco_hp.py:262); ctdet: h > 0 and w > 0 (coco.py:229) and a class the map has
template <bool POSE>
__device__ __forceinline__ bool tgt_live(const TgtArgs &a, const TgtBox &bx, bool rot, int b, int k)
{
    const bool pos = bx.h > 0.0f && bx.w > 0.0f;
    if (POSE) return pos || rot;
    const int c = a.cls[(size_t)b * a.M + k];
    return pos && c >= 0 && c < a.C;
}

template <bool POSE>
__global__ __launch_bounds__(256) void targets_objects_kernel(TgtArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= a.B * a.max_objs) return;                     // whole waves leave: no barrier below
    const int N = a.max_objs, J = a.J;
    const int b = wv / N, k = wv - b * N;
    const double *T = a.trans + (size_t)b * 12;
    const bool rot = POSE && a.rot_flag && a.rot_flag[b] != 0;
    const bool flip = a.flipped && a.flipped[b] != 0;
    const float width = flip ? (float)a.width[b] : 0.0f;
    const int n = max(0, min(a.num[b], min(a.M, N)));
    const float xmax = (float)(a.W - 1), ymax = (float)(a.H - 1);

    // live objects of the image in front of this one, and in all: the row of the compact gt_det
    int before = 0, total = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int kk = c0 + lane;
        bool lv = false;
        if (kk < n) lv = tgt_live<POSE>(a, tgt_box(a.boxes + ((size_t)b * a.M + kk) * 4, T, flip, width, xmax, ymax), rot, b, kk);
        const unsigned long long m = __ballot(lv);
        total += __popcll(m);
        if (k >= c0 + 64) before += __popcll(m);
        else if (k > c0) before += __popcll(m & ((1ull << (k - c0)) - 1ull));
    }

    TgtBox bx = {0, 0, 0, 0, 0, 0};
    bool live = false;
    if (k < n) {
        bx = tgt_box(a.boxes + ((size_t)b * a.M + k) * 4, T, flip, width, xmax, ymax);
        live = tgt_live<POSE>(a, bx, rot, b, k);
    }
    // live objects fill rows [0, total) in order, the others the zero rows behind them: every row has one writer
    const int row = live ? before : total + (k - before);
    const size_t slot = (size_t)b * N + k;
    int radius = -1, cxi = 0, cyi = 0, cls = 0;
    float ctx = 0.0f, cty = 0.0f;
    if (live) {
        radius = tgt_radius(bx.h, bx.w);
        ctx = (bx.b0 + bx.b2) / 2.0f;
        cty = (bx.b1 + bx.b3) / 2.0f;
        cxi = (int)ctx;
        cyi = (int)cty;
        if (!POSE) cls = a.cls[(size_t)b * a.M + k];
    }

    if (POSE) {
        // lane j holds joint j after the mirror's pair swaps (applied in order, as the reference's loop does)
        int src = lane;
        if (live && flip) {
            for (int p = 0; p < a.n_pairs; ++p) {
                const int e0 = a.flip_pairs[2 * p], e1 = a.flip_pairs[2 * p + 1];
                if (e0 < 0 || e0 >= J || e1 < 0 || e1 >= J) continue;          // wave-uniform
                const int s0 = __shfl(src, e0), s1 = __shfl(src, e1);
                if (lane == e0) src = s1;
                else if (lane == e1) src = s0;
            }
        }
        float x = 0.0f, y = 0.0f, v = 0.0f;
        if (live && lane < J) {
            const float *p = a.kp + (((size_t)b * a.M + k) * J + src) * 3;
            x = p[0], y = p[1], v = p[2];
            if (flip) x = (width - x) - 1.0f;
        }
        float vsum = 0.0f;                                   // pts[:, 2].sum() == 0: only the test against zero is used
        for (int j = 0; j < J; ++j) vsum += __shfl(v, j);
        bool inside = false;
        int pxi = 0, pyi = 0;
        if (live && lane < J && v > 0.0f) {
            const float px = tgt_affine(T + 6, x, y), py = tgt_affine(T + 9, x, y);
            x = px, y = py;                                  // gt_det keeps the transformed point, inside the map or not
            inside = px >= 0.0f && px < (float)a.W && py >= 0.0f && py < (float)a.H;
            if (inside) pxi = (int)px, pyi = (int)py;
        }
        if (lane < J) {
            const size_t sj = slot * J + lane;
            // pts - ct_int and pts - pt_int: float32 minus int32 is a float64 difference, rounded to float32 at the store
            if (a.kps) {
                a.kps[2 * sj] = inside ? (float)((double)x - (double)cxi) : 0.0f;
                a.kps[2 * sj + 1] = inside ? (float)((double)y - (double)cyi) : 0.0f;
            }
            if (a.kps_mask) a.kps_mask[2 * sj] = a.kps_mask[2 * sj + 1] = (inside && !rot) ? 1 : 0;
            if (a.hp_offset) {
                a.hp_offset[2 * sj] = inside ? (float)((double)x - (double)pxi) : 0.0f;
                a.hp_offset[2 * sj + 1] = inside ? (float)((double)y - (double)pyi) : 0.0f;
            }
            if (a.hp_ind) a.hp_ind[sj] = inside ? (int64_t)pyi * a.W + pxi : 0;
            if (a.hp_mask) a.hp_mask[sj] = inside ? 1 : 0;
            if (a.list) a.list[((size_t)b * (1 + J) + 1 + lane) * N + k] = make_int4(pxi, pyi, inside ? radius : -1, 0);
            if (a.gt_det) {
                float *g = a.gt_det + ((size_t)b * N + row) * (6 + 2 * J) + 5 + 2 * lane;
                g[0] = live ? x : 0.0f;
                g[1] = live ? y : 0.0f;
            }
        }
        if (lane == 0) {
            if (a.reg_mask) a.reg_mask[slot] = (live && !rot && vsum != 0.0f) ? 1 : 0;
            if (a.gt_det) {
                float *g = a.gt_det + ((size_t)b * N + row) * (6 + 2 * J);
                g[0] = live ? bx.b0 : 0.0f, g[1] = live ? bx.b1 : 0.0f, g[2] = live ? bx.b2 : 0.0f, g[3] = live ? bx.b3 : 0.0f;
                g[4] = live ? 1.0f : 0.0f;
                g[5 + 2 * J] = 0.0f;                         // cls_id = category_id - 1 of the person class
            }
        }
    } else {
        for (int i = lane; i < 2 * a.C; i += 64) {
            const bool hit = live && (i >> 1) == cls;
            if (a.cat_wh) a.cat_wh[slot * 2 * a.C + i] = hit ? ((i & 1) ? bx.h : bx.w) : 0.0f;
            if (a.cat_mask) a.cat_mask[slot * 2 * a.C + i] = hit ? 1 : 0;
        }
        if (lane == 0) {
            if (a.reg_mask) a.reg_mask[slot] = live ? 1 : 0;
            if (a.gt_det) {
                float *g = a.gt_det + ((size_t)b * N + row) * 6;
                const float hw = bx.w / 2.0f, hh = bx.h / 2.0f;
                g[0] = live ? ctx - hw : 0.0f, g[1] = live ? cty - hh : 0.0f, g[2] = live ? ctx + hw : 0.0f, g[3] = live ? cty + hh : 0.0f;
                g[4] = live ? 1.0f : 0.0f;
                g[5] = live ? (float)cls : 0.0f;
            }
        }
    }
    if (lane == 0) {
        if (a.wh) a.wh[2 * slot] = live ? bx.w : 0.0f, a.wh[2 * slot + 1] = live ? bx.h : 0.0f;
        if (a.reg) a.reg[2 * slot] = live ? ctx - (float)cxi : 0.0f, a.reg[2 * slot + 1] = live ? cty - (float)cyi : 0.0f;
        if (a.ind) a.ind[slot] = live ? (int64_t)cyi * a.W + cxi : 0;
        if (a.list) a.list[(size_t)b * (1 + J) * N + k] = make_int4(cxi, cyi, radius, cls);
        if (a.gt_count && k == 0) a.gt_count[b] = total;
    }
}

struct TgtRenderArgs {
    float *hm, *hm_hp;
    const int4 *list;
    const int32_t *rot_flag;
    int C, J, H, W, max_objs;
};

__global__ __launch_bounds__(256) void targets_render_kernel(TgtRenderArgs a)
{
    __shared__ int4 s_list[H3D_TARGETS_MAX_OBJS];
    __shared__ int s_count;
    const int b = blockIdx.z, c = blockIdx.y, tid = threadIdx.x;
    const bool is_hm = c < a.C;
    float *out = is_hm ? a.hm : a.hm_hp;
    if (!out) return;                                        // workgroup-uniform, as every return in front of the barrier
    const long HW = (long)a.H * a.W;
    out += (is_hm ? (size_t)b * a.C + c : (size_t)b * a.J + (c - a.C)) * (size_t)HW;
    // groups of 4 pixels that share an aligned 16 bytes: the map's first pixel sits `al` elements behind such a boundary
    const int al = (int)(((uintptr_t)out >> 2) & 3);
    const long lo = (long)blockIdx.x * TGT_CHUNK - al;
    if (lo >= HW) return;
    const bool fill = is_hm && a.rot_flag && a.rot_flag[b] != 0;      // rot != 0: hm = hm * 0 + 0.9999 (coco_hp.py:303-304)
    int count = 0;
    if (!fill) {
        const int ylo = (int)(max(lo, 0l) / a.W), yhi = (int)((min(lo + TGT_CHUNK, HW) - 1) / a.W);
        if (tid < 64) {
            const int4 *src = a.list + ((size_t)b * (1 + a.J) + (is_hm ? 0 : 1 + c - a.C)) * a.max_objs;
            int cnt = 0;
            for (int c0 = 0; c0 < a.max_objs; c0 += 64) {
                const int i = c0 + tid;
                int4 e = make_int4(0, 0, -1, 0);
                if (i < a.max_objs) e = src[i];
                const bool keep = e.z >= 0 && (!is_hm || e.w == c) && e.y + e.z >= ylo && e.y - e.z <= yhi;
                const unsigned long long m = __ballot(keep);
                if (keep) s_list[cnt + __popcll(m & ((1ull << tid) - 1ull))] = e;
                cnt += __popcll(m);
            }
            if (tid == 0) s_count = cnt;
        }
        __syncthreads();
        count = s_count;
    }
    const long p0 = lo + 4 * tid;
    float v[4];
    int px[4], py[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long idx = p0 + e;
        const bool in = idx >= 0 && idx < HW;
        py[e] = in ? (int)(idx / a.W) : -(1 << 20);         // far from every splat
        px[e] = in ? (int)(idx - (long)py[e] * a.W) : -(1 << 20);
        v[e] = fill ? 0.9999f : 0.0f;
    }
    for (int i = 0; i < count; ++i) {
        const int4 s = s_list[i];
        // gaussian2D (utils/image.py:120-126) at sigma = diameter / 6: exp(-(x x + y y) / (2 sigma sigma)) in float64
        const double sigma = (double)(2 * s.z + 1) / 6.0;
        const double den = 2.0 * sigma * sigma;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int dx = px[e] - s.x, dy = py[e] - s.y;
            if (abs(dx) <= s.z && abs(dy) <= s.z) {
                const double d2 = (double)dx * (double)dx + (double)dy * (double)dy;
                const float g = (dx | dy) == 0 ? 1.0f : (float)exp(-d2 / den);
                v[e] = fmaxf(v[e], g);
            }
        }
    }
    if (p0 >= 0 && p0 + 4 <= HW) {
        *reinterpret_cast<f32x4 *>(out + p0) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (p0 + e >= 0 && p0 + e < HW) out[p0 + e] = v[e];
    }
}

bool misaligned(const void *p, size_t a) { return p && ((uintptr_t)p & (a - 1)) != 0; }

size_t tgt_ws_bytes(int B, int max_objs, int J) { return (size_t)B * (size_t)(1 + J) * (size_t)max_objs * sizeof(int4); }

// the checks both entry points share; `maps` = a map output is requested
int tgt_check(const char *who, const void *boxes, const void *second, const void *num, const void *trans, const void *flipped,
              const void *width, int B, int M, int J, int H, int W, int C, int max_objs, int options, bool maps, const void *ws,
              size_t ws_bytes)
{
    if (options & (H3D_TARGETS_MSE_LOSS | H3D_TARGETS_DENSE_HP | H3D_TARGETS_DENSE_WH))
        H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: mse_loss / dense_hp / dense_wh targets are not built (options 0x%x)", who, options);
    if (options & ~7) H3D_FAIL(H3D_ERR_ARG, "%s: options 0x%x", who, options);
    if (B < 0 || M < 0 || J < 0 || H <= 0 || W <= 0 || C <= 0 || max_objs <= 0 || H > 16384 || W > 16384 || B > 65535 || C + J > 65535)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: B, M, J, Hout, Wout, classes, max_objs = %d, %d, %d, %d, %d, %d, %d", who, B, M, J, H, W, C, max_objs);
    if (J > H3D_TARGETS_MAX_JOINTS || max_objs > H3D_TARGETS_MAX_OBJS)
        H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: %d joints (at most %d), max_objs %d (at most %d)", who, J, H3D_TARGETS_MAX_JOINTS, max_objs,
                 H3D_TARGETS_MAX_OBJS);
    if (B == 0) return H3D_OK;
    if (!num || !trans || (M > 0 && (!boxes || !second)) || (flipped && !width)) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if (misaligned(boxes, 4) || misaligned(second, 4) || misaligned(num, 4) || misaligned(trans, 8) || misaligned(flipped, 4) || misaligned(width, 4))
        H3D_FAIL(H3D_ERR_ARG, "%s: misaligned input pointer", who);
    const size_t need = tgt_ws_bytes(B, max_objs, J);
    if (maps && (!ws || ws_bytes < need || misaligned(ws, 16)))
        H3D_FAIL(H3D_ERR_ARG, "%s: workspace of %zu bytes (16-byte aligned), %zu needed", who, ws ? ws_bytes : (size_t)0, need);
    return H3D_OK;
}

int tgt_launch(bool pose, const TgtArgs &a, const int32_t *rot_flag, float *hm, float *hm_hp, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const long waves = (long)a.B * a.max_objs;
    const dim3 grid((unsigned)((waves + 3) / 4));
    if (pose) H3D_TRY(h3d_launch({"targets_objects_kernel", true}, targets_objects_kernel<true>, grid, dim3(256), 0, st, a));
    else H3D_TRY(h3d_launch({"targets_objects_kernel", false}, targets_objects_kernel<false>, grid, dim3(256), 0, st, a));
    if (!hm && !hm_hp) return H3D_OK;
    // a map whose first pixel sits `al` elements behind a 16-byte boundary takes ceil((HW + al) / 1024) workgroups; with HW % 4 != 0 the
    // maps of a tensor differ in it
    const long HW = (long)a.H * a.W;
    int al = 3;
    if (HW % 4 == 0) al = max(hm ? (int)(((uintptr_t)hm >> 2) & 3) : 0, hm_hp ? (int)(((uintptr_t)hm_hp >> 2) & 3) : 0);
    TgtRenderArgs r = {hm, hm_hp, a.list, rot_flag, a.C, a.J, a.H, a.W, a.max_objs};
    const dim3 rgrid((unsigned)((HW + al + TGT_CHUNK - 1) / TGT_CHUNK), (unsigned)(a.C + a.J), (unsigned)a.B);
    return h3d_launch({"targets_render_kernel"}, targets_render_kernel, rgrid, dim3(256), 0, st, r);
}

}  // namespace

extern "C" int h3d_targets_workspace_bytes(int B, int max_objs, int num_joints, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "targets_workspace_bytes: null pointer");
    if (B < 0 || max_objs < 0 || num_joints < 0) H3D_FAIL(H3D_ERR_SHAPE, "targets_workspace_bytes: B, max_objs, num_joints = %d, %d, %d", B, max_objs, num_joints);
    *bytes = tgt_ws_bytes(B, max_objs, num_joints);
    return H3D_OK;
}

extern "C" int h3d_multi_pose_targets(const float *boxes, const float *keypoints, const int32_t *num, const double *trans,
                                      const int32_t *rot_flag, const int32_t *flipped, const int32_t *width, const int32_t *flip_pairs,
                                      int n_flip_pairs, int B, int M, int J, int Hout, int Wout, int max_objs, float *hm, float *hm_hp,
                                      float *wh, float *reg, int64_t *ind, uint8_t *reg_mask, float *kps, uint8_t *kps_mask,
                                      float *hp_offset, int64_t *hp_ind, int64_t *hp_mask, float *gt_det, int32_t *gt_count, int options,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "multi_pose_targets";
    const int rc = tgt_check(who, boxes, keypoints, num, trans, flipped, width, B, M, J, Hout, Wout, 1, max_objs, options, hm || hm_hp,
                             workspace, workspace_bytes);
    if (rc != H3D_OK || B == 0) return rc;
    if (n_flip_pairs < 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: n_flip_pairs = %d", who, n_flip_pairs);
    if (n_flip_pairs > 0 && !flip_pairs) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if (misaligned(rot_flag, 4) || misaligned(flip_pairs, 4) || misaligned(hm, 4) || misaligned(hm_hp, 4) || misaligned(wh, 4) || misaligned(reg, 4) ||
        misaligned(ind, 8) || misaligned(kps, 4) || misaligned(hp_offset, 4) || misaligned(hp_ind, 8) || misaligned(hp_mask, 8) ||
        misaligned(gt_det, 4) || misaligned(gt_count, 4))
        H3D_FAIL(H3D_ERR_ARG, "%s: misaligned pointer", who);
    TgtArgs a = {};
    a.boxes = boxes, a.kp = keypoints, a.num = num, a.trans = trans, a.rot_flag = rot_flag, a.flipped = flipped, a.width = width;
    a.flip_pairs = flip_pairs, a.n_pairs = n_flip_pairs;
    a.B = B, a.M = M, a.J = J, a.H = Hout, a.W = Wout, a.C = 1, a.max_objs = max_objs;
    a.wh = wh, a.reg = reg, a.ind = ind, a.reg_mask = reg_mask, a.kps = kps, a.kps_mask = kps_mask, a.hp_offset = hp_offset;
    a.hp_ind = hp_ind, a.hp_mask = hp_mask, a.gt_det = gt_det, a.gt_count = gt_count;
    a.list = (hm || hm_hp) ? (int4 *)workspace : nullptr;
    return tgt_launch(true, a, rot_flag, hm, hm_hp, stream);
}

extern "C" int h3d_ctdet_targets(const float *boxes, const int32_t *cls, const int32_t *num, const double *trans, const int32_t *flipped,
                                 const int32_t *width, int B, int M, int Hout, int Wout, int num_classes, int max_objs, float *hm,
                                 float *wh, float *reg, int64_t *ind, uint8_t *reg_mask, float *cat_spec_wh, uint8_t *cat_spec_mask,
                                 float *gt_det, int32_t *gt_count, int options, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "ctdet_targets";
    const int rc = tgt_check(who, boxes, cls, num, trans, flipped, width, B, M, 0, Hout, Wout, num_classes, max_objs, options, hm != nullptr,
                             workspace, workspace_bytes);
    if (rc != H3D_OK || B == 0) return rc;
    if (misaligned(hm, 4) || misaligned(wh, 4) || misaligned(reg, 4) || misaligned(ind, 8) || misaligned(cat_spec_wh, 4) ||
        misaligned(gt_det, 4) || misaligned(gt_count, 4))
        H3D_FAIL(H3D_ERR_ARG, "%s: misaligned pointer", who);
    TgtArgs a = {};
    a.boxes = boxes, a.cls = cls, a.num = num, a.trans = trans, a.flipped = flipped, a.width = width;
    a.B = B, a.M = M, a.J = 0, a.H = Hout, a.W = Wout, a.C = num_classes, a.max_objs = max_objs;
    a.wh = wh, a.reg = reg, a.ind = ind, a.reg_mask = reg_mask, a.cat_wh = cat_spec_wh, a.cat_mask = cat_spec_mask;
    a.gt_det = gt_det, a.gt_count = gt_count;
    a.list = hm ? (int4 *)workspace : nullptr;
    return tgt_launch(false, a, nullptr, hm, nullptr, stream);
}
