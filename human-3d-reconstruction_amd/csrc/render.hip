// Mesh rendering: a z-buffered visibility-buffer rasteriser under the weak-perspective camera of the keypoint loss (include/h3d.h section
// 4d; no reference code: the project's own definition).
//
//   render_raster_kernel    one workgroup of 1024 threads per person slot p = b n + m; a skipped slot returns at once.  The workgroup projects
//                           the slot's V vertices once into LDS ({xi, yi, d}: 12 bytes each, 83 KB for SMPL -> one workgroup per CU), then
//                           walks the shared index array in coalesced order, one face per thread and round.  A face whose clipped bounding
//                           box holds at most RN_SMALL_MAX pixels is walked by its own lane (on a body of a few hundred pixels nearly every
//                           one of the 13 776 faces); a larger one is pushed on a queue in LDS, and whole waves take queued faces with their
//                           lanes spread over the bounding box.  The queue has room for one entry per thread beyond its drain level, so it is
//                           drained between rounds before it can fill and no face is ever dropped.  Coverage is exact integer arithmetic
//                           (three edge functions in int64, top-left rule), the depth a fixed sequence of fp32 operations, visibility one
//                           unsigned 64-bit atomic minimum per covered pixel on {ordered depth bits, m F + f}: no float atomics, the result
//                           does not depend on the arrival order.
//   render_resolve_kernel   one lane per pixel.  <true, false>: decodes the key into face_id and depth; <false, true>: fetches the winning
//                           face's three vertices and writes the shaded overlay.  Every output byte is stored.
// Compiled with -ffp-contract=off: the definition is a sequence of separately rounded fp32 operations in a stated order.
#include "common.h"

#include <limits.h>
#include <math.h>

constexpr int RN_THREADS = 1024;
constexpr int RN_WAVES = RN_THREADS / 64;
constexpr int RN_SMALL_MAX = 16;                    // pixels of a clipped bounding box up to which a lane walks the face itself
constexpr int RN_QCAP = 1536;                       // queue entries: drained once more than RN_QCAP - RN_THREADS wait in it
constexpr int RN_BAD = INT_MIN;                     // xi of a vertex no face may use
constexpr int RS_THREADS = 256;
constexpr size_t RN_LDS_TOTAL = 160 * 1024, RN_LDS_STATIC = 256;
static_assert(12 * (size_t)H3D_RENDER_MAX_V + 4 * (size_t)RN_QCAP + RN_LDS_STATIC <= RN_LDS_TOTAL, "H3D_RENDER_MAX_V does not fit the LDS");
static_assert(12 * (size_t)(H3D_RENDER_MAX_V + 64) + 4 * (size_t)RN_QCAP + RN_LDS_STATIC > RN_LDS_TOTAL, "H3D_RENDER_MAX_V is not the largest");
static_assert(H3D_RENDER_MAX_V >= 6890 && H3D_RENDER_MAX_V % 64 == 0, "H3D_RENDER_MAX_V");
typedef unsigned long long rn_key;

struct RasterArgs {
    const float *verts, *cam, *dz;
    const int32_t *faces;
    const int64_t *ind;
    const uint8_t *valid;
    rn_key *keys;
    int max_objs, n, V, Vs, F, H, W, up, Hr, Wr, flags;
};

// a face ready to be walked: oriented to positive area, with its clipped bounding box and the top-left biases of its edges
struct RnTri {
    int x0, y0, x1, y1, x2, y2;
    float d0, e1, e2, area;    // d0, d1 - d0, d2 - d0
    int bx0, by0, bx1, by1;
    int b0, b1, b2;            // 0 for a top or left edge (w == 0 is inside), 1 otherwise
};

__device__ __forceinline__ int rn_bias(int dx, int dy) { return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1; }

// false: the face is skipped (an index outside [0,V), a bad vertex, no area, culled, nothing of its bounding box on the target)
__device__ __forceinline__ bool rn_setup(const RasterArgs &a, const int *sx, const int *sy, const float *sd, int f, RnTri &t)
{
    const int32_t *fp = a.faces + 3LL * f;
    const int i0 = fp[0], i1 = fp[1], i2 = fp[2];
    if ((unsigned)i0 >= (unsigned)a.V || (unsigned)i1 >= (unsigned)a.V || (unsigned)i2 >= (unsigned)a.V) return false;
    t.x0 = sx[i0]; t.x1 = sx[i1]; t.x2 = sx[i2];
    if (t.x0 == RN_BAD || t.x1 == RN_BAD || t.x2 == RN_BAD) return false;
    t.y0 = sy[i0]; t.y1 = sy[i1]; t.y2 = sy[i2];
    t.d0 = sd[i0];
    float d1 = sd[i1], d2 = sd[i2];
    long long o = (long long)(t.x1 - t.x0) * (t.y2 - t.y0) - (long long)(t.y1 - t.y0) * (t.x2 - t.x0);
    if (o == 0) return false;
    const bool negz = (a.flags & H3D_RENDER_NEGATE_Z) != 0;
    if ((a.flags & H3D_RENDER_CULL_BACK) && ((o > 0) != negz)) return false;        // S = negz ? o : -o is negative
    if (o < 0) {
        int ti = t.x1; t.x1 = t.x2; t.x2 = ti;
        ti = t.y1; t.y1 = t.y2; t.y2 = ti;
        const float tf = d1; d1 = d2; d2 = tf;
        o = -o;
    }
    t.e1 = d1 - t.d0;
    t.e2 = d2 - t.d0;
    t.area = (float)o;
    const int minx = min(t.x0, min(t.x1, t.x2)), maxx = max(t.x0, max(t.x1, t.x2));
    const int miny = min(t.y0, min(t.y1, t.y2)), maxy = max(t.y0, max(t.y1, t.y2));
    t.bx0 = max(0, (minx + 15) >> 4);
    t.bx1 = min(a.Wr - 1, maxx >> 4);
    t.by0 = max(0, (miny + 15) >> 4);
    t.by1 = min(a.Hr - 1, maxy >> 4);
    if (t.bx0 > t.bx1 || t.by0 > t.by1) return false;
    t.b0 = rn_bias(t.x2 - t.x1, t.y2 - t.y1);
    t.b1 = rn_bias(t.x0 - t.x2, t.y0 - t.y2);
    t.b2 = rn_bias(t.x1 - t.x0, t.y1 - t.y0);
    return true;
}

// pixel (ix, iy) of the target, inside the face's clipped bounding box (so inside the target)
__device__ __forceinline__ void rn_pixel(const RnTri &t, int ix, int iy, rn_key *keys, int Wr, unsigned id)
{
    const int px = ix << 4, py = iy << 4;
    const long long w0 = (long long)(t.x2 - t.x1) * (py - t.y1) - (long long)(t.y2 - t.y1) * (px - t.x1);
    const long long w1 = (long long)(t.x0 - t.x2) * (py - t.y2) - (long long)(t.y0 - t.y2) * (px - t.x2);
    const long long w2 = (long long)(t.x1 - t.x0) * (py - t.y0) - (long long)(t.y1 - t.y0) * (px - t.x0);
    if (((w0 - t.b0) | (w1 - t.b1) | (w2 - t.b2)) < 0) return;
    const float p1 = (float)w1 * t.e1, p2 = (float)w2 * t.e2;
    const float depth = t.d0 + (p1 + p2) / t.area;
    if (depth != depth) return;
    const uint32_t u = __float_as_uint(depth);
    const uint32_t hi = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    atomicMin(keys + (long long)iy * Wr + ix, ((rn_key)hi << 32) | id);
}

// whole waves take the queued faces, lanes spread over the bounding box
__device__ __forceinline__ void rn_drain(const RasterArgs &a, const int *sx, const int *sy, const float *sd, const int *q, int nq, rn_key *keys,
                                         unsigned id0)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = wave; e < nq; e += RN_WAVES) {
        const int f = q[e];
        RnTri t;
        if (!rn_setup(a, sx, sy, sd, f, t)) continue;       // (it passed when it was queued)
        const int bw = t.bx1 - t.bx0 + 1, cnt = bw * (t.by1 - t.by0 + 1);
        for (int k = lane; k < cnt; k += 64) {
            const int r = k / bw;
            rn_pixel(t, t.bx0 + (k - r * bw), t.by0 + r, keys, a.Wr, id0 + (unsigned)f);
        }
    }
}

__global__ __launch_bounds__(RN_THREADS) void render_raster_kernel(const RasterArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];      // xi [Vs] | yi [Vs] | d [Vs] | queue [RN_QCAP]
    __shared__ int s_qn;
    const int tid = threadIdx.x;
    const int p = blockIdx.x, b = p / a.n, m = p - b * a.n;
    // the skips: all of them uniform over the workgroup, in front of the first barrier
    if (a.valid && a.valid[p] == 0) return;
    const int64_t ind = a.ind[(long long)b * a.max_objs + m];
    const int HW = a.H * a.W;
    if (ind < 0 || ind >= HW) return;
    const float *cam = a.cam + (long long)b * 3 * HW + ind;
    const float s = cam[0];
    if (!(s > 0.0f) || !(s < INFINITY)) return;
    const float tx = cam[HW], ty = cam[2 * (long long)HW];
    const float cx = (float)(int)(ind % a.W), cy = (float)(int)(ind / a.W), upf = (float)a.up;
    const float dzp = a.dz ? a.dz[p] : 0.0f;
    const bool negz = (a.flags & H3D_RENDER_NEGATE_Z) != 0;
    int *sx = s_dyn, *sy = s_dyn + a.Vs, *q = s_dyn + 3 * a.Vs;
    float *sd = reinterpret_cast<float *>(s_dyn + 2 * a.Vs);
    if (tid == 0) s_qn = 0;
    const float *vp = a.verts + (long long)p * a.V * 3;
    for (int i = tid; i < a.V; i += RN_THREADS) {
        const float X = vp[3 * i], Y = vp[3 * i + 1], Z = vp[3 * i + 2];
        const float xs = upf * ((s * X + tx) + cx), ys = upf * ((s * Y + ty) + cy);
        const float fx = rintf(16.0f * xs), fy = rintf(16.0f * ys);
        const float d = (negz ? -Z : Z) + dzp;
        const bool ok = fabsf(fx) <= 524288.0f && fabsf(fy) <= 524288.0f && fabsf(d) < INFINITY;      // false with any NaN
        sx[i] = ok ? (int)fx : RN_BAD;
        sy[i] = ok ? (int)fy : 0;
        sd[i] = d;
    }
    __syncthreads();
    rn_key *keys = a.keys + (long long)b * a.Hr * a.Wr;
    const unsigned id0 = (unsigned)m * (unsigned)a.F;
    for (int f0 = 0; f0 < a.F; f0 += RN_THREADS) {
        // every thread may push one face in this round: make room first.  The last push is behind a barrier, and nobody pushes
        // again before everybody has read the count
        const int nq = s_qn;
        __syncthreads();
        if (nq > RN_QCAP - RN_THREADS) {
            rn_drain(a, sx, sy, sd, q, nq, keys, id0);
            __syncthreads();
            if (tid == 0) s_qn = 0;
            __syncthreads();
        }
        const int f = f0 + tid;
        RnTri t;
        if (f < a.F && rn_setup(a, sx, sy, sd, f, t)) {
            const int bw = t.bx1 - t.bx0 + 1, bh = t.by1 - t.by0 + 1;
            if (bw * bh <= RN_SMALL_MAX) {          // (bw, bh <= 16384: no overflow)
                for (int iy = t.by0; iy <= t.by1; ++iy)
                    for (int ix = t.bx0; ix <= t.bx1; ++ix) rn_pixel(t, ix, iy, keys, a.Wr, id0 + (unsigned)f);
            } else {
                q[atomicAdd(&s_qn, 1)] = f;
            }
        }
        __syncthreads();
    }
    rn_drain(a, sx, sy, sd, q, s_qn, keys, id0);
}

struct ResolveArgs {
    const rn_key *keys;
    const float *verts;
    const int32_t *faces;
    const uint8_t *colour, *image;
    int32_t *face_id;
    float *depth;
    uint8_t *rgb;
    long long npix, per_image;
    int n, V, F;
    float alpha, ambient;
    int default_colour, background;
};

__device__ __forceinline__ uint8_t rs_sat8(float v) { return v >= 255.0f ? (uint8_t)255 : v >= 0.0f ? (uint8_t)(int)v : (uint8_t)0; }

template <bool IDS, bool RGB>
__global__ __launch_bounds__(RS_THREADS) void render_resolve_kernel(const ResolveArgs a)
{
    const long long i = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= a.npix) return;
    const rn_key key = a.keys[i];
    bool bg = key == ~(rn_key)0;
    const uint32_t id = (uint32_t)key, hi = (uint32_t)(key >> 32);
    if constexpr (IDS) {
        a.face_id[i] = bg ? -1 : (int32_t)id;
        a.depth[i] = bg ? INFINITY : __uint_as_float((hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi);
    }
    if constexpr (RGB) {
        const int b = (int)(i / a.per_image);
        const uint32_t m = id / (uint32_t)a.F, f = id - m * (uint32_t)a.F;
        int i0 = 0, i1 = 0, i2 = 0;
        if (!bg) {
            bg = m >= (uint32_t)a.n;
            if (!bg) {
                const int32_t *fp = a.faces + 3LL * f;
                i0 = fp[0]; i1 = fp[1]; i2 = fp[2];
                bg = (unsigned)i0 >= (unsigned)a.V || (unsigned)i1 >= (unsigned)a.V || (unsigned)i2 >= (unsigned)a.V;
            }
        }
        float im[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) im[c] = a.image ? (float)a.image[3 * i + c] : (float)((a.background >> (16 - 8 * c)) & 255);
        uint8_t *out = a.rgb + 3 * i;
        if (bg) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = (uint8_t)(int)im[c];
            return;
        }
        const long long p = (long long)b * a.n + m;
        const float *v0 = a.verts + (p * a.V + i0) * 3, *v1 = a.verts + (p * a.V + i1) * 3, *v2 = a.verts + (p * a.V + i2) * 3;
        const float e1x = v1[0] - v0[0], e1y = v1[1] - v0[1], e1z = v1[2] - v0[2];
        const float e2x = v2[0] - v0[0], e2y = v2[1] - v0[1], e2z = v2[2] - v0[2];
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        float I = 0.0f;
        if (len != 0.0f) I = a.ambient + (1.0f - a.ambient) * (fabsf(nz) / len);
        const float oma = 1.0f - a.alpha;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float col = a.colour ? (float)a.colour[3 * p + c] : (float)((a.default_colour >> (16 - 8 * c)) & 255);
            out[c] = rs_sat8(rintf(a.alpha * (I * col) + oma * im[c]));
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static int render_check_target(const char *who, int B, int Hr, int Wr)
{
    if (B <= 0 || Hr <= 0 || Wr <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: B, Hr, Wr = %d, %d, %d", who, B, Hr, Wr);
    if (Hr > H3D_RENDER_MAX_SIDE || Wr > H3D_RENDER_MAX_SIDE)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: a target of %d x %d pixels, at most %d a side", who, Hr, Wr, H3D_RENDER_MAX_SIDE);
    if ((long long)B * Hr * Wr > 0x7fffffffLL) H3D_FAIL(H3D_ERR_SHAPE, "%s: B Hr Wr = %lld pixels", who, (long long)B * Hr * Wr);
    return H3D_OK;
}
static int render_check_mesh(const char *who, int n, int V, int F)
{
    if (n <= 0 || V <= 0 || F <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: n, V, F = %d, %d, %d", who, n, V, F);
    if ((long long)n * F > 0x7fffffffLL) H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: n F = %lld face ids, they must stay below 2^31", who, (long long)n * F);
    return H3D_OK;
}

struct RenderLayout {
    h3d_ws_layout L;
    size_t keys;
};
static RenderLayout render_layout(int B, int Hr, int Wr)
{
    RenderLayout w;
    w.keys = w.L.take((size_t)B * Hr * Wr * sizeof(rn_key));
    return w;
}

extern "C" int h3d_render_workspace_bytes(int B, int Hr, int Wr, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "render_workspace_bytes: null pointer");
    H3D_TRY(render_check_target("render_workspace_bytes", B, Hr, Wr));
    *bytes = render_layout(B, Hr, Wr).L.total;
    return H3D_OK;
}

static int render_resolve_blocks(long long npix) { return (int)((npix + RS_THREADS - 1) / RS_THREADS); }

extern "C" int h3d_render_rasterize(const float *verts, const int32_t *faces, const float *cam_map, const int64_t *ind, const uint8_t *valid,
                                    const float *dz, int B, int max_objs, int n, int V, int F, int H, int W, int up, int flags,
                                    int32_t *face_id, float *depth, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "render_rasterize";
    if (B <= 0 || max_objs <= 0 || H <= 0 || W <= 0) H3D_FAIL(H3D_ERR_SHAPE, "%s: B, max_objs, H, W = %d, %d, %d, %d", who, B, max_objs, H, W);
    H3D_TRY(render_check_mesh(who, n, V, F));
    if (n > max_objs) H3D_FAIL(H3D_ERR_SHAPE, "%s: n = %d > max_objs = %d", who, n, max_objs);
    if (up < 1 || (long long)up * H > H3D_RENDER_MAX_SIDE || (long long)up * W > H3D_RENDER_MAX_SIDE)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: up = %d on a %d x %d map, the target is at most %d a side", who, up, H, W, H3D_RENDER_MAX_SIDE);
    const int Hr = up * H, Wr = up * W;
    H3D_TRY(render_check_target(who, B, Hr, Wr));
    if ((long long)B * n > 0x7fffffffLL) H3D_FAIL(H3D_ERR_SHAPE, "%s: B n = %lld person slots", who, (long long)B * n);
    if (V > H3D_RENDER_MAX_V) H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: V = %d vertices, the kernel stages at most %d in LDS", who, V, H3D_RENDER_MAX_V);
    if (flags & ~(H3D_RENDER_NEGATE_Z | H3D_RENDER_CULL_BACK)) H3D_FAIL(H3D_ERR_ARG, "%s: flags 0x%x", who, flags);
    if (!verts || !faces || !cam_map || !ind || !face_id || !depth) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    const RenderLayout w = render_layout(B, Hr, Wr);
    if (!workspace || workspace_bytes < w.L.total || ((uintptr_t)workspace & 7))
        H3D_FAIL(H3D_ERR_ARG, "%s: workspace of %zu bytes (8-byte aligned), %zu needed", who, workspace ? workspace_bytes : (size_t)0, w.L.total);
    const hipStream_t st = (hipStream_t)stream;
    rn_key *keys = (rn_key *)((char *)workspace + w.keys);
    const long long npix = (long long)B * Hr * Wr;
    RasterArgs a;
    a.verts = verts; a.cam = cam_map; a.dz = dz; a.faces = faces; a.ind = ind; a.valid = valid; a.keys = keys;
    a.max_objs = max_objs; a.n = n; a.V = V; a.Vs = (V + 3) & ~3; a.F = F; a.H = H; a.W = W; a.up = up; a.Hr = Hr; a.Wr = Wr; a.flags = flags;
    const size_t lds = 12 * (size_t)a.Vs + 4 * (size_t)RN_QCAP;
    if (hipMemsetAsync(keys, 0xFF, (size_t)npix * sizeof(rn_key), st) != hipSuccess) H3D_FAIL(H3D_ERR_LAUNCH, "%s: the memset of the key buffer failed", who);
    static thread_local size_t max_set = 0;
    if (lds > 64 * 1024 && lds > max_set) {
        if (hipFuncSetAttribute((const void *)render_raster_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            H3D_FAIL(H3D_ERR_LAUNCH, "%s: cannot reserve %zu bytes of LDS", who, lds);
        max_set = lds;
    }
    H3D_TRY(h3d_launch({"render_raster_kernel"}, render_raster_kernel, dim3((unsigned)(B * n)), dim3(RN_THREADS), lds, st, a));
    ResolveArgs r = {};
    r.keys = keys; r.face_id = face_id; r.depth = depth; r.npix = npix; r.per_image = (long long)Hr * Wr; r.n = n; r.V = V; r.F = F;
    return h3d_launch({"render_resolve_kernel", true, false}, render_resolve_kernel<true, false>, dim3(render_resolve_blocks(npix)), dim3(RS_THREADS), 0, st, r);
}

extern "C" int h3d_render_shade(const void *keys, const float *verts, const int32_t *faces, const uint8_t *colour, const uint8_t *image, int B,
                                int n, int V, int F, int Hr, int Wr, float alpha, float ambient, int default_colour, int background,
                                uint8_t *rgb, void *stream)
{
    const char *who = "render_shade";
    H3D_TRY(render_check_target(who, B, Hr, Wr));
    H3D_TRY(render_check_mesh(who, n, V, F));
    if ((long long)B * n > 0x7fffffffLL) H3D_FAIL(H3D_ERR_SHAPE, "%s: B n = %lld person slots", who, (long long)B * n);
    if (!(alpha >= 0.0f && alpha <= 1.0f) || !(ambient >= 0.0f && ambient <= 1.0f))
        H3D_FAIL(H3D_ERR_ARG, "%s: alpha = %g, ambient = %g, both must lie in [0, 1]", who, (double)alpha, (double)ambient);
    if (!keys || !verts || !faces || !rgb) H3D_FAIL(H3D_ERR_ARG, "%s: null pointer", who);
    if ((uintptr_t)keys & 7) H3D_FAIL(H3D_ERR_ARG, "%s: the key buffer must be 8-byte aligned", who);
    ResolveArgs r = {};
    r.keys = (const rn_key *)keys; r.verts = verts; r.faces = faces; r.colour = colour; r.image = image; r.rgb = rgb;
    r.npix = (long long)B * Hr * Wr; r.per_image = (long long)Hr * Wr; r.n = n; r.V = V; r.F = F;
    r.alpha = alpha; r.ambient = ambient; r.default_colour = default_colour; r.background = background;
    return h3d_launch({"render_resolve_kernel", false, true}, render_resolve_kernel<false, true>, dim3(render_resolve_blocks(r.npix)), dim3(RS_THREADS), 0,
                      (hipStream_t)stream, r);
}
