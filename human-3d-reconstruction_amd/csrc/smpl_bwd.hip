// SMPL backward on gfx950: the gradients of the LBS mesh stage (smpl.hip) with respect to betas / thetas, or to the `shape` / `pose`
// head maps (include/h3d.h section 4b; derivation in DESIGN.md).  Forward, per person:
//     coef = [beta | vec(R[1:] - I)]      v_p = v_template + D . coef      A_j from the kinematic chain
//     T_v = sum_j w_vj A_j                verts_v = T_v [v_p; 1]           joints_j = G_j.t
// Three launches, everything recomputed from betas / thetas (h3d_smpl_pose + h3d_smpl_coef_pack into the workspace first):
//   smpl_bwd_verts_kernel  64 vertices x 256 persons per step, as smpl_verts3_kernel: v_p by the forward's six-product contraction, its
//                          vertex fetch, accumulator transposition and blended transform T (all smpl_tile.h, shared, not copied; the
//                          clamp of the joint indices is this kernel's own), then with lane = vertex g_vp = T_R^T gV -> [P][3][Vpad] and
//                          this tile's part of gA[p][j] = sum_v w_vj gV_v (x) [v_p; 1] (24 x 12 per person), summed over the tile's
//                          vertices in vertex order.  A workgroup walks SB_NVT consecutive vertex tiles and adds each into ONE partial
//                          per (tile group, person): plain loads and stores of a slot no other workgroup touches.
//   smpl_bwd_coef_kernel   g_coef[p][k] = sum_{c,v} D[v,c,k] g_vp[p][c][v]: the forward's product transposed, on the bf16 matrix cores
//                          with both operands as three bf16 terms and all six products (g_vp is split on the device while it is
//                          loaded; the directions come V-contiguous and pre-split: dirsV3).  The contraction length 3 Vpad is cut
//                          into splits of SB_KC; one plain-stored partial per (split, person).
//   smpl_bwd_pose_kernel   the mirror of smpl_pose_kernel, one lane per (person, joint), two persons per wave, in fp64 (the stage is a
//                          few microseconds, and fp64 removes the cancellations of sin(a)/a and (1 - cos a)/a^2 near the rest pose):
//                          its forward is smpl_pose.h with T = double, the code smpl_pose_kernel runs with T = float (shared, not
//                          copied); then it sums the partials of the two kernels above in their stored order, walks the chain children
//                          first (lane `step` hands its contribution to its parent by a shuffle, steps 23 .. 1: a fixed order), applies the
//                          rest-joint gradient to grad_betas and the Rodrigues backward to grad_thetas.
// No float atomics except the heads variant's scatter into the zero-filled maps (two detections may share a pixel).
// Host side: the two entry points keep their own checks, zero fills and early returns; their launches are sb_run.
#include "common.h"
#include "smpl_tile.h"
#include "smpl_pose.h"

constexpr int SB_NVT = 4;                     // vertex tiles (of 64) one workgroup folds into one gA partial
constexpr int SB_RP = 4;                      // persons per skinning round and wave
constexpr int SB_TSTRIDE = 193 * 4;           // transposed tile: bytes per person (64 v x 3 floats + 1)
constexpr int SB_T = S3_NW * SB_RP * SB_TSTRIDE;             // 24704: v_p tiles, then the gV tiles
constexpr int SB_LBS = 2 * SB_T + S3_NW * SB_RP * SMPL_J * 12 * 4;
static_assert(SB_LBS <= 2 * S3_SLOT, "the skinning staging fits the idle ring");
constexpr int SB_WS = 25;                     // row stride (floats) of the tile's dense skinning weights [64][24]
constexpr int SB_KC = 1536;                   // contraction elements per split of the coefficient kernel (96 MFMA steps)
constexpr int SB_KP = 224;                    // coefficient rows, padded as the forward pads K

static inline int sb_groups(int Vpad) { return cdiv(Vpad / S3_VT, SB_NVT); }
static inline int sb_splits(int Vpad) { return cdiv(3 * Vpad, SB_KC); }

__global__ __launch_bounds__(64 * S3_NW) void smpl_bwd_verts_kernel(const bf16_t *__restrict__ coefK3, const float *__restrict__ A,
                                                                    const float *__restrict__ v_template,
                                                                    const bf16_t *__restrict__ dirsK3,
                                                                    const int32_t *__restrict__ lbs_idx, const float *__restrict__ lbs_w,
                                                                    int nnz, int P, int Ppad, int V, int Vpad,
                                                                    const float *__restrict__ grad_verts, float *__restrict__ gvp,
                                                                    float *gApart)
{
    __shared__ __attribute__((aligned(1024))) char smem[2 * S3_SLOT];
    __shared__ float s_W[S3_VT * SB_WS];
    __shared__ int s_jl[SMPL_J + 1];          // joints with a non-zero weight in this tile, ascending; [24] = how many
    const int tid = threadIdx.x, l = tid & 63, r = l & 31, h = l >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p0 = blockIdx.y * S3_PB;
    int aoff[S3_AJ], boff[S3_BJ];
    s3_coef_offsets<true>(boff, wv, l, p0);
    const int dbytes = 3 * Vpad * S3_GROW, cbytes = Ppad * S3_GROW;
    const int fa_off = r * S3_ROWB + h * 16;
    const int fb_off = S3_APIECES * 1024 + (wv * 32 + r) * S3_ROWB + h * 16;
    char *sT = smem + wv * (SB_RP * SB_TSTRIDE);                                // [4 persons][64 v][3] (+1): v_p
    char *sG = smem + SB_T + wv * (SB_RP * SB_TSTRIDE);                         // the same shape: gV
    float *sA = reinterpret_cast<float *>(smem + 2 * SB_T) + wv * (SB_RP * SMPL_J * 12);
    const int ntile = Vpad / S3_VT;
    const int t_end = (blockIdx.x + 1) * SB_NVT < ntile ? (blockIdx.x + 1) * SB_NVT : ntile;
    for (int vt = blockIdx.x * SB_NVT; vt < t_end; ++vt) {
        const int v0 = vt * S3_VT;
        s3_dir_offsets<true>(aoff, wv, l, v0, Vpad);
        f32x16 acc[3][2];
        s3_zero(acc);
        // this lane's vertex in the skinning phase (rows past V compute a duplicate of V - 1 with a zero upstream gradient); the joint
        // indices also address s_W and gApart here, so they are clamped
        const int v = v0 + l;
        S3Vertex vx;
        s3_vertex(vx, v < V ? v : V - 1, nnz, lbs_idx, lbs_w, v_template, Vpad);
#pragma unroll
        for (int sI = 0; sI < 4; ++sI) vx.jidx[sI] = vx.jidx[sI] < 0 ? 0 : vx.jidx[sI] >= SMPL_J ? SMPL_J - 1 : vx.jidx[sI];
        if (wv == 0) {                         // the tile's skinning weights as a dense [64][24] block: row l is private to lane l
            for (int j = 0; j < SMPL_J; ++j) s_W[l * SB_WS + j] = 0.f;
#pragma unroll
            for (int sI = 0; sI < 4; ++sI)
                if (vx.jw[sI] != 0.f) s_W[l * SB_WS + vx.jidx[sI]] += vx.jw[sI];
        }
        s3_issue((const char *)dirsK3, dbytes, (const char *)coefK3, cbytes, smem, aoff, boff, wv, 0);
        s3_contract<true, 0>(acc, smem, (const char *)dirsK3, dbytes, (const char *)coefK3, cbytes, aoff, boff, wv, fa_off, fb_off);
        __syncthreads();                       // the ring is free; s_W is complete
        if (wv == 0) {
            bool pres = false;
            if (l < SMPL_J)
                for (int vv = 0; vv < S3_VT; ++vv) pres = pres || s_W[vv * SB_WS + l] != 0.f;
            const unsigned long long m = __ballot(pres);
            if (pres) s_jl[__popcll(m & ((1ull << l) - 1ull))] = l;
            if (l == 0) s_jl[SMPL_J] = __popcll(m);
        }
        __syncthreads();
        const int nj = s_jl[SMPL_J];
#pragma unroll 1
        for (int rnd = 0; rnd < 32 / SB_RP; ++rnd) {
            // sT / sG / sA are private to the wave and LDS executes a wave's instructions in order (as in smpl_verts3_kernel)
            __builtin_amdgcn_wave_barrier();
            s3_transpose_round<SB_RP, SB_TSTRIDE>(acc, sT, rnd, r, h);          // (a) the displacements of persons [4 rnd, 4 rnd + 4)
            for (int i = l; i < SB_RP * SMPL_J * 3; i += 64) {          // (b) their 3x4 transforms
                const int q = i / (SMPL_J * 3), rr = i - q * (SMPL_J * 3);
                const int p = p0 + wv * 32 + rnd * SB_RP + q;
                f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
                if (p < P) a4 = *reinterpret_cast<const f32x4 *>(A + (size_t)p * SMPL_J * 12 + 4 * rr);
                *reinterpret_cast<f32x4 *>(sA + q * SMPL_J * 12 + 4 * rr) = a4;
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < SB_RP; ++q) {   // (c) lane = vertex: g_vp = T_R^T gV; v_p and gV go back to LDS for the reduction
                const int p = p0 + wv * 32 + rnd * SB_RP + q;
                float T[12];
                s3_blend(T, sA + q * SMPL_J * 12, vx);
                float *xyz = reinterpret_cast<float *>(sT + q * SB_TSTRIDE + l * 12);
                float *gq = reinterpret_cast<float *>(sG + q * SB_TSTRIDE + l * 12);
                const float x = vx.t0 + xyz[0], y = vx.t1 + xyz[1], z = vx.t2 + xyz[2];
                float gx = 0.f, gy = 0.f, gz = 0.f;
                if (v < V && p < P) {
                    const float *gv = grad_verts + ((size_t)p * V + v) * 3;
                    gx = gv[0]; gy = gv[1]; gz = gv[2];
                }
                xyz[0] = x; xyz[1] = y; xyz[2] = z;
                gq[0] = gx; gq[1] = gy; gq[2] = gz;
                if (p < P) {
                    float *o = gvp + (size_t)p * 3 * Vpad + v;          // v < Vpad; rows past V receive zeros
                    // (the roundings written out: as a * gx + b * gy + c * gz the contraction moves with the code around it)
                    o[0] = fmaf(T[8], gz, fmaf(T[0], gx, T[4] * gy));
                    o[Vpad] = fmaf(T[9], gz, fmaf(T[1], gx, T[5] * gy));
                    o[2 * (size_t)Vpad] = fmaf(T[10], gz, fmaf(T[2], gx, T[6] * gy));
                }
            }
            __builtin_amdgcn_wave_barrier();
            // (d) gA[p][j][a][0..3] += sum_v w_vj gV_v[a] [v_p; 1], v ascending: one lane per (person, present joint, row)
            const int ntask = SB_RP * nj * 3;
            for (int id = l; id < ntask; id += 64) {
                const int a = id % 3, js = (id / 3) % nj, q = id / (3 * nj);
                const int j = s_jl[js];
                const int p = p0 + wv * 32 + rnd * SB_RP + q;
                const float *xq = reinterpret_cast<const float *>(sT + q * SB_TSTRIDE);
                const float *gq = reinterpret_cast<const float *>(sG + q * SB_TSTRIDE) + a;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 4
                for (int vv = 0; vv < S3_VT; ++vv) {
                    const float w = s_W[vv * SB_WS + j], g = w * gq[vv * 3];
                    s0 = fmaf(g, xq[vv * 3], s0);
                    s1 = fmaf(g, xq[vv * 3 + 1], s1);
                    s2 = fmaf(g, xq[vv * 3 + 2], s2);
                    s3 = fmaf(w, gq[vv * 3], s3);          // not s3 + g: one rounding, as the sum always had
                }
                if (p < P) {
                    float *o = gApart + ((size_t)blockIdx.x * P + p) * (SMPL_J * 12) + j * 12 + a * 4;
                    f32x4 old = *reinterpret_cast<const f32x4 *>(o);
                    old[0] += s0; old[1] += s1; old[2] += s2; old[3] += s3;
                    *reinterpret_cast<f32x4 *>(o) = old;
                }
            }
        }
        __syncthreads();                       // the next tile's DMA overwrites the staging areas, its wave 0 s_W; orders the partial's stores
    }
}

// bf16 three-term split of 8 consecutive fp32 values into the three MFMA fragments
__device__ __forceinline__ void sb_split8(const f32x4 &g0, const f32x4 &g1, u32x4 &fh, u32x4 &fm, u32x4 &fl)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x0 = e < 2 ? g0[2 * e] : g1[2 * e - 4], x1 = e < 2 ? g0[2 * e + 1] : g1[2 * e - 3];
        const uint32_t hh = pack_bf16x2(x0, x1);
        const float r0 = x0 - __uint_as_float(hh << 16), r1 = x1 - __uint_as_float(hh & 0xffff0000u);
        const uint32_t mm = pack_bf16x2(r0, r1);
        const float q0 = r0 - __uint_as_float(mm << 16), q1 = r1 - __uint_as_float(mm & 0xffff0000u);
        fh[e] = hh; fm[e] = mm; fl[e] = pack_bf16x2(q0, q1);
    }
}

// wave = 32 persons x 224 coefficients over one split of the contraction; fragments straight from global memory (8 consecutive
// contraction elements per lane: 32 B of g_vp, 16 B of each direction term)
__global__ __launch_bounds__(256) void smpl_bwd_coef_kernel(const float *__restrict__ gvp, const bf16_t *__restrict__ dirsV3, int P, int K3,
                                                            float *__restrict__ gcpart)
{
    using E = ET<bf16_t>;
    const int tid = threadIdx.x, l = tid & 63, r = l & 31, h = l >> 5, wv = tid >> 6;
    const int pw0 = (blockIdx.x * 4 + wv) * 32;
    if (pw0 >= P) return;
    const int k_begin = blockIdx.y * SB_KC;
    const int k_end = k_begin + SB_KC < K3 ? k_begin + SB_KC : K3;
    const int prow = pw0 + r < P ? pw0 + r : P - 1;
    const float *gp = gvp + (size_t)prow * K3 + 8 * h;
    const bf16_t *dp = dirsV3 + (size_t)r * K3 + 8 * h;
    const size_t term = (size_t)SB_KP * K3;
    f32x16 acc[SB_KP / 32];
#pragma unroll
    for (int kt = 0; kt < SB_KP / 32; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[kt][i] = 0.f;
    for (int kk = k_begin; kk < k_end; kk += 16) {
        const f32x4 g0 = *reinterpret_cast<const f32x4 *>(gp + kk), g1 = *reinterpret_cast<const f32x4 *>(gp + kk + 4);
        E::frag bh, bm, bl;
        sb_split8(g0, g1, bh.v, bm.v, bl.v);
#pragma unroll
        for (int kt = 0; kt < SB_KP / 32; ++kt) {
            const bf16_t *d = dp + (size_t)kt * 32 * K3 + kk;
            E::frag ah, am, al;
            ah.v = *reinterpret_cast<const u32x4 *>(d);
            am.v = *reinterpret_cast<const u32x4 *>(d + term);
            al.v = *reinterpret_cast<const u32x4 *>(d + 2 * term);
            E::mma(acc[kt], al, bh);           // smallest terms first, as the forward
            E::mma(acc[kt], ah, bl);
            E::mma(acc[kt], am, bm);
            E::mma(acc[kt], am, bh);
            E::mma(acc[kt], ah, bm);
            E::mma(acc[kt], ah, bh);
        }
    }
    if (pw0 + r < P) {
        float *o = gcpart + ((size_t)blockIdx.y * P + pw0 + r) * SB_KP;
#pragma unroll
        for (int kt = 0; kt < SB_KP / 32; ++kt)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[kt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h] = acc[kt][i];
    }
}

struct SmplBwdHeads : SmplHeadMaps {
    float *gpose, *gshape;                    // [B,72,HW], [B,10,HW], zero-filled by the launcher; either may be NULL
};

template <bool HEADS>
__global__ __launch_bounds__(64) void smpl_bwd_pose_kernel(const float *__restrict__ betas, const float *__restrict__ thetas,
                                                           const float *__restrict__ j_template, const float *__restrict__ j_shapedirs,
                                                           const int32_t *__restrict__ parents, int P,
                                                           const float *__restrict__ grad_joints, const float *__restrict__ gApart, int NG,
                                                           const float *__restrict__ gcpart, int NS, float *__restrict__ grad_betas,
                                                           float *__restrict__ grad_thetas, SmplBwdHeads hs)
{
    const SmplLane ln = smpl_lane(P);
    const int j = ln.j, half = ln.half, p = ln.p, pc = ln.pc, jc = ln.jc;
    const bool act = ln.act;
    // ---- the forward of smpl_pose_kernel (smpl_pose.h), in fp64 ----
    double beta[SMPL_NB], jr[3];
    float th[3];
    [[maybe_unused]] SmplHeadPix hp;
    if constexpr (HEADS) hp = smpl_head_pix(hs, pc);
    [[maybe_unused]] const size_t hb = hp.hb;
    [[maybe_unused]] const int hpix = hp.hpix;
    smpl_load_beta<HEADS>(beta, betas, hs, hp, pc);
    smpl_load_theta<HEADS>(th, thetas, hs, hp, pc, jc);
    smpl_rest_joint(jr, j_template, j_shapedirs, beta, jc);
    const SmplRot<double> rot = smpl_rodrigues<double>(th[0], th[1], th[2]);
    const double x = rot.x, y = rot.y, z = rot.z, inv = rot.inv, ex = rot.ex, ey = rot.ey, ez = rot.ez, sn = rot.sn, cs = rot.cs, oc = rot.oc;
    const double (&R)[9] = rot.R;
    const int par = parents[jc];
    const int plane = half * 32 + (par < 0 ? 0 : par);
    double rel[3], G[12];                      // G: global transform rows [R | t]
    smpl_local(rel, G, R, jr, par, plane);
    smpl_chain(G, j, plane);
    // ---- upstream: gA (the vertex kernel's partials, tile groups in order), grad_joints ----
    double gA[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) gA[i] = 0.0;
    if (gApart) {
        for (int g = 0; g < NG; ++g) {
            const float *s = gApart + ((size_t)g * P + pc) * (SMPL_J * 12) + jc * 12;
#pragma unroll
            for (int i4 = 0; i4 < 3; ++i4) {
                const f32x4 v4 = *reinterpret_cast<const f32x4 *>(s + 4 * i4);
#pragma unroll
                for (int e = 0; e < 4; ++e) gA[4 * i4 + e] += (double)v4[e];
            }
        }
    }
    double gG[12];                             // gradient at the global transform, rows [gR | gt]
    double gjr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double gj = grad_joints ? (double)grad_joints[((size_t)pc * SMPL_J + jc) * 3 + a] : 0.0;
        // A_j = [G.R | G.t - G.R jr]
        gG[a * 4] = gA[a * 4] - gA[a * 4 + 3] * jr[0];
        gG[a * 4 + 1] = gA[a * 4 + 1] - gA[a * 4 + 3] * jr[1];
        gG[a * 4 + 2] = gA[a * 4 + 2] - gA[a * 4 + 3] * jr[2];
        gG[a * 4 + 3] = gA[a * 4 + 3] + gj;
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) gjr[b] = -(G[b] * gA[3] + G[4 + b] * gA[7] + G[8 + b] * gA[11]);
    // ---- the chain in reverse, children first: G_j = G_par . [R_j | rel_j] ----
    for (int step = SMPL_J - 1; step >= 1; --step) {
        double c[12];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b)
                c[a * 4 + b] = gG[a * 4] * R[b * 3] + gG[a * 4 + 1] * R[b * 3 + 1] + gG[a * 4 + 2] * R[b * 3 + 2] + gG[a * 4 + 3] * rel[b];
            c[a * 4 + 3] = gG[a * 4 + 3];
        }
        const int src = half * 32 + step;
        const int ps = parents[step];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const double got = __shfl(c[i], src);
            if (j == ps) gG[i] += got;
        }
    }
    // gradient at the local rotation and at rel_j
    double GpR[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) GpR[a * 3 + b] = __shfl(G[a * 4 + b], plane);
    double gR[9], grel[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b)
            gR[a * 3 + b] = par < 0 ? gG[a * 4 + b] : GpR[a] * gG[b] + GpR[3 + a] * gG[4 + b] + GpR[6 + a] * gG[8 + b];
        grel[a] = par < 0 ? gG[a * 4 + 3] : GpR[a] * gG[3] + GpR[3 + a] * gG[7] + GpR[6 + a] * gG[11];
    }
    if (gcpart && jc > 0) {                    // the pose feature vec(R[1:] - I): splits in order
        for (int s = 0; s < NS; ++s) {
            const float *gc = gcpart + ((size_t)s * P + pc) * SB_KP + SMPL_NB + (jc - 1) * 9;
#pragma unroll
            for (int i = 0; i < 9; ++i) gR[i] += (double)gc[i];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) gjr[a] += grel[a];
    for (int step = 1; step < SMPL_J; ++step) {          // rel_step = jr_step - jr_parent
        const int src = half * 32 + step;
        const int ps = parents[step];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double got = __shfl(grel[a], src);
            if (j == ps) gjr[a] -= got;
        }
    }
    // ---- grad_betas: lane k < 10 of each person, joints in order ----
    {
        const int k = j < SMPL_NB ? j : 0;
        double s = 0.0;
        if (gcpart)
            for (int sp = 0; sp < NS; ++sp) s += (double)gcpart[((size_t)sp * P + pc) * SB_KP + k];
        for (int jj = 0; jj < SMPL_J; ++jj) {
            const int src = half * 32 + jj;
#pragma unroll
            for (int c = 0; c < 3; ++c) s += (double)j_shapedirs[(jj * 3 + c) * SMPL_NB + k] * __shfl(gjr[c], src);
        }
        if (p < P && j < SMPL_NB) {
            if constexpr (HEADS) {
                if (hs.gshape) atomicAdd(hs.gshape + (hb * SMPL_NB + k) * hs.HW + hpix, (float)s);
            } else {
                if (grad_betas) grad_betas[(size_t)p * SMPL_NB + k] = (float)s;
            }
        }
    }
    // ---- Rodrigues backward ----
    const double d31 = gR[3] - gR[1], d26 = gR[2] - gR[6], d75 = gR[7] - gR[5];
    const double s13 = gR[1] + gR[3], s26 = gR[2] + gR[6], s57 = gR[5] + gR[7];
    const double gsn = z * d31 + y * d26 + x * d75;
    const double goc = -(y * y + z * z) * gR[0] + x * y * s13 + x * z * s26 - (x * x + z * z) * gR[4] + y * z * s57 - (x * x + y * y) * gR[8];
    const double gx = sn * d75 + oc * (y * s13 + z * s26 - 2.0 * x * (gR[4] + gR[8]));
    const double gy = sn * d26 + oc * (x * s13 + z * s57 - 2.0 * y * (gR[0] + gR[8]));
    const double gz = sn * d31 + oc * (x * s26 + y * s57 - 2.0 * z * (gR[0] + gR[4]));
    const double ga = gsn * cs + goc * sn - (gx * x + gy * y + gz * z) * inv;
    const double gt[3] = {gx * inv + ga * ex * inv, gy * inv + ga * ey * inv, gz * inv + ga * ez * inv};
    if (act) {
        if constexpr (HEADS) {
            if (hs.gpose) {
#pragma unroll
                for (int c = 0; c < 3; ++c) atomicAdd(hs.gpose + (hb * 72 + j * 3 + c) * hs.HW + hpix, (float)gt[c]);
            }
        } else {
            if (grad_thetas) {
#pragma unroll
                for (int c = 0; c < 3; ++c) grad_thetas[(size_t)p * 72 + j * 3 + c] = (float)gt[c];
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct SbWorkspace { size_t pf, A, joints, coefK3, gvp, gApart, gcpart, total; };

static SbWorkspace sb_layout(int P, int Vpad)
{
    const size_t Ppad = (size_t)cdiv(P, S3_PPAD) * S3_PPAD;
    SbWorkspace w;
    h3d_ws_layout ws;
    w.pf = ws.take((size_t)4 * P * SMPL_PF);
    w.A = ws.take((size_t)4 * P * SMPL_J * 12);
    w.joints = ws.take((size_t)4 * P * SMPL_J * 3);
    w.coefK3 = ws.take(Ppad * S3_GROW);
    w.gvp = ws.take((size_t)4 * P * 3 * Vpad);
    w.gApart = ws.take((size_t)4 * sb_groups(Vpad) * P * SMPL_J * 12);
    w.gcpart = ws.take((size_t)4 * sb_splits(Vpad) * P * SB_KP);
    w.total = ws.total;
    return w;
}

static int sb_check_shape(const char *what, int P, int V, int Vpad, int nnz)
{
    if (P < 0 || V <= 0 || Vpad < V || Vpad % S3_VT || nnz <= 0)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: P=%d V=%d (pad %d, multiple of %d) nnz=%d", what, P, V, Vpad, S3_VT, nnz);
    if (nnz > 4) H3D_FAIL(H3D_ERR_UNSUPPORTED, "%s: nnz=%d: at most 4 skinning weights per vertex", what, nnz);
    const size_t Ppad = (size_t)cdiv(P, S3_PPAD) * S3_PPAD;
    if ((size_t)3 * Vpad * S3_GROW >= 0x7ffffff0ull || Ppad * S3_GROW >= 0x7ffffff0ull)
        H3D_FAIL(H3D_ERR_SHAPE, "%s: operand of 2 GiB or more", what);
    return H3D_OK;
}

extern "C" int h3d_smpl_backward_workspace_bytes(int P, int V, int Vpad, int nnz, int want_verts, size_t *bytes)
{
    if (!bytes) H3D_FAIL(H3D_ERR_ARG, "smpl_backward_workspace_bytes: null pointer");
    const int rc = sb_check_shape("smpl_backward_workspace_bytes", P, V, Vpad, nnz);
    if (rc != H3D_OK) return rc;
    *bytes = (want_verts && P > 0) ? sb_layout(P, Vpad).total : 0;
    return H3D_OK;
}

// what an upstream grad_verts needs: the model tensors of the vertex kernels and the workspace
static int sb_check_verts_args(const char *what, const SbWorkspace &w, const float *grad_verts, const float *v_template, const void *dirsK3,
                               const void *dirsV3, const int32_t *lbs_idx, const float *lbs_w, const void *workspace, size_t workspace_bytes)
{
    if (grad_verts && (!v_template || !dirsK3 || !dirsV3 || !lbs_idx || !lbs_w))
        H3D_FAIL(H3D_ERR_ARG, "%s: null model pointer with grad_verts given", what);
    if (grad_verts && (!workspace || workspace_bytes < w.total))
        H3D_FAIL(H3D_ERR_ARG, "%s: workspace of %zu bytes needed, %zu given", what, w.total, workspace ? workspace_bytes : (size_t)0);
    return H3D_OK;
}

// The launches of both entry points, past their checks and early returns; HEADS: the parameters come from the head maps of `hs` (betas,
// thetas, grad_betas, grad_thetas NULL), the gradients go to its maps.  With grad_verts the forward pose stage of that flavour fills
// pf / A / coefK3 of the workspace and the two hot kernels leave their partials there; the pose kernel then reads them.
template <bool HEADS>
static int sb_run(const float *betas, const float *thetas, const SmplBwdHeads &hs, const float *grad_verts, const float *grad_joints,
                  const float *j_template, const float *j_shapedirs, const int32_t *parents, const float *v_template, const void *dirsK3,
                  const void *dirsV3, const int32_t *lbs_idx, const float *lbs_w, int nnz, int P, int V, int Vpad, float *grad_betas,
                  float *grad_thetas, const SbWorkspace &w, void *workspace, void *stream)
{
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    const int NG = sb_groups(Vpad), NS = sb_splits(Vpad), Ppad = cdiv(P, S3_PPAD) * S3_PPAD;
    if (grad_verts) {
        float *pf = (float *)(ws + w.pf), *A = (float *)(ws + w.A), *joints = (float *)(ws + w.joints);
        if constexpr (HEADS) {
            H3D_TRY(h3d_smpl_pose_heads(hs.pose_map, hs.shape_map, hs.inds, P / hs.n, hs.K, hs.n, hs.HW, j_template, j_shapedirs, parents, nullptr,
                                        pf, A, joints, ws + w.coefK3, Ppad, stream));
        } else {
            H3D_TRY(h3d_smpl_pose(betas, thetas, j_template, j_shapedirs, parents, P, pf, A, joints, nullptr, Ppad, stream));
            H3D_TRY(h3d_smpl_coef_pack(betas, pf, P, Ppad, ws + w.coefK3, stream));
        }
        if (hipMemsetAsync(ws + w.gApart, 0, (size_t)4 * NG * P * SMPL_J * 12, st) != hipSuccess)
            H3D_FAIL(H3D_ERR_LAUNCH, "smpl_backward: clearing the transform-gradient partials failed");
        H3D_TRY(h3d_launch({"smpl_bwd_verts_kernel"}, smpl_bwd_verts_kernel, dim3(NG, cdiv(Ppad, S3_PB)), dim3(64 * S3_NW), 0, st, (const bf16_t *)(ws + w.coefK3),
                           (const float *)A, v_template, (const bf16_t *)dirsK3, lbs_idx, lbs_w, nnz, P, Ppad, V, Vpad, grad_verts,
                           (float *)(ws + w.gvp), (float *)(ws + w.gApart)));
        H3D_TRY(h3d_launch({"smpl_bwd_coef_kernel"}, smpl_bwd_coef_kernel, dim3(cdiv(P, 128), NS), dim3(256), 0, st, (const float *)(ws + w.gvp),
                           (const bf16_t *)dirsV3, P, 3 * Vpad, (float *)(ws + w.gcpart)));
    }
    return h3d_launch({"smpl_bwd_pose_kernel", HEADS}, smpl_bwd_pose_kernel<HEADS>, dim3(cdiv(P, 2)), dim3(64), 0, st, betas, thetas, j_template, j_shapedirs,
                      parents, P, grad_joints, grad_verts ? (const float *)(ws + w.gApart) : nullptr, NG,
                      grad_verts ? (const float *)(ws + w.gcpart) : nullptr, NS, grad_betas, grad_thetas, hs);
}

extern "C" int h3d_smpl_backward(const float *betas, const float *thetas, const float *grad_verts, const float *grad_joints,
                                 const float *j_template, const float *j_shapedirs, const int32_t *parents, const float *v_template,
                                 const void *dirsK3, const void *dirsV3, const int32_t *lbs_idx, const float *lbs_w, int nnz, int P, int V,
                                 int Vpad, float *grad_betas, float *grad_thetas, void *workspace, size_t workspace_bytes, void *stream)
{
    H3D_TRY(sb_check_shape("smpl_backward", P, V, Vpad, nnz));
    if (P == 0) return H3D_OK;
    if (!betas || !thetas || !j_template || !j_shapedirs || !parents) H3D_FAIL(H3D_ERR_ARG, "smpl_backward: null pointer");
    const SbWorkspace w = sb_layout(P, Vpad);
    H3D_TRY(sb_check_verts_args("smpl_backward", w, grad_verts, v_template, dirsK3, dirsV3, lbs_idx, lbs_w, workspace, workspace_bytes));
    if (!grad_verts && !grad_joints) {
        hipStream_t st = (hipStream_t)stream;
        if ((grad_betas && hipMemsetAsync(grad_betas, 0, (size_t)4 * P * SMPL_NB, st) != hipSuccess) ||
            (grad_thetas && hipMemsetAsync(grad_thetas, 0, (size_t)4 * P * 72, st) != hipSuccess))
            H3D_FAIL(H3D_ERR_LAUNCH, "smpl_backward: zero fill failed");
        return H3D_OK;
    }
    if (!grad_betas && !grad_thetas) return H3D_OK;
    return sb_run<false>(betas, thetas, SmplBwdHeads{}, grad_verts, grad_joints, j_template, j_shapedirs, parents, v_template, dirsK3, dirsV3, lbs_idx,
                         lbs_w, nnz, P, V, Vpad, grad_betas, grad_thetas, w, workspace, stream);
}

extern "C" int h3d_smpl_heads_backward(const float *pose_map, const float *shape_map, const int64_t *inds, int B, int K, int n, int HW,
                                       const float *grad_verts, const float *grad_joints, const float *j_template,
                                       const float *j_shapedirs, const int32_t *parents, const float *v_template, const void *dirsK3,
                                       const void *dirsV3, const int32_t *lbs_idx, const float *lbs_w, int nnz, int V, int Vpad,
                                       float *grad_pose_map, float *grad_shape_map, void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || K < 0 || n < 0 || n > K || HW < 0 || (B > 0 && n > 0 && HW == 0) || (long long)B * n > 0x7fffffffLL)
        H3D_FAIL(H3D_ERR_SHAPE, "smpl_heads_backward: B=%d K=%d n=%d HW=%d", B, K, n, HW);
    const int P = B * n;
    H3D_TRY(sb_check_shape("smpl_heads_backward", P, V, Vpad, nnz));
    hipStream_t st = (hipStream_t)stream;
    // the maps are zero-filled whatever follows: persons add at their pixels
    if ((grad_pose_map && B > 0 && HW > 0 && hipMemsetAsync(grad_pose_map, 0, (size_t)4 * B * 72 * HW, st) != hipSuccess) ||
        (grad_shape_map && B > 0 && HW > 0 && hipMemsetAsync(grad_shape_map, 0, (size_t)4 * B * SMPL_NB * HW, st) != hipSuccess))
        H3D_FAIL(H3D_ERR_LAUNCH, "smpl_heads_backward: zero fill failed");
    if (P == 0) return H3D_OK;
    if (!pose_map || !shape_map || !inds || !j_template || !j_shapedirs || !parents) H3D_FAIL(H3D_ERR_ARG, "smpl_heads_backward: null pointer");
    const SbWorkspace w = sb_layout(P, Vpad);
    H3D_TRY(sb_check_verts_args("smpl_heads_backward", w, grad_verts, v_template, dirsK3, dirsV3, lbs_idx, lbs_w, workspace, workspace_bytes));
    if ((!grad_verts && !grad_joints) || (!grad_pose_map && !grad_shape_map)) return H3D_OK;
    SmplBwdHeads hs;
    hs.pose_map = pose_map; hs.shape_map = shape_map; hs.inds = inds; hs.n = n; hs.K = K; hs.HW = HW;
    hs.gpose = grad_pose_map; hs.gshape = grad_shape_map;
    return sb_run<true>(nullptr, nullptr, hs, grad_verts, grad_joints, j_template, j_shapedirs, parents, v_template, dirsK3, dirsV3, lbs_idx, lbs_w,
                        nnz, P, V, Vpad, nullptr, nullptr, w, workspace, stream);
}
