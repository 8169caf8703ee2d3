// The generation-3 blend-shape contraction of the SMPL stage, shared by the forward (smpl.hip: smpl_verts3_kernel) and the backward
// (smpl_bwd.hip: smpl_bwd_verts_kernel, which recomputes v_posed): tile constants, the LDS-DMA staging of the 2-slot ring, the
// MFMA stream over the three-term bf16 split, and the steps of the skinning rounds after it that both kernels take: accumulator zeroing,
// the lane's vertex record (s3_vertex), the accumulator -> LDS transposition of a round (s3_transpose_round) and the blended transform
// (s3_blend).  The forward's register prefetch of A and each kernel's own outputs stay with the kernels.  The description of the tiling
// is in smpl.hip above smpl_verts3_kernel; the pose stage the two pose kernels share is smpl_pose.h.
#pragma once
#include "common.h"

constexpr int SMPL_J = 24;
constexpr int SMPL_NB = 10;
constexpr int SMPL_PF = 207;

constexpr int S3_KP = 224, S3_NST = S3_KP / 16, S3_VT = 64, S3_NW = 8, S3_PB = 32 * S3_NW;   // 8 waves x 32 persons
constexpr int S3_PPAD = 128;                                  // the hosts pad the person count to this
constexpr int S3_SPR = 7;                                     // 16-byte slots per row and stage: 6 data + 1 pad
constexpr int S3_ROWB = S3_SPR * 16;                          // 112
// slots of a row the DMA fetches: all six (h, m, l: SIX = true) or h and m only -- the lanes of the l slots then carry an out-of-range
// offset (zeros, no traffic)
template <bool SIX> constexpr int s3_dslots() { return SIX ? 6 : 4; }
constexpr int S3_GROW = S3_NST * 96;                          // bytes of a row in global memory: 1344
constexpr int S3_APIECES = 3 * S3_VT * S3_SPR / 64;           // 21 KiB pieces of direction rows
constexpr int S3_BPIECES = S3_PB * S3_SPR / 64;               // 28 of coefficient rows
constexpr int S3_SLOT = (S3_APIECES + S3_BPIECES) * 1024;     // 50176

constexpr int S3_AJ = (S3_APIECES + S3_NW - 1) / S3_NW, S3_BJ = (S3_BPIECES + S3_NW - 1) / S3_NW;   // pieces per wave: 3 + 4
static_assert(S3_APIECES % S3_NW != 0 && S3_BPIECES % S3_NW != 0 && S3_AJ + S3_BJ == 7, "piece counts behind the vmcnt immediates");

// piece j of this wave (0 .. S3_AJ-1 direction rows, then coefficient rows) of stage st -> slot
__device__ __forceinline__ void s3_issue_piece(const char *dirsK, int dbytes, const char *coefK, int cbytes, char *slot,
                                               const int *aoff, const int *boff, int wv, int st, int j)
{
    if (j < S3_AJ) {
        const auto ra = __builtin_amdgcn_make_buffer_rsrc((void *)dirsK, 0, dbytes, 0x00020000);
        const int p = wv + S3_NW * j;
        if (p < S3_APIECES)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void *)(slot + p * 1024), 16, aoff[j], st * 96,
                                                     0, 0);
    } else {
        const auto rb = __builtin_amdgcn_make_buffer_rsrc((void *)coefK, 0, cbytes, 0x00020000);
        const int p = wv + S3_NW * (j - S3_AJ);
        if (p < S3_BPIECES)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (__attribute__((address_space(3))) void *)(slot + (S3_APIECES + p) * 1024), 16,
                                                     boff[j - S3_AJ], st * 96, 0, 0);
    }
}

__device__ __forceinline__ void s3_issue(const char *dirsK, int dbytes, const char *coefK, int cbytes, char *slot,
                                         const int *aoff, const int *boff, int wv, int st)
{
#pragma unroll
    for (int j = 0; j < S3_AJ + S3_BJ; ++j) s3_issue_piece(dirsK, dbytes, coefK, cbytes, slot, aoff, boff, wv, st, j);
}

// per-lane DMA source offsets (stage 0) of this wave's direction pieces for the vertex tile at v0: slot q -> row q / 7, 16-byte
// column q % 7 (6 = pad)
template <bool SIX>
__device__ __forceinline__ void s3_dir_offsets(int *aoff, int wv, int l, int v0, int Vpad)
{
    constexpr int S3_DSLOTS = s3_dslots<SIX>();
#pragma unroll
    for (int j = 0; j < (S3_APIECES + S3_NW - 1) / S3_NW; ++j) {
        const int q = (wv + S3_NW * j) * 64 + l;
        const int row = q / S3_SPR, sub = q - S3_SPR * row;           // row = c * 64 + v
        const int c = row >> 6, v = row & 63;
        aoff[j] = (sub < S3_DSLOTS && row < 3 * S3_VT) ? (c * Vpad + v0 + v) * S3_GROW + sub * 16 : 0x7ffffff0;
    }
}

// the same for the coefficient pieces of the person block at p0
template <bool SIX>
__device__ __forceinline__ void s3_coef_offsets(int *boff, int wv, int l, int p0)
{
    constexpr int S3_DSLOTS = s3_dslots<SIX>();
#pragma unroll
    for (int j = 0; j < (S3_BPIECES + S3_NW - 1) / S3_NW; ++j) {
        const int q = (wv + S3_NW * j) * 64 + l;
        const int row = q / S3_SPR, sub = q - S3_SPR * row;           // row = person inside the workgroup
        boff[j] = (sub < S3_DSLOTS && row < S3_PB) ? (p0 + row) * S3_GROW + sub * 16 : 0x7ffffff0;
    }
}

// The 14 stages of the contraction; stage 0 is already in flight (s3_issue into slot 0).  acc[c][t]: coordinate c, vertex tile t of
// 32, C layout row = vertex, column = person.
// MODE (profiling, ABLATE builds): 0 the contraction, 1 without the MFMAs, 2 without the direction-fragment reads,
// 3 without the DMA after stage 0
template <bool SIX, int MODE>
__device__ __forceinline__ void s3_contract(f32x16 (&acc)[3][2], char *smem, const char *dirsK3, int dbytes, const char *coefK3,
                                            int cbytes, const int *aoff, const int *boff, int wv, int fa_off, int fb_off)
{
    using E = ET<bf16_t>;
    for (int st = 0; st < S3_NST; ++st) {
        __builtin_amdgcn_s_waitcnt(0x0f70);
        __syncthreads();
        if (st + 1 < S3_NST && MODE != 3)
            s3_issue(dirsK3, dbytes, coefK3, cbytes, smem + ((st + 1) & 1) * S3_SLOT, aoff, boff, wv, st + 1);
        const char *sl = smem + (st & 1) * S3_SLOT;
        // SIX: all six products down to 2^-24 relative.  Otherwise hh + hm + mh: the three dropped products (mm, hl, lh) are
        // 2^-16 relative each -- 2.2e-6 abs on the blend-shape displacement (fp64 emulation, |d| <= 0.34), 45x inside the
        // 1e-4 tolerance -- for half the MFMAs and two thirds of the fragment reads
        const E::frag bh = E::lds_frag(sl + fb_off), bm = E::lds_frag(sl + fb_off + 32);
        E::frag bl = bh;
        if constexpr (SIX) bl = E::lds_frag(sl + fb_off + 64);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // the two vertex tiles of a coordinate alternate, so consecutive MFMAs do not share an accumulator
            const char *ap0 = sl + fa_off + (c * 64) * S3_ROWB, *ap1 = ap0 + 32 * S3_ROWB;
            E::frag ah0 = bh, am0 = bm, al0 = bl, ah1 = bh, am1 = bm, al1 = bl;
            if constexpr (MODE != 2) {
                ah0 = E::lds_frag(ap0); am0 = E::lds_frag(ap0 + 32);
                ah1 = E::lds_frag(ap1); am1 = E::lds_frag(ap1 + 32);
                if constexpr (SIX) { al0 = E::lds_frag(ap0 + 64); al1 = E::lds_frag(ap1 + 64); }
            }
            if constexpr (MODE == 1) {
                asm volatile("" ::"v"(ah0.v), "v"(am0.v), "v"(al0.v), "v"(ah1.v), "v"(am1.v), "v"(al1.v), "v"(bh.v), "v"(bm.v), "v"(bl.v));
            } else {
                if constexpr (SIX) {
                    E::mma(acc[c][0], al0, bh);      // smallest terms first
                    E::mma(acc[c][1], al1, bh);
                    E::mma(acc[c][0], ah0, bl);
                    E::mma(acc[c][1], ah1, bl);
                    E::mma(acc[c][0], am0, bm);
                    E::mma(acc[c][1], am1, bm);
                }
                E::mma(acc[c][0], am0, bh);
                E::mma(acc[c][1], am1, bh);
                E::mma(acc[c][0], ah0, bm);
                E::mma(acc[c][1], ah1, bm);
                E::mma(acc[c][0], ah0, bh);
                E::mma(acc[c][1], ah1, bh);
            }
        }
    }
}

// ---- after the contraction: skinning with lane = vertex, in rounds of RP persons per wave ------------------------------------------
__device__ __forceinline__ void s3_zero(f32x16 (&acc)[3][2])
{
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[c][t][i] = 0.f;
}

// this lane's vertex in the skinning phase: (<= 4) joint indices / weights and the template position
struct S3Vertex {
    int jidx[4];
    float jw[4];
    float t0, t1, t2;
};
__device__ __forceinline__ void s3_vertex(S3Vertex &vx, int vc, int nnz, const int32_t *lbs_idx, const float *lbs_w,
                                              const float *v_template, int Vpad)
{
#pragma unroll
    for (int sI = 0; sI < 4; ++sI) {
        vx.jidx[sI] = sI < nnz ? lbs_idx[(size_t)vc * nnz + sI] : 0;
        vx.jw[sI] = sI < nnz ? lbs_w[(size_t)vc * nnz + sI] : 0.f;
    }
    vx.t0 = v_template[vc]; vx.t1 = v_template[Vpad + vc]; vx.t2 = v_template[2 * Vpad + vc];
}

// The accumulators (C layout: row = vertex, column = person; r = lane & 31, h = lane >> 5) of persons [RP rnd, RP rnd + RP) of this wave
// -> sT [RP persons][64 v][3] floats, STRIDE bytes per person: lane = person becomes lane = vertex
template <int RP, int STRIDE>
__device__ __forceinline__ void s3_transpose_round(const f32x16 (&acc)[3][2], char *sT, int rnd, int r, int h)
{
    if ((r / RP) == rnd) {
        const int pl = r % RP;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int vl = t * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    *reinterpret_cast<float *>(sT + pl * STRIDE + (vl * 3 + c) * 4) = acc[c][t][i];
                }
    }
}

// T = sum_s jw[s] A[jidx[s]]: the blended 3x4 transform of the lane's vertex for the person whose 24 transforms are at Aq (LDS)
__device__ __forceinline__ void s3_blend(float (&T)[12], const float *Aq, const S3Vertex &vx)
{
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.f;
#pragma unroll
    for (int sI = 0; sI < 4; ++sI) {
        const float *Ap = Aq + vx.jidx[sI] * 12;
#pragma unroll
        for (int i4 = 0; i4 < 3; ++i4) {
            const f32x4 a4 = *reinterpret_cast<const f32x4 *>(Ap + 4 * i4);
#pragma unroll
            for (int e = 0; e < 4; ++e) T[4 * i4 + e] = fmaf(vx.jw[sI], a4[e], T[4 * i4 + e]);
        }
    }
}

// three-term bf16 split of an fp32 value: x = h + m + l up to 2^-24 relative (round-to-nearest-even at each step)
__device__ __forceinline__ void split3(float x, bf16_t &hh, bf16_t &mm, bf16_t &ll)
{
    hh = ET<bf16_t>::from_f32(x);
    const float r1 = x - ET<bf16_t>::to_f32(hh);
    mm = ET<bf16_t>::from_f32(r1);
    const float r2 = r1 - ET<bf16_t>::to_f32(mm);
    ll = ET<bf16_t>::from_f32(r2);
}
