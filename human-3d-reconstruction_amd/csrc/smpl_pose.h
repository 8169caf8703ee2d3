// The pose stage of the SMPL kernels, written once: the lane -> (person, joint) mapping, the parameter loads (rows of betas / thetas or
// the detector's head maps), the rest joint, Rodrigues, the local transform and the kinematic chain.  smpl_pose_kernel (smpl.hip) runs
// it with T = float and stores its results; smpl_bwd_pose_kernel (smpl_bwd.hip) runs it with T = double as the forward of its backward,
// so a change of convention (the +1e-8, the joint order, the clamp of inds) reaches both.  The two scalar types differ in one place
// only: how sin, cos and 1 - cos come out of the angle (smpl_trig).
#pragma once
#include "common.h"
#include "smpl_tile.h"      // SMPL_J / SMPL_NB

// One lane per (person, joint): a wave holds two persons (lanes 32 half + j, j < 24).  Every lane computes on clamped indices (pc, jc);
// only `act` lanes own a (person, joint).
struct SmplLane {
    int j, half, p, pc, jc;
    bool act;
};
__device__ __forceinline__ SmplLane smpl_lane(int P)
{
    SmplLane ln;
    const int l = threadIdx.x;
    ln.j = l & 31; ln.half = l >> 5;
    ln.p = blockIdx.x * 2 + ln.half;
    ln.act = ln.p < P && ln.j < SMPL_J;
    ln.pc = ln.p < P ? ln.p : P - 1; ln.jc = ln.j < SMPL_J ? ln.j : 0;
    return ln;
}

// Parameters read where the network left them: person p is detection q = p % n of image b = p / n, its betas / thetas are the `shape` /
// `pose` head maps [B,10|72,HW] at pixel inds[b*K + q] (clamped into the map)
struct SmplHeadMaps {
    const float *pose_map, *shape_map;
    const int64_t *inds;
    int n, K, HW;
};
struct SmplHeadPix {
    size_t hb = 0;          // image
    int hpix = 0;           // pixel
};
__device__ __forceinline__ SmplHeadPix smpl_head_pix(const SmplHeadMaps &hs, int pc)
{
    SmplHeadPix hp;
    hp.hb = (size_t)(pc / hs.n);
    const int64_t pix = hs.inds[hp.hb * hs.K + (pc - (int)hp.hb * hs.n)];
    hp.hpix = (int)(pix < 0 ? 0 : pix >= hs.HW ? hs.HW - 1 : pix);
    return hp;
}

template <bool HEADS, typename T>
__device__ __forceinline__ void smpl_load_beta(T (&beta)[SMPL_NB], const float *betas, const SmplHeadMaps &hs,
                                               const SmplHeadPix &hp, int pc)
{
#pragma unroll
    for (int k = 0; k < SMPL_NB; ++k) {
        if constexpr (HEADS) beta[k] = hs.shape_map[(hp.hb * SMPL_NB + k) * hs.HW + hp.hpix];
        else beta[k] = betas[(size_t)pc * SMPL_NB + k];
    }
}

template <bool HEADS>
__device__ __forceinline__ void smpl_load_theta(float (&th)[3], const float *thetas, const SmplHeadMaps &hs,
                                                const SmplHeadPix &hp, int pc, int jc)
{
    if constexpr (HEADS) {
        const float *tp = hs.pose_map + (hp.hb * 72 + jc * 3) * hs.HW + hp.hpix;
        th[0] = tp[0]; th[1] = tp[hs.HW]; th[2] = tp[2 * (size_t)hs.HW];
    } else {
        th[0] = thetas[(size_t)pc * 72 + jc * 3]; th[1] = thetas[(size_t)pc * 72 + jc * 3 + 1]; th[2] = thetas[(size_t)pc * 72 + jc * 3 + 2];
    }
}

// rest joint of (p, j): J = j_template + j_shapedirs . beta
template <typename T>
__device__ __forceinline__ void smpl_rest_joint(T (&jr)[3], const float *j_template, const float *j_shapedirs,
                                                const T (&beta)[SMPL_NB], int jc)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        T s = j_template[jc * 3 + c];
#pragma unroll
        for (int k = 0; k < SMPL_NB; ++k) s = fma((T)j_shapedirs[(jc * 3 + c) * SMPL_NB + k], beta[k], s);
        jr[c] = s;
    }
}

// sin a, cos a and 1 - cos a: in fp32 as 1 - cs; in fp64 as 2 sin^2(a / 2), which keeps (1 - cos a) / a^2 free of cancellation near
// the rest pose
__device__ __forceinline__ void smpl_trig(float angle, float &sn, float &cs, float &oc)
{
    sincosf(angle, &sn, &cs);
    oc = 1.f - cs;
}
__device__ __forceinline__ void smpl_trig(double angle, double &sn, double &cs, double &oc)
{
    sn = sin(angle); cs = cos(angle);
    const double sh = sin(0.5 * angle);
    oc = 2.0 * sh * sh;
}

// Rodrigues with the smplx convention: angle = ||theta + 1e-8||, axis = theta / angle; R = I + sin K + (1 - cos) K^2, K = skew(x, y, z).
// Everything the backward differentiates through is handed back.
template <typename T>
struct SmplRot {
    T x, y, z, inv, ex, ey, ez, sn, cs, oc;
    T R[9];
};
template <typename T>
__device__ __forceinline__ SmplRot<T> smpl_rodrigues(T tx, T ty, T tz)
{
    SmplRot<T> r;
    r.ex = tx + T(1e-8); r.ey = ty + T(1e-8); r.ez = tz + T(1e-8);
    const T angle = sqrt(r.ex * r.ex + r.ey * r.ey + r.ez * r.ez);
    r.inv = T(1) / angle;
    r.x = tx * r.inv; r.y = ty * r.inv; r.z = tz * r.inv;
    smpl_trig(angle, r.sn, r.cs, r.oc);
    const T x = r.x, y = r.y, z = r.z, sn = r.sn, oc = r.oc;
    r.R[0] = T(1) + oc * (-(y * y) - z * z);
    r.R[1] = -sn * z + oc * (x * y);
    r.R[2] = sn * y + oc * (x * z);
    r.R[3] = sn * z + oc * (x * y);
    r.R[4] = T(1) + oc * (-(x * x) - z * z);
    r.R[5] = -sn * x + oc * (y * z);
    r.R[6] = -sn * y + oc * (x * z);
    r.R[7] = sn * x + oc * (y * z);
    r.R[8] = T(1) + oc * (-(x * x) - y * y);
    return r;
}

// local transform L = [R | jr - jr(parent)] (root: [R | jr]): rel and G = L, rows [R | t].  `plane` is the parent's lane.
template <typename T>
__device__ __forceinline__ void smpl_local(T (&rel)[3], T (&G)[12], const T (&R)[9], const T (&jr)[3], int par, int plane)
{
    const T px = __shfl(jr[0], plane), py = __shfl(jr[1], plane), pz = __shfl(jr[2], plane);
    rel[0] = par < 0 ? jr[0] : jr[0] - px; rel[1] = par < 0 ? jr[1] : jr[1] - py; rel[2] = par < 0 ? jr[2] : jr[2] - pz;
#pragma unroll
    for (int a = 0; a < 3; ++a) { G[a * 4] = R[a * 3]; G[a * 4 + 1] = R[a * 3 + 1]; G[a * 4 + 2] = R[a * 3 + 2]; G[a * 4 + 3] = rel[a]; }
}

// The kinematic chain: G starts as the local transform and becomes G(parent) . L.  The joints are stored parents-first (SMPL's kintree
// order), so lane j fetches its parent's already global transform by a shuffle at step j -- 23 short steps instead of a 24-joint serial
// program per lane with its 24 x 12 transform table in scratch memory (0.13 ms -> 0.02 ms at 6400 persons).
// The walk must run on a local copy of the caller's array: which product of a sum gets contracted into an fma depends on how the loop
// is vectorised, and only on twelve local values does it come out as it does inside a kernel -- the fp32 bits of A and joints are fixed.
template <typename T>
__device__ __forceinline__ void smpl_chain(T (&Gio)[12], int j, int plane)
{
    T G[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) G[i] = Gio[i];
    for (int step = 1; step < SMPL_J; ++step) {
        T Gp[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) Gp[i] = __shfl(G[i], plane);          // my parent's (already global) transform
        if (j == step) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const T g0 = Gp[a * 4], g1 = Gp[a * 4 + 1], g2 = Gp[a * 4 + 2], g3 = Gp[a * 4 + 3];
                const T l0 = G[0], l1 = G[1], l2 = G[2], l3 = G[3], l4 = G[4], l5 = G[5], l6 = G[6], l7 = G[7], l8 = G[8], l9 = G[9],
                        l10 = G[10], l11 = G[11];
                Gp[a * 4] = g0 * l0 + g1 * l4 + g2 * l8;
                Gp[a * 4 + 1] = g0 * l1 + g1 * l5 + g2 * l9;
                Gp[a * 4 + 2] = g0 * l2 + g1 * l6 + g2 * l10;
                Gp[a * 4 + 3] = g0 * l3 + g1 * l7 + g2 * l11 + g3;
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) G[i] = Gp[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) Gio[i] = G[i];
}
