// Fused output heads of DLASeg (reference models/model.py:451-460, 485-489):
//     for head in heads:  z[head] = Conv1x1(head_conv -> C_head)( ReLU( Conv3x3(64 -> head_conv)(y) ) )
// The reference runs 2 cuDNN convs per head, re-reading y for every head and round-tripping the
// head_conv(=256)-channel intermediate (16.8 MB/image in fp32) through memory for each of them:
// 37 % of the network's multiply-accumulates and the largest single source of HBM traffic.
//
// Here ONE workgroup (8 waves) keeps the 64-channel input halo tile of a TH x 32 pixel tile in LDS
// for ALL heads of the launch and never writes the intermediate: each 64-channel slab of it leaves
// the MFMA accumulators as bf16 (bias + ReLU applied) and is fed straight back as the B operand of
// the 1x1 contraction (accumulator tile -> next MFMA's operand: the 32x32 C/D map puts the pixel on
// the lane and channels in the registers, exactly the B-operand shape; the K order is the
// accumulator row order, which the host bakes into the packed 1x1 weights).
//
// Weight pipeline: the 3x3 filters stream through a 2-slot LDS ring one tap ROW (3 taps, 24 KB) per
// stage by LDS-DMA (buffer_load_dwordx4 ... lds: no staging registers, no ds_write pass), issued one
// stage (48 MFMAs per wave) ahead; one barrier per stage.  The ring rows are unpadded (an LDS-DMA
// wave-instruction writes 1 KB contiguously) and XOR-swizzled through the per-lane SOURCE address
// so the A-fragment ds_read_b128 stay conflict-free.  The 1x1 slice of a slab arrives the same way.
// Outputs are written as contiguous NCHW fp32 rows (lane = pixel), the reference's head layout.
#include "common.h"
#include <string.h>
#include <type_traits>
#include <utility>

constexpr int HEADS_MAX = 16;
constexpr int HC_IN = 64;     // channels of y (DLA-34 first_level = 2)
constexpr int HC_SLAB = 64;   // intermediate channels per slab (two 32-row MFMA tiles)
constexpr int HC_MT2 = 3;     // up to 96 output channels per head
constexpr int HEADS_LISTS_MAX = 4;   // position lists of one sparse launch (h3d_heads_sparse_lists)
#ifndef HEADS_PF_WIDE
#define HEADS_PF_WIDE 0 // the same pipeline in the 2- and 3-tile bodies (wide heads)
#endif
#ifndef HEADS_PF
#define HEADS_PF 2      // measured 0: 1.363, 1: 1.348, 2: 1.335, 3: 1.343 ms (batch 64, the narrow-heads launch)
#endif

#ifndef HEADS_SPARSE_NW
// (the LDS-patch path only, heads_kernel<SPARSE> behind H3D_TUNE_HEADS_SPARSE_LDS_PATCH; in the default heads_sparse_kernel every wave computes)
#define HEADS_SPARSE_NW 8 // waves of a sparse workgroup, two of which compute: the 24 LDS-DMA instructions of a filter stage are spread over all of them.
#endif                    // Measured (batch 64, K = 100: 100 six-head + 1700 one-head workgroups in one launch): 4: 217.7, 8: 171.0 us
static_assert(HEADS_SPARSE_NW == 4 || HEADS_SPARSE_NW == 8, "sparse heads: 24 wave-instructions per stage in whole numbers per wave, at most 512 threads");
#ifndef HEADS_SPARSE_PF
#define HEADS_SPARSE_PF 2 // heads_sparse_kernel: steps of filter fragments requested ahead of the MFMAs (HEADS_PF of the dense narrow heads)
#endif

struct HeadsArgs {
    const char *in;      // NHWC T feature map
    const char *w1;      // [nheads*head_conv][9][64] T
    const float *b1;     // [nheads*head_conv]
    const char *w2[HEADS_MAX];   // per head: [96 rows][head_conv] T, K in accumulator-row order
    const float *b2[HEADS_MAX];  // per head: fp32 [96]
    float *out[HEADS_MAX];       // per head: NCHW fp32 [B,C,H,W]
    int C[HEADS_MAX];
    int nheads, head_conv;
    int B, H, W, in_cs;
    int tiles_x, tiles_y;
    int dbg;   // profiling ablation (h3d_op.reserved & H3D_TUNE_HEADS_ABLATE_MASK): 1 = skip the weight loads after the prologue
    int xcd;   // h3d_tile_id mode
    float s1;                // f16x3 plans: 2^-wexp of the 3x3 filters AND of b1 (h3d_heads_desc.wexp); 1 otherwise
    float s2[HEADS_MAX];     // ... 2^-wexp2 of a head's 1x1 filters
    unsigned long long *stamps;   // profiling builds: per workgroup {kernel start, end, cycles wave 0 spent in the stage barriers, in gemm2, waiting for its own DMA pieces}
    // sparse launches (h3d_heads_sparse_lists): position lists in launch order.  List i owns the workgroups [l_wg0[i], l_wg0[i + 1]) and
    // evaluates the l_nh[i] heads l_head[i][0..) of the op's descriptor, in that order, at l_inds[i]
    int nlists;
    const long long *l_inds[HEADS_LISTS_MAX];   // [B*K] flat output positions y*W + x, image = entry / K
    int l_K[HEADS_LISTS_MAX], l_wg0[HEADS_LISTS_MAX], l_nh[HEADS_LISTS_MAX];
    int l_ng[HEADS_LISTS_MAX];   // heads_sparse_kernel: workgroups (groups of positions) per head of the list, see there
    int l_head[HEADS_LISTS_MAX][HEADS_MAX];
};

// What the dense tile (HeadsCfg) and both sparse layouts (HeadsSparseCfg, HeadsSparseRegCfg) share: filter ring, 1x1 slice, bias pairs, pixel stride
template <typename T>
struct HeadsRingCfg {
    static constexpr int ES = sizeof(T);
    static constexpr int SB = HC_IN * ES + 16;        // halo pixel stride (padded: register-staged once)
    static constexpr int RBW = HC_IN * ES;            // weight row bytes (64 K elements), UNPADDED: LDS-DMA image
    static constexpr int CPR = RBW / 16;              // 16-byte chunks per weight row (8 bf16 / 16 f32)
    static constexpr int SWZ_SHIFT = ES == 2 ? 1 : 0; // chunk' = chunk ^ ((row >> SWZ_SHIFT) & (CPR-1))
    static constexpr int TAPS = ES == 2 ? 3 : 1;      // taps per stage (f32: LDS only fits one)
    static constexpr int TRS = 9 / TAPS;              // stages per slab
    static constexpr int SLOT = TAPS * HC_SLAB * RBW; // ring slot bytes
    static constexpr int LDS_W2 = 32 * HC_MT2 * RBW;  // 96 rows
    static constexpr int LDS_BIAS = 1024 + 1024;      // per head: b1 (<= 256 floats) + b2 (96 floats; its DMA piece writes a whole KiB), two heads in flight
    static constexpr int RPI = 1024 / RBW;            // weight rows per LDS-DMA wave-instruction
    static constexpr int VPR = HC_IN * ES / 16;       // 16-byte vectors per halo pixel
};

template <typename T, int TH>
struct HeadsCfg : HeadsRingCfg<T> {
    using R = HeadsRingCfg<T>;
    static constexpr int TW = 32;
    static constexpr int NT = TH / 8;                 // N-tiles (rows of 32 pixels) per wave, 8 waves
    static constexpr int NW = 8;                      // waves of the workgroup
    static constexpr int IN_H = TH + 2, IN_W = TW + 2;
    static constexpr int RB = IN_W * R::SB;           // halo row stride
    static constexpr int LDS_IN = IN_H * RB;
    static constexpr int LDS = LDS_IN + 2 * R::SLOT + R::LDS_W2 + 2 * R::LDS_BIAS;
};

// Sparse launches (h3d_heads_sparse_lists): the heads at LISTS of output positions instead of a tile; a workgroup's positions come from
// one list and it runs that list's heads only.  A computing wave owns 32 positions,
// the 32 columns of ONE N-tile (a column of an MFMA result depends on that column's B operand only, so a position's value
// does not depend on what the other columns hold); each position has its own 3x3 x 64-channel neighbourhood in LDS, laid out as
// a 3-pixel-wide image of the dense kernel's pixel stride: tap (dy, dx) sits at dy * RB + dx * SB as in the halo tile, and the
// stage code, gemm2 and the epilogue are the dense kernel's at NT = 1.  The other waves only help with the LDS-DMA of the
// filters (an LDS-DMA instruction costs its wave 100-185 issue cycles; a stage is 24 MFMAs per computing wave here).
template <typename T>
struct HeadsSparseCfg : HeadsRingCfg<T> {
    using D = HeadsRingCfg<T>;
    static_assert(sizeof(T) == 2, "sparse heads: 2-byte plans");
    static constexpr int NT = 1, TW = 32;
    static constexpr int CW = 2, NW = HEADS_SPARSE_NW;   // computing waves | waves of the workgroup
    static constexpr int NPOS = 32 * CW;              // positions per workgroup
    static constexpr int RB = 3 * D::SB, PB = 3 * RB; // patch row | patch (position) stride
    static constexpr int LDS_IN = NPOS * PB;
    static constexpr int LDS = LDS_IN + 2 * D::SLOT + D::LDS_W2 + 2 * D::LDS_BIAS;
    static_assert(LDS <= 160 * 1024, "LDS of a CU");
};

// 16-byte LDS read the compiler's wait-count pass does not see (see stage_pipelined): the caller waits.
template <int OFF>
__device__ __forceinline__ void lds_read16_async(u32x4 &dst, uint32_t addr)
{
    static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// (one tile: with the loops over a kernel's tiles in here too, hipcc allocates the dense kernels' registers differently)
__device__ __forceinline__ void zero_tile(f32x16 &t)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = 0.f;
}

// Sparse launches: the list that owns workgroup `bid` (the lists start on workgroup boundaries, HeadsArgs::l_wg0) and the
// workgroup's index among that list's workgroups ...
struct HeadsList { int li, lb, ng, K; const long long *inds; };   // (ng: heads_sparse_kernel's workgroups per head, HeadsArgs::l_ng)
__device__ __forceinline__ HeadsList heads_list_of(const HeadsArgs &a, int bid)
{
    int li = 0;
#pragma unroll
    for (int i = 1; i < HEADS_LISTS_MAX; ++i)
        if (i < a.nlists && bid >= a.l_wg0[i]) li = i;
    return {li, bid - a.l_wg0[li], a.l_ng[li], a.l_K[li], a.l_inds[li]};
}
// ... and entry p of the list as a position of the maps; an entry past the list or outside the map is not `ok`: it stores nothing
struct HeadsPos { bool ok; int b, y, x; };
__device__ __forceinline__ HeadsPos heads_position(const HeadsArgs &a, const HeadsList &ls, int p)
{
    HeadsPos q = {false, 0, 0, 0};
    if (p < a.B * ls.K) {
        const long long ind = ls.inds[p];
        if (ind >= 0 && ind < (long long)a.H * a.W) { q.ok = true; q.b = p / ls.K; q.y = (int)ind / a.W; q.x = (int)ind - q.y * a.W; }
    }
    return q;
}

// Biases of one head -> LDS by LDS-DMA (wave 0: b1[head_conv] <= 1 KiB, wave 1: b2[96]); lanes past the end of either
// array carry offsets outside the buffer and write zeros.  Reading them from global memory where they are used put
// a full memory round trip at the end of every slab and before every group of output stores.
__device__ __forceinline__ void heads_issue_bias(const float *b1, int hc, const float *b2, char *dst, int wv, int l)
{
    if (wv == 0) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)b1, 0, hc * 4, 0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)dst, 16, l * 16, 0, 0, 0);
    } else if (wv == 1) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)b2, 0, 96 * 4, 0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(dst + 1024), 16, l * 16 < 512 ? l * 16 : 0x7ffffff0, 0, 0, 0);
    }
}

// Second contraction of a head: acc2[m2] += W2[rows of tile m2][slab K] . ReLU(acc + b1), then acc = 0.
// The accumulator registers 8s..8s+7 of a 32x32 tile are K-step s of the B operand (lane = pixel);
// the matching A fragment (K in accumulator-row order) sits at K offset m*32 + h*16 + s*8 of the
// host-permuted W2 row (swizzled LDS image, see HeadsCfg).
// BIASC: the accumulators were STARTED at b1 (C operand of the slab's first MFMA, see heads_kernel), so the slab leaves
// them as conv + bias and nothing is added or zeroed here; on bf16 the ReLU runs on the packed pairs (v_pk_max_i16
// against 0: a negative bf16 is a negative int16, and rounding never changes the sign).  That is 64 vector
// instructions per slab and wave instead of 224 -- all eight waves do this at the same time, right after a barrier,
// with the MFMA pipe idle.
template <typename T, int TH, int NT, int M2, bool BIASC>
__device__ __forceinline__ void gemm2(f32x16 (&acc)[2][NT], f32x16 (&acc2)[M2][NT], const char *s_b1 /* LDS: this slab's 64 b1 */,
                                      const char *s_w2, int r, int h, int sw, float s1 = 1.f)
{
    using C = HeadsCfg<T, TH>;
    using E = ET<T>;
    constexpr int ES = sizeof(T);
    typedef short s16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            typename E::frag fb[NT];
            // accumulator registers 8sb..8sb+7 hold channels m*32 + 16sb + 4h + {0..3} and + 8 + {0..3}
            float bias[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if constexpr (!BIASC) {
                const f32x4 b_lo = *reinterpret_cast<const f32x4 *>(s_b1 + (m * 32 + 16 * sb + 4 * h) * 4);
                const f32x4 b_hi = *reinterpret_cast<const f32x4 *>(s_b1 + (m * 32 + 16 * sb + 4 * h + 8) * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { bias[j] = b_lo[j]; bias[4 + j] = b_hi[j]; }
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                float x[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if constexpr (BIASC) {
                        x[j] = acc[m][n][8 * sb + j];
                    } else {
                        x[j] = fmaxf(acc[m][n][8 * sb + j] + bias[j], 0.f);
                        acc[m][n][8 * sb + j] = 0.f;
                    }
                }
                if constexpr (ES == 4) {
                    if constexpr (BIASC) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) x[j] = fmaxf(x[j], 0.f);
                    }
                    if constexpr (std::is_same_v<T, x3_t>) {
                        // f16x3: the fp32 slab values, unscaled (the 3x3 filters and b1 were packed times 2^wexp), split into (hi | lo) fp16 terms
#pragma unroll
                        for (int j = 0; j < 8; ++j) x[j] *= s1;
                        fb[n] = E::split8(x);
                    } else {
                        fb[n].lo = f32x4{x[0], x[1], x[2], x[3]};
                        fb[n].hi = f32x4{x[4], x[5], x[6], x[7]};
                    }
                } else {
                    if constexpr (std::is_same_v<T, f16_t>) {       // fp16: ReLU and the saturation at 65504 in one v_med3_f32 each
#pragma unroll
                        for (int j = 0; j < 8; ++j) x[j] = __builtin_amdgcn_fmed3f(x[j], 0.f, 65504.f);
                    }
                    uint32_t pk[4] = {EP<T>::pack2(x[0], x[1]), EP<T>::pack2(x[2], x[3]), EP<T>::pack2(x[4], x[5]), EP<T>::pack2(x[6], x[7])};
                    if constexpr (BIASC && !std::is_same_v<T, f16_t>) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            pk[j] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, pk[j]), s16x2{0, 0}));
                    }
                    fb[n].v = u32x4{pk[0], pk[1], pk[2], pk[3]};
                }
            }
            const int c = (m * 32 + h * 16 + sb * 8) * ES / 16;        // first 16-byte chunk of this K run
#pragma unroll
            for (int m2 = 0; m2 < M2; ++m2) {
                const char *row = s_w2 + (m2 * 32 + r) * C::RBW;
                const typename E::frag fa = E::lds_frag2(row + ((c ^ sw) << 4), row + (((c + 1) ^ sw) << 4));
#pragma unroll
                for (int n = 0; n < NT; ++n) E::mma(acc2[m2][n], fa, fb[n]);
            }
        }
    }
}

// The bias tile of accumulator tile m of a slab goes from LDS (s_b1: the head's b1) straight INTO the accumulators (accumulator
// row = channel).  Round 3 built it in 32 registers first and copied it into each N-tile: those 32 registers were live together
// with the fragment pipeline and pushed the 3-tile body into scratch (256 VGPRs + 24-36 bytes spilled)
__device__ __forceinline__ void load_bias(f32x16 &dst, const char *s_b1, int slab, int m, int h)
{
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(s_b1 + (slab * HC_SLAB + m * 32 + 8 * g + 4 * h) * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[4 * g + i] = bv[i];
    }
}

// One tap-row stage of the 2-byte kernels as an explicit software pipeline (bf16, narrow heads: the 3-tile instantiation spills
// with it, in the 2-tile one it measures the same as the compiler's schedule: 0.279 / 0.287 vs 0.280 ms at depth 2 / 1).  The
// fragments of step i+1 (a step = one tap x 16 channels: 2 filter + NT pixel fragments feeding 2*NT MFMAs) are requested BEFORE
// the MFMAs of step i and waited for with a counted s_waitcnt.  Left to itself hipcc issues every ds_read right in front of its
// MFMA behind lgkmcnt(0) -- and does so even when the loads are hoisted in the source -- so the reads are inline asm (invisible
// to its wait-count pass) and the waits are ours: LDS returns in order, the NT + 2 reads (2 with B in registers) of each of the
// PF newer steps may stay in flight.  sched_barrier pins the MFMAs behind their wait.
// B: where the pixel fragments come from.  A uint32_t is the LDS address of this lane's fragment of tap 0, K-group 0, N-tile 0 in
// an image of row stride C::RB and pixel stride C::SB (the halo tile, the patches of heads_kernel<SPARSE>): NT more reads per
// step.  Otherwise b is an array of fragments in registers (heads_sparse_kernel, NT = 1) and step i multiplies b[BOFF + i].
// FIRST: the slab's first MFMA of every accumulator tile takes its C operand from the bias tile.
template <typename T, class C, int NT, int PF, bool FIRST, int BOFF = 0, class B>
__device__ __forceinline__ void stage_pipelined(f32x16 (&acc)[2][NT], const char *slot, const B &b, const char *s_b1, int slab, int r, int h, int sw)
{
    using E = ET<T>;
    constexpr bool B_LDS = std::is_same_v<B, uint32_t>;
    static_assert(B_LDS || NT == 1, "fragments in registers: one N-tile");
    constexpr int NSTEP = C::TAPS * (HC_IN / 16), NBUF = PF + 1;   // steps of the stage | fragment sets: PF steps in flight ahead of the MFMAs
    constexpr int NRD = 2 + (B_LDS ? NT : 0);                      // LDS reads of a step
    static_assert(PF * NRD <= 15, "lgkmcnt field");
    const uint32_t ring = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char *)slot + r * C::RBW;
    uint32_t fa_base[HC_IN / 16];
#pragma unroll
    for (int kk = 0; kk < HC_IN / 16; ++kk) fa_base[kk] = ring + (((2 * kk + h) ^ sw) << 4);
    u32x4 fa[NBUF][2], fb[B_LDS ? NBUF : 1][NT];
    auto fetch = [&](auto step_tag) {
        constexpr int STEP = decltype(step_tag)::value, BUF = STEP % NBUF;
        constexpr int tp = STEP / (HC_IN / 16), kk = STEP - tp * (HC_IN / 16);
        lds_read16_async<(tp * HC_SLAB) * C::RBW>(fa[BUF][0], fa_base[kk]);
        lds_read16_async<(tp * HC_SLAB + 32) * C::RBW>(fa[BUF][1], fa_base[kk]);
        if constexpr (B_LDS) {
            static_for<NT>([&](auto n_tag) {
                constexpr int n = decltype(n_tag)::value;
                lds_read16_async<n * C::RB + tp * C::SB + kk * 32>(fb[BUF][n], b);
            });
        }
    };
    static_for<PF>([&](auto step_tag) { fetch(step_tag); });
    static_for<NSTEP>([&](auto step_tag) {
        constexpr int STEP = decltype(step_tag)::value, BUF = STEP % NBUF;
        if constexpr (STEP + PF < NSTEP) fetch(std::integral_constant<int, STEP + PF>{});
        constexpr int NEWER = (STEP + PF < NSTEP ? PF : NSTEP - 1 - STEP) * NRD;        // reads issued after step STEP's
        __builtin_amdgcn_s_waitcnt(0xc07f | (NEWER << 8));                              // lgkmcnt(NEWER)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                if (FIRST && STEP == 0) { load_bias(acc[m][n], s_b1, slab, m, h); }
                typename E::frag a_, b_;
                a_.v = fa[BUF][m];
                if constexpr (B_LDS) b_.v = fb[BUF][n];
                else b_.v = b[BOFF + STEP];
                E::mma(acc[m][n], a_, b_);
            }
        __builtin_amdgcn_sched_barrier(0);
    });
}

// LDS-DMA of one weight stage / one 1x1 slice in the BUFFER form: per-lane 32-bit offsets that do not depend on the stage
// (row, tap and swizzled chunk of the lane's 16 bytes) + a scalar stage offset, instead of a 64-bit per-lane address rebuilt
// for every piece (global_load_lds): an LDS-DMA instruction costs its wave 100-185 issue cycles as it is, and the address
// arithmetic in front of each of the 3 + 2 pieces per wave and stage came on top (the weight stream was 10 % of the kernel:
// ablation in DESIGN.md 2.3).  Plain functions of plain arguments: a lambda capturing a buffer descriptor drops the host stub.
template <typename T, int TH, int NW = 8>
__device__ __forceinline__ void heads_dma_w1(const char *w1, int w1_bytes, char *slot, int wv, int l, int soff)
{
    using C = HeadsCfg<T, TH>;
    constexpr int ES = sizeof(T);
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)w1, 0, w1_bytes, 0x00020000);
    constexpr int NI = C::TAPS * HC_SLAB / C::RPI;          // wave-instructions per stage (24 / 16)
    static_assert(NI % NW == 0, "whole wave-instructions per wave");
#pragma unroll
    for (int j = 0; j < NI / NW; ++j) {
        const int g = j * NW + wv;                           // 1 KB run index
        const int row_all = g * C::RPI + l / C::CPR;         // = tap_in_stage * 64 + row
        const int tp = row_all / HC_SLAB, row = row_all - tp * HC_SLAB;
        const int c = (l % C::CPR) ^ ((row >> C::SWZ_SHIFT) & (C::CPR - 1));
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(slot + g * 1024), 16,
                                                 ((row * 9 + tp) * HC_IN) * ES + c * 16, soff, 0, 0);
    }
}
template <typename T, int TH, int NW = 8>
__device__ __forceinline__ void heads_dma_w2(const char *w2, int head_conv, char *s_w2, int wv, int l, int soff)
{
    using C = HeadsCfg<T, TH>;
    constexpr int ES = sizeof(T);
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)w2, 0, 32 * HC_MT2 * head_conv * ES, 0x00020000);
    constexpr int NI = 32 * HC_MT2 / C::RPI;                 // 12 / 24 wave-instructions
#pragma unroll
    for (int j = 0; j < (NI + NW - 1) / NW; ++j) {
        const int g = j * NW + wv;
        if (g < NI) {
            const int row = g * C::RPI + l / C::CPR;
            const int c = (l % C::CPR) ^ ((row >> C::SWZ_SHIFT) & (C::CPR - 1));
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(s_w2 + g * 1024), 16,
                                                     row * head_conv * ES + c * 16, soff, 0, 0);
        }
    }
}

// Profiling build (make ABLATE=1, tools/stamp_heads.py): where heads_kernel's cycles go, per workgroup.  begin() ... end_x() brackets
// one phase of the stage loop; every member is empty in the production build.
struct HeadsTimers {
#ifdef H3D_ABLATE
    static __device__ __forceinline__ unsigned long long now() { return __builtin_readcyclecounter(); }
    unsigned long long t_bar = 0, t_g2 = 0, t_dma = 0, t_stage = 0, t0 = 0;
    const unsigned long long t_start = now();
    __device__ __forceinline__ void begin() { t0 = now(); }
    __device__ __forceinline__ void end_stage()   // + the wave's own DMA pieces of the next stage, to tell DMA wait from barrier wait
    {
        t_stage += now() - t0;
        t0 = now();
        __builtin_amdgcn_s_waitcnt(0x0f70);
        const unsigned long long t1 = now();
        t_dma += t1 - t0;
        t0 = t1;
    }
    __device__ __forceinline__ void end_barrier() { t_bar += now() - t0; }
    __device__ __forceinline__ void end_gemm2() { t_g2 += now() - t0; }
    // stamps of the workgroup: {kernel start, end, cycles wave 0 spent in the stage barriers, in gemm2, waiting for its own DMA pieces, in the stages}
    __device__ __forceinline__ void store(const HeadsArgs &a, int tid, int wv, int l) const
    {
        if (!a.stamps || blockIdx.x >= 65536) return;
        unsigned long long *st = a.stamps + blockIdx.x * H3D_NSTAMP;
        if (a.dbg & 64) {                       // per-wave barrier time instead (tools/stamp_heads.py --waves)
            if (l == 0) st[wv] = t_bar;
        } else if (tid == 0) {
            st[0] = t_start; st[1] = now(); st[2] = t_bar; st[3] = t_g2; st[4] = t_dma; st[5] = t_stage;
        }
    }
#else
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void end_stage() {}
    __device__ __forceinline__ void end_barrier() {}
    __device__ __forceinline__ void end_gemm2() {}
    __device__ __forceinline__ void store(const HeadsArgs &, int, int, int) const {}
#endif
};

// SPARSE: the workgroup's "tile" is 32 * CW entries of ONE of the position lists (HeadsSparseCfg); everything per position -- operands,
// the order of every accumulator's MFMA chain, the epilogue -- is the dense code, so the value is the dense launch's bit for bit.
template <typename T, int TH, int M2, bool BIASC, bool MIXED = false, bool SPARSE = false>
__global__ __launch_bounds__(512) void heads_kernel(HeadsArgs a)
{
    using C = std::conditional_t<SPARSE, HeadsSparseCfg<T>, HeadsCfg<T, TH>>;
    using E = ET<T>;
    constexpr int ES = C::ES;
    constexpr int NT = C::NT;
    __shared__ __attribute__((aligned(16))) char smem[C::LDS];
    char *s_in = smem;
    char *s_ring = smem + C::LDS_IN;
    char *s_w2 = s_ring + 2 * C::SLOT;
    char *s_bias = s_w2 + C::LDS_W2;

    const int tid = threadIdx.x;
    const int wv = tid >> 6, l = tid & 63, r = l & 31, h = l >> 5;
    const int tiles = a.tiles_x * a.tiles_y;
    const int bid = SPARSE ? (int)blockIdx.x : h3d_tile_id(blockIdx.x, gridDim.x, a.xcd);
    const int b = bid / tiles;
    const int t = bid - b * tiles;
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int oy0 = ty * TH, ox0 = tx * C::TW;
    const int slabs = a.head_conv / HC_SLAB;
    // sparse: this workgroup's list (they start on workgroup boundaries), its index among the list's workgroups, the list's heads
    // (heads_list_of and, below, heads_position of this lane, written out: called here they move the register allocation of this
    // instantiation by one or two VGPRs; the patch staging and heads_sparse_kernel call them)
    [[maybe_unused]] int li = 0;
    if constexpr (SPARSE) {
#pragma unroll
        for (int i = 1; i < HEADS_LISTS_MAX; ++i)
            if (i < a.nlists && bid >= a.l_wg0[i]) li = i;
    }
    [[maybe_unused]] const HeadsList ls = {li, SPARSE ? bid - a.l_wg0[li] : 0, 0, SPARSE ? a.l_K[li] : 0, SPARSE ? a.l_inds[li] : nullptr};
    const int nh = SPARSE ? a.l_nh[li] : a.nheads;      // heads this workgroup runs: the hi-th one is head_at(hi) of the descriptor
    auto head_at = [&](int hi) -> int {
        if constexpr (SPARSE) return a.l_head[li][hi];
        else return hi;
    };
    const int nstages = nh * slabs * C::TRS;             // tap-row stages of the workgroup
    const int sw = (r >> C::SWZ_SHIFT) & (C::CPR - 1);   // XOR swizzle of this lane's A-fragment rows

    // ---- LDS-DMA of stage s: TAPS taps x 64 rows of W1 for (head, slab) -> ring slot s & 1 -----------
    // lane i of a wave-instruction lands at byte i*16 of a 1 KB run = RPI rows; it fetches source
    // chunk (i % CPR) ^ swz(row) so that LDS position p of a row holds chunk p ^ swz(row).
    const int wvs = __builtin_amdgcn_readfirstlane(wv);
    const int w1_bytes = a.nheads * a.head_conv * 9 * HC_IN * ES;
    auto issue_w1 = [&](int s) {
        if ((H3D_DBG(a) & 1) && s > 0) return;
        int hs = s / C::TRS;                                    // hs = head * slabs + slab
        const int tr = s - hs * C::TRS;
        if constexpr (SPARSE) { const int hi = hs / slabs; hs += (head_at(hi) - hi) * slabs; }
        heads_dma_w1<T, TH, C::NW>(a.w1, w1_bytes, s_ring + (s & 1) * C::SLOT, wvs, l, ((hs * HC_SLAB * 9 + tr * C::TAPS) * HC_IN) * ES);
    };
    // ---- LDS-DMA of the 1x1 slice [96 rows][64 K of this slab] -> s_w2 --------------------------------
    auto issue_w2 = [&](int head, int slab) {
        if (H3D_DBG(a) & 1) return;
        heads_dma_w2<T, TH, C::NW>(a.w2[head], a.head_conv, s_w2, wvs, l, slab * HC_SLAB * ES);
    };

    // ---- prologue: stage 0 weights in flight, halo tile (all 64 channels, zero outside the image) -----
    issue_w1(0);
    heads_issue_bias(a.b1 + head_at(0) * a.head_conv, a.head_conv, a.b2[head_at(0)], s_bias, __builtin_amdgcn_readfirstlane(wv), l);
    // sparse: this lane's position (computing waves; an entry past the list or outside the map stores nothing) and whether the wave computes
    [[maybe_unused]] HeadsPos sp = {false, 0, 0, 0};
    [[maybe_unused]] bool idle = false;
    if constexpr (SPARSE) {
        idle = wvs >= C::CW;
        const int p = ls.lb * C::NPOS + wv * 32 + r;
        if (!idle && p < a.B * ls.K) {
            const long long ind = ls.inds[p];
            if (ind >= 0 && ind < (long long)a.H * a.W) { sp.ok = true; sp.b = p / ls.K; sp.y = (int)ind / a.W; sp.x = (int)ind - sp.y * a.W; }
        }
        // the 3x3 neighbourhood of every position (all 64 channels, zero outside the image, as the dense halo)
        constexpr int NPV = C::NPOS * 9 * C::VPR;
        stage_vectors<NPV, 64 * C::NW>(
            tid,
            [&](int i) -> u32x4 {
                const int v = i % C::VPR, q = i / C::VPR, pix = q % 9;
                const HeadsPos c = heads_position(a, ls, ls.lb * C::NPOS + q / 9);
                if (!c.ok) return u32x4{0u, 0u, 0u, 0u};
                const int gy = c.y - 1 + pix / 3, gx = c.x - 1 + pix % 3;
                if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
                    return *reinterpret_cast<const u32x4 *>(a.in + (((size_t)c.b * a.H * a.W + (size_t)gy * a.W + gx) * a.in_cs) * ES + v * 16);
                return u32x4{0u, 0u, 0u, 0u};
            },
            [&](int i, u32x4 val) {
                const int v = i % C::VPR, q = i / C::VPR;
                *reinterpret_cast<u32x4 *>(s_in + (q / 9) * C::PB + (q % 9) * C::SB + v * 16) = val;
            });
    } else {
        const size_t in_img = (size_t)b * a.H * a.W;
        constexpr int NHV = C::IN_H * C::IN_W * C::VPR;
        constexpr int HALF = (NHV + 1) / 2;                 // two batches bound the staging registers
        for (int part = 0; part < 2; ++part) {
            const int base = part * HALF;
            stage_vectors<HALF, 512>(
                tid,
                [&](int j) -> u32x4 {
                    const int i = base + j;
                    if (i >= NHV) return u32x4{0u, 0u, 0u, 0u};
                    const int v = i % C::VPR, pix = i / C::VPR;
                    const int iy = pix / C::IN_W, ix = pix - iy * C::IN_W;
                    const int gy = oy0 - 1 + iy, gx = ox0 - 1 + ix;
                    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
                        return *reinterpret_cast<const u32x4 *>(a.in + ((in_img + (size_t)gy * a.W + gx) * a.in_cs) * ES + v * 16);
                    return u32x4{0u, 0u, 0u, 0u};
                },
                [&](int j, u32x4 val) {
                    const int i = base + j;
                    if (i < NHV) {
                        const int v = i % C::VPR, pix = i / C::VPR;
                        const int iy = pix / C::IN_W, ix = pix - iy * C::IN_W;
                        if constexpr (std::is_same_v<T, x3_t>) x3_store4(s_in + iy * C::RB + ix * C::SB + (v >> 1) * 32, v & 1, val);
                        else *reinterpret_cast<u32x4 *>(s_in + iy * C::RB + ix * C::SB + v * 16) = val;
                    }
                });
        }
    }
    __syncthreads();   // (emits s_waitcnt vmcnt(0): the LDS-DMA of stage 0 has landed)

    int boff[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        if constexpr (SPARSE) boff[n] = ((idle ? 0 : wv * 32) + r) * C::PB + 8 * h * ES;
        else boff[n] = (wv * NT + n) * C::RB + r * C::SB + 8 * h * ES;
    }

    HeadsTimers tm;
    int s = 0;
    // one head: M2H = 32-row tiles of ITS 1x1 output.  MIXED launches (all heads of the model in one launch, so that the halo
    // tile is staged once per workgroup for all of them) instantiate the body for every width up to M2 and pick per head
    // (hi: the head's place among the heads this workgroup runs, head: its slot in the descriptor; the same number in a dense launch)
    auto head_body = [&](auto m2_tag, int hi, int head) {
        constexpr int M2H = decltype(m2_tag)::value;
        const char *s_b = s_bias + (hi & 1) * C::LDS_BIAS;
        f32x16 acc[2][NT], acc2[M2H][NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
#pragma unroll
            for (int m = 0; m < 2; ++m) zero_tile(acc[m][n]);
#pragma unroll
            for (int m = 0; m < M2H; ++m) zero_tile(acc2[m][n]);
        }
        for (int slab = 0; slab < slabs; ++slab) {
            // one tap-row stage; FIRST: the slab's first MFMA of every accumulator tile takes its C operand from the
            // bias tile (accumulator row = channel), so neither a zeroing pass nor a bias pass exists
            auto stage = [&](auto first_tag, const char *slot, int tr) {
                constexpr bool FIRST = decltype(first_tag)::value;
                auto plain = [&]() {
#pragma unroll
                    for (int tp = 0; tp < C::TAPS; ++tp) {
                        const int tap = tr * C::TAPS + tp;
                        const int dy = tap / 3, dx = tap - dy * 3;
                        const char *br = s_in + dy * C::RB + dx * C::SB;
#pragma unroll
                        for (int kk = 0; kk < HC_IN / 16; ++kk) {
                            const int c = (kk * 16 + 8 * h) * ES / 16;
                            typename E::frag fa[2], fb[NT];
#pragma unroll
                            for (int m = 0; m < 2; ++m) {
                                const char *row = slot + (tp * HC_SLAB + m * 32 + r) * C::RBW;
                                fa[m] = E::lds_frag2(row + ((c ^ sw) << 4), row + (((c + 1) ^ sw) << 4));
                            }
#pragma unroll
                            for (int n = 0; n < NT; ++n) fb[n] = E::lds_frag(br + boff[n] + kk * 16 * ES);
#pragma unroll
                            for (int m = 0; m < 2; ++m)
#pragma unroll
                                for (int n = 0; n < NT; ++n) {
                                    if (FIRST && tp == 0 && kk == 0) { load_bias(acc[m][n], s_b, slab, m, h); }
                                    E::mma(acc[m][n], fa[m], fb[n]);
                                }
                        }
                    }
                };
                // (two levels: inside this generic lambda only a condition that does not depend on M2H keeps the fp32
                // instantiation from type-checking the 2-byte fragment code)
                if constexpr (ES == 2) {
                if constexpr ((M2H == 1 && HEADS_PF > 0) || (M2H > 1 && HEADS_PF_WIDE > 0)) {
                    const uint32_t fb_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char *)s_in + boff[0] + tr * C::RB;
                    stage_pipelined<T, C, NT, (M2H == 1 ? HEADS_PF : HEADS_PF_WIDE), FIRST>(acc, slot, fb_base, s_b, slab, r, h, sw);
                } else {
                    plain();
                }
                } else if constexpr (std::is_same_v<T, x3_t>) {
                    // (a third ring slot for the one-tile heads -- the 64 rows of the 1x1 slice they never read pay for it --, filters two
                    //  stages ahead behind counted vmcnt waits: 4.364 -> 4.381 ms, tools/ab_lib.py; the one-tap stages do not wait for their DMA)
                    // f16x3: one tap x 64 channels per stage = 4 steps of (2 filter + NT pixel fragments, 32 bytes each) feeding 6 NT
                    // MFMAs.  Two fragment sets, step k+1 read while step k multiplies (the compiler's own schedule: two 16-byte reads,
                    // lgkmcnt(0), three MFMAs); the fragments are plain loads here, the order is pinned by sched_group_barrier
                    const int dy = tr / 3, dx = tr - dy * 3;
                    const char *br = s_in + dy * C::RB + dx * C::SB;
                    typename E::frag fa[2][2], fb[2][NT];
                    auto rd = [&](int kk, int q) {
                        const int c = (kk * 16 + 8 * h) * ES / 16;
#pragma unroll
                        for (int m = 0; m < 2; ++m) {
                            const char *row = slot + (m * 32 + r) * C::RBW;
                            fa[q][m] = E::lds_frag2(row + ((c ^ sw) << 4), row + (((c + 1) ^ sw) << 4));
                        }
#pragma unroll
                        for (int n = 0; n < NT; ++n) fb[q][n] = E::lds_frag(br + boff[n] + kk * 16 * ES);
                    };
                    constexpr int NRD = 2 * (2 + NT), NMM = 6 * NT;
                    rd(0, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, NRD, 0);
#pragma unroll
                    for (int kk = 0; kk < HC_IN / 16; ++kk) {
                        if (kk + 1 < HC_IN / 16) rd(kk + 1, (kk + 1) & 1);
#pragma unroll
                        for (int m = 0; m < 2; ++m)
#pragma unroll
                            for (int n = 0; n < NT; ++n) {
                                if (FIRST && kk == 0) { load_bias(acc[m][n], s_b, slab, m, h); }
                                E::mma(acc[m][n], fa[kk & 1][m], fb[kk & 1][n]);
                            }
                        if (kk + 1 < HC_IN / 16) {
#pragma unroll
                            for (int i = 0; i < (NRD < NMM ? NRD : NMM); ++i) {
                                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                            }
                            if (NMM > NRD) __builtin_amdgcn_sched_group_barrier(0x008, NMM - NRD, 0);
                        } else {
                            __builtin_amdgcn_sched_group_barrier(0x008, NMM, 0);
                        }
                    }
                } else {
                    plain();
                }
            };
#pragma unroll 1
            for (int tr = 0; tr < C::TRS; ++tr, ++s) {
                if (s + 1 < nstages) issue_w1(s + 1);          // slot (s+1)&1 was last read in stage s-1
                if (tr == (C::TRS > 1 ? 1 : 0)) issue_w2(head, slab);   // after the barrier that follows the previous gemm2
                if (slab == 0 && tr == C::TRS - 1 && hi + 1 < nh)   // next head's biases: their slot was last read in the
                    heads_issue_bias(a.b1 + head_at(hi + 1) * a.head_conv, a.head_conv, a.b2[head_at(hi + 1)],   // previous head's epilogue, at least one barrier ago
                                     s_bias + ((hi + 1) & 1) * C::LDS_BIAS, __builtin_amdgcn_readfirstlane(wv), l);
                const char *slot = s_ring + (s & 1) * C::SLOT;
                tm.begin();
                if (SPARSE && idle) { /* a wave that only moves filters */ }
                else if ((H3D_DBG(a) & 4) && wv >= 4) { /* profiling: only the older wave of each SIMD computes (timing only) */ }
                else if ((H3D_DBG(a) & 8) && wv < 4) { /* profiling: only the younger wave computes */ }
                else if (BIASC && tr == 0) stage(std::true_type{}, slot, tr);
                else stage(std::false_type{}, slot, tr);
                tm.end_stage();
                if (!(H3D_DBG(a) & 2))   // (profiling: 2 = no stage barrier -- wrong results, timing only)
                __syncthreads();   // vmcnt(0) + barrier: next stage's weights (and the 1x1 slice) have landed
                tm.end_barrier();
            }
            // ---- slab done: X = ReLU(acc [+ b1]) -> B operand; acc2 += W2[:, slab] . X ----------------------
            tm.begin();
            if (!(SPARSE && idle))
            gemm2<T, TH, NT, M2H, BIASC>(acc, acc2, s_b + slab * HC_SLAB * 4, s_w2, r, h, sw, a.s1);
            tm.end_gemm2();
            if (C::TRS == 1) __syncthreads();   // (f32 path) s_w2 is rewritten in the very next stage
        }
        // ---- head done: z = acc2 [* s2] + b2 -> NCHW fp32 (lane = pixel: coalesced rows) -----------------
        const int C_head = a.C[head];
        float *out = a.out[head];
        const size_t cstride = (size_t)a.H * a.W;
        const float s2 = a.s2[head];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int oy = SPARSE ? sp.y : oy0 + wv * NT + n, ox = SPARSE ? sp.x : ox0 + r, ob = SPARSE ? sp.b : b;
            if (SPARSE ? sp.ok : oy < a.H && ox < a.W) {
                float *op = out + (((size_t)ob * C_head + 4 * h) * a.H + oy) * a.W + ox;
#pragma unroll
                for (int m2 = 0; m2 < M2H; ++m2) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c = m2 * 32 + 8 * g + 4 * h;
                        float *p = op + (size_t)(m2 * 32 + 8 * g) * cstride;
                        const f32x4 b2v = *reinterpret_cast<const f32x4 *>(s_b + 1024 + c * 4);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (c + i < C_head) {
                                if constexpr (std::is_same_v<T, x3_t>) p[i * cstride] = fmaf(acc2[m2][n][4 * g + i], s2, b2v[i]);
                                else p[i * cstride] = acc2[m2][n][4 * g + i] + b2v[i];
                            }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        }
        };
    for (int hi = 0; hi < nh; ++hi) {
        const int head = head_at(hi);
        if constexpr (!MIXED) {
            head_body(std::integral_constant<int, M2>{}, hi, head);
        } else {
            const int m2h = __builtin_amdgcn_readfirstlane((a.C[head] + 31) >> 5);
            if (m2h <= 1) head_body(std::integral_constant<int, 1>{}, hi, head);
            else if (M2 < 3 || m2h == 2) head_body(std::integral_constant<int, (M2 < 2 ? 1 : 2)>{}, hi, head);
            else head_body(std::integral_constant<int, M2>{}, hi, head);
        }
    }
    tm.store(a, tid, wv, l);
}

// Sparse launches, the default path: a position's 3x3 x 64-channel neighbourhood lives in the REGISTERS of its lane as the 36 B
// fragments of the 3x3 contraction (9 taps x 4 K-groups of 16 channels; lane (r, h) holds the 16-byte half h of position r), loaded
// once from the feature map by range-checked buffer loads: a tap outside the image, and every tap of an entry that stores nothing,
// carries an offset outside the buffer and reads zeros, as the LDS patch of heads_kernel<SPARSE> holds zeros there.  No patch area
// in LDS, so EVERY wave computes (32 positions each) and a filter stage that streams through the ring serves 32 * NW positions
// instead of 64.  A workgroup is ONE work item = (list, one head of it, one group of 32 * NW positions): l_wg0[] counts items, the
// items of a head are l_ng[list] consecutive workgroups.  The code is heads_kernel's, the same functions: heads_dma_w1 /
// heads_dma_w2 / heads_issue_bias (the filter ring, the swizzle, the buffer-form DMA), stage_pipelined (the software-pipelined
// A-fragment reads; B from the register array), load_bias, zero_tile and gemm2; heads_list_of and heads_position (the workgroup's
// list, the lane's position) are shared with the patch staging of heads_kernel<SPARSE>.  Only the epilogue is a copy (see there).
// The three tap-row stages of a slab are unrolled so that every fragment index is a compile-time constant (a run-time index would
// put the fragments in scratch).  Per position the chain of every accumulator is the dense kernel's -- only where the B operand
// comes from differs -- so the value is the dense launch's bit for bit.
template <typename T, int NW>
struct HeadsSparseRegCfg : HeadsRingCfg<T> {
    using D = HeadsRingCfg<T>;
    static_assert(sizeof(T) == 2, "sparse heads: 2-byte plans");
    static constexpr int NPOS = 32 * NW;              // positions per workgroup: every wave computes
    static_assert(D::TAPS == 3 && D::TRS == 3, "a stage is one tap row");
    static constexpr int NFRAG = 9 * (HC_IN / 16);    // B fragments of a position: 144 VGPRs
    static constexpr int LDS_PARK = NW * HC_MT2 * 16 * 256;    // per wave: the 32-row output tiles of a wide head (16 registers each), see the kernel
    static constexpr int LDS = 2 * D::SLOT + D::LDS_W2 + D::LDS_BIAS + LDS_PARK;   // one head per workgroup: one bias pair
    static_assert(LDS <= 160 * 1024, "LDS of a CU");
    static constexpr unsigned OUTSIDE = 0x80000000u;  // a buffer offset beyond any map this path takes (HEADS_SPARSE_REG_MAX_BYTES)
};
constexpr size_t HEADS_SPARSE_REG_MAX_BYTES = (size_t)1 << 31;   // the fragment loads address the feature map by 32-bit buffer offsets

template <typename T, int NW>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void heads_sparse_kernel(HeadsArgs a)   // (4 waves: one per SIMD, up to 512 registers)
{
    using C = HeadsSparseRegCfg<T, NW>;
    constexpr int ES = C::ES;
    __shared__ __attribute__((aligned(16))) char smem[C::LDS];
    char *s_ring = smem;
    char *s_w2 = s_ring + 2 * C::SLOT;
    char *s_bias = s_w2 + C::LDS_W2;
    char *s_park = s_bias + C::LDS_BIAS;

    const int tid = threadIdx.x;
    const int wv = tid >> 6, l = tid & 63, r = l & 31, h = l >> 5;
    const int wvs = __builtin_amdgcn_readfirstlane(wv);
    // this workgroup's list (they start on workgroup boundaries), its head and its group of positions
    const HeadsList ls = heads_list_of(a, blockIdx.x);
    const int hi = ls.lb / ls.ng, grp = ls.lb - hi * ls.ng;
    const int head = a.l_head[ls.li][hi];
    const int slabs = a.head_conv / HC_SLAB;
    const int nstages = slabs * C::TRS;
    const int sw = (r >> C::SWZ_SHIFT) & (C::CPR - 1);

    const int w1_bytes = a.nheads * a.head_conv * 9 * HC_IN * ES;
    auto issue_w1 = [&](int s) {
        const int slab = s / C::TRS, tr = s - slab * C::TRS;
        heads_dma_w1<T, 16, NW>(a.w1, w1_bytes, s_ring + (s & 1) * C::SLOT, wvs, l, (((head * slabs + slab) * HC_SLAB * 9 + tr * C::TAPS) * HC_IN) * ES);
    };
    issue_w1(0);
    heads_issue_bias(a.b1 + head * a.head_conv, a.head_conv, a.b2[head], s_bias, wvs, l);

    // this lane's position (an entry past the list or outside the map stores nothing) and its 36 fragments
    const HeadsPos sp = heads_position(a, ls, grp * C::NPOS + wv * 32 + r);
    u32x4 bf[C::NFRAG];
    {
        const size_t in_bytes = (((size_t)a.B * a.H * a.W - 1) * a.in_cs + HC_IN) * ES;      // <= HEADS_SPARSE_REG_MAX_BYTES (the launcher)
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)a.in, 0, (int)in_bytes, 0x00020000);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int gy = sp.y - 1 + tap / 3, gx = sp.x - 1 + tap % 3;
            const bool inside = sp.ok && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            const unsigned off = inside ? (unsigned)((((sp.b * a.H + gy) * a.W + gx) * a.in_cs + 8 * h) * ES) : C::OUTSIDE;
#pragma unroll
            for (int kk = 0; kk < HC_IN / 16; ++kk)
                bf[tap * (HC_IN / 16) + kk] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + kk * 16 * ES, 0, 0));
        }
    }
    // The barrier waits for what writes LDS -- the LDS-DMA of stage 0 and the biases, issued BEFORE the 36 fragment loads -- and
    // not for the fragments: hipcc emits s_waitcnt vmcnt(36) here and waits for each fragment in front of the first MFMA that
    // reads it (vmcnt(38) ... vmcnt(27) through the first stage, whose own DMA pieces are younger still).
    __syncthreads();

    auto body = [&](auto m2_tag) {
        constexpr int M2H = decltype(m2_tag)::value;
        // 144 fragment registers + 32 of the slab + the filter fragments in flight leave room for ONE 32-row output tile under the 256
        // registers of two waves per SIMD.  A wide head (M2H > 1) parks its output tiles in LDS between the slabs' second
        // contractions, a wave-private 1 KiB per register (lane-contiguous 16-byte pieces: conflict-free), and runs gemm2 tile by
        // tile: plain fp32 copies, and the chain of every tile is still slab -> m -> sb.  The price: gemm2<..., 1> is called M2H times
        // per slab, so the ReLU + pack of the slab accumulators into B fragments (it does not change acc under BIASC) is redone
        // for every tile, 2 - 3 times the vector work of a gemm2 that builds them once, plus the LDS round trip of the tile.  A
        // gemm2 variant that takes prepared fragments would remove the repeat; not built.
        constexpr bool PARK = M2H > 1;
        char *park = s_park + (wv * HC_MT2 * 16 * 64 + l * 4) * 4;
        auto park_tile = [&](int m2, const f32x16 &t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4 *>(park + (m2 * 4 + q) * 1024) = f32x4{t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]};
        };
        auto parked_tile = [&](int m2, f32x16 &t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(park + (m2 * 4 + q) * 1024);
#pragma unroll
                for (int i = 0; i < 4; ++i) t[4 * q + i] = v[i];
            }
        };
        f32x16 acc[2][1], acc2[1][1];
#pragma unroll
        for (int m = 0; m < 2; ++m) zero_tile(acc[m][0]);
        zero_tile(acc2[0][0]);
        int s = 0;
        for (int slab = 0; slab < slabs; ++slab) {
            // one tap-row stage TR: its 12 steps multiply the fragments bf[12 TR ...]; TR == 0 starts every accumulator tile at
            // the bias tile (C operand of the slab's first MFMA)
            auto stage = [&](auto tr_tag) {
                constexpr int TR = decltype(tr_tag)::value;
                if (s + 1 < nstages) issue_w1(s + 1);          // slot (s+1)&1 was last read in stage s-1
                if (TR == 1) heads_dma_w2<T, 16, NW>(a.w2[head], a.head_conv, s_w2, wvs, l, slab * HC_SLAB * ES);   // after the barrier that follows the previous gemm2
                stage_pipelined<T, C, 1, HEADS_SPARSE_PF, TR == 0, TR * C::TAPS * (HC_IN / 16)>(acc, s_ring + (s & 1) * C::SLOT, bf, s_bias, slab, r, h, sw);
                __syncthreads();   // vmcnt(0) + barrier: next stage's weights (and the 1x1 slice) have landed
                ++s;
            };
            stage(std::integral_constant<int, 0>{});
            stage(std::integral_constant<int, 1>{});
            stage(std::integral_constant<int, 2>{});
            if constexpr (!PARK) {
                gemm2<T, 16, 1, 1, true>(acc, acc2, s_bias + slab * HC_SLAB * 4, s_w2, r, h, sw, a.s1);
            } else {
#pragma unroll
                for (int m2 = 0; m2 < M2H; ++m2) {
                    if (slab == 0) zero_tile(acc2[0][0]);
                    else parked_tile(m2, acc2[0][0]);
                    gemm2<T, 16, 1, 1, true>(acc, acc2, s_bias + slab * HC_SLAB * 4, s_w2 + m2 * 32 * C::RBW, r, h, sw, a.s1);
                    park_tile(m2, acc2[0][0]);
                }
            }
        }
        // ---- z = acc2 + b2 -> NCHW fp32 at the lane's position ------------------------------------------
        if (sp.ok) {
            const int C_head = a.C[head];
            const size_t cstride = (size_t)a.H * a.W;
            float *op = a.out[head] + (((size_t)sp.b * C_head + 4 * h) * a.H + sp.y) * a.W + sp.x;
#pragma unroll
            for (int m2 = 0; m2 < M2H; ++m2) {
                if (PARK) parked_tile(m2, acc2[0][0]);
                // (heads_kernel's epilogue at NT = 1 without the f16x3 scale, a copy: as one function of a tile both kernels could call it
                // changed the s_waitcnt count of a dense instantiation)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = m2 * 32 + 8 * g + 4 * h;
                    float *q = op + (size_t)(m2 * 32 + 8 * g) * cstride;
                    const f32x4 b2v = *reinterpret_cast<const f32x4 *>(s_bias + 1024 + c * 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (c + i < C_head) q[i * cstride] = acc2[0][0][4 * g + i] + b2v[i];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    };
    // the 1 / 2 / 3-tile body of this workgroup's head, as the MIXED dense launch picks it per head
    const int m2h = __builtin_amdgcn_readfirstlane((a.C[head] + 31) >> 5);
    if (m2h <= 1) body(std::integral_constant<int, 1>{});
    else if (m2h == 2) body(std::integral_constant<int, 2>{});
    else body(std::integral_constant<int, 3>{});
}

static_assert(HEADS_MAX == H3D_HEADS_MAX, "header/kernel mismatch");

// checks of an H3D_OP_HEADS op and its kernel arguments (the dense and the sparse launch)
static int heads_args(const h3d_op &op, HeadsArgs &a)
{
    if (!op.in || !op.w || !op.bias || !op.in2) H3D_FAIL(H3D_ERR_ARG, "heads: null pointer");
    const h3d_heads_desc *d = (const h3d_heads_desc *)op.in2;
    const int es = h3d_dtype_bytes(op.dtype);
    if (!es) H3D_FAIL(H3D_ERR_DTYPE, "heads: dtype %d", op.dtype);
    if (op.Cin != HC_IN || op.in_cs % (16 / es) || op.in_cs < HC_IN)
        H3D_FAIL(H3D_ERR_SHAPE, "heads: input must have %d channels (got %d, stride %d)", HC_IN, op.Cin, op.in_cs);
    if (op.Cout <= 0 || op.Cout % HC_SLAB || op.Cout > 256)
        H3D_FAIL(H3D_ERR_SHAPE, "heads: head_conv %d must be a multiple of %d, at most 256", op.Cout, HC_SLAB);
    if (d->nheads <= 0 || d->nheads > HEADS_MAX) H3D_FAIL(H3D_ERR_SHAPE, "heads: %d heads (max %d)", d->nheads, HEADS_MAX);
    a.in = (const char *)op.in; a.w1 = (const char *)op.w; a.b1 = op.bias;
    a.dbg = op.reserved & H3D_TUNE_HEADS_ABLATE_MASK;
    a.xcd = h3d_xcd_mode();
#ifdef H3D_ABLATE
    a.stamps = h3d_stamp_buffer();
#else
    a.stamps = nullptr;
#endif
    a.nlists = 0;
    memset(a.l_inds, 0, sizeof a.l_inds); memset(a.l_K, 0, sizeof a.l_K); memset(a.l_wg0, 0, sizeof a.l_wg0);
    memset(a.l_nh, 0, sizeof a.l_nh); memset(a.l_head, 0, sizeof a.l_head); memset(a.l_ng, 0, sizeof a.l_ng);
    a.nheads = d->nheads; a.head_conv = op.Cout; a.B = op.B; a.H = op.H; a.W = op.W; a.in_cs = op.in_cs;
    for (int i = 0; i < d->nheads; ++i) {
        if (!d->head[i].w2 || !d->head[i].b2 || !d->head[i].out) H3D_FAIL(H3D_ERR_ARG, "heads: head %d null pointer", i);
        if (d->head[i].C <= 0 || d->head[i].C > 32 * HC_MT2)
            H3D_FAIL(H3D_ERR_UNSUPPORTED, "heads: head %d has %d channels (max %d)", i, d->head[i].C, 32 * HC_MT2);
        a.w2[i] = (const char *)d->head[i].w2; a.b2[i] = d->head[i].b2; a.out[i] = d->head[i].out; a.C[i] = d->head[i].C;
        if (d->head[i].wexp2 < -60 || d->head[i].wexp2 > 60 || (d->head[i].wexp2 && op.dtype != H3D_F16X3))
            H3D_FAIL(H3D_ERR_ARG, "heads: head %d wexp2 %d (an H3D_F16X3 filter exponent)", i, d->head[i].wexp2);
        a.s2[i] = ldexpf(1.f, -d->head[i].wexp2);
    }
    if (d->wexp < -60 || d->wexp > 60 || (d->wexp && op.dtype != H3D_F16X3)) H3D_FAIL(H3D_ERR_ARG, "heads: wexp %d (an H3D_F16X3 filter exponent)", d->wexp);
    a.s1 = ldexpf(1.f, -d->wexp);
    return H3D_OK;
}

int h3d_launch_heads(const h3d_op &op, hipStream_t st)
{
    HeadsArgs a;
    if (const int rc = heads_args(op, a)) return rc;
    const h3d_heads_desc *d = (const h3d_heads_desc *)op.in2;
    const int es = h3d_dtype_bytes(op.dtype);
    int m2 = 1, m2min = HC_MT2;
    for (int i = 0; i < d->nheads; ++i) {
        m2 = max(m2, (d->head[i].C + 31) / 32);   // row tiles of the widest head
        m2min = min(m2min, (d->head[i].C + 31) / 32);
    }
    // heads of different widths in one launch: the kernel picks the 1 / 2 / 3-tile body per head (2-byte plans)
    const bool mixed = m2min != m2 && es == 2;
    const bool biasc = !(op.reserved & H3D_TUNE_HEADS_SEPARATE_BIAS);    // tuning override (tools/ab_heads.py): separate bias / zeroing pass
    return h3d_by_dtype<bf16_t, f16_t, float, x3_t>(op.dtype, "heads: dtype %d", [&](auto t) {
        using T = typename decltype(t)::type;
        constexpr int TH = sizeof(T) == 2 ? 16 : 8;
        a.tiles_x = cdiv(op.W, 32); a.tiles_y = cdiv(op.H, TH);
        const dim3 grid(op.B * a.tiles_x * a.tiles_y), blk(512);
        return h3d_by_values([&](auto m2c, auto bc, auto mx) {
            const h3d_kname name{"heads_kernel", t, TH, m2c, bc, h3d_opt(mx)};
            if constexpr (mx && (m2c < 2 || !bc)) {       // MIXED is instantiated for 2 | 3 row tiles with the bias in the accumulators
                if (name.dry()) return H3D_OK;
                H3D_FAIL(H3D_ERR_UNSUPPORTED, "heads: the separate-bias tuning override applies to launches of equal-width heads");
            } else {
                return h3d_launch(name, heads_kernel<T, TH, m2c, bc, mx>, grid, blk, 0, st, a);
            }
        }, h3d_vals<1, 2, 3>{}, m2, h3d_vals<false, true>{}, biasc, std::conditional_t<sizeof(T) == 2, h3d_vals<false, true>, h3d_vals<false>>{}, mixed);
    });
}

static_assert(HEADS_LISTS_MAX == H3D_HEADS_LISTS_MAX, "header/kernel mismatch");

// The per-list kernel arguments of a sparse launch from the lists in launch order (order[]), npos positions per workgroup; returns
// the grid.  per_head: a workgroup is (head, group of positions), in a list the widest heads first and all groups of a head in a row
// (heads_sparse_kernel); otherwise it is a group of positions that loops over the list's heads in descriptor order (heads_kernel<SPARSE>).
static int heads_fill_lists(HeadsArgs &a, const h3d_heads_list *lists, const int *order, bool per_head, int npos)
{
    int wgs = 0;
    for (int i = 0; i < a.nlists; ++i) {
        const h3d_heads_list &ls = lists[order[i]];
        a.l_inds[i] = (const long long *)ls.inds; a.l_K[i] = ls.K; a.l_wg0[i] = wgs; a.l_nh[i] = 0;
        for (int tiles = per_head ? HC_MT2 : 1; tiles >= 1; --tiles)
            for (int h = 0; h < a.nheads; ++h)
                if ((ls.head_mask >> h & 1) && (!per_head || (a.C[h] + 31) / 32 == tiles)) a.l_head[i][a.l_nh[i]++] = h;
        const int ng = cdiv(a.B * ls.K, npos);
        if (per_head) a.l_ng[i] = ng;
        wgs += per_head ? a.l_nh[i] * ng : ng;
    }
    return wgs;
}

// The heads of an H3D_OP_HEADS op at listed positions, written into the heads' dense maps there: bit for bit what the op's dense
// launch writes at those positions.  ONE launch for all lists, the lists with the most heads first.  Default: heads_sparse_kernel,
// one workgroup per (list, head, 256 positions).  H3D_TUNE_HEADS_SPARSE_LDS_PATCH (A/B, and maps beyond 2 GiB): heads_kernel<SPARSE>,
// where a list's workgroups (32 * CW positions each) form one run of the grid and loop over that list's heads -- there the order puts
// the longest chains of filter stages first, so that the short workgroups fill the CUs behind them instead of the other way round.
extern "C" int h3d_heads_sparse_lists(const h3d_op *op, int nlists, const h3d_heads_list *lists, void *stream)
{
    if (!op || !lists) H3D_FAIL(H3D_ERR_ARG, "heads_sparse: null pointer");
    if (op->kind != H3D_OP_HEADS) H3D_FAIL(H3D_ERR_ARG, "heads_sparse: op kind %d is not H3D_OP_HEADS", op->kind);
    if (nlists <= 0 || nlists > HEADS_LISTS_MAX) H3D_FAIL(H3D_ERR_ARG, "heads_sparse: %d position lists (1..%d)", nlists, HEADS_LISTS_MAX);
    if (op->B <= 0 || op->H <= 0 || op->W <= 0) H3D_FAIL(H3D_ERR_SHAPE, "heads_sparse: B %d, H %d, W %d", op->B, op->H, op->W);
    for (int i = 0; i < nlists; ++i) {
        if (!lists[i].inds) H3D_FAIL(H3D_ERR_ARG, "heads_sparse: list %d null pointer", i);
        if (lists[i].K <= 0 || (long long)op->B * lists[i].K > (1 << 24))
            H3D_FAIL(H3D_ERR_SHAPE, "heads_sparse: list %d: B %d, K %d", i, op->B, lists[i].K);
    }
    if (op->dtype != H3D_BF16 && op->dtype != H3D_F16)
        H3D_FAIL(H3D_ERR_UNSUPPORTED, "heads_sparse: dtype %d (the 2-byte plans)", op->dtype);
    if (op->reserved & ~(H3D_TUNE_HEADS_SPARSE_LDS_PATCH | H3D_TUNE_HEADS_SPARSE_WAVES4))
        H3D_FAIL(H3D_ERR_UNSUPPORTED, "heads_sparse: tuning word %#x", (unsigned)op->reserved);
    HeadsArgs a;
    if (const int rc = heads_args(*op, a)) return rc;
    uint32_t seen = 0;
    for (int i = 0; i < nlists; ++i) {
        const uint32_t m = lists[i].head_mask;
        if (!m || (a.nheads < 32 && m >> a.nheads))
            H3D_FAIL(H3D_ERR_ARG, "heads_sparse: list %d head mask %#x (bits 0..%d of the op's %d heads, at least one)", i, (unsigned)m, a.nheads - 1, a.nheads);
        if (m & seen) H3D_FAIL(H3D_ERR_ARG, "heads_sparse: list %d head mask %#x names a head of an earlier list (%#x)", i, (unsigned)m, (unsigned)(m & seen));
        seen |= m;
    }
    // launch order: most heads first (stable)
    int order[HEADS_LISTS_MAX];
    for (int i = 0; i < nlists; ++i) order[i] = i;
    for (int i = 1; i < nlists; ++i)
        for (int j = i; j > 0 && __builtin_popcount(lists[order[j]].head_mask) > __builtin_popcount(lists[order[j - 1]].head_mask); --j)
            std::swap(order[j], order[j - 1]);
    a.tiles_x = a.tiles_y = 1;
    a.nlists = nlists;
    // The neighbourhoods in registers (heads_sparse_kernel) unless the tuning word asks for the LDS-patch path below or the map is
    // beyond the 32-bit buffer offsets of the fragment loads.  One work item (workgroup) per (list, head, group of positions): no
    // workgroup runs more than one head's filter stages.  Grid order: the lists as below, in a list the widest heads first (their
    // second contraction and epilogue are the longest), all groups of a head in a row.
    const size_t in_bytes = (((size_t)op->B * op->H * op->W - 1) * op->in_cs + HC_IN) * h3d_dtype_bytes(op->dtype);
    if (!(op->reserved & H3D_TUNE_HEADS_SPARSE_LDS_PATCH) && in_bytes < HEADS_SPARSE_REG_MAX_BYTES) {
        const bool waves8 = !(op->reserved & H3D_TUNE_HEADS_SPARSE_WAVES4);
        const int wgs = heads_fill_lists(a, lists, order, true, 32 * (waves8 ? 8 : 4));
        return h3d_by_dtype<bf16_t, f16_t>(op->dtype, "heads_sparse: dtype %d", [&](auto t) {
            using T = typename decltype(t)::type;
            return h3d_by_values([&](auto nw) {
                constexpr int NW = decltype(nw)::value;
                const h3d_kname name{"heads_sparse_kernel", t, NW};
                return h3d_launch(name, heads_sparse_kernel<T, NW>, dim3(wgs), dim3(64 * NW), 0, (hipStream_t)stream, a);
            }, h3d_vals<4, 8>{}, waves8 ? 8 : 4);
        });
    }
    return h3d_by_dtype<bf16_t, f16_t>(op->dtype, "heads_sparse: dtype %d", [&](auto t) {
        using T = typename decltype(t)::type;
        using C = HeadsSparseCfg<T>;
        const dim3 grid(heads_fill_lists(a, lists, order, false, C::NPOS)), blk(64 * C::NW);
        // one instantiation: the body picks the 1 / 2 / 3-tile epilogue width per head
        const h3d_kname name{"heads_kernel", t, 16, 3, true, h3d_opt(true), h3d_opt(true)};
        return h3d_launch(name, heads_kernel<T, 16, 3, true, true, true>, grid, blk, 0, (hipStream_t)stream, a);
    });
}

// One list, every head of the descriptor (the K top-K centres of multi_pose_decode).
extern "C" int h3d_heads_sparse(const h3d_op *op, const int64_t *inds, int K, void *stream)
{
    if (!op || !inds) H3D_FAIL(H3D_ERR_ARG, "heads_sparse: null pointer");
    if (op->kind != H3D_OP_HEADS || !op->in2) H3D_FAIL(H3D_ERR_ARG, "heads_sparse: op kind %d is not H3D_OP_HEADS with a descriptor", op->kind);
    const int n = ((const h3d_heads_desc *)op->in2)->nheads;
    const h3d_heads_list all = {inds, K, n >= 32 ? ~0u : n > 0 ? (1u << n) - 1 : 1u};     // (a bad head count is heads_args' error)
    return h3d_heads_sparse_lists(op, 1, &all, stream);
}
