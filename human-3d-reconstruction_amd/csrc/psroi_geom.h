// Sample geometry of deformable PS-ROI pooling (reference: DCNv2/src/cuda/dcn_v2_psroi_pooling_cuda.cu:69-118, 179-240), ONE copy for
// the forward (csrc/psroi.hip), the backward (csrc/psroi_bwd.hip) and host programs that check it: every function is
// __host__ __device__ and uses plain C types and <math.h> only.
//
// Every operation is one IEEE fp32 operation in the reference's order; the translation units that include this header are compiled
// with -ffp-contract=off, so a gate, floor or ceil decision is the same wherever it is taken.  Everything about a sample except the
// channel it belongs to comes out of here: the in-map gate, the clamped corner, the two fractions and the "far corner exists" flags.
//
// Guards: a roi whose batch index is not finite or truncates outside [0, B) is not valid; infinite sample positions fail the gate, NaN
// ones are clamped to 0 by fmaxf / fminf, so 0 <= x < W, 0 <= y < H for every valid sample, and a far corner is flagged only when it
// lies inside the plane (a positive fraction implies a position below the last row / column).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSROI_HD __host__ __device__ inline
#else
#define PSROI_HD inline
#endif

enum { PSROI_VALID = 1, PSROI_FAR_X = 2, PSROI_FAR_Y = 4 };

struct PsroiRoi {
    int valid, b;                         // batch index in [0, B) when valid
    float start_w, start_h, roi_w, roi_h, bin_w, bin_h, sub_w, sub_h;
};

struct PsroiSample {
    int flags;                            // 0: not a sample (gated out); else PSROI_VALID | PSROI_FAR_X | PSROI_FAR_Y
    int x, y;                             // the near corner: floor of the clamped position
    float fx, fy;                         // position - near corner
};

// roi = (batch, x1, y1, x2, y2) in input-image pixels
PSROI_HD PsroiRoi psroi_roi(const float *roi, int B, float scale, int P, int spp)
{
    PsroiRoi g;
    const float bf = roi[0];
    g.valid = bf > -1.f && bf < (float)B;                                // NaN fails both; (int) truncates toward zero
    g.b = g.valid ? (int)bf : 0;
    g.start_w = roundf(roi[1]) * scale - 0.5f;
    g.start_h = roundf(roi[2]) * scale - 0.5f;
    const float end_w = (roundf(roi[3]) + 1.f) * scale - 0.5f;
    const float end_h = (roundf(roi[4]) + 1.f) * scale - 0.5f;
    g.roi_w = fmaxf(end_w - g.start_w, 0.1f);
    g.roi_h = fmaxf(end_h - g.start_h, 0.1f);
    g.bin_w = g.roi_w / (float)P;
    g.bin_h = g.roi_h / (float)P;
    g.sub_w = g.bin_w / (float)spp;
    g.sub_h = g.bin_h / (float)spp;
    return g;
}

// the part cell a bin row / column reads its translation from
PSROI_HD int psroi_part(int p, int P, int part)
{
    int q = (int)floorf((float)p / (float)P * (float)part);
    q = q < 0 ? 0 : q;
    return q > part - 1 ? part - 1 : q;
}

// sample (ih, iw) of bin (ph, pw); trans_x / trans_y = translation * trans_std (0 without translations)
PSROI_HD PsroiSample psroi_sample(const PsroiRoi &g, int ph, int pw, int ih, int iw, float trans_x, float trans_y, int H, int W)
{
    PsroiSample s;
    s.flags = 0; s.x = 0; s.y = 0; s.fx = 0.f; s.fy = 0.f;
    float wstart = (float)pw * g.bin_w + g.start_w;
    wstart += trans_x * g.roi_w;
    float hstart = (float)ph * g.bin_h + g.start_h;
    hstart += trans_y * g.roi_h;
    float w = wstart + (float)iw * g.sub_w;
    float h = hstart + (float)ih * g.sub_h;
    if (!(w < -0.5f || w > (float)W - 0.5f || h < -0.5f || h > (float)H - 0.5f)) {
        w = fminf(fmaxf(w, 0.f), (float)(W - 1));
        h = fminf(fmaxf(h, 0.f), (float)(H - 1));
        s.x = (int)floorf(w);
        s.y = (int)floorf(h);
        s.fx = w - (float)s.x;
        s.fy = h - (float)s.y;
        // ceil == floor + (fraction > 0): the far corners are inside the plane whenever they are used
        s.flags = PSROI_VALID | (s.fx > 0.f ? PSROI_FAR_X : 0) | (s.fy > 0.f ? PSROI_FAR_Y : 0);
    }
    return s;
}
