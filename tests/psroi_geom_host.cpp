// Host program for tests/test_oracle_psroi_backward.py: runs the sample geometry the PS-ROI pooling kernels share
// (csrc/psroi_geom.h, plain C++ on the host) over a list of rois and prints every sample's (flags, offset) pair.
//
//   psroi_geom_host CASE_FILE
// CASE_FILE: B H W scale P part spp trans_std no_trans ncls R, then R rows of 5 roi numbers, then (unless no_trans)
// R * 2 * ncls * part * part translations; "nan", "inf" and "-inf" are numbers (strtof).
// Output, one line per (roi, class): "roi N class K invalid" or "roi N class K" followed by one line per sample
// "PH PW IH IW FLAGS OFFSET FXBITS FYBITS" (offset = y * W + x of the near corner; the fractions as bit patterns).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "psroi_geom.h"

static bool next_float(FILE *f, float *v)
{
    char tok[64];
    if (fscanf(f, "%63s", tok) != 1) return false;
    char *end = nullptr;
    *v = strtof(tok, &end);
    return end != tok;
}

static uint32_t bits(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    float hdr[11];
    for (float &h : hdr)
        if (!next_float(f, &h)) return 3;
    const int B = (int)hdr[0], H = (int)hdr[1], W = (int)hdr[2], P = (int)hdr[4], part = (int)hdr[5], spp = (int)hdr[6];
    const float scale = hdr[3], trans_std = hdr[7];
    const int no_trans = (int)hdr[8], ncls = (int)hdr[9], R = (int)hdr[10];
    std::vector<float> rois((size_t)R * 5), trans(no_trans ? 0 : (size_t)R * 2 * ncls * part * part);
    for (float &v : rois)
        if (!next_float(f, &v)) return 3;
    for (float &v : trans)
        if (!next_float(f, &v)) return 3;
    fclose(f);

    for (int n = 0; n < R; ++n) {
        const PsroiRoi geo = psroi_roi(&rois[(size_t)n * 5], B, scale, P, spp);
        for (int k = 0; k < ncls; ++k) {
            if (!geo.valid) {
                printf("roi %d class %d invalid\n", n, k);
                continue;
            }
            printf("roi %d class %d\n", n, k);
            for (int ph = 0; ph < P; ++ph)
                for (int pw = 0; pw < P; ++pw) {
                    float tx = 0.f, ty = 0.f;
                    if (!no_trans) {
                        const float *tk = &trans[((size_t)n * 2 * ncls + 2 * k) * part * part] + psroi_part(ph, P, part) * part + psroi_part(pw, P, part);
                        tx = tk[0] * trans_std;
                        ty = tk[part * part] * trans_std;
                    }
                    for (int ih = 0; ih < spp; ++ih)
                        for (int iw = 0; iw < spp; ++iw) {
                            const PsroiSample s = psroi_sample(geo, ph, pw, ih, iw, tx, ty, H, W);
                            printf("%d %d %d %d %d %d %u %u\n", ph, pw, ih, iw, s.flags, s.y * W + s.x, bits(s.fx), bits(s.fy));
                        }
                }
        }
    }
    return 0;
}
