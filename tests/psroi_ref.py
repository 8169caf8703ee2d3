"""numpy restatement of deformable PS-ROI pooling, forward (reference: DCNv2/src/cuda/dcn_v2_psroi_pooling_cuda.cu:58-146).

Test-only helper.  The geometry is float32, one operation at a time in the reference's order (round half away from zero, fmax /
fmin clamps, corners floor / ceil), so sample positions and counts are the kernel's exactly; sample values and sums are float64.
Rois whose batch index is not finite or truncates outside [0, B) give 0 with count 0 (the library's decision; the reference reads
out of bounds there).  `mask` ([R, P, P] logits) multiplies each bin by sigmoid(mask), as DCNPooling's second pass does."""
import numpy as np

f32 = np.float32


def round_half_away(x):
    """C roundf: half away from zero (numpy's np.round rounds half to even)."""
    x = np.asarray(x, f32)
    t = np.trunc(x)
    frac = x - t                                             # exact in float32
    return (t + np.where(np.abs(frac) >= f32(0.5), np.sign(x), f32(0))).astype(f32)


def psroi_pool(inp, rois, trans, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size, sample_per_part,
               trans_std, mask=None):
    """Returns (output float64 [R, C, P, P], output_count float32 [R, C, P, P])."""
    inp = np.asarray(inp, f32)
    rois = np.asarray(rois, f32).reshape(-1, 5)
    B, C, H, W = inp.shape
    R, P, spp, part = rois.shape[0], pooled_size, sample_per_part, part_size
    assert group_size == 1 and output_dim == C
    ncls = 1 if no_trans else np.asarray(trans).shape[1] // 2
    cpc = output_dim // ncls
    out = np.zeros((R, C, P, P))
    cnt = np.zeros((R, C, P, P), f32)
    scale, tstd, half = f32(spatial_scale), f32(trans_std), f32(0.5)
    ph = np.arange(P).reshape(P, 1, 1, 1)
    pw = np.arange(P).reshape(1, P, 1, 1)
    ih = np.arange(spp).reshape(1, 1, spp, 1).astype(f32)
    iw = np.arange(spp).reshape(1, 1, 1, spp).astype(f32)
    part_h = np.clip(np.floor(ph.astype(f32) / f32(P) * f32(part)).astype(np.int64), 0, part - 1)
    part_w = np.clip(np.floor(pw.astype(f32) / f32(P) * f32(part)).astype(np.int64), 0, part - 1)
    if not no_trans:
        trans = np.asarray(trans, f32)
    with np.errstate(all="ignore"):
        for n in range(R):
            bf = rois[n, 0]
            if not (bf > -1 and bf < B):
                continue
            b = int(bf)
            x1, y1, x2, y2 = (round_half_away(v) for v in rois[n, 1:])
            rsw = x1 * scale - half
            rsh = y1 * scale - half
            rew = (x2 + f32(1)) * scale - half
            reh = (y2 + f32(1)) * scale - half
            roi_w = np.fmax(rew - rsw, f32(0.1))
            roi_h = np.fmax(reh - rsh, f32(0.1))
            bin_w, bin_h = roi_w / f32(P), roi_h / f32(P)
            sub_w, sub_h = bin_w / f32(spp), bin_h / f32(spp)
            for k in range(ncls):
                if no_trans:
                    tx = ty = f32(0)
                else:
                    tx = trans[n, 2 * k][part_h, part_w] * tstd
                    ty = trans[n, 2 * k + 1][part_h, part_w] * tstd
                wstart = pw.astype(f32) * bin_w + rsw
                wstart = wstart + tx * roi_w
                hstart = ph.astype(f32) * bin_h + rsh
                hstart = hstart + ty * roi_h
                w = np.broadcast_to(wstart + iw * sub_w, (P, P, spp, spp)).astype(f32)
                h = np.broadcast_to(hstart + ih * sub_h, (P, P, spp, spp)).astype(f32)
                valid = ~((w < -half) | (w > f32(W) - half) | (h < -half) | (h > f32(H) - half))
                w = np.fmin(np.fmax(w, f32(0)), f32(W - 1))
                h = np.fmin(np.fmax(h, f32(0)), f32(H - 1))
                xa, ya = np.floor(w).astype(np.int64), np.floor(h).astype(np.int64)
                xb, yb = np.ceil(w).astype(np.int64), np.ceil(h).astype(np.int64)
                dx = (w - xa.astype(f32)).astype(np.float64)
                dy = (h - ya.astype(f32)).astype(np.float64)
                plane = inp[b, k * cpc:(k + 1) * cpc].astype(np.float64)
                val = ((1 - dx) * (1 - dy) * plane[:, ya, xa] + (1 - dx) * dy * plane[:, yb, xa]
                       + dx * (1 - dy) * plane[:, ya, xb] + dx * dy * plane[:, yb, xb])
                val = np.where(valid, val, 0.0)
                s = val.sum(axis=(-1, -2))
                c = valid.sum(axis=(-1, -2))
                o = np.where(c > 0, s / np.maximum(c, 1), 0.0)
                if mask is not None:
                    o = o * (1.0 / (1.0 + np.exp(-np.asarray(mask[n], np.float64))))
                out[n, k * cpc:(k + 1) * cpc] = o
                cnt[n, k * cpc:(k + 1) * cpc] = c
    return out, cnt
