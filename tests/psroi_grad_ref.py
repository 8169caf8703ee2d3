"""numpy restatement of deformable PS-ROI pooling WITH its backward (reference: DCNv2/src/cuda/dcn_v2_psroi_pooling_cuda.cu:58-269),
in operator mode (trans [R, 2*classes, part, part], output_count) and in modulated mode (DCNPooling's second pass: offset_mask
[R, 3, P, P], channels 0/1 the translations, the result times sigmoid(channel 2), the count recomputed).

Test-only helper.  `geometry=np.float32`: positions, gates and corners are the kernel's exactly (one fp32 operation at a time in the
reference's order, as tests/psroi_ref.py, whose forward this file reproduces bit for bit); `geometry=np.float64`: the same operations
on the same fp32 inputs in float64, where central differences with a step of 1e-6 resolve the gradients.  Values and sums are float64
(`acc=np.float32` computes them in float32 instead: the yardstick of the module test).

`bounds()` returns the float64 gradients and a per-element bound on the error of an fp32 evaluation in any summation order,
(n_terms + c) * 2^-24 * sum |contributions| (DESIGN.md section 33 derives c from the operation count of one contribution)."""
import numpy as np
import torch

from psroi_ref import round_half_away

f32 = np.float32
U = 2.0 ** -24
# roundings of ONE contribution, plus 1 for the second-order terms
C_INPUT = 6        # go / cnt | 1 - fx | 1 - fy | q | q * diff_val
C_TRANS = 10       # go / cnt | 1 - f | product | 3 adds | * trans_std | * diff_val | * roi size
C_SIGMOID = 5      # expf (1 ulp = 2 u) | 1 + e | 1 / x | go * s
C_MASK = 8         # 1 - fx | 1 - fy | q | q * U | / cnt | go * pooled | * s(1 - s), and its own product


def part_index(P, part):
    p = np.arange(P).astype(f32)
    return np.clip(np.floor(p / f32(P) * f32(part)).astype(np.int64), 0, part - 1)


def _roi(roi, scale, P, spp, gt):
    x1, y1, x2, y2 = (gt(v) for v in round_half_away(roi[1:5]))
    scale, half = gt(f32(scale)), gt(0.5)
    rsw = x1 * scale - half
    rsh = y1 * scale - half
    rew = (x2 + gt(1)) * scale - half
    reh = (y2 + gt(1)) * scale - half
    roi_w = np.fmax(rew - rsw, gt(f32(0.1)))
    roi_h = np.fmax(reh - rsh, gt(f32(0.1)))
    bin_w, bin_h = roi_w / gt(P), roi_h / gt(P)
    return rsw, rsh, roi_w, roi_h, bin_w, bin_h, bin_w / gt(spp), bin_h / gt(spp)


def _kink(v, valid, L):
    """Smallest distance of a valid sample coordinate to an integer inside the map or to the gate / clamp edges -0.5, 0, L-1, L-0.5."""
    if not valid.any():
        return np.inf
    v = v[valid].astype(np.float64)
    d = np.minimum(np.abs(v - np.clip(np.rint(v), 0, L - 1)), np.minimum(np.abs(v + 0.5), np.abs(v - (L - 0.5))))
    return float(d.min())


def _samples(geo, tx, ty, P, spp, H, W, gt):
    """Per (bin, sample) [P, P, spp, spp]: valid, near / far corners, the two fractions (dtype gt), kink distance."""
    rsw, rsh, roi_w, roi_h, bin_w, bin_h, sub_w, sub_h = geo
    half = gt(0.5)
    ph = np.arange(P).reshape(P, 1, 1, 1).astype(gt)
    pw = np.arange(P).reshape(1, P, 1, 1).astype(gt)
    ih = np.arange(spp).reshape(1, 1, spp, 1).astype(gt)
    iw = np.arange(spp).reshape(1, 1, 1, spp).astype(gt)
    wstart = pw * bin_w + rsw
    wstart = wstart + tx[:, :, None, None] * roi_w
    hstart = ph * bin_h + rsh
    hstart = hstart + ty[:, :, None, None] * roi_h
    w = np.broadcast_to(wstart + iw * sub_w, (P, P, spp, spp)).astype(gt)
    h = np.broadcast_to(hstart + ih * sub_h, (P, P, spp, spp)).astype(gt)
    valid = ~((w < -half) | (w > gt(W) - half) | (h < -half) | (h > gt(H) - half))
    kink = min(_kink(w, valid, W), _kink(h, valid, H))
    w = np.fmin(np.fmax(w, gt(0)), gt(W - 1))
    h = np.fmin(np.fmax(h, gt(0)), gt(H - 1))
    xa, ya = np.floor(w).astype(np.int64), np.floor(h).astype(np.int64)
    xb, yb = np.ceil(w).astype(np.int64), np.ceil(h).astype(np.int64)
    return valid, xa, ya, xb, yb, w - xa.astype(gt), h - ya.astype(gt), kink


def _classes(inp, rois, trans, no_trans, scale, P, part, spp, tstd, mask, geometry):
    """Iterate the (roi, class) pairs that contribute: n, k, channel slice, batch index, roi_w, roi_h, sample arrays."""
    B, C, H, W = inp.shape
    gt = geometry
    ncls = 1 if no_trans else (1 if mask is not None else np.asarray(trans).shape[1] // 2)
    cpc = C // ncls
    ph_part, pw_part = part_index(P, part).reshape(P, 1), part_index(P, part).reshape(1, P)
    tstd = gt(f32(tstd))
    for n in range(rois.shape[0]):
        bf = rois[n, 0]
        if not (bf > -1 and bf < B):
            continue
        for k in range(ncls):
            with np.errstate(all="ignore"):
                geo = _roi(rois[n], scale, P, spp, gt)
                if no_trans:
                    tx = ty = np.zeros((P, P), gt)
                else:
                    tx = np.asarray(trans[n, 2 * k]).astype(gt)[ph_part, pw_part] * tstd
                    ty = np.asarray(trans[n, 2 * k + 1]).astype(gt)[ph_part, pw_part] * tstd
                sm = _samples(geo, tx, ty, P, spp, H, W, gt)
            yield n, k, slice(k * cpc, (k + 1) * cpc), int(bf), geo[2], geo[3], sm


def _prep(inp, rois, trans, no_trans, mask):
    inp = np.asarray(inp, f32)
    rois = np.asarray(rois, f32).reshape(-1, 5)
    if mask is not None:
        no_trans = 0
    return inp, rois, (None if no_trans else np.asarray(trans)), int(bool(no_trans))


def forward(inp, rois, trans, no_trans, spatial_scale, pooled_size, part_size, sample_per_part, trans_std, mask=None,
            geometry=f32, acc=np.float64, want_kink=False):
    """(output [R, C, P, P] of dtype acc, output_count float32); mask = [R, P, P] logits (modulated mode; trans = [R, >= 2, P, P])."""
    inp, rois, trans, no_trans = _prep(inp, rois, trans, no_trans, mask)
    P, spp = pooled_size, sample_per_part
    R, C = rois.shape[0], inp.shape[1]
    out = np.zeros((R, C, P, P), acc)
    cnt = np.zeros((R, C, P, P), f32)
    kink = np.inf
    with np.errstate(all="ignore"):
        for n, k, ks, b, _, _, (valid, xa, ya, xb, yb, dx, dy, kd) in _classes(inp, rois, trans, no_trans, spatial_scale, P, part_size,
                                                                              spp, trans_std, mask, geometry):
            kink = min(kink, kd)
            dx, dy = dx.astype(acc), dy.astype(acc)
            plane = inp[b, ks].astype(acc)
            val = ((1 - dx) * (1 - dy) * plane[:, ya, xa] + (1 - dx) * dy * plane[:, yb, xa]
                   + dx * (1 - dy) * plane[:, ya, xb] + dx * dy * plane[:, yb, xb])
            val = np.where(valid, val, acc(0))
            s = val.sum(axis=(-1, -2))
            c = valid.sum(axis=(-1, -2))
            o = np.where(c > 0, s / np.maximum(c, 1).astype(acc), acc(0))
            if mask is not None:
                o = o * (1.0 / (1.0 + np.exp(-np.asarray(mask[n], acc))))
            out[n, ks] = o
            cnt[n, ks] = c
    return (out, cnt, kink) if want_kink else (out, cnt)


def backward(grad_out, inp, rois, trans, count, no_trans, spatial_scale, pooled_size, part_size, sample_per_part, trans_std, mask=None,
             geometry=f32, acc=np.float64):
    """Gradients of sum(grad_out * forward) and what `bounds` needs.  count = the forward's output_count (operator mode; None: recomputed,
    as modulated mode always does).  Returns a dict: g_input [B,C,H,W], g_trans (like trans; modulated: [R,3,P,P] with the mask-logit
    gradient in channel 2), a_* = sum |contributions|, n_* = number of contributions, c_* = roundings per contribution (arrays for the
    mask logit), kink."""
    inp, rois, trans, no_trans = _prep(inp, rois, trans, no_trans, mask)
    grad_out = np.asarray(grad_out)                          # (float32 from a kernel's caller; the replica below hands over its own dtype)
    B, C, H, W = inp.shape
    P, spp, part = pooled_size, sample_per_part, part_size
    R = rois.shape[0]
    g_in, a_in, n_in = np.zeros(B * C * H * W, acc), np.zeros(B * C * H * W), np.zeros(B * C * H * W)
    tshape = None if no_trans else ((R, 3, P, P) if mask is not None else np.asarray(trans).shape)
    g_tr = a_tr = n_tr = c_tr = None
    if tshape is not None:
        g_tr, a_tr, n_tr = np.zeros(tshape, acc), np.zeros(tshape), np.zeros(tshape)
        c_tr = np.full(tshape, float(C_TRANS + (C_SIGMOID if mask is not None else 0)))
    ph_part, pw_part = np.broadcast_arrays(part_index(P, part).reshape(P, 1), part_index(P, part).reshape(1, P))
    tstd = acc(f32(trans_std))
    kink = np.inf

    def scatter(dst, idx, w):
        if dst.dtype == np.float64:
            dst += np.bincount(idx.ravel(), weights=np.asarray(w, np.float64).ravel(), minlength=dst.size)
        else:
            np.add.at(dst, idx.ravel(), w.ravel())

    with np.errstate(all="ignore"):
        for n, k, ks, b, roi_w, roi_h, (valid, xa, ya, xb, yb, dx, dy, kd) in _classes(inp, rois, trans, no_trans, spatial_scale, P, part,
                                                                                      spp, trans_std, mask, geometry):
            kink = min(kink, kd)
            dx, dy, roi_w, roi_h = dx.astype(acc), dy.astype(acc), acc(roi_w), acc(roi_h)
            plane = inp[b, ks].astype(acc)
            cpc = plane.shape[0]
            go = grad_out[n, ks].astype(acc)
            cnt = valid.sum(axis=(-1, -2)).astype(acc)[None] if (count is None or mask is not None) else np.asarray(count[n, ks], acc)
            cnt = np.broadcast_to(cnt, go.shape)
            sig = None
            up = go
            if mask is not None:
                sig = 1.0 / (1.0 + np.exp(-np.asarray(mask[n], acc)))
                up = go * sig
            live = cnt > 0
            dv = np.where(live, up / np.where(live, cnt, acc(1)), acc(0))[:, :, :, None, None]        # [cpc, P, P, 1, 1]
            vm = valid[None] & live[:, :, :, None, None]
            cbase = ((b * C + ks.start + np.arange(cpc)) * H * W).reshape(cpc, 1, 1, 1, 1)
            q = {(0, 0): (1 - dx) * (1 - dy), (0, 1): (1 - dx) * dy, (1, 0): dx * (1 - dy), (1, 1): dx * dy}      # (far x, far y)
            for (fx_, fy_), qq in q.items():
                x, y = (xb if fx_ else xa), (yb if fy_ else ya)
                exists = vm & ((dx > 0) if fx_ else True) & ((dy > 0) if fy_ else True)
                idx = np.broadcast_to(cbase + (y * W + x)[None], exists.shape)[exists]
                contrib = np.broadcast_to(qq[None] * dv, exists.shape)[exists]
                scatter(g_in, idx, contrib)
                a_in += np.bincount(idx, weights=np.abs(contrib).astype(np.float64), minlength=a_in.size)
                n_in += np.bincount(idx, minlength=n_in.size)
            if tshape is None:
                continue
            U00, U01, U10, U11 = plane[:, ya, xa], plane[:, yb, xa], plane[:, ya, xb], plane[:, yb, xb]
            fac_x, fac_y = tstd * dv * roi_w, tstd * dv * roi_h
            gx = np.where(vm, (U11 * dy + U10 * (1 - dy) - U01 * dy - U00 * (1 - dy)) * fac_x, acc(0))
            gy = np.where(vm, (U11 * dx + U01 * (1 - dx) - U10 * dx - U00 * (1 - dx)) * fac_y, acc(0))
            ax = np.where(vm, (np.abs(U11) * dy + np.abs(U10) * (1 - dy) + np.abs(U01) * dy + np.abs(U00) * (1 - dy)) * np.abs(fac_x), 0)
            ay = np.where(vm, (np.abs(U11) * dx + np.abs(U01) * (1 - dx) + np.abs(U10) * dx + np.abs(U00) * (1 - dx)) * np.abs(fac_y), 0)
            terms = vm.sum(axis=(0, 3, 4)).astype(np.float64)                                              # [P, P]
            for ch, g, aa in ((2 * k, gx, ax), (2 * k + 1, gy, ay)):
                np.add.at(g_tr[n, ch], (ph_part, pw_part), g.sum(axis=(0, 3, 4)))
                np.add.at(a_tr[n, ch], (ph_part, pw_part), aa.sum(axis=(0, 3, 4), dtype=np.float64))
                np.add.at(n_tr[n, ch], (ph_part, pw_part), terms)
            if mask is not None:
                qa = (np.abs(U00) * q[(0, 0)] + np.abs(U01) * q[(0, 1)] + np.abs(U10) * q[(1, 0)] + np.abs(U11) * q[(1, 1)])
                val = np.where(vm, U00 * q[(0, 0)] + U01 * q[(0, 1)] + U10 * q[(1, 0)] + U11 * q[(1, 1)], acc(0))
                safe = np.where(live, cnt, acc(1))
                pooled = val.sum(axis=(-1, -2)) / safe
                s1 = sig * (1 - sig)
                g_tr[n, 2] = s1 * (go * pooled).sum(axis=0)
                a_tr[n, 2] = s1 * (np.abs(go) * np.where(vm, qa, 0).sum(axis=(-1, -2), dtype=np.float64) / safe).sum(axis=0)
                n_tr[n, 2] = 4 * terms
                # s(1 - s): s carries 4 u; 1 - s inherits 4 u s / (1 - s) and adds one rounding
                c_tr[n, 2] = C_MASK + 4 + 4 * sig / (1 - sig) + 1
    c_in = float(C_INPUT + (C_SIGMOID if mask is not None else 0))
    res = dict(g_input=g_in.reshape(B, C, H, W), a_input=a_in.reshape(B, C, H, W), n_input=n_in.reshape(B, C, H, W), c_input=c_in,
               g_trans=g_tr, a_trans=a_tr, n_trans=n_tr, c_trans=c_tr, kink=kink)
    return res


def bounds(grad_out, inp, rois, trans, count, no_trans, spatial_scale, pooled_size, part_size, sample_per_part, trans_std, mask=None):
    """((grad_input, grad_trans), (bound_input, bound_trans)): float64 gradients on the kernel's geometry and, per element, the bound
    (n_terms + c) * 2^-24 * sum |contributions| on the error of an fp32 evaluation in any summation order.  grad_trans / bound_trans are
    None with no_trans; in modulated mode they are [R, 3, P, P] (channel 2: the mask logit)."""
    r = backward(grad_out, inp, rois, trans, count, no_trans, spatial_scale, pooled_size, part_size, sample_per_part, trans_std, mask)
    b_in = (r["n_input"] + r["c_input"]) * U * r["a_input"]
    b_tr = None if r["g_trans"] is None else (r["n_trans"] + r["c_trans"]) * U * r["a_trans"]
    return (r["g_input"], r["g_trans"]), (b_in, b_tr)


def check(name, got, ref, bound):
    """max over elements of |got - ref| - bound must be <= 0; prints the worst ratio err / bound.  A NaN must meet a NaN (a roi with
    infinite coordinates has an infinite width, and 0 * inf is the reference's translation gradient there)."""
    got = np.asarray(got, np.float64)
    with np.errstate(all="ignore"):
        err = np.where(np.isnan(got) & np.isnan(ref), 0.0, np.where(np.isnan(got) | np.isnan(ref), np.inf, np.abs(got - ref)))
        bound = np.where(np.isnan(bound), 0.0, bound)
    with np.errstate(all="ignore"):
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)))) if err.size else 0.0
    print("%s: max err %.3g, max |ref| %.3g, worst err / bound %.3g" % (name, float(err.max()) if err.size else 0.0,
                                                                          float(np.nanmax(np.abs(ref))) if err.size else 0.0, ratio))
    assert ratio <= 1.0, (name, ratio)
    return ratio


# ---- a CPU replica of the TrainableDCNPooling module: torch MLP + autograd wrappers around the restatement ------------------------

class _Pool(torch.autograd.Function):
    """Operator mode without translations (DCNPooling's first pass) or modulated mode (its second), on numpy."""

    @staticmethod
    def forward(ctx, inp, offset_mask, rois, cfg, geometry, acc):
        ctx.cfg, ctx.rois, ctx.np = cfg, rois, (geometry, acc)
        ctx.save_for_backward(inp, offset_mask)
        x = inp.detach().numpy().astype(f32)
        if offset_mask is None:
            out, _ = forward(x, rois, None, 1, *cfg, geometry=geometry, acc=acc)
        else:
            om = offset_mask.detach().numpy()
            out, _ = forward(x, rois, om, 0, *cfg, mask=om[:, 2], geometry=geometry, acc=acc)
        return torch.from_numpy(out).to(inp.dtype)

    @staticmethod
    def backward(ctx, grad):
        inp, offset_mask = ctx.saved_tensors
        geometry, acc = ctx.np
        x, g = inp.detach().numpy().astype(f32), grad.detach().numpy()
        if offset_mask is None:
            r = backward(g, x, ctx.rois, None, None, 1, *ctx.cfg, geometry=geometry, acc=acc)
            return torch.from_numpy(r["g_input"]).to(inp.dtype), None, None, None, None, None
        om = offset_mask.detach().numpy()
        r = backward(g, x, ctx.rois, om, None, 0, *ctx.cfg, mask=om[:, 2], geometry=geometry, acc=acc)
        return torch.from_numpy(r["g_input"]).to(inp.dtype), torch.from_numpy(r["g_trans"]).to(offset_mask.dtype), None, None, None, None


def module_replica(state_dict, inp, rois, grad_out, spatial_scale, pooled_size, sample_per_part, trans_std, dtype):
    """TrainableDCNPooling on the CPU in `dtype` (torch.float64: float64 geometry and sums; torch.float32: both in float32):
    returns (output, input gradient, {parameter name: gradient}, kink distance of the second pass) for the upstream `grad_out`."""
    gt = np.float64 if dtype == torch.float64 else np.float32
    P = pooled_size
    cfg = (spatial_scale, P, P, sample_per_part, trans_std)
    sd = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in state_dict.items()}
    x = torch.as_tensor(np.asarray(inp, f32)).to(dtype).requires_grad_(True)
    rois = np.asarray(rois, f32)
    n = rois.shape[0]
    roi = _Pool.apply(x, None, rois, cfg, gt, gt)
    h = roi.reshape(n, -1)
    for i in (0, 2, 4):
        h = torch.nn.functional.linear(h, sd["offset_mask_fc.%d.weight" % i], sd["offset_mask_fc.%d.bias" % i])
        if i < 4:
            h = torch.relu(h)
    out = _Pool.apply(x, h.view(n, 3, P, P), rois, cfg, gt, gt)
    out.backward(torch.as_tensor(np.asarray(grad_out, f32)).to(dtype))
    om = h.detach().numpy().reshape(n, 3, P, P)
    # (the second pass is the one whose positions are differentiated; the first has no translations and is linear in the input)
    kink = forward(x.detach().numpy(), rois, om, 0, *cfg, mask=om[:, 2], geometry=gt, want_kink=True)[2]
    return out.detach(), x.grad, {k: v.grad for k, v in sd.items()}, kink


# ---- cases shared by tests/test_oracle_psroi_backward.py and tests/test_gpu_psroi_backward.py ---------------------------------------

# tests/test_gpu_psroi.py::test_edge_rois's list (input [2, 16, 21, 17], scale 0.25)
EDGE_SHAPE = (2, 16, 21, 17)
EDGE_ROIS = np.array([
    [0, 10, 10, 4, 3],              # x2 < x1
    [1, 8, 8, 8, 8],                # one pixel
    [0, 7.5, 6.5, 7.5, 6.5],        # zero size at half-integers
    [1, 500, 500, 900, 800],        # far outside
    [0, -400, -300, -200, -100],    # far outside, negative
    [1, 2.5, 3.5, 30.5, 41.5],      # half-integer corners
    [0, -2.5, -0.5, 10.49, 12.51],  # fractional, partly outside
    [1, 0, 0, 67, 83],              # the whole map
    [0.9, 3, 3, 20, 20],            # batch index truncates to 0
    [1.99, 3, 3, 20, 20],           # ... and to 1
], f32)
_nan, _inf = np.nan, np.inf
# invalid batch indices and non-finite / huge coordinates
BAD_ROIS = np.array([
    [_nan, 2, 2, 30, 30], [-1, 2, 2, 30, 30], [2, 2, 2, 30, 30], [_inf, 2, 2, 30, 30], [-_inf, 2, 2, 30, 30], [1e30, 2, 2, 30, 30],
    [0, _nan, 2, 30, 30], [1, 2, _nan, 30, 30], [0, 2, 2, _inf, 30], [1, -_inf, 2, 30, 30], [0, 2, 2, 30, -_inf],
    [1, 1e30, 2, 30, 30], [0, 2, -1e30, 30, 1e30], [1, _nan, _nan, _nan, _nan], [0, -_inf, -_inf, _inf, _inf],
], f32)


def random_rois(rng, R, B, H, W, scale):
    x = rng.uniform(-0.2 * W / scale, 1.2 * W / scale, (R, 2))
    y = rng.uniform(-0.2 * H / scale, 1.2 * H / scale, (R, 2))
    return np.stack([rng.integers(0, B, R), x.min(1), y.min(1), x.max(1), y.max(1)], 1).astype(f32)


def lattice_case(seed=0, R=6):
    """B 2, C 4 (2 classes), 12 x 12, scale 0.25, P = part = 2, spp 2, trans_std 0.5: integer inputs in [-8, 8], integer roi corners with
    width and height in {16, 32} px partly outside the map, trans a multiple of 0.25 in [-0.5, 0.5], grad_out a multiple of 12 in [-48, 48]
    (every count 1 .. 4 divides it).  Every position is a multiple of 0.25, every weight a multiple of 1/16."""
    rng = np.random.default_rng(seed)
    inp = rng.integers(-8, 9, (2, 4, 12, 12)).astype(f32)
    x1, y1 = rng.integers(-16, 41, R), rng.integers(-16, 41, R)
    w, h = rng.choice([16, 32], R), rng.choice([16, 32], R)
    rois = np.stack([rng.integers(0, 2, R), x1, y1, x1 + w - 1, y1 + h - 1], 1).astype(f32)
    trans = (rng.integers(-2, 3, (R, 4, 2, 2)) * 0.25).astype(f32)
    grad_out = (rng.integers(-4, 5, (R, 4, 2, 2)) * 12).astype(f32)
    return dict(inp=inp, rois=rois, trans=trans, grad_out=grad_out, scale=0.25, P=2, part=2, spp=2, tstd=0.5)
