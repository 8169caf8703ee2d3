"""fp64 references, the derived element-wise error bound and a CPU emulation of the "f16x3" arithmetic (csrc/common.h ET<x3_t>): fp32
storage, every contraction as three fp16 MFMAs on operands split as x = hi + lo.  Shared by tests/test_oracle_x3_domain.py (CPU: the
emulation keeps the bound, the bound is not vacuous) and tests/test_gpu_x3_domain.py (the kernels keep it).

The bound, for one contraction y = sum_k w_k x_k + b with filters packed times 2^wexp (engine.x3_exp):

    |y - y64| <= TAU (A + |b|) + 2^-25 S + 2^-38 max|w| X

  A = sum |w_k| |x_k|, S = sum |w_k|, X = sum |x_k| over the receptive field in fp64, x clamped to +-65504; y64 the fp64 result on the
  clamped x.
  * 2^-25 S: the activation split has an ABSOLUTE floor.  hi = fp16(x) is a subnormal fp16 below 2^-14 and lo = fp16(x - hi) is one
    below |x| ~ 2^-2; both then round to a multiple of 2^-24, so |x - hi - lo| <= 2^-25 whatever |x| is.
  * 2^-38 max|w| X: the same floor for a filter far below its bank's maximum -- 2^-25 in scaled units, and 2^wexp max|w| >= 2^13.
  * TAU (A + |b|): while lo is a normal fp16 the split is 2^-23 relative per operand, the dropped lo.lo product 2^-22, and the MFMA
    accumulates in fp32 in the kernel's own order.  TAU = 2e-6 is the constant of the fp32 DCNv2 operator (tests/test_gpu_dcn_domain.py);
    tests/test_oracle_x3_domain.py calibrates it: F.conv2d in fp32 stays below TAU / 4 on every case.
A residual adds TAU |res| (one fp32 addition of the epilogue), ReLU and the clamp are 1-Lipschitz.  Chained kernels (heads: 3x3 -> ReLU ->
1x1; stem3x: 7x7 -> 3x3 -> 3x3 stride 2) propagate the bound: with e the bound of layer n's output, layer n+1 adds sum |w| e and takes
A and X over |x64| + e (`_layer`).  The DeformConv takes A, S and X through the oracle's sampling (oracle.dcn.dcn_v2_forward_absbound) and
adds 2^-22 A for the fp32 blend and the fp32 sigmoid of the mask.

Activations: `uniform` U(-1, 1), `spread` a random sign times 2^U[-12, 0] per element, `regions` U(-1, 1) decaying by 2^-2 every two
columns -- each times an overall scale g of SCALES (the bias and the residual are scaled with the output).  Filters times GAINS."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from h3d_amd import engine, synth, weights
from oracle import dcn as odcn

TAU = 2e-6
FMAX = 65504.0
FLOOR = 2.0 ** -25            # |x - hi - lo| of an activation, absolute
WFLOOR = 2.0 ** -38           # the same for a filter, relative to its bank's maximum
BLEND = 2.0 ** -22            # DeformConv: the bilinear blend and the mask's sigmoid in fp32
SCALES = [2.0 ** -20, 2.0 ** -12, 2.0 ** -6, 1.0, 2.0 ** 10, 2.0 ** 15]
GAINS = [1e-6, 1.0, 3e3]
GENERATORS = ["uniform", "spread", "regions"]
STEM_SCALES = [2.0 ** -12, 1.0, 2.0 ** 10]       # times the first layer's folded BatchNorm scale: the LDS intermediates go small / large
FAST = (3, 3, 1, 1, 1, 1, 1, 1, 1)


def _u(key, shape, lo=-1.0, hi=1.0, seed=0):
    return torch.from_numpy(synth.uniform(key, shape, lo, hi, seed)).double()


# ---- activation generators ---------------------------------------------------------------------------------------------------------
def uniform(g, shape, key="x"):
    return (_u(key, shape) * g).float()


def spread(g, shape, key="x"):
    """per-element exponents uniform in [-12, 0], random sign"""
    return (torch.sign(_u(key + "s", shape)) * 2.0 ** _u(key + "e", shape, -12.0, 0.0) * g).float()


def regions(g, shape, key="x"):
    """U(-1, 1) decaying by 2^-2 every two columns, down to 2^-18 in column 19; a wider map starts over every 20 columns (below that the
    values are lost whole, which the bound admits without saying anything), so it also holds O(1) columns next to the smallest ones"""
    cols = (torch.arange(shape[-1], dtype=torch.float64) % 20) // 2
    return (_u(key, shape) * 2.0 ** (-2.0 * cols) * g).float()


def activation(gen, g, shape, key="x"):
    return {"uniform": uniform, "spread": spread, "regions": regions}[gen](g, shape, key)


# ---- the split arithmetic ------------------------------------------------------------------------------------------------------------
def x3_split_emulated(x):
    """fp32 x -> (clamped x, hi, lo) in fp64: the staging split of csrc/common.h x3_split4 (round to nearest even, fp16 subnormals kept)"""
    xc = x.float().clamp(-FMAX, FMAX)
    hi = xc.half()
    lo = (xc - hi.float()).half()            # (the difference is exact in fp32)
    return xc.double(), hi.double(), lo.double()


def x3_filters(w, e=None, bank=None, unbank=None):
    """Filters [Co,Ci,k,k] -> (hi, lo, e): the (hi | lo) fp16 terms of w * 2^e as the product's packer stores them (engine.x3_exp /
    x3_split on the [Co][taps][Ci] bank, or on `bank(w)` with `unbank` as its inverse), decoded back to fp64 [Co,Ci,k,k]."""
    co, ci, kh, kw = w.shape
    if bank is None:
        assert (ci * kh * kw) % 8 == 0 and ci % 8 == 0
        bank = lambda t: t.permute(0, 2, 3, 1).reshape(co, kh * kw, ci)                        # noqa: E731
        unbank = lambda t: t.reshape(co, kh, kw, ci).permute(0, 3, 1, 2)                       # noqa: E731
    wp = bank(w.float())
    if e is None:
        e = engine.x3_exp(wp)
    raw = engine.x3_split(wp * 2.0 ** e).contiguous().view(torch.float16)                      # [..., 2 K]: per 8 elements 8 hi | 8 lo
    K = wp.shape[-1]
    g = raw.reshape(-1, K // 8, 2, 8)
    hi, lo = g[:, :, 0, :].reshape(wp.shape), g[:, :, 1, :].reshape(wp.shape)
    return unbank(hi).double().contiguous(), unbank(lo).double().contiguous(), e


def _stem_unbank(t):
    co = t.shape[0]
    return t.reshape(co, 7, 8, 4)[:, :, :7, :3].permute(0, 3, 1, 2)


def x3_conv_emulated(x, w, b, stride, pad, res=None, relu=False, drop=None, e=None, stem=False):
    """The f16x3 arithmetic of one convolution on the CPU: clamp, split, the three products hi.hi + hi.lo + lo.hi in fp64 on the packer's
    filter terms, times 2^-wexp, + bias (+ residual), ONE fp32 rounding.  Mutants: drop = "xlo_whi" leaves the x.lo w.hi product out
    altogether, drop = ("xlo_whi", ky, kx, c0) leaves it out of ONE MFMA step (tap (ky, kx), input channels c0 .. c0 + 15)."""
    _, xh, xl = x3_split_emulated(x)
    wh, wl, e = x3_filters(w, e, weights._stem_bank if stem else None, _stem_unbank if stem else None)
    acc = F.conv2d(xh, wh, None, stride, pad) + F.conv2d(xh, wl, None, stride, pad)
    if isinstance(drop, tuple):
        wh = wh.clone()
        wh[:, drop[3]:drop[3] + 16, drop[1], drop[2]] = 0.0
    if drop != "xlo_whi":
        acc = acc + F.conv2d(xl, wh, None, stride, pad)
    y = acc * 2.0 ** -e + b.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    if relu:
        y = F.relu(y)
    return y.float()


# ---- the bound -------------------------------------------------------------------------------------------------------------------------
def _layer(x64, e_in, w, b, stride, pad, wmax=None, res=None, relu=False, floor=True):
    """One contraction of a chain.  x64: the fp64 input of the reference chain; e_in: the bound on |kernel's input - x64| (None: the
    kernel reads x64 itself).  -> (y64, bound on |kernel's output - y64|).  floor=False: the TAU terms alone (what fp32 arithmetic is
    held to: the CPU test's calibration, and its check that the floor terms are needed)."""
    w64 = w.double()
    aw = w64.abs()
    xc = x64.clamp(-FMAX, FMAX)
    ax = xc.abs() if e_in is None else (xc.abs() + e_in).clamp(max=FMAX)      # what the kernel's (clamped) input can be at most
    ones = torch.ones(1, w.shape[1], w.shape[2], w.shape[3], dtype=torch.float64)
    y = F.conv2d(xc, w64, b.double(), stride, pad)
    A = F.conv2d(ax, aw, None, stride, pad)
    S = F.conv2d(torch.ones_like(xc[:1]), aw, None, stride, pad)              # (padding holds exact zeros: no split error there)
    X = F.conv2d(ax, ones, None, stride, pad)
    wmax = float(aw.max()) if wmax is None else wmax
    bound = TAU * (A + b.double().abs().view(1, -1, 1, 1))
    if floor:
        bound = bound + FLOOR * S + WFLOOR * wmax * X
    if e_in is not None:
        bound = bound + F.conv2d(e_in, aw, None, stride, pad)
    if res is not None:
        y = y + res.double()
        bound = bound + TAU * res.double().abs()
    if relu:
        y = F.relu(y)
    return y, bound


def bound_conv(x, w, b, stride, pad, res=None, relu=False, floor=True):
    """-> (y64, bound): the fp64 convolution of the clamped x (+ residual, ReLU) and the element-wise bound of the module docstring"""
    return _layer(x.double(), None, w, b, stride, pad, res=res, relu=relu, floor=floor)


HEADS = {"hm": 1, "hps": 34, "pose": 72, "wh": 2}
HEAD_GROUPS = (("hm", "wh"), ("hps",), ("pose",))      # one launch per number of 32-row output tiles, as engine.Plan._lower_heads


def _head_group(h):
    return [g for g in HEAD_GROUPS if h in g][0]


def bound_heads(x, sd, floor=True):
    """{head: (y64, bound)} of Conv3x3(64 -> 256) + ReLU -> Conv1x1(256 -> C): the 3x3 banks of one launch share one exponent, so the
    filter floor of the first layer is relative to the launch's largest 3x3 filter"""
    out = {}
    for h in HEADS:
        wmax1 = max(float(sd[n + ".0.weight"].abs().max()) for n in _head_group(h))
        t, e1 = _layer(x.double(), None, sd[h + ".0.weight"], sd[h + ".0.bias"], 1, 1, wmax=wmax1, relu=True, floor=floor)
        out[h] = _layer(t, e1, sd[h + ".2.weight"], sd[h + ".2.bias"], 1, 0, floor=floor)
    return out


def heads_emulated(x, sd, drop=None):
    out = {}
    for h in HEADS:
        e1 = engine.x3_exp(torch.cat([weights.pack_head_3x3(sd[n + ".0.weight"]) for n in _head_group(h)]))
        t = x3_conv_emulated(x, sd[h + ".0.weight"], sd[h + ".0.bias"], 1, 1, relu=True, drop=drop, e=e1)
        out[h] = x3_conv_emulated(t, sd[h + ".2.weight"], sd[h + ".2.bias"], 1, 0, drop=drop)
    return out


STEM_LAYERS = (("base.base_layer", 7, 1), ("base.level0", 3, 1), ("base.level1", 3, 2))


def stem_folded(sd):
    """[(w, b, k, stride)] of the three layers with their BatchNorm folded by the product's packer"""
    pw = engine.PackedWeights.from_tensors(sd, "f16x3", "cpu")
    return [pw._fold(sd[n + ".0.weight"], None, n + ".1") + (k, s) for n, k, s in STEM_LAYERS]


def bound_stem3(x, sd, floor=True):
    """-> (y64, bound) of the fused stem: each intermediate is clamped and split as it goes into LDS, zero outside the image"""
    t, e = x.double(), None
    for w, b, k, s in stem_folded(sd):
        t, e = _layer(t, e, w, b, s, k // 2, relu=True, floor=floor)
    return t, e


def stem3_emulated(x, sd, drop=None):
    t = x
    for i, (w, b, k, s) in enumerate(stem_folded(sd)):
        t = x3_conv_emulated(t, w, b, s, k // 2, relu=True, drop=drop, stem=i == 0)
    return t


def _const_maps(off18, mlogit, B, H, W):
    off = off18.double().view(1, 18, 1, 1).expand(B, 18, H, W).contiguous()
    m = torch.sigmoid(mlogit.double()).view(1, 9, 1, 1).expand(B, 9, H, W).contiguous()
    return off, m


def bound_dcn(x, w, b, off18, mlogit, floor=True):
    """Fused DeformConv (+ ReLU) whose conv_offset_mask has ZERO filters: offsets (off18[2 t], off18[2 t + 1]) and mask logit mlogit[t]
    are constants per tap, exact and independent of x.  A from oracle.dcn.dcn_v2_forward_absbound, S = sum |w| mask and X = sum |column|
    through the same sampling, + 2^-22 A for the fp32 blend.  -> (y64, bound)"""
    B, C, H, W = x.shape
    off, m = _const_maps(off18, mlogit, B, H, W)
    xc = x.double().clamp(-FMAX, FMAX)
    y = odcn.dcn_v2_forward(xc, w.double(), b.double(), off, m, *FAST)
    A = odcn.dcn_v2_forward_absbound(xc, w, off, m, *FAST)
    S = odcn.dcn_v2_forward_absbound(torch.ones_like(xc[:1]), w, off[:1], m[:1], *FAST)
    X = odcn.dcn_v2_forward_absbound(xc, torch.ones(1, C, 3, 3), off, m, *FAST)
    bound = (TAU + BLEND) * A + TAU * b.double().abs().view(1, -1, 1, 1)
    if floor:
        bound = bound + FLOOR * S + WFLOOR * float(w.abs().max()) * X
    return F.relu(y), bound


def dcn_columns(x64, off, m):
    """[B, C * 9, H * W]: the sampled, masked columns of the oracle (an identity filter bank reads them out)"""
    B, C, H, W = x64.shape
    eye = torch.eye(C * 9, dtype=torch.float64).view(C * 9, C, 3, 3)
    return odcn.dcn_v2_forward(x64, eye, torch.zeros(C * 9, dtype=torch.float64), off, m, *FAST).reshape(B, C * 9, H * W)


def dcn_emulated(x, w, b, off18, mlogit, drop=None):
    """The f16x3 DeformConv on the CPU: columns blended in fp64 from the clamped x and rounded ONCE to fp32 (the kernel's sample), split,
    three products against the packer's filter terms, 2^-wexp, + bias, one fp32 rounding, ReLU"""
    B, C, H, W = x.shape
    off, m = _const_maps(off18, mlogit, B, H, W)
    cols = dcn_columns(x.double().clamp(-FMAX, FMAX), off, m).float()
    _, ch, cl = x3_split_emulated(cols)
    wh, wl, e = x3_filters(w)
    wh, wl = wh.reshape(w.shape[0], -1), wl.reshape(w.shape[0], -1)
    acc = torch.matmul(wh, ch) + torch.matmul(wl, ch)
    if drop != "xlo_whi":
        acc = acc + torch.matmul(wh, cl)
    y = acc * 2.0 ** -e + b.double().view(1, -1, 1)
    return F.relu(y).float().view(B, -1, H, W)


# ---- DeformConv sample geometry (csrc/dcn3.hip): which path serves each (pixel, tap) ---------------------------------------------------
GATED, APRON, PATCH, PASS2 = 0, 1, 2, 3


def dcn_sample_paths(H, W, margin, slots, off18):
    """int8 [H, W, 9]: the path of every sample under constant per-tap offsets.  A 16 x 16 tile stages an apron of `margin` + 1 pixels
    around itself; a sample inside the image whose low corner leaves rows / columns [-margin - 1, 15 + margin] of the tile is FAR: it
    takes one of the tile's `slots` patch slots in (wave, tap u = 0..4, lane) order -- wave = 2 tile rows, lanes 0..31 hold tap u of the
    wave's 32 pixels, lanes 32..63 tap 5 + u -- and goes through pass 2 once they are used up (slots = 0: always)."""
    off = off18.float()
    cls = np.zeros((H, W, 9), np.int8)
    for ty in range(0, H, 16):
        for tx in range(0, W, 16):
            n = 0
            for wv in range(8):
                for u in range(5):
                    for lane in range(64):
                        r, hh = lane & 31, lane >> 5
                        if hh and u == 4:
                            continue
                        tap = 5 * hh + u
                        oy, ox = ty + 2 * wv + (r >> 4), tx + (r & 15)
                        if oy >= H or ox >= W:
                            continue
                        h_im = float(torch.tensor(float(oy - 1 + tap // 3)) + off[2 * tap])
                        w_im = float(torch.tensor(float(ox - 1 + tap % 3)) + off[2 * tap + 1])
                        if not (h_im > -1 and w_im > -1 and h_im < H and w_im < W):
                            continue
                        ry, rx = int(np.floor(h_im)) - (ty - 1 - margin), int(np.floor(w_im)) - (tx - 1 - margin)
                        hh_ = 16 + 2 + 2 * margin
                        if 0 <= ry < hh_ - 1 and 0 <= rx < hh_ - 1:
                            cls[oy, ox, tap] = APRON
                        elif n < slots:
                            cls[oy, ox, tap] = PATCH
                            n += 1
                        else:
                            cls[oy, ox, tap] = PASS2
                            n += 1
    return cls


def dcn_reach(ind, off18, mlogit, paths=None, which=None):
    """bool [B, 1, H, W]: outputs with a nonzero-weight corner on an element of the indicator `ind` [B, C, H, W] -- through every
    sample, or only through the samples whose entry of `paths` (dcn_sample_paths) is in `which`"""
    B, C, H, W = ind.shape
    off, m = _const_maps(off18, mlogit, B, H, W)
    if paths is not None:
        sel = torch.from_numpy(np.isin(paths, which)).permute(2, 0, 1).double()         # [9, H, W]
        m = m * sel.unsqueeze(0)
    return odcn.dcn_v2_forward_absbound(ind.double(), torch.ones(1, C, 3, 3), off, m, *FAST) > 0


def dcn_far_elements(c):
    """[(b, c, y, x)]: per far path of case `c` (patch slots, pass 2) the low corner, inside the image, of the first sample on that path --
    activations the out-of-range tests overwrite on purpose"""
    kind, B, Ci, Co, H, W, ov, oname, margin, slots, _ = c
    off = OFFSETS[oname]
    paths = dcn_sample_paths(H, W, margin, slots, off18_of(oname))
    out = []
    for p in (PATCH, PASS2):
        for oy, ox, tap in np.argwhere(paths == p):
            y, x = int(np.floor(oy - 1 + tap // 3 + off[tap][0])), int(np.floor(ox - 1 + tap % 3 + off[tap][1]))
            if 0 <= y < H and 0 <= x < W:
                out.append((0, (7 * len(out) + 5) % Ci, y, x))
                break
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
CONV_CASES = [
    # (B, Cin, Cout, H, W, k, stride, residual + ReLU)
    (2, 64, 64, 16, 20, 3, 1, False),       # partial tile
    (2, 64, 64, 16, 20, 3, 1, True),
    (1, 128, 192, 32, 40, 3, 1, False),     # 32-row tiles, two N-tiles per wave
    (1, 128, 192, 32, 40, 3, 1, True),
    (1, 64, 128, 24, 24, 3, 2, False),      # stride 2
    (1, 64, 128, 24, 24, 3, 2, True),
    (1, 128, 64, 13, 21, 1, 1, False),      # 1x1, odd map
]
HEADS_SHAPES = [(1, 13, 21), (1, 16, 32)]
STEM_SHAPES = [(1, 45, 72), (1, 16, 32)]
# offsets per tap (dh, dw): dyadic neighbours of +-0.75, +-3.3 and +-7.6 (3 5/16, 7 5/8), so that the sampling positions and the bilinear
# weights are exact in fp32 and in fp64 alike and the comparison holds no geometry term; every weight of every sample is nonzero
N_, M_, F_ = 0.75, 3.3125, 7.625
OFFSETS = {
    # taps pushed outwards: the top row up / left, the bottom row down / right -- samples in the apron, beyond it, and outside the image
    "mixed": [(-M_, -N_), (-F_, N_), (N_, F_), (N_, -M_), (N_, -N_), (-N_, M_), (M_, -N_), (F_, N_), (N_, M_)],
    # few far samples: every tile of the 24 x 40 map keeps within its 256 patch slots, two tiles go into the second fill round (> 128)
    "few": [(-M_, -N_), (-N_, N_), (N_, N_), (N_, -M_), (N_, -N_), (-N_, M_), (M_, -N_), (F_, N_), (N_, N_)],
    # more far samples than a tile has patch slots
    "far": [(-F_, -F_), (-F_, N_), (-M_, F_), (N_, -F_), (-N_, N_), (N_, F_), (F_, -M_), (F_, N_), (F_, F_)],
}
MASK_LOGITS = [-2.0, 0.0, 3.0, 0.0, 3.0, -2.0, 3.0, -2.0, 0.0]
DCN_CASES = [
    # (kind, B, Cin, Cout, H, W, margin override, offsets, expected apron margin, patch slots, paths its samples take besides GATED)
    ("fused", 1, 64, 64, 20, 24, 2, "mixed", 2, 0, (APRON, PASS2)),
    ("fused", 1, 64, 64, 20, 24, 6, "mixed", 6, 0, (APRON, PASS2)),
    ("fused", 1, 256, 128, 16, 16, 2, "mixed", 2, 0, (APRON,)),        # (a 16 x 16 map lies inside every apron: two channel groups,
    ("fused", 1, 256, 128, 16, 16, 6, "mixed", 6, 0, (APRON,)),        #  two 64-channel workgroups)
    ("stream", 1, 128, 64, 24, 40, 0, "few", 2, 256, (APRON, PATCH)),              # patches only
    ("stream", 1, 64, 64, 40, 24, 0, "far", 2, 256, (APRON, PATCH, PASS2)),       # patches AND pass 2
    ("stream", 1, 256, 256, 16, 16, 0, "mixed", 4, 256, (APRON,)),                # margin 4 (Cin == Cout > 64), grid.y = 4
]


def conv_id(c):
    return "%dx%d-%dx%d-k%d-s%d%s" % (c[1], c[2], c[3], c[4], c[5], c[6], "-res-relu" if c[7] else "")


def dcn_id(c):
    return "%s-%dx%d-%dx%d-m%d-%s" % (c[0], c[2], c[3], c[4], c[5], c[8], c[7])


def off18_of(name):
    return torch.tensor([v for pair in OFFSETS[name] for v in pair], dtype=torch.float32)


def conv_out_hw(c):
    k, s = c[5], c[6]
    return (c[3] + 2 * (k // 2) - k) // s + 1, (c[4] + 2 * (k // 2) - k) // s + 1


def conv_operands(c, gen, g, gain):
    """x at g, filters at gain, bias and residual at the output's scale g * gain"""
    B, Ci, Co, H, W, k, s, rr = c
    x = activation(gen, g, (B, Ci, H, W))
    w = (_u("w", (Co, Ci, k, k)) * (1.5 / np.sqrt(Ci * k * k)) * gain).float()
    b = (_u("b", (Co,)) * g * gain).float()
    res = (_u("r", (B, Co) + conv_out_hw(c)) * g * gain).float() if rr else None
    return x, w, b, res


def heads_operands(shape, gen, g, gain):
    """The four multi_pose heads on a 64-channel map at g; both layers' filters at gain, each bias at its layer's output scale"""
    B, H, W = shape
    sd = {}
    for h, c in HEADS.items():
        sd[h + ".0.weight"] = (_u(h + "w1", (256, 64, 3, 3)) * (1.6 / np.sqrt(64 * 9)) * gain).float()
        sd[h + ".0.bias"] = (_u(h + "b1", (256,), -0.2, 0.2) * g * gain).float()
        sd[h + ".2.weight"] = (_u(h + "w2", (c, 256, 1, 1)) * (1.6 / np.sqrt(256)) * gain).float()
        sd[h + ".2.bias"] = (_u(h + "b2", (c,), -0.5, 0.5) * g * gain * gain).float()
    return activation(gen, g, (B, 64, H, W), "feat"), sd


def stem_operands(shape, s, gain):
    """Image in [-3, 3]; the state dict of test_fused_stem_op_matches_torch with layer n's folded filters times f_n (f_1 = s * gain,
    f_2 = f_3 = gain) and its folded bias at its output's scale F_n = f_1 ... f_n: BatchNorm weight * f_n, bias * F_n, mean * F_(n-1)"""
    B, H, W = shape
    sd, Fp = {}, 1.0
    for i, (name, (co, ci, k)) in enumerate((("base.base_layer", (16, 3, 7)), ("base.level0", (16, 16, 3)), ("base.level1", (32, 16, 3)))):
        f = gain * (s if i == 0 else 1.0)
        sd[name + ".0.weight"] = (_u(name + "w", (co, ci, k, k)) * (1.8 / np.sqrt(ci * k * k))).float()
        sd[name + ".1.weight"] = (_u(name + "g", (co,), 0.6, 1.4) * f).float()
        sd[name + ".1.bias"] = (_u(name + "b", (co,), -0.3, 0.3) * Fp * f).float()
        sd[name + ".1.running_mean"] = (_u(name + "m", (co,), -0.2, 0.2) * Fp).float()
        sd[name + ".1.running_var"] = _u(name + "v", (co,), 0.5, 1.5).float()
        Fp *= f
    return _u("img", (B, 3, H, W), -3.0, 3.0).float(), sd


def dcn_operands(c, gen, g, gain):
    """-> x, (w, b) as given to the packer, (wf, bf) with the identity BatchNorm folded as the packer folds it, off18, mask logits"""
    kind, B, Ci, Co, H, W = c[:6]
    x = activation(gen, g, (B, Ci, H, W))
    w = (_u("w", (Co, Ci, 3, 3)) * (1.5 / np.sqrt(Ci * 9)) * gain).float()
    b = (_u("b", (Co,)) * g * gain).float()
    sd = {"p.actf.0.weight": torch.ones(Co), "p.actf.0.bias": torch.zeros(Co), "p.actf.0.running_mean": torch.zeros(Co),
          "p.actf.0.running_var": torch.full((Co,), 1.0 - 1e-5)}
    wf, bf = engine.PackedWeights.from_tensors(sd, "f16x3", "cpu")._fold(w, b, "p.actf.0")
    return x, (w, b), (wf, bf), off18_of(c[7]), torch.tensor(MASK_LOGITS)


# ---- out-of-range and non-finite activations ------------------------------------------------------------------------------------------
BIG = [1e5, 3e38, -3e38]
NONFINITE = [float("inf"), float("-inf"), float("nan")]


CORNERS = ((0, 0), (7, 15), (8, 16), (15, 15), (16, 16), (7, 31), (15, 31))      # corners of the kernels' 8 x 16, 16 x 16, 32 x 16 and 8 x 32 tiles


def poison(x, values, share=0.01, extra=()):
    """A copy of x with one channel of about `share` of its pixels (at least 4) overwritten by `values` in turn, among them the tile corners
    CORNERS and the last pixel where the map has them, and the elements (b, c, y, x) of `extra`.  -> (copy, bool indicator).  (One
    element per pixel: the outputs that see none of them are the ones the non-finite tests can still compare.)"""
    B, C, H, W = x.shape
    r = np.random.default_rng(11)
    n = max(4, int(B * H * W * share))
    idx = np.stack([r.integers(0, d, n) for d in (B, C, H, W)], 1).tolist()
    for y_, x_ in CORNERS + ((H - 1, W - 1),):
        if y_ < H and x_ < W:
            idx.append([int(r.integers(0, B)), int(r.integers(0, C)), y_, x_])
    idx += [list(e) for e in extra]
    out, ind = x.clone(), torch.zeros(x.shape, dtype=torch.bool)
    for i, p in enumerate(idx):
        out[tuple(p)] = values[i % len(values)]
        ind[tuple(p)] = True
    return out, ind


def conv_reach(ind, k, stride):
    """bool [B, 1, Ho, Wo]: outputs whose k x k receptive field holds an element of `ind`"""
    C = ind.shape[1]
    return F.conv2d(ind.double(), torch.ones(1, C, k, k, dtype=torch.float64), None, stride, k // 2) > 0


def stem_reach(ind):
    t = ind
    for _, k, s in STEM_LAYERS:
        t = conv_reach(t, k, s)
    return t


# ---- shared references: computed once per process, never modified ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_reference(ci, gen, g, gain):
    x, w, b, res = conv_operands(CONV_CASES[ci], gen, g, gain)
    c = CONV_CASES[ci]
    return (x, w, b, res) + bound_conv(x, w, b, c[6], c[5] // 2, res, c[7])


def report(tag, got, y64, bound, tile=(16, 16), where=None):
    """worst err / bound over the elements of `where` (default: all); on a violation the message holds its position and its tile"""
    err = (got.double() - y64).abs()
    ratio = err / bound
    if where is not None:
        ratio = torch.where(where.expand_as(ratio), ratio, torch.zeros((), dtype=ratio.dtype))
    ratio = torch.where(torch.isnan(ratio), torch.full((), float("inf"), dtype=ratio.dtype), ratio)
    worst = float(ratio.max())
    msg = ""
    if not worst <= 1.0:
        pos = np.unravel_index(int(ratio.argmax()), ratio.shape)
        msg = "%s: worst err / bound = %.3g at (b, c, y, x) = %s, %d x %d tile (%d, %d): got %.9g, fp64 %.9g, bound %.3g; %d of %d elements over" % (
            tag, worst, tuple(int(p) for p in pos), tile[0], tile[1], pos[2] // tile[0], pos[3] // tile[1], float(got[pos]), float(y64[pos]),
            float(bound[pos]), int((ratio > 1.0).sum()), ratio.numel())
    return worst, msg
