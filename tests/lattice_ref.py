"""Integer-lattice operands and exact references for the forward matrix-core ops (conv, gemm1, conv2, stems, heads, up-sample + add,
fused DeformConv).  CPU only: nothing here loads the HIP library.

Why a lattice: with x in {-3..3} and w in {-1, 0, 1} * 2^e every product is exact in bf16, fp16, fp32 and as an f16x3 hi/lo split
(lo = 0; the filter pre-scale is a power of two), every fp32 partial sum is an integer (times a fixed power of two) far below 2^24,
so the accumulation is exact in ANY order, and the only rounding left is the one round-to-nearest-even into the storage type where the
kernel stores.  The comparison is then torch.equal(kernel, round(fp64 reference)): a dropped, duplicated or misplaced tap, a wrong halo
pixel or a channel read from its neighbour changes most of the pixels it touches instead of hiding under a 2^-8 * max|ref| tolerance.

tests/test_oracle_lattice.py pins the conditions above for every case tests/test_gpu_lattice.py runs.

The up-sample + add FOLDED into the DeformConv that writes its skip has its reference here too (`fold_operands`, `exact_fold`, the
loop-form `fold_restated` with four defects of the folding tail): tests/test_gpu_upadd_fold.py runs it, tests/test_oracle_upadd_fold.py
pins its conditions.

The DeformConv also runs on a QUARTER-PIXEL lattice (the last two sections): sampling positions on k/4 and dyadic masks keep the bilinear
blend exact, for the fused plan kernels (`dcn_frac_operands`) and for the fp32 operator and its backward (`dcn_grid_case`,
tests/test_gpu_dcn_lattice.py; conditions in tests/test_oracle_dcn_backward.py)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import h3d_amd  # noqa: F401
from h3d_amd import synth

TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f16x3": torch.float32}
EXACT_RANGE = {"bf16": 256.0, "f16": 2048.0}        # integers up to here are representable (8 / 11 significand bits)
RELU_SHIFT_SIGMAS = 0.8                             # bias shift in standard deviations: a normal output clips Phi(-0.8) = 21 %
RELU_CLIP = (0.05, 0.40)
MAX_OUTSIDE = 0.02
W_DENSITY = 2.0 / 3.0
W_DENSITY_K = 1536.0                                # contractions longer than 2304 get sparser filters: density = min(2/3, 1536 / K)


def lowp_round(t, dtype):
    """One round-to-nearest-even into the plan's storage type (f32 / f16x3 store fp32: unchanged)."""
    t = t.float()
    return t if dtype in ("f32", "f16x3") else t.to(TD[dtype]).float()


def round_to(t, store):
    """One round-to-nearest-even of an fp64 (or fp32) tensor into the torch dtype `store`, back as fp32: for ops whose stored type is not
    the plan's (H3D_OUT_NHWC_F16 in a bf16 plan).  The lattice values are exact in fp32, so the conversion rounds once whichever way torch
    takes from fp64."""
    return t.to(store).float()


def _ints(key, shape, lo, hi):
    """Uniform integers in [lo, hi], a pure function of (key, shape)."""
    n = hi - lo + 1
    u = synth.uniform01(key, tuple(shape))
    return torch.from_numpy((np.minimum(np.floor(u * n), n - 1) + lo).astype(np.float32))


def lattice_x(shape, key="lx"):
    return _ints(key, shape, -3, 3)


def lattice_w(shape, key="lw", exp=0, density=None):
    """Filters in {-1, 0, 1} * 2^exp; `density` = share of non-zero taps (default: 2/3, less for contractions beyond 2304 terms so that
    the outputs stay inside the exactly representable range of bf16)."""
    K = int(np.prod(shape[1:]))
    d = min(W_DENSITY, W_DENSITY_K / K) if density is None else density
    u = torch.from_numpy(synth.uniform01(key, tuple(shape)))
    w = torch.zeros(tuple(shape), dtype=torch.float64)
    w[u < d / 2] = -1.0
    w[u >= 1.0 - d / 2] = 1.0
    return (w * 2.0 ** exp).float()


def lattice_bias(co, key="lb"):
    return _ints(key, (co,), -4, 4)


def lattice_res(shape, key="lr"):
    return _ints(key, shape, -8, 8)


def lattice_image(shape, key="limg"):
    """The stems' fp32 image on the grid k/256 in [-2, 2): 9 significand bits, so the kernel's own conversion to bf16 rounds (ties
    included); exact in fp16 and as an f16x3 split."""
    return _ints(key, shape, -512, 511) / 256.0


def lattice_up_w(shape, key="lup"):
    """Depthwise transposed-conv (bilinear-like) weights on the grid k/8 in [0, 1]."""
    return _ints(key, shape, 0, 8) / 8.0


def pre_conv(x, w, b=None, stride=1, pad=0, res=None):
    """fp64 conv + bias + residual, before ReLU and rounding."""
    y = F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride, pad)
    return y if res is None else y + res.double()


def relu_shift(pre, sigmas=RELU_SHIFT_SIGMAS):
    """Integer bias shift that moves a zero-centred output up by 0.8 of the reference's own standard deviation, so that ReLU clips about
    a fifth of the outputs instead of half of them."""
    return float(int(round(sigmas * float(pre.double().std()))))


def exact_conv(x, w, b=None, stride=1, pad=0, relu=False, res=None, dtype="f32"):
    """The op's result as the kernel must store it: fp64 conv + bias + residual + ReLU, rounded ONCE to the plan's storage type."""
    y = pre_conv(x, w, b, stride, pad, res)
    return lowp_round(F.relu(y) if relu else y, dtype)


def conditions(x, w, b=None, stride=1, pad=0, res=None, unit=1.0):
    """What makes a zero tolerance legitimate for one contraction, measured on the CPU:
         fp32_exact   fp32 F.conv2d (+ bias, residual) equals the fp64 result bit for bit
         max_units    max over outputs of (sum |x| |w| + |b| + |res|) / unit -- every fp32 partial sum, in any order, is an integer
                      number of `unit`s of at most this size (must stay below 2^24)
         outside      {dtype: share of pre-rounding outputs beyond the exactly representable range}
         pre          the fp64 result (before ReLU)"""
    pre = pre_conv(x, w, b, stride, pad, res)
    y32 = F.conv2d(x.float(), w.float(), None if b is None else b.float(), stride, pad)
    if res is not None:
        y32 = y32 + res.float()
    bound = F.conv2d(x.double().abs(), w.double().abs(), None if b is None else b.double().abs(), stride, pad)
    if res is not None:
        bound = bound + res.double().abs()
    units = pre / unit
    return {"fp32_exact": torch.equal(y32.double(), pre), "max_units": float(bound.max()) / unit,
            "on_grid": bool((units == units.round()).all()),
            "outside": {d: float((pre.abs() > r * unit).double().mean()) for d, r in EXACT_RANGE.items()}, "pre": pre}


def clipped_share(pre):
    return float((pre <= 0).double().mean())


# ---- operands per family ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_operands(B, Ci, Co, H, W, k, stride, relu, use_res):
    """(x, w, b, res) of one conv case; with ReLU the bias carries the shift of `relu_shift`.  Identical for every arithmetic: the
    lattice is exact in all of them."""
    x = lattice_x((B, Ci, H, W))
    w = lattice_w((Co, Ci, k, k))
    b = lattice_bias(Co)
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    res = lattice_res((B, Co, Ho, Wo)) if use_res else None
    if relu:
        b = b + relu_shift(pre_conv(x, w, b, stride, k // 2, res))
    return x, w, b, res


@functools.lru_cache(maxsize=None)
def stem_operands(B, Co, H, W, stride):
    """(image on k/256, w [Co,3,7,7], b) of a 7x7 stem + ReLU."""
    x = lattice_image((B, 3, H, W))
    w = lattice_w((Co, 3, 7, 7), "lws")
    b = lattice_bias(Co, "lbs")
    return x, w, b + relu_shift(pre_conv(x, w, b, stride, 3))


def exact_stem(x, w, b, stride, dtype):
    """7x7 stem + ReLU: the kernel converts the fp32 image to the plan's 2-byte type itself (round to nearest even)."""
    return exact_conv(lowp_round(x, dtype), w, b, stride, 3, True, None, dtype)


STEM3_LAYERS = (("base.base_layer", 16, 3, 7, 1, 0), ("base.level0", 16, 16, 3, 1, -3), ("base.level1", 32, 16, 3, 2, -3))
#                 name, Cout, Cin, k, stride, filter exponent: 2^-3 keeps level0 / level1 near the magnitude of the layer before


def identity_bn(prefix, b):
    """Eval BatchNorm that only adds `b`: gamma 1, mean 0, var 1 - eps (tests/gpu_helpers._dcn_sd)."""
    co = b.shape[0]
    return {prefix + ".weight": torch.ones(co), prefix + ".bias": b.clone(), prefix + ".running_mean": torch.zeros(co),
            prefix + ".running_var": torch.full((co,), 1.0 - 1e-5)}


@functools.lru_cache(maxsize=None)
def stem3_operands(B, H, W):
    """(image, state dict of the three conv + BatchNorm layers, [(w, b, k, stride)]) of the fused stem.  The bias shifts come from the
    unrounded (fp32-plan) chain; the 2-byte chains clip the same share within a fraction of a percent (test_oracle_lattice)."""
    x = lattice_image((B, 3, H, W))
    sd, layers, t = {}, [], x.double()
    for name, co, ci, k, s, e in STEM3_LAYERS:
        w = lattice_w((co, ci, k, k), name + "w", e)
        b = lattice_bias(co, name + "b")
        b = b + relu_shift(pre_conv(t, w, b, s, k // 2))
        t = F.relu(pre_conv(t, w, b, s, k // 2))
        sd[name + ".0.weight"] = w
        sd.update(identity_bn(name + ".1", b))
        layers.append((w, b, k, s))
    return x, sd, layers


def stem3_chain(x, layers, dtype):
    """[(input as the layer reads it, w, b, k, stride)] of the fused stem: the 2-byte plans round the image and both intermediates
    to the storage type (csrc/stem3.hip keeps them in LDS as bf16 / fp16); fp32 and f16x3 plans round nothing."""
    t, out = lowp_round(x, dtype), []
    for w, b, k, s in layers:
        out.append((t, w, b, k, s))
        t = exact_conv(t, w, b, s, k // 2, True, None, dtype)
    return out, t


def exact_stem3(x, layers, dtype):
    return stem3_chain(x, layers, dtype)[1]


HEADS = {"hm": 1, "hps": 34, "pose": 72, "wh": 2}


@functools.lru_cache(maxsize=None)
def heads_operands(B, H, W):
    """(feature map, state dict) of the fused heads: Conv3x3(64 -> 256) + bias + ReLU -> Conv1x1(256 -> C) + bias per head."""
    x = lattice_x((B, 64, H, W), "lfeat")
    sd = {}
    for h, c in HEADS.items():
        w1 = lattice_w((256, 64, 3, 3), h + "w1")
        b1 = lattice_bias(256, h + "b1")
        sd[h + ".0.weight"] = w1
        sd[h + ".0.bias"] = b1 + relu_shift(pre_conv(x, w1, b1, 1, 1))
        sd[h + ".2.weight"] = lattice_w((c, 256, 1, 1), h + "w2")
        sd[h + ".2.bias"] = lattice_bias(c, h + "b2")
    return x, sd


def heads_intermediate(x, sd, h, dtype):
    """The 256-channel intermediate as the 1x1 conv reads it: rounded to the storage type in bf16 / fp16 plans only (csrc/heads.hip
    hands it back to the matrix core in the plan's operand type; f32 / f16x3 keep fp32)."""
    return exact_conv(x, sd[h + ".0.weight"], sd[h + ".0.bias"], 1, 1, True, None, dtype)


def exact_head(x, sd, h, dtype):
    """fp32 output map of head `h` (never rounded: the heads write fp32 in every plan)."""
    return pre_conv(heads_intermediate(x, sd, h, dtype), sd[h + ".2.weight"], sd[h + ".2.bias"]).float()


@functools.lru_cache(maxsize=None)
def upadd_operands(B, C, h, w, f):
    x = lattice_x((B, C, h, w), "lu")
    skip = lattice_res((B, C, h * f, w * f), "ls")
    return x, skip, lattice_up_w((C, 1, 2 * f, 2 * f))


def exact_upadd(x, skip, w, f, dtype):
    y = F.conv_transpose2d(x.double(), w.double(), None, stride=f, padding=f // 2, groups=x.shape[1]) + skip.double()
    return lowp_round(y, dtype)


# ---- up-sample + add folded into the DeformConv that writes its skip (H3D_OPF_UPADD_FOLDED) ---------------------------------------------
# out = round_out( up(x_lo) + round_node( relu(dcn_pre) ) ): the node value is rounded to the plan's type where the kernel packs it into
# LDS, the sum once more to the stored type (bf16 -> bf16, bf16 -> fp16 with H3D_OUT_NHWC_F16, fp16 -> fp16).  x_lo in -3..3, taps on k/8,
# node values integers: every product and every partial sum is a multiple of 1/8 below 2^10, exact in fp32 in any order.
FOLD_DEFECTS = ("swap_rx_ry", "clamp_border", "group0_taps", "image0_map")
FOLD_UNIT = 1.0 / 8.0


def fold_operands(B, Ci, Co, H, W, f):
    """(x, w, b, wo, bo, x_lo, w_up): the producer operands of `dcn_operands(B, Ci, Co, H, W)`, then the low-resolution map [B, Co, H/f, W/f]
    and the depthwise taps [Co, 1, 2f, 2f] of `upadd_operands(B, Co, H // f, W // f, f)` (whose `skip` is not used: the skip is the producer's
    result)."""
    x_lo, _, w_up = upadd_operands(B, Co, H // f, W // f, f)
    return dcn_operands(B, Ci, Co, H, W) + (x_lo, w_up)


@functools.lru_cache(maxsize=None)
def fold_pre(B, Ci, Co, H, W):
    """fp64 DeformConv output before ReLU of `dcn_operands(B, Ci, Co, H, W)`; computed once per producer shape."""
    return dcn_pre(*dcn_operands(B, Ci, Co, H, W))


def fold_node(pre, node_dtype):
    """The producer's own result as the kernel holds it before the add: ReLU, rounded once to the plan's type."""
    return round_to(F.relu(pre.double()), node_dtype)


def exact_fold(x_lo, w_up, pre, f, node_dtype, out_dtype):
    """The folded pair's output: fp64 depthwise transposed conv of the low-resolution map + the rounded node value, rounded once to the
    stored type.  node_dtype / out_dtype: torch dtypes."""
    up = F.conv_transpose2d(x_lo.double(), w_up.double(), None, stride=f, padding=f // 2, groups=x_lo.shape[1])
    return round_to(up + fold_node(pre, node_dtype).double(), out_dtype)


def fold_restated(x_lo, w_up, pre, f, node_dtype, out_dtype, defect=None, acc_dtype=torch.float64, rounded=True):
    """`exact_fold` restated the way the kernels walk it (csrc/epilogue.h upadd_vec): per output pixel the two contributing rows and columns
    iy0 - a, ix0 - c2 with iy0 = (oy + f/2) / f, their table rows (ry + a f) * 2f + rx + c2 f with ry = (oy + f/2) % f, acc = 0, the valid taps
    (a, c2) ascending as acc += w * x (an invalid tap is skipped), then + node -- equal to `exact_fold` bit for bit (in fp32 too:
    acc_dtype=torch.float32; a lattice product is exact, so a fused multiply-add gives the same) -- with one defect on request:
      swap_rx_ry    ry and rx exchanged in the tap-table index;
      clamp_border  an invalid border tap is read from the clamped pixel instead of being skipped;
      group0_taps   channels >= 64 use the tap rows of channel c - 64 (a workgroup's cout0 left out of the table offset);
      image0_map    images b > 0 read image 0 of the low-resolution map (the per-image base left out).
    rounded=False: the sum before the final rounding, in acc_dtype."""
    assert defect is None or defect in FOLD_DEFECTS, defect
    B, C, h, w = x_lo.shape
    k, p = 2 * f, f // 2
    oy, ox = torch.arange(h * f), torch.arange(w * f)
    ry, iy0, rx, ix0 = (oy + p) % f, (oy + p) // f, (ox + p) % f, (ox + p) // f
    table = w_up.to(acc_dtype).reshape(C, k, k)
    if defect == "group0_taps":
        table = torch.cat([table[:64]] + [table[c0 - 64:c0 - 64 + min(64, C - c0)] for c0 in range(64, C, 64)])
    xs = x_lo.to(acc_dtype)
    if defect == "image0_map":
        xs = xs[:1].expand(B, C, h, w)
    acc = torch.zeros(B, C, h * f, w * f, dtype=acc_dtype)
    for a in range(2):
        for c2 in range(2):
            iy, ix, ki, kj = iy0 - a, ix0 - c2, ry + a * f, rx + c2 * f
            ok = ((iy >= 0) & (iy < h)).view(-1, 1) & ((ix >= 0) & (ix < w)).view(1, -1)
            if defect == "clamp_border":
                ok = torch.ones_like(ok)
            xv = xs[:, :, iy.clamp(0, h - 1)][:, :, :, ix.clamp(0, w - 1)]
            if defect == "swap_rx_ry":
                wt = table[:, rx + a * f][:, :, ry + c2 * f].transpose(1, 2)         # row index from the column's phase and the reverse
            else:
                wt = table[:, ki][:, :, kj]
            acc = torch.where(ok.view(1, 1, h * f, w * f), acc + wt.unsqueeze(0) * xv, acc)
    acc = acc + fold_node(pre, node_dtype).to(acc_dtype)
    return round_to(acc, out_dtype) if rounded else acc


@functools.lru_cache(maxsize=None)
def fold_chain_operands(Ci, Co):
    """(w, b, wo, bo) of a DeformConv that READS a folded pair's output (multiples of 1/8, no integers): zero offset filters and integer
    offset biases in -2..2, so every pixel of a tap samples at the same integer displacement whatever the input holds, bilinear weights 0
    or 1, masks as in `dcn_operands`.  A sample is then an input value itself (exact in the fp16 blend), and the contraction with w in
    {-1, 0, 1} sums multiples of 1/8 below 2^18: exact in fp32 in any order."""
    w = lattice_w((Co, Ci, 3, 3), "lcw")
    b = lattice_bias(Co, "lcb")
    wo = torch.zeros(27, Ci, 3, 3)
    bo = torch.zeros(27)
    bo[:18] = _ints("lco", (18,), -2, 2)
    on = _ints("lcm", (9,), 0, 3)
    bo[18:] = torch.where(on > 0, torch.tensor(DCN_MASK_ON), torch.tensor(DCN_MASK_OFF))
    bo[18 + 4] = DCN_MASK_ON
    return w, b, wo, bo


# ---- fused DeformConv with integer offsets ------------------------------------------------------------------------------------------
DCN_OFFSET_SCALES = (1, 2, 4)
DCN_RELU_SHIFT_SIGMAS = 1.3                         # masked-off taps and samples outside the image already hide a tap at some pixels: clip 10 %, not 21 %
DCN_MASK_ON, DCN_MASK_OFF = 32.0, -128.0           # sigmoid(32) rounds to exactly 1 in fp32, sigmoid(-128) is exactly 0


@functools.lru_cache(maxsize=None)
def dcn_operands(B, Ci, Co, H, W):
    """(x, w, b, wo, bo) of a fused DeformConv whose offsets are integers that differ from pixel to pixel.
    Offset rows of conv_offset_mask: ONE non-zero tap each, the centre tap of one input channel, times 1, 2 or 4 -- the offset of a
    pixel is that channel's own value there: an integer in +-3, +-6 or +-12 (inside the apron, in patch slots, in pass 2, outside the
    image).  Mask rows: zero filters, bias +32 or -128 per tap, so sigmoid is exactly 1 or 0.  The bilinear weights are then 0 or 1."""
    x = lattice_x((B, Ci, H, W), "ldx")
    w = lattice_w((Co, Ci, 3, 3), "ldw")
    b = lattice_bias(Co, "ldb")
    wo = torch.zeros(27, Ci, 3, 3)
    bo = torch.zeros(27)
    ch = _ints("ldc", (18,), 0, Ci - 1).long()
    sc = _ints("lds", (18,), 0, len(DCN_OFFSET_SCALES) - 1).long()
    sg = _ints("ldg", (18,), 0, 1)
    for r in range(18):
        scale = 1 if r in (8, 9) else DCN_OFFSET_SCALES[sc[r]]          # (the centre tap moves by at most 3: most of its samples stay in the image)
        wo[r, ch[r], 1, 1] = float(scale) * (1.0 if sg[r] else -1.0)
    on = _ints("ldm", (9,), 0, 3)                   # three taps in four are on
    bo[18:] = torch.where(on > 0, torch.tensor(DCN_MASK_ON), torch.tensor(DCN_MASK_OFF))
    bo[18 + 4] = DCN_MASK_ON                        # (the centre tap always)
    return x, w, b + relu_shift(dcn_pre(x, w, b, wo, bo), DCN_RELU_SHIFT_SIGMAS), wo, bo     # DCN layers end in BatchNorm + ReLU


def dcn_offsets(x, wo, bo):
    """fp64 conv_offset_mask output [B,27,H,W]."""
    return F.conv2d(x.double(), wo.double(), bo.double(), 1, 1)


def dcn_pre(x, w, b, wo, bo, acc_dtype=torch.float64):
    """DeformConv output before ReLU from the oracle (oracle/dcn.py), as tests/gpu_helpers.dcn_fused_reference; acc_dtype=None: the
    contraction in fp32."""
    from oracle import dcn as odcn
    om = dcn_offsets(x, wo, bo).float()
    o1, o2, mask = torch.chunk(om, 3, dim=1)
    return odcn.dcn_v2_forward(x, w, b, torch.cat((o1, o2), dim=1).contiguous(), torch.sigmoid(mask).contiguous(), 3, 3, 1, 1, 1, 1, 1, 1, 1,
                               acc_dtype=acc_dtype).double()


# ---- fused DeformConv on the quarter-pixel lattice --------------------------------------------------------------------------------
# Sampling positions on k/4 and masks in {0, 1/2, 1}: every bilinear weight (times the mask) is a multiple of 1/32, every product with an
# integer activation and every partial sum of the blend is exact in fp16 and in fp32 in any order, and the contraction with w in
# {-1, 0, 1} sums multiples of 1/32 far below 2^24 / 32.  The four-corner blend, the mask folded into the weights, the partial-corner
# samples at the image border (h_im in (-1, 0) and (H - 1, H)) and the gate exactly at -1 and H are then compared with torch.equal.
DCN_FRAC_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
DCN_MASK_HALF = 0.0                                 # sigmoid(0) = 1 / (1 + 1) = 0.5 exactly, if the reciprocal of 2 is exact
DCN_MASK_LEVELS = {"binary": (DCN_MASK_OFF, DCN_MASK_ON), "half": (DCN_MASK_OFF, DCN_MASK_HALF, DCN_MASK_ON)}
DCN_FRAC_UNIT = 1.0 / 64.0                          # every output is a multiple of this
DCN_MIN_FRACTIONAL = 0.25                           # share of the offset coordinates off the integers, per coordinate
DCN_FRAC_DRAW = "8"                                 # suffix of the draw's keys: the first one under which every case meets tests/test_oracle_lattice.py's conditions


@functools.lru_cache(maxsize=None)
def dcn_frac_operands(B, Ci, Co, H, W, mask_levels):
    """(x, w, b, wo, bo) of a fused DeformConv whose offsets are multiples of 1/4 that differ from pixel to pixel: x, w, bias and the
    ReLU shift as in `dcn_operands`; offset rows of conv_offset_mask = the centre tap of one input channel times +-{1/4, 1/2, 1, 2, 4}
    (rows 8 and 9, the centre tap's own offsets: 1/4 only), so a pixel's offset is k/4, k/2, k, 2k or 4k with k that channel's value in
    -3..3 there -- inside the apron, in patch slots, in pass 2 and outside the image.  Mask rows: zero filters, bias per tap from
    `mask_levels`: "binary" {+32, -128} (mask 1 or 0), "half" {+32, -128, 0} (mask 1, 0 or 1/2); the centre tap is always on.  The scales
    and the mask levels are drawn once for all shapes (their keys hold no shape), the channels per Ci."""
    levels = DCN_MASK_LEVELS[mask_levels]
    x = lattice_x((B, Ci, H, W), "ldx")
    w = lattice_w((Co, Ci, 3, 3), "ldw")
    b = lattice_bias(Co, "ldb")
    wo = torch.zeros(27, Ci, 3, 3)
    bo = torch.zeros(27)
    ch = _ints("lfc" + DCN_FRAC_DRAW, (18,), 0, Ci - 1).long()
    sc = _ints("lfs" + DCN_FRAC_DRAW, (18,), 0, len(DCN_FRAC_SCALES) - 1).long()
    sg = _ints("lfg" + DCN_FRAC_DRAW, (18,), 0, 1)
    for r in range(18):
        scale = DCN_FRAC_SCALES[0] if r in (8, 9) else DCN_FRAC_SCALES[sc[r]]
        wo[r, ch[r], 1, 1] = float(scale) * (1.0 if sg[r] else -1.0)
    lv = _ints("lfm" + DCN_FRAC_DRAW, (9,), 0, 3).long()            # per tap: 0 off, 1 the middle level (on, where there is none), 2 and 3 on
    for t in range(9):
        bo[18 + t] = levels[0] if lv[t] == 0 else levels[1] if lv[t] == 1 else levels[-1]
    bo[18 + 4] = DCN_MASK_ON                        # (the centre tap always)
    return x, w, b + relu_shift(dcn_pre(x, w, b, wo, bo), DCN_RELU_SHIFT_SIGMAS), wo, bo


@functools.lru_cache(maxsize=None)
def dcn_frac_exact(B, Ci, Co, H, W, mask_levels):
    """(fp64-accumulated DeformConv + ReLU as fp32, conv_offset_mask output) of `dcn_frac_operands`; computed once per case."""
    x, w, b, wo, bo = dcn_frac_operands(B, Ci, Co, H, W, mask_levels)
    return F.relu(dcn_pre(x, w, b, wo, bo)).float(), dcn_offsets(x, wo, bo)


def dcn_positions(offset, H, W, k=(3, 3), s=1, p=1, d=1):
    """(h_im, w_im), each [B, dg * kh * kw, Ho, Wo] in fp64: the sampling positions of DCNv2 (offset channel 2 t is tap t's row offset,
    2 t + 1 its column offset, group after group)."""
    B, n2, Ho, Wo = offset.shape
    K = k[0] * k[1]
    o = offset.double().reshape(B, n2 // (2 * K), K, 2, Ho, Wo)
    ti = (torch.arange(K) // k[1]).double().view(1, 1, K, 1, 1) * d
    tj = (torch.arange(K) % k[1]).double().view(1, 1, K, 1, 1) * d
    ys = (torch.arange(Ho).double() * s - p).view(1, 1, 1, Ho, 1)
    xs = (torch.arange(Wo).double() * s - p).view(1, 1, 1, 1, Wo)
    return (ys + ti + o[:, :, :, 0]).reshape(B, -1, Ho, Wo), (xs + tj + o[:, :, :, 1]).reshape(B, -1, Ho, Wo)


DCN_CLASSES = ("h_partial_low", "h_partial_high", "h_on_gate_low", "h_on_gate_high", "w_partial_low", "w_partial_high", "w_on_gate_low",
               "w_on_gate_high", "far")


def dcn_sample_classes(h_im, w_im, H, W):
    """Number of samples per border class.  partial: the coordinate in (-1, 0) / (size - 1, size), two of the four corners outside the
    image, the other coordinate inside the gate; on_gate: the coordinate exactly -1 / size (gated off: the reference's `>` and `<`) while
    the other coordinate is fractional and inside the gate, so that only this comparison gates the sample; far: beyond the gate."""
    def frac(t):
        return t != t.floor()
    h_in, w_in = (h_im > -1) & (h_im < H), (w_im > -1) & (w_im < W)
    n = lambda m: int(m.sum())
    return {"h_partial_low": n((h_im > -1) & (h_im < 0) & w_in), "h_partial_high": n((h_im > H - 1) & (h_im < H) & w_in),
            "h_on_gate_low": n((h_im == -1) & w_in & frac(w_im)), "h_on_gate_high": n((h_im == H) & w_in & frac(w_im)),
            "w_partial_low": n((w_im > -1) & (w_im < 0) & h_in), "w_partial_high": n((w_im > W - 1) & (w_im < W) & h_in),
            "w_on_gate_low": n((w_im == -1) & h_in & frac(h_im)), "w_on_gate_high": n((w_im == W) & h_in & frac(h_im)),
            "far": n((h_im < -1) | (h_im > H) | (w_im < -1) | (w_im > W))}


def dcn_fractional_share(offset, k=(3, 3)):
    """(share of the row offsets, share of the column offsets) that are no integers."""
    B, n2, Ho, Wo = offset.shape
    o = offset.double().reshape(B, n2 // 2, 2, Ho, Wo)
    return float((o[:, :, 0] != o[:, :, 0].round()).double().mean()), float((o[:, :, 1] != o[:, :, 1].round()).double().mean())


def dcn_pre_restated(x, w, b, wo, bo, swap_tap=None, keep_tap=None, channels=None):
    """The fused DeformConv (3 x 3, stride 1, pad 1) before ReLU, restated in fp64 with plain loops over taps and corners -- equal to
    `dcn_pre` bit for bit on lattice operands -- with one of two defects on request, on input channels [0, channels) (None: all):
      swap_tap   lh and lw exchanged in the four bilinear weights of that tap;
      keep_tap   that tap's corner (h_low, w_low) is not zeroed when it lies outside the image: the clamped pixel is read instead."""
    om = dcn_offsets(x, wo, bo).float().double()
    B, C, H, W = x.shape
    Co = w.shape[0]
    flat = x.double().reshape(B, C, H * W)
    h_all, w_all = dcn_positions(om[:, :18], H, W)
    cols = torch.zeros(B, C, 9, H * W, dtype=torch.float64)

    def blend(t, swap, keep):
        h_im, w_im = h_all[:, t], w_all[:, t]
        inside = ((h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)).double()
        hl, wl = h_im.floor(), w_im.floor()
        lh, lw = (w_im - wl, h_im - hl) if swap else (h_im - hl, w_im - wl)
        m = torch.sigmoid(om[:, 18 + t].float()).double() * inside
        acc = torch.zeros(B, C, H * W, dtype=torch.float64)
        for dy, dx, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
            yy, xx = hl.long() + dy, wl.long() + dx
            ok = ((yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)).double()
            if keep and (dy, dx) == (0, 0):
                ok = torch.ones_like(ok)
            v = torch.gather(flat, 2, (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(B, 1, -1).expand(B, C, -1))
            acc = acc + (wt * ok * m).view(B, 1, -1) * v
        return acc
    for t in range(9):
        cols[:, :, t] = blend(t, False, False)
        if t in (swap_tap, keep_tap):
            n = C if channels is None else channels
            cols[:, :n, t] = blend(t, t == swap_tap, t == keep_tap)[:, :n]
    return (torch.matmul(w.double().reshape(Co, -1), cols.reshape(B, C * 9, H * W)) + b.double().view(1, Co, 1)).view(B, Co, H, W)



# ---- the DCNv2 operator and its backward on the same lattice -------------------------------------------------------------------------
def dcn_grid_case(seed, B, C, Co, H, W, k=(3, 3), s=1, p=1, d=1, dg=1):
    """(x, w, b, offset, mask, grad_y) for dcn_v2_forward / dcn_v2_backward: x and grad_y integers in [-3, 3], w in {-1, 0, 1}, b integers in
    [-4, 4], offsets on k/4 (an integer in [-5, 5] plus 0, 1/4, 1/2 or 3/4), a tenth of them pushed past the gate by H + W + 8 (as
    dcn_backward_ref.make_offsets does), masks on k/8, k = 0..8.  Every bilinear weight, its derivative and every product with the mask is
    a multiple of 1/128: the output and all five gradients are sums of such multiples far below 2^24 / 128, exact in fp32 in any order --
    grad_input under float atomics included."""
    g = torch.Generator().manual_seed(seed)
    Ho = (H + 2 * p - (d * (k[0] - 1) + 1)) // s + 1
    Wo = (W + 2 * p - (d * (k[1] - 1) + 1)) // s + 1
    K = dg * k[0] * k[1]
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    x = ri(-3, 3, (B, C, H, W))
    w = ri(-1, 1, (Co, C, k[0], k[1]))
    b = ri(-4, 4, (Co,))
    off = ri(-5, 5, (B, 2 * K, Ho, Wo)) + ri(0, 3, (B, 2 * K, Ho, Wo)) / 4.0
    push = torch.rand(off.shape, generator=g) < 0.1
    sign = torch.where(torch.rand(off.shape, generator=g) < 0.5, -1.0, 1.0)
    off = torch.where(push, off + sign * float(H + W + 8), off)
    m = ri(0, 8, (B, K, Ho, Wo)) / 8.0
    gy = ri(-3, 3, (B, Co, Ho, Wo))
    return x, w, b, off, m, gy


# name -> (seed, B, C, Co, H, W, k, s, p, d, dg).  The seeds are the first ones from 1 on under which the case holds a sample of every class
# of `dcn_sample_classes` (tests/test_oracle_dcn_backward.py asserts it).
DCN_GRID_MFMA = {"m_2x48to7_13x11": (1, 2, 48, 7, 13, 11, (3, 3), 1, 1, 1, 1), "m_64to64_24x40": (1, 1, 64, 64, 24, 40, (3, 3), 1, 1, 1, 1),
                 "m_512to256_16x16": (1, 1, 512, 256, 16, 16, (3, 3), 1, 1, 1, 1), "m_16to27_20x37": (1, 1, 16, 27, 20, 37, (3, 3), 1, 1, 1, 1)}
DCN_GRID_GENERAL = {"g_s2": (1, 2, 8, 7, 13, 11, (3, 3), 2, 1, 1, 1), "g_d2_dg2": (1, 2, 8, 7, 13, 11, (3, 3), 1, 2, 2, 2),
                    "g_dg4": (1, 2, 8, 7, 13, 11, (3, 3), 1, 1, 1, 4), "g_1x1": (5, 2, 5, 3, 9, 7, (1, 1), 1, 0, 1, 1),
                    "g_3x1_dg3": (1, 1, 6, 67, 15, 17, (3, 1), 1, 1, 1, 3)}
DCN_GRID_CASES = dict(DCN_GRID_MFMA, **DCN_GRID_GENERAL)


@functools.lru_cache(maxsize=None)
def dcn_grid(name):
    return dcn_grid_case(*DCN_GRID_CASES[name])


@functools.lru_cache(maxsize=None)
def dcn_grid_exact(name):
    """(forward, (grad_input, grad_offset, grad_mask, grad_weight, grad_bias)) of a named case from the fp64 oracle, cast to float32 (no
    rounding happens: tests/test_oracle_dcn_backward.py asserts that the float32 oracle gives the same bits).  Computed once."""
    import dcn_backward_ref as R
    x, w, b, off, m, gy = dcn_grid(name)
    k, s, p, d, dg = DCN_GRID_CASES[name][6:]
    y = R.forward(*[t.double() for t in (x, w, b, off, m)], k, s, p, d, dg)
    return y.float(), tuple(t.float() for t in R.oracle_grads(x, w, b, off, m, gy, k, s, p, d, dg))

