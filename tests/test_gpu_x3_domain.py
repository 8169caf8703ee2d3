"""The f16x3 plan kernels (csrc/common.h ET<x3_t>: fp32 storage, three fp16 MFMAs on split operands) element by element across
activation magnitudes, and their clamp / non-finite rule.

One criterion, derived in tests/x3_ref.py and checked on the CPU by tests/test_oracle_x3_domain.py:

    |y - y64| <= TAU (A + |b|) + 2^-25 S + 2^-38 max|w| X          per output element, propagated through chained kernels

on conv_kernel<x3_t> (3x3, 3x3 stride 2, 1x1, with and without residual + ReLU), heads_kernel<x3_t>, stem3x_kernel and the fused
DeformConv dcn3_kernel<x3_t> (register-staged and patch-slot variants), with activations `uniform`, `spread` (per-element exponents
over 2^-12 ... 1) and `regions` (decaying by 2^-2 every two columns) at overall scales 2^-20 ... 2^15 and filter gains 1e-6, 1, 3e3.
The DeformConv's conv_offset_mask has zero filters and a bias per row: offsets and masks are constants per tap, exact and independent
of x (the activation-dependent offset convolution away from O(1) is not in this file's scope).

Out of range and non-finite (g = 1), for every kernel: activations of 1e5 and +-3e38 give the fp64 result on the CLAMPED tensor within
the bound; +-inf and NaN leave every output finite, and every output whose receptive field holds none of them within the bound of the
untouched tensor.  The overwritten elements include tile corners and, for the DeformConv, the corners of samples that only the
patch slots / pass 2 read (the reach is asserted on the sample geometry in tests/test_oracle_x3_domain.py).

`pytest -s` prints the worst err / bound per kernel and scale (DESIGN.md quotes the table)."""
import ctypes

import numpy as np
import pytest
import torch

import x3_ref as R
from gpu_helpers import DEV, conv, dcn_fused_op, fake_pw, mk, nhwc, run
from h3d_amd import _lib

pytestmark = pytest.mark.gpu

WORST = {}
X3 = "f16x3"


def _check(kernel, key, tag, got, y64, bound, tile=(16, 16), where=None):
    ratio, msg = R.report(tag, got, y64, bound, tile, where)
    WORST[(kernel, key)] = max(WORST.get((kernel, key), 0.0), ratio)
    print("%s: worst err / bound = %.3g" % (tag, ratio))
    assert ratio <= 1.0, msg


def _targs(name):
    """the template arguments of a kernel instantiation's name"""
    return name[name.index("<") + 1:name.rindex(">")].split(", ")


# ---- conv_kernel<x3_t> -------------------------------------------------------------------------------------------------------------------
def _conv(c, x, w, b, res):
    return conv(x, w, b, X3, stride=c[6], relu=c[7], res=res)[0]


def _conv_tile(c, x, w, b, res):
    name = conv(x, w, b, X3, stride=c[6], relu=c[7], res=res, name_only=True)
    assert name.startswith("conv_kernel<x3_t"), name
    return int(_targs(name)[5]), 16


@pytest.mark.parametrize("gen", R.GENERATORS)
@pytest.mark.parametrize("ci", range(len(R.CONV_CASES)), ids=[R.conv_id(c) for c in R.CONV_CASES])
def test_conv_meets_the_bound_at_every_activation_scale(ci, gen):
    c = R.CONV_CASES[ci]
    tile = None
    for g in R.SCALES:
        for gain in R.GAINS:
            x, w, b, res, y64, bound = R.conv_reference(ci, gen, g, gain)
            tile = tile or _conv_tile(c, x, w, b, res)
            _check("conv", g, "%s %s g=2^%d gain=%g" % (R.conv_id(c), gen, np.log2(g), gain), _conv(c, x, w, b, res), y64, bound, tile)


@pytest.mark.parametrize("ci", range(len(R.CONV_CASES)), ids=[R.conv_id(c) for c in R.CONV_CASES])
def test_conv_clamps_out_of_range_and_keeps_non_finite_activations_out(ci):
    c = R.CONV_CASES[ci]
    k, s, rr = c[5], c[6], c[7]
    x, w, b, res, y64, bound = R.conv_reference(ci, "uniform", 1.0, 1.0)
    tile = _conv_tile(c, x, w, b, res)
    xb, _ = R.poison(x, R.BIG)
    yb, bb = R.bound_conv(xb, w, b, s, k // 2, res, rr)                  # (the reference clamps)
    _check("conv", "1e5, +-3e38", "%s out of range" % R.conv_id(c), _conv(c, xb, w, b, res), yb, bb, tile)
    xn, ind = R.poison(x, R.NONFINITE)
    got = _conv(c, xn, w, b, res)
    assert bool(torch.isfinite(got).all()), "%s: a non-finite activation reached the output" % R.conv_id(c)
    clean = ~R.conv_reach(ind, k, s)
    assert 0.5 < float(clean.double().mean()) < 1.0
    _check("conv", "+-inf, NaN", "%s non-finite" % R.conv_id(c), got, y64, bound, tile, where=clean)


# ---- heads_kernel<x3_t> ------------------------------------------------------------------------------------------------------------------
def _heads(x, sd):
    """The four multi_pose heads in one H3D_OP_HEADS launch per width class (the op construction of test_fused_heads_op_matches_torch)"""
    B, _, H, W = x.shape
    pw = fake_pw(sd, X3)
    pw.heads, pw.head_conv = dict(R.HEADS), 256
    xb, xp = nhwc(x, X3)
    outs, keep = {}, [xb]
    for names in R.HEAD_GROUPS:
        w1, b1, per = pw.fused_heads(names)
        desc = _lib.H3dHeadsDesc()
        desc.nheads = len(per)
        desc.wexp = pw.wexp.get(w1.data_ptr(), 0)
        for i, (hname, c, w2, b2) in enumerate(per):
            outs[hname] = torch.full((B, c, H, W), float("nan"), dtype=torch.float32, device=DEV)
            desc.head[i].w2, desc.head[i].b2, desc.head[i].out, desc.head[i].C = w2.data_ptr(), b2.data_ptr(), outs[hname].data_ptr(), c
            desc.head[i].wexp2 = pw.wexp.get(w2.data_ptr(), 0)
        keep.append(desc)
        run(mk(_lib.OP_HEADS, X3, in_=xp, in2=ctypes.addressof(desc), w=w1.data_ptr(), bias=b1.data_ptr(), B=B, H=H, W=W, Cin=64, in_cs=64,
               Ho=H, Wo=W, Cout=256, ksize=3, stride=1))
    return {h: t.cpu() for h, t in outs.items()}


@pytest.mark.parametrize("gen", R.GENERATORS)
@pytest.mark.parametrize("shape", R.HEADS_SHAPES, ids=lambda s: "%dx%d" % s[1:])
def test_heads_meet_the_propagated_bound_at_every_activation_scale(shape, gen):
    for g in R.SCALES:
        for gain in R.GAINS:
            x, sd = R.heads_operands(shape, gen, g, gain)
            ref, got = R.bound_heads(x, sd), _heads(x, sd)
            for h in R.HEADS:
                _check("heads", g, "heads/%s %dx%d %s g=2^%d gain=%g" % ((h,) + shape[1:] + (gen, np.log2(g), gain)), got[h], ref[h][0], ref[h][1], (8, 32))


@pytest.mark.parametrize("shape", R.HEADS_SHAPES, ids=lambda s: "%dx%d" % s[1:])
def test_heads_clamp_out_of_range_and_keep_non_finite_activations_out(shape):
    x, sd = R.heads_operands(shape, "uniform", 1.0, 1.0)
    ref = R.bound_heads(x, sd)
    xb, _ = R.poison(x, R.BIG)
    refb, gotb = R.bound_heads(xb, sd), _heads(xb, sd)
    xn, ind = R.poison(x, R.NONFINITE)
    gotn = _heads(xn, sd)
    clean = ~R.conv_reach(ind, 3, 1)
    assert 0.5 < float(clean.double().mean()) < 1.0
    for h in R.HEADS:
        _check("heads", "1e5, +-3e38", "heads/%s %dx%d out of range" % ((h,) + shape[1:]), gotb[h], refb[h][0], refb[h][1], (8, 32))
        assert bool(torch.isfinite(gotn[h]).all()), "heads/%s: a non-finite activation reached the output" % h
        _check("heads", "+-inf, NaN", "heads/%s %dx%d non-finite" % ((h,) + shape[1:]), gotn[h], ref[h][0], ref[h][1], (8, 32), where=clean)


# ---- stem3x_kernel -------------------------------------------------------------------------------------------------------------------------
def _stem(x, sd):
    """H3D_OP_STEM3 of an f16x3 plan (the op construction of test_fused_stem_op_matches_torch)"""
    B, _, H, W = x.shape
    pw = fake_pw(sd, X3)
    wdev, bdev = pw.stem3_x3()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img = x.to(DEV).contiguous()
    out = torch.full((B, Ho, Wo, 32), float("nan"), dtype=torch.float32, device=DEV)
    run(mk(_lib.OP_STEM3, X3, in_=img.data_ptr(), w=wdev.data_ptr(), bias=bdev.data_ptr(), out=out.data_ptr(), B=B, H=H, W=W, Cin=3,
           in_cs=3, Ho=Ho, Wo=Wo, Cout=32, out_cs=32, ksize=7, stride=1, relu=1))
    return out.permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("shape", R.STEM_SHAPES, ids=lambda s: "%dx%d" % s[1:])
def test_stem_meets_the_propagated_bound_with_small_and_large_intermediates(shape):
    for s in R.STEM_SCALES:
        for gain in R.GAINS:
            x, sd = R.stem_operands(shape, s, gain)
            y64, bound = R.bound_stem3(x, sd)
            _check("stem3x", s, "stem3x %dx%d scale=2^%d gain=%g" % (shape[1:] + (np.log2(s), gain)), _stem(x, sd), y64, bound, (8, 16))


@pytest.mark.parametrize("shape", R.STEM_SHAPES, ids=lambda s: "%dx%d" % s[1:])
def test_stem_clamps_out_of_range_and_keeps_non_finite_pixels_out(shape):
    # the image at scale 1, and the intermediates pushed beyond 65504 by a first layer 2^10 * 3e3 times as large (the reference chain clamps
    # each intermediate as the LDS staging does).  A level1 output sees 11 x 11 image pixels: 0.25 % of them overwritten leaves outputs to compare
    for s, gain in ((1.0, 1.0), (2.0 ** 10, 3e3)):
        x, sd = R.stem_operands(shape, s, gain)
        y64, bound = R.bound_stem3(x, sd)
        if gain > 1.0:
            t = x.double()
            w, b, k, st = R.stem_folded(sd)[0]
            assert float(torch.nn.functional.conv2d(t, w.double(), b.double(), st, k // 2).max()) > 10 * R.FMAX       # the clamp of the intermediates IS reached
        xb, _ = R.poison(x, R.BIG, share=0.0025)
        yb, bb = R.bound_stem3(xb, sd)
        _check("stem3x", "1e5, +-3e38", "stem3x %dx%d scale=2^%d out of range" % (shape[1:] + (np.log2(s),)), _stem(xb, sd), yb, bb, (8, 16))
        xn, ind = R.poison(x, R.NONFINITE, share=0.0025)
        got = _stem(xn, sd)
        assert bool(torch.isfinite(got).all()), "stem3x: a non-finite pixel reached the output"
        clean = ~R.stem_reach(ind)
        assert 0.1 < float(clean.double().mean()) < 1.0
        _check("stem3x", "+-inf, NaN", "stem3x %dx%d scale=2^%d non-finite" % (shape[1:] + (np.log2(s),)), got, y64, bound, (8, 16), where=clean)


# ---- dcn3_kernel<x3_t> ---------------------------------------------------------------------------------------------------------------------
_MARGIN_FLAG = {("fused", 2): _lib.TUNE_DCN_FUSED_X3_MARGIN2, ("fused", 6): _lib.TUNE_DCN_FUSED_X3_MARGIN6}


def _dcn(c, x, w, b, off18, ml):
    """Fused DeformConv through H3D_OP_DCN_FUSED / _STREAM with zero conv_offset_mask filters and (offsets | mask logits) as its bias"""
    kind, Ci, ov, margin, slots = c[0], c[2], c[6], c[8], c[9]
    wo = torch.zeros(27, Ci, 3, 3)
    bo = torch.cat([off18, ml]).float()
    built = dcn_fused_op(kind, x, w, b, wo, bo, X3, _MARGIN_FLAG.get((kind, ov), 0))
    name = built.name
    args = _targs(name)                           # <T, MT, CK, MARGIN, EPI, WDMA, NP>: the apron and the slots the CPU geometry assumed
    assert name.startswith("dcn3_kernel<x3_t") and int(args[3]) == margin and (int(args[6]) if len(args) > 6 else 0) == slots, name
    return built.run()


@pytest.mark.parametrize("gen", R.GENERATORS)
@pytest.mark.parametrize("ci", range(len(R.DCN_CASES)), ids=[R.dcn_id(c) for c in R.DCN_CASES])
def test_dcn_meets_the_bound_at_every_activation_scale(ci, gen):
    c = R.DCN_CASES[ci]
    for g in R.SCALES:
        for gain in R.GAINS:
            x, (w, b), (wf, bf), off18, ml = R.dcn_operands(c, gen, g, gain)
            y64, bound = R.bound_dcn(x, wf, bf, off18, ml)
            _check("dcn3 " + c[0], g, "%s %s g=2^%d gain=%g" % (R.dcn_id(c), gen, np.log2(g), gain), _dcn(c, x, w, b, off18, ml), y64, bound)


@pytest.mark.parametrize("ci", range(len(R.DCN_CASES)), ids=[R.dcn_id(c) for c in R.DCN_CASES])
def test_dcn_clamps_out_of_range_and_keeps_non_finite_activations_out(ci):
    c = R.DCN_CASES[ci]
    x, (w, b), (wf, bf), off18, ml = R.dcn_operands(c, "uniform", 1.0, 1.0)
    y64, bound = R.bound_dcn(x, wf, bf, off18, ml)
    extra = R.dcn_far_elements(c)                 # corners of one sample per far path: read through the patch slots / pass 2
    xb, _ = R.poison(x, R.BIG, extra=extra)
    yb, bb = R.bound_dcn(xb, wf, bf, off18, ml)
    _check("dcn3 " + c[0], "1e5, +-3e38", "%s out of range" % R.dcn_id(c), _dcn(c, xb, w, b, off18, ml), yb, bb)
    xn, ind = R.poison(x, R.NONFINITE, extra=extra)
    got = _dcn(c, xn, w, b, off18, ml)
    assert bool(torch.isfinite(got).all()), "%s: a non-finite activation reached the output" % R.dcn_id(c)
    clean = ~R.dcn_reach(ind, off18, ml)          # no corner with a nonzero weight on an overwritten element (csrc/dcn3.hip: the 0 * v rule)
    assert 0.1 < float(clean.double().mean()) < 1.0
    _check("dcn3 " + c[0], "+-inf, NaN", "%s non-finite" % R.dcn_id(c), got, y64, bound, where=clean)


def test_zz_print_the_worst_ratios():
    # (runs last in this file: the table DESIGN.md quotes)
    for kernel in sorted({k for k, _ in WORST}):
        row = [(g, r) for (k, g), r in WORST.items() if k == kernel]
        nums = sorted((g, r) for g, r in row if not isinstance(g, str))
        print("worst err / bound, %-11s: %s  |  %s" % (kernel, "  ".join("2^%d: %.3f" % (int(np.log2(g)), r) for g, r in nums),
                                                      "  ".join("%s: %.3f" % (g, r) for g, r in row if isinstance(g, str))))
