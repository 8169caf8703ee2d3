"""CPU: the derived f16x3 bound of tests/x3_ref.py on every case tests/test_gpu_x3_domain.py runs, without a GPU.

  * a torch emulation of the split arithmetic alone (clamp, hi / lo, three fp64 products on the PACKER's filter terms, one fp32 rounding)
    stays within the bound, everywhere;
  * plain fp32 arithmetic stays within TAU / 4 of (A + |b|): the first term of the bound leaves a real kernel's accumulation order room;
  * the floor terms are needed: at g <= 2^-12 the emulated error exceeds TAU (A + |b|) at more than half of the outputs -- the test is
    not vacuous, and f16x3 is NOT fp32-grade there;
  * what the element-wise bound sees and the suite's max-norm rule (test_gpu_conv._check: 3e-5 max|ref|) does not: a mutant that leaves
    the x.lo w.hi product out of ONE MFMA step (one tap, 16 input channels) breaks the bound at g = 1 and passes the max-norm rule.
    (Leaving that product out of EVERY step breaks both: 3.4 ... 5.1 times the max-norm tolerance on these cases -- the numbers are
    asserted below.)
  * the DeformConv cases reach the paths they are named after: the sample geometry of csrc/dcn3.hip restated on the CPU
    (x3_ref.dcn_sample_paths) puts samples in the apron, in patch slots and in pass 2, and the overwritten activations of the
    out-of-range tests are read through each of them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import x3_ref as R

SMALL = 2.0 ** -12
WORST = {}


def _note(kernel, g, ratio):
    WORST[(kernel, g)] = max(WORST.get((kernel, g), 0.0), ratio)


def _open(y64, relu):
    """the outputs a floor error can show in: all of them, or those the ReLU lets through"""
    return (y64 > 0) if relu else torch.ones_like(y64, dtype=torch.bool)


def _share_over(err, tau_bound, sel):
    return float((err > tau_bound)[sel].double().mean())


@pytest.mark.parametrize("ci", range(len(R.CONV_CASES)), ids=[R.conv_id(c) for c in R.CONV_CASES])
def test_conv_emulation_keeps_the_bound_and_fp32_keeps_a_quarter_of_tau(ci):
    c = R.CONV_CASES[ci]
    k, s, rr = c[5], c[6], c[7]
    worst_cal = worst_fused = 0.0
    for gen in R.GENERATORS:
        for g in R.SCALES:
            for gain in R.GAINS:
                x, w, b, res, y64, bound = R.conv_reference(ci, gen, g, gain)
                emu = R.x3_conv_emulated(x, w, b, s, k // 2, res, rr)
                ratio, msg = R.report("emulation %s %s g=%g gain=%g" % (R.conv_id(c), gen, g, gain), emu, y64, bound)
                _note("conv", g, ratio)
                assert ratio <= 1.0, msg
                _, tau_bound = R.bound_conv(x, w, b, s, k // 2, res, rr, floor=False)
                # fp32: the contraction from a zero accumulator, then bias (+ residual) -- and F.conv2d with the bias fused in, whose
                # oneDNN kernel STARTS the accumulator at b: every tiny product is then rounded at ulp(b), which costs outputs that
                # are all bias up to half of TAU (recorded, held to TAU itself)
                y32 = F.conv2d(x, w, None, s, k // 2) + b.view(1, -1, 1, 1)
                yf = F.conv2d(x, w, b, s, k // 2)
                if rr:
                    y32, yf = F.relu(y32 + res), F.relu(yf + res)
                worst_cal = max(worst_cal, float(((y32.double() - y64).abs() / tau_bound).max()))
                worst_fused = max(worst_fused, float(((yf.double() - y64).abs() / tau_bound).max()))
                if g <= SMALL:
                    share = _share_over((emu.double() - y64).abs(), tau_bound, _open(y64, rr))
                    assert share > 0.5, (gen, g, gain, share)
    print("%s: fp32 worst err / (TAU (A + |b|)) = %.3f (bias after the sum), %.3f (F.conv2d's fused bias)" % (R.conv_id(c), worst_cal, worst_fused))
    assert worst_cal <= 0.25 and worst_fused <= 1.0, (worst_cal, worst_fused)


@pytest.mark.parametrize("shape", R.HEADS_SHAPES, ids=lambda s: "%dx%d" % s[1:])
def test_heads_emulation_keeps_the_propagated_bound(shape):
    worst_cal = 0.0
    for gen in R.GENERATORS:
        for g in R.SCALES:
            for gain in R.GAINS:
                x, sd = R.heads_operands(shape, gen, g, gain)
                ref, tau_ref, emu = R.bound_heads(x, sd), R.bound_heads(x, sd, floor=False), R.heads_emulated(x, sd)
                for h in R.HEADS:
                    y64, bound = ref[h]
                    ratio, msg = R.report("emulation heads/%s %s g=%g gain=%g" % (h, gen, g, gain), emu[h], y64, bound)
                    _note("heads", g, ratio)
                    assert ratio <= 1.0, msg
                    t = F.relu(F.conv2d(x.clamp(-R.FMAX, R.FMAX), sd[h + ".0.weight"], None, 1, 1) + sd[h + ".0.bias"].view(1, -1, 1, 1))
                    y32 = F.conv2d(t.clamp(-R.FMAX, R.FMAX), sd[h + ".2.weight"], None) + sd[h + ".2.bias"].view(1, -1, 1, 1)
                    worst_cal = max(worst_cal, float(((y32.double() - y64).abs() / tau_ref[h][1]).max()))
                    # the TAU terms of a CHAIN are a sum of absolute values over the 256 intermediate channels, which the random signs of
                    # the emulated error stay under until every activation is below the floor: the share is asserted at the smallest g
                    if g <= 2.0 ** -20:
                        assert _share_over((emu[h].double() - y64).abs(), tau_ref[h][1], _open(y64, False)) > 0.5, (h, gen, g, gain)
    print("heads %s: fp32 worst err / TAU terms = %.3f" % (shape, worst_cal))
    assert worst_cal <= 0.25


@pytest.mark.parametrize("shape", R.STEM_SHAPES, ids=lambda s: "%dx%d" % s[1:])
def test_stem_emulation_keeps_the_propagated_bound(shape):
    # (the image is O(1) by contract, so the first contraction is never in the floor regime: no share to assert)
    worst_cal = 0.0
    for s in R.STEM_SCALES:
        for gain in R.GAINS:
            x, sd = R.stem_operands(shape, s, gain)
            y64, bound = R.bound_stem3(x, sd)
            ratio, msg = R.report("emulation stem3x scale=%g gain=%g" % (s, gain), R.stem3_emulated(x, sd), y64, bound, tile=(8, 16))
            _note("stem3x", s, ratio)
            assert ratio <= 1.0, msg
            t = x
            for w, b, k, st in R.stem_folded(sd):
                t = F.relu(F.conv2d(t.clamp(-R.FMAX, R.FMAX), w, None, st, k // 2) + b.view(1, -1, 1, 1))
            worst_cal = max(worst_cal, float(((t.double() - y64).abs() / R.bound_stem3(x, sd, floor=False)[1]).max()))
    print("stem3x %s: fp32 worst err / TAU terms = %.3f" % (shape, worst_cal))
    assert worst_cal <= 0.25


@pytest.mark.parametrize("ci", range(len(R.DCN_CASES)), ids=[R.dcn_id(c) for c in R.DCN_CASES])
def test_dcn_emulation_keeps_the_bound(ci):
    c = R.DCN_CASES[ci]
    worst_cal = 0.0
    for gen in R.GENERATORS:
        for g in R.SCALES:
            for gain in R.GAINS:
                x, _, (w, b), off18, ml = R.dcn_operands(c, gen, g, gain)
                y64, bound = R.bound_dcn(x, w, b, off18, ml)
                emu = R.dcn_emulated(x, w, b, off18, ml)
                ratio, msg = R.report("emulation %s %s g=%g gain=%g" % (R.dcn_id(c), gen, g, gain), emu, y64, bound)
                _note("dcn", g, ratio)
                assert ratio <= 1.0, msg
                _, tau_bound = R.bound_dcn(x, w, b, off18, ml, floor=False)
                if gain == 1.0:       # fp32: the oracle in the reference's arithmetic (fp32 sampling, fp32 GEMM)
                    off, m = R._const_maps(off18, ml, *[x.shape[i] for i in (0, 2, 3)])
                    y32 = F.relu(R.odcn.dcn_v2_forward(x.clamp(-R.FMAX, R.FMAX), w, b, off.float(), m.float(), *R.FAST))
                    worst_cal = max(worst_cal, float(((y32.double() - y64).abs() / tau_bound).max()))
                if g <= SMALL:
                    share = _share_over((emu.double() - y64).abs(), tau_bound, _open(y64, True))
                    assert share > 0.5, (gen, g, gain, share)
    print("%s: fp32 oracle worst err / TAU terms = %.3f" % (R.dcn_id(c), worst_cal))
    assert worst_cal <= 0.25


def _max_norm_rule(got, ref):
    """test_gpu_conv._check for f16x3: max error over 3e-5 max(1, max |ref|)"""
    return float((got.double() - ref).abs().max()) / (3e-5 * max(1.0, float(ref.abs().max())))


@pytest.mark.parametrize("gen", R.GENERATORS)
@pytest.mark.parametrize("ci", [0, 2, 4], ids=[R.conv_id(R.CONV_CASES[i]) for i in (0, 2, 4)])
def test_one_dropped_lo_product_breaks_the_bound_and_hides_under_the_max_norm_rule(ci, gen):
    c = R.CONV_CASES[ci]
    x, w, b, res, y64, bound = R.conv_reference(ci, gen, 1.0, 1.0)
    step = R.x3_conv_emulated(x, w, b, c[6], c[5] // 2, drop=("xlo_whi", 1, 1, 16))      # ONE MFMA step: the centre tap, channels 16 .. 31
    every = R.x3_conv_emulated(x, w, b, c[6], c[5] // 2, drop="xlo_whi")
    good = R.x3_conv_emulated(x, w, b, c[6], c[5] // 2)
    r_step, r_every, r_good = [R.report("", t, y64, bound)[0] for t in (step, every, good)]
    m_step, m_every, m_good = [_max_norm_rule(t, y64) for t in (step, every, good)]
    print("%s %s: err / bound -- intact %.3f, one step %.2f, every step %.1f; err / (3e-5 max|ref|) -- intact %.4f, one step %.3f, every step %.2f"
          % (R.conv_id(c), gen, r_good, r_step, r_every, m_good, m_step, m_every))
    assert r_good <= 0.2 and m_good <= 0.01
    assert r_step > 2.5 and m_step < 1.0               # measured 2.7 ... 9.0 times the bound, 0.52 ... 0.90 of the max-norm tolerance
    assert r_every > 15.0 and m_every > 3.0            # measured 16 ... 39 times the bound, 3.4 ... 5.1 times the max-norm tolerance


def test_deformconv_cases_reach_apron_patch_slots_and_pass_two():
    for c in R.DCN_CASES:
        kind, B, Ci, Co, H, W, ov, oname, margin, slots, expect = c
        expect = set(expect)
        paths = R.dcn_sample_paths(H, W, margin, slots, R.off18_of(oname))
        have = set(np.unique(paths).tolist()) - {R.GATED}
        assert have == expect, (R.dcn_id(c), have)
        assert (paths == R.GATED).any(), R.dcn_id(c)           # some samples fall outside the image
        per_tile = [int((paths[ty:ty + 16, tx:tx + 16] >= R.PATCH).sum()) for ty in range(0, H, 16) for tx in range(0, W, 16)]
        if oname == "far":      # tiles with more far samples than slots, and one the slots suffice for
            assert max(per_tile) > slots >= min(per_tile) > 0, per_tile
        if oname == "few":      # every tile within its slots, some in the second fill round (entries >= 128)
            assert slots >= max(per_tile) > 128 and min(per_tile) > 0, per_tile
        # the overwritten activations (x3_ref.poison, with the low corners of one sample per far path: x3_ref.dcn_far_elements) are read
        # through every path.  (Every element is also read by the +-0.75 taps of its neighbours, and at 1 % of the elements nearly every
        # output sees an overwritten value somewhere: no element and no output is far-only.  An unclamped far path still shows: 1e5
        # instead of 65504 through one corner is ~1e3 times the bound of an output whose A holds a few clamped values.)
        x = torch.zeros(B, Ci, H, W)
        extra = R.dcn_far_elements(c)
        assert len(extra) == len(expect - {R.APRON})
        _, ind = R.poison(x, R.BIG, extra=extra)
        off18, ml = R.off18_of(oname), torch.tensor(R.MASK_LOGITS)
        by = {p: R.dcn_reach(ind, off18, ml, paths, [p]) for p in expect}
        for p in expect:
            assert by[p].any(), (R.dcn_id(c), p)
        for e, p in zip(extra, sorted(expect - {R.APRON})):
            only = torch.zeros_like(ind)
            only[tuple(e)] = True
            assert R.dcn_reach(only, off18, ml, paths, [p]).any(), (R.dcn_id(c), e, p)


def test_zz_print_the_emulations_worst_ratios():
    # (runs last in this file: the table DESIGN.md quotes)
    for kernel in ("conv", "heads", "stem3x", "dcn"):
        row = sorted((g, r) for (k, g), r in WORST.items() if k == kernel)
        print("emulation worst err / bound, %-6s: %s" % (kernel, "  ".join("2^%d: %.3f" % (int(np.log2(g)), r) for g, r in row)))
