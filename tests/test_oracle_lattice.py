"""CPU: the conditions that make a ZERO tolerance legitimate for every case tests/test_gpu_lattice.py runs (tests/lattice_ref.py).

  * fp32 F.conv2d on the lattice operands equals the fp64 result bit for bit;
  * every fp32 partial sum, in any order, is an integer number of grid units bounded by sum |x| |w| (+ |b| + |res|) < 2^24;
  * at most 2 % of the pre-rounding outputs of the integer-lattice families lie beyond the range a 2-byte type holds exactly
    (|y| <= 256 bf16, <= 2048 fp16) -- those are still determined by the one round-to-nearest-even, but a coarser grid hides more;
  * ReLU clips between 5 % and 40 % of the outputs;
  * the packed operands ARE the lattice: identity-BatchNorm folding returns the integers, the f16x3 split has an all-zero lo half.

The stems and the up-sample + add run on DYADIC operands by design (image on k/256 so that the kernel's own conversion rounds; deconv
weights on k/8): their outputs are rounded in every 2-byte case, so for them the grid conditions (exact fp32 sums in units of 2^-8 ...)
are pinned instead of the integer range cap.

The fused DeformConv also runs on a QUARTER-PIXEL lattice (offsets k/4, masks 0, 1/2, 1: `test_dcn_frac_*`): the same conditions, plus
the share of fractional offsets, a census of the border classes (partial corners, a coordinate exactly on the gate, beyond the gate) and
the 2-byte plans' fp16 blend being exact; `test_exchanged_lh_lw_*` / `test_kept_border_corner_*` measure two blend defects against the
tolerance of tests/test_gpu_variants.py.

`test_one_dropped_tap_*` records why the lattice files exist: one zeroed filter tap changes most of that filter's rounded lattice
outputs, and stays below the existing bf16 tolerance under the suite's uniform operand recipe."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lattice_ref as L
import test_gpu_lattice as G
from h3d_amd import engine, synth

LIMIT = 2.0 ** 24


def _conv_keys():
    keys = [tuple(c) for c in G.CONV_CASES] + [G.VIEW_CASE, G.OUT_NCHW_CASE, G.OUT_NHWC_CASE]
    for c in G.GEMM1_LATTICE:
        keys.append((c[0], c[1], c[2], c[3], c[4], 1, c[10] if len(c) > 10 else 1, c[5], c[6]))
    for c, _ in G.CONV2_LATTICE:
        keys.append((c[1], c[2], c[3], c[4], c[5], 3, c[6], c[7], c[8]))
    return list(dict.fromkeys(keys))


def _check_integer_family(cond, relu, what):
    assert cond["fp32_exact"], what
    assert cond["on_grid"] and cond["max_units"] < LIMIT, (what, cond["max_units"])
    for d, share in cond["outside"].items():
        assert share <= L.MAX_OUTSIDE, (what, d, share)
    if relu:
        assert L.RELU_CLIP[0] <= L.clipped_share(cond["pre"]) <= L.RELU_CLIP[1], (what, L.clipped_share(cond["pre"]))


@pytest.mark.parametrize("key", _conv_keys(), ids=lambda k: "%dx%d-%dx%d-k%d-s%d-b%d%s%s" % (k[1], k[2], k[3], k[4], k[5], k[6], k[0], "-relu" * k[7], "-res" * k[8]))
def test_conv_cases_are_exact_in_fp32(key):
    x, w, b, res = L.conv_operands(*key)
    for t, lo, hi in ((x, -3, 3), (w, -1, 1)) + (((res, -8, 8),) if res is not None else ()):
        assert torch.equal(t, t.round()) and lo <= float(t.min()) and float(t.max()) <= hi
    assert torch.equal(b, b.round())
    _check_integer_family(L.conditions(x, w, b, key[6], key[5] // 2, res), key[7], key)


def test_lattice_draws_are_deterministic_and_cover_their_grids():
    assert torch.equal(L.lattice_x((3, 5, 7, 9)), L.lattice_x((3, 5, 7, 9)))
    assert sorted(set(L.lattice_x((4000,)).tolist())) == [-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]
    assert sorted(set(L.lattice_w((64, 16, 3, 3)).flatten().tolist())) == [-1.0, 0.0, 1.0]
    assert sorted(set(L.lattice_w((64, 16, 3, 3), exp=-3).flatten().tolist())) == [-0.125, 0.0, 0.125]
    assert sorted(set(L.lattice_res((4000,)).tolist())) == [float(v) for v in range(-8, 9)]
    assert sorted(set(L.lattice_up_w((4000,)).tolist())) == [v / 8.0 for v in range(9)]
    img = L.lattice_image((1, 3, 64, 64))
    assert torch.equal(img * 256, (img * 256).round()) and -2.0 <= float(img.min()) and float(img.max()) < 2.0
    # the image exercises the kernels' own conversion: bf16 has to round it (ties to even included), fp16 and the f16x3 split hold it
    r = L.lowp_round(img, "bf16")
    assert bool((r != img).any()) and bool(((r - img).abs() * 256 == 1.0).any())      # |v| in [1, 2): k odd is a tie between two bf16 values
    assert torch.equal(L.lowp_round(img, "f16"), img)
    long_k = L.lattice_w((8, 512, 3, 3))
    assert float((long_k != 0).float().mean()) < 0.4                                  # 4608 terms: sparser filters


# ---- stems -------------------------------------------------------------------------------------------------------------------------------
def _stem_cases():
    B, Co, H, W = G.STEM_S1_SHAPE
    return [((B, Co, H, W, 1), d) for d in G.ALL] + [((s[0], s[1], s[2], s[3], 2), d) for s in G.STEM_S2_SHAPES for d in ("bf16", "f16")]


@pytest.mark.parametrize("key,dtype", _stem_cases())
def test_stem_cases_are_exact_in_fp32(key, dtype):
    x, w, b = L.stem_operands(*key)
    cond = L.conditions(L.lowp_round(x, dtype), w, b, key[4], 3, None, unit=2.0 ** -8)
    assert cond["fp32_exact"] and cond["on_grid"] and cond["max_units"] < LIMIT, (key, dtype, cond["max_units"])
    assert L.RELU_CLIP[0] <= L.clipped_share(cond["pre"]) <= L.RELU_CLIP[1], L.clipped_share(cond["pre"])


@pytest.mark.parametrize("shape,dtype", G.stem3_lattice_cases())
def test_fused_stem_cases_are_exact_in_fp32(shape, dtype):
    x, sd, layers = L.stem3_operands(*shape)
    chain, out = L.stem3_chain(x, layers, dtype)
    unit = 2.0 ** -8
    for (t, w, b, k, s), (_, _, _, _, _, e) in zip(chain, L.STEM3_LAYERS):
        unit *= 2.0 ** e
        cond = L.conditions(t, w, b, s, k // 2, None, unit=unit)
        assert cond["fp32_exact"] and cond["on_grid"] and cond["max_units"] < LIMIT, (shape, dtype, k, cond["max_units"])
        assert L.RELU_CLIP[0] <= L.clipped_share(cond["pre"]) <= L.RELU_CLIP[1], (shape, dtype, k, L.clipped_share(cond["pre"]))
    if dtype in L.EXACT_RANGE:          # "mostly inside the exact range": the third layer's outputs keep at least 1/16 resolution in bf16
        assert float((cond["pre"].abs() > 128.0).double().mean()) <= L.MAX_OUTSIDE
    # the packed banks are the lattice: identity BatchNorm folds to the same numbers
    pw = engine.PackedWeights.from_tensors(sd, dtype, "cpu")
    for (name, *_), (w, b, k, s) in zip(L.STEM3_LAYERS, layers):
        wf, bf = pw._fold(sd[name + ".0.weight"], None, name + ".1")
        assert torch.equal(wf, w) and torch.equal(bf, b), name


# ---- heads -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.HEADS_SHAPES)
def test_heads_cases_are_exact_in_fp32(shape):
    x, sd = L.heads_operands(*shape)
    for h in L.HEADS:
        _check_integer_family(L.conditions(x, sd[h + ".0.weight"], sd[h + ".0.bias"], 1, 1), True, (shape, h))
        for dtype in G.ALL:
            t = L.heads_intermediate(x, sd, h, dtype)
            cond = L.conditions(t, sd[h + ".2.weight"], sd[h + ".2.bias"])          # fp32 output maps: never rounded
            assert cond["fp32_exact"] and cond["on_grid"] and cond["max_units"] < LIMIT, (shape, h, dtype, cond["max_units"])


# ---- up-sample + add ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,size", G.UPADD_SHAPES)
def test_upadd_cases_are_exact_in_every_storage_type(f, size):
    x, skip, w = L.upadd_operands(G.UPADD_B, G.UPADD_C, size[0], size[1], f)
    y64 = F.conv_transpose2d(x.double(), w.double(), None, stride=f, padding=f // 2, groups=G.UPADD_C) + skip.double()
    y32 = F.conv_transpose2d(x, w, None, stride=f, padding=f // 2, groups=G.UPADD_C) + skip
    assert torch.equal(y32.double(), y64)
    assert torch.equal(y64 * 8, (y64 * 8).round()) and float(y64.abs().max()) * 8 <= 256.0       # eighths below 32: 8 significand bits
    for dtype in G.ALL:
        assert torch.equal(L.exact_upadd(x, skip, w, f, dtype).double(), y64), dtype


# ---- fused DeformConv ----------------------------------------------------------------------------------------------------------------------
def _dcn_keys():
    return list(dict.fromkeys(tuple(c[3:8]) for c in G.dcn_lattice_cases()))


@pytest.mark.parametrize("key", _dcn_keys(), ids=lambda k: "%dx%d-%dx%d-b%d" % (k[1], k[2], k[3], k[4], k[0]))
def test_dcn_cases_have_integer_offsets_binary_masks_and_exact_sums(key):
    B, Ci, Co, H, W = key
    x, w, b, wo, bo = L.dcn_operands(*key)
    om = L.dcn_offsets(x, wo, bo)
    off, mask = om[:, :18], torch.sigmoid(om[:, 18:].float())
    assert torch.equal(off, off.round()) and float(off.abs().max()) == 12.0
    assert float(off.std(dim=(0, 2, 3)).min()) > 0.0                                     # every offset row varies from pixel to pixel
    assert set(off.abs().amax(dim=(0, 2, 3)).tolist()) == {3.0, 6.0, 12.0}               # inside the apron, patch slots, pass 2 / outside
    assert bool(((mask == 0.0) | (mask == 1.0)).all()) and float(mask[:, 4].min()) == 1.0 and float(mask.min()) == 0.0
    pre = L.dcn_pre(x, w, b, wo, bo)
    assert torch.equal(L.dcn_pre(x, w, b, wo, bo, acc_dtype=None), pre)                  # the fp32 contraction is the fp64 one
    assert torch.equal(pre, pre.round()) and 3.0 * 9 * Ci + float(b.abs().max()) < LIMIT      # |sample * mask| <= 3, |w| <= 1
    for d, r in L.EXACT_RANGE.items():
        assert float((pre.abs() > r).double().mean()) <= L.MAX_OUTSIDE, (key, d)
    assert L.RELU_CLIP[0] <= L.clipped_share(pre) <= L.RELU_CLIP[1], L.clipped_share(pre)
    # packed operands: the identity BatchNorm of tests/gpu_helpers._dcn_sd folds to the same integers
    from gpu_helpers import _dcn_sd
    pw = engine.PackedWeights.from_tensors(_dcn_sd(w, b, wo, bo), "bf16", "cpu")
    wf, bf = pw._folded("p.conv.weight", "p.conv.bias", "p.actf.0")
    assert torch.equal(wf, w) and torch.equal(bf, b)


# ---- fused DeformConv on the quarter-pixel lattice -------------------------------------------------------------------------------------------
MASK_LEVELS = ("binary", "half")


@pytest.mark.parametrize("mask_levels", MASK_LEVELS)
@pytest.mark.parametrize("key", _dcn_keys(), ids=lambda k: "%dx%d-%dx%d-b%d" % (k[1], k[2], k[3], k[4], k[0]))
def test_dcn_frac_cases_meet_the_conditions_of_a_zero_tolerance(key, mask_levels):
    B, Ci, Co, H, W = key
    x, w, b, wo, bo = L.dcn_frac_operands(B, Ci, Co, H, W, mask_levels)
    x0, w0, _, _, _ = L.dcn_operands(*key)
    assert torch.equal(x, x0) and torch.equal(w, w0) and torch.equal(b, b.round())
    om = L.dcn_offsets(x, wo, bo)
    off, mask = om[:, :18], torch.sigmoid(om[:, 18:].float())
    # offsets: multiples of 1/4 that differ per pixel; every scale is there (inside the apron ... outside the image); the centre tap moves by < 1
    assert torch.equal(off * 4, (off * 4).round()) and float(off.std(dim=(0, 2, 3)).min()) > 0.0
    assert set(off.abs().amax(dim=(0, 2, 3)).tolist()) == {3.0 * s for s in L.DCN_FRAC_SCALES}
    assert float(off[:, 8:10].abs().max()) == 0.75
    fh, fw = L.dcn_fractional_share(off)
    assert fh >= L.DCN_MIN_FRACTIONAL and fw >= L.DCN_MIN_FRACTIONAL, (fh, fw)
    # masks: exactly the levels asked for, all of them present, the centre tap on
    want = {0.0, 1.0} if mask_levels == "binary" else {0.0, 0.5, 1.0}
    assert set(mask.unique().tolist()) == want and float(mask[:, 4].min()) == 1.0
    # every border class has a sample
    h_im, w_im = L.dcn_positions(off, H, W)
    classes = L.dcn_sample_classes(h_im, w_im, H, W)
    assert list(classes) == list(L.DCN_CLASSES) and min(classes.values()) >= 1, classes
    # the fp32 contraction is the fp64 one; outputs on the 1/64 grid, below 2^24 units in any order; the 2-byte plans' fp16 blend is exact
    pre = L.dcn_pre(x, w, b, wo, bo)
    assert torch.equal(L.dcn_pre(x, w, b, wo, bo, acc_dtype=None), pre)
    units = pre / L.DCN_FRAC_UNIT
    assert torch.equal(units, units.round()) and (3.0 * 9 * Ci + float(b.abs().max())) / L.DCN_FRAC_UNIT < LIMIT
    from oracle import dcn as odcn
    blend16 = odcn.dcn_v2_forward(x, w, b, off.float().contiguous(), mask.contiguous(), 3, 3, 1, 1, 1, 1, 1, 1, 1, acc_dtype=torch.float64, blend="f16")
    assert torch.equal(blend16.double(), pre)
    for d, r in L.EXACT_RANGE.items():          # beyond r the 2-byte grid is coarser than 1: still one rounding, but it hides more
        assert float((pre.abs() > r).double().mean()) <= L.MAX_OUTSIDE, (key, d)
    assert L.RELU_CLIP[0] <= L.clipped_share(pre) <= L.RELU_CLIP[1], L.clipped_share(pre)
    ref, om2 = L.dcn_frac_exact(B, Ci, Co, H, W, mask_levels)
    assert torch.equal(ref.double(), F.relu(pre)) and torch.equal(om2, om)
    # the rounding into the storage type is a real one: some outputs are no bf16 numbers
    assert bool((L.lowp_round(ref, "bf16") != ref).any())


def test_dcn_frac_draws_are_deterministic_and_shared_between_the_mask_levels():
    a, b_ = L.dcn_frac_operands(1, 64, 64, 13, 21, "binary"), L.dcn_frac_operands(1, 64, 64, 13, 21, "half")
    L.dcn_frac_operands.cache_clear()
    again = L.dcn_frac_operands(1, 64, 64, 13, 21, "binary")
    assert all(torch.equal(s, t) for s, t in zip(a, again))
    assert torch.equal(a[3], b_[3]) and torch.equal(a[4][:18], b_[4][:18])          # the same offsets under both mask levels
    half = b_[4][18:] == L.DCN_MASK_HALF
    assert 2 <= int(half.sum()) and torch.equal(a[4][18:][half], torch.full((int(half.sum()),), L.DCN_MASK_ON))
    assert torch.equal(a[4][18:][~half], b_[4][18:][~half]) and int((a[4][18:] == L.DCN_MASK_OFF).sum()) >= 1
    assert _x3_lo_is_zero(a[3].permute(0, 2, 3, 1).reshape(27, 9, 64))               # offset filters +-1/4 ... 4: no lo half in the f16x3 split


# ---- packed operands -----------------------------------------------------------------------------------------------------------------------
def _x3_lo_is_zero(w):
    K = w.shape[-1]
    raw = engine.x3_split(w * 2.0 ** engine.x3_exp(w)).contiguous().view(torch.float16).reshape(-1, K // 8, 2, 8)
    back = raw[:, :, 0].float().reshape(w.shape) * 2.0 ** -engine.x3_exp(w)
    return bool((raw[:, :, 1] == 0).all()) and torch.equal(back, w)


def test_f16x3_split_of_lattice_operands_has_no_lo_half():
    assert _x3_lo_is_zero(L.lattice_w((128, 9, 64)))
    assert _x3_lo_is_zero(L.lattice_w((128, 9, 64), exp=-3))
    assert _x3_lo_is_zero(L.dcn_operands(1, 64, 64, 16, 16)[3].permute(0, 2, 3, 1).reshape(27, 9, 64))      # offset filters +-1, 2, 4
    assert _x3_lo_is_zero(L.lattice_x((4, 64)))                        # activations: integers
    assert _x3_lo_is_zero(L.lattice_res((4, 64)))
    assert _x3_lo_is_zero(L.lattice_image((3, 64, 64)))                # k/256 below 2: 10 significand bits
    assert not _x3_lo_is_zero(torch.full((1, 8), 0.1))                 # (an ordinary filter does have one)


# ---- why: one dropped tap -------------------------------------------------------------------------------------------------------------------
def _rnd(key, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform(key, shape, lo, hi, 0))


def _drop(w, co, ci):
    m = w.clone()
    m[co, ci, w.shape[2] // 2, w.shape[3] // 2] = 0.0
    return m


def _first_live_channel(w, co=0):
    return int((w[co, :, w.shape[2] // 2, w.shape[3] // 2] != 0).nonzero()[0])


# (family, (B, Cin, Cout, H, W, k, stride, relu, residual) of its longest contraction, the existing bf16 tolerance relative to max |ref|)
LONGEST = [("conv 3x3", (1, 256, 512, 8, 8, 3, 2, True, False), 1.2e-2), ("conv 1x1", (1, 1280, 512, 4, 4, 1, 1, True, False), 1.2e-2),
           ("gemm1", (1, 1280, 512, 8, 8, 1, 1, True, False), 1.2e-2), ("conv2", (1, 256, 256, 12, 20, 3, 1, False, False), 2.0 ** -8)]


@pytest.mark.parametrize("family,key,tol", LONGEST, ids=[f for f, _, _ in LONGEST])
def test_one_dropped_tap_changes_the_lattice_result_and_hides_under_the_uniform_tolerance(family, key, tol):
    assert key in _conv_keys()
    B, Ci, Co, H, W, k, s, relu, use_res = key
    x, w, b, res = L.conv_operands(*key)
    ci = _first_live_channel(w)
    good, bad = L.exact_conv(x, w, b, s, k // 2, relu, res, "bf16"), L.exact_conv(x, _drop(w, 0, ci), b, s, k // 2, relu, res, "bf16")
    assert torch.equal(good[:, 1:], bad[:, 1:])
    assert float((good[:, 0] != bad[:, 0]).float().mean()) >= 0.5
    # the suite's recipe (tests/test_gpu_conv._case_tensors): x ~ U(-1, 1), w ~ U(-1, 1) * 1.5 / sqrt(Cin k k), rounded to bf16
    xu, wu, bu = L.lowp_round(_rnd("x", (B, Ci, H, W)), "bf16"), L.lowp_round(_rnd("w", (Co, Ci, k, k)) * (1.5 / np.sqrt(Ci * k * k)), "bf16"), _rnd("b", (Co,))
    ref = L.exact_conv(xu, wu, bu, s, k // 2, relu, None, "f32")
    err = float((L.exact_conv(xu, _drop(wu, 0, 0), bu, s, k // 2, relu, None, "f32") - ref).abs().max())
    assert 0.0 < err <= tol * max(1.0, float(ref.abs().max())), (err, tol * max(1.0, float(ref.abs().max())))


def test_one_dropped_tap_in_the_heads():
    shape = G.HEADS_SHAPES[-1]
    x, sd = L.heads_operands(*shape)
    ci = _first_live_channel(sd["pose.0.weight"])
    bad_sd = dict(sd)
    bad_sd["pose.0.weight"] = _drop(sd["pose.0.weight"], 0, ci)
    good, bad = L.heads_intermediate(x, sd, "pose", "bf16"), L.heads_intermediate(x, bad_sd, "pose", "bf16")
    assert float((good[:, 0] != bad[:, 0]).float().mean()) >= 0.5
    live = sd["pose.2.weight"][:, 0, 0, 0] != 0                                        # the output maps that read intermediate channel 0
    changed = L.exact_head(x, sd, "pose", "bf16")[:, live] != L.exact_head(x, bad_sd, "pose", "bf16")[:, live]
    assert int(live.sum()) > 0 and float(changed.float().mean()) >= 0.5
    # tests/test_gpu_conv.test_fused_heads_op_matches_torch's recipe and its bf16 tolerance, 3e-2 * max |ref|
    xu = L.lowp_round(_rnd("feat", (shape[0], 64, shape[1], shape[2]), -1.5, 1.5), "bf16")
    w1, b1 = L.lowp_round(_rnd("posew1", (256, 64, 3, 3)) * (1.6 / np.sqrt(64 * 9)), "bf16"), _rnd("poseb1", (256,), -0.2, 0.2)
    w2, b2 = L.lowp_round(_rnd("posew2", (72, 256, 1, 1)) * (1.6 / np.sqrt(256)), "bf16"), _rnd("poseb2", (72,), -0.5, 0.5)
    ref = L.pre_conv(L.exact_conv(xu, w1, b1, 1, 1, True, None, "bf16"), w2, b2)
    mut = L.pre_conv(L.exact_conv(xu, _drop(w1, 0, 0), b1, 1, 1, True, None, "bf16"), w2, b2)
    assert 0.0 < float((mut - ref).abs().max()) <= 3e-2 * max(1.0, float(ref.abs().max()))


def test_one_dropped_tap_in_the_deformconv():
    key = max(_dcn_keys(), key=lambda k: k[1])                                          # the longest contraction: 512 x 9
    B, Ci, Co, H, W = key
    x, w, b, wo, bo = L.dcn_operands(*key)
    ci = _first_live_channel(w)
    good = L.lowp_round(F.relu(L.dcn_pre(x, w, b, wo, bo)), "bf16")
    bad = L.lowp_round(F.relu(L.dcn_pre(x, _drop(w, 0, ci), b, wo, bo)), "bf16")
    assert torch.equal(good[:, 1:], bad[:, 1:])
    assert float((good[:, 0] != bad[:, 0]).float().mean()) >= 0.5
    # tests/test_gpu_variants._dcn_built's recipe and its bf16 tolerance, 1.2e-2 * max |ref|
    a = float(np.sqrt(3.0 / (Ci * 9)))
    xu = L.lowp_round(_rnd("x", (B, Ci, H, W)), "bf16")
    wu, bu = (_rnd("w", (Co, Ci, 3, 3)) * (1.5 / np.sqrt(Ci * 9))).half().float(), _rnd("b", (Co,))
    wou, bou = (_rnd("wo", (27, Ci, 3, 3)) * (a * 3.0 * np.sqrt(3.0))).half().float(), _rnd("bo", (27,), -0.1, 0.1)
    ref = F.relu(L.dcn_pre(xu, wu, bu, wou, bou))
    err = float((F.relu(L.dcn_pre(xu, _drop(wu, 0, 0), bu, wou, bou)) - ref).abs().max())
    assert 0.0 < err <= 1.2e-2 * max(1.0, float(ref.abs().max())), err


# ---- why: two defects of the bilinear blend --------------------------------------------------------------------------------------------------
FRAC_SMALLEST, FRAC_LONGEST = (1, 128, 128, 7, 5), (1, 512, 256, 16, 16)
DEFECT_TAP = 0                      # the first tap: its samples reach the top and the left border
VARIANTS_BF16_TOL = 1.2e-2          # tests/test_gpu_variants.test_dcn_fused_variant_matches_oracle, relative to max |ref|


def _defect_figures(defect):
    """(outputs changed on the smallest case by the one-channel defect, by the all-channel one, max error / max |ref| on the longest case for
    the one-channel defect, for the all-channel one), all after ReLU; the counts after the rounding to bf16."""
    assert FRAC_SMALLEST in _dcn_keys() and FRAC_LONGEST in _dcn_keys()
    out = []
    x, w, b, wo, bo = L.dcn_frac_operands(*FRAC_SMALLEST, "half")
    assert torch.equal(L.dcn_pre_restated(x, w, b, wo, bo), L.dcn_pre(x, w, b, wo, bo))          # the restatement itself is exact
    good = L.lowp_round(F.relu(L.dcn_pre(x, w, b, wo, bo)), "bf16")
    for channels in (1, None):
        bad = L.lowp_round(F.relu(L.dcn_pre_restated(x, w, b, wo, bo, channels=channels, **{defect: DEFECT_TAP})), "bf16")
        out.append(int((bad != good).sum()))
    x, w, b, wo, bo = L.dcn_frac_operands(*FRAC_LONGEST, "half")
    ref = F.relu(L.dcn_pre(x, w, b, wo, bo))
    for channels in (1, None):
        bad = F.relu(L.dcn_pre_restated(x, w, b, wo, bo, channels=channels, **{defect: DEFECT_TAP}))
        out.append(float((bad - ref).abs().max()) / float(ref.abs().max()))
    print("%s on tap %d: changes %d (one channel) / %d (all channels) of %d outputs at %s; max error / max |ref| at %s: %.3g / %.3g"
          % (defect, DEFECT_TAP, out[0], out[1], good.numel(), FRAC_SMALLEST, FRAC_LONGEST, out[2], out[3]))
    return out


def test_exchanged_lh_lw_on_one_tap_changes_the_exact_result_and_one_channel_of_it_hides_under_the_tolerance():
    """lh and lw exchanged in one tap's bilinear weights.  In ONE input channel (one lane's element of a fragment) it changes at least 32
    outputs of the smallest case and stays under 1.2e-2 max |ref| on the longest contraction: the tolerance test cannot see it.  In all
    channels of the tap it moves outputs by a quarter of max |ref|: that one the tolerance test does see."""
    one, every, rel_one, rel_every = _defect_figures("swap_tap")
    assert one >= 32 and every >= 256, (one, every)
    assert 0.0 < rel_one <= VARIANTS_BF16_TOL, rel_one
    assert rel_every > VARIANTS_BF16_TOL, rel_every


def test_kept_border_corner_on_one_tap_changes_the_exact_result_and_one_channel_of_it_hides_under_the_tolerance():
    """A corner outside the image that is read (clamped) instead of zeroed: touches only the partial-corner samples at the top and left
    border.  One channel: at least 32 outputs of the smallest case, under 1.2e-2 max |ref| on the longest contraction."""
    one, every, rel_one, rel_every = _defect_figures("keep_tap")
    assert one >= 32 and every >= 64, (one, every)
    assert 0.0 < rel_one <= VARIANTS_BF16_TOL, rel_one
    assert rel_every > VARIANTS_BF16_TOL, rel_every
