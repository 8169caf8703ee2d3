"""Bit-exact GPU parity of the forward matrix-core ops on integer-lattice operands (tests/lattice_ref.py): csrc/conv.hip, gemm1.hip,
conv2.hip, extra.hip (stems), stem3.hip, stem3x.hip, heads.hip, the up-sample + add helper and the fused DeformConv of dcn3.hip.

Every comparison is torch.equal(kernel, reference rounded once to the storage type): products and fp32 partial sums of the lattice
operands are exact in bf16, fp16, fp32 and f16x3 in any summation order (tests/test_oracle_lattice.py pins that, case by case), so a
dropped, duplicated or misplaced tap, a wrong halo pixel or a stale ring slot cannot hide under the 2^-8 * max|ref| tolerances of
test_gpu_conv.py / test_gpu_variants.py.  The case tables and the variant-forcing `reserved` values are theirs."""
import ctypes

import pytest
import torch

import lattice_ref as L
from gpu_helpers import (DEV, TD, TN, conv, conv_stream_op, dcn_fused_op, dcn_fused_reference, fake_pw, from_nhwc, kernel_name, mk,
                         nhwc, run)
from h3d_amd import _lib
from test_gpu_conv import CONV_CASES, GEMM1_CASES
from test_gpu_variants import CONV2_CASES, CONV2_F16_CASES, DCN_CASES, _is_extra

pytestmark = pytest.mark.gpu

ALL = ("f32", "bf16", "f16", "f16x3")
MAX_PIXELS = 20000          # cases above this many output pixels are selected only by their grid: a forced variant reaches the same kernel


def assert_exact(got, ref, name):
    """torch.equal, and on failure: kernel, number of mismatches, the first one and where it sits in the tiles the kernels use."""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    if torch.equal(got, ref):
        return
    bad = ~(got == ref)             # (a NaN counts)
    b, c, y, x = bad.nonzero()[0].tolist()
    W = got.shape[3]
    raise AssertionError("%s: %d of %d outputs differ from the exact reference; first at (b, c, y, x) = (%d, %d, %d, %d): got %r, expected %r; "
                         "c mod 32 / 128 = %d / %d, y mod 8 / 16 / 32 = %d / %d / %d, x mod 16 / 32 = %d / %d, pixel index mod 128 / 256 = %d / %d"
                         % (name, int(bad.sum()), bad.numel(), b, c, y, x, float(got[b, c, y, x]), float(ref[b, c, y, x]), c % 32, c % 128,
                            y % 8, y % 16, y % 32, x % 16, x % 32, (y * W + x) % 128, (y * W + x) % 256))


# ---- A. H3D_OP_CONV (csrc/conv.hip) ---------------------------------------------------------------------------------------------
def _conv_args(case):
    B, Ci, Co, H, W, k, s, relu, use_res = case
    x, w, b, res = L.conv_operands(*case)
    return x, w, b, res, dict(stride=s, relu=relu, res=res)


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_lattice(case, dtype):
    x, w, b, res, kw = _conv_args(case)
    got, _ = conv(x, w, b, dtype, **kw)
    assert_exact(got, L.exact_conv(x, w, b, case[6], case[5] // 2, case[7], res, dtype), conv(x, w, b, dtype, name_only=True, **kw))


@pytest.mark.parametrize("dtype", ["bf16", "f16x3"])
def test_a_dropped_tap_on_the_device_is_seen(dtype):
    """The check itself, on the longest 3x3 contraction: with one filter tap zeroed in the KERNEL's operands only, the result equals the
    mutated reference bit for bit and differs from the intact one in at least half of that filter's pixels (and nowhere else)."""
    case = (1, 256, 512, 8, 8, 3, 2, True, False)
    assert case in CONV_CASES
    x, w, b, res, kw = _conv_args(case)
    bad = w.clone()
    bad[0, int((w[0, :, 1, 1] != 0).nonzero()[0]), 1, 1] = 0.0
    got, _ = conv(x, bad, b, dtype, **kw)
    assert_exact(got, L.exact_conv(x, bad, b, 2, 1, True, None, dtype), "conv with a dropped tap, " + dtype)
    ref = L.exact_conv(x, w, b, 2, 1, True, None, dtype)
    assert torch.equal(got[:, 1:], ref[:, 1:]) and float((got[:, 0] != ref[:, 0]).float().mean()) >= 0.5
    with pytest.raises(AssertionError, match=r"outputs differ from the exact reference; first at \(b, c, y, x\) = \(0, 0, "):
        assert_exact(got, ref, "conv with a dropped tap")


VIEW_CASE = (2, 64, 64, 16, 32, 3, 1, True, False)             # test_conv_channel_strided_views
OUT_NCHW_CASE = (2, 256, 34, 16, 24, 1, 1, False, False)        # test_conv_output_modes
OUT_NHWC_CASE = (1, 64, 27, 16, 16, 3, 1, False, False)


@pytest.mark.parametrize("dtype", ALL)
def test_conv_lattice_channel_strided_views(dtype):
    x, w, b, res, kw = _conv_args(VIEW_CASE)
    got, untouched = conv(x, w, b, dtype, in_pad=64, out_pad=128, **kw)
    assert_exact(got, L.exact_conv(x, w, b, 1, 1, True, None, dtype), "conv in/out inside wider buffers, " + dtype)
    assert untouched


@pytest.mark.parametrize("dtype", ALL)
def test_conv_lattice_fp32_output_modes(dtype):
    # fp32 outputs: the exact integer, no rounding at all, in every plan
    x, w, b, _, _ = _conv_args(OUT_NCHW_CASE)
    got, _ = conv(x, w, b, dtype, out_mode=_lib.OUT_NCHW_F32)
    assert_exact(got, L.exact_conv(x, w, b), "conv NCHW fp32 output, " + dtype)
    x, w, b, _, _ = _conv_args(OUT_NHWC_CASE)
    got, _ = conv(x, w, b, dtype, out_mode=_lib.OUT_NHWC_F32, pad_cout_to=32)
    assert_exact(got[:, :27], L.exact_conv(x, w, b, 1, 1), "conv NHWC fp32 output, " + dtype)
    assert float(got[:, 27:].abs().max()) == 0.0


# ---- B. csrc/gemm1.hip -------------------------------------------------------------------------------------------------------------
GEMM1_LATTICE = [c for c in GEMM1_CASES if c[7]]                # the forced-tile rows


def _gemm1_args(case):
    B, Ci, Co, H, W, relu, use_res, reserved, in_pad, out_pad = case[:10]
    st = case[10] if len(case) > 10 else 1
    x, w, b, res = L.conv_operands(B, Ci, Co, H, W, 1, st, relu, use_res)
    return x, w, b, res, st, dict(relu=relu, res=res, in_pad=in_pad, out_pad=out_pad, stride=st)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", GEMM1_LATTICE)
def test_gemm1_lattice_and_halo_kernel_bit_identical(case, dtype):
    x, w, b, res, st, kw = _gemm1_args(case)
    name = conv(x, w, b, dtype, reserved=case[7], name_only=True, **kw)
    assert name.startswith("gemm1_kernel<%s, " % TN[dtype]), name
    got, untouched = conv(x, w, b, dtype, reserved=case[7], **kw)
    ref = L.exact_conv(x, w, b, st, 0, case[5], res, dtype)
    assert_exact(got, ref, name)
    assert untouched is None or untouched
    halo = conv(x, w, b, dtype, reserved=_lib.TUNE_CONV_HALO_TILE, name_only=True, **kw)
    assert halo.startswith("conv_kernel<%s, " % TN[dtype]), halo
    old, _ = conv(x, w, b, dtype, reserved=_lib.TUNE_CONV_HALO_TILE, **kw)
    assert_exact(old, ref, halo)
    assert torch.equal(got, old), (name, halo)


# ---- C. H3D_OP_CONV_STREAM (csrc/conv2.hip) --------------------------------------------------------------------------------------
def _out_pixels(c):
    return c[1] * ((c[4] - 1) // c[6] + 1) * ((c[5] - 1) // c[6] + 1)


CONV2_LATTICE = [(c, "bf16") for c in CONV2_CASES if _out_pixels(c) <= MAX_PIXELS] + \
                [(c, "f16") for c in CONV2_F16_CASES if _out_pixels(c) <= MAX_PIXELS]


def _conv2_built(case, dtype):
    ov, B, Ci, Co, H, W, s, relu, use_res, ipad, opad = case
    x, w, b, res = L.conv_operands(B, Ci, Co, H, W, 3, s, relu, use_res)
    return x, w, b, res, conv_stream_op(x, w, b, s, relu, res, ov, ipad, opad, dtype=dtype)


@pytest.mark.parametrize("case,dtype", CONV2_LATTICE, ids=lambda v: v if isinstance(v, str) else "%#x-%dx%d-%dx%d-s%d-b%d" % (v[0], v[2], v[3], v[4], v[5], v[6], v[1]))
def test_conv_stream_lattice(case, dtype):
    x, w, b, res, built = _conv2_built(case, dtype)
    assert built.name.startswith("conv2_kernel<%s, " % TN[dtype]), built.name
    assert_exact(built.run(), L.exact_conv(x, w, b, case[6], 1, case[7], res, dtype), built.name)


# ---- D. stems and heads -------------------------------------------------------------------------------------------------------------
def _stem_op(x, w, b, stride, dtype, out_pad=0):
    from h3d_amd import engine, weights
    B, _, H, W = x.shape
    Co = w.shape[0]
    wexp = 0
    if dtype == "f32":
        wd = w.contiguous().to(DEV)
    elif dtype == "f16x3":
        bank = weights._stem_bank(w)
        wexp = engine.x3_exp(bank)
        wd = engine.x3_split(bank * 2.0 ** wexp).contiguous().to(DEV)
    else:
        wd = weights._stem_bank(w).to(TD[dtype]).contiguous().to(DEV)
    xi, bd = x.contiguous().to(DEV), b.to(DEV)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.full((B, Ho, Wo, Co + out_pad), 7.0, dtype=TD[dtype], device=DEV)
    op = mk(_lib.OP_STEM, dtype, in_=xi.data_ptr(), w=wd.data_ptr(), bias=bd.data_ptr(), out=out.data_ptr(), B=B, H=H, W=W, Cin=3, in_cs=3,
            Ho=Ho, Wo=Wo, Cout=Co, out_cs=Co + out_pad, ksize=7, stride=stride, relu=1, wexp=wexp)
    return op, out, (xi, wd, bd)


STEM_S1_SHAPE = (2, 16, 40, 56)                                                             # test_stem
STEM_S2_SHAPES = [(2, 64, 48, 80, 0), (1, 128, 37, 51, 0), (2, 64, 64, 64, 32), (1, 80, 23, 20, 0)]      # test_stem_stride2_matches_torch
STEM3_SHAPES = [(2, 48, 64), (1, 45, 72), (1, 45, 70), (3, 16, 32), (1, 130, 34), (1, 131, 36)]         # test_fused_stem_op_matches_torch
HEADS_SHAPES = [(1, 7, 5), (2, 13, 21), (1, 33, 65)]


@pytest.mark.parametrize("dtype", ALL)
def test_stem_lattice(dtype):
    B, Co, H, W = STEM_S1_SHAPE
    x, w, b = L.stem_operands(B, Co, H, W, 1)
    op, out, keep = _stem_op(x, w, b, 1, dtype)
    name = kernel_name(op)
    run(op)
    assert_exact(from_nhwc(out, Co), L.exact_stem(x, w, b, 1, dtype), name)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", STEM_S2_SHAPES)
def test_stem_stride2_lattice(shape, dtype):
    B, Co, H, W, out_pad = shape
    x, w, b = L.stem_operands(B, Co, H, W, 2)
    op, out, keep = _stem_op(x, w, b, 2, dtype, out_pad)
    assert kernel_name(op) == "stem_s2_kernel<%s>" % TN[dtype]
    run(op)
    assert_exact(from_nhwc(out, Co), L.exact_stem(x, w, b, 2, dtype), kernel_name(op))
    if out_pad:
        assert bool((out[..., Co:].float() == 7.0).all().item())


def stem3_lattice_cases():
    """(shape, dtype): the 2-byte kernel reads aligned float4 (widths that are a multiple of 4), the f16x3 kernel takes any width."""
    return [(s, d) for s in STEM3_SHAPES for d in ("bf16", "f16", "f16x3") if d == "f16x3" or s[2] % 4 == 0]


@pytest.mark.parametrize("shape,dtype", stem3_lattice_cases())
def test_fused_stem_lattice(shape, dtype):
    B, H, W = shape
    x, sd, layers = L.stem3_operands(B, H, W)
    pw = fake_pw(sd, dtype)
    wdev, bdev = pw.stem3_x3() if dtype == "f16x3" else pw.stem3()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img = x.to(DEV).contiguous()
    out = torch.full((B, Ho, Wo, 32), float("nan"), dtype=TD[dtype], device=DEV)
    op = mk(_lib.OP_STEM3, dtype, in_=img.data_ptr(), w=wdev.data_ptr(), bias=bdev.data_ptr(), out=out.data_ptr(), B=B, H=H, W=W, Cin=3,
            in_cs=3, Ho=Ho, Wo=Wo, Cout=32, out_cs=32, ksize=7, stride=1, relu=1)
    name = kernel_name(op)
    run(op)
    assert_exact(from_nhwc(out, 32), L.exact_stem3(x, layers, dtype), name)


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("shape", HEADS_SHAPES)
def test_fused_heads_lattice(shape, dtype):
    B, H, W = shape
    x, sd = L.heads_operands(B, H, W)
    pw = fake_pw(sd, dtype)
    pw.heads, pw.head_conv = dict(L.HEADS), 256
    xb, xp = nhwc(x, dtype)
    outs, keep, name = {}, [], ""
    for names in (("hm", "wh"), ("hps",), ("pose",)):                      # one launch per number of 32-row output tiles, as engine.Plan._lower_heads
        w1, b1, per = pw.fused_heads(names)
        desc = _lib.H3dHeadsDesc()
        desc.nheads = len(per)
        desc.wexp = pw.wexp.get(w1.data_ptr(), 0)
        for i, (hname, c, w2, b2) in enumerate(per):
            outs[hname] = torch.full((B, c, H, W), float("nan"), dtype=torch.float32, device=DEV)
            desc.head[i].w2, desc.head[i].b2, desc.head[i].out, desc.head[i].C = w2.data_ptr(), b2.data_ptr(), outs[hname].data_ptr(), c
            desc.head[i].wexp2 = pw.wexp.get(w2.data_ptr(), 0)
        keep.append(desc)
        op = mk(_lib.OP_HEADS, dtype, in_=xp, in2=ctypes.addressof(desc), w=w1.data_ptr(), bias=b1.data_ptr(), B=B, H=H, W=W, Cin=64, in_cs=64,
                Ho=H, Wo=W, Cout=256, ksize=3, stride=1)
        name = kernel_name(op)
        run(op)
    for h in L.HEADS:
        assert_exact(outs[h], L.exact_head(x, sd, h, dtype), "%s head %s" % (name, h))


# ---- E. H3D_OP_UPADD ------------------------------------------------------------------------------------------------------------------
UPADD_SHAPES = [(2, (6, 10)), (4, (6, 10)), (2, (5, 7)), (4, (3, 1)), (8, (2, 3))]        # test_maxpool_and_upadd_and_copy
UPADD_B, UPADD_C = 2, 64


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("f,size", UPADD_SHAPES)
def test_upadd_lattice(f, size, dtype):
    uh, uw = size
    C, k = UPADD_C, 2 * f
    x, skip, w = L.upadd_operands(UPADD_B, C, uh, uw, f)
    xb, xp = nhwc(x, dtype)
    sb, sp = nhwc(skip, dtype)
    wd = w.reshape(C, k * k).t().contiguous().to(DEV)
    out = torch.zeros(UPADD_B, uh * f, uw * f, C, dtype=TD[dtype], device=DEV)
    op = mk(_lib.OP_UPADD, dtype, in_=xp, in2=sp, w=wd.data_ptr(), out=out.data_ptr(), B=UPADD_B, H=uh, W=uw, Cin=C, in_cs=C,
            in2_cs=C, Ho=uh * f, Wo=uw * f, Cout=C, out_cs=C, ksize=k, stride=f)
    name = kernel_name(op)
    run(op)
    assert_exact(from_nhwc(out, C), L.exact_upadd(x, skip, w, f, dtype), "%s f=%d %dx%d" % (name, f, uh, uw))


# ---- F. fused DeformConv (csrc/dcn3.hip) with integer offsets that vary per pixel ---------------------------------------------------
def dcn_lattice_cases():
    """One row of DCN_CASES per (kind, dtype, override, Cin, Cout, >= 64 rows): what the launchers choose an instantiation from, apart
    from the grid size -- the smallest map listed for each; the rows selected only by a large grid are left to the forced variants
    (test_lattice_cases_cover_the_plans checks that no instantiation is lost)."""
    best = {}
    for c in DCN_CASES:
        if _is_extra(c) or c[3] * c[6] * c[7] > MAX_PIXELS:
            continue
        key = (c[0], c[1], c[2], c[4], c[5], c[6] >= 64)
        if key not in best or c[3] * c[6] * c[7] < best[key][3] * best[key][6] * best[key][7]:
            best[key] = c
    odd = [c for c in DCN_CASES if not _is_extra(c) and (c[6], c[7]) in ((13, 21), (7, 5))]
    return list(dict.fromkeys(list(best.values()) + odd))


def _dcn_built(case):
    kind, dtype, ov, B, Ci, Co, H, W, _ = case
    x, w, b, wo, bo = L.dcn_operands(B, Ci, Co, H, W)
    return x, w, b, wo, bo, dcn_fused_op(kind, x, w, b, wo, bo, dtype, ov)


@pytest.mark.parametrize("case", dcn_lattice_cases(), ids=lambda c: "%s-%s-%#x-%dx%d-%dx%d-b%d" % (c[0], c[1], c[2], c[4], c[5], c[6], c[7], c[3]))
def test_dcn_fused_lattice(case):
    x, w, b, wo, bo, built = _dcn_built(case)
    ref, om = dcn_fused_reference(x, w, b, wo, bo)
    assert torch.equal(om[:, :18], om[:, :18].round()) and float(om[:, :18].abs().max()) > 3.0       # integer offsets, beyond the apron
    assert_exact(built.run(), L.lowp_round(ref, case[1]), built.name)


def _case_id(c):
    return "%s-%s-%#x-%dx%d-%dx%d-b%d" % (c[0], c[1], c[2], c[4], c[5], c[6], c[7], c[3])


@pytest.mark.parametrize("mask_levels", ["binary", "half"])
@pytest.mark.parametrize("case", dcn_lattice_cases(), ids=_case_id)
def test_dcn_fused_frac_lattice(case, mask_levels):
    """The same kernels on the quarter-pixel lattice (lattice_ref.dcn_frac_operands): offsets k/4 and masks 0, 1/2, 1, so the four-corner
    blend, the mask folded into the weights, the partial corners at the border and the gate exactly at -1 and H are compared bit for bit.
    "half" needs sigmoid(0) = rcp(2) to be exactly 0.5 on the device, as the integer lattice needs rcp(1) = 1."""
    kind, dtype, ov, B, Ci, Co, H, W, _ = case
    x, w, b, wo, bo = L.dcn_frac_operands(B, Ci, Co, H, W, mask_levels)
    built = dcn_fused_op(kind, x, w, b, wo, bo, dtype, ov)
    ref, om = L.dcn_frac_exact(B, Ci, Co, H, W, mask_levels)
    got = built.run()
    assert_exact(got, L.lowp_round(ref, dtype), "%s, %s masks" % (built.name, mask_levels))
    assert torch.equal(built.run(), got), built.name


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
def test_lattice_cases_cover_the_plans():
    """Every conv_kernel< / conv2_kernel< / gemm1_kernel< / dcn3_kernel< instantiation of the batch 64 / 32 / 16 / 8 bf16 plans has a lattice
    case above; so has every instantiation of the (non-extra) DeformConv rows this file leaves out for their size."""
    from test_gpu_variants import _active_dcn_cases, _dcn_built as dcn_built_uniform, _plan_kernel_names
    tested = {conv(*_conv_args(c)[:3], "bf16", name_only=True, **_conv_args(c)[4]) for c in CONV_CASES}
    tested |= {conv(*_gemm1_args(c)[:3], "bf16", reserved=c[7], name_only=True, **_gemm1_args(c)[5]) for c in GEMM1_LATTICE}
    tested |= {_conv2_built(c, d)[4].name for c, d in CONV2_LATTICE}
    dcn = {_dcn_built(c)[5].name for c in dcn_lattice_cases()}
    left_out = {dcn_built_uniform(c)[5].name for c in _active_dcn_cases() if not _is_extra(c)} - dcn
    assert not left_out, "no lattice case dispatches to %s" % sorted(left_out)
    tested |= dcn
    families = ("conv_kernel<", "conv2_kernel<", "gemm1_kernel<", "dcn3_kernel<")
    for batch in (64, 32, 16, 8):
        missing = sorted(n for n in _plan_kernel_names(batch) if n.startswith(families) and n not in tested)
        assert not missing, "batch %d: no lattice case dispatches to %s" % (batch, missing)
        torch.cuda.empty_cache()
