"""Bit-identity of the decode / helper kernels (nms_topk_kernel, upadd_kernel, maxpool_kernel) against a plain torch
statement of the same op, computed on the device in fp32 and rounded once.  No tolerance anywhere: these kernels are
elementwise or an exact integer select, so a faster version of them has to give the same bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import h3d_amd  # noqa: F401
from h3d_amd import _lib, decode, utils
from gpu_helpers import DEV, TD, from_nhwc, mk, nhwc, run

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


# ------------------------------------------------------------------------------------------------
# nms_topk: heat * (max_pool2d(heat, 3, 1, 1) == heat), then the K largest per map, equal scores lowest flat index first
def _nms_topk_statement(v, K):
    B, C, H, W = v.shape
    keep = F.max_pool2d(v, 3, 1, 1) == v
    val = torch.where(keep, v, v * 0.0) + 0.0                        # (+0.0 folds -0 into +0)
    s, i = torch.sort(val.reshape(B, C, H * W), dim=2, descending=True, stable=True)       # stable: lowest index first
    s, i = s[..., :K].contiguous(), i[..., :K].contiguous()
    return s, i, torch.div(i, W, rounding_mode="floor").float(), (i % W).float()


def _maps(kind, B, C, H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.randn(B, C, H, W, generator=g) * 2 - 1
    if kind == "ties":              # a handful of levels: plateaus of equal maxima, many equal scores around the K-th
        x = torch.round(x * 2) / 2
    elif kind == "sparse":          # few maxima above a flat floor: fewer than K positive survivors, zeros are selected too
        x = torch.where(x > 5.0, x, torch.zeros(()))
        x[:, :, 0, 0] = -1.0
    elif kind == "equal":
        x = torch.full((B, C, H, W), 0.25)
    return x.to(DEV)


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("shape", [(128, 128), (96, 160), (37, 53)])
@pytest.mark.parametrize("kind", ["random", "ties", "sparse", "equal"])
def test_nms_topk_bit_identical(kind, shape, sigmoid):
    H, W = shape
    x = _maps(kind, 2, 3, H, W)
    v = utils._sigmoid(x) if sigmoid else x              # the library's own _sigmoid: the same expf, so the same bits
    for K in (1, 100, 128):
        got = decode._map_topk(x, K, decode.NMS_SIGMOID if sigmoid else 0)
        torch.cuda.synchronize()
        exp = _nms_topk_statement(v, K)
        for name, g, e in zip(("score", "ind", "y", "x"), got, exp):
            a, b = (_bits(g), _bits(e)) if g.dtype == torch.float32 else (g.cpu().numpy(), e.cpu().numpy())
            np.testing.assert_array_equal(a, b, err_msg="%s %s K=%d sigmoid=%d: %s" % (kind, shape, K, sigmoid, name))
    if kind == "equal":             # every pixel is a maximum: pixels 0 .. K-1
        assert got[1].cpu().numpy().tolist() == [[list(range(128))] * 3] * 2


def test_nms_topk2_paired_launch_bit_identical():
    a, b = _maps("random", 2, 1, 128, 128), _maps("ties", 2, 17, 128, 128)
    outs = decode._map_topk2(a, b, 100, decode.NMS_SIGMOID)
    torch.cuda.synchronize()
    for t, got in zip((a, b), outs):
        exp = _nms_topk_statement(utils._sigmoid(t), 100)
        for g, e in zip(got, exp):
            np.testing.assert_array_equal(_bits(g) if g.dtype == torch.float32 else g.cpu().numpy(),
                                          _bits(e) if e.dtype == torch.float32 else e.cpu().numpy())


# ------------------------------------------------------------------------------------------------
# upadd: depthwise ConvTranspose2d(k = 2f, stride f, padding f/2) + skip.  Each output has two contributing rows and two columns;
# the kernel adds them as fp32 fused multiply-adds, taps (row, column) ascending, then adds the skip value and rounds once.
def _upadd_statement(x, skip, w, f, out_dtype):
    """x [B,C,H,W], skip [B,C,fH,fW] fp32 (holding the storage type's values), w [C,k,k] fp32, all on the device."""
    B, C, H, W = x.shape
    k, p = 2 * f, f // 2
    Ho, Wo = H * f, W * f
    oy = torch.arange(Ho, device=x.device)
    ox = torch.arange(Wo, device=x.device)
    acc = torch.zeros(B, C, Ho, Wo, device=x.device)
    for a in range(2):
        ki = (oy + p) % f + a * f
        ny = oy + p - ki
        iy = torch.div(ny, f, rounding_mode="floor")
        yok = (ny >= 0) & (iy < H)
        for c2 in range(2):
            kj = (ox + p) % f + c2 * f
            nx = ox + p - kj
            ix = torch.div(nx, f, rounding_mode="floor")
            xok = (nx >= 0) & (ix < W)
            xs = x[:, :, iy.clamp(0, H - 1)][:, :, :, ix.clamp(0, W - 1)]
            ws = w[:, ki][:, :, kj].unsqueeze(0)
            # fmaf: the product of two fp32 values is exact in fp64; the sum is rounded to fp32 once
            fma = (ws.double() * xs.double() + acc.double()).float()
            acc = torch.where((yok[:, None] & xok[None, :])[None, None], fma, acc)
    return (acc + skip).to(out_dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", [(2, 64, 6, 10), (2, 64, 5, 7), (2, 128, 9, 13), (2, 256, 3, 5), (4, 64, 6, 10), (4, 64, 3, 1), (8, 64, 2, 3)])
def test_upadd_bit_identical(case, dtype):
    f, C, H, W = case
    k = 2 * f
    g = torch.Generator().manual_seed(f * 100 + C + H)
    td = TD[dtype]
    x = torch.randn(2, C, H, W, generator=g).to(td).float()
    skip = torch.randn(2, C, H * f, W * f, generator=g).to(td).float()
    w = torch.rand(C, k, k, generator=g)
    xb, xp = nhwc(x, dtype)
    sb, sp = nhwc(skip, dtype)
    wd = w.reshape(C, k * k).t().contiguous().to(DEV)
    modes = [(_lib.OUT_NHWC, td)] + ([(_lib.OUT_NHWC_F16, torch.float16)] if dtype == "bf16" else [])
    for out_mode, od in modes:
        for reserved in (0, _lib.TUNE_UPADD_TAPS_GLOBAL, _lib.TUNE_UPADD_TAPS_LDS):                       # the launcher's choice, tap table never / always in LDS
            out = torch.zeros(2, H * f, W * f, C, dtype=td, device=DEV)
            run(mk(_lib.OP_UPADD, dtype, in_=xp, in2=sp, w=wd.data_ptr(), out=out.data_ptr(), B=2, H=H, W=W, Cin=C, in_cs=C,
                   in2_cs=C, Ho=H * f, Wo=W * f, Cout=C, out_cs=C, ksize=k, stride=f, out_mode=out_mode, reserved=reserved))
            got = out.view(od) if od != td else out
            exp = _upadd_statement(x.to(DEV), skip.to(DEV), w.to(DEV), f, od).permute(0, 2, 3, 1).contiguous()
            assert torch.equal(got, exp), "upadd %s f=%d C=%d %dx%d reserved=%d out=%s" % (dtype, f, C, H, W, reserved, od)


# ------------------------------------------------------------------------------------------------
# maxpool: 2x2 / 2, floor; fmax of the four values in the order (0,0), (0,1), (1,0), (1,1): a NaN loses against a number
def _maxpool_statement(x):
    Ho, Wo = x.shape[2] // 2, x.shape[3] // 2
    x = x[:, :, :2 * Ho, :2 * Wo]
    m = torch.fmax(x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2])
    m = torch.fmax(m, x[:, :, 1::2, 0::2])
    return torch.fmax(m, x[:, :, 1::2, 1::2])


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", [(2, 32, 18, 22, 48, 8), (1, 16, 19, 23, 16, 0), (3, 64, 64, 64, 64, 0), (2, 128, 7, 33, 136, 8), (1, 24, 5, 4, 24, 0)])
def test_maxpool_bit_identical(case, dtype):
    B, C, H, W, cs, coff = case
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g).to(TD[dtype]).float()
    pick = torch.randint(0, 12, x.shape, generator=g)
    for code, val in ((0, -0.0), (1, 0.0), (2, float("inf")), (3, float("-inf")), (4, float("nan"))):
        x = torch.where(pick == code, torch.full((), val), x)
    x[:, :, 0:2, 0:2] = float("nan")                   # one window of four NaNs, one of four -0, one of four -inf
    x[:, :, 2:4, 0:2] = -0.0
    x[:, :, 0:2, 2:4] = float("-inf")
    xb, xp = nhwc(x, dtype, cs, coff)
    Ho, Wo = H // 2, W // 2
    out = torch.full((B, Ho, Wo, cs), 7.0, dtype=TD[dtype], device=DEV)
    run(mk(_lib.OP_MAXPOOL, dtype, in_=xp, out=out.data_ptr() + coff * out.element_size(), B=B, H=H, W=W, Cin=C, in_cs=cs,
           Ho=Ho, Wo=Wo, Cout=C, out_cs=cs, ksize=2, stride=2))
    got = from_nhwc(out, C, coff).numpy()
    exp = _maxpool_statement(x.to(DEV))
    if dtype == "f16":              # the fp16 storage type saturates (csrc/common.h: med3(v, -65504, 65504); a NaN stores as -65504)
        exp = torch.where(torch.isnan(exp), torch.full_like(exp, -65504.0), exp.clamp(-65504.0, 65504.0))
    exp = exp.to(TD[dtype]).float().cpu().numpy()
    np.testing.assert_array_equal(got, exp)            # (NaN matches NaN)
    np.testing.assert_array_equal(np.signbit(got)[~np.isnan(got)], np.signbit(exp)[~np.isnan(exp)])     # -0 is not +0
    if cs > C:
        rest = torch.ones(cs, dtype=torch.bool)
        rest[coff:coff + C] = False
        assert bool((out[..., rest.to(DEV)].float() == 7.0).all().item())
