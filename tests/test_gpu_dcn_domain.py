"""The fp32 DCNv2 operator over the whole fp32 input domain: input scales from 1e-7 to 1e7, magnitudes spread inside one tensor, masks
outside [0, 1], NaN / inf in offsets, activations and masks, and the stream / per-call order of the device-derived scales.

One element-wise criterion against the fp64 oracle (oracle/dcn.py, fixed non-finite semantics pinned by tests/test_oracle_dcn.py):
    |y - y64| <= TAU (A + |b|),  A = sum |w| |column|  (oracle.dcn.dcn_v2_forward_absbound)
TAU = 2e-6 is about 10x what the reference's own fp32 arithmetic gives (tests/test_oracle_dcn.py calibrates it on the CPU).

Entry points: E1 dcn_v2_forward (NCHW, packed + cached pack), E2 the same with a channels_last input (no relayout, NHWC output),
E3 h3d_dcn_v2_forward_ws with a caller workspace, E4 the `DCN` module's fused launch, E5 the general kernel (stride 2 / dg 2);
arithmetics: the default (split operands on the fp16 matrix cores) and dcn_v2.OP_F32_MFMA."""
import numpy as np
import pytest
import torch

from gpu_helpers import DEV
from h3d_amd import _lib, dcn_v2
from oracle import dcn as odcn

pytestmark = pytest.mark.gpu

TAU = 2e-6

FAST = (3, 3, 1, 1, 1, 1, 1, 1, 1)
SHAPES = [(2, 64, 96, 24, 40), (1, 32, 40, 19, 23)]      # (B, C, Co, H, W); the second one leaves partial tiles
ARITH = ["default", "f32_mfma"]
WORST = {}


def _data(shape, g=1.0, seed=0, mlo=0.0, mhi=1.0, a=FAST):
    B, C, Co, H, W = shape
    kh, kw, sh, sw, ph, pw, dh, dw, dg = a
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    r = np.random.default_rng(seed)
    x = torch.from_numpy(r.uniform(-2, 2, (B, C, H, W)).astype(np.float32)) * g
    w = torch.from_numpy((r.uniform(-1, 1, (Co, C, kh, kw)) * 1.5 / np.sqrt(C * kh * kw)).astype(np.float32))
    b = torch.from_numpy(r.uniform(-1, 1, (Co,)).astype(np.float32)) * g
    off = torch.from_numpy(r.uniform(-3, 3, (B, 2 * dg * kh * kw, Ho, Wo)).astype(np.float32))
    m = torch.from_numpy(r.uniform(mlo, mhi, (B, dg * kh * kw, Ho, Wo)).astype(np.float32))
    return x, w, b, off, m


def _oracle(x, w, b, off, m, a=FAST, finite_only=False):
    y64 = odcn.dcn_v2_forward(x, w, b, off, m, *a, acc_dtype=torch.float64).double()
    A = odcn.dcn_v2_forward_absbound(x, w, off, m, *a, finite_only=finite_only)
    return y64, A + b.double().abs().view(1, -1, 1, 1)


def _arith(name):
    class _Ctx:
        def __enter__(self):
            self.old = dcn_v2.OP_F32_MFMA
            dcn_v2.OP_F32_MFMA = name == "f32_mfma"

        def __exit__(self, *e):
            dcn_v2.OP_F32_MFMA = self.old
    return _Ctx()


def e1(x, w, b, off, m, a=FAST):
    with torch.no_grad():
        return dcn_v2.dcn_v2_forward(x.to(DEV), w.to(DEV), b.to(DEV), off.to(DEV), m.to(DEV), *a).cpu()


def e2(x, w, b, off, m, a=FAST):
    xc = x.to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y = dcn_v2.dcn_v2_forward(xc, w.to(DEV), b.to(DEV), off.to(DEV), m.to(DEV), *a)
    assert y.is_contiguous(memory_format=torch.channels_last)
    return y.contiguous().cpu()


_WS = {}


def e3(x, w, b, off, m, a=FAST):
    B, C, H, W = x.shape
    Co = w.shape[0]
    L = _lib.lib()
    nws = int(L.h3d_dcn_v2_workspace_bytes(B, C, H, W, Co))
    ws = _WS.get(nws)
    if ws is None:
        ws = _WS.setdefault(nws, torch.empty(nws, dtype=torch.uint8, device=DEV))     # the SAME workspace across calls
    xd, wd, bd, od, md = [t.contiguous().to(DEV) for t in (x, w, b, off, m)]
    out = torch.empty(B, Co, H, W, device=DEV)
    _lib.check(L.h3d_dcn_v2_forward_ws(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(od), _lib.ptr(md), _lib.ptr(out), B, C, H, W, Co,
                                       *a, _lib.ptr(ws), nws, _lib.stream_ptr()), "forward_ws")
    return out.cpu()


ENTRIES = {"E1": e1, "E2": e2, "E3": e3}


def _check(tag, y, y64, bound, tau=TAU):
    y = y.double()
    fin = torch.isfinite(y64)
    assert torch.isfinite(y[fin]).all(), "%s: non-finite output where the oracle is finite" % tag
    ratio = float(((y - y64).abs()[fin] / (tau * bound[fin])).max())
    WORST[tag] = max(WORST.get(tag, 0.0), ratio)
    print("%s: worst |y - y64| / (tau (A + |b|)) = %.3g" % (tag, ratio))
    assert ratio <= 1.0, (tag, ratio)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("arith", ARITH)
def test_uniform_input_scale_every_entry_point(shape, arith):
    # case 1: x and b scaled by g, filters unchanged -- on E1, E2, E3 (and E5 below, E4 in its own test)
    for g in (1e-7, 1e-5, 1e-3, 1.0, 1e3, 1e5, 1e7):
        x, w, b, off, m = _data(shape, g)
        y64, bound = _oracle(x, w, b, off, m)
        with _arith(arith):
            for name, fn in ENTRIES.items():
                if name == "E3" and arith == "f32_mfma":
                    continue                 # (_ws has no flag: its arithmetic is the library default)
                _check("%s/%s/g=%g/%s" % (name, arith, g, shape), fn(x, w, b, off, m), y64, bound)


@pytest.mark.parametrize("arith", ARITH)
def test_general_kernel_uniform_scale_and_non_finite_offsets(arith):
    # E5: the general kernel (fp32 FMA) on non-fast configurations; case 1 and case 6
    for a in ((3, 3, 2, 2, 1, 1, 1, 1, 1), (3, 3, 1, 1, 1, 1, 1, 1, 2)):
        for g in (1e-7, 1e-5, 1e-3, 1.0, 1e3, 1e5, 1e7):
            x, w, b, off, m = _data((2, 32, 24, 17, 21), g, a=a)
            y64, bound = _oracle(x, w, b, off, m, a)
            with _arith(arith):
                _check("E5/%s/%s/g=%g" % (arith, a, g), e1(x, w, b, off, m, a), y64, bound)
        x, w, b, off, m = _data((2, 32, 24, 17, 21), 1.0, seed=3, a=a)
        _poison_offsets(off)
        y64, bound = _oracle(x, w, b, off, m, a)
        assert torch.isfinite(y64).all()
        with _arith(arith):
            y = e1(x, w, b, off, m, a)
        assert torch.isfinite(y).all()
        _check("E5/%s/%s/nonfinite-offsets" % (arith, a), y, y64, bound)


def _module(C, Co, w, b, g, seed=7):
    torch.manual_seed(seed)
    dcn = dcn_v2.DCN(C, Co, (3, 3), stride=1, padding=1, dilation=1, deformable_groups=1).to(DEV).eval()
    with torch.no_grad():
        dcn.weight.copy_(w)
        dcn.bias.copy_(b)
        dcn.conv_offset_mask.weight.copy_(torch.randn_like(dcn.conv_offset_mask.weight) * (0.02 / g))
        dcn.conv_offset_mask.bias.copy_(torch.randn_like(dcn.conv_offset_mask.bias) * 0.3)
    return dcn


def _module_oracle(dcn, x, finite_only=False):
    p = [t.detach().cpu() for t in (dcn.weight, dcn.bias, dcn.conv_offset_mask.weight, dcn.conv_offset_mask.bias)]
    y64 = odcn.dcn_module_forward(x, *p, acc_dtype=torch.float64).double()
    o = torch.nn.functional.conv2d(x, p[2], p[3], 1, 1)
    o1, o2, mk = torch.chunk(o, 3, dim=1)
    A = odcn.dcn_v2_forward_absbound(x, p[0], torch.cat((o1, o2), dim=1), torch.sigmoid(mk), *FAST, finite_only=finite_only)
    return y64, A + p[1].double().abs().view(1, -1, 1, 1)


@pytest.mark.parametrize("arith", ARITH)
def test_dcn_module_fused_launch_input_scale(arith):
    # E4, case 1 / 2: x scaled by g and conv_offset_mask.weight by 1 / g -- the offsets and the mask stay, the sampled activations scale
    B, C, Co, H, W = SHAPES[0]
    _, w, b, _, _ = _data(SHAPES[0])
    for g in (1e-7, 1e-5, 1e-3, 1.0, 1e3, 1e5, 1e7):
        x, _, _, _, _ = _data(SHAPES[0], g, seed=1)
        dcn = _module(C, Co, w, b * g, g)
        with _arith(arith), torch.no_grad():
            y = dcn(x.to(DEV)).cpu()
        y64, bound = _module_oracle(dcn, x)
        _check("E4/%s/g=%g" % (arith, g), y, y64, bound)
    x, _, _, _, _ = _data(SHAPES[0], 1.0, seed=2)
    x[1] *= 2.0 ** -17                                            # case 2: the second image 2^-17 below the first
    dcn = _module(C, Co, w, b, 1.0)
    with _arith(arith), torch.no_grad():
        y = dcn(x.to(DEV)).cpu()
    y64, bound = _module_oracle(dcn, x)
    _check("E4/%s/spread" % arith, y, y64, bound)


@pytest.mark.parametrize("arith", ARITH)
def test_spread_inside_one_tensor(arith):
    # case 2: one image at 1 and one at 2^-17; even channels at 1, odd ones at 1e-4
    x, w, b, off, m = _data(SHAPES[0], seed=4)
    x[1] *= 2.0 ** -17
    y64, bound = _oracle(x, w, b, off, m)
    x2 = x.clone()
    x2[1] = x[0]
    x2[:, 1::2] *= 1e-4
    y64b, boundb = _oracle(x2, w, b, off, m)
    with _arith(arith):
        for name, fn in ENTRIES.items():
            _check("%s/%s/spread-images" % (name, arith), fn(x, w, b, off, m), y64, bound)
            _check("%s/%s/spread-channels" % (name, arith), fn(x2, w, b, off, m), y64b, boundb)


@pytest.mark.parametrize("arith", ARITH)
def test_below_the_window_meets_the_documented_floor(arith):
    # case 3: image 1 at 1e-9 of image 0: |y - y64| <= 4e-7 max |x| sum_row |w| (+ TAU |b|), include/h3d.h
    x, w, b, off, m = _data(SHAPES[0], seed=5)
    x[1] *= 1e-9
    b = b * 1e-9
    y64, _ = _oracle(x, w, b, off, m)
    floor = 4e-7 * float(x.abs().max()) * w.double().abs().sum(dim=(1, 2, 3)).view(1, -1, 1, 1) + TAU * b.double().abs().view(1, -1, 1, 1)
    with _arith(arith):
        for name, fn in ENTRIES.items():
            y = fn(x, w, b, off, m).double()
            ratio = float(((y - y64).abs() / floor).max())
            # the floor alone is ~400x image 1's outputs (a kernel that drops image 1 meets it): image 1 must still be computed --
            # its relative L2 error within 5 % (fp16 subnormal operands give ~0.5 %; an unscaled split rounds them all to zero: 100 %)
            rel1 = float((y[1] - y64[1]).norm() / (y64[1] - b.double().view(-1, 1, 1)).norm())
            print("%s/%s/below-window: worst error / floor = %.3g, image 1 relative L2 error %.3g" % (name, arith, ratio, rel1))
            assert ratio <= 1.0, (name, ratio)
            assert rel1 <= 0.05, (name, rel1)


@pytest.mark.parametrize("arith", ARITH)
def test_mask_outside_unit_interval(arith):
    # case 4: the reference takes any fp32 mask; 3e4 * 4 is above fp16's 65504 before any scale
    for g in (1.0, 3e4):
        x, w, b, off, m = _data(SHAPES[0], g, seed=6, mlo=-4.0, mhi=4.0)
        y64, bound = _oracle(x, w, b, off, m)
        with _arith(arith):
            for name, fn in ENTRIES.items():
                y = fn(x, w, b, off, m)
                assert torch.isfinite(y).all(), name
                _check("%s/%s/mask[-4,4]/g=%g" % (name, arith, g), y, y64, bound)


def test_scale_is_per_call_not_stale():
    # case 5: the same filters (cached pack, E1) and the same explicit workspace (E3): x at 1e-6, 1e6, 1e-6
    x, w, b, off, m = _data(SHAPES[0], seed=8)
    wd, bd = w.to(DEV), b.to(DEV)
    for g in (1e-6, 1e6, 1e-6):
        y64, bound = _oracle(x * g, w, b * g, off, m)
        with torch.no_grad():
            y1 = dcn_v2.dcn_v2_forward((x * g).to(DEV), wd, bd * g, off.to(DEV), m.to(DEV), *FAST).cpu()
        _check("E1/cached/g=%g" % g, y1, y64, bound)
        _check("E3/same-ws/g=%g" % g, e3(x * g, w, b * g, off, m), y64, bound)


def _poison_offsets(off):
    off[0, 0, 3, 4] = float("nan")
    off[0, 7, 5, 6] = float("inf")
    off[-1, 12, 2, 2] = float("-inf")
    off[-1, 17, 6, 1] = float("nan")


@pytest.mark.parametrize("arith", ARITH)
def test_non_finite_offsets_gate_their_tap(arith):
    # case 6: a NaN / inf offset gates its tap out (the reference reads nothing): finite outputs that meet TAU
    x, w, b, off, m = _data(SHAPES[0], seed=9)
    _poison_offsets(off)
    y64, bound = _oracle(x, w, b, off, m)
    assert torch.isfinite(y64).all()
    with _arith(arith):
        for name, fn in ENTRIES.items():
            y = fn(x, w, b, off, m)
            assert torch.isfinite(y).all(), name
            _check("%s/%s/nonfinite-offsets" % (name, arith), y, y64, bound)


def _allowed_extra(bad_px, shape):
    """Outputs that MAY be non-finite beyond the oracle's (include/h3d.h): a non-finite pixel (b, c, py, px) in rows oy-1 .. oy+2 and
    columns ox-1 .. ox+2 of output (oy, ox), any output channel."""
    B, Co, H, W = shape
    ok = torch.zeros(shape, dtype=torch.bool)
    for (bb, py, px) in bad_px:
        ok[bb, :, max(py - 2, 0):py + 2, max(px - 2, 0):px + 2] = True
    return ok


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("g", [1.0, 1e-6])
def test_non_finite_activations_and_masks(arith, g):
    # case 7: one NaN and one +inf pixel in x, one NaN mask value; at g = 1e-6 the NaN must not poison the activation scale
    x, w, b, off, m = _data(SHAPES[0], g, seed=10)
    x[0, 5, 7, 9] = float("nan")
    x[1, 17, 12, 30] = float("inf")
    m[1, 4, 3, 3] = float("nan")
    y64, bound = _oracle(x, w, b, off, m, finite_only=True)
    bad_o = ~torch.isfinite(y64)
    assert bad_o.any()
    extra_ok = _allowed_extra([(0, 7, 9), (1, 12, 30)], tuple(y64.shape))
    with _arith(arith):
        for name, fn in ENTRIES.items():
            _check_non_finite("%s/%s/g=%g" % (name, arith, g), fn(x, w, b, off, m), y64, bound, extra_ok)


def _check_non_finite(tag, y, y64, bound, extra_ok):
    # every non-finite output of the oracle is non-finite in the kernel; the kernel's extra ones lie where include/h3d.h allows them;
    # the outputs finite in both meet TAU with A over the finite terms
    y = y.double()
    bad_o, bad_k = ~torch.isfinite(y64), ~torch.isfinite(y)
    assert bad_o.any()
    assert bad_k[bad_o].all(), "%s: a NaN / inf of the oracle became a finite number" % tag
    extra = bad_k & ~bad_o
    print("%s: %d non-finite outputs in the oracle, %d extra in the kernel" % (tag, int(bad_o.sum()), int(extra.sum())))
    assert not (extra & ~extra_ok).any(), tag
    fin = ~bad_k & ~bad_o
    ratio = float(((y - y64).abs()[fin] / (TAU * bound[fin])).max())
    print("%s/non-finite: worst finite ratio %.3g" % (tag, ratio))
    assert ratio <= 1.0, (tag, ratio)


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("g", [1.0, 1e-6])
def test_dcn_module_non_finite_activations(arith, g):
    # case 7 on E4: a NaN pixel gives NaN offsets and a NaN mask (sigmoid(NaN)) to every output whose offset convolution sees it, and
    # 0 * NaN is NaN there as in the reference; the +inf pixel likewise.  x at g with conv_offset_mask.weight at 1 / g.
    B, C, Co, H, W = SHAPES[0]
    x, w, b, _, _ = _data(SHAPES[0], g, seed=12)
    x[0, 5, 7, 9] = float("nan")
    x[1, 17, 12, 30] = float("inf")
    dcn = _module(C, Co, w, b, g)
    with _arith(arith), torch.no_grad():
        y = dcn(x.to(DEV)).cpu()
    y64, bound = _module_oracle(dcn, x, finite_only=True)
    _check_non_finite("E4/%s/g=%g" % (arith, g), y, y64, bound, _allowed_extra([(0, 7, 9), (1, 12, 30)], tuple(y64.shape)))


def test_scale_words_are_ordered_on_the_callers_stream():
    # case 8: E1 at g = 1e-6 on a non-default stream (the reductions and the scale words follow the caller's stream)
    x, w, b, off, m = _data(SHAPES[0], 1e-6, seed=11)
    y64, bound = _oracle(x, w, b, off, m)
    s = torch.cuda.Stream(device=DEV)
    xs, ws, bs, os_, ms = [t.to(DEV) for t in (x, w, b, off, m)]
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s), torch.no_grad():
        y = dcn_v2.dcn_v2_forward(xs, ws, bs, os_, ms, *FAST)
        for t in (xs, ws, bs, os_, ms):
            t.record_stream(s)
    s.synchronize()
    _check("E1/side-stream/g=1e-6", y.cpu(), y64, bound)

