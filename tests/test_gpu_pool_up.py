"""GPU: the max-pool and up-sample + add backward (csrc/pool_up_bwd.hip, include/h3d.h section 2d) and their autograd functions
(h3d_amd/pool_up.py) against the yardstick of tests/pool_up_ref.py -- F.max_pool2d and F.conv_transpose2d(groups = C) + skip under torch
autograd on the CPU.  Max-pool: bit equality.  Up-sample: per tensor max |g - g64| <= 4 e32 + 1e-7 max |g64| (e32 = the error of the
yardstick's own float32 run) on random floats, bit equality on the lattice cases."""
import ctypes
import itertools

import pytest
import torch

import pool_up_ref as R
from gpu_helpers import DEV
import gpu_helpers as G
from h3d_amd import _lib, pool_up

pytestmark = pytest.mark.gpu
SENT = -777.25


def strided(t, cs, fill=float("nan")):
    """NCHW cpu tensor -> a device view of the same values whose pixels are `cs` floats apart inside a buffer filled with `fill`."""
    B, C, H, W = t.shape
    buf = torch.full((B, H, W, cs), fill, dtype=torch.float32, device=DEV)
    buf[..., :C] = t.float().permute(0, 2, 3, 1).to(DEV)
    return buf[..., :C].permute(0, 3, 1, 2)


def cl(t):
    return t.float().to(DEV).contiguous(memory_format=torch.channels_last)


# ---- max-pool --------------------------------------------------------------------------------------------------------------------------------
POOL_CASES = {"1x4x2x2": ((1, 4, 2, 2), True, None), "2x20x5x7_cs24": ((2, 20, 5, 7), True, 24), "1x64x8x6": ((1, 64, 8, 6), True, None),
              "random_2x8x7x9": ((2, 8, 7, 9), False, None)}


@pytest.mark.parametrize("name", sorted(POOL_CASES))
def test_max_pool_forward_and_grad_x_are_the_yardsticks_bits(name):
    shape, ties, cs = POOL_CASES[name]
    x, gy = R.pool_case(shape, 11, ties)
    y_ref, gx_ref = R.pool_yardstick(x, gy, torch.float32)
    xd = (strided(x, cs) if cs else cl(x)).requires_grad_(True)
    gd = strided(gy, cs) if cs else cl(gy)
    y = pool_up.max_pool2_autograd(xd)
    y.backward(gd)
    torch.cuda.synchronize()
    assert y.permute(0, 2, 3, 1).is_contiguous()                       # channels_last out
    assert torch.equal(y.detach().cpu(), y_ref) and torch.equal(xd.grad.cpu(), gx_ref)
    assert torch.equal(pool_up.max_pool2_backward(xd.detach(), gd).cpu(), gx_ref)
    assert torch.equal(pool_up.max_pool2_backward(x.to(DEV), gy.to(DEV)).cpu(), gx_ref)            # NCHW inputs
    H, W = shape[2:]
    g = xd.grad
    if H % 2:
        assert float(g[:, :, H - 1].abs().max()) == 0.0
    if W % 2:
        assert float(g[:, :, :, W - 1].abs().max()) == 0.0


def test_max_pool_backward_writes_only_its_elements():
    """The raw call into a sentinel-filled buffer with a channel stride: the pad channels and the words behind the last pixel keep the
    sentinel, every element of grad_x is written (no sentinel, no NaN left), a second call gives the same bits."""
    shape, cs = (2, 20, 5, 7), 24
    B, C, H, W = shape
    x, gy = R.pool_case(shape, 5)
    xv, gv = strided(x, cs).permute(0, 2, 3, 1), strided(gy, cs).permute(0, 2, 3, 1)
    outs = []
    for _ in range(2):
        buf = torch.full((B * H * W * cs + 64,), SENT, dtype=torch.float32, device=DEV)
        rc = _lib.lib().h3d_maxpool2_backward(_lib.ptr(xv), cs, _lib.ptr(gv), cs, _lib.ptr(buf), cs, B, C, H, W, _lib.stream_ptr())
        _lib.check(rc, "h3d_maxpool2_backward")
        torch.cuda.synchronize()
        img = buf[:B * H * W * cs].view(B, H, W, cs)
        assert bool((img[..., C:] == SENT).all()) and bool((buf[B * H * W * cs:] == SENT).all())
        outs.append(img[..., :C].permute(0, 3, 1, 2).cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], R.pool_yardstick(x, gy, torch.float32)[1])


def test_max_pool_backward_follows_torchs_scan_through_nans():
    """`v > max || isnan(v)`: a NaN takes the window, the LAST NaN of a window keeps it.  grad_x against F.max_pool2d's on windows with a
    NaN at each position, two NaNs, four NaNs, and a NaN beside +inf."""
    nan, inf = float("nan"), float("inf")
    wins = [[nan, 1, 2, 3], [1, nan, 2, 3], [1, 2, nan, 3], [3, 2, 1, nan], [nan, nan, 5, 1], [nan, 7, nan, 1], [1, nan, 9, nan],
            [nan, nan, nan, nan], [inf, nan, 0, 0], [nan, inf, 0, 0], [-inf, -inf, -inf, -inf], [2, 2, 2, 2]]
    x = torch.zeros(2, 4, 2 * len(wins), 2)
    for i, w in enumerate(wins):
        x[0, :, 2 * i:2 * i + 2] = torch.tensor(w).view(2, 2)
        x[1, :, 2 * i:2 * i + 2] = torch.tensor(w[::-1]).view(2, 2)          # the same windows in reverse order in the second image
    gy = torch.arange(1, 1 + 2 * 4 * len(wins), dtype=torch.float32).view(2, 4, len(wins), 1)
    want = R.pool_yardstick(x, gy, torch.float32)[1]
    assert int((want != 0).sum()) == gy.numel()
    got = pool_up.max_pool2_backward(cl(x), cl(gy))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)


# ---- up-sample + add: ordinary cases ---------------------------------------------------------------------------------------------------------
def gpu_up(c, need=(True, True, True)):
    """up_add_autograd forward + backward on the case -> (y, grad_x, grad_w, grad_skip), None where not needed."""
    x = (strided(c.x, c.cs) if c.cs else cl(c.x)).requires_grad_(need[0])
    w = c.w.float().to(DEV).requires_grad_(need[1])
    s = (strided(c.skip, c.cs) if c.cs else cl(c.skip)).requires_grad_(need[2])
    y = pool_up.up_add_autograd(x, w, s, c.f)
    if any(need):
        y.backward(strided(c.gy, c.cs) if c.cs else cl(c.gy))
    torch.cuda.synchronize()
    return y.detach(), x.grad, w.grad, s.grad


RATIOS = {}


@pytest.mark.parametrize("name", sorted(R.UP_CASES))
def test_up_add_every_case_vs_yardstick(name):
    c = R.up_case(name)
    r64, e32 = R.up_bounds(name)
    got = gpu_up(c)
    for nm, g, r, e in zip(R.NAMES, got, r64, e32):
        RATIOS[(name, nm)] = R.check("%s %s" % (name, nm), g, r, e)
    assert torch.equal(got[3].cpu().double(), c.gy)
    print("largest err / e32 so far: %.2f" % max(RATIOS.values()))


@pytest.mark.parametrize("name", R.LATTICE_CASES)
def test_up_add_lattice_cases_are_bit_equal_to_float64(name):
    """Bilinear weights and integers in [-8, 8]: every sum is exact in fp32 in any order (tests/test_oracle_pool_up.py pins that per
    case), so the forward, grad_x and grad_w are compared with torch.equal."""
    c = R.up_case(name, True)
    r64 = c.run(torch.float64)
    for nm, g, r in zip(R.NAMES, gpu_up(c), r64):
        g = g.cpu().double().contiguous()
        bad = ~(g == r)
        assert torch.equal(g, r), "%s %s: %d of %d elements differ, max |difference| %.3g" % (name, nm, int(bad.sum()), bad.numel(),
                                                                                             float((g - r)[bad].abs().max()))


# ---- up-sample + add: known answers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [2, 4, 8])
def test_one_hot_grad_y_gives_the_tap_weights_at_the_covering_pixels(f):
    B, C, H, W = 1, 8, 5, 6
    k, p = 2 * f, f // 2
    g = torch.Generator().manual_seed(f)
    w = torch.randn(C, 1, k, k, generator=g)
    x = torch.randn(B, C, H, W, generator=g)
    for oy, ox in ((0, 0), (H * f - 1, W * f - 1), (2 * f + 1, 3 * f + p), (f, W * f - 2)):
        gy = torch.zeros(B, C, H * f, W * f)
        gy[0, :, oy, ox] = 1.0
        gx, _ = pool_up.upsample_backward(cl(x), w.to(DEV), cl(gy), f, (True, False))
        want = torch.zeros(B, C, H, W)
        hits = 0
        for iy in range(H):
            for ix in range(W):
                ki, kj = oy - iy * f + p, ox - ix * f + p
                if 0 <= ki < k and 0 <= kj < k:
                    want[0, :, iy, ix] = w[:, 0, ki, kj]
                    hits += 1
        assert 1 <= hits <= 4 and torch.equal(gx.cpu(), want), (f, oy, ox)


@pytest.mark.parametrize("f", [2, 4, 8])
def test_grad_w_of_a_constant_x_is_the_windowed_sum_of_grad_y(f):
    B, C, H, W = 2, 4, 5, 3
    k, p = 2 * f, f // 2
    g = torch.Generator().manual_seed(10 + f)
    gy = torch.randint(-8, 9, (B, C, H * f, W * f), generator=g).float()          # integers: the sums are exact
    w = torch.randn(C, 1, k, k, generator=g)
    _, gw = pool_up.upsample_backward(cl(torch.ones(B, C, H, W)), w.to(DEV), cl(gy), f, (False, True))
    pad = torch.zeros(B, C, H * f + 2 * k, W * f + 2 * k)
    pad[:, :, k:k + H * f, k:k + W * f] = gy
    want = torch.zeros(C, 1, k, k)
    for ki in range(k):
        for kj in range(k):
            want[:, 0, ki, kj] = pad[:, :, k - p + ki:k - p + ki + H * f:f, k - p + kj:k - p + kj + W * f:f].sum((0, 2, 3))
    assert torch.equal(gw.cpu(), want)


# ---- up-sample + add: behaviour ------------------------------------------------------------------------------------------------------------------
def raw_up(c, want, ws=None, sentinel=False):
    """h3d_upsample_backward on the case's tensors -> (grad_x [B,C,H,W], grad_w tap-major) or None each."""
    xv, gv = cl(c.x).permute(0, 2, 3, 1), cl(c.gy).permute(0, 2, 3, 1)
    wp = pool_up.pack_up_weight(c.w.float().to(DEV))
    gx, gw = pool_up._up_backward_nhwc(xv, wp, gv, c.f, want, ws)
    torch.cuda.synchronize()
    return None if gx is None else gx.permute(0, 3, 1, 2), gw


def test_every_subset_of_outputs_and_a_second_call_give_the_same_bits():
    for name in ("f2_2x8x3x5", "f4_tile_h+1_w-1", "f8_chains_65", "f2_chains_80"):
        c = R.up_case(name)
        full, again = raw_up(c, (True, True)), raw_up(c, (True, True))
        assert all(torch.equal(a, b) for a, b in zip(full, again)), name
        for want in itertools.product((False, True), repeat=2):
            got = raw_up(c, want)
            for w_, a, b in zip(want, got, full):
                assert (a is None) == (not w_)
                if w_:
                    assert torch.equal(a, b), (name, want)


def test_up_backward_writes_only_its_elements():
    """Raw call, grad_x with a channel stride in a sentinel-filled buffer, grad_w and the workspace with sentinels behind them."""
    c = R.up_case("f4_c20_cs24")
    B, C, H, W, f, cs = c.B, c.C, c.H, c.W, c.f, c.cs
    xv, gv = strided(c.x, cs).permute(0, 2, 3, 1), strided(c.gy, cs).permute(0, 2, 3, 1)
    wp = pool_up.pack_up_weight(c.w.float().to(DEV))
    gxb = torch.full((B * H * W * cs + 64,), SENT, dtype=torch.float32, device=DEV)
    gwb = torch.full((4 * f * f * C + 64,), SENT, dtype=torch.float32, device=DEV)
    n = ctypes.c_size_t(0)
    _lib.check(_lib.lib().h3d_upsample_backward_workspace_bytes(B, C, H, W, f, ctypes.byref(n)), "workspace_bytes")
    ws = torch.full((n.value + 256,), 0x5a, dtype=torch.uint8, device=DEV)
    rc = _lib.lib().h3d_upsample_backward(_lib.ptr(xv), cs, _lib.ptr(wp), _lib.ptr(gv), cs, _lib.ptr(gxb), cs, _lib.ptr(gwb), B, C, H, W, f,
                                          _lib.ptr(ws), n.value, _lib.stream_ptr())
    _lib.check(rc, "h3d_upsample_backward")
    torch.cuda.synchronize()
    img = gxb[:B * H * W * cs].view(B, H, W, cs)
    assert bool((img[..., C:] == SENT).all()) and bool((gxb[B * H * W * cs:] == SENT).all()) and bool((gwb[4 * f * f * C:] == SENT).all())
    assert bool((ws[n.value:] == 0x5a).all())
    r64, e32 = R.up_bounds("f4_c20_cs24")
    R.check("raw grad_x", img[..., :C].permute(0, 3, 1, 2), r64[1], e32[1])
    R.check("raw grad_w", gwb[:4 * f * f * C].view(4 * f * f, C).t().reshape(C, 1, 2 * f, 2 * f), r64[2], e32[2])


def test_a_second_stream_gives_the_same_bits():
    c = R.up_case("f2_1x64x4x4")
    first = gpu_up(c)
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        second = gpu_up(c)
    s.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_nchw_and_channels_last_inputs_give_the_same_bits():
    for name in ("f2_2x8x3x5", "f8_1x64x4x4"):
        c = R.up_case(name)
        ref = gpu_up(c)
        x, w, s = [t.float().to(DEV).contiguous().requires_grad_(True) for t in (c.x, c.w, c.skip)]
        y = pool_up.up_add_autograd(x, w, s, c.f)
        y.backward(c.gy.float().to(DEV).contiguous())
        torch.cuda.synchronize()
        for a, b in zip(ref, (y.detach(), x.grad, w.grad, s.grad)):
            assert torch.equal(a, b), name
        gx, gw = pool_up.upsample_backward(x.detach(), w.detach(), c.gy.float().to(DEV), c.f)
        assert torch.equal(gx, ref[1]) and torch.equal(gw, ref[2])


@pytest.mark.parametrize("name", ["f2_1x64x4x4", "f4_2x8x3x5", "f8_c20_cs24"])
def test_autograd_forward_is_the_inference_ops_f32_launch(name):
    c = R.up_case(name)
    B, C, H, W, f = c.B, c.C, c.H, c.W, c.f
    cs = c.cs or C
    xb, xp = G.nhwc(c.x.float(), "f32", cs)
    sb, sp = G.nhwc(c.skip.float(), "f32", cs)
    wimg = c.w.float().reshape(C, 4 * f * f).t().contiguous().to(DEV)
    out = torch.empty(B, H * f, W * f, C, dtype=torch.float32, device=DEV)
    G.run(G.mk(_lib.OP_UPADD, "f32", in_=xp, in2=sp, w=wimg.data_ptr(), out=out.data_ptr(), B=B, H=H, W=W, Cin=C, in_cs=cs, in2_cs=cs,
               Ho=H * f, Wo=W * f, Cout=C, out_cs=C, ksize=2 * f, stride=f, out_mode=_lib.OUT_NHWC))
    y = gpu_up(c, (False, False, False))[0]
    assert torch.equal(y, out.permute(0, 3, 1, 2))


def test_needs_input_grad_is_honoured_and_the_skip_gradient_is_grad_y_itself():
    c = R.up_case("f2_2x8x3x5")
    full = gpu_up(c)
    for need in itertools.product((False, True), repeat=3):
        got = gpu_up(c, need)
        for n, a, b in zip(need, got[1:], full[1:]):
            assert (a is None) == (not n)
            if n:
                assert torch.equal(a, b), need
    s = cl(c.skip).requires_grad_(True)
    gy = cl(c.gy)
    y = pool_up.up_add_autograd(cl(c.x), c.w.float().to(DEV), s, c.f)
    (gs,) = torch.autograd.grad(y, s, gy)
    assert gs.data_ptr() == gy.data_ptr()              # passed on, not copied
