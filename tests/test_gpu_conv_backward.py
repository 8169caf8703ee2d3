"""GPU: the convolution backward (csrc/conv_bwd.hip, include/h3d.h section 2c) and its autograd path (h3d_amd/conv.py) against the
yardstick of tests/conv_grad_ref.py -- F.conv2d (+ res) (-> relu) under torch autograd on the CPU.  Rule per case and tensor (the
project's own, DESIGN sections 13 and 18): max |g - g64| <= 4 e32 + 1e-7 max |g64|, e32 = the error of the yardstick's own float32 run."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as R
import heads_grad_ref as HR
from gpu_helpers import DEV
import gpu_helpers as G
from h3d_amd import _lib, conv, heads
from h3d_amd.dcn_v2 import dcn_v2_backward

pytestmark = pytest.mark.gpu
SENT = -777.25


def dev(t, channels_last=True):
    if t is None:
        return None
    t = t.to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t.contiguous()


def gpu_grads(c, need=(True,) * 4, general=False, channels_last=True):
    got = conv.conv2d_backward(dev(c.x, channels_last), c.w.to(DEV), dev(c.y(), channels_last) if c.relu else None, dev(c.gy, channels_last),
                               c.stride, c.padding, c.dilation, c.relu, need, general)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_case_vs_yardstick(name):
    c = R.case(name)
    g64, e32 = R.bounds(name)
    R.check(name, gpu_grads(c), g64, e32)


@pytest.mark.parametrize("name", R.GENERAL_ON_MFMA)
def test_general_kernels_on_matrix_core_configurations(name):
    c = R.case(name)
    g64, e32 = R.bounds(name)
    R.check(name + " general", gpu_grads(c, general=True), g64, e32)


@pytest.mark.parametrize("general", [False, True], ids=["auto", "general"])
@pytest.mark.parametrize("name", R.INT_GY_CASES)
def test_integer_grad_y_cases_are_bit_equal_to_the_float64_yardstick(name, general):
    """An integer grad_y on the gridded operands: every gradient is exact in fp32 in any split or summation order
    (tests/test_oracle_conv_backward.py pins that per case), so all four outputs are compared with torch.equal -- an error confined to the
    small elements of a tensor cannot hide under the max-norm rule.  auto: the matrix-core kernels where the configuration has them."""
    c = R.int_gy_case(name)
    got = gpu_grads(c, general=general)
    for nm, g, r in zip(R.NAMES, got, R.int_gy_exact(name)):
        if r is None:               # (no residual in the case: the yardstick has no grad_res)
            continue
        g = g.detach().cpu().contiguous()
        bad = ~(g == r)
        assert torch.equal(g, r), "%s %s: %d of %d elements differ, first at %s, max |difference| %.3g, max |ref| %.3g" % (
            name, nm, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), float((g - r)[bad].abs().max()), float(r.abs().max()))


def test_ungridded_random_case_with_a_gate_margin():
    c = R.make_random_case()
    p = c.pre().abs()
    assert float(p.min()) >= 1e-3 * float(p.max())
    g64, e32 = R.bounds_of(c)
    R.check("random", gpu_grads(c), g64, e32)
    R.check("random general", gpu_grads(c, general=True), g64, e32)


@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("general", [False, True])
def test_known_answers(i, general):
    what, c, ok = R.known_answer_cases()[i]
    gr = [None if t is None else t.cpu().double() for t in gpu_grads(c, general=general)]
    assert ok(gr), what


def test_agrees_with_dcn_v2_backward_at_zero_offsets_and_unit_mask():
    """An independent implementation in this repository: the DeformConv backward (csrc/dcn_bwd.hip) with zero offsets and a unit mask is
    the plain 3x3 stride-1 convolution's."""
    name = "s1_2x9x33_16to32"
    c = R.case(name)
    g64, e32 = R.bounds(name)
    B, Co, H, W = c.gy.shape
    gi, _, _, gw, gb = dcn_v2_backward(c.x.to(DEV), c.w.to(DEV), c.b.to(DEV), torch.zeros(B, 18, H, W, device=DEV), torch.ones(B, 9, H, W, device=DEV),
                                       c.gy.to(DEV), 3, 3, 1, 1, 1, 1, 1, 1, 1)
    gx, _, gw2, gb2 = gpu_grads(c)
    for nm, a, b, r, e in (("grad_x", gx, gi, g64[0], e32[0]), ("grad_weight", gw2, gw, g64[2], e32[2]), ("grad_bias", gb2, gb, g64[3], e32[3])):
        err = float((a.double() - b.double()).abs().max())
        limit = 4 * e + 1e-7 * float(r.abs().max())
        print("%s vs dcn_v2_backward: diff %.3g limit %.3g" % (nm, err, limit))
        assert err <= limit, nm


def test_every_subset_of_outputs_and_a_second_call_give_the_same_bits():
    for name in ("s1_2x9x33_48to80_res_relu", "s2_7x9_48to80", "k1_80to48", "g_5x3"):
        c = R.case(name)
        full = gpu_grads(c)
        again = gpu_grads(c)
        for nm, x, y in zip(R.NAMES, full, again):
            assert torch.equal(x, y), "run to run: " + nm
        for want in itertools.product((False, True), repeat=4):
            if not any(want):
                continue
            got = gpu_grads(c, want)
            for nm, w, x, y in zip(R.NAMES, want, got, full):
                assert (x is None) == (not w)
                if w:
                    assert torch.equal(x, y), (name, want, nm)


def raw_call(c, outs, general=False, ws=None):
    """h3d_conv2d_backward on the case's tensors with raw output pointers (grad_x, grad_res, grad_weight, grad_bias)."""
    xv, yv, gv = [dev(t).permute(0, 2, 3, 1) for t in (c.x, c.y(), c.gy)]
    geo, Ho, Wo = conv._geometry(tuple(c.x.shape), tuple(c.w.shape), c.stride, c.padding, c.dilation)
    flags = _lib.CONV_BWD_RELU if c.relu else 0
    if ws is None:
        ws = conv._workspace(xv.device, geo, flags)
    w = c.w.to(DEV)
    L = _lib.lib()
    fn = L.h3d_conv2d_backward_general if general else L.h3d_conv2d_backward
    rc = fn(xv.data_ptr(), xv.shape[3], w.data_ptr(), yv.data_ptr(), yv.shape[3], gv.data_ptr(), gv.shape[3], *outs, *geo, flags,
            ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "h3d_conv2d_backward")
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,general", [("s1_1x17x40_48to80_res_relu", False), ("s2_7x9_48to80", False), ("k1_80to48", False),
                                          ("s1_1x17x40_48to80_res_relu", True)])
def test_sentinels_behind_every_output(name, general):
    c = R.case(name)
    full = gpu_grads(c, general=general)
    PAD = 64
    shapes = [tuple(full[0].permute(0, 2, 3, 1).shape), tuple(full[1].permute(0, 2, 3, 1).shape), tuple(c.w.shape), tuple(c.b.shape)]
    offs = (4, 8, 1, 3)                      # floats: grad_x / grad_res 16-byte aligned (their contract), the others 4-byte aligned only
    bufs = [torch.full((int(np.prod(s)) + 2 * PAD,), SENT, device=DEV) for s in shapes]
    raw_call(c, [b.data_ptr() + 4 * o for b, o in zip(bufs, offs)], general)
    refs = [full[0].permute(0, 2, 3, 1), full[1].permute(0, 2, 3, 1), full[2], full[3]]
    for nm, b, o, s, ref in zip(R.NAMES, bufs, offs, shapes, refs):
        n = int(np.prod(s))
        assert bool((b[:o] == SENT).all()) and bool((b[o + n:] == SENT).all()), nm
        assert torch.equal(b[o:o + n].reshape(s), ref), nm
    with pytest.raises(RuntimeError, match="workspace"):       # a short workspace is an error, not an overrun
        raw_call(c, [b.data_ptr() + 4 * o for b, o in zip(bufs, offs)], general, ws=torch.empty(1024, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("name", ["s1_2x9x33_48to80_res_relu", "s2_8x9_16to32", "k1_80to48", "g_3x3_d2"])
def test_channel_strided_views_read_only_their_own_channels(name):
    c = R.case(name)
    full = gpu_grads(c)

    def wide(t, lead, extra):
        B, C, H, W = t.shape
        buf = torch.full((B, H, W, lead + C + extra), float("nan"), device=DEV)
        buf[..., lead:lead + C] = t.to(DEV).permute(0, 2, 3, 1)
        return buf[..., lead:lead + C].permute(0, 3, 1, 2)
    x, y, gy = wide(c.x, 4, 8), wide(c.y(), 8, 4), wide(c.gy, 4, 4)
    assert conv._cs(conv._as_nhwc(x, "x")) == c.x.shape[1] + 12 and conv._as_nhwc(x, "x").data_ptr() == x.data_ptr()      # used in place
    got = conv.conv2d_backward(x, c.w.to(DEV), y, gy, c.stride, c.padding, c.dilation, c.relu)
    for nm, a, b in zip(R.NAMES, got, full):
        assert torch.equal(a, b), nm


def test_non_default_stream():
    c = R.case("s1_2x9x33_32to144_res_relu")
    full = gpu_grads(c)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        got = gpu_grads(c)
    for x, y in zip(got, full):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["s1_2x9x33_48to80_res_relu", "s2_7x10_16to32", "g_stem7x7", "g_5x3"])
def test_contiguous_nchw_and_channels_last_inputs_give_equal_bits(name):
    c = R.case(name)
    a, b = gpu_grads(c, channels_last=True), gpu_grads(c, channels_last=False)
    for nm, x, y in zip(R.NAMES, a, b):
        assert torch.equal(x, y), nm
        if nm in ("grad_x", "grad_res"):
            assert x.permute(0, 2, 3, 1).is_contiguous() and y.permute(0, 2, 3, 1).is_contiguous()


# ---- the autograd function and the modules ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s1_2x9x33_48to80_res_relu", "s1_1x5x7_16to16", "s2_7x9_48to80", "k1_80to48"])
def test_autograd_forward_is_bit_equal_to_the_f32_op_conv_and_follows_a_parameter_update(name):
    c = R.case(name)
    ref, _ = G.conv(c.x, c.w, c.b, "f32", stride=c.stride[0], relu=c.relu, res=c.res)
    w, b = c.w.to(DEV).requires_grad_(True), c.b.to(DEV).requires_grad_(True)
    y = conv.conv2d_autograd(dev(c.x), w, b, c.stride, c.padding, c.dilation, dev(c.res), c.relu)
    assert y.permute(0, 2, 3, 1).is_contiguous() and y.requires_grad
    assert torch.equal(y.detach().cpu(), ref)
    assert torch.equal(ref, c.y())                       # gridded: the forward is exact in fp32 in any order
    with torch.no_grad():
        w.mul_(0.5)
        b.add_(0.125)
    ref2, _ = G.conv(c.x, c.w * 0.5, c.b + 0.125, "f32", stride=c.stride[0], relu=c.relu, res=c.res)
    y2 = conv.conv2d_autograd(dev(c.x, False), w, b, c.stride, c.padding, c.dilation, dev(c.res, False), c.relu)      # (contiguous NCHW in)
    assert torch.equal(y2.detach().cpu(), ref2) and not torch.equal(ref2, ref)
    assert y2.permute(0, 2, 3, 1).is_contiguous()


@pytest.mark.parametrize("name", ["s1_2x9x33_48to80_res_relu", "s2_8x10_16to32", "k1_448to64", "g_stem7x7", "g_3x3_d2", "g_5x3"])
def test_autograd_gradients_without_any_vendor_convolution(name, monkeypatch):
    """Forward and backward with torch's convolutions patched to raise (as test_gpu_dcn.py does for DCN), in eager autograd with
    needs_input_grad honoured."""
    c = R.case(name)
    g64, e32 = R.bounds(name)
    y_ref = c.y(torch.float64)

    def boom(*a, **kw):
        raise AssertionError("a torch convolution was called inside h3d_amd.conv")
    leaves = [dev(c.x, False).requires_grad_(True), c.w.to(DEV).requires_grad_(True), c.b.to(DEV).requires_grad_(True)]
    res = None if c.res is None else dev(c.res).requires_grad_(True)
    monkeypatch.setattr(torch.nn.Conv2d, "forward", boom)
    monkeypatch.setattr(torch.nn.functional, "conv2d", boom)
    monkeypatch.setattr(torch, "conv2d", boom)
    y = conv.conv2d_autograd(leaves[0], leaves[1], leaves[2], c.stride, c.padding, c.dilation, res, c.relu)
    y.backward(dev(c.gy, False))
    # only the weight needs a gradient: the others come back None
    w_only = c.w.to(DEV).requires_grad_(True)
    conv.conv2d_autograd(dev(c.x), w_only, c.b.to(DEV), c.stride, c.padding, c.dilation, dev(c.res), c.relu).backward(dev(c.gy))
    monkeypatch.undo()
    err = float((y.detach().cpu().double() - y_ref).abs().max())
    assert err <= 1e-5 * float(y_ref.abs().max()), err
    R.check(name + " autograd", [leaves[0].grad, None if res is None else res.grad, leaves[1].grad, leaves[2].grad], g64, e32)
    assert leaves[0].grad.shape == c.x.shape
    assert torch.equal(w_only.grad, leaves[1].grad)


def test_trainable_conv2d_is_nn_conv2d_with_res_and_relu():
    c = R.case("k1_80to48")
    m = conv.TrainableConv2d(80, 48, 1).to(DEV)
    ref = torch.nn.Conv2d(80, 48, 1)
    with torch.no_grad():
        ref.weight.copy_(c.w)
        ref.bias.copy_(c.b)
    m.load_state_dict(ref.state_dict())
    y = m(dev(c.x), res=dev(c.res), relu=True)
    assert torch.equal(y.detach().cpu(), c.y())
    y.backward(dev(c.gy))
    g64, e32 = R.bounds("k1_80to48")
    R.check("TrainableConv2d", [None, None, m.weight.grad, m.bias.grad], g64, e32)


def _rule(name, got, g64, g32):
    fails = []
    for i, (g, r, a) in enumerate(zip(got, g64, g32)):
        e = float((a.double() - r).abs().max())
        err = float((g.detach().cpu().double() - r).abs().max())
        limit = 4 * e + 1e-7 * float(r.abs().max())
        print("%s tensor %d: err %.3g e32 %.3g ratio %.3g limit %.3g" % (name, i, err, e, err / e if e else 0.0, limit))
        if not err <= limit:
            fails.append((i, err, limit))
    assert not fails, (name, fails)


def _block_restatement(sd, prefix, cin, cout, stride):
    """The reference's BasicBlock as nn modules, BatchNorm in eval mode."""
    mods = {"conv1": torch.nn.Conv2d(cin, cout, 3, stride, 1, bias=False), "bn1": torch.nn.BatchNorm2d(cout),
            "conv2": torch.nn.Conv2d(cout, cout, 3, 1, 1, bias=False), "bn2": torch.nn.BatchNorm2d(cout)}
    net = torch.nn.ModuleDict(mods)
    net.load_state_dict({k[len(prefix):]: v for k, v in sd.items()})
    return net.eval().double()


def _block_folded(x, w1, b1, w2, b2, res, stride):
    h = torch.relu(F.conv2d(x, w1, b1, stride, 1))
    return torch.relu(F.conv2d(h, w2, b2, 1, 1) + (x if res is None else res))


def _block_case(stride, tries=400):
    """A block, an input (and the residual of a stride-2 block) whose two pre-activations keep min |pre| >= 1e-5 max |pre|: a bounded
    search on the CPU, so that the gates do not depend on the summation order."""
    cin, cout = (32, 32) if stride == 1 else (16, 32)
    for s in range(tries):
        sd = R.make_block_state_dict(cin, cout, seed=100 * stride + s)
        blk = conv.TrainableBasicBlock(sd, "level2.tree1.", stride)
        g = torch.Generator().manual_seed(900 + s)
        x = torch.randn(2, cin, 9, 33, generator=g)
        res = None if stride == 1 else torch.randn(2, cout, 5, 17, generator=g)
        p = [t.detach().double() for t in (blk.weight1, blk.bias1, blk.weight2, blk.bias2)]
        pre1 = F.conv2d(x.double(), p[0], p[1], stride, 1)
        pre2 = F.conv2d(torch.relu(pre1), p[2], p[3], 1, 1) + (x if res is None else res).double()
        if all(float(t.abs().min()) >= 1e-5 * float(t.abs().max()) for t in (pre1, pre2)):
            return sd, blk, x, res, torch.randn(pre2.shape, generator=g)
    raise AssertionError("no block with a gate margin in %d tries" % tries)


@pytest.mark.parametrize("stride", [1, 2])
def test_trainable_basic_block_vs_restatement(stride):
    sd, blk, x, res, gy = _block_case(stride)
    cin, cout = x.shape[1], gy.shape[1]
    # the folded parameters compute what the nn modules with eval-mode BatchNorm compute
    net = _block_restatement(sd, "level2.tree1.", cin, cout, stride)
    with torch.no_grad():
        want = torch.relu(net["bn2"](net["conv2"](torch.relu(net["bn1"](net["conv1"](x.double()))))) + (x if res is None else res).double())

    def cpu(dtype):
        leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (x, blk.weight1, blk.bias1, blk.weight2, blk.bias2)]
        r = None if res is None else res.to(dtype).clone().requires_grad_(True)
        y = _block_folded(*leaves, r, stride)
        return y.detach(), torch.autograd.grad(y, leaves + ([] if r is None else [r]), gy.to(dtype))
    y64, g64 = cpu(torch.float64)
    _, g32 = cpu(torch.float32)
    assert float((y64 - want).abs().max()) <= 1e-5 * float(want.abs().max())
    blk = blk.to(DEV)
    xd = dev(x).requires_grad_(True)
    rd = None if res is None else dev(res).requires_grad_(True)
    y = blk(xd, rd)
    assert float((y.detach().cpu().double() - y64).abs().max()) <= 1e-5 * float(y64.abs().max())
    y.backward(dev(gy))
    got = [xd.grad, blk.weight1.grad, blk.bias1.grad, blk.weight2.grad, blk.bias2.grad] + ([] if rd is None else [rd.grad])
    _rule("BasicBlock stride %d" % stride, got, g64, g32)


def test_five_sgd_steps_on_a_block_and_heads_chain():
    """TrainableBasicBlock -> heads_autograd on a 64-channel 16 x 16 map, squared error against fixed targets.  The learning rate is the
    smallest of a fixed list that lowers the CPU restatement's loss by 10 % in five steps; the GPU loss follows the CPU's."""
    g = torch.Generator().manual_seed(11)
    sd = R.make_block_state_dict(64, 64, seed=77)
    blk = conv.TrainableBasicBlock(sd, "level2.tree1.", 1)
    x = torch.randn(1, 64, 16, 16, generator=g)
    chans = {"a": 3, "b": 2}
    hp = {h: [(torch.rand(64, 64, 3, 3, generator=g) * 2 - 1) / 24.0, (torch.rand(64, generator=g) * 2 - 1) / 24.0,
              (torch.rand(c, 64, 1, 1, generator=g) * 2 - 1) / 8.0, torch.zeros(c)] for h, c in chans.items()}
    tgt = {h: torch.randn(1, c, 16, 16, generator=g) for h, c in chans.items()}
    start = [t.detach().clone() for t in (blk.weight1, blk.bias1, blk.weight2, blk.bias2)]

    def cpu_losses(lr):
        bp = [t.clone().requires_grad_(True) for t in start]
        ps = {h: [t.clone().requires_grad_(True) for t in v] for h, v in hp.items()}
        opt = torch.optim.SGD(bp + [t for v in ps.values() for t in v], lr=lr)
        vals = []
        for _ in range(6):
            opt.zero_grad()
            feat = _block_folded(x, *bp, None, 1)
            loss = sum(((HR.forward(feat, v[0], v[1], v[2].reshape(v[2].shape[0], -1), v[3]) - tgt[h]) ** 2).mean() for h, v in ps.items())
            vals.append(float(loss.detach()))
            loss.backward()
            opt.step()
        return vals
    lr = None
    for cand in (1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 1.0):
        cpu = cpu_losses(cand)
        if np.isfinite(cpu).all() and cpu[5] <= 0.9 * cpu[0]:
            lr = cand
            break
    assert lr is not None, cpu
    blk = blk.to(DEV)
    ps = {h: [t.to(DEV).requires_grad_(True) for t in v] for h, v in hp.items()}
    opt = torch.optim.SGD(list(blk.parameters()) + [t for v in ps.values() for t in v], lr=lr)
    xd, td = dev(x), {h: t.to(DEV) for h, t in tgt.items()}
    vals = []
    for _ in range(6):
        opt.zero_grad()
        out = heads.heads_autograd(blk(xd), {h: tuple(v) for h, v in ps.items()})
        loss = sum(((out[h] - td[h]) ** 2).mean() for h in chans)
        vals.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print("SGD lr %g: cpu %s gpu %s" % (lr, cpu, vals))
    assert np.isfinite(vals).all()
    for i in (0, 5):
        assert abs(vals[i] - cpu[i]) <= 5e-4 * abs(cpu[i]), (i, vals[i], cpu[i])        # three digits
