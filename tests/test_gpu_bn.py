"""GPU: h3d_amd.bn (csrc/bn.hip, include/h3d.h section 2e) against the yardsticks of tests/bn_ref.py.

Rule per tensor: max |t - t64| <= 4 e32 + 1e-7 max |t64|, t64 = torch in float64; e32 = the float32 numpy restatement's error in training
mode, torch's float32 error in evaluation mode.  The backward's ReLU mask is [y > 0] of the GPU's own output in all three arithmetics,
as the operator takes it from its saved output.  Tensors: save_mean, the biased variance, y, the updated running statistics, grad_x,
grad_gamma, grad_beta (evaluation: y and the three gradients)."""
import contextlib
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R
from gpu_helpers import DEV
from h3d_amd import _lib, bn
from test_oracle_bn import lattice

pytestmark = pytest.mark.gpu

# the two shapes of the implementation's own tile constants (bn.plan): C = 4 -> workgroups of 256 pixels x 8 terms = chunks of 2048 pixels,
# C = 8 -> 128 x 8 = 1024; (2,4,260,260) has 67 slots (> 64: two chains, of 34 and 33), (1,8,301,300) has 89 (chains of 45 and 44: the
# last one short), and in both the last chunk is partial
SLOTS_SHAPE, SHORT_CHAIN_SHAPE = (2, 4, 260, 260), (1, 8, 301, 300)
SHAPES = [(1, 4, 1, 2), (2, 20, 5, 7), (1, 64, 8, 6), (2, 512, 2, 2), (2, 16, 96, 96), SLOTS_SHAPE, SHORT_CHAIN_SHAPE]
STRIDE = {(2, 20, 5, 7): 24}
SENT = 12345.0
WORST = {}


@contextlib.contextmanager
def no_vendor_batch_norm():
    """torch's batch norms raise: whatever runs inside is this library's kernels (and torch's element-wise ops)."""
    def refuse(*a, **kw):
        raise AssertionError("a vendor batch norm was called")
    names = [(torch, "batch_norm"), (F, "batch_norm"), (torch, "native_batch_norm"), (torch, "miopen_batch_norm")]
    saved = [(m, n, getattr(m, n)) for m, n in names if hasattr(m, n)]
    for m, n, _ in saved:
        setattr(m, n, refuse)
    try:
        yield
    finally:
        for m, n, f in saved:
            setattr(m, n, f)


def dev(a, shape=None):
    """numpy -> device tensor; a [B,C,H,W] map of a shape in STRIDE lives at that channel stride inside a NaN-filled buffer."""
    t = torch.from_numpy(np.asarray(a))
    cs = STRIDE.get(tuple(t.shape)) if t.dim() == 4 else None
    if cs is None:
        return t.to(DEV)
    B, C, H, W = t.shape
    buf = torch.full((B, H, W, cs), float("nan"), dtype=torch.float32, device=DEV)
    buf[..., :C] = t.permute(0, 2, 3, 1).to(DEV)
    return buf[..., :C].permute(0, 3, 1, 2)


def gpu_run(x, o, res, relu, training, need=(True, True, True, True)):
    """forward + backward through the raw calls -> dict of device tensors like bn_ref's."""
    xd, gd = dev(x), dev(o["grad_y"])
    rd = dev(o["res"]) if res else None
    gamma, beta, rm, rv = (dev(o[k]) for k in ("gamma", "beta", "running_mean", "running_var"))
    with no_vendor_batch_norm():
        if training:
            y, mean, var, invstd = bn.batch_norm_forward(xd, gamma, beta, None, None, True, rm, rv, R.MOMENTUM, R.EPS, rd, relu)
        else:
            y, mean, var, invstd = bn.batch_norm_forward(xd, gamma, beta, rm, rv, False, None, None, R.MOMENTUM, R.EPS, rd, relu)
        gx, gr, gw, gb = bn.batch_norm_backward(xd, y, gd, gamma, mean, invstd, training, relu, need)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, var=var, invstd=invstd, running_mean=rm, running_var=rv, grad_x=gx, grad_res=gr, grad_gamma=gw, grad_beta=gb,
                grad_y=gd)


def test_the_tile_shapes_are_what_their_names_say():
    chunk, slots = bn.plan(*SLOTS_SHAPE)
    assert (chunk, slots) == (2048, 67) and slots > 64 and (2 * 260 * 260) % chunk
    chunk, slots = bn.plan(*SHORT_CHAIN_SHAPE)
    groups = -(-slots // 64)
    assert (chunk, slots) == (1024, 89) and groups == 2 and slots % groups and (301 * 300) % chunk
    assert bn.plan(2, 16, 96, 96)[1] > 1 and bn.plan(2, 512, 2, 2)[1] == 1 and bn.plan(2, 20, 5, 7)[1] == 1


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_every_tensor_within_the_rule(shape, kind):
    x, o = R.data(shape, kind), R.operands(shape)
    worst = {}
    for training, (res, relu) in itertools.product((True, False), R.MODES):
        got = gpu_run(x, o, res, relu, training)
        mask = (got["y"] > 0).cpu().numpy()
        t64, t32 = R.yardsticks(x, o, res, relu, training, mask)
        names = ["y", "grad_x", "grad_gamma", "grad_beta"] + (["mean", "var", "running_mean", "running_var"] if training else [])
        for k in names:
            what = "%s %s res %d relu %d %s" % (shape, kind, res, relu, k)
            key = ("train " if training else "eval ") + k
            worst[key] = max(worst.get(key, 0.0), R.check(what, got[k], t64[k], t32[k]))
        # exact: the skip's gradient is grad_y under the mask of the saved output; without ReLU the very tensor
        if res:
            want = torch.where(got["y"] > 0, got["grad_y"], torch.zeros_like(got["grad_y"])) if relu else got["grad_y"]
            assert torch.equal(got["grad_res"], want) and (relu or got["grad_res"] is got["grad_y"])
        if not training:
            assert torch.equal(got["running_mean"].cpu(), torch.from_numpy(o["running_mean"]))
            assert torch.equal(got["running_var"].cpu(), torch.from_numpy(o["running_var"]))
        inv64 = 1.0 / np.sqrt(t64["var"] + R.EPS)
        assert np.abs(got["invstd"].cpu().numpy() - inv64).max() <= 1e-5 * inv64.max()
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("%s %s: err / e32 <= %s" % (shape, kind, ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    print("so far: %s" % ", ".join("%s %.2f" % kv for kv in sorted(WORST.items())))


def test_the_lattice_statistics_are_exact():
    x = lattice()
    o = R.operands(x.shape)
    got = gpu_run(x, o, False, False, True)
    t64 = R.restate(x, o, False, False, True, np.float64)
    assert torch.equal(got["mean"].cpu().double(), torch.from_numpy(t64["mean"]))
    assert torch.equal(got["var"].cpu().double(), torch.from_numpy(t64["var"]))


BITS_SHAPES = [(2, 20, 5, 7), (2, 16, 96, 96), SHORT_CHAIN_SHAPE]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", BITS_SHAPES, ids=["x".join(map(str, s)) for s in BITS_SHAPES])
def test_equal_bits_whatever_is_requested_and_wherever_it_runs(shape, training):
    x, o = R.data(shape, "relu"), R.operands(shape)
    keys = ("y", "mean", "var", "invstd", "running_mean", "running_var", "grad_x", "grad_res", "grad_gamma", "grad_beta")
    base = gpu_run(x, o, True, True, training)

    def same(other, need=(True,) * 4):
        for k, n in zip(keys, (True,) * 6 + tuple(need)):
            if n:
                assert torch.equal(base[k].view(torch.int32), other[k].view(torch.int32)), k
            else:
                assert other[k] is None, k
    same(gpu_run(x, o, True, True, training))                                       # a second call
    for need in itertools.product((False, True), repeat=4):                         # every subset of the gradients
        same(gpu_run(x, o, True, True, training, need), need)
    side = torch.cuda.Stream(device=DEV)                                            # a second stream
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = gpu_run(x, o, True, True, training)
    same(other)
    # NCHW and channels_last inputs
    if shape not in STRIDE:
        runs = []
        for fmt in (torch.contiguous_format, torch.channels_last):
            xd, gd, rd = (torch.from_numpy(a).to(DEV).contiguous(memory_format=fmt) for a in (x, o["grad_y"], o["res"]))
            gamma, beta, rm, rv = (torch.from_numpy(o[k]).to(DEV) for k in ("gamma", "beta", "running_mean", "running_var"))
            xd.requires_grad_(True), rd.requires_grad_(True), gamma.requires_grad_(True), beta.requires_grad_(True)
            with no_vendor_batch_norm():
                y = bn.batch_norm_autograd(xd, gamma, beta, rm, rv, training, R.MOMENTUM, R.EPS, rd, True)
                y.backward(gd)
            assert y.is_contiguous(memory_format=torch.channels_last)       # (a leaf's .grad takes the leaf's own layout)
            runs.append(dict(y=y.detach(), running_mean=rm, running_var=rv, grad_x=xd.grad, grad_res=rd.grad, grad_gamma=gamma.grad,
                             grad_beta=beta.grad))
        torch.cuda.synchronize()
        for r in runs:
            for k, v in r.items():
                assert torch.equal(v.view(torch.int32), base[k].view(torch.int32)), k


def test_one_value_per_channel_is_refused_in_training():
    x = torch.randn(1, 8, 1, 1, device=DEV)
    w, b, rm, rv = torch.ones(8, device=DEV), torch.zeros(8, device=DEV), torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bn.batch_norm_autograd(x, w, b, rm, rv, True)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bn.batch_norm_forward(x, w, b, training=True)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
    y = torch.empty(1, 1, 1, 8, device=DEV)
    rc = _lib.lib().h3d_batch_norm_forward(_lib.ptr(x), 8, _lib.ptr(w), _lib.ptr(b), None, 8, _lib.ptr(y), 8, None, None, None, None, None,
                                           1, 8, 1, 1, 1, 0, 0.1, 1e-5, _lib.ptr(ws), 4096, _lib.stream_ptr())
    assert rc == -1 and "more than 1 value per channel" in _lib.lib().h3d_last_error().decode()
    y = bn.batch_norm_autograd(x, w, b, rm, rv, False)                              # evaluation takes it
    torch.cuda.synchronize()
    assert torch.allclose(y, x / np.sqrt(1 + 1e-5), rtol=1e-6, atol=0)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_strided_outputs_stay_inside_their_channels(training):
    """(2,20,5,7): every map at channel stride 24 inside a NaN-filled (inputs) / sentinel-filled (outputs) buffer, sentinels behind every
    output; the values are the dense call's bits."""
    shape, cs = (2, 20, 5, 7), 24
    B, C, H, W = shape
    x, o = R.data(shape, "normal"), R.operands(shape)
    base = gpu_run(x, o, True, True, training)
    xd, gd, rd = dev(x).permute(0, 2, 3, 1), dev(o["grad_y"]).permute(0, 2, 3, 1), dev(o["res"]).permute(0, 2, 3, 1)
    vec = lambda a=None: torch.cat([torch.from_numpy(a).to(DEV) if a is not None else torch.full((C,), SENT, device=DEV), torch.full((12,), SENT, device=DEV)])
    img = lambda: torch.full((B * H * W * cs + 64,), SENT, dtype=torch.float32, device=DEV)
    gamma, beta = vec(o["gamma"]), vec(o["beta"])
    mean, var = (vec(o["running_mean"]), vec(o["running_var"])) if not training else (vec(), vec())
    rm, rv, invstd, gw, gb = vec(o["running_mean"]), vec(o["running_var"]), vec(), vec(), vec()
    y, gx, gr = img(), img(), img()
    n = ctypes.c_size_t(0)
    _lib.check(_lib.lib().h3d_batch_norm_workspace_bytes(B, C, H, W, ctypes.byref(n)), "workspace_bytes")
    ws = torch.full((n.value + 256,), 0x5a, dtype=torch.uint8, device=DEV)
    L, p = _lib.lib(), _lib.ptr
    _lib.check(L.h3d_batch_norm_forward(p(xd), cs, p(gamma), p(beta), p(rd), cs, p(y), cs, p(mean), p(var), p(invstd), p(rm) if training else None,
                                        p(rv) if training else None, B, C, H, W, int(training), 1, R.MOMENTUM, R.EPS, p(ws), n.value,
                                        _lib.stream_ptr()), "forward")
    _lib.check(L.h3d_batch_norm_backward(p(xd), cs, p(y), cs, p(gd), cs, p(gamma), p(mean), p(invstd), p(gx), cs, p(gr), cs, p(gw), p(gb), B, C, H, W,
                                         int(training), 1, p(ws), n.value, _lib.stream_ptr()), "backward")
    torch.cuda.synchronize()
    for name, buf in (("y", y), ("grad_x", gx), ("grad_res", gr)):
        m = buf[:B * H * W * cs].view(B, H, W, cs)
        assert bool((m[..., C:] == SENT).all()) and bool((buf[B * H * W * cs:] == SENT).all()), name
        assert torch.equal(m[..., :C].permute(0, 3, 1, 2), base[name]), name
    for name, buf in (("mean", mean), ("var", var), ("invstd", invstd), ("running_mean", rm), ("running_var", rv), ("grad_gamma", gw), ("grad_beta", gb)):
        assert bool((buf[C:] == SENT).all()) and torch.equal(buf[:C], base[name]), name
    assert bool((ws[n.value:] == 0x5a).all())


def test_the_module_counts_its_batches_and_honours_needs_input_grad():
    m = bn.TrainableBatchNorm2d(16, eps=R.EPS, momentum=R.MOMENTUM).to(DEV)
    ref = torch.nn.BatchNorm2d(16, eps=R.EPS, momentum=R.MOMENTUM).double()
    assert list(m.state_dict()) == list(ref.state_dict())
    x = torch.from_numpy(R.data((2, 16, 6, 5), "normal")).to(DEV)
    res = torch.from_numpy(R.operands((2, 16, 6, 5))["res"]).to(DEV).requires_grad_(True)
    m.weight.requires_grad_(False)
    with no_vendor_batch_norm():
        for _ in range(3):
            y = m(x, res, relu=True)
        y.sum().backward()
        m.eval()
        ye = m(x, res, relu=True)
    for _ in range(3):
        want = torch.relu(ref(x.cpu().double()) + res.detach().cpu().double())
    torch.cuda.synchronize()
    assert int(m.num_batches_tracked) == 3 and m.weight.grad is None and m.bias.grad is not None and res.grad is not None
    assert torch.equal(res.grad, (y > 0).float())
    assert torch.allclose(y.detach().cpu().double(), want, rtol=0, atol=1e-5)
    assert torch.allclose(m.running_var.cpu().double(), ref.running_var, rtol=1e-6, atol=0)
    assert torch.allclose(ye.detach().cpu().double(), torch.relu(ref.eval()(x.cpu().double()) + res.detach().cpu().double()), rtol=0, atol=1e-5)
    assert int(m.num_batches_tracked) == 3
