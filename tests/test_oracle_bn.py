"""CPU: the yardsticks of tests/bn_ref.py against each other, the lattice conditions of the exact GPU test, the argument checks of
h3d_batch_norm_forward / _backward (they run before the first HIP call, so without a device), and the keys of TrainableDLASeg(bn=...)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bn_ref as R
import network_grad_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 4, 1, 2), (2, 20, 5, 7), (2, 8, 9, 11)]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_the_numpy_restatement_is_the_torch_yardstick_in_float64(kind, training):
    for shape in SHAPES:
        x, o = R.data(shape, kind), R.operands(shape)
        for res, relu in R.MODES:
            a = R.torch_bn(x, o, res, relu, training, torch.float64)
            b = R.restate(x, o, res, relu, training, np.float64, mask=a["y"] > 0)
            for k, v in a.items():
                if v is None:
                    assert b[k] is None
                    continue
                # two float64 evaluations: 1e-12 of the tensor's size plus, behind invstd <= 316 of a (near-)constant channel, 1e-10
                assert np.abs(v - b[k]).max() <= 1e-12 * np.abs(v).max() + 1e-10, (shape, res, relu, k)


def test_the_running_update_is_nn_batchnorm2ds():
    shape = (2, 8, 5, 3)
    x, o = R.data(shape, "normal"), R.operands(shape)
    m = torch.nn.BatchNorm2d(8, eps=R.EPS, momentum=R.MOMENTUM).double()
    with torch.no_grad():
        m.running_mean.copy_(torch.from_numpy(o["running_mean"]))
        m.running_var.copy_(torch.from_numpy(o["running_var"]))
    m.train()(torch.from_numpy(x).double())
    t = R.torch_bn(x, o, False, False, True, torch.float64)
    rm, rv = R.running_update(o["running_mean"], o["running_var"], t["mean"], t["var"], 30)
    for a, b, c in ((rm, t["running_mean"], m.running_mean), (rv, t["running_var"], m.running_var)):
        assert np.abs(a - b).max() <= 1e-14 and np.abs(a - c.numpy()).max() <= 1e-14
    assert int(m.num_batches_tracked) == 1


def lattice():
    """Integers in [-8, 8] at (2, 8, 4, 4): N = 32, sum x <= 256, and with mean = k / 32 the centred squares are integers in units of
    1 / 32^2, their sum at most 32 (16 * 32)^2 = 2^23 units: every sum is below 2^24 units and exact in float32 in any order."""
    rs = np.random.RandomState(3)
    return rs.randint(-8, 9, (2, 8, 4, 4)).astype(np.float32)


def test_the_lattice_is_exact_in_float32():
    x = lattice()
    o = R.operands(x.shape)
    a, b = R.restate(x, o, False, False, True, np.float64), R.restate(x, o, False, False, True, np.float32)
    assert np.array_equal(a["mean"], b["mean"].astype(np.float64)) and np.array_equal(a["var"], b["var"].astype(np.float64))
    units = (x.astype(np.float64) * 32 - x.astype(np.float64).sum((0, 2, 3)).reshape(1, 8, 1, 1)) ** 2
    assert units.sum((0, 2, 3)).max() < 2 ** 24 and np.array_equal(units, np.round(units))
    # the same sums in another order (chains over a permutation) have the same bits
    perm = np.random.RandomState(4).permutation(32)
    rows = np.transpose(x, (0, 2, 3, 1)).reshape(32, 8)[perm]
    m = np.zeros(8, np.float32)
    for r in rows:
        m = m + r
    m = m / np.float32(32)
    v = np.zeros(8, np.float32)
    for r in rows:
        v = v + (r - m) * (r - m)
    assert np.array_equal(m, b["mean"]) and np.array_equal(v / np.float32(32), b["var"])


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    import h3d_amd
    from h3d_amd import _lib, bn
    assert "bn" in h3d_amd.__all__
    for name in ("h3d_batch_norm_workspace_bytes", "h3d_batch_norm_plan", "h3d_batch_norm_forward", "h3d_batch_norm_backward"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "h3d.h")).read()
    assert "#define H3D_ABI_VERSION 4" in hdr and "h3d_batch_norm_forward(" in hdr and "h3d_batch_norm_backward(" in hdr
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        bn.batch_norm_autograd(torch.zeros(1, 4, 2, 2), torch.ones(4), torch.zeros(4), torch.zeros(4), torch.ones(4), True)


def fwd(x=256, x_cs=8, gamma=256, beta=256, res=0, res_cs=8, y=256, y_cs=8, mean=256, var=256, invstd=256, rm=256, rv=256, B=1, C=8, H=2, W=2,
        training=1, relu=0, momentum=0.1, eps=1e-5, ws=256, ws_bytes=1 << 20):
    """h3d_batch_norm_forward on made-up addresses: only calls that fail a check (before the first HIP call) are made."""
    from h3d_amd import _lib
    p = ctypes.c_void_p
    return _lib.lib().h3d_batch_norm_forward(p(x), x_cs, p(gamma), p(beta), p(res), res_cs, p(y), y_cs, p(mean), p(var), p(invstd), p(rm), p(rv),
                                             B, C, H, W, training, relu, momentum, eps, p(ws), ws_bytes, p(0))


def bwd(x=256, x_cs=8, y=256, y_cs=8, gy=256, gy_cs=8, gamma=256, mean=256, invstd=256, gx=256, gx_cs=8, gr=256, gr_cs=8, gg=256, gb=256, B=1,
        C=8, H=2, W=2, training=1, relu=1, ws=256, ws_bytes=1 << 20):
    from h3d_amd import _lib
    p = ctypes.c_void_p
    return _lib.lib().h3d_batch_norm_backward(p(x), x_cs, p(y), y_cs, p(gy), gy_cs, p(gamma), p(mean), p(invstd), p(gx), gx_cs, p(gr), gr_cs,
                                              p(gg), p(gb), B, C, H, W, training, relu, p(ws), ws_bytes, p(0))


SHAPE_ERR, ARG_ERR = -1, -5


@pytest.mark.parametrize("call,kw,code,word", [
    (fwd, dict(C=6), SHAPE_ERR, "multiple of 4"), (fwd, dict(B=0), SHAPE_ERR, "non-positive"), (fwd, dict(x_cs=4), SHAPE_ERR, "x channel stride"),
    (fwd, dict(y_cs=10), SHAPE_ERR, "y channel stride"), (fwd, dict(res=256, res_cs=6), SHAPE_ERR, "res channel stride"),
    (fwd, dict(H=1, W=1), SHAPE_ERR, "more than 1 value per channel"), (fwd, dict(B=1 << 15, H=1 << 10, W=1 << 10), SHAPE_ERR, "pixels"),
    (fwd, dict(x=0), ARG_ERR, "null"), (fwd, dict(gamma=0), ARG_ERR, "null"), (fwd, dict(training=0, mean=0), ARG_ERR, "null"),
    (fwd, dict(y=260), ARG_ERR, "16-byte"), (fwd, dict(rm=264), ARG_ERR, "16-byte"), (fwd, dict(eps=-1.0), ARG_ERR, "eps"),
    (fwd, dict(momentum=1.5), ARG_ERR, "momentum"),
    (fwd, dict(H=300, W=300, ws=0), ARG_ERR, "workspace"), (fwd, dict(H=300, W=300, ws_bytes=16), ARG_ERR, "workspace"),
    (fwd, dict(H=300, W=300, ws=384), ARG_ERR, "workspace"),
    (bwd, dict(C=10), SHAPE_ERR, "multiple of 4"), (bwd, dict(W=-1), SHAPE_ERR, "non-positive"), (bwd, dict(gy_cs=4), SHAPE_ERR, "grad_y channel stride"),
    (bwd, dict(gx_cs=9), SHAPE_ERR, "grad_x channel stride"), (bwd, dict(gr_cs=4), SHAPE_ERR, "grad_res channel stride"),
    (bwd, dict(y_cs=4), SHAPE_ERR, "y channel stride"), (bwd, dict(gy=0), ARG_ERR, "null"), (bwd, dict(y=0), ARG_ERR, "null"),
    (bwd, dict(gamma=0), ARG_ERR, "null"), (bwd, dict(invstd=0), ARG_ERR, "null"), (bwd, dict(gb=258), ARG_ERR, "16-byte"),
    (bwd, dict(ws=0), ARG_ERR, "workspace"), (bwd, dict(ws_bytes=100), ARG_ERR, "workspace"), (bwd, dict(ws=272), ARG_ERR, "workspace"),
])
def test_argument_checks_run_before_any_hip_call(call, kw, code, word):
    from h3d_amd import _lib
    assert call(**kw) == code
    assert word in _lib.lib().h3d_last_error().decode()


def test_nothing_requested_is_ok_and_the_plan_is_reported():
    from h3d_amd import _lib, bn
    assert bwd(gx=0, gr=0, gg=0, gb=0, ws=0) == 0
    assert fwd(training=0, y=0, invstd=0) == 0
    assert bn.plan(8, 512, 16, 16) == (2048, 1)                      # level 5 at 512^2, B = 8: one launch
    chunk, slots = bn.plan(8, 16, 512, 512)                           # level 0: many workgroups per channel, then a second stage
    assert slots > 64 and slots == -(-8 * 512 * 512 // chunk) and slots <= 4096 and chunk % 64 == 0
    n = ctypes.c_size_t(0)
    assert _lib.lib().h3d_batch_norm_workspace_bytes(8, 16, 512, 512, ctypes.byref(n)) == 0 and n.value >= 2 * slots * 16 * 4 + 2 * 16 * 4
    assert _lib.lib().h3d_batch_norm_workspace_bytes(8, 18, 512, 512, ctypes.byref(n)) == SHAPE_ERR


# ---- TrainableDLASeg(bn=...) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_dcn", [True, False], ids=["dcn", "plain"])
def test_batch_mode_holds_the_references_own_keys(use_dcn):
    from h3d_amd.train_model import TrainableDLASeg
    net = N.make_model(use_dcn)
    tm = TrainableDLASeg(net, bn="batch")
    ref = N.state_dict(use_dcn)
    used = {k for k in ref if not k.startswith(N.UNUSED)}
    stats = ("running_mean", "running_var", "num_batches_tracked")
    heads = {"%s.%s" % (h, l) for h in N.HEADS for l in ("0.weight", "0.bias", "2.weight", "2.bias")}
    params = {n[len("ref."):].replace("__", ".") if n.startswith("ref.") else n for n, _ in tm.named_parameters()}
    buffers = {n.replace("__", ".") for n, _ in tm.named_buffers()}
    assert params == {k for k in used if k.rsplit(".", 1)[1] not in stats}
    assert heads <= params
    assert buffers == {k for k in used if k.rsplit(".", 1)[1] in stats}
    assert set(tm.state_dict()) == set(ref) == set(tm.export_state_dict())
    assert not any(k.startswith("trainable_folded.") for k in tm.state_dict())
    assert all(torch.equal(v.cpu(), ref[k]) for k, v in tm.state_dict().items())
    assert tm.training


def test_batch_mode_export_and_load_round_trip():
    from h3d_amd.train_model import TrainableDLASeg
    tm = TrainableDLASeg(N.make_model(False), bn="batch")
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in tm.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        for n, b in tm.named_buffers():
            b.add_(3) if n.endswith("num_batches_tracked") else b.mul_(1.25)
    sd = tm.state_dict()
    other = TrainableDLASeg(N.make_model(False), bn="batch")
    assert not torch.equal(other.state_dict()["base.level2.tree1.bn1.running_var"], sd["base.level2.tree1.bn1.running_var"])
    other.load_state_dict(sd)
    back = other.state_dict()
    assert set(back) == set(sd) and all(torch.equal(back[k], v) for k, v in sd.items())
    assert all(torch.equal(a, b) for a, b in zip(tm.parameters(), other.parameters()))
    assert int(back["base.level5.root.bn.num_batches_tracked"]) == 3
    # sync(): the wrapped model holds the export
    net = other.sync()
    assert all(torch.equal(net.state_dict()[k], v) for k, v in sd.items())


def test_frozen_mode_has_the_parents_keys():
    from h3d_amd.train_model import FOLDED_PREFIX, TrainableDLASeg
    net = N.make_model(True)
    a, b = TrainableDLASeg(net), TrainableDLASeg(net, bn="frozen")
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()] and not list(a.named_buffers())
    assert all(n.startswith("folded.") or n.split(".")[0] in N.HEADS for n, _ in a.named_parameters())
    ref = set(N.state_dict(True))
    assert {k for k in a.state_dict() if not k.startswith(FOLDED_PREFIX)} == ref and list(a.state_dict()) == list(b.state_dict())
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    with pytest.raises(ValueError):
        TrainableDLASeg(net, bn="sync")
