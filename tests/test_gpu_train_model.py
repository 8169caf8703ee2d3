"""GPU: the whole DLA-34 under autograd (h3d_amd/train_model.py TrainableDLASeg, trainer.NetworkTrainer) against the yardstick of
tests/network_grad_ref.py -- oracle.dla.DLAOracle under torch autograd on the CPU in float64 and float32.

Rules.  Head maps: max |y - y64| <= 4 e32 + 1e-7 max |y64|.  Gradients, per parameter tensor: ||g - g64|| <= 4 ||g32 - g64|| + 1e-6 ||g64||
(L2: single ReLU gates legitimately flip between arithmetics).  Loss values of the Adam run: the gradient rule applied to the numbers.
Model dla_net({'hm': 1, 'wh': 2, 'hps': 34}, head_conv = 64), synthetic weights, a 64 x 64 input, B = 1 and 2, with and without DCN."""
import contextlib
import random
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import network_grad_ref as N
import targets_ref
from gpu_helpers import DEV
from h3d_amd import optim, train_input, trainer
from h3d_amd.train_model import TrainableDLASeg

pytestmark = pytest.mark.gpu
IDS = ["%s_B%d" % ("dcn" if d else "plain", b) for d, b in N.CONFIGS]


@contextlib.contextmanager
def no_vendor_convolution():
    """torch's convolutions and pooling raise: whatever runs inside is this library's kernels (and torch's element-wise ops)."""
    def refuse(*a, **kw):
        raise AssertionError("a vendor convolution / pooling was called")
    saved = [(m, n, getattr(m, n)) for m, n in ((torch, "conv2d"), (F, "conv2d"), (torch, "conv_transpose2d"), (F, "conv_transpose2d"),
                                                (torch, "max_pool2d"), (F, "max_pool2d"), (torch, "convolution"), (torch, "_convolution"))]
    for m, n, _ in saved:
        setattr(m, n, refuse)
    try:
        yield
    finally:
        for m, n, f in saved:
            setattr(m, n, f)


def gpu_grads(tm):
    g = {n.replace("__", "."): p.grad for n, p in tm.folded.items()}
    for h, ps in tm.head_params().items():
        for leaf, p in zip(("0.weight", "0.bias", "2.weight", "2.bias"), ps):
            g["%s.%s" % (h, leaf)] = p.grad
    return g


@pytest.mark.parametrize("use_dcn,B", N.CONFIGS, ids=IDS)
def test_forward_and_every_gradient_vs_the_oracle(use_dcn, B):
    o64, g64, o32, g32 = N.functional_runs(use_dcn, B)
    assert all(N.l2(g) > 0 for g in g64.values())              # no tensor passes vacuously
    tm = TrainableDLASeg(N.make_model(use_dcn, DEV))
    assert set(g64) == {n.replace("__", ".") for n in tm.folded} | {"%s.%s" % (h, l) for h in N.HEADS for l in ("0.weight", "0.bias", "2.weight", "2.bias")}
    coef = N.functional(B)
    with no_vendor_convolution():
        out = tm(N.images(B).to(DEV))[0]
        loss = sum((out[h] * coef[h].to(DEV)).sum() for h in N.HEADS)
        loss.backward()
    torch.cuda.synchronize()
    worst = max(N.check_max("head %s" % h, out[h], o64[h], o32[h]) for h in N.HEADS)
    got = gpu_grads(tm)
    ratios = {k: N.check_l2(k, got[k], g64[k], g32[k]) for k in g64}
    k = max(ratios, key=ratios.get)
    print("%s B %d: heads err / e32 <= %.2f; gradients err / e32 <= %.2f (%s)" % ("dcn" if use_dcn else "plain", B, worst, ratios[k], k))


@pytest.mark.parametrize("use_dcn", [True, False], ids=["dcn", "plain"])
def test_export_into_a_fresh_model_reproduces_the_forward(use_dcn):
    """Untrained: the export carries the original tensors' forward.  After every parameter has moved: a fresh dla_net loaded with the
    export and the trainable object agree with the oracle evaluated at the moved parameters, each within the forward rule."""
    B = 2
    x = N.images(B).to(DEV)
    o64, _, o32, _ = N.functional_runs(use_dcn, B)
    net = N.make_model(use_dcn, DEV)
    tm = TrainableDLASeg(net)
    fresh = N.make_model(use_dcn, DEV)
    with torch.no_grad():
        for p in fresh.parameters():
            p.mul_(0.5)                                            # (so that only the load can make it right)
    fresh.load_state_dict(tm.export_state_dict())
    for h, y in fresh(x)[0].items():
        N.check_max("untrained export, head %s" % h, y, o64[h], o32[h])
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in tm.parameters():
            p.add_((0.02 * float(p.abs().max()) * torch.randn(p.shape, generator=g)).to(DEV))
    base = {k: v.detach().cpu().clone() for k, v in N.make_model(use_dcn).state_dict().items()}
    with torch.no_grad():
        m64 = N.oracle_forward(N.leaves_of(tm, torch.float64), base, N.images(B), use_dcn, torch.float64)
        m32 = N.oracle_forward(N.leaves_of(tm, torch.float32), base, N.images(B), use_dcn, torch.float32)
    assert max(float((m64[h] - o64[h]).abs().max()) for h in N.HEADS) > 1e-3          # the parameters did move the output
    fresh.load_state_dict(tm.export_state_dict())
    with no_vendor_convolution():
        mine = tm(x)[0]
    theirs = fresh(x)[0]
    for h in N.HEADS:
        N.check_max("trainable forward, head %s" % h, mine[h], m64[h], m32[h])
        N.check_max("export in a fresh model, head %s" % h, theirs[h], m64[h], m32[h])
    assert tm.sync() is net
    for h, y in net(x)[0].items():
        N.check_max("sync, head %s" % h, y, m64[h], m32[h])


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------------
LR = 1e-3


def train_opt(lr=LR):
    return NS(task="multi_pose", lr=lr, lr_step=[2, 4], num_iters=-1, input_res=N.RES, output_res=N.RES // 4, not_rand_crop=False, aug_rot=0.0,
              rotate=0.0, flip=0.5, no_color_aug=False, reg_offset=False, reg_hp_offset=False, hm_hp=False)


@pytest.fixture(scope="module")
def batch():
    """tests/test_gpu_optim.py's synthetic multi_pose batch, one image."""
    sizes = [(48, 64)]
    rs = np.random.RandomState(13)
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    scenes = [targets_ref.scene(20 + b, 1, M=2, img_w=w, img_h=h, min_size=24.0, max_size=40.0) for b, (h, w) in enumerate(sizes)]
    boxes, kps = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    np.random.seed(17), random.seed(17)
    b = train_input.multi_pose_train_batch([torch.from_numpy(i).to(DEV) for i in imgs], boxes, kps, [1], train_opt(), data_rng=np.random.RandomState(123))
    # the regression losses scatter their gradients with float atomic adds: up to two adds into a zeroed cell commute
    live = b["ind"][0][b["reg_mask"][0] > 0]
    assert live.numel() > 0 and int(torch.bincount(live).max()) <= 2
    return b


def param_bits(tr):
    return [p.detach().clone() for p in tr.heads.parameters()]


def test_five_steps_lower_the_loss_as_the_oracles_adam_run_does(batch):
    """NetworkTrainer.train_step five times on the DCN model against torch.optim.Adam on the same (folded) leaves through the oracle's
    autograd in float64 and float32; then sync(): model(images) is the trainable forward."""
    use_dcn = True
    net = N.make_model(use_dcn, DEV)
    tr = trainer.NetworkTrainer(train_opt(), net)
    assert isinstance(tr.heads, TrainableDLASeg) and isinstance(tr.optimizer, optim.Adam)
    assert len(list(tr.heads.parameters())) == len(tr.heads.folded) + 4 * len(N.HEADS)
    base = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    c64 = N.adam_losses(tr.heads, base, batch, use_dcn, LR, 5, torch.float64)
    c32 = N.adam_losses(tr.heads, base, batch, use_dcn, LR, 5, torch.float32)
    vals = []
    with no_vendor_convolution():
        for _ in range(5):
            out, loss, stats = tr.train_step(dict(batch))
            vals.append(float(loss.detach()))
        with torch.no_grad():
            last = float(tr.model_with_loss(dict(batch))[1])
    print("Adam lr %g: cpu64 %s cpu32 %s gpu %s, then %.9g" % (LR, ["%.9g" % v for v in c64], ["%.9g" % v for v in c32], ["%.9g" % v for v in vals], last))
    assert np.isfinite(vals).all() and last < vals[0] and c64[4] < c64[0]
    for i, (v, a, b) in enumerate(zip(vals, c64, c32)):
        assert abs(v - a) <= 4 * abs(b - a) + 1e-6 * abs(a), "step %d: gpu %.9g cpu64 %.9g cpu32 %.9g" % (i, v, a, b)
    assert all(float(tr.optimizer.state[p]["step"]) == 5.0 for p in tr.heads.parameters())
    # val()'s first act: the trained weights go back into the model
    x = batch["input"]
    with torch.no_grad():
        mine = tr.heads(x)[0]
        m64 = N.oracle_forward(N.leaves_of(tr.heads, torch.float64), base, x.cpu(), use_dcn, torch.float64)
        m32 = N.oracle_forward(N.leaves_of(tr.heads, torch.float32), base, x.cpu(), use_dcn, torch.float32)
    tr._before_val()
    theirs = net(x)[0]
    for h in N.HEADS:
        N.check_max("trained forward, head %s" % h, mine[h], m64[h], m32[h])
        N.check_max("model after sync, head %s" % h, theirs[h], m64[h], m32[h])


@pytest.mark.parametrize("use_dcn", [False, True], ids=["plain", "dcn"])
def test_a_resumed_run_continues_from_the_checkpoints_bits(batch, tmp_path, use_dcn):
    """save_model -> load_model(resume) into a fresh trainer: every parameter and the optimiser state come back bit for bit, and on the
    plain-conv model the next train_step has the bits of the uninterrupted run's.  (With DCN dcn_v2_backward scatters grad_input with
    float atomic adds, csrc/dcn_bwd.hip: two runs of the same step differ in their last bits, checkpoint or not; there the restored
    state is what is compared.)"""
    tr = trainer.NetworkTrainer(train_opt(), N.make_model(use_dcn, DEV))
    for _ in range(2):
        tr.train_step(dict(batch))
    path = str(tmp_path / "model_last.pth")
    tr.save_model(path, 2)
    saved = param_bits(tr)
    other = trainer.NetworkTrainer(train_opt(), N.make_model(use_dcn, DEV))
    with torch.no_grad():
        for p in other.heads.parameters():
            p.mul_(0.5)
    assert other.load_model(path, resume=True) == 2
    for g in other.optimizer.param_groups:
        g["lr"] = LR                                               # (the uninterrupted run never dropped it)
    assert all(torch.equal(a, b) for a, b in zip(param_bits(other), saved))
    for p, q in zip(tr.heads.parameters(), other.heads.parameters()):
        assert all(torch.equal(tr.optimizer.state[p][k], other.optimizer.state[q][k]) for k in ("exp_avg", "exp_avg_sq"))
    tr.train_step(dict(batch))
    other.train_step(dict(batch))
    torch.cuda.synchronize()
    assert all(float(other.optimizer.state[p]["step"]) == 3.0 for p in other.heads.parameters())
    if not use_dcn:
        assert all(torch.equal(a, b) for a, b in zip(param_bits(tr), param_bits(other)))
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer"} and set(N.state_dict(use_dcn)) <= set(ck["state_dict"])


def test_heads_trainer_is_unaffected(batch):
    """HeadsTrainer on the same model: the heads' parameters only, and one step has the same bits before and after a NetworkTrainer was
    built and run in the process."""
    def one_step():
        tr = trainer.HeadsTrainer(train_opt(), N.make_model(True, DEV))
        assert type(tr.heads).__name__ == "TrainableHeads" and len(list(tr.heads.parameters())) == 4 * len(N.HEADS)
        loss = float(tr.train_step(dict(batch))[1].detach())
        return loss, param_bits(tr)
    l0, p0 = one_step()
    nt = trainer.NetworkTrainer(train_opt(), N.make_model(True, DEV))
    nt.train_step(dict(batch))
    l1, p1 = one_step()
    assert l0 == l1 and all(torch.equal(a, b) for a, b in zip(p0, p1))
