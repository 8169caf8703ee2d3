"""GPU: TrainableDLASeg(bn="batch") and NetworkTrainer(bn="batch") -- the DLA-34 trained with batch statistics -- against the yardsticks of
tests/bn_network_ref.py (oracle.dla.DLAOracle under torch autograd) and tests/bn_ref.py (the operator, call by call).

A whole-network training-mode comparison "GPU vs float64 within 4 x (float32 CPU - float64)" is deliberately absent: four float32 CPU
evaluations of that graph differ from float64 by 2-6 % of a gradient's norm and among themselves by up to 1000 times such a bound, so a
right kernel would fail it.  Instead: evaluation mode checks the whole graph's wiring at the conditioning the frozen tests pass; training
mode is checked call by call against the operator's rule, its forward with the statistics taken out of the comparison, and its gradients
against a cap that a missing or mis-signed term breaks."""
import random
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import bn_network_ref as BR
import bn_ref as R
import network_grad_ref as N
import targets_ref
from gpu_helpers import DEV
from h3d_amd import train_input, trainer
from h3d_amd.train_model import TrainableDLASeg
from test_gpu_bn import no_vendor_batch_norm
from test_gpu_train_model import no_vendor_convolution

pytestmark = pytest.mark.gpu
IDS = ["%s_B%d" % ("dcn" if d else "plain", b) for d, b in N.CONFIGS]
DCN = pytest.mark.parametrize("use_dcn", [True, False], ids=["dcn", "plain"])


def test_the_feature_exists():
    """Fails on the parent: TrainableDLASeg takes no `bn` (TypeError) and h3d_amd.bn does not import (ImportError)."""
    import h3d_amd.bn  # noqa: F401
    tm = TrainableDLASeg(N.make_model(False, DEV), bn="batch")
    assert tm.bn == "batch" and tm.training and len(tm._bns) > 30


def gpu_grads(tm):
    return {k: p.grad for k, p in BR.ref_params(tm).items() if p.grad is not None}


def run_gpu(tm, x, coef):
    with no_vendor_convolution(), no_vendor_batch_norm():
        out = tm(x.to(DEV))[0]
        loss = sum((out[h] * coef[h].to(DEV)).sum() for h in N.HEADS)
        loss.backward()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("use_dcn,B", N.CONFIGS, ids=IDS)
def test_evaluation_mode_forward_and_every_gradient_vs_the_oracle(use_dcn, B):
    o64, g64, o32, g32 = BR.eval_runs(use_dcn, B)
    tm = TrainableDLASeg(N.make_model(use_dcn, DEV), bn="batch").eval()
    assert set(g64) == set(BR.ref_params(tm)) and all(N.l2(g) > 0 for g in g64.values())
    before = {k: v.clone() for k, v in tm.state_dict().items()}
    out = run_gpu(tm, N.images(B), N.functional(B))
    worst = max(N.check_max("head %s" % h, out[h], o64[h], o32[h]) for h in N.HEADS)
    got = gpu_grads(tm)
    assert set(got) == set(g64)
    ratios = {k: N.check_l2(k, got[k], g64[k], g32[k]) for k in g64}
    k = max(ratios, key=ratios.get)
    print("eval %s B %d: heads err / e32 <= %.2f; gradients err / e32 <= %.2f (%s)" % ("dcn" if use_dcn else "plain", B, worst, ratios[k], k))
    assert all(torch.equal(v, before[k]) for k, v in tm.state_dict().items())       # eval() moves no statistic and no counter


class Recorder:
    """Wraps bn.batch_norm_autograd (train_model calls it through the module): per call the inputs, the output, the saved statistics, the
    running statistics before and after, and -- by hooks -- grad_y and grad_x."""

    def __init__(self, tm):
        from h3d_amd import bn
        self.bn, self.orig, self.calls = bn, bn.batch_norm_autograd, []
        self.key_of = {id(p): k[:-len(".weight")] for k, p in BR.ref_params(tm).items()}

    def __enter__(self):
        self.bn.batch_norm_autograd = self
        return self

    def __exit__(self, *a):
        self.bn.batch_norm_autograd = self.orig

    def __call__(self, x, weight, bias, running_mean, running_var, training, momentum=0.1, eps=1e-5, res=None, relu=False):
        c = NS(key=self.key_of[id(weight)], x=x.detach().clone(), weight=weight, bias=bias, rm0=running_mean.clone(), rv0=running_var.clone(),
               training=training, momentum=momentum, eps=eps, res=None if res is None else res.detach().clone(), relu=relu, grad_y=None, grad_x=None)
        y = self.orig(x, weight, bias, running_mean, running_var, training, momentum, eps, res, relu)
        c.y, c.rm1, c.rv1 = y.detach().clone(), running_mean.clone(), running_var.clone()
        saved = y.grad_fn.saved_tensors
        c.save_mean, c.save_invstd = saved[3].clone(), saved[4].clone()
        # the biased variance is not kept for the backward: one more (deterministic) statistics call returns it
        _, m2, c.var, _ = self.bn.batch_norm_forward(x.detach(), weight.detach(), bias.detach(), training=True) if training else (None,) * 4
        assert not training or torch.equal(m2, c.save_mean)
        y.register_hook(lambda g, c=c: setattr(c, "grad_y", g.detach().clone()))
        x.register_hook(lambda g, c=c: setattr(c, "grad_x", g.detach().clone()))
        self.calls.append(c)
        return y


@pytest.fixture(scope="module", params=[True, False], ids=["dcn", "plain"])
def recorded(request):
    """One training-mode forward + backward at 64^2, B = 2, every BatchNorm call recorded."""
    use_dcn, B = request.param, 2
    net = N.make_model(use_dcn, DEV)
    tm = TrainableDLASeg(net, bn="batch")
    with Recorder(tm) as rec:
        out = run_gpu(tm, N.images(B), N.functional(B))
    return NS(use_dcn=use_dcn, B=B, net=net, tm=tm, calls=rec.calls, out={h: v.detach() for h, v in out.items()})


def test_training_mode_call_by_call(recorded):
    tm, calls = recorded.tm, recorded.calls
    assert sorted(c.key for c in calls) == sorted(tm._bns) and all(c.training for c in calls)
    params = BR.ref_params(tm)
    worst, n_min, v_min = {}, 1 << 30, 1e30
    for c in calls:
        cpu = lambda t: t.detach().cpu().numpy()
        x = cpu(c.x)
        assert c.grad_y is not None and c.grad_x is not None, c.key
        o = dict(gamma=cpu(c.weight), beta=cpu(c.bias), running_mean=cpu(c.rm0), running_var=cpu(c.rv0), grad_y=cpu(c.grad_y),
                 res=None if c.res is None else cpu(c.res))
        assert c.momentum == 0.1 and c.eps == 1e-5
        t64, t32 = R.yardsticks(x, o, c.res is not None, c.relu, True, mask=cpu(c.y) > 0)
        got = dict(y=c.y, mean=c.save_mean, var=c.var, running_mean=c.rm1, running_var=c.rv1, grad_x=c.grad_x,
                   grad_gamma=params[c.key + ".weight"].grad, grad_beta=params[c.key + ".bias"].grad)
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), R.check("%s %s" % (c.key, k), v, t64[k], t32[k]))
        inv = lambda v, f: f(1) / np.sqrt(v.astype(f) + f(c.eps))
        worst["invstd"] = max(worst.get("invstd", 0.0), R.check(c.key + " invstd", c.save_invstd, inv(t64["var"], np.float64), inv(t32["var"], np.float32)))
        n_min, v_min = min(n_min, x.size // x.shape[1]), min(v_min, float(t64["var"].min()))
        assert int(tm.state_dict()[c.key + ".num_batches_tracked"]) == 1
    print("%s: %d calls, smallest N %d, smallest variance %.3g; err / e32 <= %s" % ("dcn" if recorded.use_dcn else "plain", len(calls), n_min, v_min,
                                                                                   ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))))


def test_training_mode_forward_wiring(recorded):
    """The recorded batch statistics as running statistics of the unmodified evaluation-mode oracle bound the training-mode heads."""
    tm = recorded.tm
    base = {k: v.detach().cpu().clone() for k, v in recorded.net.state_dict().items()}
    for c in recorded.calls:
        base[c.key + ".running_mean"], base[c.key + ".running_var"] = c.save_mean.cpu().clone(), c.var.cpu().clone()
    x = N.images(recorded.B)
    with torch.no_grad():
        o64 = BR.oracle_forward(BR.leaves_of(tm, torch.float64), base, x, recorded.use_dcn, torch.float64, False)
        o32 = BR.oracle_forward(BR.leaves_of(tm, torch.float32), base, x, recorded.use_dcn, torch.float32, False)
    worst = max(N.check_max("head %s" % h, recorded.out[h], o64[h], o32[h]) for h in N.HEADS)
    print("%s: training-mode heads err / e32 <= %.2f" % ("dcn" if recorded.use_dcn else "plain", worst))


def test_sync_carries_the_moved_statistics(recorded):
    """After the training-mode forward moved the statistics: the inference engine (folded running statistics) and tm.eval() agree with the
    oracle on the exported state."""
    tm, net = recorded.tm, recorded.net
    moved = tm.state_dict()
    assert not torch.equal(moved["base.level2.tree1.bn1.running_mean"], N.state_dict(recorded.use_dcn)["base.level2.tree1.bn1.running_mean"].to(DEV))
    base = {k: v.detach().cpu().clone() for k, v in moved.items()}
    x = N.images(recorded.B)
    with torch.no_grad():
        o64 = BR.oracle_forward({}, base, x, recorded.use_dcn, torch.float64, False)
        o32 = BR.oracle_forward({}, base, x, recorded.use_dcn, torch.float32, False)
        assert tm.sync() is net
        theirs = net(x.to(DEV))[0]
        tm.eval()
        mine = tm(x.to(DEV))[0]
        tm.train()
    for h in N.HEADS:
        N.check_max("engine after sync, head %s" % h, theirs[h], o64[h], o32[h])
        N.check_max("tm.eval(), head %s" % h, mine[h], o64[h], o32[h])


@DCN
def test_training_mode_gradient_sanity(use_dcn):
    """A cap, not a precision claim: per parameter tensor ||g - g64|| <= 0.25 ||g64|| against the training-mode oracle in float64 at 128^2,
    B = 2 -- ten times the 0.023 that four float32 CPU evaluations reach there; a missing or mis-signed term costs O(1).  The conv biases
    in front of a BatchNorm have an analytically zero gradient: ||g|| <= 1e-4 ||g_beta|| of the same BatchNorm (7e-7 measured on the CPU)."""
    B, res = 2, 128
    o64, g64 = BR.train_run64(use_dcn, B, res)
    tm = TrainableDLASeg(N.make_model(use_dcn, DEV), bn="batch")
    run_gpu(tm, BR.images(B, res), BR.functional(B, res))
    got = gpu_grads(tm)
    assert set(got) == set(g64)
    zero = {k for k in got if k.endswith(".conv.bias")}
    assert len(zero) == 16 == sum(b.endswith(".actf.0") for b in tm._bns)          # every DeformConv of DLAUp and IDAUp
    worst = 0.0
    for k in sorted(set(got) - zero):
        err, n = N.l2(got[k].cpu().double() - g64[k]), N.l2(g64[k])
        assert n > 0 and err <= 0.25 * n, "%s: err %.3g |g64| %.3g" % (k, err, n)
        worst = max(worst, err / n)
    wz = 0.0
    for k in sorted(zero):
        gb = got[k[:-len(".conv.bias")] + ".actf.0.bias"]
        assert N.l2(got[k]) <= 1e-4 * N.l2(gb), "%s: |g| %.3g |g_beta| %.3g" % (k, N.l2(got[k]), N.l2(gb))
        wz = max(wz, N.l2(got[k]) / N.l2(gb))
    print("%s 128^2 B 2: worst relative L2 error %.3g; conv biases |g| / |g_beta| <= %.3g" % ("dcn" if use_dcn else "plain", worst, wz))


def test_the_frozen_path_is_unchanged():
    x, coef = N.images(2), N.functional(2)
    runs = []
    for kw in ({}, {"bn": "frozen"}):
        tm = TrainableDLASeg(N.make_model(False, DEV), **kw)
        out = run_gpu(tm, x, coef)
        runs.append((tm, out, [p.grad for p in tm.parameters()]))
    (a, oa, ga), (b, ob, gb) = runs
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()] and list(a.state_dict()) == list(b.state_dict())
    assert all(torch.equal(oa[h], ob[h]) for h in N.HEADS) and all(torch.equal(p, q) for p, q in zip(ga, gb)) and len(ga) > 100


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------
LR = 1e-3


def train_opt(lr=LR, **kw):
    return NS(task="multi_pose", lr=lr, lr_step=[2, 4], num_iters=-1, input_res=N.RES, output_res=N.RES // 4, not_rand_crop=False, aug_rot=0.0,
              rotate=0.0, flip=0.5, no_color_aug=False, reg_offset=False, reg_hp_offset=False, hm_hp=False, **kw)


@pytest.fixture(scope="module")
def batch():
    """tests/test_gpu_train_model.py's synthetic multi_pose batch, one image."""
    sizes = [(48, 64)]
    rs = np.random.RandomState(13)
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    scenes = [targets_ref.scene(20 + b, 1, M=2, img_w=w, img_h=h, min_size=24.0, max_size=40.0) for b, (h, w) in enumerate(sizes)]
    boxes, kps = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    np.random.seed(17), random.seed(17)
    b = train_input.multi_pose_train_batch([torch.from_numpy(i).to(DEV) for i in imgs], boxes, kps, [1], train_opt(), data_rng=np.random.RandomState(123))
    live = b["ind"][0][b["reg_mask"][0] > 0]
    assert live.numel() > 0 and int(torch.bincount(live).max()) <= 2
    return b


def test_three_steps_of_the_network_trainer(batch):
    use_dcn = True
    net = N.make_model(use_dcn, DEV)
    tr = trainer.NetworkTrainer(train_opt(), net, bn="batch")
    assert isinstance(tr.heads, TrainableDLASeg) and tr.heads.bn == "batch"
    assert trainer.NetworkTrainer(train_opt(bn="batch"), N.make_model(False, DEV)).heads.bn == "batch"
    assert trainer.NetworkTrainer(train_opt(), N.make_model(False, DEV)).heads.bn == "frozen"
    base = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    c64 = BR.adam_losses64(tr.heads, base, batch, use_dcn, LR, 3)
    vals = []
    with no_vendor_convolution(), no_vendor_batch_norm():
        for _ in range(3):
            vals.append(float(tr.train_step(dict(batch))[1].detach()))
        sd = tr.heads.state_dict()
        assert all(int(sd[b + ".num_batches_tracked"]) == 3 for b in tr.heads._bns)
        with torch.no_grad():
            last = float(tr.model_with_loss(dict(batch))[1])
    print("Adam lr %g, training-mode BatchNorm: cpu64 %s gpu %s, then %.9g" % (LR, ["%.9g" % v for v in c64], ["%.9g" % v for v in vals], last))
    assert np.isfinite(vals + [last]).all()
    assert (last < vals[0]) == (c64[3] < 0.9 * c64[0])


@DCN
def test_a_resumed_run_continues_from_the_checkpoints_bits(batch, tmp_path, use_dcn):
    tr = trainer.NetworkTrainer(train_opt(), N.make_model(use_dcn, DEV), bn="batch")
    for _ in range(2):
        tr.train_step(dict(batch))
    path = str(tmp_path / "model_last.pth")
    tr.save_model(path, 2)
    saved = {k: v.clone() for k, v in tr.heads.state_dict().items()}
    other = trainer.NetworkTrainer(train_opt(), N.make_model(use_dcn, DEV), bn="batch")
    with torch.no_grad():
        for p in other.heads.parameters():
            p.mul_(0.5)
    assert other.load_model(path, resume=True) == 2
    for g in other.optimizer.param_groups:
        g["lr"] = LR
    back = other.heads.state_dict()
    assert set(back) == set(saved) == set(N.state_dict(use_dcn)) and all(torch.equal(back[k], v) for k, v in saved.items())
    assert all(int(back[b + ".num_batches_tracked"]) == 2 for b in other.heads._bns)
    assert not torch.equal(back["base.level5.root.bn.running_var"], torch.ones_like(back["base.level5.root.bn.running_var"]))
    assert all(torch.equal(p, q) for p, q in zip(tr.heads.parameters(), other.heads.parameters()))
    for p, q in zip(tr.heads.parameters(), other.heads.parameters()):
        if p in tr.optimizer.state:
            assert all(torch.equal(tr.optimizer.state[p][k], other.optimizer.state[q][k]) for k in ("exp_avg", "exp_avg_sq"))
    tr.train_step(dict(batch))
    other.train_step(dict(batch))
    torch.cuda.synchronize()
    if not use_dcn:
        a, b = tr.heads.state_dict(), other.heads.state_dict()
        assert all(torch.equal(a[k], b[k]) for k in a)
