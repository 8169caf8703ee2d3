"""TEST INFRASTRUCTURE: the yardstick of TrainableDLASeg(bn="batch") -- oracle.dla.DLAOracle (imported, not edited) under torch autograd on
the CPU.  Evaluation mode is DLAOracle itself; training mode is the subclass below, whose BatchNorms use the batch's statistics.  The leaves
are the trainable object's own parameters under the reference's keys (nothing is folded), so the oracle's state_dict is the model's
tensors with the leaves put in.  Model, images, functional and the rules come from tests/network_grad_ref.py."""
import functools

import torch
import torch.nn.functional as F

import losses_ref as LR
import network_grad_ref as N
from oracle.dla import BN_EPS, DLAOracle

STATS = ("running_mean", "running_var", "num_batches_tracked")


class TrainOracle(DLAOracle):
    """DLAOracle in train(): every BatchNorm normalises with the batch's own mean and biased variance, differentiated through."""

    def _bn(self, x, key):
        sd = self.sd
        return F.batch_norm(x, None, None, sd[key + ".weight"], sd[key + ".bias"], True, 0.0, BN_EPS)


def images(B, res):
    from h3d_amd import synth
    return torch.from_numpy(synth.synth_images(B, res, res))


def functional(B, res):
    g = torch.Generator().manual_seed(78)
    return {h: torch.randn(B, c, res // 4, res // 4, generator=g) for h, c in N.HEADS.items()}


def ref_params(tm):
    """{reference key: parameter} of a TrainableDLASeg(bn="batch")."""
    out = {n.replace("__", "."): p for n, p in tm.ref.items()}
    for h, ps in tm.head_params().items():
        for leaf, p in zip(("0.weight", "0.bias", "2.weight", "2.bias"), ps):
            out["%s.%s" % (h, leaf)] = p
    return out


def leaves_of(tm, dtype):
    return {k: p.detach().cpu().to(dtype).clone().requires_grad_(True) for k, p in ref_params(tm).items()}


def oracle_state(leaves, base, dtype):
    sd = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in base.items()}
    sd.update(leaves)
    return sd


def oracle_forward(leaves, base, x, use_dcn, dtype, training):
    net = (TrainOracle if training else DLAOracle)(oracle_state(leaves, base, dtype), N.HEADS, use_dcn)
    return net(x.to(dtype))[0]


def run_functional(tm, base, x, coef, use_dcn, dtype, training):
    """-> ({head: output}, {reference key: gradient}) of sum_h <coef_h, head_h> on the CPU in `dtype`."""
    leaves = leaves_of(tm, dtype)
    out = oracle_forward(leaves, base, x, use_dcn, dtype, training)
    loss = sum((out[h] * coef[h].to(dtype)).sum() for h in N.HEADS)
    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return {h: out[h].detach() for h in N.HEADS}, {k: g for k, g in zip(leaves, grads) if g is not None}


def fresh(use_dcn):
    from h3d_amd.train_model import TrainableDLASeg
    net = N.make_model(use_dcn)
    return TrainableDLASeg(net, bn="batch"), {k: v.detach().clone() for k, v in net.state_dict().items()}


@functools.lru_cache(maxsize=None)
def eval_runs(use_dcn, B):
    """Evaluation mode at 64^2: (outputs64, grads64, outputs32, grads32)."""
    tm, base = fresh(use_dcn)
    o64, g64 = run_functional(tm, base, N.images(B), N.functional(B), use_dcn, torch.float64, False)
    o32, g32 = run_functional(tm, base, N.images(B), N.functional(B), use_dcn, torch.float32, False)
    return o64, g64, o32, g32


@functools.lru_cache(maxsize=None)
def train_run64(use_dcn, B, res):
    """Training mode in float64: (outputs64, grads64)."""
    tm, base = fresh(use_dcn)
    return run_functional(tm, base, images(B, res), functional(B, res), use_dcn, torch.float64, True)


def adam_losses64(tm, base, batch, use_dcn, lr, steps):
    """`steps` Adam steps (torch.optim.Adam on the reference-keyed leaves) through the training-mode oracle in float64 -> the loss before
    each step and after the last."""
    leaves = leaves_of(tm, torch.float64)
    opt = torch.optim.Adam(list(leaves.values()), lr=lr)
    gold = LR.cast({k: v.detach().cpu() for k, v in batch.items() if torch.is_tensor(v)}, torch.float64)
    vals = []
    for i in range(steps + 1):
        opt.zero_grad()
        loss = N.multi_pose_loss(oracle_forward(leaves, base, gold["input"], use_dcn, torch.float64, True), gold)
        vals.append(float(loss.detach()))
        if i < steps:
            loss.backward()
            opt.step()
    return vals
