"""TEST INFRASTRUCTURE: the yardstick of h3d_amd.train_model.TrainableDLASeg -- oracle.dla.DLAOracle (imported, not edited) under torch
autograd on the CPU, in float64 and float32.

The trainable object's parameters are the FOLDED filters and biases, the oracle reads the reference's keys.  The leaves here are the
object's own parameters (cast to the run's dtype); the oracle's state_dict is built from them with differentiable torch ops -- the fold
undone (conv.weight = W' / scale, BatchNorm bias = b' - (conv.bias - running_mean) * scale) -- so autograd carries every gradient through
the fold's chain rule and folded and reference-keyed parameters compare like for like.  oracle.dcn.dcn_module_forward is written in
differentiable torch ops (floor, gather, where), so the DCN variant needs no other composition."""
import functools

import numpy as np
import torch

import losses_ref as LR
from oracle.dla import BN_EPS, DLAOracle

HEADS = {"hm": 1, "wh": 2, "hps": 34}
HC = 64                     # the head_conv of the trainer tests (tests/test_gpu_optim.py)
RES = 64                    # the smallest input DLA-34 admits (level5 is 2 x 2)
CONFIGS = [(use_dcn, B) for use_dcn in (True, False) for B in (1, 2)]


def state_dict(use_dcn):
    from h3d_amd import arch, synth
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, use_dcn, HC), seed=0)
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def make_model(use_dcn, device="cpu"):
    from h3d_amd import model
    net = model.dla_net(HEADS, head_conv=HC, not_use_dcn=not use_dcn, dtype="f32")
    net.load_state_dict(state_dict(use_dcn))
    return net.to(device)


def images(B):
    from h3d_amd import synth
    return torch.from_numpy(synth.synth_images(B, RES, RES))


def functional(B):
    """The fixed random linear functional of the heads: {head: coefficients [B,C,16,16]}."""
    g = torch.Generator().manual_seed(77)
    return {h: torch.randn(B, c, RES // 4, RES // 4, generator=g) for h, c in HEADS.items()}


def conv_of_bn(bn):
    """The convolution in front of a BatchNorm of the reference's DLASeg (models/model.py), by state_dict prefix."""
    head, leaf = bn.rsplit(".", 1)
    if leaf in ("bn1", "bn2"):
        return head + ".conv" + leaf[2]
    if leaf == "bn":
        return head + ".conv"
    if leaf == "1":
        return head + ".0"
    assert leaf == "0" and head.endswith(".actf"), bn
    return head[:-5] + ".conv"


UNUSED = ("base.level3.project.", "base.level4.project.")       # a two-level Tree computes its own `project` and never uses it (model.py:212)


def leaves_of(tm, dtype):
    """The trainable object's parameters as CPU leaves of `dtype`, keyed like TrainableDLASeg.state_dict's folded entries / the heads'
    reference keys."""
    out = {}
    for name, p in tm.folded.items():
        out[name.replace("__", ".")] = p.detach().cpu().to(dtype).clone().requires_grad_(True)
    for h, ps in tm.head_params().items():
        for leaf, p in zip(("0.weight", "0.bias", "2.weight", "2.bias"), ps):
            out["%s.%s" % (h, leaf)] = p.detach().cpu().to(dtype).clone().requires_grad_(True)
    return out


def oracle_state(leaves, base, dtype):
    """The reference-keyed state_dict the oracle reads, as differentiable functions of the leaves; `base`: the model's original tensors
    (BatchNorm statistics and weights, the DeformConvs' stored conv.bias, the unused `project`s)."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in base.items()}
    for k in [k for k in base if k.endswith(".running_mean") and not k.startswith(UNUSED)]:
        bn = k[:-len(".running_mean")]
        conv = conv_of_bn(bn)
        s = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + BN_EPS)
        b0 = sd[conv + ".bias"] if conv + ".bias" in base else torch.zeros_like(s)
        sd[conv + ".weight"] = leaves[conv + ".weight"] / s.view(-1, 1, 1, 1)
        sd[bn + ".bias"] = leaves[conv + ".bias"] - (b0 - sd[bn + ".running_mean"]) * s
    for k in leaves:
        if ".conv_offset_mask." in k or ".up_" in k or k.split(".")[0] in HEADS:
            sd[k] = leaves[k]
    return sd


def oracle_forward(leaves, base, x, use_dcn, dtype):
    net = DLAOracle(oracle_state(leaves, base, dtype), HEADS, use_dcn)
    return net(x.to(dtype))[0]


def run_functional(tm, base, x, coef, use_dcn, dtype):
    """-> ({head: output}, {leaf: gradient}) of sum_h <coef_h, head_h> on the CPU in `dtype`."""
    leaves = leaves_of(tm, dtype)
    out = oracle_forward(leaves, base, x, use_dcn, dtype)
    loss = sum((out[h] * coef[h].to(dtype)).sum() for h in HEADS)
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return {h: out[h].detach() for h in HEADS}, dict(zip(leaves, grads))


def multi_pose_loss(out, batch):
    """loss_multi_pose (trainer.py:86-137) with reg_offset, reg_hp_offset and hm_hp off: the three heads of HEADS."""
    w = LR.WEIGHTS
    return (w["hm_weight"] * LR.focal_logits(out["hm"], batch["hm"])
            + w["hp_weight"] * LR.reg("RegWeightedL1Loss", out["hps"], batch["hps_mask"], batch["ind"], batch["hps"])
            + w["wh_weight"] * LR.reg("RegL1Loss", out["wh"], batch["reg_mask"], batch["ind"], batch["wh"]))


def adam_losses(tm, base, batch, use_dcn, lr, steps, dtype):
    """`steps` Adam steps (torch.optim.Adam on the folded leaves) through the oracle's autograd -> the loss before each step."""
    leaves = leaves_of(tm, dtype)
    opt = torch.optim.Adam(list(leaves.values()), lr=lr)
    gold = LR.cast({k: v.detach().cpu() for k, v in batch.items() if torch.is_tensor(v)}, dtype)
    vals = []
    for _ in range(steps):
        opt.zero_grad()
        loss = multi_pose_loss(oracle_forward(leaves, base, gold["input"], use_dcn, dtype), gold)
        vals.append(float(loss.detach()))
        loss.backward()
        opt.step()
    return vals


def l2(t):
    return float(t.detach().double().norm())


def check_l2(what, got, g64, g32):
    """The rule per tensor: ||g - g64|| <= 4 ||g32 - g64|| + 1e-6 ||g64|| (L2: single ReLU gates legitimately flip between arithmetics).
    -> err / e32."""
    err, e32, n = l2(got.detach().cpu().double() - g64), l2(g32.double() - g64), l2(g64)
    assert err <= 4 * e32 + 1e-6 * n, "%s: err %.3g e32 %.3g |g64| %.3g" % (what, err, e32, n)
    return err / e32 if e32 else 0.0


def check_max(what, got, r64, r32):
    """Forward rule per tensor: max |y - y64| <= 4 e32 + 1e-7 max |y64|."""
    err = float((got.detach().cpu().double() - r64).abs().max())
    e32 = float((r32.double() - r64).abs().max())
    assert err <= 4 * e32 + 1e-7 * float(r64.abs().max()), "%s: err %.3g e32 %.3g max %.3g" % (what, err, e32, float(r64.abs().max()))
    return err / e32 if e32 else 0.0


@functools.lru_cache(maxsize=None)
def functional_runs(use_dcn, B):
    """The CPU half, computed once per configuration: (outputs64, grads64, outputs32, grads32)."""
    from h3d_amd.train_model import TrainableDLASeg
    net = make_model(use_dcn)
    tm = TrainableDLASeg(net)
    base = {k: v.detach().clone() for k, v in net.state_dict().items()}
    o64, g64 = run_functional(tm, base, images(B), functional(B), use_dcn, torch.float64)
    o32, g32 = run_functional(tm, base, images(B), functional(B), use_dcn, torch.float32)
    return o64, g64, o32, g32
