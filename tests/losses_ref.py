"""TEST INFRASTRUCTURE ONLY -- the oracle of h3d_amd.losses: the formulas of the reference's models/losses.py and of the task losses of
trains/trainer.py:29-137 restated in differentiable torch ops, dtype-generic (fp64 for the value, fp32 for the yardstick of the
comparison); plus the input builders shared by tests/test_oracle_losses.py, tests/test_gpu_losses.py, tools/gen_losses_golden.py and
tools/time_losses.py.  tests/golden/losses_ref.npz pins these restatements to the reference's own classes."""
import numpy as np
import torch

EPS = 1e-4
CLAMP_LOGIT = 9.2102          # |logit| at which sigmoid meets the clamp: log((1 - 1e-4) / 1e-4)
REG_CLASSES = ("RegL1Loss", "RegWeightedL1Loss", "NormRegL1Loss", "RegLoss")


# ---- the formulas -----------------------------------------------------------------------------------------------------------------
def sigmoid_clamp(x):
    """models/utils.py:8-10."""
    return torch.clamp(torch.sigmoid(x), min=1e-4, max=1 - 1e-4)


def focal(pred, gt):
    """`_neg_loss` (losses.py:42-67): pred = probabilities."""
    pos, neg = gt.eq(1), gt.lt(1)
    zero = torch.zeros((), dtype=pred.dtype)
    pos_sum = torch.where(pos, torch.log(pred) * (1 - pred) ** 2, zero).sum()
    neg_sum = torch.where(neg, torch.log(1 - pred) * pred ** 2 * (1 - gt) ** 4, zero).sum()
    num_pos = pos.to(pred.dtype).sum()
    if float(num_pos) == 0:
        return -neg_sum
    return -(pos_sum + neg_sum) / num_pos


def focal_logits(x, gt):
    return focal(sigmoid_clamp(x), gt)


def gather(feat, ind):
    """`_transpose_and_gather_feat` (utils.py:23-27): feat [B,C,H,W], ind [B,M] -> [B,M,C]."""
    B, C = feat.shape[:2]
    return feat.reshape(B, C, -1).gather(2, ind[:, None, :].expand(B, C, ind.shape[1])).permute(0, 2, 1)


def reg(cls, feat, mask, ind, target):
    """The four gathered regression losses (losses.py:97-175) by class name."""
    pred = gather(feat, ind)
    m = mask.to(feat.dtype)
    num = m.sum()
    if cls != "RegWeightedL1Loss":
        m = m[:, :, None].expand_as(pred)
    if cls == "NormRegL1Loss":
        return (pred / (target + EPS) * m - m).abs().sum() / (m.sum() + EPS)
    d = (pred * m - target * m).abs()
    if cls == "RegLoss":
        return torch.where(d < 1, 0.5 * d * d, d - 0.5).sum() / (num + EPS)
    return d.sum() / (m.sum() + EPS)


WEIGHTS = {"hm_weight": 1.0, "off_weight": 1.0, "wh_weight": 0.1, "hp_weight": 1.0, "hm_hp_weight": 1.0}      # opts.py:121-129


def multi_pose(output, batch, reg_loss="l1", weights=WEIGHTS):
    """loss_multi_pose.forward (trainer.py:86-137), default options: output = head LOGITS; -> (loss, loss_stats)."""
    crit = "RegL1Loss" if reg_loss == "l1" else "RegLoss"
    w = weights
    st = {"hm_loss": focal_logits(output["hm"], batch["hm"]),
          "hp_loss": reg("RegWeightedL1Loss", output["hps"], batch["hps_mask"], batch["ind"], batch["hps"]),
          "wh_loss": reg(crit, output["wh"], batch["reg_mask"], batch["ind"], batch["wh"]),
          "off_loss": reg(crit, output["reg"], batch["reg_mask"], batch["ind"], batch["reg"]),
          "hp_offset_loss": reg(crit, output["hp_offset"], batch["hp_mask"], batch["hp_ind"], batch["hp_offset"]),
          "hm_hp_loss": focal_logits(output["hm_hp"], batch["hm_hp"])}
    st["loss"] = (w["hm_weight"] * st["hm_loss"] + w["wh_weight"] * st["wh_loss"] + w["off_weight"] * st["off_loss"]
                  + w["hp_weight"] * st["hp_loss"] + w["hm_hp_weight"] * st["hm_hp_loss"] + w["off_weight"] * st["hp_offset_loss"])
    return st["loss"], st


def ctdet(output, batch, reg_loss="l1", weights=WEIGHTS):
    """loss_obj_detection.forward (trainer.py:40-73), default options, one stack."""
    crit = "RegL1Loss" if reg_loss == "l1" else "RegLoss"
    w = weights
    st = {"hm_loss": focal_logits(output["hm"], batch["hm"]),
          "wh_loss": reg(crit, output["wh"], batch["reg_mask"], batch["ind"], batch["wh"]),
          "off_loss": reg(crit, output["reg"], batch["reg_mask"], batch["ind"], batch["reg"])}
    st["loss"] = w["hm_weight"] * st["hm_loss"] + w["wh_weight"] * st["wh_loss"] + w["off_weight"] * st["off_loss"]
    return st["loss"], st


def cast(d, dtype):
    """Floating tensors of a dict (or a tensor) to `dtype`; index and uint8 tensors stay."""
    if torch.is_tensor(d):
        return d.to(dtype) if d.is_floating_point() else d
    return {k: cast(v, dtype) for k, v in d.items()}


def value_and_grad(fn, head, dtype):
    """(value, d value / d head) of fn(head) with head cast to `dtype` on the CPU."""
    h = head.detach().cpu().to(dtype).clone().requires_grad_(True)
    v = fn(h)
    g, = torch.autograd.grad(v, h)
    return v.detach(), g


# ---- input builders ---------------------------------------------------------------------------------------------------------------
def focal_inputs(seed, shape, positives="some"):
    """(logits, gt) fp32: logits 3 randn with some at +-12 (past the clamp) and none within 1e-3 of +-CLAMP_LOGIT; gt = rand^4 with about
    1 in 500 exactly 1 and a few 1.5.  positives: 'some' | 'none' (the num_pos == 0 branch) | 'all'."""
    gen = torch.Generator().manual_seed(seed)
    x = 3 * torch.randn(shape, generator=gen)
    r = torch.rand(shape, generator=gen)
    x = torch.where(r < 0.01, torch.full_like(x, 12.0), x)
    x = torch.where(r > 0.99, torch.full_like(x, -12.0), x)
    near = (x.abs() - CLAMP_LOGIT).abs() < 1e-3
    x = torch.where(near, x * 0.5, x)
    gt = torch.rand(shape, generator=gen) ** 4
    r = torch.rand(shape, generator=gen)
    if positives == "some":
        gt = torch.where(r < 1 / 500, torch.ones_like(gt), gt)
    elif positives == "all":
        gt = torch.ones_like(gt)
    if positives != "all":
        gt = torch.where(r > 0.995, torch.full_like(gt, 1.5), gt)
        gt = torch.where(gt.eq(1) & torch.tensor(positives == "none"), torch.full_like(gt, 0.5), gt)
    return x, gt


def reg_inputs(seed, cls, B, C, M, H, W, mask_dtype=torch.uint8, zero_mask=False):
    """(feat [B,C,H,W], mask, ind [B,M], target [B,M,C]): ind holds 0 and HW-1, a duplicated pair with both masks set, and (M > 4) padding
    slots with ind 0 and mask 0 at the end; NormRegL1Loss targets have |t| >= 0.5."""
    gen = torch.Generator().manual_seed(seed)
    HW = H * W
    feat = torch.randn(B, C, H, W, generator=gen)
    ind = torch.randint(0, HW, (B, M), generator=gen)
    mshape = (B, M, C) if cls == "RegWeightedL1Loss" else (B, M)
    on = torch.rand(mshape, generator=gen) < 0.7
    ind[0, 0] = 0
    ind[-1, -1 if M <= 4 else M // 2] = HW - 1
    if M > 4:
        ind[:, 3] = ind[:, 2]
        on[:, 2:4] = True
        ind[:, M - M // 4:] = 0
        on[:, M - M // 4:] = False
    if zero_mask:
        on[:] = False
    if mask_dtype == torch.uint8:
        mask = on.to(torch.uint8)
    else:
        mask = on.float() * (0.25 + torch.rand(mshape, generator=gen))
    target = torch.randn(B, M, C, generator=gen)
    if cls == "NormRegL1Loss":
        target = torch.where(target < 0, target - 0.5, target + 0.5)
    return feat, mask, ind, target


def multi_pose_inputs(seed, B, H, W, M=32, J=17):
    """(output, batch) of the multi_pose task: head logits / maps and a synthetic batch with the keys loss_multi_pose reads."""
    hm, gt_hm = focal_inputs(seed, (B, 1, H, W))
    hm_hp, gt_hm_hp = focal_inputs(seed + 1, (B, J, H, W))
    hps, hps_mask, ind, t_hps = reg_inputs(seed + 2, "RegWeightedL1Loss", B, 2 * J, M, H, W, torch.float32)
    wh, reg_mask, _, t_wh = reg_inputs(seed + 3, "RegL1Loss", B, 2, M, H, W)
    off, _, _, t_off = reg_inputs(seed + 4, "RegL1Loss", B, 2, M, H, W)
    hpo, hp_mask, hp_ind, t_hpo = reg_inputs(seed + 5, "RegL1Loss", B, 2, M * J, H, W)
    output = {"hm": hm, "wh": wh, "hps": hps, "reg": off, "hm_hp": hm_hp, "hp_offset": hpo}
    batch = {"hm": gt_hm, "hm_hp": gt_hm_hp, "hps": t_hps, "hps_mask": hps_mask, "ind": ind, "wh": t_wh, "reg": t_off, "reg_mask": reg_mask,
             "hp_offset": t_hpo, "hp_mask": hp_mask, "hp_ind": hp_ind}
    return output, batch


def ctdet_inputs(seed, B, H, W, M=32, classes=3):
    hm, gt_hm = focal_inputs(seed, (B, classes, H, W))
    wh, reg_mask, ind, t_wh = reg_inputs(seed + 3, "RegL1Loss", B, 2, M, H, W)
    off, _, _, t_off = reg_inputs(seed + 4, "RegL1Loss", B, 2, M, H, W)
    return {"hm": hm, "wh": wh, "reg": off}, {"hm": gt_hm, "wh": t_wh, "reg": t_off, "reg_mask": reg_mask, "ind": ind}


# ---- the rules of the comparisons -------------------------------------------------------------------------------------------------
def rel(a, ref):
    a, ref = float(a), float(ref)
    return abs(a - ref) / abs(ref) if ref != 0 else abs(a)


def pooled_e32(values32, values64):
    """Scalar losses: the yardstick is the LARGEST relative error of the fp32 restatement over the seeds of a case (a single number's
    fp32 error is a matter of luck: 2e-8 .. 1e-5 relative across seeds)."""
    return max(rel(a, r) for a, r in zip(values32, values64))


def check_scalars(name, got, values64, e32, factor=4.0):
    """every seed: rel err <= factor * e32_pooled + 1e-7; returns the worst ratio err / e32_pooled."""
    worst, fails = 0.0, []
    for i, (g, r) in enumerate(zip(got, values64)):
        err = rel(g, r)
        worst = max(worst, err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf")))
        if not err <= factor * e32 + 1e-7:
            fails.append((i, err))
    print("%s: e32 pooled %.3g, worst ratio %.3g over %d seeds" % (name, e32, worst, len(got)))
    assert not fails, (name, e32, fails)
    return worst


def check_tensor(name, got, ref64, ref32, factor=4.0):
    """per-element tensors: max |g - g64| <= factor * e32 + 1e-7 * max |g64|, e32 = max |g32 - g64| (tests/test_gpu_dcn_backward.py)."""
    r = ref64.double()
    e = float((ref32.double() - r).abs().max())
    err = float((got.detach().cpu().double() - r).abs().max())
    limit = factor * e + 1e-7 * float(r.abs().max())
    print("%s: err %.3g e32 %.3g ratio %.3g limit %.3g max|g64| %.3g" % (name, err, e, err / e if e else 0.0, limit, float(r.abs().max())))
    assert err <= limit, (name, err, limit)
    return err / e if e else 0.0
