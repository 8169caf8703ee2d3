"""Host mirror of the reference's models/losses.py and of the task losses of trains/trainer.py:29-137 -- same class names,
constructor and `forward` arguments -- computed by libh3d_hip.so (csrc/loss.hip, include/h3d.h section 5).

    FocalLoss, RegL1Loss, RegLoss, NormRegL1Loss, RegWeightedL1Loss      (losses.py:114-175)
    loss_multi_pose(opt), loss_obj_detection(opt)                         (trainer.py:29-137): forward(outputs, batch) -> (loss, loss_stats)

Every call is ONE h3d_loss_forward (a partial-sum launch over all its terms + a finish launch, no host synchronisation) and, under
autograd, ONE h3d_loss_backward.  The task losses hand the head LOGITS to the kernel (H3D_LOSS_FROM_LOGITS): the clamped sigmoid the
reference computes first (`output['hm'] = _sigmoid(output['hm'])`, trainer.py:46,93,127) is a by-product of the same pass and is what
`output['hm']` is rebound to -- the tensor the caller passed in (a head buffer of the launch plan) is not written.
Gradients flow to the head maps (`pred` / `output`) only; `gt`, `mask`, `ind`, `target` get None."""
import ctypes

import torch

from . import _lib

FOCAL, REG_L1, REG_WEIGHTED_L1, NORM_REG_L1, REG_SL1 = 1, 2, 3, 4, 5      # H3D_LOSS_*
MASK_U8, MASK_F32 = 0, 1
FROM_LOGITS, TUNE_GRID8 = 1, 0x100
MAX_TERMS = 16


class H3dLossTerm(ctypes.Structure):
    """Mirror of `struct h3d_loss_term` in include/h3d.h."""
    _fields_ = [
        ("kind", ctypes.c_int32), ("flags", ctypes.c_int32),
        ("x", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("pred", ctypes.c_void_p), ("ind", ctypes.c_void_p),
        ("mask", ctypes.c_void_p), ("grad", ctypes.c_void_p),
        ("n", ctypes.c_int64),
        ("B", ctypes.c_int32), ("C", ctypes.c_int32), ("HW", ctypes.c_int32), ("M", ctypes.c_int32),
        ("mask_type", ctypes.c_int32), ("weight", ctypes.c_float),
    ]


def _head(t, what):
    """The tensor the gradient flows to: float32 on the GPU, made contiguous (a differentiable copy when it is not)."""
    if t.dtype != torch.float32:
        raise RuntimeError("%s: expected float32 tensors (reference uses .data<float>())" % what)
    _lib.require_cuda(t)
    return t.contiguous()


def _f32(t, dev):
    _lib.require_cuda(t)
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


class Term:
    """One h3d_loss_term and the tensors it points into.  `x` is the head tensor (logits / probabilities / feature map)."""

    def __init__(self, kind, x, gt, ind=None, mask=None, weight=1.0, flags=0, pred=None):
        self.kind, self.x, self.gt, self.ind, self.mask, self.weight, self.flags, self.pred = kind, x, gt, ind, mask, float(weight), flags, pred
        self.mask_type = MASK_F32 if (mask is not None and mask.dtype == torch.float32) else MASK_U8

    def fill(self, c, grad=None):
        c.kind, c.flags, c.weight, c.mask_type = self.kind, self.flags, self.weight, self.mask_type
        c.x, c.gt = self.x.data_ptr(), self.gt.data_ptr()
        c.pred = 0 if self.pred is None else self.pred.data_ptr()
        c.grad = 0 if grad is None else grad.data_ptr()
        if self.kind == FOCAL:
            c.n = self.x.numel()
        else:
            B, C, H, W = self.x.shape
            c.B, c.C, c.HW, c.M = B, C, H * W, self.ind.shape[1]
            c.ind, c.mask = self.ind.data_ptr(), self.mask.data_ptr()


def focal_term(x, gt, weight=1.0, from_logits=False, store_pred=True, flags=0, what="FocalLoss"):
    x = _head(x, what)
    gt = _f32(gt, x.device)
    if gt.numel() != x.numel():
        raise RuntimeError("%s: pred %s and gt %s differ in size" % (what, tuple(x.shape), tuple(gt.shape)))
    pred = torch.empty_like(x) if (from_logits and store_pred) else None
    return Term(FOCAL, x, gt, weight=weight, flags=flags | (FROM_LOGITS if from_logits else 0), pred=pred)


def reg_term(kind, output, mask, ind, target, weight=1.0, flags=0, what="RegL1Loss"):
    output = _head(output, what)
    if output.dim() != 4:
        raise RuntimeError("%s: output must be [B,C,H,W], got %s" % (what, tuple(output.shape)))
    B, C = output.shape[:2]
    _lib.require_cuda(ind, mask, target)
    ind = ind.detach().to(device=output.device, dtype=torch.int64).contiguous()
    if ind.dim() != 2 or ind.shape[0] != B:
        raise RuntimeError("%s: ind must be [B,M], got %s" % (what, tuple(ind.shape)))
    M = ind.shape[1]
    target = _f32(target, output.device)
    if tuple(target.shape) != (B, M, C):
        raise RuntimeError("%s: target %s does not match [B,M,C] = %s" % (what, tuple(target.shape), (B, M, C)))
    mask = mask.detach()
    if mask.dtype == torch.bool:
        mask = mask.contiguous().view(torch.uint8)
    elif mask.dtype not in (torch.uint8, torch.float32):
        mask = mask.float()                                   # the reference's `mask.float()`
    mask = mask.to(output.device).contiguous()
    want = (B, M, C) if kind == REG_WEIGHTED_L1 else (B, M)
    if tuple(mask.shape) != want:
        raise RuntimeError("%s: mask %s does not match %s" % (what, tuple(mask.shape), want))
    return Term(kind, output, target, ind=ind, mask=mask, weight=weight, flags=flags)


def _term_array(terms, grads=None):
    arr = (H3dLossTerm * max(len(terms), 1))()
    for i, t in enumerate(terms):
        t.fill(arr[i], None if grads is None else grads[i])
    return arr


def forward_terms(terms):
    """h3d_loss_forward over `terms`: stats [4 * n + 1] = per term {loss, aux0, aux1, aux2}, then the weighted total."""
    if len(terms) > MAX_TERMS:
        raise RuntimeError("losses: %d terms, at most %d per call" % (len(terms), MAX_TERMS))
    dev = terms[0].x.device if terms else torch.device("cuda")
    L = _lib.lib()
    arr = _term_array(terms)
    ws = _lib.workspace(L.h3d_loss_workspace_bytes, arr, len(terms), device=dev, min_bytes=16)
    stats = torch.empty(4 * len(terms) + 1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.h3d_loss_forward(arr, len(terms), _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "h3d_loss_forward")
    return stats


def backward_terms(terms, stats, coef, grads):
    """h3d_loss_backward: grads[i] (a tensor shaped like terms[i].x, or None = skip) receives coef[i] * d loss_i / d x_i."""
    L = _lib.lib()
    arr = _term_array(terms, grads)
    with torch.cuda.device(stats.device):
        _lib.check(L.h3d_loss_backward(arr, len(terms), _lib.ptr(stats), _lib.ptr(coef), _lib.stream_ptr()), "h3d_loss_backward")


class _FusedLossFn(torch.autograd.Function):
    """(terms, *heads) -> (losses [n], total []): the differentiable inputs are the terms' head tensors, in order."""

    @staticmethod
    def forward(ctx, terms, *heads):
        stats = forward_terms(terms)
        n = len(terms)
        ctx.terms, ctx.stats = terms, stats
        return stats[:4 * n].view(n, 4)[:, 0].clone(), stats[4 * n].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_losses, g_total):
        terms, stats = ctx.terms, ctx.stats
        # the upstream coefficient of every term, on the device: its own loss's grad + weight * the total's grad
        w = torch.tensor([t.weight for t in terms], dtype=torch.float32).to(stats.device, non_blocking=True)
        coef = (g_losses.float() + w * g_total.float()).contiguous()
        grads = [torch.empty_like(t.x) if ctx.needs_input_grad[i + 1] else None for i, t in enumerate(terms)]
        backward_terms(terms, stats, coef, grads)
        return (None,) + tuple(grads)


def fused(terms):
    """Run `terms` as one fused call: (per-term losses [n], weighted total [])."""
    return _FusedLossFn.apply(terms, *[t.x for t in terms])


def _single(term):
    return fused([term])[0][0]


class FocalLoss(torch.nn.Module):
    """nn.Module wrapper of `_neg_loss` (losses.py:42-67, 114-121): out = probabilities, target = gt."""

    def forward(self, out, target):
        return _single(focal_term(out, target))


class _RegBase(torch.nn.Module):
    KIND = None

    def forward(self, output, mask, ind, target):
        return _single(reg_term(self.KIND, output, mask, ind, target, what=type(self).__name__))


class RegLoss(_RegBase):
    """losses.py:123-137: smooth-L1 on the masked values, divided by the number of masked slots + 1e-4."""
    KIND = REG_SL1


class RegL1Loss(_RegBase):
    """losses.py:139-149."""
    KIND = REG_L1


class NormRegL1Loss(_RegBase):
    """losses.py:151-163."""
    KIND = NORM_REG_L1


class RegWeightedL1Loss(_RegBase):
    """losses.py:165-175: mask [B,M,C]."""
    KIND = REG_WEIGHTED_L1


def _opt(opt, name, default):
    return getattr(opt, name, default)


class _TaskLoss(torch.nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        # opts.py:121-129
        self.hm_weight, self.off_weight, self.wh_weight = _opt(opt, "hm_weight", 1), _opt(opt, "off_weight", 1), _opt(opt, "wh_weight", 0.1)
        self.hp_weight, self.hm_hp_weight = _opt(opt, "hp_weight", 1), _opt(opt, "hm_hp_weight", 1)
        self.mse_loss, self.reg_loss = _opt(opt, "mse_loss", False), _opt(opt, "reg_loss", "l1")
        if self.reg_loss not in ("l1", "sl1"):
            raise ValueError("reg_loss must be 'l1' or 'sl1' (opts.py:118)")
        self.reg_kind = REG_L1 if self.reg_loss == "l1" else REG_SL1

    @staticmethod
    def _finish(terms, names, extra, keys):
        """terms[i] adds to loss_stats[names[i]]; extra = [(name, weight, torch-computed loss)]; -> (loss, loss_stats)."""
        dev = terms[0].x.device
        stats = {k: torch.zeros((), dtype=torch.float32, device=dev) for k in keys}
        losses, total = fused(terms)
        for i, nm in enumerate(names):
            stats[nm] = stats[nm] + losses[i]
        for nm, w, v in extra:
            stats[nm] = stats[nm] + v
            total = total + w * v
        stats["loss"] = total
        return total, stats


class loss_multi_pose(_TaskLoss):
    """trainer.py:75-137."""
    KEYS = ("loss", "hm_loss", "hp_loss", "hm_hp_loss", "hp_offset_loss", "wh_loss", "off_loss")

    def forward(self, outputs, batch):
        opt = self.opt
        output = outputs[0]
        terms, names, extra = [], [], []
        t = focal_term(output["hm"], batch["hm"], self.hm_weight, from_logits=True, what="loss_multi_pose")
        output["hm"] = t.pred
        terms.append(t), names.append("hm_loss")
        if _opt(opt, "dense_hp", False):
            mask_weight = batch["dense_hps_mask"].sum() + 1e-4
            v = torch.nn.functional.l1_loss(output["hps"] * batch["dense_hps_mask"], batch["dense_hps"] * batch["dense_hps_mask"],
                                            reduction="sum") / mask_weight
            extra.append(("hp_loss", self.hp_weight, v))
        else:
            terms.append(reg_term(REG_WEIGHTED_L1, output["hps"], batch["hps_mask"], batch["ind"], batch["hps"], self.hp_weight))
            names.append("hp_loss")
        if self.wh_weight > 0:
            terms.append(reg_term(self.reg_kind, output["wh"], batch["reg_mask"], batch["ind"], batch["wh"], self.wh_weight))
            names.append("wh_loss")
        if _opt(opt, "reg_offset", True) and self.off_weight > 0:
            terms.append(reg_term(self.reg_kind, output["reg"], batch["reg_mask"], batch["ind"], batch["reg"], self.off_weight))
            names.append("off_loss")
        if _opt(opt, "reg_hp_offset", True) and self.off_weight > 0:
            terms.append(reg_term(self.reg_kind, output["hp_offset"], batch["hp_mask"], batch["hp_ind"], batch["hp_offset"], self.off_weight))
            names.append("hp_offset_loss")
        if _opt(opt, "hm_hp", True) and self.hm_hp_weight > 0:
            if self.mse_loss:
                extra.append(("hm_hp_loss", self.hm_hp_weight, torch.nn.functional.mse_loss(output["hm_hp"], batch["hm_hp"])))
            else:
                t = focal_term(output["hm_hp"], batch["hm_hp"], self.hm_hp_weight, from_logits=True, what="loss_multi_pose")
                output["hm_hp"] = t.pred
                terms.append(t), names.append("hm_hp_loss")
        return self._finish(terms, names, extra, self.KEYS)


class loss_obj_detection(_TaskLoss):
    """trainer.py:29-73."""
    KEYS = ("loss", "hm_loss", "wh_loss", "off_loss")

    def forward(self, outputs, batch):
        opt = self.opt
        terms, names, extra = [], [], []
        for s in range(_opt(opt, "num_stacks", 1)):
            output = outputs[s]
            if self.mse_loss:
                extra.append(("hm_loss", self.hm_weight, torch.nn.functional.mse_loss(output["hm"], batch["hm"])))
            else:
                t = focal_term(output["hm"], batch["hm"], self.hm_weight, from_logits=True, what="loss_obj_detection")
                output["hm"] = t.pred
                terms.append(t), names.append("hm_loss")
            if self.wh_weight > 0:
                if _opt(opt, "dense_wh", False):
                    mask_weight = batch["dense_wh_mask"].sum() + 1e-4
                    v = torch.nn.functional.l1_loss(output["wh"] * batch["dense_wh_mask"], batch["dense_wh"] * batch["dense_wh_mask"],
                                                    reduction="sum") / mask_weight
                    extra.append(("wh_loss", self.wh_weight, v))
                elif _opt(opt, "cat_spec_wh", False):
                    # crit_wh (trainer.py:35-37): NormRegL1Loss under norm_wh, else RegWeightedL1Loss; norm_wh alone falls through to
                    # crit_reg, as in the reference's forward (trainer.py:56-63)
                    kind = NORM_REG_L1 if _opt(opt, "norm_wh", False) else REG_WEIGHTED_L1
                    terms.append(reg_term(kind, output["wh"], batch["cat_spec_mask"], batch["ind"], batch["cat_spec_wh"], self.wh_weight,
                                          what="loss_obj_detection"))
                    names.append("wh_loss")
                else:
                    terms.append(reg_term(self.reg_kind, output["wh"], batch["reg_mask"], batch["ind"], batch["wh"], self.wh_weight))
                    names.append("wh_loss")
            if _opt(opt, "reg_offset", True) and self.off_weight > 0:
                terms.append(reg_term(self.reg_kind, output["reg"], batch["reg_mask"], batch["ind"], batch["reg"], self.off_weight))
                names.append("off_loss")
        if not terms:          # mse_loss with every regression weight at 0: nothing for the kernels
            dev = outputs[0]["hm"].device
            stats = {k: torch.zeros((), dtype=torch.float32, device=dev) for k in self.KEYS}
            total = stats["loss"]
            for nm, w, v in extra:
                stats[nm] = stats[nm] + v
                total = total + w * v
            stats["loss"] = total
            return total, stats
        return self._finish(terms, names, extra, self.KEYS)
