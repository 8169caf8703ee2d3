"""SMPL 3D supervision (csrc/smpl_sup.hip, include/h3d.h section 4e): the link between per-person SMPL labels
(axis-angle pose, betas, 3D joints) and the `pose` / `shape` head maps.  There is no SMPL code in the reference, so the definition is the
project's own; model x / y are the output map's x / y (y down), as the keypoint reprojection loss (smpl_loss.py) has them.

    smpl_targets(pose, shape, valid, num, reg_mask, rot, flipped, c, s, ...)   the labels moved with the augmentation (mirror, then the
                                                      in-plane rotation) -> smpl_rotmat, smpl_pose_w, smpl_shape, smpl_shape_w, smpl_joints, smpl_joints_w
    smpl_supervised_loss(pose_map, shape_map, ind, joints, labels, n)          -> (pose_loss, shape_loss, j3d_loss), differentiable at the two
                                                      maps and at joints (what smpl.lbs_from_heads(..., return_joints=True) returns)
    SmplSupervisedLoss(smpl_model, n)                 forward(output, batch): lbs_from_heads (only with the joint term) + the loss
    loss_multi_pose_smpl3d(opt, smpl_model, regressor)    losses.loss_multi_pose + the three terms (+ smpl_loss's keypoint term)

    pose_loss  = sum wp |R(theta) - R_lab|^2 / (9 sum wp + 1e-4)          R = Rodrigues, 24 joints, Frobenius
    shape_loss = sum ws |beta - beta_lab|^2 / (10 sum ws + 1e-4)
    j3d_loss   = sum wj |(J - root(J)) - (J_lab - root(J_lab))|^2 / (3 sum wj + 1e-4)      root = the mean of joints 1 and 2

One launch for the labels, two for the forward, two for the backward; nothing is synchronised with the host."""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib, losses, smpl, targets

MIRROR_PAIRS = ((1, 2), (4, 5), (7, 8), (10, 11), (13, 14), (16, 17), (18, 19), (20, 21), (22, 23))
MIRROR = list(range(smpl.NUM_JOINTS))          # the permutation pi: an involution
for _a, _b in MIRROR_PAIRS:
    MIRROR[_a], MIRROR[_b] = _b, _a
LABEL_NAMES = ("smpl_rotmat", "smpl_pose_w", "smpl_shape", "smpl_shape_w", "smpl_joints", "smpl_joints_w")
LOSS_KEYS = ("smpl_pose_loss", "smpl_shape_loss", "smpl_j3d_loss")


def _opt(opt, name, default):
    return getattr(opt, name, default)


def _np(x, dtype=None):
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype)


def label_specs(B, max_objs):
    """name -> shape of the six label tensors (all float32)."""
    N, J = max_objs, smpl.NUM_JOINTS
    return {"smpl_rotmat": (B, N, J, 9), "smpl_pose_w": (B, N, J), "smpl_shape": (B, N, smpl.NUM_BETAS), "smpl_shape_w": (B, N),
            "smpl_joints": (B, N, J, 3), "smpl_joints_w": (B, N, J)}


def rot2_from_params(c, s, rot, out_w=128, out_h=128):
    """[B,2,2] float64: per image the 2x2 linear part of targets.target_transforms(...)[b, 1] (trans_output_rot) divided by the square
    root of its determinant -- [[cos r, sin r], [-sin r, cos r]] with r = rot pi / 180 up to rounding -- and exactly the identity where
    rot[b] == 0.  None when no image is rotated.  A per-axis s [B,2] together with a rotation is refused."""
    if rot is None:
        return None
    rot = _np(rot, np.float64).reshape(-1)
    if not (rot != 0).any():
        return None
    B = rot.shape[0]
    if c is None or s is None:
        raise ValueError("smpl_targets: c and s (the crop the rotation was drawn for) are needed with rot != 0")
    s_np = _np(s)
    if s_np.ndim == 2 and s_np.shape[-1] == 2:
        raise ValueError("smpl_targets: a per-axis s [B,2] together with rot != 0 is not a similarity: refused")
    trans = targets.target_transforms(_np(c, np.float32).reshape(B, 2), s_np.reshape(B), rot, out_w, out_h).numpy()
    out = np.tile(np.eye(2), (B, 1, 1))
    for b in range(B):
        if rot[b] != 0:
            A = trans[b, 1].reshape(2, 3)[:, :2]
            out[b] = A / np.sqrt(A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0])
    return out


def smpl_targets_raw(pose, shape, joints, valid, pose_w, joints_w, num, reg_mask, flipped, rot2, max_objs, out=None):
    """One h3d_smpl_sup_labels call on device tensors: pose [B,M,72], shape [B,M,10], joints [B,M,24,3] or None, valid [B,M], pose_w /
    joints_w [B,M,24] or None (all f32), num [B] i32, reg_mask [B,max_objs] u8, flipped [B] i32 or None, rot2 [B,2,2] f64 or None.
    -> {name: tensor} of the six outputs (written into `out`'s tensors when given)."""
    _lib.require_cuda(pose, shape, joints, valid, pose_w, joints_w, num, reg_mask, flipped, rot2)
    B, M = pose.shape[:2]
    dev = pose.device
    o = {}
    for name, shp in label_specs(B, max_objs).items():
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shp, dtype=torch.float32, device=dev)
        else:
            _lib.require_cuda(t)
            if tuple(t.shape) != shp or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("smpl_targets: output %s must be contiguous float32 %s, got %s of %s" % (name, shp, tuple(t.shape), t.dtype))
        o[name] = t
    p = _lib.ptr
    with torch.cuda.device(dev):
        rc = _lib.lib().h3d_smpl_sup_labels(p(pose), p(shape), p(joints), p(valid), p(pose_w), p(joints_w), p(num), p(reg_mask), p(flipped), p(rot2),
                                            B, M, max_objs, *[p(o[nm]) for nm in LABEL_NAMES], _lib.stream_ptr())
    _lib.check(rc, "h3d_smpl_sup_labels")
    return o


def smpl_targets(pose, shape, valid, num, reg_mask, rot=None, flipped=None, c=None, s=None, joints=None, joint_weight=None, pose_weight=None,
                 smpl_model=None, opt=None, out=None):
    """The SMPL labels of a batch, moved with the augmentation multi_pose_targets applied to the 2D labels.  pose [B,M,72] axis-angle,
    shape [B,M,10], valid [B,M] (0 = no label; also the default weight), num [B], reg_mask [B,max_objs] (multi_pose_targets' output, on
    the device: an object dropped from the crop teaches nothing), rot [B] degrees / flipped [B] / c [B,2] / s [B] = draw_params' values.
    joints [B,M,24,3]: the 3D label joints; with None and an smpl_model they are smpl.lbs(..., kernel="auto_exact") of the untransformed
    labels (mesh_eval.GroundTruth3D.from_smpl's call); with neither the joint term gets weight 0.  joint_weight / pose_weight [B,M,24].
    opt: max_objs, output_res (or output_h / output_w).  -> the dict of the six tensors (LABEL_NAMES), float32 on reg_mask's device."""
    if not isinstance(reg_mask, torch.Tensor):
        raise TypeError("smpl_targets: reg_mask must be the tensor multi_pose_targets returned")
    _lib.require_cuda(reg_mask)
    dev = reg_mask.device
    max_objs = _opt(opt, "max_objs", 32)
    f32 = lambda x: targets._dev(x, torch.float32, dev)
    pose, shape, valid = f32(pose), f32(shape), f32(valid)
    if pose.dim() == 4:
        pose = pose.reshape(pose.shape[0], pose.shape[1], 72)
    if pose.dim() != 3 or pose.shape[2] != 72:
        raise RuntimeError("smpl_targets: pose must be [B,M,72], got %s" % (tuple(pose.shape),))
    B, M = pose.shape[:2]
    if tuple(shape.shape) != (B, M, smpl.NUM_BETAS) or tuple(valid.shape) != (B, M):
        raise RuntimeError("smpl_targets: shape must be [B,M,10] and valid [B,M] beside pose [B,M,72], got %s and %s" % (tuple(shape.shape), tuple(valid.shape)))
    if tuple(reg_mask.shape) != (B, max_objs):
        raise RuntimeError("smpl_targets: reg_mask must be [B,max_objs] = %s, got %s" % ((B, max_objs), tuple(reg_mask.shape)))
    reg_mask = reg_mask.detach()
    reg_mask = (reg_mask if reg_mask.dtype == torch.uint8 else (reg_mask != 0).to(torch.uint8)).contiguous()
    num = targets._dev(num, torch.int32, dev).reshape(B)
    res = _opt(opt, "output_res", None)
    H, W = (res, res) if res else (_opt(opt, "output_h", 128), _opt(opt, "output_w", 128))
    rot2 = rot2_from_params(c, s, rot, W, H)
    rot2 = None if rot2 is None else torch.from_numpy(np.ascontiguousarray(rot2, np.float64)).to(dev)
    flipped = None if flipped is None else targets._dev(_np(flipped).astype(np.int32), torch.int32, dev).reshape(B)
    if joints is None and smpl_model is not None:
        _, joints = smpl.lbs(smpl_model, shape.reshape(B * M, smpl.NUM_BETAS), pose.reshape(B * M, 72), return_joints=True, kernel="auto_exact")
    if joints is not None:
        joints = f32(joints).reshape(B, M, smpl.NUM_JOINTS, 3)
    elif joint_weight is not None:
        raise ValueError("smpl_targets: joint_weight without joints or an smpl_model")
    weights = []
    for nm, wt in (("pose_weight", pose_weight), ("joint_weight", joint_weight)):
        wt = None if wt is None else f32(wt)
        if wt is not None and tuple(wt.shape) != (B, M, smpl.NUM_JOINTS):
            raise RuntimeError("smpl_targets: %s must be [B,M,24], got %s" % (nm, tuple(wt.shape)))
        weights.append(wt)
    return smpl_targets_raw(pose, shape, joints, valid, weights[0], weights[1], num, reg_mask, flipped, rot2, max_objs, out=out)


class _Inputs:
    """The checked, contiguous operands of one loss call."""

    def __init__(self, pose_map, shape_map, ind, joints, labels, n):
        what = "smpl_supervised_loss"
        lab = [labels[nm] for nm in LABEL_NAMES]
        _lib.require_cuda(pose_map, shape_map, ind, joints, *lab)
        for nm, t in (("pose_map", pose_map), ("shape_map", shape_map), ("joints", joints)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                raise RuntimeError("%s: %s must be a contiguous float32 tensor" % (what, nm))
        if pose_map.dim() != 4 or pose_map.shape[1] != 72 or shape_map.dim() != 4 or shape_map.shape[1] != smpl.NUM_BETAS or \
                shape_map.shape[0] != pose_map.shape[0] or shape_map.shape[2:] != pose_map.shape[2:]:
            raise RuntimeError("%s: pose_map [B,72,H,W] and shape_map [B,10,H,W] expected, got %s and %s" % (what, tuple(pose_map.shape), tuple(shape_map.shape)))
        dev = pose_map.device
        B, HW = pose_map.shape[0], pose_map.shape[2] * pose_map.shape[3]
        ind = ind.detach().to(device=dev, dtype=torch.int64).contiguous()
        if ind.dim() != 2 or ind.shape[0] != B:
            raise RuntimeError("%s: ind must be [B,max_objs], got %s" % (what, tuple(ind.shape)))
        M = ind.shape[1]
        if n is None:
            n = joints.shape[0] // B if joints is not None else M
        if not 0 < n <= M:
            raise RuntimeError("%s: n = %d person slots per image, 0 < n <= max_objs = %d expected" % (what, n, M))
        if joints is not None and tuple(joints.shape) != (B * n, smpl.NUM_JOINTS, 3):
            raise RuntimeError("%s: joints must be [B n,24,3] = %s, got %s" % (what, (B * n, smpl.NUM_JOINTS, 3), tuple(joints.shape)))
        self.lab = []
        for (nm, shp), t in zip(label_specs(B, M).items(), lab):
            t = t.detach()
            if tuple(t.shape) != shp:
                raise RuntimeError("%s: labels[%r] must be %s, got %s" % (what, nm, shp, tuple(t.shape)))
            self.lab.append(t.to(device=dev, dtype=torch.float32).contiguous())
        if shape_map.device != dev or (joints is not None and joints.device != dev):
            raise RuntimeError("%s: pose_map, shape_map and joints must be on one device" % what)
        self.pose_map, self.shape_map, self.ind, self.joints = pose_map, shape_map, ind, joints
        self.B, self.M, self.n, self.HW, self.P, self.dev = B, M, n, HW, B * n, dev

    def ptrs(self):
        p = _lib.ptr
        return [p(self.pose_map), p(self.shape_map), p(self.ind), p(self.joints)] + [p(t) for t in self.lab] + [self.B, self.M, self.n, self.HW]


def supervised_loss_forward(pose_map, shape_map=None, ind=None, joints=None, labels=None, n=None):
    """h3d_smpl_sup_loss_forward: -> (stats [9] = {loss, l, num} of the pose, shape and joint terms, the checked inputs).  joints = None:
    no joint term (stats[6:9] = 0)."""
    a = pose_map if isinstance(pose_map, _Inputs) else _Inputs(pose_map, shape_map, ind, joints, labels, n)
    stats = torch.empty(9, dtype=torch.float32, device=a.dev)
    L = _lib.lib()
    ws = _lib.workspace(L.h3d_smpl_sup_loss_workspace_bytes, a.B, a.n, device=a.dev)
    with torch.cuda.device(a.dev):
        _lib.check(L.h3d_smpl_sup_loss_forward(*a.ptrs(), _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "h3d_smpl_sup_loss_forward")
    return stats, a


def supervised_loss_backward(a, stats, grad_out, want=(True, True, True), out=None):
    """h3d_smpl_sup_loss_backward for the inputs `a` of a forward: -> (grad_pose_map, grad_shape_map, grad_joints [P,24,3]), None where not
    wanted (grad_joints also without joints).  grad_out: float32 [3] on the device, the upstream of the three losses.  out = the three
    tensors to write into."""
    if out is None:
        gp = torch.empty_like(a.pose_map) if want[0] else None
        gs = torch.empty_like(a.shape_map) if want[1] else None
        gj = torch.empty(a.P, smpl.NUM_JOINTS, 3, dtype=torch.float32, device=a.dev) if (want[2] and a.joints is not None) else None
    else:
        gp, gs, gj = out
    grad_out = grad_out.detach().to(device=a.dev, dtype=torch.float32).reshape(3).contiguous()
    with torch.cuda.device(a.dev):
        _lib.check(_lib.lib().h3d_smpl_sup_loss_backward(*a.ptrs(), _lib.ptr(stats), _lib.ptr(grad_out), _lib.ptr(gp), _lib.ptr(gs), _lib.ptr(gj),
                                                         _lib.stream_ptr()), "h3d_smpl_sup_loss_backward")
    return gp, gs, gj


class _SupervisedLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, pose_map, shape_map, joints):
        stats, _ = supervised_loss_forward(a)
        ctx.a, ctx.stats = a, stats
        ctx.set_materialize_grads(False)
        return stats[0::3].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if grad_out is None:
            return None, None, None, None
        need = ctx.needs_input_grad
        gp, gs, gj = supervised_loss_backward(ctx.a, ctx.stats, grad_out, want=(need[1], need[2], need[3]))
        return None, gp, gs, gj


def smpl_supervised_loss(pose_map, shape_map, ind, joints, labels, n=None):
    """pose_map [B,72,H,W], shape_map [B,10,H,W] (contiguous fp32 on the GPU), ind [B,max_objs], joints [B n,24,3] or None (no joint
    term), labels = smpl_targets' dict, the first n slots of every image (default: joints' B n / B, else max_objs)
    -> (pose_loss, shape_loss, j3d_loss), scalars.  Differentiable at pose_map, shape_map and joints."""
    a = _Inputs(pose_map, shape_map, ind, joints, labels, n)
    out = _SupervisedLossFn.apply(a, a.pose_map, a.shape_map, a.joints)
    return out[0], out[1], out[2]


class SmplSupervisedLoss(torch.nn.Module):
    """forward(output, batch): the three losses of the heads' `pose` / `shape` maps at batch['ind'] against batch's six label tensors.
    use_joints: whether a joint weight is in use -- only then smpl.lbs_from_heads(..., exact=True) runs (smpl_model may be None without it);
    forward(..., joints=) takes the joints of a call the caller already made.  n = the person slots per image (default: all max_objs)."""

    def __init__(self, smpl_model=None, n=None, use_joints=True):
        super().__init__()
        if use_joints and smpl_model is None:
            raise ValueError("SmplSupervisedLoss: the joint term needs an smpl_model")
        self.smpl_model, self.n, self.use_joints = smpl_model, n, bool(use_joints)

    def forward(self, output, batch, joints=None):
        ind = batch["ind"]
        n = self.n or ind.shape[1]
        _lib.require_cuda(output["pose"], output["shape"], ind)
        ind = ind.detach().to(dtype=torch.int64).contiguous()
        if self.use_joints and joints is None:
            _, joints = smpl.lbs_from_heads(self.smpl_model, output["pose"], output["shape"], ind, n, return_joints=True, exact=True)
        return smpl_supervised_loss(output["pose"], output["shape"], ind, joints if self.use_joints else None, batch, n)


class loss_multi_pose_smpl3d(losses.loss_multi_pose):
    """losses.loss_multi_pose plus 'smpl_pose_loss', 'smpl_shape_loss' and 'smpl_j3d_loss', added to `loss` with the weights
    opt.smpl_pose_weight / smpl_shape_weight / smpl_j3d_weight (each default 0: reported, not trained on).  With a `regressor` and
    opt.smpl_kp_weight > 0 smpl_loss's 'smpl_kp_loss' is added as well, on the same lbs_from_heads call."""
    KEYS = losses.loss_multi_pose.KEYS + LOSS_KEYS

    def __init__(self, opt, smpl_model, regressor=None):
        super().__init__(opt)
        self.weights = tuple(float(_opt(opt, nm, 0.0)) for nm in ("smpl_pose_weight", "smpl_shape_weight", "smpl_j3d_weight"))
        self.smpl_model = smpl_model
        self.smpl_sup = SmplSupervisedLoss(smpl_model, use_joints=self.weights[2] > 0)
        self.smpl_kp_weight = float(_opt(opt, "smpl_kp_weight", 0.0))
        self.smpl_kp = None
        if regressor is not None and self.smpl_kp_weight > 0:
            from . import smpl_loss
            self.smpl_kp = smpl_loss.SmplKeypointLoss(smpl_model, regressor)
            self.KEYS = self.KEYS + ("smpl_kp_loss",)

    def forward(self, outputs, batch):
        total, stats = super().forward(outputs, batch)
        output = outputs[0]
        ind = batch["ind"].detach().to(dtype=torch.int64).contiguous()
        n = ind.shape[1]
        verts = joints = None
        if self.smpl_sup.use_joints or self.smpl_kp is not None:
            _lib.require_cuda(output["pose"], output["shape"], ind)
            verts, joints = smpl.lbs_from_heads(self.smpl_model, output["pose"], output["shape"], ind, n, return_joints=True, exact=True)
        for key, wt, val in zip(LOSS_KEYS, self.weights, self.smpl_sup(output, batch, joints=joints)):
            stats[key] = val
            if wt > 0:
                total = total + wt * val
        if self.smpl_kp is not None:
            from . import smpl_loss
            reg = self.smpl_kp.regressor
            kp = smpl_loss.smpl_keypoint_loss(joints, verts if reg.NV > 0 else None, output["cam"], ind, batch["hps"], batch["hps_mask"], reg, n)
            stats["smpl_kp_loss"] = kp
            total = total + self.smpl_kp_weight * kp
        stats["loss"] = total
        return total, stats
