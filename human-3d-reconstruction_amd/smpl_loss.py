"""Weak-perspective keypoint reprojection loss on the SMPL output (csrc/smpl_loss.hip, include/h3d.h section 4c):
the link between the 2D keypoint labels `multi_pose_targets` writes (`hps`, `hps_mask`, `ind`) and the `pose` / `shape` head maps, through
`smpl.lbs_from_heads` and its backward.  There is no SMPL code in the reference, so the definition is the project's own:

    kp3d[p,k]   = sum_j JW[k,j] joints[p,j] + sum_i VW[k,i] verts[p, VI[k,i]]
    (s, tx, ty) = cam_map[b, 0..2, ind[b,m]]                  (a raw 3-channel `cam` head, read in place)
    pred[p,k,c] = s kp3d[p,k,c] + t_c                         (output-map pixels relative to the integer centre: what `hps` holds)
    loss        = sum m |pred - hps| / (sum m + 1e-4)         (RegWeightedL1Loss's convention)

    KeypointRegressor(joint_w, vert_idx, vert_w)              the [K,24] joint part and the sparse [K,NV] vertex part of the regressor
    smpl_keypoint_loss(joints, verts, cam_map, ind, hps, hps_mask, regressor, n)   the scalar loss, differentiable at joints / verts / cam_map
    SmplKeypointLoss(smpl_model, regressor)                   forward(output, batch): lbs_from_heads + the loss
    loss_multi_pose_smpl(opt, smpl_model, regressor)          losses.loss_multi_pose + opt.smpl_kp_weight * smpl_kp_loss

The forward is two launches, the backward two; nothing is synchronised with the host."""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib, losses, smpl, synth

MAX_K, MAX_NV = _lib.SMPL_KP_MAX_K, _lib.SMPL_KP_MAX_NV
# COCO's 17 keypoints (nose, eyes, ears, then left / right shoulder, elbow, wrist, hip, knee, ankle) -> SMPL joint, -1 = none (face)
COCO17_SMPL_JOINTS = (-1, -1, -1, -1, -1, 16, 17, 18, 19, 20, 21, 1, 2, 4, 5, 7, 8)


class KeypointRegressor:
    """joint_w [K,24] f32, vert_idx [K,NV] i32, vert_w [K,NV] f32 (NV >= 0; None = no vertex part): keypoint k is
    sum_j joint_w[k,j] joints[j] + sum_i vert_w[k,i] verts[vert_idx[k,i]].  A padding entry has weight 0 and any index in [0, V).
    `inv_*`: the same vertex part listed per touched vertex (ascending), each with its (k, w) in (k, i) order -- what lets the backward
    write every grad_verts row once, in a fixed order, without atomics."""

    def __init__(self, joint_w, vert_idx=None, vert_w=None, num_verts=smpl.NUM_VERTS):
        jw = np.ascontiguousarray(joint_w, np.float32)
        if jw.ndim != 2 or jw.shape[1] != smpl.NUM_JOINTS or jw.shape[0] < 1:
            raise ValueError("KeypointRegressor: joint_w must be [K,%d], got %s" % (smpl.NUM_JOINTS, jw.shape))
        K = jw.shape[0]
        if K > MAX_K:
            raise ValueError("KeypointRegressor: %d keypoints, the kernels are built for at most %d" % (K, MAX_K))
        if (vert_idx is None) != (vert_w is None):
            raise ValueError("KeypointRegressor: vert_idx and vert_w come together")
        if vert_idx is None:
            vi, vw = np.zeros((K, 0), np.int32), np.zeros((K, 0), np.float32)
        else:
            vi_in = np.asarray(vert_idx)
            if vi_in.dtype.kind not in "iu":
                raise ValueError("KeypointRegressor: vert_idx must be integers, got %s" % vi_in.dtype)
            vw = np.ascontiguousarray(vert_w, np.float32)
            if vi_in.ndim != 2 or vi_in.shape[0] != K or vw.shape != vi_in.shape:
                raise ValueError("KeypointRegressor: vert_idx and vert_w must both be [K,NV] with K = %d, got %s and %s" % (K, vi_in.shape, vw.shape))
            if vi_in.size and (int(vi_in.min()) < 0 or int(vi_in.max()) >= num_verts):
                raise ValueError("KeypointRegressor: vertex indices must lie in [0, %d), got %d .. %d" % (num_verts, vi_in.min(), vi_in.max()))
            vi = np.ascontiguousarray(vi_in, np.int32)
        if vi.shape[1] > MAX_NV:
            raise ValueError("KeypointRegressor: %d vertices per keypoint, the kernels are built for at most %d" % (vi.shape[1], MAX_NV))
        if not (np.isfinite(jw).all() and np.isfinite(vw).all()):
            raise ValueError("KeypointRegressor: weights must be finite")
        if num_verts < 1:
            raise ValueError("KeypointRegressor: num_verts = %d" % num_verts)
        self.joint_w, self.vert_idx, self.vert_w = jw, vi, vw
        self.K, self.NV, self.V = K, vi.shape[1], int(num_verts)
        # the inverted table: entries with weight 0 (padding) touch nothing
        rows = {}
        for k in range(K):
            for i in range(self.NV):
                if vw[k, i] != 0.0:
                    rows.setdefault(int(vi[k, i]), []).append((k, vw[k, i]))
        self.inv_vertex = np.array(sorted(rows), np.int32)
        self.inv_start = np.zeros(len(rows) + 1, np.int32)
        ks, ws = [], []
        for t, v in enumerate(self.inv_vertex):
            ks += [k for k, _ in rows[int(v)]]
            ws += [w for _, w in rows[int(v)]]
            self.inv_start[t + 1] = len(ks)
        self.inv_k, self.inv_w = np.array(ks, np.int32), np.array(ws, np.float32)
        self._dev = None

    @classmethod
    def coco17_from_joints(cls, num_verts=smpl.NUM_VERTS):
        """COCO's 12 limb keypoints one-to-one on SMPL joints; the five face rows are zero (mask them, or supply vertex rows).  NV = 0."""
        jw = np.zeros((17, smpl.NUM_JOINTS), np.float32)
        for k, j in enumerate(COCO17_SMPL_JOINTS):
            if j >= 0:
                jw[k, j] = 1.0
        return cls(jw, num_verts=num_verts)

    @classmethod
    def synthetic(cls, K=17, V=smpl.NUM_VERTS, NV=4, seed=0):
        """A seeded regressor for tests: joint rows with three non-zero weights, vertex weights in (0.05, 0.3]; row K-1 is all zero, and
        with NV > 0 keypoints 0 and 1 share a vertex, keypoint 2 ends in a padding entry (weight 0) and keypoint 0 lists a vertex twice when
        NV > 2."""
        u = synth.uniform01("smpl_loss.joint_w", (K, smpl.NUM_JOINTS), seed)
        kth = np.sort(u, axis=1)[:, -3][:, None]
        jw = np.where(u >= kth, u, 0.0)
        jw = (jw / jw.sum(1, keepdims=True) * 0.7).astype(np.float32)
        vi = np.minimum((synth.uniform01("smpl_loss.vert_idx", (K, NV), seed) * V).astype(np.int32), V - 1)
        vw = (0.05 + 0.25 * synth.uniform01("smpl_loss.vert_w", (K, NV), seed)).astype(np.float32)
        jw[K - 1] = 0.0
        if NV > 0:
            vw[K - 1] = 0.0
            if K > 1:
                vi[1, 0] = vi[0, 0]
            if K > 2:
                vw[2, NV - 1] = 0.0
            if NV > 2:
                vi[0, 2] = vi[0, 1]
        return cls(jw, vi if NV > 0 else None, vw if NV > 0 else None, num_verts=V)

    def dense(self):
        """(joint_w [K,24], the vertex part as a dense [K,V] matrix), float64: for restatements and tests."""
        D = np.zeros((self.K, self.V))
        for k in range(self.K):
            for i in range(self.NV):
                D[k, self.vert_idx[k, i]] += float(self.vert_w[k, i])
        return self.joint_w.astype(np.float64), D

    def device(self, dev):
        """The regressor's tensors on `dev`, built once per device."""
        dev = torch.device(dev)
        if self._dev is None or self._dev["joint_w"].device != dev:
            names = ("joint_w", "vert_idx", "vert_w", "inv_vertex", "inv_start", "inv_k", "inv_w")
            self._dev = {nm: torch.from_numpy(getattr(self, nm)).to(dev) for nm in names}
        return self._dev


def _mask(mask, dev):
    """losses.reg_term's mask rule: bool -> uint8 view, uint8 and float32 as they are, anything else through .float()."""
    mask = mask.detach()
    if mask.dtype == torch.bool:
        mask = mask.contiguous().view(torch.uint8)
    elif mask.dtype not in (torch.uint8, torch.float32):
        mask = mask.float()
    return mask.to(dev).contiguous()


class _Inputs:
    """The checked, contiguous operands of one call."""

    def __init__(self, joints, verts, cam_map, ind, hps, hps_mask, regressor, n):
        what = "smpl_keypoint_loss"
        if not isinstance(regressor, KeypointRegressor):
            raise TypeError("%s: regressor must be a KeypointRegressor" % what)
        _lib.require_cuda(joints, verts, cam_map, ind, hps, hps_mask)
        r = regressor
        for nm, t in (("joints", joints), ("verts", verts), ("cam_map", cam_map)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                raise RuntimeError("%s: %s must be a contiguous float32 tensor" % (what, nm))
        if cam_map.dim() != 4 or cam_map.shape[1] != 3:
            raise RuntimeError("%s: cam_map must be [B,3,H,W], got %s" % (what, tuple(cam_map.shape)))
        dev = cam_map.device
        B, HW = cam_map.shape[0], cam_map.shape[2] * cam_map.shape[3]
        ind = ind.detach().to(device=dev, dtype=torch.int64).contiguous()
        if ind.dim() != 2 or ind.shape[0] != B:
            raise RuntimeError("%s: ind must be [B,max_objs], got %s" % (what, tuple(ind.shape)))
        M = ind.shape[1]
        if joints.dim() != 3 or tuple(joints.shape[1:]) != (smpl.NUM_JOINTS, 3):
            raise RuntimeError("%s: joints must be [P,24,3], got %s" % (what, tuple(joints.shape)))
        P = joints.shape[0]
        if n is None:
            n = P // B if B else 0
        if not 0 < n <= M or P != B * n:
            raise RuntimeError("%s: joints hold %d person slots, B * n = %d * %d with 0 < n <= max_objs = %d expected" % (what, P, B, n, M))
        if r.NV > 0:
            if verts is None:
                raise RuntimeError("%s: the regressor has a vertex part (NV = %d), verts must be given" % (what, r.NV))
            if tuple(verts.shape) != (P, r.V, 3):
                raise RuntimeError("%s: verts must be [P,V,3] = %s, got %s" % (what, (P, r.V, 3), tuple(verts.shape)))
        else:
            verts = None
        hps = hps.detach().to(device=dev, dtype=torch.float32).contiguous()
        mask = _mask(hps_mask, dev)
        if tuple(hps.shape) != (B, M, 2 * r.K) or tuple(mask.shape) != (B, M, 2 * r.K):
            raise RuntimeError("%s: hps %s and hps_mask %s must be [B,max_objs,2K] = %s" % (what, tuple(hps.shape), tuple(mask.shape), (B, M, 2 * r.K)))
        if joints.device != dev or (verts is not None and verts.device != dev):
            raise RuntimeError("%s: joints, verts and cam_map must be on one device" % what)
        self.joints, self.verts, self.cam_map, self.ind, self.hps, self.mask = joints, verts, cam_map, ind, hps, mask
        self.mask_type = losses.MASK_F32 if mask.dtype == torch.float32 else losses.MASK_U8
        self.r, self.d = r, r.device(dev)
        self.B, self.M, self.n, self.HW, self.P, self.dev = B, M, n, HW, P, dev


def keypoint_loss_forward(joints, verts, cam_map, ind, hps, hps_mask, regressor, n=None, out=None):
    """h3d_smpl_kp_loss_forward: -> (stats [3] = {loss, l, num}, kp3d [P,K,3], pred [P,K,2], the checked inputs).  out = (kp3d, pred)
    writes into the caller's tensors."""
    a = joints if isinstance(joints, _Inputs) else _Inputs(joints, verts, cam_map, ind, hps, hps_mask, regressor, n)
    r, d = a.r, a.d
    if out is None:
        kp3d = torch.empty(a.P, r.K, 3, dtype=torch.float32, device=a.dev)
        pred = torch.empty(a.P, r.K, 2, dtype=torch.float32, device=a.dev)
    else:
        kp3d, pred = out
    stats = torch.empty(3, dtype=torch.float32, device=a.dev)
    L = _lib.lib()
    ws = _lib.workspace(L.h3d_smpl_kp_loss_workspace_bytes, a.B, a.n, device=a.dev)
    with torch.cuda.device(a.dev):
        _lib.check(L.h3d_smpl_kp_loss_forward(_lib.ptr(a.joints), _lib.ptr(a.verts), _lib.ptr(a.cam_map), _lib.ptr(a.ind), _lib.ptr(a.hps),
                                              _lib.ptr(a.mask), a.mask_type, _lib.ptr(d["joint_w"]), _lib.ptr(d["vert_idx"] if r.NV else None),
                                              _lib.ptr(d["vert_w"] if r.NV else None), a.B, a.M, a.n, a.HW, r.K, r.NV, r.V, _lib.ptr(kp3d),
                                              _lib.ptr(pred), _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "h3d_smpl_kp_loss_forward")
    return stats, kp3d, pred, a


def keypoint_loss_backward(a, stats, kp3d, pred, grad_out, want=(True, True, True), out=None):
    """h3d_smpl_kp_loss_backward for the inputs `a` of a forward: -> (grad_joints [P,24,3], grad_verts [P,V,3], grad_cam_map), None where
    not wanted (grad_verts also with NV == 0).  grad_out: a float32 scalar on the device.  out = the three tensors to write into."""
    r, d = a.r, a.d
    want_v = want[1] and r.NV > 0
    if out is None:
        gj = torch.empty(a.P, smpl.NUM_JOINTS, 3, dtype=torch.float32, device=a.dev) if want[0] else None
        gv = torch.empty(a.P, r.V, 3, dtype=torch.float32, device=a.dev) if want_v else None
        gc = torch.empty_like(a.cam_map) if want[2] else None
    else:
        gj, gv, gc = out
    grad_out = grad_out.detach().to(device=a.dev, dtype=torch.float32).reshape(1).contiguous()
    with torch.cuda.device(a.dev):
        _lib.check(_lib.lib().h3d_smpl_kp_loss_backward(
            _lib.ptr(kp3d), _lib.ptr(pred), _lib.ptr(a.cam_map), _lib.ptr(a.ind), _lib.ptr(a.hps), _lib.ptr(a.mask), a.mask_type, _lib.ptr(stats),
            _lib.ptr(grad_out), _lib.ptr(d["joint_w"]), _lib.ptr(d["inv_vertex"]), _lib.ptr(d["inv_start"]), _lib.ptr(d["inv_k"]),
            _lib.ptr(d["inv_w"]), len(r.inv_vertex), a.B, a.M, a.n, a.HW, r.K, r.V, _lib.ptr(gj), _lib.ptr(gv), _lib.ptr(gc), _lib.stream_ptr()),
            "h3d_smpl_kp_loss_backward")
    return gj, gv, gc


class _KeypointLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, joints, verts, cam_map):
        stats, kp3d, pred, _ = keypoint_loss_forward(a, None, None, None, None, None, None)
        ctx.a, ctx.saved = a, (stats, kp3d, pred)
        ctx.set_materialize_grads(False)
        return stats[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if grad_out is None:
            return None, None, None, None
        stats, kp3d, pred = ctx.saved
        need = ctx.needs_input_grad
        gj, gv, gc = keypoint_loss_backward(ctx.a, stats, kp3d, pred, grad_out, want=(need[1], need[2], need[3]))
        return None, gj, gv, gc


def smpl_keypoint_loss(joints, verts, cam_map, ind, hps, hps_mask, regressor, n=None):
    """joints [P,24,3], verts [P,V,3] (None allowed when regressor.NV == 0, and ignored then), cam_map [B,3,H,W] (contiguous fp32 on the
    GPU), ind [B,max_objs], hps / hps_mask [B,max_objs,2K] (the rows of targets.multi_pose_targets), the first n slots of every image
    (default P / B) -> the scalar loss.  Differentiable at joints, verts and cam_map; with NV == 0 verts receives no gradient (None)."""
    a = _Inputs(joints, verts, cam_map, ind, hps, hps_mask, regressor, n)
    return _KeypointLossFn.apply(a, a.joints, a.verts, a.cam_map)


class SmplKeypointLoss(torch.nn.Module):
    """forward(output, batch): the heads' `pose` / `shape` maps through smpl.lbs_from_heads at batch['ind'], then the loss against
    batch['hps'] / batch['hps_mask'] with the camera read from output['cam'].  n = the person slots per image (default: all max_objs).
    The SMPL forward runs with all six products of its three-term split (fp32-level values, what the f32 detectors run)."""

    def __init__(self, smpl_model, regressor, n=None):
        super().__init__()
        if regressor.V != smpl_model.v_template.shape[0]:
            raise ValueError("SmplKeypointLoss: the regressor is built for %d vertices, the body has %d" % (regressor.V, smpl_model.v_template.shape[0]))
        self.smpl_model, self.regressor, self.n = smpl_model, regressor, n

    def forward(self, output, batch):
        ind = batch["ind"]
        n = self.n or ind.shape[1]
        _lib.require_cuda(output["pose"], output["shape"], output["cam"], ind)
        ind = ind.detach().to(dtype=torch.int64).contiguous()
        verts, joints = smpl.lbs_from_heads(self.smpl_model, output["pose"], output["shape"], ind, n, return_joints=True, exact=True)
        return smpl_keypoint_loss(joints, verts if self.regressor.NV > 0 else None, output["cam"], ind, batch["hps"], batch["hps_mask"],
                                  self.regressor, n)


class loss_multi_pose_smpl(losses.loss_multi_pose):
    """losses.loss_multi_pose plus 'smpl_kp_loss', added to `loss` with weight opt.smpl_kp_weight (default 1)."""
    KEYS = losses.loss_multi_pose.KEYS + ("smpl_kp_loss",)

    def __init__(self, opt, smpl_model, regressor):
        super().__init__(opt)
        self.smpl_kp_weight = getattr(opt, "smpl_kp_weight", 1.0)
        self.smpl_kp = SmplKeypointLoss(smpl_model, regressor)

    def forward(self, outputs, batch):
        total, stats = super().forward(outputs, batch)
        kp = self.smpl_kp(outputs[0], batch)
        stats["smpl_kp_loss"] = kp
        total = total + self.smpl_kp_weight * kp
        stats["loss"] = total
        return total, stats
