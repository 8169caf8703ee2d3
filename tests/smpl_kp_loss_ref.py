"""TEST INFRASTRUCTURE ONLY -- the yardstick of the SMPL keypoint reprojection loss (h3d_amd/smpl_loss.py, include/h3d.h section 4c): the
definition restated in differentiable torch ops with a `dtype` argument (float64 for the value, float32 for the error a plain fp32
implementation of the same formulas makes), the case builders, and the rule of the comparison.  There is no reference code for this loss
(SURVEY section 0): as for the SMPL stage itself the yardstick is the project's own fp64 restatement.  No GPU needed.

The rule (losses_ref.check_tensor, the project's: DESIGN sections 13 / 15 / 18): max |gpu - f64| <= 4 e32 + 1e-7 max |f64| with e32 = max |f32
restatement - f64 restatement| over the tensor.  A scalar's fp32 error is a matter of luck for a single input (losses_ref.pooled_e32), so
the loss scalars of the test cases are pooled: e32 = the largest relative fp32 error over the cases, rel err <= 4 e32 + 1e-7
(losses_ref.check_scalars).

The L1 sign is discontinuous: every case is drawn (and re-drawn by seed until it holds, on the CPU) so that every masked |pred - hps| of the
fp64 restatement is at least SIGN_MARGIN of the largest -- the labels of the generated cases are the fp64 restatement's own projection moved
by 0.25 .. 4 pixels either way; no element is ever excluded from a comparison."""
import numpy as np
import torch

import smpl_grad_ref as G

SIGN_MARGIN = 1e-3
FACTOR = 4.0


def kp_loss(joints, verts, cam_map, ind, hps, mask, reg, n, dtype=torch.float64):
    """The definition: joints [P,24,3], verts [P,V,3] or None, cam_map [B,3,H,W], ind [B,M] int64, hps / mask [B,M,2K], reg = a
    KeypointRegressor, the first n slots -> (loss, kp3d [P,K,3], pred [P,K,2], masked |pred - hps| [P,K,2], the effective mask [P,K,2])."""
    B, HW = cam_map.shape[0], cam_map.shape[2] * cam_map.shape[3]
    K, P = reg.K, joints.shape[0]
    kp3d = torch.einsum("kj,pjc->pkc", torch.from_numpy(reg.joint_w).to(dtype), joints.to(dtype))
    if reg.NV > 0:
        vi = torch.from_numpy(reg.vert_idx.astype(np.int64)).reshape(-1)
        g = verts.to(dtype)[:, vi].reshape(P, K, reg.NV, 3)
        kp3d = kp3d + (torch.from_numpy(reg.vert_w).to(dtype)[None, :, :, None] * g).sum(2)
    idx = ind[:, :n]
    valid = ((idx >= 0) & (idx < HW)).reshape(P, 1, 1).to(dtype)           # a slot outside the map adds nothing (and its pred is 0)
    cam = cam_map.to(dtype).reshape(B, 3, HW).gather(2, idx.clamp(0, HW - 1)[:, None, :].expand(B, 3, n)).permute(0, 2, 1).reshape(P, 3)
    pred = (cam[:, 0, None, None] * kp3d[..., :2] + cam[:, None, 1:3]) * valid
    m = mask[:, :n].to(dtype).reshape(P, K, 2) * valid
    diff = m * (pred - hps[:, :n].to(dtype).reshape(P, K, 2)).abs()
    return diff.sum() / (m.sum() + 1e-4), kp3d, pred, diff, m


def value_and_grads(c, dtype):
    """(loss, kp3d, pred, grad_joints, grad_verts or None, grad_cam_map) of case `c` in `dtype` on the CPU, upstream gradient c.go."""
    j = c.joints.to(dtype).clone().requires_grad_(True)
    v = None if c.reg.NV == 0 else c.verts.to(dtype).clone().requires_grad_(True)
    cam = c.cam.to(dtype).clone().requires_grad_(True)
    loss, kp3d, pred, _, _ = kp_loss(j, v, cam, c.ind, c.hps, c.mask, c.reg, c.n, dtype)
    leaves = [j, cam] + ([v] if v is not None else [])
    gr = torch.autograd.grad(loss * c.go, leaves, allow_unused=True)
    z = lambda g, like: torch.zeros_like(like) if g is None else g
    return (loss.detach(), kp3d.detach(), pred.detach(), z(gr[0], j), None if v is None else z(gr[2], v), z(gr[1], cam))


def sign_margin(diff, m):
    """The smallest masked |pred - hps| over the largest (1 when nothing is masked in)."""
    live = m > 0
    if not bool(live.any()):
        return 1.0
    return float(diff[live].min()) / float(diff.max()) if float(diff.max()) > 0 else 0.0


class Case:
    """One set of inputs at the joints / vertices, float32 on the CPU, which passes the sign condition."""

    def __init__(self, reg, B, M, n, H, W, seed, mask="some", bad_ind=None, share=None, tries=50):
        self.reg, self.B, self.M, self.n, self.H, self.W = reg, B, M, n, H, W
        for s in range(seed, seed + tries):
            self._draw(s, mask, bad_ind, share)
            if self.margin() >= SIGN_MARGIN:
                self.seed = s
                return
        raise AssertionError("no draw with a sign margin in %d tries" % tries)

    def _draw(self, seed, mask, bad_ind, share):
        rs = np.random.RandomState(seed)
        r, B, M, n, HW = self.reg, self.B, self.M, self.n, self.H * self.W
        P, K = B * n, r.K
        f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
        self.joints = f(rs.randn(P, 24, 3) * 0.4)
        self.verts = f(rs.randn(P, r.V, 3) * 0.4)
        cam = rs.randn(B, 3, HW)
        cam[:, 0] = 4.0 + 8.0 * rs.rand(B, HW)                  # a positive scale of a few map pixels per unit, as a trained head would hold
        self.cam = f(cam.reshape(B, 3, self.H, self.W))
        ind = np.stack([rs.permutation(HW)[np.arange(M) % HW] for _ in range(B)]).astype(np.int64)
        if share is not None:                                   # (b, m0, m1): two slots of image b on one pixel
            ind[share[0], share[2]] = ind[share[0], share[1]]
        if bad_ind is not None:                                 # {(b, m): value outside [0, HW)}
            for (b, m), v in bad_ind.items():
                ind[b, m] = v
        self.ind = torch.from_numpy(ind)
        self.hps = torch.zeros(B, M, 2 * K)
        self.mask = torch.ones(B, M, 2 * K, dtype=torch.uint8)
        # the labels: the fp64 restatement's own projection moved by 0.25 .. 4 pixels either way, so that no |pred - hps| is near its kink
        pred = kp_loss(self.joints, self.verts, self.cam, self.ind, self.hps, self.mask, r, n)[2].reshape(B, n, 2 * K)
        self.hps = f(rs.randn(B, M, 2 * K) * 3.0)
        self.hps[:, :n] = (pred + torch.from_numpy(rs.choice([-1.0, 1.0], pred.shape) * rs.uniform(0.25, 4.0, pred.shape))).float()
        if mask == "some":
            mk = rs.rand(B, M, 2 * K) < 0.7
            mk[:, 0] = True
            if M > 1:
                mk[:, 1, ::3] = False                           # a partially masked person
            if M > 2:
                mk[-1, 2] = False                               # a fully masked one
        elif mask == "none":
            mk = np.zeros((B, M, 2 * K), bool)
        else:
            mk = np.ones((B, M, 2 * K), bool)
        self.mask = torch.from_numpy(mk.astype(np.uint8))
        self.go = float(0.5 + rs.rand())                        # the upstream gradient of the scalar

    def margin(self):
        return sign_margin(*kp_loss(self.joints, self.verts, self.cam, self.ind, self.hps, self.mask, self.reg, self.n)[3:5])

    def refs(self):
        """(float64 results, float32 results) of value_and_grads, computed once."""
        if not hasattr(self, "_refs"):
            self._refs = (value_and_grads(self, torch.float64), value_and_grads(self, torch.float32))
        return self._refs


# ---- through the SMPL stage: the head maps -> the loss ------------------------------------------------------------------------------------
def gather_rows(fmap, idx):
    """fmap [B,C,H,W], idx [B,n] -> [B*n, C]: what _transpose_and_gather_feat would copy out (differentiable)."""
    B, C = fmap.shape[:2]
    n = idx.shape[1]
    return fmap.reshape(B, C, -1).gather(2, idx[:, None, :].expand(B, C, n)).permute(0, 2, 1).reshape(B * n, C)


def maps_loss(pose_map, shape_map, cam_map, ind, hps, mask, reg, n, mt, dtype=torch.float64):
    """lbs_from_heads + the loss, restated: the first n slots' thetas / betas gathered from the maps, smpl_grad_ref.lbs, kp_loss.
    mt = smpl_grad_ref.model_tensors(body, dtype).  -> (loss, masked |pred - hps|, the effective mask, pred)."""
    idx = ind[:, :n]
    verts, joints, _, _ = G.lbs(gather_rows(shape_map.to(dtype), idx), gather_rows(pose_map.to(dtype), idx), mt, dtype)
    loss, _, pred, diff, m = kp_loss(joints, verts if reg.NV > 0 else None, cam_map, ind, hps, mask, reg, n, dtype)
    return loss, diff, m, pred


def maps_value_and_grads(pose_map, shape_map, cam_map, ind, hps, mask, reg, n, body, dtype):
    """(loss, grad_pose_map, grad_shape_map, grad_cam_map, margin) in `dtype` on the CPU; body = an SMPLModel.numpy_dict()."""
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (pose_map, shape_map, cam_map)]
    loss, diff, m, _ = maps_loss(leaves[0], leaves[1], leaves[2], ind, hps, mask, reg, n, G.model_tensors(body, dtype), dtype)
    gr = torch.autograd.grad(loss, leaves)
    return (loss.detach(),) + tuple(gr) + (sign_margin(diff.detach(), m),)
