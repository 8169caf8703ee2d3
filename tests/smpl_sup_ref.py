"""The yardstick of the SMPL 3D supervision (include/h3d.h section 4e): the label transform restated in numpy
float64 and the three-term loss in torch ops with a `dtype` argument (float64 under autograd is the reference, float32 the error scale).

The rule of every comparison: max |gpu - f64| <= 4 e32 + 1e-7 max |f64| per tensor, e32 = the float32 restatement's error on the same
inputs (losses_ref.check_tensor); the loss scalars pooled over the cases (losses_ref.check_scalars)."""
import numpy as np
import torch

import smpl_grad_ref as G
from smpl_kp_loss_ref import gather_rows

NJ, NB = 24, 10
PAIRS = ((1, 2), (4, 5), (7, 8), (10, 11), (13, 14), (16, 17), (18, 19), (20, 21), (22, 23))
PI = list(range(NJ))
for _a, _b in PAIRS:
    PI[_a], PI[_b] = _b, _a
S = np.diag([-1.0, 1.0, 1.0])
NAMES = ("smpl_rotmat", "smpl_pose_w", "smpl_shape", "smpl_shape_w", "smpl_joints", "smpl_joints_w")
FACTOR = 4.0


# ---- the label transform, numpy float64 ------------------------------------------------------------------------------------------------------
def rodrigues_np(theta):
    """[...,3] -> [...,3,3] float64: angle = ||theta + 1e-8||, axis = theta / angle, R = I + sin K + (1 - cos) K^2 (smpl_pose.h)."""
    theta = np.asarray(theta, np.float64)
    e = theta + 1e-8
    angle = np.sqrt((e * e).sum(-1, keepdims=True))
    d = theta / angle
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    zero = np.zeros_like(x)
    K = np.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(theta.shape[:-1] + (3, 3))
    sn, oc = np.sin(angle)[..., None], (2.0 * np.sin(0.5 * angle) ** 2)[..., None]
    return np.eye(3) + sn * K + oc * (K @ K)


def closed_form_rot2(rot_deg):
    r = np.asarray(rot_deg, np.float64) * np.pi / 180
    return np.stack([np.stack([np.cos(r), np.sin(r)], -1), np.stack([-np.sin(r), np.cos(r)], -1)], -2)


def rz(A2):
    out = np.eye(3)
    out[:2, :2] = A2
    return out


def transform_one(R, J, w, flipped, A2):
    """One annotation in float64: R [24,3,3], J [24,3] or None, w [k,24] (any number of weight rows) -> the same, mirrored then rotated."""
    R, w = np.array(R, np.float64), np.array(w, np.float64)
    J = None if J is None else np.array(J, np.float64)
    if flipped:
        R2, w2 = np.empty_like(R), np.empty_like(w)
        for j in range(NJ):
            R2[PI[j]] = S @ R[j] @ S
            w2[:, PI[j]] = w[:, j]
        R, w = R2, w2
        if J is not None:
            J2 = np.empty_like(J)
            for j in range(NJ):
                J2[PI[j]] = S @ J[j]
            J = J2
    if A2 is not None:
        Z = rz(A2)
        R = R.copy()
        R[0] = Z @ R[0]
        if J is not None:
            J = J @ Z.T
    return R, J, w


def labels_np(pose, shape, joints, valid, pose_w, joints_w, num, reg_mask, flipped, rot2, max_objs):
    """The six outputs of h3d_smpl_sup_labels as float64 arrays (round to float32 to compare; weights and smpl_shape are exact)."""
    pose, shape, valid = np.asarray(pose, np.float64), np.asarray(shape, np.float64), np.asarray(valid, np.float64)
    B, M = valid.shape
    N = max_objs
    o = {"smpl_rotmat": np.zeros((B, N, NJ, 9)), "smpl_pose_w": np.zeros((B, N, NJ)), "smpl_shape": np.zeros((B, N, NB)),
         "smpl_shape_w": np.zeros((B, N)), "smpl_joints": np.zeros((B, N, NJ, 3)), "smpl_joints_w": np.zeros((B, N, NJ))}
    for b in range(B):
        for m in range(min(int(num[b]), N, M)):
            if reg_mask[b, m] == 0 or valid[b, m] == 0:
                continue
            wp = np.asarray(pose_w[b, m], np.float64) if pose_w is not None else np.full(NJ, valid[b, m])
            wj = np.zeros(NJ) if joints is None else np.asarray(joints_w[b, m], np.float64) if joints_w is not None else np.full(NJ, valid[b, m])
            th = np.where((wp != 0)[:, None], pose[b, m].reshape(NJ, 3), 0.0)                # a label behind weight 0 is not read
            J = None if joints is None else np.where((wj != 0)[:, None], np.asarray(joints[b, m], np.float64), 0.0)
            R, J, w = transform_one(rodrigues_np(th), J, np.stack([wp, wj]), bool(flipped is not None and flipped[b]),
                                    None if rot2 is None else rot2[b])
            o["smpl_pose_w"][b, m], o["smpl_joints_w"][b, m] = w[0], w[1]
            o["smpl_rotmat"][b, m] = np.where((w[0] != 0)[:, None], R.reshape(NJ, 9), 0.0)
            if J is not None:
                o["smpl_joints"][b, m] = np.where((w[1] != 0)[:, None], J, 0.0)
            o["smpl_shape"][b, m], o["smpl_shape_w"][b, m] = shape[b, m], valid[b, m]
    return o


# ---- the loss, torch ---------------------------------------------------------------------------------------------------------------------------
def sup_loss(pose_map, shape_map, ind, joints, lab, n, dtype=torch.float64):
    """-> (losses [3], l [3], num [3]) of the pose, shape and joint terms.  lab: the six tensors [B,max_objs,...]; joints [B n,24,3] or None.
    A weight of 0 selects 0 (its label may be NaN); a slot whose ind lies outside the map has all its weights taken as 0."""
    B, HW = pose_map.shape[0], pose_map.shape[2] * pose_map.shape[3]
    idx = ind[:, :n]
    ok = (idx >= 0) & (idx < HW)
    idc = idx.clamp(0, HW - 1)
    zero = torch.zeros((), dtype=dtype)
    cut = lambda nm: lab[nm][:, :n].to(dtype)
    wp = torch.where(ok[..., None], cut("smpl_pose_w"), zero)
    ws = torch.where(ok, cut("smpl_shape_w"), zero)
    theta = gather_rows(pose_map.to(dtype), idc).reshape(B, n, NJ, 3)
    beta = gather_rows(shape_map.to(dtype), idc).reshape(B, n, NB)
    R = G.rodrigues(theta, dtype).reshape(B, n, NJ, 9)
    Rl = torch.where((wp != 0)[..., None], cut("smpl_rotmat"), zero)
    l_pose, num_pose = (wp * ((R - Rl) ** 2).sum(-1)).sum(), 9.0 * wp.sum()
    bl = torch.where((ws != 0)[..., None], cut("smpl_shape"), zero)
    l_shape, num_shape = (ws * ((beta - bl) ** 2).sum(-1)).sum(), 10.0 * ws.sum()
    if joints is None:
        l_j, num_j = zero, zero
    else:
        wj = torch.where(ok[..., None], cut("smpl_joints_w"), zero)
        J = joints.to(dtype).reshape(B, n, NJ, 3)
        Jl_raw = cut("smpl_joints")
        Jl = torch.where((wj != 0)[..., None], Jl_raw, zero)
        any_w = (wj != 0).any(-1)[..., None]
        root_l = torch.where(any_w, 0.5 * (Jl_raw[:, :, 1] + Jl_raw[:, :, 2]), zero)[:, :, None]          # read whatever the weights of joints 1, 2
        root = 0.5 * (J[:, :, 1] + J[:, :, 2])[:, :, None]
        d = (J - root) - (Jl - root_l)
        l_j, num_j = (wj * (d ** 2).sum(-1)).sum(), 3.0 * wj.sum()
    l, num = torch.stack([l_pose, l_shape, l_j]), torch.stack([num_pose, num_shape, num_j])
    return l / (num + 1e-4), l, num


class Case:
    """Seeded head maps, joints and label tensors.  Pose rows hold theta_j = 0 exactly, |theta_j| = 1e-6, |theta_j| = 3.1 and N(0, 0.5) draws."""

    def __init__(self, B, M, n, H, W, seed, weights="some", bad_ind=None, nan_behind=False):
        rs = np.random.RandomState(seed)
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
        self.B, self.M, self.n, self.H, self.W = B, M, n, H, W
        pose = rs.randn(B, NJ, 3, H * W) * 0.5
        ind = np.stack([rs.permutation(H * W)[:M] for _ in range(B)]).astype(np.int64)
        for b in range(B):                                   # the special rows sit on labelled pixels
            unit = rs.randn(3, 3)
            unit /= np.linalg.norm(unit, axis=1, keepdims=True)
            pose[b, 0, :, ind[b, 0]] = 0.0
            pose[b, 3, :, ind[b, 0]] = 0.0
            pose[b, 5, :, ind[b, 0]] = 1e-6 * unit[0]
            pose[b, 7, :, ind[b, min(1, M - 1)]] = 3.1 * unit[1]
            pose[b, 2, :, ind[b, min(1, M - 1)]] = 1e-6 * unit[2]
        self.pose = f(pose.reshape(B, 72, H, W))
        self.shape = f(rs.randn(B, NB, H, W))
        for (b, m), v in (bad_ind or {}).items():
            ind[b, m] = v
        self.ind = torch.from_numpy(ind)
        self.joints = f(rs.randn(B * n, NJ, 3) * 0.4)
        lab_pose = rs.randn(B, M, NJ, 3) * 0.5
        lab_pose[:, 0, 4] = 0.0                              # a label at the rest pose
        wp = (rs.rand(B, M, NJ) < 0.8) * (0.25 + rs.rand(B, M, NJ))
        wj = (rs.rand(B, M, NJ) < 0.8) * (0.25 + rs.rand(B, M, NJ))
        wj[:, :, 1:3] = 0.25 + rs.rand(B, M, 2)              # the root joints of a labelled person carry weight
        ws = (rs.rand(B, M) < 0.8) * (0.25 + rs.rand(B, M))
        wp[:, 0], ws[:, 0] = 0.25 + rs.rand(B, NJ), 1.0
        if weights == "none":
            wp, wj, ws = wp * 0, wj * 0, ws * 0
        gone = wj.sum(-1) == 0
        Jl = rs.randn(B, M, NJ, 3) * 0.4
        Rl = rodrigues_np(lab_pose).reshape(B, M, NJ, 9)
        bl = rs.randn(B, M, NB)
        if weights == "none" or nan_behind:                  # NaN labels behind every weight of 0 (the label root only in all-zero rows)
            Rl = np.where((wp != 0)[..., None], Rl, np.nan)
            bl = np.where((ws != 0)[..., None], bl, np.nan)
            nanj = (wj == 0) & (gone[..., None] | ~np.isin(np.arange(NJ), (1, 2)))
            Jl = np.where(nanj[..., None], np.nan, Jl)
        if nan_behind:                                       # rows m >= n are never read: NaN everywhere, NaN weights included
            Rl[:, n:], bl[:, n:], Jl[:, n:] = np.nan, np.nan, np.nan
            wp[:, n:], ws[:, n:], wj[:, n:] = np.nan, np.nan, np.nan
        self.lab = {"smpl_rotmat": f(Rl), "smpl_pose_w": f(wp), "smpl_shape": f(bl), "smpl_shape_w": f(ws), "smpl_joints": f(Jl), "smpl_joints_w": f(wj)}
        self.go = torch.from_numpy((0.5 + rs.rand(3)).astype(np.float32))       # the upstream gradient of the three losses
        self._refs = {}

    def refs(self, with_joints=True):
        """(r64, r32), each (losses [3], l [3], num [3], grad_pose_map, grad_shape_map, grad_joints | None): computed once."""
        if with_joints not in self._refs:
            self._refs[with_joints] = tuple(value_and_grads(self, dt, with_joints) for dt in (torch.float64, torch.float32))
        return self._refs[with_joints]


def value_and_grads(c, dtype, with_joints=True):
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (c.pose, c.shape)]
    j = c.joints.to(dtype).clone().requires_grad_(True) if with_joints else None
    loss, l, num = sup_loss(leaves[0], leaves[1], c.ind, j, c.lab, c.n, dtype)
    gr = torch.autograd.grad((loss * c.go.to(dtype)).sum(), leaves + ([j] if with_joints else []), allow_unused=True)
    gr = [torch.zeros_like(t) if g is None else g for g, t in zip(gr, leaves + ([j] if with_joints else []))]
    return (loss.detach(), l.detach(), num.detach(), gr[0], gr[1], gr[2] if with_joints else None)


# ---- through the SMPL stage ------------------------------------------------------------------------------------------------------------------
def maps_loss(pose_map, shape_map, ind, lab, n, mt, dtype=torch.float64):
    """lbs_from_heads(..., return_joints=True) + the loss, restated: mt = smpl_grad_ref.model_tensors(body, dtype)."""
    idx = ind[:, :n].clamp(0, pose_map.shape[2] * pose_map.shape[3] - 1)
    _, joints, _, _ = G.lbs(gather_rows(shape_map.to(dtype), idx), gather_rows(pose_map.to(dtype), idx), mt, dtype)
    return sup_loss(pose_map, shape_map, ind, joints, lab, n, dtype)


def maps_value_and_grads(c, body, dtype, go=None):
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (c.pose, c.shape)]
    loss, l, num = maps_loss(leaves[0], leaves[1], c.ind, c.lab, c.n, G.model_tensors(body, dtype), dtype)
    gr = torch.autograd.grad((loss * (c.go if go is None else go).to(dtype)).sum(), leaves)
    return loss.detach(), gr[0], gr[1]
