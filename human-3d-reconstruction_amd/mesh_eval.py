"""MPJPE / PA-MPJPE / PVE / PA-PVE on the device: the 3D figures of the body-mesh literature for the meshes the SMPL stage produces
(csrc/mesh_eval.hip, include/h3d.h section 8b).  The reference has no code for this (as it has none for SMPL):
include/h3d.h section 8b is the written definition, tests/mesh_eval_ref.py restates it with loops, `evaluate_numpy` is the host mirror,
and the kernels are bit-equal to both.

    GroundTruth3D(joints, verts, valid, joint_weight) / .from_smpl(smpl_model, betas, thetas, valid) / .to(device) / .select(image_index)
    pointset_errors(pred, gt, pred_idx, gt_idx, weight, pred_root, gt_root, root)  -> err [P,2] (plain, aligned), count [P], transform [P,13]
    metric_means(err, count)                                                       -> means [2], n_pairs [1]
    evaluate_numpy(...), metric_means_numpy(...)                                   the host mirror
    evaluate_pairs(pred_joints, pred_verts, gt3d_flat, pred_idx, gt_idx, root)     -> MeshEvalResult(mpjpe, pa_mpjpe, pve, pa_pve, n_pairs, ...)
    MeshEvaluator(gt, gt3d, iou_thr).update(image_index, results, joints, verts) / .compute()

Plain error: the mean distance over the valid points after both sets are moved to their root (the midpoint of two root points, the hips 1
and 2 of the 24 SMPL joints by default; the vertices are aligned by the joints' root).  Aligned error: the same after the best similarity
(scale, rotation, translation) of the prediction onto the ground truth.  Units are the caller's; summarize() assumes metres.  Nothing is
synchronised with the host before the means are read."""
import math

import numpy as np

THREADS, WAVE = 256, 64
JACOBI_TOL = 2.0 ** -50


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------------------
def _block_sum(terms):
    """SUM of include/h3d.h section 8b over the last axis of `terms` [..., n] (invalid points already 0.0: adding +0.0 changes no bit of
    a sum that started at +0.0) -> [...]."""
    n = terms.shape[-1]
    rounds = -(-n // THREADS)
    pad = np.zeros(terms.shape[:-1] + (rounds * THREADS,))
    pad[..., :n] = terms
    pad = pad.reshape(terms.shape[:-1] + (rounds, THREADS))
    acc = np.zeros(terms.shape[:-1] + (THREADS,))
    for k in range(rounds):
        acc = acc + pad[..., k, :]
    v = acc.reshape(terms.shape[:-1] + (THREADS // WAVE, WAVE)).copy()
    off = WAVE // 2
    while off:
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _dot3(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def similarity(M, var, max_sweeps=None):
    """The SVD / U / R, s steps of section 8b on Python floats (IEEE binary64, one operation per step): M = 9 moments row-major, var
    -> (s, R as 9 floats row-major, sweeps run)."""
    from . import _lib
    max_sweeps = _lib.MESH_EVAL_MAX_SWEEPS if max_sweeps is None else max_sweeps
    R = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    if var == 0.0:
        return 1.0, R, 0
    A = [[M[3 * r + c] for r in range(3)] for c in range(3)]            # the columns
    V = [[1.0 if r == c else 0.0 for r in range(3)] for c in range(3)]
    sweeps = 0
    for _ in range(max_sweeps):
        sweeps += 1
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            a, b, g = _dot3(A[p], A[p]), _dot3(A[q], A[q]), _dot3(A[p], A[q])
            if abs(g) <= JACOBI_TOL * max(a, b):
                continue
            rotated = True
            h, g2 = b - a, 2.0 * g
            if abs(g2) <= abs(h):
                r = g2 / h
                t = r / (1.0 + math.sqrt(1.0 + r * r))
            else:
                z = h / g2
                u = 1.0 / (abs(z) + math.sqrt(1.0 + z * z))
                t = -u if z < 0.0 else u
            cs = 1.0 / math.sqrt(1.0 + t * t)
            sn = cs * t
            for X in (A, V):
                for r in range(3):
                    xp, xq = X[p][r], X[q][r]
                    X[p][r] = cs * xp - sn * xq
                    X[q][r] = sn * xp + cs * xq
        if not rotated:
            break
    nn = [_dot3(A[j], A[j]) for j in range(3)]
    o, dv = [0, 1, 2], 1.0
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if nn[o[j]] > nn[o[i]]:
            o[i], o[j], dv = o[j], o[i], -dv
    c0, c1, c2 = A[o[0]], A[o[1]], A[o[2]]
    V0, V1, V2 = V[o[0]], V[o[1]], V[o[2]]
    S0, S1, S2 = math.sqrt(nn[o[0]]), math.sqrt(nn[o[1]]), math.sqrt(nn[o[2]])
    if S0 == 0.0:
        return 0.0, R, sweeps
    U0 = [c0[r] / S0 for r in range(3)]
    U1 = None
    if S1 > 0.0:
        u = [c1[r] / S1 for r in range(3)]
        hh = _dot3(u, U0)
        w = [u[r] - hh * U0[r] for r in range(3)]
        nw = math.sqrt(_dot3(w, w))
        if nw >= 0.5:
            U1 = [w[r] / nw for r in range(3)]
    if U1 is None:
        k = 0
        if abs(U0[1]) < abs(U0[k]):
            k = 1
        if abs(U0[2]) < abs(U0[k]):
            k = 2
        w = [(1.0 if r == k else 0.0) - U0[k] * U0[r] for r in range(3)]
        nw = math.sqrt(_dot3(w, w))
        U1 = [w[r] / nw for r in range(3)]
    U2 = [U0[1] * U1[2] - U0[2] * U1[1], U0[2] * U1[0] - U0[0] * U1[2], U0[0] * U1[1] - U0[1] * U1[0]]
    R = [(U0[r] * V0[c] + U1[r] * V1[c]) + dv * (U2[r] * V2[c]) for r in range(3) for c in range(3)]
    d = -dv if _dot3(c2, U2) < 0.0 else dv
    return ((S0 + S1) + d * S2) / var, R, sweeps


def _norm3(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def evaluate_numpy(pred, gt, pred_idx, gt_idx, weight=None, pred_root=None, gt_root=None, root=(1, 2), return_sweeps=False):
    """The host mirror of `pointset_errors` (numpy float64, the definition of include/h3d.h section 8b op by op, the sum order and the
    Jacobi loop included) -> (err [P,2], count [P] int32, transform [P,13])."""
    pred, gt = np.ascontiguousarray(pred, np.float32), np.ascontiguousarray(gt, np.float32)
    pi, gi = np.asarray(pred_idx, np.int64).reshape(-1), np.asarray(gt_idx, np.int64).reshape(-1)
    P, n = len(pi), pred.shape[1]
    Np, Ng = pred.shape[0], gt.shape[0]
    err, count, tr = np.zeros((P, 2)), np.zeros(P, np.int32), np.zeros((P, 13))
    sweeps = np.zeros(P, np.int32)
    ok = np.nonzero((pi >= 0) & (pi < Np) & (gi >= 0) & (gi < Ng))[0]
    if len(ok) == 0 or n == 0:
        return (err, count, tr, sweeps) if return_sweeps else (err, count, tr)
    p, g = pred[pi[ok]].astype(np.float64), gt[gi[ok]].astype(np.float64)                     # [Q,n,3]
    valid = np.ones(p.shape[:2], bool) if weight is None else np.asarray(weight)[gi[ok]] != 0
    op = og = np.zeros((len(ok), 1, 3))
    if pred_root is not None:
        a, b = root
        rp = np.asarray(pred_root, np.float32)[pi[ok]].astype(np.float64)
        rg = np.asarray(gt_root, np.float32)[gi[ok]].astype(np.float64)
        op, og = ((rp[:, a] + rp[:, b]) * 0.5)[:, None], ((rg[:, a] + rg[:, b]) * 0.5)[:, None]

    def total(f):                       # [Q,n] -> [Q]
        return _block_sum(np.where(valid, f, 0.0))

    cnt = valid.sum(1)
    dn = np.where(cnt > 0, cnt, 1).astype(np.float64)
    plain = total(_norm3((p - op) - (g - og))) / dn
    mp = np.stack([total(p[..., c]) for c in range(3)], 1) / dn[:, None]
    mg = np.stack([total(g[..., c]) for c in range(3)], 1) / dn[:, None]
    x, y = p - mp[:, None], g - mg[:, None]
    M = np.stack([total(y[..., r] * x[..., c]) for r in range(3) for c in range(3)], 1)      # [Q,9]
    var = total((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])
    s, R = np.ones(len(ok)), np.zeros((len(ok), 9))
    for k in range(len(ok)):
        if cnt[k] > 0:
            s[k], R[k], sweeps[ok[k]] = similarity([float(v) for v in M[k]], float(var[k]))
    R3 = R.reshape(-1, 3, 3)
    t = np.stack([mg[:, r] - s * ((R3[:, r, 0] * mp[:, 0] + R3[:, r, 1] * mp[:, 1]) + R3[:, r, 2] * mp[:, 2]) for r in range(3)], 1)
    q = np.stack([s[:, None] * ((R3[:, r, 0, None] * p[..., 0] + R3[:, r, 1, None] * p[..., 1]) + R3[:, r, 2, None] * p[..., 2]) + t[:, r, None]
                  for r in range(3)], 2)
    aligned = total(_norm3(q - g)) / dn
    has = cnt > 0
    err[ok] = np.where(has[:, None], np.stack([plain, aligned], 1), 0.0)
    count[ok] = cnt
    tr[ok] = np.where(has[:, None], np.concatenate([s[:, None], R, t], 1), 0.0)
    return (err, count, tr, sweeps) if return_sweeps else (err, count, tr)


def metric_means_numpy(err, count):
    """The host mirror of `metric_means` -> (means [2], n_pairs)."""
    err, count = np.asarray(err, np.float64).reshape(-1, 2), np.asarray(count).reshape(-1)
    P = len(count)
    keep = count > 0
    rounds = -(-P // WAVE)
    pad = np.zeros((2, max(rounds, 1) * WAVE))
    pad[:, :P] = np.where(keep[None], err.T, 0.0)
    pad = pad.reshape(2, -1, WAVE)
    v = np.zeros((2, WAVE))
    for k in range(pad.shape[1]):
        v = v + pad[:, k]
    off = WAVE // 2
    while off:
        v[:, :off] = v[:, :off] + v[:, off:2 * off]
        off //= 2
    c = int(keep.sum())
    return (v[:, 0] / float(c) if c else np.zeros(2)), c


# ---- the device path ---------------------------------------------------------------------------------------------------------------------------
def pointset_errors(pred, gt, pred_idx, gt_idx, weight=None, pred_root=None, gt_root=None, root=(1, 2), want_transform=False):
    """pred [Np,n,3], gt [Ng,n,3] float32 on the device, pred_idx / gt_idx [P] int32 (-1 or out of range: an invalid pair), weight
    [Ng,n] uint8 or None, root sources pred_root [Np,nr,3] / gt_root [Ng,nr,3] or None with root = (a, b)
    -> (err [P,2] float64: plain and aligned, count [P] int32, transform [P,13] float64 (s, R row-major, t) or None).  One launch."""
    import torch
    from . import _lib
    what = "mesh_eval.pointset_errors"
    _lib.require_cuda(pred, gt, pred_idx, gt_idx, weight, pred_root, gt_root)
    if pred.dim() != 3 or gt.dim() != 3 or pred.shape[2] != 3 or gt.shape[1:] != pred.shape[1:] or pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError("%s: pred [Np,n,3] and gt [Ng,n,3] float32, got %s %s and %s %s"
                           % (what, pred.dtype, tuple(pred.shape), gt.dtype, tuple(gt.shape)))
    dev = pred.device
    pred, gt = pred.detach().contiguous(), gt.detach().contiguous()
    Np, n, Ng = pred.shape[0], pred.shape[1], gt.shape[0]
    pred_idx = pred_idx.detach().to(device=dev, dtype=torch.int32).contiguous().view(-1)
    gt_idx = gt_idx.detach().to(device=dev, dtype=torch.int32).contiguous().view(-1)
    P = pred_idx.numel()
    if gt_idx.numel() != P:
        raise RuntimeError("%s: %d pred_idx and %d gt_idx" % (what, P, gt_idx.numel()))
    if weight is not None:
        weight = (weight.detach() != 0).to(torch.uint8).contiguous()
        if tuple(weight.shape) != (Ng, n):
            raise RuntimeError("%s: weight must be [%d,%d], got %s" % (what, Ng, n, tuple(weight.shape)))
    nr, (a, b) = 0, root
    if (pred_root is None) != (gt_root is None):
        raise RuntimeError("%s: one root source without the other" % what)
    if pred_root is not None:
        pred_root, gt_root = pred_root.detach().contiguous(), gt_root.detach().contiguous()
        nr = pred_root.shape[1]
        if (pred_root.dtype != torch.float32 or gt_root.dtype != torch.float32 or tuple(pred_root.shape) != (Np, nr, 3)
                or tuple(gt_root.shape) != (Ng, nr, 3)):
            raise RuntimeError("%s: root sources must be float32 [%d,nr,3] and [%d,nr,3], got %s and %s"
                               % (what, Np, Ng, tuple(pred_root.shape), tuple(gt_root.shape)))
    err = torch.empty(P, 2, dtype=torch.float64, device=dev)
    count = torch.empty(P, dtype=torch.int32, device=dev)
    tr = torch.empty(P, 13, dtype=torch.float64, device=dev) if want_transform else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().h3d_pointset_errors(
            _lib.ptr(pred), Np, _lib.ptr(gt), Ng, n, _lib.ptr(pred_idx), _lib.ptr(gt_idx), P, _lib.ptr(weight), _lib.ptr(pred_root),
            _lib.ptr(gt_root), nr, int(a), int(b), _lib.ptr(err), _lib.ptr(count), _lib.ptr(tr), _lib.stream_ptr()), "h3d_pointset_errors")
    return err, count, tr


def metric_means(err, count):
    """err [P,2] float64, count [P] int32 on the device -> (means [2] float64 over the pairs with count > 0, n_pairs [1] int32)."""
    import torch
    from . import _lib
    _lib.require_cuda(err, count)
    if err.dtype != torch.float64 or err.dim() != 2 or err.shape[1] != 2 or count.dtype != torch.int32 or count.numel() != err.shape[0]:
        raise RuntimeError("mesh_eval.metric_means: err float64 [P,2] and count int32 [P], got %s %s and %s %s"
                           % (err.dtype, tuple(err.shape), count.dtype, tuple(count.shape)))
    dev = err.device
    err, count = err.detach().contiguous(), count.detach().contiguous()
    means = torch.empty(2, dtype=torch.float64, device=dev)
    n_pairs = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().h3d_metric_means(_lib.ptr(err), _lib.ptr(count), err.shape[0], _lib.ptr(means), _lib.ptr(n_pairs),
                                               _lib.stream_ptr()), "h3d_metric_means")
    return means, n_pairs


class GroundTruth3D:
    """joints [N,G,J,3] or None, verts [N,G,V,3] or None (float32), valid [N,G] (0: no 3D label; crowd ground truths must be 0),
    joint_weight [N,G,J] or None (0: the joint is not labelled; it also selects a subset such as 14 of the 24): numpy arrays or torch
    tensors on any device, padded per image like coco_eval.GroundTruth."""

    def __init__(self, joints, verts, valid, joint_weight=None):
        import torch

        def t(a, dtype):
            return None if a is None else torch.as_tensor(a).detach().to(dtype).contiguous()
        self.joints, self.verts = t(joints, torch.float32), t(verts, torch.float32)
        self.valid = (t(valid, torch.float32) != 0).to(torch.uint8)
        self.joint_weight = None if joint_weight is None else (t(joint_weight, torch.float32) != 0).to(torch.uint8)
        if self.valid.dim() != 2:
            raise ValueError("GroundTruth3D: valid must be [N,G], got %s" % (tuple(self.valid.shape),))
        self.N, self.G = self.valid.shape
        for name, a in (("joints", self.joints), ("verts", self.verts)):
            if a is not None and (a.dim() != 4 or tuple(a.shape[:2]) != (self.N, self.G) or a.shape[3] != 3):
                raise ValueError("GroundTruth3D: %s must be [%d,%d,n,3], got %s" % (name, self.N, self.G, tuple(a.shape)))
        if self.joint_weight is not None and (self.joints is None or tuple(self.joint_weight.shape) != tuple(self.joints.shape[:3])):
            raise ValueError("GroundTruth3D: joint_weight must be [N,G,J] beside joints")
        self._dev = {}

    @classmethod
    def from_smpl(cls, smpl_model, betas, thetas, valid, joint_weight=None):
        """betas [N,G,10], thetas [N,G,72] on the device -> the joints and vertices of smpl.lbs(..., return_joints=True), on that device."""
        from . import smpl
        N, G = betas.shape[:2]
        verts, joints = smpl.lbs(smpl_model, betas.detach().reshape(N * G, 10), thetas.detach().reshape(N * G, 72), return_joints=True,
                                 kernel="auto_exact")
        return cls(joints.view(N, G, -1, 3), verts.view(N, G, -1, 3), valid, joint_weight)

    def _fields(self):
        return {k: getattr(self, k) for k in ("joints", "verts", "valid", "joint_weight")}

    def to(self, device):
        """The device tensors (made once per device): dict(joints, verts, valid, joint_weight)."""
        import torch
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = {k: None if v is None else v.to(device) for k, v in self._fields().items()}
        return self._dev[device]

    def select(self, image_index):
        """The images at `image_index` (any order, repeats allowed) as a GroundTruth3D on the device the data lives on."""
        import torch
        idx = torch.as_tensor(image_index, dtype=torch.int64).reshape(-1)
        f = {k: None if v is None else v.index_select(0, idx.to(v.device)) for k, v in self._fields().items()}
        return GroundTruth3D(f["joints"], f["verts"], f["valid"], f["joint_weight"])

    def flat(self, device):
        """The per-person view evaluate_pairs indexes with image * G + g: dict(joints [N G,J,3], verts [N G,V,3], joint_weight [N G,J])."""
        d = self.to(device)
        return {k: None if d[k] is None else d[k].reshape((self.N * self.G,) + tuple(d[k].shape[2:])) for k in ("joints", "verts", "joint_weight")}


class MeshEvalResult:
    """mpjpe, pa_mpjpe, pve, pa_pve: floats in the caller's unit (None: that point set was not given), n_pairs = the pairs behind the
    means; joint_err / vert_err [P,2] float64 (plain, aligned) and joint_count / vert_count [P] per pair (numpy, invalid pairs 0);
    extra: n_gt3d, n_matched from MeshEvaluator."""

    def __init__(self, joint=None, vert=None, extra=None):
        self.mpjpe = self.pa_mpjpe = self.pve = self.pa_pve = None
        self.joint_err = self.joint_count = self.vert_err = self.vert_count = None
        self.n_pairs = 0
        if vert is not None:
            (self.pve, self.pa_pve), self.n_pairs, self.vert_err, self.vert_count = [float(v) for v in vert[0]], int(vert[1]), vert[2], vert[3]
        if joint is not None:
            (self.mpjpe, self.pa_mpjpe), self.n_pairs, self.joint_err, self.joint_count = [float(v) for v in joint[0]], int(joint[1]), joint[2], joint[3]
        self.extra = extra or {}

    def summarize(self, file=None):
        """The four lines in millimetres (metres in)."""
        lines = []
        for name, v in (("MPJPE", self.mpjpe), ("PA-MPJPE", self.pa_mpjpe), ("PVE", self.pve), ("PA-PVE", self.pa_pve)):
            lines.append(" {:<9} over {:>6d} pairs = {}".format(name, self.n_pairs, "n/a" if v is None else "{:0.2f} mm".format(v * 1000.0)))
        for ln in lines:
            print(ln, file=file)
        return lines


def _pair_errors(pred_joints, pred_verts, flat, pred_idx, gt_idx, root):
    """-> (joint (err, count) or None, vert (err, count) or None) on the device."""
    have_root = pred_joints is not None and flat["joints"] is not None
    rp, rg = (pred_joints, flat["joints"]) if have_root else (None, None)
    joint = vert = None
    if have_root:
        joint = pointset_errors(pred_joints, flat["joints"], pred_idx, gt_idx, flat["joint_weight"], rp, rg, root)[:2]
    if pred_verts is not None and flat["verts"] is not None:
        vert = pointset_errors(pred_verts, flat["verts"], pred_idx, gt_idx, None, rp, rg, root)[:2]
    return joint, vert


def _finish(pairs):
    """(err, count) on the device or None -> what MeshEvalResult takes: the means by metric_means, one read-back at the end."""
    if pairs is None:
        return None
    means, n = metric_means(*pairs)
    return means.cpu().numpy(), int(n.cpu()), pairs[0].cpu().numpy(), pairs[1].cpu().numpy()


def evaluate_pairs(pred_joints, pred_verts, gt3d_flat, pred_idx, gt_idx, root=(1, 2)):
    """pred_joints [Np,J,3] and / or pred_verts [Np,V,3] float32 on the device (None: not evaluated), gt3d_flat = GroundTruth3D.flat(device)
    (or a dict with joints [Ng,J,3], verts [Ng,V,3], joint_weight [Ng,J] or None), pred_idx / gt_idx [P] -> MeshEvalResult.  The joints
    are rooted at the midpoint of joints root[0] and root[1] of either side; the vertices at the same joint roots."""
    joint, vert = _pair_errors(pred_joints, pred_verts, gt3d_flat, pred_idx, gt_idx, root)
    return MeshEvalResult(_finish(joint), _finish(vert))


class MeshEvaluator:
    """Collects a validation run batch by batch.  update(image_index, results, joints, verts): results [B,K,39] as
    detector.multi_pose_post_process returns it, joints [B K,J,3] and verts [B K,V,3] of the same detection slots (smpl.lbs_from_heads).
    A detection is compared with the ground-truth person COCO's greedy box matching (coco_eval.match, 'bbox', area range 'all') gives it
    at IoU `iou_thr`, when that person is `valid` in gt3d and no crowd; the pairs run by detection slot.  Only the per-pair errors and
    counts are kept.  compute() -> MeshEvalResult with extra = dict(n_gt3d: valid persons in the images seen, n_matched: of them
    matched): coverage is reported beside the errors, not folded into them."""

    def __init__(self, gt, gt3d, iou_thr=0.5, root=(1, 2)):
        from . import coco_eval
        if gt3d.N != gt.N or gt3d.G != gt.G:
            raise ValueError("MeshEvaluator: gt3d is [%d,%d], the ground truth [%d,%d]" % (gt3d.N, gt3d.G, gt.N, gt.G))
        at = np.nonzero(np.isclose(coco_eval.IOU_THRS, iou_thr))[0]
        if len(at) != 1:
            raise ValueError("MeshEvaluator: iou_thr %r is none of %s" % (iou_thr, coco_eval.IOU_THRS.tolist()))
        self.gt, self.gt3d, self.t_index, self.root = gt, gt3d, int(at[0]), tuple(root)
        self.area_index = coco_eval.PARAMS["bbox"]["area_lbl"].index("all")
        self.reset()

    def reset(self):
        self._joint, self._vert, self._n_gt3d, self._n_matched = [], [], [], []

    def update(self, image_index, results, joints, verts):
        import torch
        from . import coco_eval
        dev = results.device
        idx = torch.as_tensor(image_index, dtype=torch.int64).reshape(-1)
        if results.dim() != 3 or results.shape[0] != idx.numel():
            raise RuntimeError("MeshEvaluator.update: results %s for %d images" % (tuple(results.shape), idx.numel()))
        B, K = results.shape[:2]
        for name, a in (("joints", joints), ("verts", verts)):
            if a is not None and (a.dim() != 3 or a.shape[0] != B * K or a.shape[2] != 3):
                raise RuntimeError("MeshEvaluator.update: %s must be [%d,n,3], got %s" % (name, B * K, tuple(a.shape)))
        gsel = self.gt.select(idx.tolist())
        g3 = self.gt3d.select(idx)
        m = coco_eval.match(results.detach().float(), gsel, "bbox", want_ious=False)
        dm = m["dt_match"][:, self.area_index, self.t_index, :].to(torch.int64)                 # [B,K]: index into the image's ground truths
        G = self.gt.G
        g = gsel.to(dev)
        usable = (g3.to(dev)["valid"] != 0) & (g["iscrowd"] == 0) & (torch.arange(G, device=dev)[None] < g["num"][:, None])   # [B,G]
        hit = dm >= 0
        if G:
            hit = hit & torch.gather(usable, 1, dm.clamp(min=0))
        gt_idx = torch.where(hit, torch.arange(B, device=dev)[:, None] * G + dm, torch.full_like(dm, -1)).to(torch.int32).reshape(-1)
        pred_idx = torch.arange(B * K, dtype=torch.int32, device=dev)
        joint, vert = _pair_errors(None if joints is None else joints.detach().float(), None if verts is None else verts.detach().float(),
                                   g3.flat(dev), pred_idx, gt_idx, self.root)
        if joint is not None:
            self._joint.append(joint)
        if vert is not None:
            self._vert.append(vert)
        self._n_gt3d.append(usable.sum())
        self._n_matched.append(hit.sum())

    def compute(self):
        import torch
        if not self._n_gt3d:
            raise RuntimeError("MeshEvaluator.compute: no update() yet")

        def cat(parts):
            return (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])) if parts else None
        extra = {"n_gt3d": int(torch.stack(self._n_gt3d).sum().cpu()), "n_matched": int(torch.stack(self._n_matched).sum().cpu())}
        return MeshEvalResult(_finish(cat(self._joint)), _finish(cat(self._vert)), extra)
