"""TEST INFRASTRUCTURE ONLY -- the yardstick of the SMPL gradient comparisons: tests/smpl_ref.lbs restated in torch with a `dtype` argument,
differentiable by torch autograd (float64 for the value, float32 for the error a correct fp32 implementation of the same formulas makes),
and the rule of the comparison, which is smpl_ref.check's.  There is no reference SMPL code to measure against, so the
yardstick is the project's own fp64 restatement -- the position the SMPL forward tests take.  Beside the rule over a whole tensor (`check`)
stands the same rule person by person (`check_per_person`), and the mirrors of the kernels' partial counts (`groups`, `splits`).  Shared by tests/test_oracle_smpl_backward.py
and tests/test_gpu_smpl_backward.py; no GPU needed."""
import inspect

import numpy as np
import torch

import smpl_ref as R

GRAD_NAMES = ("grad_betas", "grad_thetas")
FACTOR = inspect.signature(R.check).parameters["factor"].default          # 4.0: taken from smpl_ref.check, not tuned here

# Mirrors of the kernels' constants (tests/test_oracle_smpl_backward.py pins each to its source line)
TILE = 64                 # csrc/smpl_tile.h: `S3_VT = 64` -- vertices per tile; Vpad is V rounded up to it
GROUP_TILES = 4           # csrc/smpl_bwd.hip: `constexpr int SB_NVT = 4;` -- vertex tiles one workgroup folds into one gA partial
SPLIT_K = 1536            # csrc/smpl_bwd.hip: `constexpr int SB_KC = 1536;` -- contraction elements (of 3 Vpad) per coefficient split


def vpad(V):
    """V rounded up to the vertex tile (smpl._device_pack's Vpad)."""
    return -(-V // TILE) * TILE


def groups(V):
    """NG: tile-group partials per person of smpl_bwd_verts_kernel (sb_groups of csrc/smpl_bwd.hip)."""
    return -(-(vpad(V) // TILE) // GROUP_TILES)


def splits(V):
    """NS: split partials per person of smpl_bwd_coef_kernel (sb_splits of csrc/smpl_bwd.hip)."""
    return -(-3 * vpad(V) // SPLIT_K)


def rodrigues(theta, dtype):
    """smpl_ref.rodrigues in torch: angle = ||theta + 1e-8||, axis = theta / angle."""
    e = theta + torch.tensor(1e-8, dtype=dtype, device=theta.device)
    angle = torch.sqrt(e[..., 0:1] * e[..., 0:1] + e[..., 1:2] * e[..., 1:2] + e[..., 2:3] * e[..., 2:3])
    d = theta / angle
    s = torch.sin(angle)[..., None]
    c = torch.cos(angle)[..., None]
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(theta.shape[:-1] + (3, 3))
    return torch.eye(3, dtype=dtype, device=theta.device) + s * K + (1 - c) * (K @ K)


def model_tensors(model, dtype, device="cpu"):
    t = {k: torch.as_tensor(np.asarray(model[k]), dtype=dtype, device=device)
         for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")}
    t["parents"] = [int(p) for p in np.asarray(model["parents"])]
    return t


def lbs(betas, thetas, mt, dtype=torch.float64):
    """smpl_ref.lbs on torch tensors (mt = model_tensors(...)): -> verts [P,V,3], joints [P,24,3], pose_feat [P,207], A [P,24,12]."""
    betas = betas.to(dtype)
    P = betas.shape[0]
    thetas = thetas.to(dtype).reshape(P, R.NJ, 3)
    v_s = mt["v_template"][None] + torch.einsum("vck,pk->pvc", mt["shapedirs"], betas)
    J = torch.einsum("jv,pvc->pjc", mt["J_regressor"], v_s)
    Rm = rodrigues(thetas, dtype)
    pf = (Rm[:, 1:] - torch.eye(3, dtype=dtype, device=betas.device)).reshape(P, R.NPF)
    v_p = v_s + torch.einsum("vck,pk->pvc", mt["posedirs"], pf)
    GR, Gt = [], []
    for j, par in enumerate(mt["parents"]):
        if par < 0:
            GR.append(Rm[:, j])
            Gt.append(J[:, j])
        else:
            GR.append(GR[par] @ Rm[:, j])
            Gt.append((GR[par] @ (J[:, j] - J[:, par])[..., None])[..., 0] + Gt[par])
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)                      # [P,24,3,3], [P,24,3]
    joints = Gt
    At = Gt - torch.einsum("pjab,pjb->pja", GR, J)
    A = torch.cat([GR, At[..., None]], -1)                               # [P,24,3,4]
    Tv = torch.einsum("vj,pjab->pvab", mt["weights"], A)
    vh = torch.cat([v_p, torch.ones(P, v_p.shape[1], 1, dtype=dtype, device=betas.device)], -1)
    verts = torch.einsum("pvab,pvb->pva", Tv, vh)
    return verts, joints, pf, A.reshape(P, R.NJ, 12)


def grads(betas, thetas, model, grad_verts=None, grad_joints=None, dtype=torch.float64, device="cpu"):
    """(grad_betas [P,10], grad_thetas [P,72]) of sum(verts * grad_verts) + sum(joints * grad_joints) by torch autograd in `dtype`
    (numpy or torch inputs; a None upstream is absent)."""
    mt = model_tensors(model, dtype, device)
    b = torch.as_tensor(np.asarray(betas), dtype=dtype, device=device).clone().requires_grad_(True)
    t = torch.as_tensor(np.asarray(thetas), dtype=dtype, device=device).clone().requires_grad_(True)
    verts, joints, _, _ = lbs(b, t, mt, dtype)
    loss = b.sum() * 0 + t.sum() * 0
    if grad_verts is not None:
        loss = loss + (verts * torch.as_tensor(np.asarray(grad_verts), dtype=dtype, device=device)).sum()
    if grad_joints is not None:
        loss = loss + (joints * torch.as_tensor(np.asarray(grad_joints), dtype=dtype, device=device)).sum()
    gb, gt = torch.autograd.grad(loss, (b, t))
    return gb.detach(), gt.detach().reshape(-1, 72)


def bounds(betas, thetas, model, grad_verts=None, grad_joints=None):
    """(target, e32): the float64 gradients and, per tensor, max |float32 autograd - float64 autograd| on the same inputs."""
    g64 = grads(betas, thetas, model, grad_verts, grad_joints, torch.float64)
    g32 = grads(betas, thetas, model, grad_verts, grad_joints, torch.float32)
    e32 = [float((a.double() - r).abs().max()) for a, r in zip(g32, g64)]
    return [g.numpy() for g in g64], e32


def check(name, got, target, e32):
    """smpl_ref.check's rule per gradient tensor: max |gpu - f64| <= FACTOR * e32 + 2^-23 * max |f64|.  Returns the ratios err / e32."""
    ratios, fails = {}, []
    for nm, g, r, e in zip(GRAD_NAMES, got, target, e32):
        g = np.asarray(g.detach().cpu().numpy() if hasattr(g, "detach") else g, np.float64).reshape(r.shape)
        err = float(np.abs(g - r).max())
        limit = FACTOR * e + 2.0 ** -23 * float(np.abs(r).max())
        ratios[nm] = err / e if e > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %s: err %.3g e32 %.3g ratio %.3g limit %.3g max|f64| %.3g" % (name, nm, err, e, ratios[nm], limit, float(np.abs(r).max())))
        if not err <= limit:
            fails.append((nm, err, limit))
    assert not fails, (name, fails)
    return ratios


def _rows(a, shape=None):
    """A gradient tensor (torch or numpy) as float64 [P, -1]."""
    a = np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a.reshape(a.shape[0], -1)


def bounds_per_person(betas, thetas, model, grad_verts=None, grad_joints=None):
    """(target, e32): the float64 gradients and, per tensor, the vector e32[p] = max over person p's row of |float32 autograd - float64
    autograd| on the same inputs.  max(e32[i]) is `bounds`' e32[i]."""
    g64 = grads(betas, thetas, model, grad_verts, grad_joints, torch.float64)
    g32 = grads(betas, thetas, model, grad_verts, grad_joints, torch.float32)
    e32 = [np.abs(_rows(a) - _rows(r)).max(1) for a, r in zip(g32, g64)]
    return [g.numpy() for g in g64], e32


def person_errors(got, target, e32):
    """Per tensor (err [P], limit [P]) of the per-person rule: err[p] = max over person p's row of |g - f64|,
    limit[p] = FACTOR * max(e32[p], median_p e32) + 2^-23 * max over the row of |f64|."""
    out = {}
    for nm, g, r, e in zip(GRAD_NAMES, got, target, e32):
        r = np.asarray(r, np.float64)
        e = np.asarray(e, np.float64).reshape(r.shape[0])
        err = np.abs(_rows(g, r.shape) - _rows(r)).max(1)
        limit = FACTOR * np.maximum(e, np.median(e)) + 2.0 ** -23 * np.abs(_rows(r)).max(1)
        out[nm] = (err, limit)
    return out


def check_per_person(name, got, target, e32):
    """The rule of `check` person by person, e32 = bounds_per_person's vectors: for every person p and each tensor
        max_row |g[p] - f64[p]| <= FACTOR * max(e32[p], median_p e32) + 2^-23 * max_row |f64[p]|.
    One edge pose (special_thetas) raises the whole tensor's e32 a few hundred times above an ordinary person's; here it raises only its
    own limit.  The median floor: a single row's float32 error is partly luck (a factor 5 between ordinary persons), and the floor takes
    the lucky low end away while an edge person keeps its own, larger, e32[p].  Returns the worst err / limit per tensor (<= 1 passes)."""
    worst, fails = {}, []
    for nm, (err, limit) in person_errors(got, target, e32).items():
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(limit > 0, err / limit, np.where(err == 0, 0.0, np.inf))
        ratio = np.where(np.isnan(ratio), np.inf, ratio)                  # a NaN in the result is a failure, not a pass
        p = int(np.argmax(ratio))
        worst[nm] = float(ratio[p])
        print("%s %s per person: worst person %d of %d err %.3g limit %.3g ratio %.3g (e32[p] %.3g, median e32 %.3g)"
              % (name, nm, p, len(err), err[p], limit[p], ratio[p], np.asarray(e32[GRAD_NAMES.index(nm)]).reshape(-1)[p],
                 float(np.median(e32[GRAD_NAMES.index(nm)]))))
        if not ratio[p] <= 1.0:
            fails.append((nm, p, float(err[p]), float(limit[p]), int((ratio > 1.0).sum())))
    assert not fails, (name, [dict(tensor=f[0], person=f[1], err=f[2], limit=f[3], persons_over=f[4]) for f in fails])
    return worst
