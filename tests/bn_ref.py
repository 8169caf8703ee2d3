"""TEST INFRASTRUCTURE: the yardsticks of h3d_amd.bn (include/h3d.h section 2e).

    torch_bn(...)      act(F.batch_norm(x, ..., training) + res) under torch autograd on the CPU, in the dtype asked for (float64: the
                       truth; float32: e32 of the EVALUATION-mode rule), with the running-statistics update of nn.BatchNorm2d.
    restate(...)       the operator restated in numpy in one dtype: m = sum x / N, v = sum (x - m)^2 / N with np.sum(axis=0, dtype=...),
                       then the formulas of the header.  In float32 it is e32 of the TRAINING-mode rule: torch's fp32 CPU batch_norm
                       accumulates float inputs in double, so its error says nothing about an fp32 kernel's sums.
    check(...)         the rule per tensor: max |t - t64| <= 4 e32 + 1e-7 max |t64|  -> err / e32.

The ReLU mask of the backward is an argument ([y > 0] of the output under test, as the operator takes it from its saved output); None:
the yardstick's own."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
MOMENTUM = 0.1
KINDS = ("normal", "big", "tight", "relu", "const")
MODES = [(res, relu) for res in (False, True) for relu in (False, True)]


def data(shape, kind, seed=0):
    """x [B,C,H,W] float32.  normal; big: 100 + noise; tight: 3 + 1e-3 noise; relu: post-ReLU noise with per-channel scales 0.1 ... 10,
    channel 0 all zero; const: noise with the last channel constant.  (The constant is 1.5: N copies of it add up exactly in float32, so
    its mean is 1.5 in every arithmetic and the channel tests var = 0, invstd = eps^-1/2 and nothing else; a constant whose fp32 mean
    rounds would put a rounding error times 316 into y, of a size e32 has only by chance.)"""
    B, C, H, W = shape
    rs = np.random.RandomState(1000 + seed)
    n = rs.randn(B, C, H, W)
    if kind == "normal":
        x = n
    elif kind == "big":
        x = 100.0 + n
    elif kind == "tight":
        x = 3.0 + 1e-3 * n
    elif kind == "relu":
        x = np.maximum(n, 0.0) * np.logspace(-1, 1, C).reshape(1, C, 1, 1)
        x[:, 0] = 0.0
    elif kind == "const":
        x = n
        x[:, C - 1] = 1.5
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def operands(shape, seed=0):
    """gamma, beta, running_mean, running_var [C], res, grad_y [B,C,H,W]: float32 numpy."""
    B, C, H, W = shape
    rs = np.random.RandomState(2000 + seed)
    f = np.float32
    return dict(gamma=(0.5 + rs.rand(C)).astype(f) * np.where(np.arange(C) % 3 == 1, -1, 1).astype(f), beta=(0.3 * rs.randn(C)).astype(f),
                running_mean=(0.2 * rs.randn(C)).astype(f), running_var=(0.5 + rs.rand(C)).astype(f), res=rs.randn(B, C, H, W).astype(f),
                grad_y=rs.randn(B, C, H, W).astype(f))


def torch_bn(x, o, res, relu, training, dtype, mask=None, momentum=MOMENTUM, eps=EPS):
    """-> dict of numpy arrays in `dtype`: y, mean, var (biased; the given statistics in evaluation), running_mean, running_var (after the
    call), grad_x, grad_gamma, grad_beta, grad_res."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    xt, gamma, beta = t(x).requires_grad_(True), t(o["gamma"]).requires_grad_(True), t(o["beta"]).requires_grad_(True)
    rt = t(o["res"]).requires_grad_(True) if res else None
    rm, rv = t(o["running_mean"]).clone(), t(o["running_var"]).clone()
    m0, v0 = rm.clone(), rv.clone()
    z = F.batch_norm(xt, rm, rv, gamma, beta, training, momentum, eps)
    if rt is not None:
        z = z + rt
    if relu:
        m = (z.detach() > 0) if mask is None else torch.from_numpy(np.asarray(mask))
        y = z * m.to(dtype)
    else:
        y = z
    leaves = [xt, gamma, beta] + ([rt] if res else [])
    grads = torch.autograd.grad((y * t(o["grad_y"])).sum(), leaves)
    out = dict(y=y.detach(), running_mean=rm, running_var=rv, grad_x=grads[0], grad_gamma=grads[1], grad_beta=grads[2],
               grad_res=grads[3] if res else None)
    if training:
        xd = xt.detach()
        out["mean"] = xd.mean((0, 2, 3))
        out["var"] = ((xd - out["mean"].view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    else:
        out["mean"], out["var"] = m0, v0
    return {k: (None if v is None else v.numpy()) for k, v in out.items()}


def restate(x, o, res, relu, training, dtype, mask=None, momentum=MOMENTUM, eps=EPS):
    """The operator in numpy, every value and every sum in `dtype` -> the same dict as torch_bn."""
    f = np.dtype(dtype).type
    B, C, H, W = x.shape
    N = B * H * W
    rows = lambda a: np.ascontiguousarray(np.transpose(np.asarray(a), (0, 2, 3, 1))).reshape(N, C).astype(f)
    back = lambda a: np.ascontiguousarray(np.transpose(a.reshape(B, H, W, C), (0, 3, 1, 2)))
    xs, g = rows(x), rows(o["grad_y"])
    gamma, beta, rm, rv = (np.asarray(o[k]).astype(f) for k in ("gamma", "beta", "running_mean", "running_var"))
    if training:
        mean = np.sum(xs, axis=0, dtype=f) / f(N)
        d = xs - mean
        var = np.sum(d * d, axis=0, dtype=f) / f(N)
        new_rm = (f(1) - f(momentum)) * rm + f(momentum) * mean
        new_rv = (f(1) - f(momentum)) * rv + f(momentum) * (var * f(N) / f(N - 1))
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    invstd = f(1) / np.sqrt(var + f(eps))
    z = (xs - mean) * (gamma * invstd) + beta
    if res:
        z = z + rows(o["res"])
    if relu:
        m = (z > 0) if mask is None else rows(mask) > 0
        y, gg = np.where(m, z, f(0)), np.where(m, g, f(0))
    else:
        y, gg = z, g
    xh = (xs - mean) * invstd
    gb = np.sum(gg, axis=0, dtype=f)
    gw = np.sum(gg * xh, axis=0, dtype=f)
    if training:
        gx = (gamma * invstd) * (gg - gb / f(N) - xh * (gw / f(N)))
    else:
        gx = gg * (gamma * invstd)
    out = dict(y=back(y), mean=mean, var=var, running_mean=new_rm, running_var=new_rv, grad_x=back(gx), grad_gamma=gw, grad_beta=gb,
               grad_res=back(gg) if res else None)
    assert all(v is None or v.dtype == f for v in out.values())
    return out


def running_update(rm, rv, mean, var, N, momentum=MOMENTUM):
    """nn.BatchNorm2d's update in float64: (1 - m) running + m batch, the variance unbiased."""
    rm, rv, mean, var = (np.asarray(a, np.float64) for a in (rm, rv, mean, var))
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var * N / (N - 1)


def yardsticks(x, o, res, relu, training, mask=None):
    """(t64, t32): the truth and the arithmetic whose error is e32 -- the numpy restatement in training, torch's float32 in evaluation."""
    t64 = torch_bn(x, o, res, relu, training, torch.float64, mask)
    t32 = restate(x, o, res, relu, training, np.float32, mask) if training else torch_bn(x, o, res, relu, training, torch.float32, mask)
    return t64, t32


def check(what, got, t64, t32):
    """max |t - t64| <= 4 e32 + 1e-7 max |t64| -> err / e32 (0 when both vanish)."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    r64 = np.asarray(t64, np.float64)
    assert got.shape == r64.shape, "%s: shape %s, expected %s" % (what, got.shape, r64.shape)
    err = float(np.abs(got.astype(np.float64) - r64).max())
    e32 = float(np.abs(np.asarray(t32, np.float64) - r64).max())
    top = float(np.abs(r64).max())
    assert np.isfinite(got).all() and err <= 4 * e32 + 1e-7 * top, "%s: err %.3g e32 %.3g max %.3g" % (what, err, e32, top)
    return err / e32 if e32 else 0.0
