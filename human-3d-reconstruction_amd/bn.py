"""BatchNorm2d with batch statistics (include/h3d.h section 2e, csrc/bn.hip): nn.BatchNorm2d (+ residual) (+ ReLU) as the reference
trains it (models/model.py: every nn.BatchNorm2d(…, momentum=BN_MOMENTUM) under HMRTrainer's model.train()), and its gradients.

    batch_norm_forward(x, weight, bias, mean, var, training, ...)   one h3d_batch_norm_forward call -> (y, save_mean, var, save_invstd)
    batch_norm_backward(x, y, grad_y, weight, save_mean, save_invstd, training, relu, need)
                                                                    one h3d_batch_norm_backward call -> (grad_x, grad_res, grad_w, grad_b)
    batch_norm_autograd(x, weight, bias, running_mean, running_var, training, momentum, eps, res, relu)
                                                                    act(F.batch_norm(...) + res) as ONE torch.autograd.Function
    TrainableBatchNorm2d                                            nn.BatchNorm2d on it: forward(input, res=None, relu=False)

    y = act((x - mean) * (weight * invstd) + bias + res),  invstd = 1 / sqrt(var + eps)
training: mean / var are the batch's (biased variance), differentiated through; the running statistics move by `momentum` (the variance
unbiased, N / (N - 1)) inside the operator's own launches.  evaluation: mean / var are the running statistics, constants.
Memory format: `conv._as_nhwc`'s rules, so a chain with `conv.conv2d_autograd` never relays out.  The skip's gradient without ReLU is
grad_y itself, passed on without a copy.
"""
import ctypes

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, arch
from .conv import _as_nhwc, _cs

_WORKSPACES = {}       # (device, stream, B, C, H, W) -> uint8 tensor


def _check(what, x, shape=None):
    _lib.require_cuda(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise RuntimeError("%s must be float32 [B,C,H,W], got %s %s" % (what, x.dtype, tuple(x.shape)))
    if x.shape[1] % 4:
        raise RuntimeError("%s: %d channels (a multiple of 4 is required)" % (what, x.shape[1]))
    if shape is not None and tuple(x.shape) != tuple(shape):
        raise RuntimeError("%s must be %s, got %s" % (what, tuple(shape), tuple(x.shape)))


def _check_vec(what, t, C):
    _lib.require_cuda(t)
    if t.dtype != torch.float32 or tuple(t.shape) != (C,) or not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous float32 [%d], got %s %s" % (what, C, t.dtype, tuple(t.shape)))


def plan(B, C, H, W):
    """(chunk, slots) of the operator's sums for this shape: workgroups of `chunk` pixels, `slots` = ceil(B H W / chunk) partial sums per
    channel, added in chains of at most 64 (include/h3d.h section 2e)."""
    chunk, slots = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().h3d_batch_norm_plan(B, C, H, W, ctypes.byref(chunk), ctypes.byref(slots)), "h3d_batch_norm_plan")
    return chunk.value, slots.value


def _workspace(dev, B, C, H, W):
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream, B, C, H, W)
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _lib.workspace(_lib.lib().h3d_batch_norm_workspace_bytes, B, C, H, W, device=dev, min_bytes=256, what="batch_norm")
        _WORKSPACES[key] = ws
    return ws


def _forward_nhwc(xv, weight, bias, resv, mean, var, running_mean, running_var, training, relu, momentum, eps):
    """One h3d_batch_norm_forward call on NHWC views -> (y [B,H,W,C], save_mean, var, save_invstd).  training: mean / var are ignored and
    fresh tensors returned, running_* (or None) are updated in place; evaluation: mean / var are read."""
    B, H, W, C = xv.shape
    dev = xv.device
    y = torch.empty(B, H, W, C, dtype=torch.float32, device=dev)
    if training:
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        var = torch.empty(C, dtype=torch.float32, device=dev)
    invstd = torch.empty(C, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(dev, B, C, H, W)
        rc = _lib.lib().h3d_batch_norm_forward(_lib.ptr(xv), _cs(xv), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(resv),
                                               C if resv is None else _cs(resv), _lib.ptr(y), C, _lib.ptr(mean), _lib.ptr(var),
                                               _lib.ptr(invstd), _lib.ptr(running_mean if training else None),
                                               _lib.ptr(running_var if training else None), B, C, H, W, int(bool(training)), int(bool(relu)),
                                               float(momentum), float(eps), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "h3d_batch_norm_forward")
    return y, mean, var, invstd


def _backward_nhwc(xv, yv, gv, weight, save_mean, save_invstd, training, relu, need):
    """One h3d_batch_norm_backward call on NHWC views -> (grad_x, grad_res [B,H,W,C], grad_weight, grad_bias [C]), None where `need` is
    false.  grad_res is produced only under ReLU (without it the skip's gradient is grad_y)."""
    B, H, W, C = xv.shape
    dev = xv.device
    gx = torch.empty(B, H, W, C, dtype=torch.float32, device=dev) if need[0] else None
    gr = torch.empty(B, H, W, C, dtype=torch.float32, device=dev) if need[1] and relu else None
    gw = torch.empty(C, dtype=torch.float32, device=dev) if need[2] else None
    gb = torch.empty(C, dtype=torch.float32, device=dev) if need[3] else None
    with torch.cuda.device(dev):
        ws = _workspace(dev, B, C, H, W)
        rc = _lib.lib().h3d_batch_norm_backward(_lib.ptr(xv), _cs(xv), _lib.ptr(yv if relu else None), _cs(yv) if relu else C, _lib.ptr(gv),
                                                _cs(gv), _lib.ptr(weight), _lib.ptr(save_mean), _lib.ptr(save_invstd), _lib.ptr(gx), C,
                                                _lib.ptr(gr), C, _lib.ptr(gw), _lib.ptr(gb), B, C, H, W, int(bool(training)), int(bool(relu)),
                                                _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "h3d_batch_norm_backward")
    return gx, gr, gw, gb


def _nchw(v):
    return None if v is None else v.permute(0, 3, 1, 2)


def batch_norm_forward(x, weight, bias, mean=None, var=None, training=True, running_mean=None, running_var=None, momentum=0.1,
                       eps=arch.BN_EPS, res=None, relu=False):
    """act(batch_norm(x) + res) of a float32 device tensor x [B,C,H,W] (C % 4 == 0) -> (y channels_last, save_mean, biased var,
    save_invstd).  training: the batch's statistics; running_mean / running_var (optional) are updated in place.  evaluation:
    `mean` / `var` are the statistics to use."""
    _check("batch_norm_forward: x", x)
    C = x.shape[1]
    for name, t in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)) + \
            (() if training else (("mean", mean), ("var", var))):
        if t is not None or name in ("weight", "bias", "mean", "var"):
            _check_vec("batch_norm_forward: " + name, t, C)
    if training and x.numel() // C == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    xv = _as_nhwc(x.detach(), "batch_norm_forward: x")
    resv = None
    if res is not None:
        _check("batch_norm_forward: res", res, x.shape)
        resv = _as_nhwc(res.detach(), "batch_norm_forward: res")
    y, m, v, i = _forward_nhwc(xv, weight.detach(), bias.detach(), resv, mean, var, running_mean, running_var, training, relu, momentum, eps)
    return _nchw(y), m, v, i


def batch_norm_backward(x, y, grad_y, weight, save_mean, save_invstd, training=True, relu=False, need=(True, True, True, True)):
    """The gradients of act(batch_norm(x) + res) for grad_y = dL/dy -> (grad_x, grad_res, grad_weight, grad_bias), None where `need` is
    false.  y (the saved output) is read only under ReLU, for the mask [y > 0]; without ReLU grad_res is the tensor grad_y itself."""
    _check("batch_norm_backward: x", x)
    _check("batch_norm_backward: grad_y", grad_y, x.shape)
    C = x.shape[1]
    for name, t in (("weight", weight), ("save_mean", save_mean), ("save_invstd", save_invstd)):
        _check_vec("batch_norm_backward: " + name, t, C)
    xv = _as_nhwc(x.detach(), "batch_norm_backward: x")
    gv = _as_nhwc(grad_y.detach(), "batch_norm_backward: grad_y")
    yv = None
    if relu:
        _check("batch_norm_backward: y", y, x.shape)
        yv = _as_nhwc(y.detach(), "batch_norm_backward: y")
    need = tuple(bool(n) for n in need)
    gx, gr, gw, gb = _backward_nhwc(xv, yv, gv, weight.detach(), save_mean, save_invstd, training, relu, need)
    return _nchw(gx), (_nchw(gr) if relu else grad_y) if need[1] else None, gw, gb


class _BatchNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, res, running_mean, running_var, training, momentum, eps, relu):
        xv = _as_nhwc(x, "batch_norm_autograd: x")
        resv = None if res is None else _as_nhwc(res, "batch_norm_autograd: res")
        y, mean, _, invstd = _forward_nhwc(xv, weight, bias, resv, running_mean, running_var, running_mean, running_var, training, relu,
                                           momentum, eps)
        y = _nchw(y)
        ctx.training, ctx.relu = training, relu
        ctx.save_for_backward(_nchw(xv), y if relu else None, weight, mean, invstd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, y, weight, mean, invstd = ctx.saved_tensors
        n = ctx.needs_input_grad
        need = (n[0], n[3], n[1], n[2])
        gx = gr = gw = gb = None
        if need[0] or need[2] or need[3] or (need[1] and ctx.relu):
            xv = _as_nhwc(x, "batch_norm_autograd: x")
            gv = _as_nhwc(grad_y, "batch_norm_autograd: grad_y")
            yv = _as_nhwc(y, "batch_norm_autograd: y") if ctx.relu else None
            gx, gr, gw, gb = _backward_nhwc(xv, yv, gv, weight, mean, invstd, ctx.training, ctx.relu, need)
        if need[1]:
            gr = _nchw(gr) if ctx.relu else grad_y
        return _nchw(gx), gw, gb, gr if need[1] else None, None, None, None, None, None, None


def batch_norm_autograd(x, weight, bias, running_mean, running_var, training, momentum=0.1, eps=arch.BN_EPS, res=None, relu=False):
    """act(F.batch_norm(x, running_mean, running_var, weight, bias, training, momentum, eps) + res): float32 device tensors x [B,C,H,W]
    (C % 4 == 0), weight / bias / running_mean / running_var [C], res [B,C,H,W] or None -> [B,C,H,W] in channels_last memory format,
    differentiable at x, weight, bias and res.  training: running_mean / running_var are updated in place (None: not kept)."""
    _check("batch_norm_autograd: x", x)
    C = x.shape[1]
    _check_vec("batch_norm_autograd: weight", weight, C)
    _check_vec("batch_norm_autograd: bias", bias, C)
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None or not training:
            if t is None:
                raise RuntimeError("batch_norm_autograd: %s is needed in evaluation mode" % name)
            _check_vec("batch_norm_autograd: " + name, t, C)
    if res is not None:
        _check("batch_norm_autograd: res", res, x.shape)
    if training and x.numel() // C == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    return _BatchNormFn.apply(x, weight, bias, res, running_mean, running_var, bool(training), float(momentum), float(eps), bool(relu))


class TrainableBatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d (same constructor, same state_dict keys; affine, a fixed momentum) on `batch_norm_autograd`, with the residual add
    and the ReLU that follow it in the reference as options of the call."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if not self.affine or self.momentum is None:
            raise ValueError("TrainableBatchNorm2d: affine=True and a numeric momentum only")

    def forward(self, input, res=None, relu=False):
        training = self.training or not self.track_running_stats
        if self.training and self.track_running_stats:
            self.num_batches_tracked.add_(1)
        return batch_norm_autograd(input, self.weight, self.bias, self.running_mean, self.running_var, training, self.momentum, self.eps,
                                   res, relu)
