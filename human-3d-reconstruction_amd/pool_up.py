"""Trainable max-pool and up-sample + add (include/h3d.h section 2d, csrc/pool_up_bwd.hip): the two operators of DLA-34 next to the
convolutions, as H3D_OP_MAXPOOL / H3D_OP_UPADD run them, and their gradients.

    max_pool2_backward(x, grad_y)            one h3d_maxpool2_backward call -> grad_x
    upsample_backward(x, weight, grad_y, f, need)
                                             one h3d_upsample_backward call -> (grad_x, grad_weight [C,1,2f,2f])
    max_pool2_autograd(x)                    nn.MaxPool2d(2, 2) (models/model.py:201) as ONE torch.autograd.Function
    up_add_autograd(x, weight, skip, f)      skip + ConvTranspose2d(C, C, 2f, stride=f, padding=f//2, groups=C, bias=False)(x)
                                             (IDAUp.forward, models/model.py:384-390) as ONE torch.autograd.Function; the skip's gradient
                                             is grad_y itself, passed on without a copy

Forward = the `f32` launch of the inference op through h3d_run_ops, the tap-major weight image packed from the CURRENT parameter values.
Memory format: `conv._as_nhwc`'s rules -- channels_last tensors (or channel slices of them) are used in place, outputs and input
gradients are channels_last, so a chain of these functions and `conv2d_autograd` never relays out.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .conv import _as_nhwc, _cs

_WORKSPACES = {}       # (device, B, C, H, W, f) -> uint8 tensor


def _check(what, x):
    _lib.require_cuda(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise RuntimeError("%s must be float32 [B,C,H,W], got %s %s" % (what, x.dtype, tuple(x.shape)))
    if x.shape[1] % 4:
        raise RuntimeError("%s: %d channels (a multiple of 4 is required)" % (what, x.shape[1]))


def _workspace(dev, B, C, H, W, f):
    key = (str(dev), B, C, H, W, f)
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _lib.workspace(_lib.lib().h3d_upsample_backward_workspace_bytes, B, C, H, W, f, device=dev, min_bytes=256, what="upsample_backward")
        _WORKSPACES[key] = ws
    return ws


def _run_op(op, dev):
    arr = (_lib.H3dOp * 1)(op)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().h3d_run_ops(arr, 1, _lib.stream_ptr()), "h3d_run_ops")


def pack_up_weight(weight):
    """The reference's [C,1,k,k] parameter -> H3D_OP_UPADD's tap-major fp32 image [k*k][C] (weights.PackedWeights.up)."""
    c, one, k, k2 = weight.shape
    if one != 1 or k != k2:
        raise RuntimeError("up-sample weight must be [C,1,k,k], got %s" % (tuple(weight.shape),))
    return weight.detach().reshape(c, k * k).t().contiguous()


# ---- max-pool ----------------------------------------------------------------------------------------------------------------------------
def _pool_forward_nhwc(xv):
    B, H, W, C = xv.shape
    Ho, Wo = H // 2, W // 2
    out = torch.empty(B, Ho, Wo, C, dtype=torch.float32, device=xv.device)
    if out.numel() == 0:
        return out
    op = _lib.H3dOp()
    op.kind, op.dtype = _lib.OP_MAXPOOL, _lib.H3D_F32
    op.in_, op.out = xv.data_ptr(), out.data_ptr()
    op.B, op.H, op.W, op.Cin, op.in_cs = B, H, W, C, _cs(xv)
    op.Ho, op.Wo, op.Cout, op.out_cs = Ho, Wo, C, C
    op.ksize, op.stride, op.out_mode = 2, 2, _lib.OUT_NHWC
    _run_op(op, xv.device)
    return out


def _pool_backward_nhwc(xv, gv):
    B, H, W, C = xv.shape
    gx = torch.empty(B, H, W, C, dtype=torch.float32, device=xv.device)
    with torch.cuda.device(xv.device):
        rc = _lib.lib().h3d_maxpool2_backward(_lib.ptr(xv), _cs(xv), _lib.ptr(gv) if gv.numel() else None, _cs(gv) if gv.numel() else C,
                                              _lib.ptr(gx), C, B, C, H, W, _lib.stream_ptr())
    _lib.check(rc, "h3d_maxpool2_backward")
    return gx


def max_pool2_backward(x, grad_y):
    """The gradient of F.max_pool2d(x, 2, 2) for grad_y = dL/dy: float32 x [B,C,H,W], grad_y [B,C,H//2,W//2] -> grad_x [B,C,H,W]
    (channels_last).  Ties go to the first maximum of a window in the order (0,0), (0,1), (1,0), (1,1): torch's CPU rule."""
    _check("max_pool2_backward: x", x)
    _check("max_pool2_backward: grad_y", grad_y)
    B, C, H, W = x.shape
    if tuple(grad_y.shape) != (B, C, H // 2, W // 2):
        raise RuntimeError("max_pool2_backward: grad_y must be %s, got %s" % ((B, C, H // 2, W // 2), tuple(grad_y.shape)))
    xv = _as_nhwc(x.detach(), "max_pool2_backward: x")
    gv = _as_nhwc(grad_y.detach(), "max_pool2_backward: grad_y") if grad_y.numel() else grad_y.detach().permute(0, 2, 3, 1)
    return _pool_backward_nhwc(xv, gv).permute(0, 3, 1, 2)


class _MaxPool2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xv = _as_nhwc(x, "max_pool2_autograd: x")
        ctx.save_for_backward(xv.permute(0, 3, 1, 2))
        return _pool_forward_nhwc(xv).permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        if not ctx.needs_input_grad[0]:
            return None
        x, = ctx.saved_tensors
        xv = _as_nhwc(x, "max_pool2_autograd: x")
        gv = _as_nhwc(grad_y, "max_pool2_autograd: grad_y") if grad_y.numel() else grad_y.permute(0, 2, 3, 1)
        return _pool_backward_nhwc(xv, gv).permute(0, 3, 1, 2)


def max_pool2_autograd(x):
    """F.max_pool2d(x, 2, 2) of a float32 device tensor [B,C,H,W] (C % 4 == 0) -> [B,C,H//2,W//2] in channels_last memory format,
    differentiable at x."""
    _check("max_pool2_autograd: x", x)
    return _MaxPool2Fn.apply(x)


# ---- up-sample + add -----------------------------------------------------------------------------------------------------------------------
def _up_geometry(what, x, weight, f):
    f = int(f)
    if f not in (2, 4, 8):
        raise RuntimeError("%s: f = %d (2, 4 or 8)" % (what, f))
    if tuple(weight.shape) != (x.shape[1], 1, 2 * f, 2 * f) or weight.dtype != torch.float32:
        raise RuntimeError("%s: weight must be float32 %s, got %s %s" % (what, (x.shape[1], 1, 2 * f, 2 * f), weight.dtype, tuple(weight.shape)))
    return f


def _up_forward_nhwc(xv, wp, sv, f):
    B, H, W, C = xv.shape
    out = torch.empty(B, H * f, W * f, C, dtype=torch.float32, device=xv.device)
    op = _lib.H3dOp()
    op.kind, op.dtype = _lib.OP_UPADD, _lib.H3D_F32
    op.in_, op.in2, op.w, op.out = xv.data_ptr(), sv.data_ptr(), wp.data_ptr(), out.data_ptr()
    op.B, op.H, op.W, op.Cin, op.in_cs, op.in2_cs = B, H, W, C, _cs(xv), _cs(sv)
    op.Ho, op.Wo, op.Cout, op.out_cs = H * f, W * f, C, C
    op.ksize, op.stride, op.out_mode = 2 * f, f, _lib.OUT_NHWC
    _run_op(op, xv.device)
    return out


def _up_backward_nhwc(xv, wp, gv, f, need, workspace=None):
    """One h3d_upsample_backward call on NHWC views -> (grad_x [B,H,W,C], grad_w tap-major [k*k][C]) or None each."""
    B, H, W, C = xv.shape
    dev = xv.device
    gx = torch.empty(B, H, W, C, dtype=torch.float32, device=dev) if need[0] else None
    gw = torch.empty(4 * f * f, C, dtype=torch.float32, device=dev) if need[1] else None
    ws = None
    if need[1]:
        ws = _workspace(dev, B, C, H, W, f) if workspace is None else workspace
    with torch.cuda.device(dev):
        rc = _lib.lib().h3d_upsample_backward(_lib.ptr(xv), _cs(xv), _lib.ptr(wp), _lib.ptr(gv), _cs(gv), _lib.ptr(gx), C, _lib.ptr(gw),
                                              B, C, H, W, f, _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "h3d_upsample_backward")
    return gx, gw


def _unpack_up_grad(gw, f):
    return None if gw is None else gw.t().reshape(gw.shape[1], 1, 2 * f, 2 * f)


def upsample_backward(x, weight, grad_y, f, need=(True, True)):
    """The gradients of skip + conv_transpose2d(x, weight, stride=f, padding=f//2, groups=C) at x and weight for grad_y = dL/dy:
    float32 x [B,C,H,W], weight [C,1,2f,2f], grad_y [B,C,H f,W f] -> (grad_x [B,C,H,W] channels_last, grad_weight [C,1,2f,2f]), None where
    `need` is false.  (The skip's gradient is grad_y.)"""
    _check("upsample_backward: x", x)
    _check("upsample_backward: grad_y", grad_y)
    _lib.require_cuda(weight)
    f = _up_geometry("upsample_backward", x, weight, f)
    B, C, H, W = x.shape
    if tuple(grad_y.shape) != (B, C, H * f, W * f):
        raise RuntimeError("upsample_backward: grad_y must be %s, got %s" % ((B, C, H * f, W * f), tuple(grad_y.shape)))
    xv = _as_nhwc(x.detach(), "upsample_backward: x")
    gv = _as_nhwc(grad_y.detach(), "upsample_backward: grad_y")
    gx, gw = _up_backward_nhwc(xv, pack_up_weight(weight), gv, f, tuple(bool(n) for n in need))
    return None if gx is None else gx.permute(0, 3, 1, 2), _unpack_up_grad(gw, f)


class _UpAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, skip, f):
        xv = _as_nhwc(x, "up_add_autograd: x")
        sv = _as_nhwc(skip, "up_add_autograd: skip")
        y = _up_forward_nhwc(xv, pack_up_weight(weight), sv, f).permute(0, 3, 1, 2)
        ctx.f = f
        ctx.save_for_backward(xv.permute(0, 3, 1, 2), weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        n = ctx.needs_input_grad
        gx = gw = None
        if n[0] or n[1]:
            xv = _as_nhwc(x, "up_add_autograd: x")
            gv = _as_nhwc(grad_y, "up_add_autograd: grad_y")
            gx, gw = _up_backward_nhwc(xv, pack_up_weight(weight), gv, ctx.f, (n[0], n[1]))
        return (None if gx is None else gx.permute(0, 3, 1, 2), _unpack_up_grad(gw, ctx.f), grad_y if n[2] else None, None)


def up_add_autograd(x, weight, skip, f):
    """skip + conv_transpose2d(x, weight, stride=f, padding=f//2, groups=C): float32 device tensors x [B,C,H,W], weight [C,1,2f,2f],
    skip [B,C,H f,W f] (C % 4 == 0, f in 2, 4, 8) -> [B,C,H f,W f] in channels_last memory format, differentiable at all three."""
    _check("up_add_autograd: x", x)
    _check("up_add_autograd: skip", skip)
    _lib.require_cuda(weight)
    f = _up_geometry("up_add_autograd", x, weight, f)
    B, C, H, W = x.shape
    if tuple(skip.shape) != (B, C, H * f, W * f):
        raise RuntimeError("up_add_autograd: skip must be %s, got %s" % ((B, C, H * f, W * f), tuple(skip.shape)))
    return _UpAddFn.apply(x, weight, skip, f)
