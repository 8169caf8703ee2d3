"""Trainable plain convolutions (include/h3d.h section 2c, csrc/conv_bwd.hip): the operator of H3D_OP_CONV,

    y = act(conv2d(x, W, b) + res)          act = ReLU or the identity, groups = 1, BatchNorm folded into W, b

and its gradients at x, res, W and b.

    conv2d_backward(x, weight, y, grad_y, stride, padding, dilation, relu, need, general)
                                   one h3d_conv2d_backward call -> (grad_x, grad_res, grad_weight, grad_bias)
    conv2d_autograd(x, weight, bias, stride, padding, dilation, res, relu)
                                   the operator as ONE torch.autograd.Function: forward = the H3D_OP_CONV launch in the `f32` arithmetic on
                                   filters packed from the CURRENT parameter values (3x3 / 1x1, stride 1 / 2, padding k // 2, channels in
                                   multiples of 16), otherwise the general DeformConv operator with zero offsets and a unit mask; no vendor
                                   convolution either way.  backward = one h3d_conv2d_backward call.
    TrainableConv2d                nn.Conv2d's constructor and state_dict keys (groups = 1), forward(x, res=None, relu=False)
    TrainableBasicBlock            the reference's BasicBlock (models/model.py) with its BatchNorms folded: fine-tuning with frozen statistics

Memory format: a tensor in torch.channels_last memory format (or a channel slice of one: channel stride a multiple of 4, 16-byte
aligned) is used in place; anything else is relaid out through h3d_nchw_f32_to_nhwc.  Outputs and input gradients are channels_last, so
a chain of these functions and `heads_autograd` never relays out.

A Root (models/model.py:148-166: conv1x1 of the concatenated children, BatchNorm, + the first child if `residual`, ReLU) needs no class:

    root = TrainableConv2d(c1 + c2, cout, 1)              # weight / bias = the folded filters
    y = root(torch.cat((x1, x2), 1), res=x1 if residual else None, relu=True)
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib

_WORKSPACES = {}       # (device, geometry, flags) -> uint8 tensor


def _pair(v):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("expected an int or a pair, got %r" % (v,))
        return int(v[0]), int(v[1])
    return int(v), int(v)


def _cs(v):
    """Channel stride of an NHWC view [B,H,W,C] as `_as_nhwc` returns it."""
    B, H, W, C = v.shape
    return v.stride(2) if W > 1 else v.stride(1) if H > 1 else v.stride(0) if B > 1 else ((C + 3) // 4) * 4


def _as_nhwc(t, what):
    """float32 [B,C,H,W] -> an NHWC view [B,H,W,C] whose pixels are `cs` floats apart (cs >= C, a multiple of 4; 16-byte aligned): `t`'s
    own memory when it is channels_last (or a channel slice of such a tensor), a relaid-out copy otherwise."""
    if t.dim() != 4 or t.dtype != torch.float32:
        raise RuntimeError("%s must be float32 [B,C,H,W], got %s %s" % (what, t.dtype, tuple(t.shape)))
    B, C, H, W = t.shape
    v = t.permute(0, 2, 3, 1)
    cs = _cs(v)
    ok = (C == 1 or v.stride(3) == 1) and cs >= C and cs % 4 == 0 and t.data_ptr() % 16 == 0
    ok = ok and (W == 1 or v.stride(2) == cs) and (H == 1 or v.stride(1) == W * cs) and (B == 1 or v.stride(0) == H * W * cs)
    if ok:
        return v
    src = t.contiguous()
    cs = ((C + 3) // 4) * 4
    dst = torch.empty(B, H, W, cs, dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().h3d_nchw_f32_to_nhwc(_lib.ptr(src), _lib.ptr(dst), _lib.H3D_F32, B, C, H, W, cs, _lib.stream_ptr()), "h3d_nchw_f32_to_nhwc")
    return dst[..., :C]


def _geometry(x_shape, w_shape, stride, padding, dilation):
    """-> (B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw), Ho, Wo"""
    if len(x_shape) != 4 or len(w_shape) != 4:
        raise RuntimeError("conv2d: input must be [B,C,H,W] and weight [Cout,C,kh,kw]")
    B, C, H, W = x_shape
    Cout, Ck, kh, kw = w_shape
    if Ck != C:
        raise RuntimeError("conv2d: input has %d channels, the filters %d (groups = 1 only)" % (C, Ck))
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    if Ho <= 0 or Wo <= 0:
        raise RuntimeError("conv2d: the kernel does not fit the padded input %d x %d" % (H, W))
    return (B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw), Ho, Wo


def _workspace(dev, geo, flags):
    key = (str(dev), geo, flags)
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _lib.workspace(_lib.lib().h3d_conv2d_backward_workspace_bytes, *geo, flags, device=dev, min_bytes=256, what="conv2d_backward")
        _WORKSPACES[key] = ws
    return ws


def _backward_nhwc(xv, weight, yv, gv, geo, relu, need, general=False, workspace=None):
    """One h3d_conv2d_backward call on NHWC views -> (grad_x [B,H,W,C], grad_res [B,Ho,Wo,Cout], grad_weight, grad_bias) or None each."""
    B, C, H, W, Cout = geo[:5]
    Ho, Wo = gv.shape[1:3]
    dev = xv.device
    flags = _lib.CONV_BWD_RELU if relu else 0
    ws = _workspace(dev, geo, flags) if workspace is None else workspace
    weight = weight.detach().contiguous()
    gx = torch.empty(B, H, W, C, dtype=torch.float32, device=dev) if need[0] else None
    gres = torch.empty(B, Ho, Wo, Cout, dtype=torch.float32, device=dev) if need[1] else None
    gw = torch.empty_like(weight) if need[2] else None
    gb = torch.empty(Cout, dtype=torch.float32, device=dev) if need[3] else None
    L = _lib.lib()
    fn = L.h3d_conv2d_backward_general if general else L.h3d_conv2d_backward
    with torch.cuda.device(dev):
        rc = fn(_lib.ptr(xv), _cs(xv), _lib.ptr(weight), _lib.ptr(yv), 0 if yv is None else _cs(yv), _lib.ptr(gv), _cs(gv),
                _lib.ptr(gx), _lib.ptr(gres), _lib.ptr(gw), _lib.ptr(gb), *geo, flags, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "h3d_conv2d_backward")
    return gx, gres, gw, gb


def conv2d_backward(x, weight, y, grad_y, stride=1, padding=0, dilation=1, relu=False, need=(True,) * 4, general=False):
    """The gradients of y = act(conv2d(x, weight, b) + res) for grad_y = dL/dy: float32 tensors x [B,C,H,W], weight [Cout,C,kh,kw],
    y (the saved output; read only with relu=True, may be None otherwise) and grad_y [B,Cout,Ho,Wo] ->
    (grad_x [B,C,H,W], grad_res [B,Cout,Ho,Wo], grad_weight, grad_bias), None where `need` is false.  grad_x and grad_res are in
    torch.channels_last memory format.  `general`: the general kernels on the matrix-core configurations too."""
    _lib.require_cuda(x, weight, y, grad_y)
    if weight.dtype != torch.float32:
        raise RuntimeError("conv2d_backward: expected float32 tensors")
    geo, Ho, Wo = _geometry(tuple(x.shape), tuple(weight.shape), stride, padding, dilation)
    want = (geo[0], geo[4], Ho, Wo)
    if tuple(grad_y.shape) != want or (y is not None and tuple(y.shape) != want):
        raise RuntimeError("conv2d_backward: y / grad_y must be [B, Cout, Ho, Wo] = %s" % (want,))
    if relu and y is None:
        raise RuntimeError("conv2d_backward: relu=True needs the saved output y")
    xv = _as_nhwc(x.detach(), "conv2d_backward: x")
    yv = _as_nhwc(y.detach(), "conv2d_backward: y") if relu else None
    gv = _as_nhwc(grad_y.detach(), "conv2d_backward: grad_y")
    gx, gres, gw, gb = _backward_nhwc(xv, weight, yv, gv, geo, relu, tuple(bool(n) for n in need), general)
    return (None if gx is None else gx.permute(0, 3, 1, 2), None if gres is None else gres.permute(0, 3, 1, 2), gw, gb)


def _op_conv_takes(geo):
    B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw = geo
    return (kh == kw and kh in (1, 3) and sh == sw and sh in (1, 2) and ph == pw == kh // 2 and dh == dw == 1
            and C % 16 == 0 and Cout % 16 == 0)


def _forward_nhwc(xv, weight, bias, geo, Ho, Wo, resv, relu):
    """y = act(conv2d(x, W, b) + res) on NHWC views -> contiguous [B,Ho,Wo,Cout]."""
    B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw = geo
    dev = xv.device
    weight = weight.detach()
    bias = torch.zeros(Cout, dtype=torch.float32, device=dev) if bias is None else bias.detach()
    if _op_conv_takes(geo):
        rows = ((Cout + 127) // 128) * 128
        wp = torch.zeros(rows, kh * kw, C, dtype=torch.float32, device=dev)          # [rows][taps][Cin], zero beyond Cout (weights._bank)
        wp[:Cout] = weight.permute(0, 2, 3, 1).reshape(Cout, kh * kw, C)
        bp = torch.zeros(rows, dtype=torch.float32, device=dev)
        bp[:Cout] = bias
        out = torch.empty(B, Ho, Wo, Cout, dtype=torch.float32, device=dev)
        op = _lib.H3dOp()
        op.kind, op.dtype = _lib.OP_CONV, _lib.H3D_F32
        op.in_, op.w, op.bias, op.out = xv.data_ptr(), wp.data_ptr(), bp.data_ptr(), out.data_ptr()
        op.B, op.H, op.W, op.Cin, op.in_cs = B, H, W, C, _cs(xv)
        op.Ho, op.Wo, op.Cout, op.out_cs = Ho, Wo, Cout, Cout
        op.ksize, op.stride, op.relu, op.out_mode, op.wrows = kh, sh, int(relu), _lib.OUT_NHWC, rows
        if resv is not None:
            op.in2, op.in2_cs = resv.data_ptr(), _cs(resv)
        arr = (_lib.H3dOp * 1)(op)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().h3d_run_ops(arr, 1, _lib.stream_ptr()), "h3d_run_ops")
        return out
    from .dcn_v2 import dcn_v2_forward
    zero = torch.zeros(B, 2 * kh * kw, Ho, Wo, dtype=torch.float32, device=dev)
    one = torch.ones(B, kh * kw, Ho, Wo, dtype=torch.float32, device=dev)
    y = dcn_v2_forward(xv.permute(0, 3, 1, 2).contiguous(), weight.contiguous(), bias.contiguous(), zero, one,
                       kh, kw, sh, sw, ph, pw, dh, dw, 1).permute(0, 2, 3, 1)
    if resv is not None:
        y = y + resv
    if relu:
        y = torch.relu(y)
    return y.contiguous()


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, dilation, res, relu):
        geo, Ho, Wo = _geometry(tuple(x.shape), tuple(weight.shape), stride, padding, dilation)
        xv = _as_nhwc(x, "conv2d_autograd: x")
        resv = None
        if res is not None:
            if tuple(res.shape) != (geo[0], geo[4], Ho, Wo):
                raise RuntimeError("conv2d_autograd: res must be [B, Cout, Ho, Wo] = %s, got %s" % ((geo[0], geo[4], Ho, Wo), tuple(res.shape)))
            resv = _as_nhwc(res, "conv2d_autograd: res")
        y = _forward_nhwc(xv, weight, bias, geo, Ho, Wo, resv, relu).permute(0, 3, 1, 2)
        ctx.geo, ctx.relu = geo, bool(relu)
        ctx.save_for_backward(xv.permute(0, 3, 1, 2), weight, y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, weight, y = ctx.saved_tensors
        n = ctx.needs_input_grad
        need = (n[0], n[6], n[1], n[2])
        xv = _as_nhwc(x, "conv2d_autograd: x")
        yv = _as_nhwc(y, "conv2d_autograd: y") if ctx.relu else None
        gv = _as_nhwc(grad_y, "conv2d_autograd: grad_y")
        gx, gres, gw, gb = _backward_nhwc(xv, weight, yv, gv, ctx.geo, ctx.relu, need)
        return (None if gx is None else gx.permute(0, 3, 1, 2), gw, gb, None, None, None,
                None if gres is None else gres.permute(0, 3, 1, 2), None)


def conv2d_autograd(x, weight, bias=None, stride=1, padding=0, dilation=1, res=None, relu=False):
    """y = act(conv2d(x, weight, bias) + res), differentiable at x, weight, bias and res.  float32 device tensors: x [B,C,H,W],
    weight [Cout,C,kh,kw], bias [Cout] or None, res [B,Cout,Ho,Wo] or None -> y [B,Cout,Ho,Wo] in torch.channels_last memory format."""
    _lib.require_cuda(x, weight, bias, res)
    for t in (x, weight, bias, res):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("conv2d_autograd: expected float32 tensors, got %s" % (t.dtype,))
    return _Conv2dFn.apply(x, weight, bias, stride, padding, dilation, res, relu)


class TrainableConv2d(nn.Conv2d):
    """nn.Conv2d (same constructor, same state_dict keys; groups = 1, zero padding) on `conv2d_autograd`, with the residual add and
    the ReLU of H3D_OP_CONV as options of the call."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.groups != 1:
            raise ValueError("TrainableConv2d: groups = %d is not implemented (groups = 1 only)" % self.groups)
        if self.padding_mode != "zeros" or isinstance(self.padding, str):
            raise ValueError("TrainableConv2d: zero padding given as numbers only")

    def forward(self, input, res=None, relu=False):
        return conv2d_autograd(input, self.weight, self.bias, self.stride, self.padding, self.dilation, res, relu)


class TrainableBasicBlock(nn.Module):
    """The reference's BasicBlock (models/model.py:32-60): conv3x3(stride) -> BN -> ReLU -> conv3x3 -> BN, + residual, ReLU, built from
    the reference state_dict entries `prefix + {conv1,bn1,conv2,bn2}.*`.  The BatchNorms are folded into the filters
    (engine.PackedWeights._fold) and the folded filters and biases are the parameters: fine-tuning with frozen statistics."""

    def __init__(self, state_dict, prefix, stride=1):
        super().__init__()
        from .weights import PackedWeights
        sub = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix) and not k.endswith("num_batches_tracked")}
        pw = PackedWeights.from_tensors(sub, "f32", "cpu")
        for i in (1, 2):
            w, b = pw._fold(pw.sd["conv%d.weight" % i], pw.sd.get("conv%d.bias" % i), "bn%d" % i)
            if tuple(w.shape[2:]) != (3, 3):
                raise ValueError("TrainableBasicBlock: %sconv%d is not a 3x3 convolution" % (prefix, i))
            self.register_parameter("weight%d" % i, nn.Parameter(w.contiguous()))
            self.register_parameter("bias%d" % i, nn.Parameter(b.contiguous()))
        self.stride = int(stride)

    def forward(self, x, residual=None):
        if residual is None:
            residual = x
        h = conv2d_autograd(x, self.weight1, self.bias1, self.stride, 1, 1, None, True)
        return conv2d_autograd(h, self.weight2, self.bias2, 1, 1, 1, residual, True)
