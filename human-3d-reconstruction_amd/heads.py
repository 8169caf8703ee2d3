"""Trainable output heads on a frozen backbone (include/h3d.h section 2b, csrc/heads_bwd.hip).

    heads_autograd(feat, params)   the heads `Conv3x3(64 -> head_conv) + ReLU + Conv1x1(-> C)` (reference models/model.py:451-464,
                                   485-489) of a [B,64,H,W] feature map as ONE torch.autograd.Function: forward = the fused
                                   H3D_OP_HEADS launch in the `f32` arithmetic on filters packed from the CURRENT parameter values,
                                   backward = one h3d_heads_backward call.
    TrainableHeads(model)          a DLASeg whose backbone runs frozen (folded BatchNorm, no_grad) through the engine's plan and whose
                                   heads are trained: forward(x) -> [{head: [B,C,H/4,W/4]}], the input of loss_multi_pose /
                                   loss_obj_detection / smpl.lbs_from_heads.
"""
import ctypes

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from .engine import DLAEngine, heads_k_perm, pack_head_1x1, pack_head_3x3

_WORKSPACES = {}       # (device, B, H, W, head_conv, channels of the heads) -> uint8 tensor


def _workspace(dev, B, H, W, hc, chans):
    key = (str(dev), B, H, W, hc, tuple(chans))
    ws = _WORKSPACES.get(key)
    if ws is None:
        carr = (ctypes.c_int * max(len(chans), 1))(*chans)
        ws = _lib.workspace(_lib.lib().h3d_heads_backward_workspace_bytes, B, H, W, hc, len(chans), carr, device=dev, min_bytes=256)
        _WORKSPACES[key] = ws
    return ws


def heads_ops(feat_nhwc, params):
    """The plan's H3D_OP_HEADS launches (`f32` arithmetic, one per group of heads with the same number of 32-row output tiles) for
    {head: (w1, b1, w2, b2)} on the NHWC fp32 map `feat_nhwc` [B,H,W,>=64 (channel stride)], filters packed from the values the
    parameters hold now -> (h3d_op array, {head: [B,C,H,W] fp32 output}, the tensors the ops point into)."""
    B, H, W = feat_nhwc.shape[:3]
    dev = feat_nhwc.device
    names = list(params)
    hc = params[names[0]][0].shape[0]
    perm = heads_k_perm(hc)
    groups = {}
    for head in names:
        groups.setdefault((params[head][2].shape[0] + 31) // 32, []).append(head)
    outs, keep = {}, []
    ops = []
    for m2 in sorted(groups):
        g = groups[m2]
        w1 = torch.cat([pack_head_3x3(params[h][0]) for h in g]).contiguous()
        b1 = torch.cat([params[h][1] for h in g]).float().contiguous()
        desc = _lib.H3dHeadsDesc()
        desc.nheads = len(g)
        for i, h in enumerate(g):
            w2, b2 = pack_head_1x1(params[h][2], params[h][3], perm)
            c = params[h][2].shape[0]
            o = torch.empty(B, c, H, W, dtype=torch.float32, device=dev)
            outs[h] = o
            keep += [w2, b2]
            desc.head[i].w2, desc.head[i].b2, desc.head[i].out, desc.head[i].C = w2.data_ptr(), b2.data_ptr(), o.data_ptr(), c
        keep += [w1, b1, desc]
        op = _lib.H3dOp()
        op.kind, op.dtype, op.B = _lib.OP_HEADS, _lib.H3D_F32, B
        op.in_, op.in2, op.w, op.bias = feat_nhwc.data_ptr(), ctypes.addressof(desc), w1.data_ptr(), b1.data_ptr()
        op.H, op.W, op.Cin, op.in_cs, op.Ho, op.Wo, op.Cout, op.ksize, op.stride = H, W, 64, feat_nhwc.stride(2), H, W, hc, 3, 1
        ops.append(op)
    return (_lib.H3dOp * len(ops))(*ops), {h: outs[h] for h in names}, keep


def heads_forward(feat_nhwc, params):
    """`heads_ops`, launched on the current stream -> {head: [B,C,H,W] fp32}."""
    arr, outs, keep = heads_ops(feat_nhwc, params)
    with torch.cuda.device(feat_nhwc.device):
        _lib.check(_lib.lib().h3d_run_ops(arr, len(arr), _lib.stream_ptr()), "h3d_run_ops")
    return outs


class H3dHeadsBwdHead(ctypes.Structure):
    """Mirror of `struct h3d_heads_bwd_head` in include/h3d.h."""
    _fields_ = [("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("grad_out", ctypes.c_void_p),
                ("grad_w1", ctypes.c_void_p), ("grad_b1", ctypes.c_void_p), ("grad_w2", ctypes.c_void_p), ("grad_b2", ctypes.c_void_p),
                ("C", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def heads_backward(feat_nhwc, heads, want_feat=True, workspace=None):
    """One h3d_heads_backward call.  `heads`: list of (w1, b1, w2, grad_out or None, (want_w1, want_b1, want_w2, want_b2)) in the
    reference's layouts -> (grad_feat [B,H,W,64] or None, [per head (gw1, gb1, gw2, gb2), None where not requested or skipped])."""
    _lib.require_cuda(feat_nhwc)
    B, H, W = feat_nhwc.shape[:3]
    dev = feat_nhwc.device
    hc = heads[0][0].shape[0]
    chans = [h[2].shape[0] for h in heads]
    ws = _workspace(dev, B, H, W, hc, chans) if workspace is None else workspace
    arr = (H3dHeadsBwdHead * len(heads))()
    grads, keep = [], []
    for i, (w1, b1, w2, go, want) in enumerate(heads):
        w1, b1, w2 = w1.detach().contiguous(), b1.detach().contiguous(), w2.detach().contiguous()
        keep += [w1, b1, w2]
        arr[i].w1, arr[i].b1, arr[i].w2, arr[i].C = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), chans[i]
        g = [None] * 4
        if go is not None:
            if go.dtype != torch.float32 or tuple(go.shape) != (B, chans[i], H, W):
                raise RuntimeError("heads_backward: grad_out of head %d must be float32 %s, got %s %s"
                                   % (i, (B, chans[i], H, W), go.dtype, tuple(go.shape)))
            go = go.contiguous()
            keep.append(go)
            arr[i].grad_out = go.data_ptr()
            for j, src in enumerate((w1, b1, w2, None)):
                if want[j]:
                    g[j] = torch.empty(chans[i], dtype=torch.float32, device=dev) if src is None else torch.empty_like(src)
            arr[i].grad_w1, arr[i].grad_b1, arr[i].grad_w2, arr[i].grad_b2 = [0 if t is None else t.data_ptr() for t in g]
        grads.append(tuple(g))
    gfeat = torch.empty(B, H, W, 64, dtype=torch.float32, device=dev) if want_feat else None
    with torch.cuda.device(dev):
        rc = _lib.lib().h3d_heads_backward(feat_nhwc.data_ptr(), feat_nhwc.stride(2), B, H, W, hc, len(heads), arr, _lib.ptr(gfeat),
                                           ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "h3d_heads_backward")
    return gfeat, grads


def _nhwc(feat):
    if feat.dim() != 4 or feat.shape[1] != 64 or feat.dtype != torch.float32:
        raise RuntimeError("heads_autograd: feat must be float32 [B,64,H,W], got %s %s" % (feat.dtype, tuple(feat.shape)))
    v = feat.permute(0, 2, 3, 1)
    if not v.is_contiguous():
        raise RuntimeError("heads_autograd: feat must be in torch.channels_last memory format")
    return v


class _HeadsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, names, *flat):
        params = {h: tuple(flat[4 * i:4 * i + 4]) for i, h in enumerate(names)}
        outs = heads_forward(_nhwc(feat), params)
        ctx.names = names
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(feat, *flat)
        return tuple(outs[h] for h in names)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gouts):
        feat, flat = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        need = ctx.needs_input_grad
        heads = []
        for i in range(len(ctx.names)):
            w1, b1, w2 = flat[4 * i], flat[4 * i + 1], flat[4 * i + 2]
            heads.append((w1, b1, w2.reshape(w2.shape[0], -1), gouts[i], tuple(need[2 + 4 * i + j] for j in range(4))))
        gfeat, grads = heads_backward(_nhwc(feat), heads, want_feat=need[0])
        flat_g = []
        for i, g in enumerate(grads):
            gw1, gb1, gw2, gb2 = g
            flat_g += [gw1, gb1, None if gw2 is None else gw2.reshape(flat[4 * i + 2].shape), gb2]
        return (None if gfeat is None else gfeat.permute(0, 3, 1, 2), None) + tuple(flat_g)


def heads_autograd(feat, params):
    """feat [B,64,H,W] fp32 in torch.channels_last memory format, params {head: (w1 [head_conv,64,3,3], b1, w2 [C,head_conv(,1,1)], b2)}
    -> {head: [B,C,H,W] fp32}, differentiable at the parameters and at `feat`."""
    flat = []
    for h, p in params.items():
        if len(p) != 4:
            raise ValueError("heads_autograd: head %r needs (w1, b1, w2, b2)" % (h,))
        flat += list(p)
    _lib.require_cuda(feat, *flat)
    names = tuple(params)
    outs = _HeadsFn.apply(feat, names, *flat)
    return dict(zip(names, outs))


class TrainableHeads(nn.Module):
    """`model`'s heads as trainable parameters on `model`'s frozen backbone.  The head parameters are the model's own nn.Parameters
    under their reference state_dict names (`hm.0.weight`, ...): `parameters()` yields only them, `state_dict()` /
    `load_state_dict()` are the wrapped model's, so checkpoint.save_model / load_model work on either object."""

    DTYPES = ("f32", "f16x3")

    def __init__(self, model):
        super().__init__()
        if model.compute_dtype not in self.DTYPES:
            raise ValueError("TrainableHeads: the backbone must run in 'f32' or 'f16x3' (fp32 feature map), not %r" % (model.compute_dtype,))
        if getattr(model, "arch_name", "") != "dla34" or model.head_conv <= 0:
            raise ValueError("TrainableHeads: a DLASeg with head_conv > 0 is required")
        object.__setattr__(self, "_model", model)        # (not a sub-module: its backbone stays out of parameters())
        for head in model.heads:
            self.add_module(head, model._modules[head])
        self._backbone = None

    @property
    def model(self):
        return self._model

    def state_dict(self, *a, **kw):
        return self._model.state_dict(*a, **kw)

    def load_state_dict(self, *a, **kw):
        self._backbone = None
        return self._model.load_state_dict(*a, **kw)

    def _apply(self, fn, *a, **kw):
        self._backbone = None
        self._model._apply(fn, *a, **kw)
        return self

    def head_params(self):
        return {h: (self._modules[h]._modules["0"].weight, self._modules[h]._modules["0"].bias,
                    self._modules[h]._modules["2"].weight, self._modules[h]._modules["2"].bias) for h in self._model.heads}

    def backbone(self, device):
        if self._backbone is None or self._backbone.device != torch.device(device):
            m = self._model
            eng = DLAEngine(m.state_dict(), m.heads, m.use_dcn, m.compute_dtype, device, m.head_conv, m.arch_name)
            eng.lower_heads = False
            self._backbone = eng
        return self._backbone

    def features(self, x):
        """The frozen backbone's [B,64,H/4,W/4] fp32 map (channels_last), copied out of the plan's buffer."""
        if not x.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        with torch.no_grad():
            eng = self.backbone(x.device)
            eng.forward(x)
            v = eng.plan(x.shape[0], x.shape[2], x.shape[3]).feat
            feat = v.buf[..., v.coff:v.coff + 64].float().contiguous()
            if feat.data_ptr() == v.buf.data_ptr():
                feat = feat.clone()
        return feat.permute(0, 3, 1, 2)

    def forward(self, x):
        return [heads_autograd(self.features(x), self.head_params())]
