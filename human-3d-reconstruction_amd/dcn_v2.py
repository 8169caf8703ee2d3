"""Host mirror of the reference's models/DCNv2/dcn_v2.py (forward path): `dcn_v2_forward`
(the `_ext` entry point, DCNv2/src/dcn_v2.h:9-39), `dcn_v2_conv`, `DCNv2`, `DCN` with the same
constructor arguments and state_dict keys (weight, bias, conv_offset_mask.{weight,bias}); and the
deformable PS-ROI pooling forward: `dcn_v2_psroi_pooling_forward` (the `_ext` entry point,
DCNv2/src/dcn_v2.h:76-107), `dcn_v2_pooling`, `DCNv2Pooling`, `DCNPooling` (state_dict keys
offset_mask_fc.{0,2,4}.{weight,bias}).

`dcn_v2_conv`, `DCNv2`, `DCN` and the pooling classes are inference only -- an INPUT that requires grad (with autograd enabled)
raises; parameters may require grad (the nn.Parameter default), results are computed without a graph and returned detached.

Training is opt-in: `dcn_v2_backward` (the `_ext` entry point, DCNv2/src/dcn_v2.h:41-74; kernels: csrc/dcn_bwd.hip), the autograd
function `_DCNv2` / `dcn_v2_conv_autograd` (dcn_v2.py:16-51) and the modules `TrainableDCNv2` / `TrainableDCN` (same constructors and
state_dict keys as `DCNv2` / `DCN`; their forward builds a graph); and for the pooling `dcn_v2_psroi_pooling_backward` (the `_ext` entry
point, DCNv2/src/dcn_v2.h:109-142; kernels: csrc/psroi_bwd.hip), the autograd function `_DCNv2Pooling` / `dcn_v2_pooling_autograd`
(dcn_v2.py:132-187) and the modules `TrainableDCNv2Pooling` / `TrainableDCNPooling` (same constructors and state_dict keys as
`DCNv2Pooling` / `DCNPooling`)."""
import math

import os

import torch
from torch import nn
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from . import _lib


_PACKED = {}          # (weight ptr, bias ptr, shape, dtype, device) -> (packed filter image, 16-byte device state of its validation)
_PACKED_MAX = 64


# fp32 tensors in the model's configuration: False (default since round 5) = three fp16 MFMAs on split operands per fp32 product
# (H3D_F16X3: 2^-22 relative per product, fp32 accumulation, ~2x the rate), True = exact fmaf chains on the fp32 matrix instruction
# (H3D_DCN_F32_MFMA; the environment variable H3D_DCN_OP_F32=1 selects the same for every entry point of the library)
OP_F32_MFMA = os.environ.get("H3D_DCN_OP_F32", "") not in ("", "0")

def _packed_weights(weight, bias, dtype):
    """The operator's filters in the kernels' layout, KEPT across calls and validated on the device at every call
    (`h3d_dcn_v2_pack_weights_cached`): the bytes of `weight` and `bias` are hashed on the current stream and the pack kernel runs
    only when the hash differs from the one the image was built from -- no host synchronisation.  Neither `tensor._version` (an
    edit through `.data`, as the reference does in dcn_v2.py:80-81 and DCNv2/test.py:21, does not bump it) nor the address (it can
    be reused) is taken as proof that the filters are unchanged; the host key only finds the buffer.  All of it is stream ordered
    on the stream that OWNS the entry (the stream of the call that created it): the 16-byte validation state is one accumulator, so
    two streams hashing the same layer at once would add into it together (spurious re-packs into a buffer another stream is still
    reading).  A call on any other stream therefore does not touch the cached image: it packs into a buffer of its own
    (`h3d_dcn_v2_pack_weights`, the reference contract's per-call work) -- correct on every stream, cached on one.  The cache holds
    no reference to the parameters.  Call with the tensor's device current (`dcn_v2_forward` does)."""
    key = (weight.data_ptr(), bias.data_ptr(), tuple(weight.shape), dtype, str(weight.device))
    Cout, C = weight.shape[0], weight.shape[1]
    L = _lib.lib()
    stream = torch.cuda.current_stream(weight.device).cuda_stream
    ent = _PACKED.pop(key, None)
    if ent is not None and ent[2] != stream:
        _PACKED[key] = ent
        n = int(L.h3d_dcn_v2_packed_weight_bytes(Cout, C, dtype))
        own = torch.empty(n, dtype=torch.uint8, device=weight.device)
        _lib.check(L.h3d_dcn_v2_pack_weights(_lib.ptr(weight), _lib.ptr(bias), Cout, C, dtype, _lib.ptr(own), _lib.stream_ptr()),
                   "dcn_v2_pack_weights")
        return own
    if ent is None:
        n = int(L.h3d_dcn_v2_packed_weight_bytes(Cout, C, dtype))
        ent = (torch.empty(n, dtype=torch.uint8, device=weight.device), torch.zeros(2, dtype=torch.int64, device=weight.device), stream)
        while len(_PACKED) >= _PACKED_MAX:
            _PACKED.pop(next(iter(_PACKED)))
    _PACKED[key] = ent                                     # (re-inserted: most recently used last)
    _lib.check(L.h3d_dcn_v2_pack_weights_cached(_lib.ptr(weight), _lib.ptr(bias), Cout, C, dtype, _lib.ptr(ent[0]), _lib.ptr(ent[1]),
                                                _lib.stream_ptr()), "dcn_v2_pack_weights_cached")
    return ent[0]


def _dcn_operands(what, input, weight, bias, offset, mask, geo):
    """The shape checks dcn_v2_forward and dcn_v2_backward share (the reference's messages, dcn_v2_cuda.cu:60-66) -> (B, C, H, W, Cout, Ho, Wo)."""
    kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group = geo
    if input.dim() != 4 or weight.dim() != 4:
        raise RuntimeError("%s: input must be [B,C,H,W] and weight [Cout,C,kh,kw]" % what)
    B, C, H, W = input.shape
    Cout, Ck, kh_, kw_ = weight.shape
    if kh_ != kernel_h or kw_ != kernel_w:
        raise RuntimeError("Input shape and kernel shape wont match: (%d x %d vs %d x %d)."
                           % (kernel_h, kernel_w, kh_, kw_))
    if C != Ck:
        raise RuntimeError("Input shape and kernel channels wont match: (%d vs %d)." % (C, Ck))
    Ho = (H + 2 * pad_h - (dilation_h * (kernel_h - 1) + 1)) // stride_h + 1
    Wo = (W + 2 * pad_w - (dilation_w * (kernel_w - 1) + 1)) // stride_w + 1
    if tuple(offset.shape) != (B, 2 * deformable_group * kernel_h * kernel_w, Ho, Wo):
        raise RuntimeError("offset shape %s does not match [B, 2*dg*kh*kw, Ho, Wo] = %s"
                           % (tuple(offset.shape), (B, 2 * deformable_group * kernel_h * kernel_w, Ho, Wo)))
    if tuple(mask.shape) != (B, deformable_group * kernel_h * kernel_w, Ho, Wo):
        raise RuntimeError("mask shape %s does not match [B, dg*kh*kw, Ho, Wo]" % (tuple(mask.shape),))
    if bias.numel() != Cout:
        raise RuntimeError("bias has %d elements, expected %d" % (bias.numel(), Cout))
    return B, C, H, W, Cout, Ho, Wo


def dcn_v2_forward(input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w,
                   pad_h, pad_w, dilation_h, dilation_w, deformable_group):
    """Positional twin of `_ext.dcn_v2_forward` (dcn_v2.py:25-31 call site): fp32 contiguous NCHW CUDA tensors in, a new
    [B,Cout,Ho,Wo] fp32 tensor out.

    Throughput form (same function, nothing to opt into): in the model's configuration (3x3 s1 p1 d1 dg1, C % 16 == 0)
      * the packed filters are cached per (weight, bias) version -- a layer that runs every batch packs once;
      * an `input` in torch.channels_last memory format is read in place (no relayout) and the output comes back
        channels-last as well (torch's convention: the output follows the input's memory format);
      * a bfloat16 channels-last `input` runs the network's bf16 DeformConv path (fp16 filters and blend, f16 MFMA, fp32
        accumulation) and returns bfloat16; offset / mask stay fp32 NCHW as in the reference."""
    _lib.require_cuda(input, weight, bias, offset, mask)
    lowp = input.dtype == torch.bfloat16
    for t in (weight, bias, offset, mask) + (() if lowp else (input,)):
        if t.dtype != torch.float32:
            raise RuntimeError("dcn_v2_forward: expected float32 tensors (reference uses .data<float>())")
    nhwc = input.dim() == 4 and input.is_contiguous(memory_format=torch.channels_last) and not input.is_contiguous()
    if lowp and not (input.dim() == 4 and input.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("dcn_v2_forward: a bfloat16 input must be in torch.channels_last memory format")
    nhwc = nhwc or lowp
    if not nhwc:
        input = input.contiguous()
    weight, bias, offset, mask = [t.contiguous() for t in (weight, bias, offset, mask)]
    B, C, H, W, Cout, Ho, Wo = _dcn_operands("dcn_v2_forward", input, weight, bias, offset, mask,
                                             (kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group))
    fast = ((kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group)
            == (3, 3, 1, 1, 1, 1, 1, 1, 1) and C % 16 == 0 and H <= 32767 and W <= 32767)
    L = _lib.lib()
    with torch.cuda.device(input.device):
        if fast:
            # LDS-apron + MFMA kernel on packed filters (cached); the workspace holds the [B,H,W,32] offset/mask rows and, for an
            # NCHW input, its channels-last copy (the reference allocates `columns` / `ones` itself, dcn_v2_cuda.cu:90-103;
            # here torch's caching allocator does, stream-ordered)
            out_nhwc = nhwc and Cout % 4 == 0
            dtype = _lib.H3D_BF16 if lowp else _lib.H3D_F32
            if lowp and not out_nhwc:
                raise RuntimeError("dcn_v2_forward: bfloat16 needs Cout % 4 == 0")
            flags = (_lib.DCN_INPUT_NHWC if nhwc else 0) | (_lib.DCN_OUTPUT_NHWC if out_nhwc else 0) | (_lib.DCN_F32_MFMA if OP_F32_MFMA and not lowp else 0)
            packed = _packed_weights(weight, bias, dtype)
            out = torch.empty(B, Cout, Ho, Wo, dtype=input.dtype if lowp else torch.float32, device=input.device,
                              memory_format=torch.channels_last if out_nhwc else torch.contiguous_format)
            nws = int(L.h3d_dcn_v2_packed_workspace_bytes(B, C, H, W, flags))
            ws = torch.empty(nws, dtype=torch.uint8, device=input.device)
            rc = L.h3d_dcn_v2_forward_packed(_lib.ptr(input), _lib.ptr(packed), _lib.ptr(offset), _lib.ptr(mask), _lib.ptr(out),
                                             B, C, H, W, Cout, dtype, flags, _lib.ptr(ws), nws, _lib.stream_ptr())
        else:
            if lowp:
                raise RuntimeError("dcn_v2_forward: bfloat16 is implemented for the model's configuration only (3x3 s1 p1 d1 dg1)")
            if nhwc:
                input = input.contiguous()
            out = torch.empty(B, Cout, Ho, Wo, dtype=torch.float32, device=input.device)
            rc = L.h3d_dcn_v2_forward_ws(
                _lib.ptr(input), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(offset), _lib.ptr(mask), _lib.ptr(out),
                B, C, H, W, Cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                deformable_group, None, 0, _lib.stream_ptr())
    _lib.check(rc, "dcn_v2_forward")
    return out


def dcn_v2_conv(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups):
    """`_DCNv2.apply` argument order (dcn_v2.py:18-33), forward only."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (input, offset, mask)):
        raise RuntimeError("h3d_amd DCNv2 is inference-only (use dcn_v2_conv_autograd / TrainableDCNv2 to train): "
                           "an input tensor requires grad")
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    dh, dw = _pair(dilation)
    kh, kw = weight.shape[2:4]
    with torch.no_grad():       # (parameters require grad by default; the result carries no graph)
        return dcn_v2_forward(input, weight, bias, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, deformable_groups)


class _InferenceOnly(torch.autograd.Function):
    """Identity whose backward raises: a module in training mode returns its forward result (the reference's plain usage
    `DCN(...).cuda()(x)`, DCNv2/test.py:169-180, is forward-only), and a training loop that calls .backward() through it learns at
    once that dcn_v2_backward (dcn_v2_cuda.cu:175-336) is out of scope instead of silently getting no gradients."""

    @staticmethod
    def forward(ctx, out, *params):
        return out.view_as(out)

    @staticmethod
    def backward(ctx, grad):
        raise RuntimeError("h3d_amd DCNv2 is inference-only (use TrainableDCNv2 / TrainableDCN to train): call .eval() or run under torch.no_grad()")


class DCNv2(nn.Module):
    """Parameters + forward(input, offset, mask) (dcn_v2.py:57-94)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.dilation = _pair(padding), _pair(dilation)
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.in_channels * self.kernel_size[0] * self.kernel_size[1])
        with torch.no_grad():
            self.weight.uniform_(-stdv, stdv)
            self.bias.zero_()

    def forward(self, input, offset, mask):
        k = self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]
        assert 2 * k == offset.shape[1]
        assert k == mask.shape[1]
        out = dcn_v2_conv(input, offset, mask, self.weight, self.bias, self.stride, self.padding,
                          self.dilation, self.deformable_groups)
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _InferenceOnly.apply(out, *[p for p in self.parameters() if p.requires_grad])    # forward works, backward raises
        return out


class DCN(DCNv2):
    """DCNv2 + its own offset/mask conv (dcn_v2.py:97-128): zero-initialised
    `conv_offset_mask`, offset = first 2/3 of its output, mask = sigmoid(last 1/3)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups)
        ch = self.deformable_groups * 3 * self.kernel_size[0] * self.kernel_size[1]
        self.conv_offset_mask = nn.Conv2d(self.in_channels, ch, kernel_size=self.kernel_size, stride=self.stride,
                                          padding=self.padding, bias=True)
        with torch.no_grad():
            self.conv_offset_mask.weight.zero_()
            self.conv_offset_mask.bias.zero_()

    def _fused_ok(self, input):
        return (self.kernel_size == (3, 3) and self.stride == (1, 1) and self.padding == (1, 1) and self.dilation == (1, 1)
                and self.deformable_groups == 1 and self.in_channels % 16 == 0 and input.is_cuda
                and input.dtype == torch.float32 and input.dim() == 4)

    def _packed(self, device):
        """Weights in the layout of the fused DeformConv kernel (csrc/dcn3.hip, fp32), kept on the module and validated on the
        device at every forward (`h3d_dcn_fused_pack_f32_cached`: a hash of the four parameters' bytes decides, on the stream,
        whether the pack kernel has anything to do) -- so `dcn.weight.data.zero_()` between two forwards (DCNv2/test.py:21) is
        seen although no version counter moves.  `.to(device)` / `load_state_dict` need no hook: new bytes, new hash.
        Called with `device` current.  The kept pack belongs to the stream that created it (one validation accumulator: see
        `_packed_weights`); a forward on another stream packs into buffers of its own."""
        rows = (self.out_channels + 127) // 128 * 128
        C = self.in_channels
        stream = torch.cuda.current_stream(device).cuda_stream

        def fresh():
            return (torch.empty(rows * 9 * C, dtype=torch.float32, device=device), torch.empty(128 * 9 * C, dtype=torch.float32, device=device),
                    torch.zeros(rows + 32 + 64, dtype=torch.float32, device=device), torch.zeros(2, dtype=torch.int64, device=device), (rows, C), stream)
        ent = getattr(self, "_pack", None)
        if ent is None or ent[0].device != device or ent[4] != (rows, C):
            ent = fresh()
            object.__setattr__(self, "_pack", ent)
        elif ent[5] != stream:
            ent = fresh()               # (a zeroed state never matches: the pack kernel runs; nothing is kept)
        ps = [p.detach().contiguous() for p in (self.weight, self.bias, self.conv_offset_mask.weight, self.conv_offset_mask.bias)]
        if any(p.dtype != torch.float32 for p in ps):
            raise RuntimeError("DCN: expected float32 parameters (reference uses .data<float>())")
        _lib.check(_lib.lib().h3d_dcn_fused_pack_f32_cached(*[_lib.ptr(p) for p in ps], self.out_channels, C, _lib.ptr(ent[0]), _lib.ptr(ent[1]),
                                                            _lib.ptr(ent[2]), _lib.ptr(ent[3]), _lib.stream_ptr()), "dcn_fused_pack_f32_cached")
        return ent[0], ent[1], ent[2], rows

    def forward(self, input):
        """conv_offset_mask -> chunk/cat/sigmoid -> dcn_v2_conv (dcn_v2.py:118-128).  In the configuration the model uses
        (model.py:355) all of it is ONE launch of the fused DeformConv kernel in fp32 parity mode (offsets and mask never
        reach memory); other configurations run conv_offset_mask + chunk / cat / sigmoid as one launch of the library's general
        kernel (`h3d_dcn_offset_mask`) and then the operator: no nn.Conv2d / vendor library call on any path."""
        if torch.is_grad_enabled() and input.requires_grad:
            raise RuntimeError("h3d_amd DCNv2 is inference-only (use TrainableDCN to train): the input requires grad")
        if not input.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        # (parameters require grad by default: `dcn(x)` outside no_grad must return the forward result as it does in the reference,
        #  DCNv2/test.py:17-30, 169-180)
        with torch.no_grad():
            out = self._forward(input)
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            # a fine-tuning loop must not silently get no gradients (the reference implements dcn_v2_backward, out of scope here):
            # the result carries a graph node whose backward raises
            return _InferenceOnly.apply(out, *[p for p in self.parameters() if p.requires_grad])
        return out

    def _forward(self, input):
        if self._fused_ok(input):
            from ._lib import H3dOp
            x = input.contiguous()
            B, C, H, W = x.shape
            with torch.cuda.device(x.device):       # (the pack's launches go to x.device's current stream, like the forward's)
                wp, wo, bias, rows = self._packed(x.device)
                xn = torch.empty(B, H, W, C, dtype=torch.float32, device=x.device)
                out = torch.empty(B, self.out_channels, H, W, dtype=torch.float32, device=x.device)
                L = _lib.lib()
                if OP_F32_MFMA:
                    _lib.check(L.h3d_nchw_f32_to_nhwc(_lib.ptr(x), _lib.ptr(xn), _lib.H3D_F32, B, C, H, W, C, _lib.stream_ptr()), "DCN: to NHWC")
                else:
                    # the relayout scales x by the power of two the device derives from max |x| (into the word behind the filter maxima)
                    _lib.check(L.h3d_dcn_nchw_to_nhwc_scaled(_lib.ptr(x), _lib.ptr(xn), B, C, H, W, bias.data_ptr() + 4 * (rows + _lib.DCN_FUSED_BIAS_AMAX),
                                                             _lib.stream_ptr()), "DCN: to NHWC")
                op = H3dOp()
                # fp32 tensors, fp32 packs; since round 5 every product as three fp16 MFMAs on split operands (filters scaled and split while
                # they are staged: OPF_DCN_FUSED_RAW_PACK; activations scaled in the relayout: OPF_DCN_FUSED_SCALED_INPUT), or exact fmaf chains on the fp32 matrix
                # instruction with OP_F32_MFMA
                op.kind, op.dtype, op.B, op.H, op.W, op.Ho, op.Wo = _lib.OP_DCN_FUSED, (_lib.H3D_F32 if OP_F32_MFMA else _lib.H3D_F16X3), B, H, W, H, W
                op.reserved = 0 if OP_F32_MFMA else _lib.OPF_DCN_FUSED_RAW_PACK | _lib.OPF_DCN_FUSED_SCALED_INPUT
                op.in_, op.in2, op.w, op.bias, op.out = xn.data_ptr(), wo.data_ptr(), wp.data_ptr(), bias.data_ptr(), out.data_ptr()
                op.Cin, op.in_cs, op.Cout, op.out_cs, op.ksize, op.stride, op.relu = C, C, self.out_channels, self.out_channels, 3, 1, 0
                op.out_mode, op.wrows = _lib.OUT_NCHW_F32, rows
                arr = (H3dOp * 1)(op)
                _lib.check(L.h3d_run_ops(arr, 1, _lib.stream_ptr()), "DCN.forward")
            return out
        # any other configuration (stride / dilation / deformable_groups / kernel size / channel count): conv_offset_mask -> chunk /
        # cat / sigmoid (dcn_v2.py:119-124) in ONE launch of this library's general kernel (`h3d_dcn_offset_mask`: no nn.Conv2d, i.e.
        # no vendor convolution library anywhere in the module), then the operator
        if input.dtype != torch.float32 or input.dim() != 4:
            raise RuntimeError("DCN: expected a float32 [B,C,H,W] input (reference uses .data<float>())")
        x = input.contiguous()
        B, C, H, W = x.shape
        kh, kw = self.kernel_size
        k = self.deformable_groups * kh * kw
        ow, ob = self.conv_offset_mask.weight.detach().contiguous(), self.conv_offset_mask.bias.detach().contiguous()
        if tuple(ow.shape) != (3 * k, C, kh, kw) or ow.dtype != torch.float32 or ob.dtype != torch.float32:
            raise RuntimeError("DCN: conv_offset_mask.weight %s does not match [3*dg*kh*kw, C, kh, kw] = %s (float32)"
                               % (tuple(ow.shape), (3 * k, C, kh, kw)))
        Ho = (H + 2 * self.padding[0] - kh) // self.stride[0] + 1
        Wo = (W + 2 * self.padding[1] - kw) // self.stride[1] + 1
        with torch.cuda.device(x.device):
            offset = torch.empty(B, 2 * k, Ho, Wo, dtype=torch.float32, device=x.device)
            mask = torch.empty(B, k, Ho, Wo, dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().h3d_dcn_offset_mask(_lib.ptr(x), _lib.ptr(ow), _lib.ptr(ob), _lib.ptr(offset), _lib.ptr(mask), B, C, H, W,
                                                      kh, kw, self.stride[0], self.stride[1], self.padding[0], self.padding[1],
                                                      self.deformable_groups, _lib.stream_ptr()), "DCN: conv_offset_mask")
        return dcn_v2_conv(x, offset, mask, self.weight, self.bias, self.stride, self.padding,
                           self.dilation, self.deformable_groups)


# ---- training: dcn_v2_backward, the autograd function and the trainable modules (kernels: csrc/dcn_bwd.hip) ----------------------

def _dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                     dilation_h, dilation_w, deformable_group, need=(True,) * 5, general=False):
    """`dcn_v2_backward` with a choice of outputs (`need`: input, offset, mask, weight, bias -- autograd's needs_input_grad; an output that is
    not needed is None) and of kernels (`general`: the general kernels on the model's configuration too)."""
    _lib.require_cuda(input, weight, bias, offset, mask, grad_output)
    for t in (input, weight, bias, offset, mask, grad_output):
        if t.dtype != torch.float32:
            raise RuntimeError("dcn_v2_backward: expected float32 tensors (reference uses .data<float>())")
    input, weight, bias, offset, mask, grad_output = [t.contiguous() for t in (input, weight, bias, offset, mask, grad_output)]
    B, C, H, W, Cout, Ho, Wo = _dcn_operands("dcn_v2_backward", input, weight, bias, offset, mask,
                                             (kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group))
    if tuple(grad_output.shape) != (B, Cout, Ho, Wo):
        raise RuntimeError("grad_output shape %s does not match [B, Cout, Ho, Wo] = %s" % (tuple(grad_output.shape), (B, Cout, Ho, Wo)))
    geo = (B, C, H, W, Cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group)
    L = _lib.lib()
    with torch.cuda.device(input.device):
        ws = _lib.workspace(L.h3d_dcn_v2_backward_workspace_bytes, *geo, device=input.device, min_bytes=1, what="dcn_v2_backward")
        outs = [torch.empty_like(t) if n else None for t, n in zip((input, offset, mask, weight, bias), need)]
        fn = L.h3d_dcn_v2_backward_general if general else L.h3d_dcn_v2_backward
        rc = fn(*[_lib.ptr(t) for t in (input, weight, bias, offset, mask, grad_output)], *[_lib.ptr(t) for t in outs], *geo,
                _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "dcn_v2_backward")
    return tuple(outs)


def dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w,
                    pad_h, pad_w, dilation_h, dilation_w, deformable_group):
    """Positional twin of `_ext.dcn_v2_backward` (dcn_v2.py:39-48 call site): fp32 CUDA tensors in, new tensors
    (grad_input, grad_offset, grad_mask, grad_weight, grad_bias) out.  Current stream, no host synchronisation."""
    return _dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                            dilation_h, dilation_w, deformable_group)


class _DCNv2(torch.autograd.Function):
    """The reference's autograd function (dcn_v2.py:16-51), argument order included."""

    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups):
        ctx.stride, ctx.padding, ctx.dilation = _pair(stride), _pair(padding), _pair(dilation)
        ctx.kernel_size = _pair(weight.shape[2:4])
        ctx.deformable_groups = deformable_groups
        output = dcn_v2_forward(input, weight, bias, offset, mask, ctx.kernel_size[0], ctx.kernel_size[1], ctx.stride[0], ctx.stride[1],
                                ctx.padding[0], ctx.padding[1], ctx.dilation[0], ctx.dilation[1], ctx.deformable_groups)
        ctx.save_for_backward(input, offset, mask, weight, bias)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input, offset, mask, weight, bias = ctx.saved_tensors
        ni, no, nm, nw, nb = ctx.needs_input_grad[:5]
        gi, go, gm, gw, gb = _dcn_v2_backward(input, weight, bias, offset, mask, grad_output, ctx.kernel_size[0], ctx.kernel_size[1],
                                              ctx.stride[0], ctx.stride[1], ctx.padding[0], ctx.padding[1], ctx.dilation[0],
                                              ctx.dilation[1], ctx.deformable_groups, need=(ni, no, nm, nw, nb))
        return gi, go, gm, gw, gb, None, None, None, None


dcn_v2_conv_autograd = _DCNv2.apply


class TrainableDCNv2(DCNv2):
    """`DCNv2` whose forward builds a graph (the reference's behaviour): same constructor, same state_dict keys."""

    def forward(self, input, offset, mask):
        k = self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]
        assert 2 * k == offset.shape[1]
        assert k == mask.shape[1]
        return dcn_v2_conv_autograd(input, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                    self.deformable_groups)


class TrainableDCN(DCN):
    """`DCN` whose forward builds a graph: same constructor, same state_dict keys.  conv_offset_mask runs as the operator itself with zero
    offsets and a unit mask (what `h3d_dcn_offset_mask` does for the inference module), so its gradients come from the same kernels and
    no vendor convolution enters the module; chunk / cat / sigmoid are torch ops (dcn_v2.py:118-128)."""

    def forward(self, input):
        if not input.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        if input.dtype != torch.float32 or input.dim() != 4:
            raise RuntimeError("DCN: expected a float32 [B,C,H,W] input (reference uses .data<float>())")
        B, C, H, W = input.shape
        kh, kw = self.kernel_size
        Ho = (H + 2 * self.padding[0] - kh) // self.stride[0] + 1
        Wo = (W + 2 * self.padding[1] - kw) // self.stride[1] + 1
        zero = torch.zeros(B, 2 * kh * kw, Ho, Wo, dtype=torch.float32, device=input.device)
        one = torch.ones(B, kh * kw, Ho, Wo, dtype=torch.float32, device=input.device)
        out = dcn_v2_conv_autograd(input, zero, one, self.conv_offset_mask.weight, self.conv_offset_mask.bias, self.stride, self.padding,
                                   (1, 1), 1)             # (nn.Conv2d of dcn_v2.py:107-111: no dilation, no groups)
        o1, o2, mask = torch.chunk(out, 3, dim=1)
        offset = torch.cat((o1, o2), dim=1)
        mask = torch.sigmoid(mask)
        return dcn_v2_conv_autograd(input, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                    self.deformable_groups)


# ---- deformable PS-ROI pooling, forward (dcn_v2.py:130-303 of the reference; kernel: csrc/psroi.hip) ----------------------------

def _pool_common(what, input, bbox, output_dim, group_size, pooled_size, part_size, sample_per_part):
    """Argument checks shared by the two pooling entry points; returns contiguous (input, bbox) and (B, C, H, W, R)."""
    _lib.require_cuda(input, bbox)
    for t in (input, bbox):
        if t.dtype != torch.float32:
            raise RuntimeError("%s: expected float32 tensors (reference uses .data<float>())" % what)
    if input.dim() != 4:
        raise RuntimeError("%s: input must be [B,C,H,W], got %s" % (what, tuple(input.shape)))
    if bbox.dim() != 2 or bbox.shape[1] != 5:
        raise RuntimeError("%s: rois must be [R,5] (batch, x1, y1, x2, y2), got %s" % (what, tuple(bbox.shape)))
    if bbox.device != input.device:
        raise RuntimeError("%s: rois are on %s, input on %s" % (what, bbox.device, input.device))
    B, C, H, W = input.shape
    if C != output_dim:
        raise RuntimeError("input channels and output channels must equal")
    if group_size != 1:
        raise RuntimeError("%s: only group_size == 1 is supported (the reference reads channel (ctop*gs+gh)*gs+gw past the input "
                           "for group_size %d)" % (what, group_size))
    if pooled_size < 1 or part_size < 1 or sample_per_part < 1:
        raise RuntimeError("%s: pooled_size, part_size and sample_per_part must be positive" % what)
    if B == 0 or H == 0 or W == 0:
        raise RuntimeError("%s: empty input %s" % (what, tuple(input.shape)))
    return input.contiguous(), bbox.contiguous(), (B, C, H, W, bbox.shape[0])


def dcn_v2_psroi_pooling_forward(input, bbox, trans, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                                 sample_per_part, trans_std):
    """Positional twin of `_ext.dcn_v2_psroi_pooling_forward` (DCNv2/src/dcn_v2.h:76-107): returns (output, output_count), both
    [R, output_dim, P, P] fp32, P = pooled_size; output_count holds the number of valid samples per bin.  Launches on the current
    stream of input's device; no host synchronisation.  fp32 only, group_size == 1 only, output_dim == C; without no_trans, trans
    is [>= R, 2*num_classes, part_size, part_size] (include/h3d.h lists what this library decides where the reference does not)."""
    what = "dcn_v2_psroi_pooling_forward"
    input, bbox, (B, C, H, W, R) = _pool_common(what, input, bbox, output_dim, group_size, pooled_size, part_size, sample_per_part)
    no_trans = int(bool(no_trans))
    ct = 0
    if not no_trans:
        _lib.require_cuda(trans)
        if trans.dtype != torch.float32:
            raise RuntimeError("%s: expected float32 tensors (reference uses .data<float>())" % what)
        if trans.device != input.device:
            raise RuntimeError("%s: trans is on %s, input on %s" % (what, trans.device, input.device))
        if trans.dim() != 4 or tuple(trans.shape[2:]) != (part_size, part_size) or trans.shape[0] < R:
            raise RuntimeError("%s: trans %s does not match [>= %d, 2*num_classes, %d, %d]"
                               % (what, tuple(trans.shape), R, part_size, part_size))
        ct = trans.shape[1]
        if ct < 2 or ct % 2:
            raise RuntimeError("%s: trans has %d channels, expected 2 * num_classes" % (what, ct))
        if output_dim % (ct // 2):
            raise RuntimeError("%s: output_dim %d is not a multiple of num_classes %d" % (what, output_dim, ct // 2))
        trans = trans.contiguous()
    out = torch.empty(R, output_dim, pooled_size, pooled_size, dtype=torch.float32, device=input.device)
    count = torch.empty_like(out)
    if R == 0:
        return out, count
    with torch.cuda.device(input.device):
        rc = _lib.lib().h3d_dcn_v2_psroi_pooling_forward(
            _lib.ptr(input), _lib.ptr(bbox), _lib.ptr(None if no_trans else trans), _lib.ptr(out), _lib.ptr(count),
            B, C, H, W, R, ct, no_trans, float(spatial_scale), output_dim, group_size, pooled_size, part_size, sample_per_part,
            float(trans_std), _lib.stream_ptr())
    _lib.check(rc, what)
    return out, count


def _dcn_pooling_modulated(input, rois, offset_mask, spatial_scale, pooled_size, output_dim, group_size, part_size,
                           sample_per_part, trans_std):
    """DCNPooling's second pass (dcn_v2.py:281-292): offset = channels 0/1 of offset_mask [R,3,P,P], result x sigmoid(channel 2),
    in one launch (`h3d_dcn_pooling_modulated`)."""
    what = "DCNPooling"
    input, rois, (B, C, H, W, R) = _pool_common(what, input, rois, output_dim, group_size, pooled_size, part_size, sample_per_part)
    if part_size != pooled_size:
        raise RuntimeError("%s: part_size %d != pooled_size %d: the reference indexes its [R,2,P,P] offsets with part_size"
                           % (what, part_size, pooled_size))
    offset_mask = offset_mask.contiguous()
    if offset_mask.dtype != torch.float32 or tuple(offset_mask.shape) != (R, 3, pooled_size, pooled_size):
        raise RuntimeError("%s: offset/mask %s is not float32 [%d, 3, %d, %d]" % (what, tuple(offset_mask.shape), R, pooled_size,
                                                                                 pooled_size))
    out = torch.empty(R, output_dim, pooled_size, pooled_size, dtype=torch.float32, device=input.device)
    if R == 0:
        return out
    with torch.cuda.device(input.device):
        rc = _lib.lib().h3d_dcn_pooling_modulated(
            _lib.ptr(input), _lib.ptr(rois), _lib.ptr(offset_mask), _lib.ptr(out), B, C, H, W, R, float(spatial_scale), output_dim,
            group_size, pooled_size, part_size, sample_per_part, float(trans_std), _lib.stream_ptr())
    _lib.check(rc, what)
    return out


def dcn_v2_pooling(input, rois, offset, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None,
                   sample_per_part=4, trans_std=.0):
    """`_DCNv2Pooling.apply` argument order and defaults (dcn_v2.py:132-161), forward only: returns `output`."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (input, offset)):
        raise RuntimeError("h3d_amd DCNv2 pooling is inference-only (use dcn_v2_pooling_autograd / TrainableDCNv2Pooling to train): "
                           "an input tensor requires grad")
    part_size = pooled_size if part_size is None else part_size
    with torch.no_grad():
        out, _ = dcn_v2_psroi_pooling_forward(input, rois, offset, int(no_trans), spatial_scale, output_dim, group_size, pooled_size,
                                              part_size, sample_per_part, trans_std)
    return out


class DCNv2Pooling(nn.Module):
    """Pooling parameters + forward(input, rois, offset) (dcn_v2.py:190-226)."""

    def __init__(self, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None, sample_per_part=4,
                 trans_std=.0):
        super().__init__()
        self.spatial_scale = spatial_scale
        self.pooled_size = pooled_size
        self.output_dim = output_dim
        self.no_trans = no_trans
        self.group_size = group_size
        self.part_size = pooled_size if part_size is None else part_size
        self.sample_per_part = sample_per_part
        self.trans_std = trans_std

    def forward(self, input, rois, offset):
        assert input.shape[1] == self.output_dim
        if self.no_trans:
            offset = input.new()
        return dcn_v2_pooling(input, rois, offset, self.spatial_scale, self.pooled_size, self.output_dim, self.no_trans,
                              self.group_size, self.part_size, self.sample_per_part, self.trans_std)


class DCNPooling(DCNv2Pooling):
    """DCNv2Pooling + its own offset/mask predictor (dcn_v2.py:229-303): `offset_mask_fc` = Linear / ReLU / Linear / ReLU / Linear,
    the last layer zero-initialised.  forward(input, rois): pool without translation, run the MLP (torch nn.Linear: plumbing), then
    ONE launch pools with the predicted offsets and multiplies by sigmoid(mask)."""

    def __init__(self, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None, sample_per_part=4,
                 trans_std=.0, deform_fc_dim=1024):
        super().__init__(spatial_scale, pooled_size, output_dim, no_trans, group_size, part_size, sample_per_part, trans_std)
        self.deform_fc_dim = deform_fc_dim
        if not no_trans:
            self.offset_mask_fc = nn.Sequential(
                nn.Linear(self.pooled_size * self.pooled_size * self.output_dim, self.deform_fc_dim),
                nn.ReLU(inplace=True),
                nn.Linear(self.deform_fc_dim, self.deform_fc_dim),
                nn.ReLU(inplace=True),
                nn.Linear(self.deform_fc_dim, self.pooled_size * self.pooled_size * 3))
            with torch.no_grad():
                self.offset_mask_fc[4].weight.zero_()
                self.offset_mask_fc[4].bias.zero_()

    def forward(self, input, rois):
        if torch.is_grad_enabled() and input.requires_grad:
            raise RuntimeError("h3d_amd DCNv2 pooling is inference-only (use TrainableDCNPooling to train): the input requires grad")
        with torch.no_grad():
            out = self._forward(input, rois)
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _InferenceOnly.apply(out, *[p for p in self.parameters() if p.requires_grad])    # forward works, backward raises
        return out

    def _forward(self, input, rois):
        if self.no_trans:
            return dcn_v2_pooling(input, rois, input.new(), self.spatial_scale, self.pooled_size, self.output_dim, self.no_trans,
                                  self.group_size, self.part_size, self.sample_per_part, self.trans_std)
        if self.part_size != self.pooled_size:
            raise RuntimeError("DCNPooling: part_size %d != pooled_size %d: the reference indexes its [R,2,P,P] offsets with "
                               "part_size" % (self.part_size, self.pooled_size))
        n = rois.shape[0]
        roi = dcn_v2_pooling(input, rois, input.new(), self.spatial_scale, self.pooled_size, self.output_dim, True,
                             self.group_size, self.part_size, self.sample_per_part, self.trans_std)
        offset_mask = self.offset_mask_fc(roi.reshape(n, self.output_dim * self.pooled_size ** 2)).view(n, 3, self.pooled_size, self.pooled_size)
        return _dcn_pooling_modulated(input, rois, offset_mask, self.spatial_scale, self.pooled_size, self.output_dim,
                                      self.group_size, self.part_size, self.sample_per_part, self.trans_std)


# ---- training: dcn_v2_psroi_pooling_backward, the autograd functions and the trainable modules (kernels: csrc/psroi_bwd.hip) -----

def _check_trans(what, trans, input, R, output_dim, part_size):
    """The forward's checks of `trans` ([>= R, 2*num_classes, part, part] fp32 on input's device) -> contiguous trans."""
    _lib.require_cuda(trans)
    if trans.dtype != torch.float32:
        raise RuntimeError("%s: expected float32 tensors (reference uses .data<float>())" % what)
    if trans.device != input.device:
        raise RuntimeError("%s: trans is on %s, input on %s" % (what, trans.device, input.device))
    if trans.dim() != 4 or tuple(trans.shape[2:]) != (part_size, part_size) or trans.shape[0] < R:
        raise RuntimeError("%s: trans %s does not match [>= %d, 2*num_classes, %d, %d]"
                           % (what, tuple(trans.shape), R, part_size, part_size))
    ct = trans.shape[1]
    if ct < 2 or ct % 2:
        raise RuntimeError("%s: trans has %d channels, expected 2 * num_classes" % (what, ct))
    if output_dim % (ct // 2):
        raise RuntimeError("%s: output_dim %d is not a multiple of num_classes %d" % (what, output_dim, ct // 2))
    return trans.contiguous()


def _check_grad_output(what, grad_output, input, R, output_dim, pooled_size):
    _lib.require_cuda(grad_output)
    if grad_output.dtype != torch.float32:
        raise RuntimeError("%s: expected float32 tensors (reference uses .data<float>())" % what)
    if grad_output.device != input.device or tuple(grad_output.shape) != (R, output_dim, pooled_size, pooled_size):
        raise RuntimeError("%s: grad_output %s on %s does not match [%d, %d, %d, %d] on %s"
                           % (what, tuple(grad_output.shape), grad_output.device, R, output_dim, pooled_size, pooled_size, input.device))
    return grad_output.contiguous()


def _dcn_v2_psroi_pooling_backward(grad_output, input, bbox, trans, output_count, no_trans, spatial_scale, output_dim, group_size,
                                   pooled_size, part_size, sample_per_part, trans_std, need=(True, True), direct=False):
    """`dcn_v2_psroi_pooling_backward` with a choice of outputs (`need`: input, trans -- autograd's needs_input_grad; an output that is not
    needed is None) and of the grad_input path (`direct`: one global atomic per sample corner, never combined in LDS)."""
    what = "dcn_v2_psroi_pooling_backward"
    input, bbox, (B, C, H, W, R) = _pool_common(what, input, bbox, output_dim, group_size, pooled_size, part_size, sample_per_part)
    no_trans = int(bool(no_trans))
    grad_output = _check_grad_output(what, grad_output, input, R, output_dim, pooled_size)
    _lib.require_cuda(output_count)
    if output_count.dtype != torch.float32 or output_count.device != input.device or output_count.shape != grad_output.shape:
        raise RuntimeError("%s: output_count %s does not match grad_output %s (float32)" % (what, tuple(output_count.shape), tuple(grad_output.shape)))
    output_count = output_count.contiguous()
    ct = 0
    if not no_trans:
        trans = _check_trans(what, trans, input, R, output_dim, part_size)
        ct = trans.shape[1]
    with torch.cuda.device(input.device):
        grad_input = torch.empty_like(input) if need[0] else None
        # (the reference returns zeros_like(trans) in either mode: with no_trans that is whatever placeholder it was given)
        grad_trans = (torch.zeros_like(trans) if no_trans else torch.empty_like(trans)) if need[1] and trans is not None else None
        rc = _lib.lib().h3d_dcn_v2_psroi_pooling_backward(
            _lib.ptr(grad_output), _lib.ptr(input), _lib.ptr(bbox), _lib.ptr(None if no_trans else trans), _lib.ptr(output_count),
            _lib.ptr(grad_input), _lib.ptr(None if no_trans else grad_trans), B, C, H, W, R, 0 if no_trans else trans.shape[0], ct, no_trans,
            float(spatial_scale), output_dim, group_size, pooled_size, part_size, sample_per_part, float(trans_std), int(bool(direct)),
            _lib.stream_ptr())
    _lib.check(rc, what)
    return grad_input, grad_trans


def dcn_v2_psroi_pooling_backward(grad_output, input, bbox, trans, output_count, no_trans, spatial_scale, output_dim, group_size,
                                  pooled_size, part_size, sample_per_part, trans_std):
    """Positional twin of `_ext.dcn_v2_psroi_pooling_backward` (dcn_v2.py:165-178 call site): returns (grad_input, grad_trans), new
    tensors shaped like input and trans.  An element whose `output_count` is <= 0 is skipped, the others contribute grad_output /
    output_count per valid sample.  grad_input is summed by float atomics; grad_trans in a fixed order (bit-identical from run to run),
    rows of trans beyond the rois get zero.  Current stream, no host synchronisation; the forward's argument checks and error texts."""
    return _dcn_v2_psroi_pooling_backward(grad_output, input, bbox, trans, output_count, no_trans, spatial_scale, output_dim, group_size,
                                          pooled_size, part_size, sample_per_part, trans_std)


def _dcn_pooling_modulated_backward(grad_output, input, rois, offset_mask, spatial_scale, pooled_size, output_dim, group_size, part_size,
                                    sample_per_part, trans_std, need=(True, True), direct=False):
    """Backward of `_dcn_pooling_modulated` (`h3d_dcn_pooling_modulated_backward`) -> (grad_input, grad_offset_mask [R,3,P,P]): channels 0/1 the
    offset gradients, channel 2 the gradient of the mask logit; the chunk / cat / sigmoid / mul chain never appears as torch ops."""
    what = "DCNPooling"
    input, rois, (B, C, H, W, R) = _pool_common(what, input, rois, output_dim, group_size, pooled_size, part_size, sample_per_part)
    if part_size != pooled_size:
        raise RuntimeError("%s: part_size %d != pooled_size %d: the reference indexes its [R,2,P,P] offsets with part_size"
                           % (what, part_size, pooled_size))
    _lib.require_cuda(offset_mask)
    if offset_mask.device != input.device:
        raise RuntimeError("%s: offset/mask is on %s, input on %s" % (what, offset_mask.device, input.device))
    offset_mask = offset_mask.contiguous()
    if offset_mask.dtype != torch.float32 or tuple(offset_mask.shape) != (R, 3, pooled_size, pooled_size):
        raise RuntimeError("%s: offset/mask %s is not float32 [%d, 3, %d, %d]" % (what, tuple(offset_mask.shape), R, pooled_size,
                                                                                 pooled_size))
    grad_output = _check_grad_output(what, grad_output, input, R, output_dim, pooled_size)
    with torch.cuda.device(input.device):
        grad_input = torch.empty_like(input) if need[0] else None
        grad_om = torch.empty_like(offset_mask) if need[1] else None
        rc = _lib.lib().h3d_dcn_pooling_modulated_backward(
            _lib.ptr(grad_output), _lib.ptr(input), _lib.ptr(rois), _lib.ptr(offset_mask), _lib.ptr(grad_input), _lib.ptr(grad_om),
            B, C, H, W, R, float(spatial_scale), output_dim, group_size, pooled_size, part_size, sample_per_part, float(trans_std),
            int(bool(direct)), _lib.stream_ptr())
    _lib.check(rc, what)
    return grad_input, grad_om


def psroi_backward_path(roi, trans_row, input_shape, no_trans, spatial_scale, pooled_size, part_size, sample_per_part, trans_std,
                        class_id=0, direct=False):
    """Which grad_input path the backward kernel takes for one (roi, class) -- a function of the geometry alone, computed on the host
    by the code the kernel runs (`h3d_psroi_backward_path`): 0 = nothing to add, 1 = combined in LDS, 2 = added directly.  roi: 5
    numbers; trans_row: the roi's [2*num_classes, part, part] translations (an offset_mask row [3,P,P] in modulated mode) or None."""
    import ctypes
    B, C, H, W = input_shape
    r = (ctypes.c_float * 5)(*[float(v) for v in roi])
    ct, t = 0, None
    if not no_trans:
        tr = torch.as_tensor(trans_row, dtype=torch.float32).cpu().contiguous()
        ct = tr.shape[0] - tr.shape[0] % 2
        t = ctypes.c_void_p(tr.data_ptr())
    path = ctypes.c_int(-1)
    _lib.check(_lib.lib().h3d_psroi_backward_path(ctypes.cast(r, ctypes.c_void_p), t, B, C, H, W, ct, int(bool(no_trans)), float(spatial_scale),
                                                  pooled_size, part_size, sample_per_part, float(trans_std), class_id, int(bool(direct)),
                                                  ctypes.byref(path)), "psroi_backward_path")
    return path.value


class _DCNv2Pooling(torch.autograd.Function):
    """The reference's autograd function (dcn_v2.py:132-181), argument order and defaults included; rois get no gradient."""

    @staticmethod
    def forward(ctx, input, rois, offset, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None,
                sample_per_part=4, trans_std=.0):
        ctx.spatial_scale = spatial_scale
        ctx.no_trans = int(no_trans)
        ctx.output_dim = output_dim
        ctx.group_size = group_size
        ctx.pooled_size = pooled_size
        ctx.part_size = pooled_size if part_size is None else part_size
        ctx.sample_per_part = sample_per_part
        ctx.trans_std = trans_std
        output, output_count = dcn_v2_psroi_pooling_forward(input, rois, offset, ctx.no_trans, ctx.spatial_scale, ctx.output_dim,
                                                            ctx.group_size, ctx.pooled_size, ctx.part_size, ctx.sample_per_part,
                                                            ctx.trans_std)
        ctx.save_for_backward(input, rois, offset, output_count)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input, rois, offset, output_count = ctx.saved_tensors
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[2])
        grad_input, grad_offset = _dcn_v2_psroi_pooling_backward(grad_output, input, rois, offset, output_count, ctx.no_trans,
                                                                 ctx.spatial_scale, ctx.output_dim, ctx.group_size, ctx.pooled_size,
                                                                 ctx.part_size, ctx.sample_per_part, ctx.trans_std, need=need)
        return grad_input, None, grad_offset, None, None, None, None, None, None, None, None


dcn_v2_pooling_autograd = _DCNv2Pooling.apply


class _DCNPoolingModulated(torch.autograd.Function):
    """DCNPooling's second pass with its backward: forward(input, rois, offset_mask [R,3,P,P], ...) = `_dcn_pooling_modulated`."""

    @staticmethod
    def forward(ctx, input, rois, offset_mask, spatial_scale, pooled_size, output_dim, group_size, part_size, sample_per_part, trans_std):
        ctx.geo = (spatial_scale, pooled_size, output_dim, group_size, part_size, sample_per_part, trans_std)
        ctx.save_for_backward(input, rois, offset_mask)
        return _dcn_pooling_modulated(input, rois, offset_mask, *ctx.geo)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input, rois, offset_mask = ctx.saved_tensors
        grad_input, grad_om = _dcn_pooling_modulated_backward(grad_output, input, rois, offset_mask, *ctx.geo,
                                                              need=(ctx.needs_input_grad[0], ctx.needs_input_grad[2]))
        return grad_input, None, grad_om, None, None, None, None, None, None, None


class TrainableDCNv2Pooling(DCNv2Pooling):
    """`DCNv2Pooling` whose forward builds a graph (the reference's behaviour): same constructor, no parameters."""

    def forward(self, input, rois, offset):
        assert input.shape[1] == self.output_dim
        if self.no_trans:
            offset = input.new()
        return dcn_v2_pooling_autograd(input, rois, offset, self.spatial_scale, self.pooled_size, self.output_dim, self.no_trans,
                                       self.group_size, self.part_size, self.sample_per_part, self.trans_std)


class TrainableDCNPooling(DCNPooling):
    """`DCNPooling` whose forward builds a graph: same constructor, same state_dict keys.  Pass 1 is `dcn_v2_pooling_autograd` without
    translations, the MLP runs in torch, pass 2 is ONE launch forward (`h3d_dcn_pooling_modulated`) and one backward
    (`h3d_dcn_pooling_modulated_backward`): the same launches as `DCNPooling`, so the forward results are bit-identical to its."""

    def forward(self, input, rois):
        if self.no_trans:
            return dcn_v2_pooling_autograd(input, rois, input.new(), self.spatial_scale, self.pooled_size, self.output_dim, self.no_trans,
                                           self.group_size, self.part_size, self.sample_per_part, self.trans_std)
        if self.part_size != self.pooled_size:
            raise RuntimeError("DCNPooling: part_size %d != pooled_size %d: the reference indexes its [R,2,P,P] offsets with "
                               "part_size" % (self.part_size, self.pooled_size))
        n = rois.shape[0]
        roi = dcn_v2_pooling_autograd(input, rois, input.new(), self.spatial_scale, self.pooled_size, self.output_dim, True,
                                      self.group_size, self.part_size, self.sample_per_part, self.trans_std)
        offset_mask = self.offset_mask_fc(roi.reshape(n, self.output_dim * self.pooled_size ** 2)).view(n, 3, self.pooled_size, self.pooled_size)
        return _DCNPoolingModulated.apply(input, rois, offset_mask, self.spatial_scale, self.pooled_size, self.output_dim, self.group_size,
                                          self.part_size, self.sample_per_part, self.trans_std)
