"""The whole DLA-34 under autograd (reference models/model.py: DLA.forward, Tree, Root, DLAUp, IDAUp, DeformConv, the heads), composed of
the trainable operators: `conv.conv2d_autograd` (stem, level0 / level1, BasicBlocks, `project`, Root on torch.cat),
`pool_up.max_pool2_autograd` (Tree.downsample), `TrainableDCN`'s route (the DeformConvs; `conv2d_autograd` with `not_use_dcn`),
`pool_up.up_add_autograd` (IDAUp's up-sampling + skip add) and `heads.heads_autograd`.

bn="frozen" (the default): every BatchNorm is folded into the convolution in front of it (weights.PackedWeights._fold, the engine's
folding): training the folded filters and biases is fine-tuning with FROZEN statistics.
bn="batch": the reference's own training (HMRTrainer.run_epoch: model.train()): the parameters are the reference's tensors (conv.weight,
each BatchNorm's weight / bias, the DeformConvs' conv.bias and conv_offset_mask.*, up_k.weight, the heads), the running statistics and
num_batches_tracked are buffers, nothing is folded: a convolution without bias, residual or ReLU, then `bn.batch_norm_autograd`
(+ residual) (+ ReLU) where the reference has its BatchNorm.  .train(): batch statistics, the running ones move; .eval(): the running
ones, through the same operator.  The state_dict is the reference's keys and nothing else.  One deviation: the reference's two-level
Trees also run their unused `project` in train() and so move base.level3/4.project.1's running statistics, which no output reads;
here they stay as stored.

    TrainableDLASeg(model, bn="frozen")    model: a model.dla_net(...) in 'f32' or 'f16x3' with head_conv > 0, with or without DCN
      .forward(x)               [ {head: [B,C,H/4,W/4]} ], differentiable at every parameter
      .export_state_dict()      the reference's keys, every fold undone (conv.weight = W' / scale, the shift in the BatchNorm's bias)
      .state_dict() / .load_state_dict()    the export (plus the folded tensors themselves, below) and its inverse
      .sync()                   loads the export into `model`: its engine, MultiPoseDetector and val() see the trained weights
"""
import torch
from torch import nn

from . import arch
from . import bn as bn_ops
from .conv import conv2d_autograd
from .dcn_v2 import dcn_v2_conv_autograd
from .heads import heads_autograd
from .pool_up import max_pool2_autograd, up_add_autograd

FOLDED_PREFIX = "trainable_folded."     # state_dict keys of the folded tensors themselves (see TrainableDLASeg.state_dict)


def _conv_of_bn(bn):
    """The state_dict prefix of the convolution in front of BatchNorm `bn` (models/model.py)."""
    head, leaf = bn.rsplit(".", 1)
    if leaf in ("bn1", "bn2"):
        return head + ".conv" + leaf[2]
    if leaf == "bn":
        return head + ".conv"                              # Root
    if leaf == "1":
        return head + ".0"                                 # nn.Sequential(conv, bn): base_layer, level0 / level1, project
    if leaf == "0" and head.endswith(".actf"):
        return head[:-len(".actf")] + ".conv"              # DeformConv: conv -> actf = Sequential(bn, relu)
    raise ValueError("TrainableDLASeg: no convolution known in front of BatchNorm %r" % bn)


def _bn_of_conv(conv):
    """The inverse of `_conv_of_bn` for the plain convolutions (not the DeformConvs)."""
    head, leaf = conv.rsplit(".", 1)
    if leaf in ("conv1", "conv2"):
        return head + ".bn" + leaf[4]
    if leaf == "conv":
        return head + ".bn"
    if leaf == "0":
        return head + ".1"
    raise ValueError("TrainableDLASeg: no BatchNorm known behind convolution %r" % conv)


def _name(key):
    return key.replace(".", "__")       # (parameter names may not hold a dot; no reference key holds two underscores in a row)


class TrainableDLASeg(nn.Module):
    DTYPES = ("f32", "f16x3")
    BN_MODES = ("frozen", "batch")

    def __init__(self, model, bn="frozen"):
        super().__init__()
        if bn not in self.BN_MODES:
            raise ValueError("TrainableDLASeg: bn must be one of %s, not %r" % (self.BN_MODES, bn))
        self.bn = bn
        if model.compute_dtype not in self.DTYPES:
            raise ValueError("TrainableDLASeg: the model must run in 'f32' or 'f16x3' (fp32 maps), not %r" % (model.compute_dtype,))
        if getattr(model, "arch_name", "") != "dla34" or model.head_conv <= 0:
            raise ValueError("TrainableDLASeg: a DLASeg (DLA-34) with head_conv > 0 is required")
        object.__setattr__(self, "_model", model)        # (not a sub-module: its unfolded tensors stay out of parameters())
        self.use_dcn = bool(model.use_dcn)
        sd = model.state_dict()
        # a Tree of more than one level computes its own `project` and never uses it (models/model.py:212): not part of the graph
        self._unused = tuple("base.level%d.project" % lv for lv in range(2, 6) if arch.LEVELS[lv] > 1)
        self._bns = [k[:-len(".running_mean")] for k in sd if k.endswith(".running_mean")
                     and not any(k.startswith(u + ".") for u in self._unused)]
        self._plain = [k for k in sd if ".conv_offset_mask." in k or ".up_" in k]
        dev = next(model.parameters()).device
        if bn == "batch":
            # the reference's own tensors: parameters under `ref`, the running statistics and counters as buffers
            convs = [_conv_of_bn(b) for b in self._bns]
            self._ref_params = [c + ".weight" for c in convs] + [c + ".bias" for c in convs if c + ".bias" in sd] + \
                               [b + leaf for b in self._bns for leaf in (".weight", ".bias")] + list(self._plain)
            self._ref_buffers = [b + leaf for b in self._bns for leaf in (".running_mean", ".running_var", ".num_batches_tracked") if b + leaf in sd]
            self.ref = nn.ParameterDict()
            for key in self._ref_params:
                self.ref[_name(key)] = nn.Parameter(sd[key].detach().clone().to(dev))
            for key in self._ref_buffers:
                self.register_buffer(_name(key), sd[key].detach().clone().to(dev))
        else:
            self.folded = nn.ParameterDict()
            for key, t in self._fold_all(sd).items():
                self.folded[_name(key)] = nn.Parameter(t.to(dev))
        for head in model.heads:
            self.add_module(head, model._modules[head])

    @property
    def model(self):
        return self._model

    # ---- folding and its inverse -----------------------------------------------------------------------------------------------------
    def _scales(self, sd):
        return {bn: sd[bn + ".weight"].detach().double().cpu() / torch.sqrt(sd[bn + ".running_var"].detach().double().cpu() + arch.BN_EPS)
                for bn in self._bns}

    def _fold_all(self, sd):
        """Reference-keyed tensors -> {'<conv>.weight' / '<conv>.bias': folded fp32 tensor on the CPU} + the plain trained tensors."""
        from .weights import PackedWeights
        pw = PackedWeights.from_tensors({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked") and torch.is_tensor(v)}, "f32", "cpu")
        for bn, s in self._scales(sd).items():
            if bool((s == 0).any()):
                raise ValueError("TrainableDLASeg: the folded scale of BatchNorm %r is 0 for %d channels: the fold could not be undone"
                                 % (bn, int((s == 0).sum())))
        out = {}
        for bn in self._bns:
            conv = _conv_of_bn(bn)
            w, b = pw._fold(pw.sd[conv + ".weight"], pw.sd.get(conv + ".bias"), bn)
            out[conv + ".weight"], out[conv + ".bias"] = w.contiguous(), b.contiguous()
        for k in self._plain:
            out[k] = pw.sd[k].clone().contiguous()
        return out

    def _p(self, key):
        return self.ref[_name(key)] if self.bn == "batch" else self.folded[_name(key)]

    def _b(self, key):
        return self._buffers[_name(key)]

    @staticmethod
    def _unfold(w, b, s, b0, mean):
        """Folded (W', b') -> (conv.weight, BatchNorm bias) for the scale s, the stored conv bias b0 and the running mean (fp64 inside)."""
        w, b = w.detach().double().cpu(), b.detach().double().cpu()
        return (w / s.view(-1, 1, 1, 1)).float(), (b - (b0 - mean) * s).float()

    def _export_of(self, sd, get):
        """{reference key: exported tensor on the CPU} of the folded tensors `get(key)` against the BatchNorm tensors of `sd`."""
        out = {}
        scales = self._scales(sd)
        for bn in self._bns:
            conv = _conv_of_bn(bn)
            b0 = sd[conv + ".bias"].detach().double().cpu() if conv + ".bias" in sd else torch.zeros_like(scales[bn])
            out[conv + ".weight"], out[bn + ".bias"] = self._unfold(get(conv + ".weight"), get(conv + ".bias"), scales[bn], b0,
                                                                    sd[bn + ".running_mean"].detach().double().cpu())
        for k in self._plain:
            out[k] = get(k).detach().float().cpu().clone()
        return out

    def export_state_dict(self):
        """The reference's state_dict with the trained values: BatchNorm tensors kept, every fold undone -- conv.weight = W' / scale, the
        shift b' - (conv.bias - running_mean) * scale in the BatchNorm's bias (conv.bias of a DeformConv stays as stored); running
        statistics and the BatchNorm weights untouched.  Tensors on the model's device."""
        sd = {k: v.detach().clone() for k, v in self._model.state_dict().items()}
        if self.bn == "batch":
            for k in self._ref_params + self._ref_buffers:
                sd[k] = (self._p(k) if k in self._ref_params else self._b(k)).detach().clone().to(sd[k].device)
            return sd
        for k, v in self._export_of(sd, self._p).items():
            sd[k] = v.to(sd[k].device)
        return sd

    def state_dict(self, *a, **kw):
        """`export_state_dict()` plus the folded tensors under `FOLDED_PREFIX + key`: W' -> W' / scale -> W' does not round-trip in
        fp32 (for |scale| > 1 not every W' is the rounded product of an fp32 filter), so a resumed run could not continue with the bits
        of the uninterrupted one from the reference's keys alone.  A reader that only knows the reference's keys ignores the rest."""
        sd = self.export_state_dict()
        if self.bn == "batch":
            return sd
        for name, p in self.folded.items():
            sd[FOLDED_PREFIX + name.replace("__", ".")] = p.detach().clone()
        return sd

    def load_state_dict(self, state_dict, strict=True):
        """The inverse of the export: the reference's keys go into the wrapped model and are folded again.  The folded tensors the dict
        holds beside them are taken instead (bit-exact resume) only if they are complete and their own export reproduces the loaded
        reference tensors bit for bit -- i.e. if both halves come from one state_dict() call; anything else is the plain re-fold."""
        ref = {k: v for k, v in state_dict.items() if not k.startswith(FOLDED_PREFIX)}
        ret = self._model.load_state_dict(ref, strict=strict)
        loaded = self._model.state_dict()
        if self.bn == "batch":
            with torch.no_grad():
                for k in self._ref_params + self._ref_buffers:
                    dst = self._p(k) if k in self._ref_params else self._b(k)
                    dst.copy_(loaded[k].to(dst.device))
            return ret
        folded = self._fold_all(loaded)
        kept = {k: state_dict.get(FOLDED_PREFIX + k) for k in folded}
        if all(v is not None and tuple(v.shape) == tuple(folded[k].shape) for k, v in kept.items()):
            again = self._export_of(loaded, lambda k: kept[k].detach().float())
            if all(torch.equal(v, loaded[k].detach().float().cpu()) for k, v in again.items()):
                folded = {k: v.detach().float() for k, v in kept.items()}
        with torch.no_grad():
            for key, t in folded.items():
                self._p(key).copy_(t.to(self._p(key).device))
        return ret

    def _apply(self, fn, *a, **kw):
        self._model._apply(fn, *a, **kw)
        return super()._apply(fn, *a, **kw)

    def sync(self):
        """Load the export into the wrapped model (drops its packed engine): inference, MultiPoseDetector and val() see the trained weights."""
        self._model.load_state_dict(self.export_state_dict())
        return self._model

    # ---- the graph (oracle/dla.py follows the same reference lines) ----------------------------------------------------------------------
    def _bn(self, x, key, res=None, relu=False):
        """BatchNorm `key` (+ res) (+ ReLU) on the batch's statistics in train(), the running ones in eval()."""
        if self.training and key + ".num_batches_tracked" in self._ref_buffers:
            self._b(key + ".num_batches_tracked").add_(1)
        return bn_ops.batch_norm_autograd(x, self._p(key + ".weight"), self._p(key + ".bias"), self._b(key + ".running_mean"),
                                          self._b(key + ".running_var"), self.training, arch.BN_MOMENTUM, arch.BN_EPS, res, relu)

    def _cb(self, x, conv, stride=1, padding=0, res=None, relu=False):
        if self.bn == "batch":
            y = conv2d_autograd(x, self._p(conv + ".weight"), None, stride, padding, 1, None, False)
            return self._bn(y, _bn_of_conv(conv), res, relu)
        return conv2d_autograd(x, self._p(conv + ".weight"), self._p(conv + ".bias"), stride, padding, 1, res, relu)

    def _block(self, x, p, stride, residual=None):
        if residual is None:
            residual = x
        y = self._cb(x, p + ".conv1", stride, 1, None, True)
        return self._cb(y, p + ".conv2", 1, 1, residual, True)

    def _tree(self, x, p, levels, cin, cout, stride, level_root, children=None, bottom=None):
        children = [] if children is None else children
        if bottom is None:
            bottom = max_pool2_autograd(x) if stride > 1 else x
        if level_root:
            children.append(bottom)
        if levels == 1:
            residual = self._cb(bottom, p + ".project.0") if cin != cout else bottom
            x1 = self._block(x, p + ".tree1", stride, residual)
            x2 = self._block(x1, p + ".tree2", 1)
            return self._cb(torch.cat([x2, x1] + children, 1), p + ".root.conv", relu=True)      # (residual_root = False in dla34)
        # (the inner tree pools the same x again in the reference: the same values, so one pool serves both uses)
        x1 = self._tree(x, p + ".tree1", levels - 1, cin, cout, stride, False, None, bottom)
        children.append(x1)
        return self._tree(x1, p + ".tree2", levels - 1, cout, cout, 1, False, children)

    def _deform_conv(self, x, p):
        w, b = self._p(p + ".conv.weight"), self._p(p + ".conv.bias")
        batch = self.bn == "batch"
        if not self.use_dcn:
            if batch:
                return self._bn(conv2d_autograd(x, w, b, 1, 1, 1, None, False), p + ".actf.0", None, True)
            return conv2d_autograd(x, w, b, 1, 1, 1, None, True)
        B, _, H, W = x.shape
        x = x.contiguous()                                   # (the DeformConv operator and its backward are NCHW)
        zero = torch.zeros(B, 18, H, W, dtype=torch.float32, device=x.device)
        one = torch.ones(B, 9, H, W, dtype=torch.float32, device=x.device)
        # TrainableDCN.forward: conv_offset_mask as the operator itself at zero offsets and a unit mask, chunk / cat / sigmoid in torch
        out = dcn_v2_conv_autograd(x, zero, one, self._p(p + ".conv.conv_offset_mask.weight"), self._p(p + ".conv.conv_offset_mask.bias"),
                                   (1, 1), (1, 1), (1, 1), 1)
        o1, o2, mask = torch.chunk(out, 3, dim=1)
        y = dcn_v2_conv_autograd(x, torch.cat((o1, o2), dim=1), torch.sigmoid(mask), w, b, (1, 1), (1, 1), (1, 1), 1)
        return self._bn(y, p + ".actf.0", None, True) if batch else torch.relu(y)

    def _ida_up(self, layers, p, startp, endp):
        for i in range(startp + 1, endp):
            k = i - startp
            w = self._p("%s.up_%d.weight" % (p, k))
            y = self._deform_conv(layers[i], "%s.proj_%d" % (p, k))
            s = up_add_autograd(y, w, layers[i - 1], w.shape[2] // 2)
            layers[i] = self._deform_conv(s, "%s.node_%d" % (p, k))

    def features(self, x):
        """The [B,64,H/4,W/4] map the heads read (channels_last)."""
        if not x.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 32 or x.shape[3] % 32 or x.shape[2] < 64 or x.shape[3] < 64:
            raise RuntimeError("TrainableDLASeg: input must be [B,3,H,W] with H, W multiples of 32, at least 64; got %s" % (tuple(x.shape),))
        x = x.float()
        x = self._cb(x, "base.base_layer.0", 1, 3, None, True)
        x = self._cb(x, "base.level0.0", 1, 1, None, True)
        layers = [x]
        x = self._cb(x, "base.level1.0", 2, 1, None, True)
        layers.append(x)
        for lv in range(2, 6):
            x = self._tree(x, "base.level%d" % lv, arch.LEVELS[lv], arch.CHANNELS[lv - 1], arch.CHANNELS[lv], 2, lv > 2)
            layers.append(x)
        first, last = 2, 5                                   # down_ratio 4, last_level 5 (models/model.py:501-516)
        out = [layers[-1]]
        for i in range(len(layers) - first - 1):
            self._ida_up(layers, "dla_up.ida_%d" % i, len(layers) - i - 2, len(layers))
            out.insert(0, layers[-1])
        y = list(out[:last - first])
        self._ida_up(y, "ida_up", 0, len(y))
        return y[-1].contiguous(memory_format=torch.channels_last)

    def head_params(self):
        return {h: (self._modules[h]._modules["0"].weight, self._modules[h]._modules["0"].bias,
                    self._modules[h]._modules["2"].weight, self._modules[h]._modules["2"].bias) for h in self._model.heads}

    def forward(self, x):
        return [heads_autograd(self.features(x), self.head_params())]
