"""BN-folded, re-laid-out filter banks of the launch plans (`PackedWeights`) and the operand formats they are stored in.

Every layout has ONE routine here (the zero-padded [rows][taps][Cin] bank, the offset/mask row permutation of the fused DeformConv,
the 7x7 stem bank, level0's five tap pairs, the "f16x3" split-and-scale store); the pack methods of `PackedWeights` combine them
and cache what they return in `PackedWeights.t` under a key per (method, arguments)."""
import numpy as np
import torch

from . import _lib, arch, arch_hg, arch_res

_TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f16x3": torch.float32}
LOWP = ("bf16", "f16")      # the 2-byte plans: same kernels, lowering and tile choices; "f16" = BASELINE configs[4]'s arithmetic


def _t(v):
    return v.detach().float().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v)).float()


def x3_exp(w):
    """Exponent e of the power-of-two pre-scale of an "f16x3" filter bank: 2^e * max|w| lands in [2^13, 2^14), so the fp16 hi terms stay
    far below 65504 and the lo terms (~2^-12 of the value) of every filter above 2^-16 of the largest are NORMAL fp16 numbers -- an
    unscaled 0.05 has a subnormal lo term (3e-8 absolute = 2^-20.7 relative, five times the 2^-23 of the split itself).  The kernels
    multiply their accumulators by 2^-e, which is exact (h3d_op.wexp)."""
    m = float(w.abs().max())
    if not (m > 0.0) or not np.isfinite(m):
        return 0
    return int(max(-60, min(60, 13 - int(np.floor(np.log2(m))))))


def x3_split(w):
    """fp32 filters [..., K] (K % 8 == 0: the contraction index, 8 consecutive elements = one MFMA fragment of a lane) -> the
    operand format of the "f16x3" plans (csrc/common.h ET<x3_t>): per group of 8 elements the 8 fp16 high terms hi = fp16(x)
    followed by the 8 fp16 low terms lo = fp16(x - hi) (round to nearest even), in the 32 bytes the 8 fp32 values occupied --
    returned as a float32-typed tensor of the same shape (raw bytes, not numbers)."""
    w = w.float().contiguous()
    K = w.shape[-1]
    assert K % 8 == 0, K
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)
    g = torch.stack([hi.reshape(-1, K // 8, 8), lo.reshape(-1, K // 8, 8)], dim=2)            # [rows, K/8, 2, 8]
    return g.reshape(-1, 2 * K).contiguous().view(torch.float32).reshape(w.shape)


def heads_k_perm(hc):
    """K order of a fused head's 1x1 filters (csrc/heads.hip): within every 32-channel group, position h*16 + r holds channel
    (r&3) + 8*(r>>2) + 4*h, the MFMA accumulator row order."""
    return torch.tensor([g * 32 + (r & 3) + 8 * (r >> 2) + 4 * h
                         for g in range(hc // 32) for h in range(2) for r in range(16)])


def pack_head_3x3(w):
    """[head_conv,64,3,3] -> [head_conv][9][64] (PackedWeights.fused_heads and h3d_amd.heads.heads_autograd)."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1])


def pack_head_1x1(w, b, perm):
    """[C,head_conv,1,1], [C] -> ([96 rows][head_conv] with K in `perm` order, [96]), zero beyond C; on the tensors' device."""
    c, hc = w.shape[0], w.shape[1]
    w2 = torch.zeros(96, hc, dtype=w.dtype, device=w.device)
    w2[:c] = w.reshape(c, hc)[:, perm.to(w.device)]
    b2 = torch.zeros(96, dtype=b.dtype, device=b.device)
    b2[:c] = b
    return w2, b2


def _rows128(cout):
    return ((cout + 127) // 128) * 128


def _bank(w, b, rows):
    """[Cout,Cin,kh,kw], [Cout] -> ([rows][kh*kw][Cin], [rows]) fp32, zero beyond Cout."""
    co, ci, kh, kw = w.shape
    wp = torch.zeros(rows, kh * kw, ci)
    wp[:co] = w.permute(0, 2, 3, 1).reshape(co, kh * kw, ci)
    bp = torch.zeros(rows)
    bp[:co] = b
    return wp, bp


def _offset_bank(w, b, rows):
    """conv_offset_mask [27,Cin,3,3], [27] spread over 32 MFMA rows so that accumulator half h of a pixel owns whole (dh, dw, mask)
    triples (csrc/dcn3.hip): value i = 3u + c of half h sits in row (i&3) + 8*(i>>2) + 4*h; half 0 holds taps 0..4, half 1 taps 5..8.
    -> ([rows][9][Cin] (32 used), [32]) fp32."""
    ci = w.shape[1]
    wp = torch.zeros(rows, 9, ci)
    bp = torch.zeros(32)
    for tap in range(9):
        hh, u = (0, tap) if tap < 5 else (1, tap - 5)
        for c, ch in enumerate((2 * tap, 2 * tap + 1, 18 + tap)):
            i = 3 * u + c
            row = (i & 3) + 8 * (i >> 2) + 4 * hh
            wp[row] = w[ch].permute(1, 2, 0).reshape(9, ci)
            bp[row] = b[ch]
    return wp, bp


def _stem_bank(w):
    """7x7 stem filters [Cout,3,7,7] -> [Cout][7 dy][32] with k = dx*4 + c (zero for dx = 7 and c = 3)."""
    co = w.shape[0]
    wp = torch.zeros(co, 7, 8, 4)
    wp[:, :, :7, :3] = w.permute(0, 2, 3, 1)          # [o][dy][dx][c]
    return wp.reshape(co, 7, 32)


def _level0_bank(w):
    """level0's 3x3 filters [16,16,3,3] as five tap pairs [5][16][32] (csrc/stem3.hip): k = (tap % 2) * 16 + c of pair tap // 2."""
    t = torch.zeros(5, 16, 2, 16)
    wt = w.permute(0, 2, 3, 1).reshape(16, 9, 16)                                    # [o][tap][c]
    for tap in range(9):
        t[tap // 2, :, tap % 2, :] = wt[:, tap, :]
    return t.reshape(5, 16, 32)


class PackedWeights:
    """BN-folded, re-laid-out weights on the device (built once per state_dict/dtype)."""

    def __init__(self, state_dict, heads, use_dcn, dtype, device, head_conv=256, arch_name="dla34"):
        self.heads, self.use_dcn, self.dtype, self.device = dict(heads), use_dcn, dtype, device
        self.head_conv = head_conv
        self.arch = arch_name
        self.sd = {k: _t(v) for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
        shapes = (arch_hg.state_dict_shapes(heads) if arch_name == "hourglass" else
                  arch_res.state_dict_shapes(heads, head_conv) if arch_name == "resdcn101" else
                  arch.state_dict_shapes(heads, use_dcn, head_conv))
        missing = [k for k in shapes
                   if not k.endswith("num_batches_tracked") and k not in self.sd]
        if missing:
            raise KeyError("state_dict is missing %d keys, e.g. %s" % (len(missing), missing[:3]))
        self.t = {}
        self.wexp = {}              # f16x3: device pointer of a packed filter bank -> its power-of-two pre-scale exponent (x3_exp; h3d_op.wexp)
        self.dcn_variant = {}       # DeformConv layer (state_dict prefix) -> csrc/dcn3.hip variant bits (DLAEngine.calibrate_dcn_margins)
        if arch_name == "resdcn101":
            # the DCN of up-sampling stage i is `deconv_layers.{6i}` (weight, bias, conv_offset_mask.*) followed by the
            # BatchNorm `deconv_layers.{6i+1}`: alias them to the key pattern the DeformConv lowering reads
            # (`p.conv.*`, `p.actf.0.*` of the DLA neck, model.py:346-362)
            for i in range(len(arch_res.DECONV)):
                p, bn = "deconv_layers.%d" % (6 * i), "deconv_layers.%d" % (6 * i + 1)
                for a, b in ((".conv.weight", ".weight"), (".conv.bias", ".bias"),
                             (".conv.conv_offset_mask.weight", ".conv_offset_mask.weight"),
                             (".conv.conv_offset_mask.bias", ".conv_offset_mask.bias")):
                    self.sd[p + a] = self.sd[p + b]
                for leaf in ("weight", "bias", "running_mean", "running_var"):
                    self.sd["%s.actf.0.%s" % (p, leaf)] = self.sd["%s.%s" % (bn, leaf)]

    @classmethod
    def from_tensors(cls, tensors, dtype, device):
        """A packer over a bare {name: tensor} table (no architecture key check): the per-op tests pack ad-hoc layers with the
        same `conv` / `offset_conv` / `dcn_stream` routines as the network."""
        self = cls.__new__(cls)
        self.heads, self.use_dcn, self.dtype, self.device = {}, True, dtype, torch.device(device)
        self.head_conv, self.arch = 0, "bare"
        self.sd = {k: _t(v) for k, v in tensors.items()}
        self.t = {}
        self.wexp = {}
        self.dcn_variant = {}
        return self

    @property
    def dcn_wide(self):
        return {p for p, v in self.dcn_variant.items() if v == _lib.OPF_DCN_STREAM_WIDE_MARGIN}

    def _fold(self, w, b, bn):
        """conv(+bias) followed by eval BatchNorm `bn` -> (w', b')."""
        if b is None:
            b = torch.zeros(w.shape[0])
        if bn is None:
            return w, b
        sd = self.sd
        scale = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + arch.BN_EPS)
        w2 = (w.double() * scale.view(-1, 1, 1, 1)).float()
        b2 = ((b.double() - sd[bn + ".running_mean"].double()) * scale + sd[bn + ".bias"].double()).float()
        return w2, b2

    def _folded(self, wkey, bkey, bn):
        return self._fold(self.sd[wkey], self.sd[bkey] if bkey else None, bn)

    def _dev(self, t):
        return t.contiguous().to(self.device)

    def _store(self, w, td=None):
        """fp32 filter bank -> its device tensor: cast to `td` (default: the plan's storage type), or in an f16x3 plan the (hi | lo)
        fp16 terms of w * 2^e (x3_split, x3_exp).  The exponent lands in `self.wexp` under the tensor's device pointer (0 otherwise)."""
        e = x3_exp(w) if self.dtype == "f16x3" else 0
        t = self._dev(x3_split(w * 2.0 ** e) if self.dtype == "f16x3" else w.to(td or _TORCH_DT[self.dtype]))
        self.wexp[t.data_ptr()] = e
        return t

    def conv(self, wkey, bkey=None, bn=None, pad_cout_to=None, as_half=False):
        """-> (packed weights [rows][kh*kw][Cin], bias fp32 [rows], Cout, Cin, k).
        as_half: store fp16 instead of bf16 (DCN layers in bf16 mode, csrc/dcn2.hip)."""
        key = ("conv", wkey, bn, pad_cout_to, as_half)
        if key not in self.t:
            w, b = self._folded(wkey, bkey, bn)
            cout = pad_cout_to or w.shape[0]
            rows = _rows128(cout)
            wp, bp = _bank(w, b, rows)
            td = torch.float16 if (as_half and self.dtype in LOWP) else _TORCH_DT[self.dtype]
            self.t[key] = (self._store(wp, td), self._dev(bp), cout, w.shape[1], w.shape[2], rows)
        return self.t[key]

    def conv_stream(self, wkey, bkey=None, bn=None):
        """3x3 filter bank as the stage-major LDS image of csrc/conv2.hip: [Cin/16][G][32 rows][19 slots][8]
        bf16, slot 2*tap+h = input channels 16*stage + 8h..8h+7 of tap `tap`, slot 18 zero; G = Cout/32
        row groups padded to a multiple of 4.  -> (image, bias fp32 [32 G], Cout, Cin, rows = 32 G)."""
        key = ("conv_stream", wkey, bn)
        if key not in self.t:
            w, b = self._folded(wkey, bkey, bn)
            co, ci, kh, kw = w.shape
            assert kh == 3 and kw == 3 and ci % 16 == 0
            rows = _rows128(co)
            wp, bp = _bank(w, b, rows)
            self.t[key] = (self._dev(self._stage_image(wp).to(_TORCH_DT[self.dtype])), self._dev(bp), co, ci, rows)
        return self.t[key]

    @staticmethod
    def _stage_image(wp, ck=16):
        """[rows (multiple of 32)][9][Cin] -> stage-major LDS image [Cin/ck][rows/32][32][9*ck/8 + 1 slots][8]:
        slot tap*ck/8 + j = input channels ck*stage + 8j..8j+7 of tap `tap`, last slot zero (csrc/conv2.hip and
        dcn4.hip: ck = 16; csrc/dcn3.hip WDMA: ck = h3d_dcn_fused_ck)."""
        rows, _, ci = wp.shape
        G, spt = rows // 32, ck // 8
        img = torch.zeros(ci // ck, G, 32, 9 * spt + 1, 8)
        v = wp.reshape(G, 32, 9, ci // ck, spt, 8).permute(3, 0, 1, 2, 4, 5)
        img[:, :, :, :9 * spt] = v.reshape(ci // ck, G, 32, 9 * spt, 8)
        return img

    @staticmethod
    def _stage_image_x3(ws):
        """float32-TYPED split filters [rows (multiple of 32)][9][Cin] (x3_split: per 8 channels 8 hi | 8 lo fp16 terms) -> the stage-major
        LDS image of the f16x3 patch-slot DeformConv (csrc/dcn3.hip WDMA, 16 channels per stage): [Cin/16][rows/32][32][37 slots of 16 B]:
        slot 4 * tap + j = bytes 16 j .. 16 j + 15 of the tap's 64 bytes (channels 16 * stage ... + 15), slot 36 zero -- rows of 592 B."""
        rows, _, ci = ws.shape
        G = rows // 32
        img = torch.zeros(ci // 16, G, 32, 37, 4)
        v = ws.reshape(G, 32, 9, ci // 16, 4, 4).permute(3, 0, 1, 2, 4, 5)
        img[:, :, :, :36] = v.reshape(ci // 16, G, 32, 36, 4)
        return img

    def _dcn_main_bank(self, p):
        """Main filters of DeformConv `p` with its BatchNorm folded -> (bank [rows][9][Cin], bias [rows], Cout, Cin, rows)."""
        w, b = self._folded(p + ".conv.weight", p + ".conv.bias", p + ".actf.0")
        rows = _rows128(w.shape[0])
        return _bank(w, b, rows) + (w.shape[0], w.shape[1], rows)

    def dcn_stream_x3(self, p):
        """Fused DeformConv `p` for the f16x3 patch-slot variant: (main image, offset image, bias [rows | 32], Cout, Cin, rows); the
        power-of-two pre-scale exponents of the two banks land in `self.wexp` under the images' device pointers."""
        key = ("dcn_stream_x3", p)
        if key not in self.t:
            wp, bp, co, ci, rows = self._dcn_main_bank(p)
            wo, bo = _offset_bank(self.sd[p + ".conv.conv_offset_mask.weight"], self.sd[p + ".conv.conv_offset_mask.bias"], 32)
            e, eo = x3_exp(wp), x3_exp(wo)
            wimg = self._dev(self._stage_image_x3(x3_split(wp * 2.0 ** e)))
            woimg = self._dev(self._stage_image_x3(x3_split(wo * 2.0 ** eo)))
            self.t[key] = (wimg, woimg, self._dev(torch.cat([bp, bo])), co, ci, rows)
            self.wexp[wimg.data_ptr()], self.wexp[woimg.data_ptr()] = e, eo
        return self.t[key]

    def dcn_stream(self, p, ck=16):
        """Fused DeformConv `p` packed as fp16 stage-major images of the main and the offset/mask filters, `ck`
        channels per stage (csrc/dcn4.hip: 16; csrc/dcn3.hip WDMA: h3d_dcn_fused_ck)
        -> (main image, offset image, bias [rows | 32], Cout, Cin, rows)."""
        key = ("dcn_stream", p, ck)
        if key not in self.t:
            wp, bp, co, ci, rows = self._dcn_main_bank(p)
            wo, bo = self.offset_conv(p + ".conv.conv_offset_mask.weight", p + ".conv.conv_offset_mask.bias", rows)
            self.t[key] = (self._dev(self._stage_image(wp, ck).to(torch.float16)),
                           self._dev(self._stage_image(wo[:32].float().cpu(), ck).to(torch.float16)),
                           self._dev(torch.cat([bp, bo])), co, ci, rows)
        return self.t[key]

    def dcn_fused(self, p):
        """Fused DeformConv `p` for the register-staged kernel (H3D_OP_DCN_FUSED): `conv(as_half)` and `offset_conv` banks with one
        bias [rows | 32] -> (main bank, offset bank, bias, Cout, Cin, rows)."""
        wp, bp, cout, cin, k, rows = self.conv(p + ".conv.weight", p + ".conv.bias", p + ".actf.0", as_half=True)
        wo, bo = self.offset_conv(p + ".conv.conv_offset_mask.weight", p + ".conv.conv_offset_mask.bias", rows)
        key = ("dcnbias", p)
        if key not in self.t:
            self.t[key] = self._dev(torch.cat([bp.cpu(), bo]))
        return wp, wo, self.t[key], cout, cin, rows

    def stem(self):
        key = ("stem",)
        if key not in self.t:
            w, b = self._folded("base.base_layer.0.weight", None, "base.base_layer.1")
            if self.dtype in LOWP or self.dtype == "f16x3":
                w = _stem_bank(w)       # MFMA stem (csrc/conv.hip stem_mfma_kernel / stem_x3_kernel): [16][7 dy][32] with k = dx*4 + c
            self.t[key] = (self._store(w), self._dev(b))
        return self.t[key]

    def stem_s2(self, wkey, bkey, bn):
        """7x7 stride-2 stem filters [Cout,3,7,7] (+ BatchNorm `bn` folded) for csrc/extra.hip stem_s2_kernel:
        bf16 [Cout][7 dy][32] with k = dx*4 + c (zero for dx = 7 and c = 3), bias fp32 [Cout]."""
        key = ("stem_s2", wkey, bn)
        if key not in self.t:
            w, b = self._folded(wkey, bkey, bn)
            self.t[key] = (self._dev(_stem_bank(w).to(_TORCH_DT[self.dtype])), self._dev(b.float()))
        return self.t[key]

    def stem3(self, proj=False):
        """base_layer + level0 + level1 packed for csrc/stem3.hip: bf16 [16][7][32] | [5][16][32] | [32][9][16] and
        fp32 biases [16 | 16 | 32] (BatchNorm folded).  proj: + level2's `project` 1x1 conv (model.py:202-207) [64][32] and its
        bias [64], for the launch that also produces level2's residual branch."""
        key = ("stem3", proj)
        if key not in self.t and proj:
            flat, bias = self.stem3(False)
            wp, bp = self._folded("base.level2.project.0.weight", None, "base.level2.project.1")      # [64,32,1,1]
            assert tuple(wp.shape) == (64, 32, 1, 1)
            self.t[key] = (self._dev(torch.cat([flat.cpu(), wp.reshape(-1).to(_TORCH_DT[self.dtype])])),
                           self._dev(torch.cat([bias.cpu(), bp.float()])))
        if key not in self.t:
            w0, b0 = self.stem()
            w1, b1 = self._folded("base.level0.0.weight", None, "base.level0.1")       # [16,16,3,3]
            w2, b2 = self._folded("base.level1.0.weight", None, "base.level1.1")       # [32,16,3,3]
            w2t = w2.permute(0, 2, 3, 1).reshape(32, 9, 16)
            flat = torch.cat([w0.cpu().float().reshape(-1), _level0_bank(w1).reshape(-1), w2t.reshape(-1)]).to(_TORCH_DT[self.dtype])
            bias = torch.cat([b0.cpu().float(), b1.float(), b2.float()])
            self.t[key] = (self._dev(flat), self._dev(bias))
        return self.t[key]

    def stem3_x3(self):
        """base_layer + level0 + level1 for csrc/stem3x.hip (f16x3 plans): the three banks of `stem3()` as float32-typed (hi | lo) fp16
        terms per 8 k, each times its own power of two, and fp32 biases [16 | 16 | 32 | 2^-e0, 2^-e1, 2^-e2, 0]."""
        key = ("stem3_x3",)
        if key not in self.t:
            w0, b0 = self._folded("base.base_layer.0.weight", None, "base.base_layer.1")
            w1, b1 = self._folded("base.level0.0.weight", None, "base.level0.1")       # [16,16,3,3]
            w2, b2 = self._folded("base.level1.0.weight", None, "base.level1.1")       # [32,16,3,3]
            banks = (_stem_bank(w0), _level0_bank(w1), w2.permute(0, 2, 3, 1).reshape(32, 9, 16))
            es = [x3_exp(t) for t in banks]
            flat = torch.cat([x3_split(t * 2.0 ** e).reshape(-1) for t, e in zip(banks, es)])
            bias = torch.cat([b0.float(), b1.float(), b2.float(), torch.tensor([2.0 ** -es[0], 2.0 ** -es[1], 2.0 ** -es[2], 0.0])])
            self.t[key] = (self._dev(flat), self._dev(bias))
        return self.t[key]

    def offset_conv(self, wkey, bkey, main_rows):
        """conv_offset_mask packed for the fused DeformConv kernel (csrc/dcn3.hip): the 27 filters in the row order of `_offset_bank`.
        Returns (weights [128 rows][9][Cin] (32 used), permuted bias fp32 [32], on the host)."""
        key = ("offconv", wkey)
        if key not in self.t:
            wp, bp = _offset_bank(self.sd[wkey], self.sd[bkey], 128)              # [27,Cin,3,3], [27]
            self.t[key] = (self._store(wp, torch.float16 if self.dtype in LOWP else torch.float32), bp)
        return self.t[key]

    def fused_heads(self, names=None):
        """Fused-heads pack: 3x3 weights of all heads stacked [nheads*head_conv][9][64]; per head the
        1x1 weights as [96 rows][head_conv] with K re-ordered to the MFMA accumulator row order
        (csrc/heads.hip): within every 32-channel group, position h*16 + r holds channel
        (r&3) + 8*(r>>2) + 4*h."""
        names = tuple(self.heads) if names is None else names
        key = ("heads", names)
        if key not in self.t:
            w1, b1, per = [], [], []
            perm = heads_k_perm(self.head_conv)
            for head in names:
                w1.append(pack_head_3x3(self.sd[head + ".0.weight"]))                      # [hc,64,3,3]
                b1.append(self.sd[head + ".0.bias"])
                w2, b2 = pack_head_1x1(self.sd[head + ".2.weight"], self.sd[head + ".2.bias"], perm)
                per.append((head, self.heads[head], self._store(w2), b2.to(self.device)))
            w1 = self._store(torch.cat(w1))
            e1 = self.wexp[w1.data_ptr()]           # (one exponent for the launch's 3x3 bank; its biases are scaled with it)
            self.t[key] = (w1, self._dev(torch.cat(b1).float() * 2.0 ** e1), per)
        return self.t[key]

    def nearest_up_key(self, c):
        """Nearest-neighbour x2 up-sampling (Hourglass `nn.Upsample(scale_factor=2)`) as the depthwise
        ConvTranspose2d(k=4, s=2, p=1) the up-sample + add kernel evaluates: taps (1..2, 1..2) = 1, the rest 0 --
        output row y reads input row (y + 1 - ky) / 2 for ky = 1 (y even) or 2 (y odd), i.e. row y // 2."""
        key = "__nearest_up2__.%d" % c
        if key not in self.sd:
            w = torch.zeros(c, 1, 4, 4)
            w[:, 0, 1:3, 1:3] = 1.0
            self.sd[key] = w
        return key

    def deconv4_as_conv3(self, wkey, bn):
        """ConvTranspose2d(C, C, 4, stride 2, padding 1, bias=False) + BatchNorm `bn` as ONE 3x3 conv with 4C output
        channels followed by H3D_OP_DEPTH2SPACE: output pixel (2y+py, 2x+px) only sees inputs (y+dy, x+dx) with
        dy in {-1, 0} (py = 0) or {0, 1} (py = 1) through kernel row ky = py + 1 - 2 dy, so group g = 2 py + px of the
        3x3 filters is that 2x2 sub-kernel, zero elsewhere (2.25x the transposed conv's MACs, all of them on the MFMA conv
        kernel).  -> (weight key [4C, C, 3, 3], BatchNorm prefix with the statistics repeated per group)."""
        key, bkey = wkey + "#conv3", bn + "#x4"
        if key not in self.sd:
            w = self.sd[wkey]                                    # [Cin, Cout, 4, 4]
            ci, co = w.shape[0], w.shape[1]
            w3 = torch.zeros(4, co, ci, 3, 3)
            for py in range(2):
                for px in range(2):
                    for dy in ((-1, 0) if py == 0 else (0, 1)):
                        for dx in ((-1, 0) if px == 0 else (0, 1)):
                            w3[2 * py + px, :, :, dy + 1, dx + 1] = w[:, :, py + 1 - 2 * dy, px + 1 - 2 * dx].t()
            self.sd[key] = w3.reshape(4 * co, ci, 3, 3)
            for leaf in ("weight", "bias", "running_mean", "running_var"):
                self.sd["%s.%s" % (bkey, leaf)] = self.sd["%s.%s" % (bn, leaf)].repeat(4)
        return key, bkey

    def im2col_key(self, wkey, kpad=160):
        """[Cout,3,7,7] stem filters as a 1x1 conv over H3D_OP_IM2COL patches: [Cout,kpad,1,1], k = c*49 + ky*7 + kx."""
        key = wkey + "#im2col"
        if key not in self.sd:
            w = self.sd[wkey]
            co, k = w.shape[0], w.shape[1] * w.shape[2] * w.shape[3]
            wp = torch.zeros(co, kpad, 1, 1)
            wp[:, :k, 0, 0] = w.reshape(co, k)
            self.sd[key] = wp
        return key

    def up(self, wkey):
        key = ("up", wkey)
        if key not in self.t:
            w = self.sd[wkey]                               # [C,1,k,k]
            c, _, k, _ = w.shape
            self.t[key] = (self._dev(w.reshape(c, k * k).t()), k)   # [k*k][C] fp32
        return self.t[key]
