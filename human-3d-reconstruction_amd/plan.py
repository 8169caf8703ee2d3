"""The launch plan of one (batch, height, width): the network lowered into an array of `h3d_op` descriptors (include/h3d.h) over
pre-allocated NHWC buffers (`View`s) and the packed weights of `weights.PackedWeights`.

Every op is emitted by `Plan._op` from the Views it reads and writes: the pointers, sizes and channel strides of an op are never
spelled out at a lowering site, which states only what is particular to it (kind, filters, kernel size, stride, epilogue, flags).
The lowering decisions are the switches of `Plan.FLAGS`; two of them mark ops the run loop launches together with their neighbours
(fold_upadd: up-sample + add into its skip's DeformConv; fold_tree_entry: a Tree's max-pool and project conv into its stride-2 conv)."""
import ctypes

import torch

from . import _lib, arch, arch_hg, arch_res
from ._lib import H3dOp
from .weights import _TORCH_DT, LOWP

_H3D_DT = {"bf16": _lib.H3D_BF16, "f16": _lib.H3D_F16, "f32": _lib.H3D_F32, "f16x3": _lib.H3D_F16X3}
DCN_F16IN = _lib.OPF_DCN_STREAM_F16_INPUT         # h3d_op.reserved of a fused DeformConv in a bf16 plan: its input tensor holds fp16 values (csrc/dcn3.hip F16IN)


class View:
    """A [B,H,W,C] tensor living at channel offset `coff` of an NHWC buffer of channel stride `cs`."""
    __slots__ = ("buf", "H", "W", "C", "cs", "coff", "es")

    def __init__(self, buf, H, W, C, cs, coff, es):
        self.buf, self.H, self.W, self.C, self.cs, self.coff, self.es = buf, H, W, C, cs, coff, es

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.coff * self.es

    def slice(self, c0, c):
        assert c0 + c <= self.C
        return View(self.buf, self.H, self.W, c, self.cs, self.coff + c0, self.es)


class Plan:
    """Op array + the buffers it points into, for one (B,H,W)."""

    # lowering switches (DLAEngine mirrors them as attributes; the defaults are the measured-best choices)
    FLAGS = dict(
        fuse_heads=True,       # False: one conv3x3 + conv1x1 launch pair per head (debug/ablation)
        fuse_offsets=True,     # False: conv_offset_mask as its own launch + dcn2_kernel reading NHWC offsets
        stream_convs=True,     # False: 3x3 convs through the register-staged kernel (csrc/conv.hip)
        stream_dcn=False,      # True: 64-channel node DeformConvs through csrc/dcn4.hip (fp16 input, up-sampling folded in): 0.35 ms
                               # per batch-64 step faster while the offsets stay below ~1 px, 5x SLOWER per launch at 2 px
                               # (no patch slots: its LDS is full); default since round 2: csrc/dcn3.hip with patches
        stream_s2=True,        # False: stride-2 3x3 convs (Cin >= 64) through csrc/conv.hip
        stream_dcn3=True,      # ALL remaining fused DeformConvs take their filters by LDS-DMA (csrc/dcn3.hip WDMA: the variants with patches)
        dcn_patches=True,      # False: round 1's WDMA configurations (no patch slots: samples that leave the apron go through pass 2)
        dense_dcn3=True,       # those with <= 64 output channels do: margin-1 apron, two workgroups per CU (csrc/dcn3.hip)
        dense_dcn3_min_tiles=512,   # ... when the layer has at least this many 16x16 tiles (two per CU)
        fuse_upnode=True,      # False: up-sample + add always as its own launch in front of the 64-channel node DeformConvs
        fuse_upnode_min_f=2,   # ... from this up-sampling factor.  Same box, batch 64, up-sampling + node over the five layers:
                               # 1.234 ms as two launches each, 1.194 with the 4x layer folded, 1.156 with all five
        dcn_slots512=0,        # 1: margin 2 on the PACKED apron with 512 patch slots per tile (second 256 filled in a second round per stage)
        dcn_wide_margin=0,     # 1: every fused DeformConv (<= 64-channel workgroups) on the margin-4 packed apron (csrc/dcn3.hip PK): slower
                               # while the offsets stay small (more apron to stage), far faster once many samples of a tile leave a
                               # margin-2 apron; per-layer choices from a calibration batch: DLAEngine.calibrate_dcn_margins
        node_f16=True,         # bf16 plans: the up-sample + add kernel writes the `node` DeformConvs' input as fp16 (only they read it) and those
                               # DeformConvs run csrc/dcn3.hip's fp16-input variants (no conversion while the apron is staged)
        share_pool=True,       # False: level3/level4 max-pool their input twice (outer and inner tree), as the reference does
        fuse_stem=True,        # False: base_layer, level0 and level1 as three launches
        fuse_stem_proj=False,  # True: the fused stem launch also max-pools its output and applies level2's `project` conv (the residual branch
                               # of level2's first block: nothing else reads the pooled map): two HBM-bound launches and a 67 MB map less,
                               # bit-identical -- and measured a wash (round 4, same process, batch 64): the stem launch goes from 0.455 to
                               # 0.622 ms for the 0.113 ms of the two launches it absorbs (0.912 with the 1x1 conv on the waves that pool,
                               # 0.710 with its filters fetched per tile): the kernel sits at its 128-VGPR cap (52 more bytes of scratch)
                               # and its P3 phase, which every wave of the workgroup waits for, gets 16 cross-lane exchanges longer
        mixed_heads=0,         # 1: all heads in ONE launch (the kernel picks the 1 / 2 / 3-tile body per head; the halo tile is staged once).
                               # Measured (batch 64, same process / same box): the heads take 1.838 instead of 1.913 ms, but the STEP with
                               # three steps in flight gets 0.4 % slower (8424 / 8465 vs 8461 / 8499 images/s): the merged kernel
                               # needs 256 VGPRs, two of its waves fill a SIMD's register file, and the other streams' small kernels
                               # (up-sample + add, max-pool, gathers), which the 198-register narrow-heads launch lets onto its
                               # CUs, have to wait
        wide_heads_m2=0,       # 3: heads wider than 32 channels share one launch (measured: no gain)
        x3_dcn_patches=True,      # f16x3 plans: the patch-slot DeformConv variant (filters by LDS-DMA, far samples as patch pixels) for layers with
                                  # Cin % 32 == 0; False: the f32 plan's register-staged tiles, every far sample through pass 2
        stem_s2_direct=True,      # bf16 plans of the other backbones: the 7x7 stride-2 stem conv itself instead of im2col + 1x1 conv
        conv1x1_th16_min_cin=0,   # > 0: 1x1 convs with at least this many input channels (and > 32 outputs) use 16-row tiles
        lower_heads=True,         # False: the plan ends at the 64-channel feature map `Plan.feat` (no heads ops, no head outputs): the
                                  # frozen backbone of h3d_amd.heads.TrainableHeads
        split_heads=(),           # a tuple of head names (fused heads only): the heads ops come in two parts.  The EAGER part, one launch for
                                  # these heads (the maps a decode reads whole), ends the prefix `run_eager` executes; the DEFERRED part,
                                  # the other heads in the default groups, follows it (`run_deferred`).  `run_sparse` evaluates the
                                  # deferred heads (without the peak_heads) at listed positions only (h3d_heads_sparse).  `run` still runs everything:
                                  # same instantiations, same per-head arithmetic, the default lowering's maps bit for bit
        fold_upadd=False,         # True (MultiPoseDetector sets it for DLA-34 bf16 / f16): every IDAUp lowers its proj DeformConvs first, and where the
                                  # skip of an up-sample + add is the output of the node DeformConv lowered just before it, read by nothing else
                                  # (dla_up.ida_2 steps 2 and 3, ida_up steps 1 and 2: 64 channels at a quarter of the input size), the op
                                  # carries H3D_OPF_UPADD_FOLDED: h3d_run_ops launches the pair as one kernel whose epilogue adds the up-sampled
                                  # map to each vector before it is stored (csrc/epilogue.h tile_epilogue_lds_fold).  The node's own output
                                  # buffer is then never written; same bits downstream.  Off by default: the default lowering is pinned
        fold_tree_entry=False,    # True (MultiPoseDetector sets it for DLA-34 bf16 / f16; needs share_pool): the entry of a Tree -- the max-pool of x,
                                  # `project` of the pooled map and the stride-2 conv1 of x, lowered next to each other in this order -- carries
                                  # H3D_OPF_TREE_ENTRY on all three ops (levels 2 to 5): h3d_run_ops launches the triple as one kernel (the pool is
                                  # the maximum of four taps conv1 holds, project one more MFMA chain per stage); same bits in all three maps.
                                  # Level 2's conv1 (32 -> 64) then runs on csrc/conv2.hip's one-slot 64-channel tile instead of csrc/conv.hip
                                  # (same accumulation order, same bits), and its pooled map, which nothing else reads, is not written.
                                  # Off by default: the default lowering is pinned
        peak_heads=(),            # with split_heads: heads (of split_heads or not) that are NOT read whole either, but at a second, longer position
                                  # list (multi_pose_decode reads `hp_offset` at the 17 x K key-point peaks).  They leave the eager launch
                                  # for the deferred groups, in their default place, and join the sparse op, where `run_sparse_lists`
                                  # evaluates them at that second list in the same launch as the centre heads.  Alone: no effect
    )

    def __init__(self, pw, B, H, W, **flags):
        unknown = set(flags) - set(self.FLAGS)
        if unknown:
            raise TypeError("unknown lowering flags: %s" % sorted(unknown))
        for k, v in self.FLAGS.items():
            setattr(self, k, flags.get(k, v))
        self.stream_s2_min_cin = 64     # measured: the 32-channel stride-2 layer is faster on csrc/conv.hip (0.136 vs 0.165 ms)
        if pw.arch == "hourglass" and (H % 128 or W % 128):
            raise RuntimeError("Hourglass-104: input height/width must be multiples of 128 (got %dx%d): the published test "
                               "code pads to (x|127)+1" % (H, W))
        if H % 32 or W % 32:
            raise RuntimeError("input height/width must be multiples of 32 (got %dx%d): the reference pads "
                               "to (x|31)+1 (datasets/coco.py:160-163)" % (H, W))
        self.pw, self.B, self.H, self.W = pw, B, H, W
        self.dtype = pw.dtype
        self.es = 2 if pw.dtype in LOWP else 4
        self.ops = []
        self.dcn_layers = []    # (state_dict prefix, op index) of the fused DeformConvs
        self.keep = []          # tensors the ops point into
        self.images = torch.empty(B, 3, H, W, dtype=torch.float32, device=pw.device)
        self.image = View(self.images, H, W, 3, 3, 0, 4)       # the NCHW fp32 batch as the stem ops describe it (Cin = in_cs = 3)
        self.outputs = {}
        self.all_outputs = None         # Hourglass: one head dict per stack (outputs = the last one)
        self._out_at = {}               # head -> where its output pointer lives: an op index, or (heads descriptor, slot)
        self.n_eager = None             # split_heads: ops[:n_eager] = backbone + eager heads, ops[n_eager:] = the deferred heads
        self.sparse_op = None           # ... and the deferred heads as ONE op outside the array, for h3d_heads_sparse
        self._sparse_at = {}            # ... head -> (its descriptor, slot)
        self.sparse_masks = (0, 0)      # ... descriptor slots of the heads read at the centres | at the peak list (peak_heads)
        self.pending = None             # an event behind launches another stream issued into this plan's maps (detector.LazyHeads)
        if pw.arch == "hourglass":
            self._lower_hourglass()
        elif pw.arch == "resdcn101":
            self._lower_resdcn()
        else:
            self._lower()
        self.op_array = (H3dOp * len(self.ops))(*self.ops)

    # -- buffer / op helpers --------------------------------------------------------------------
    def _alloc(self, H, W, C, dtype=None):
        td = _TORCH_DT[self.dtype] if dtype is None else dtype
        buf = torch.empty(self.B, H, W, C, dtype=td, device=self.pw.device)
        self.keep.append(buf)
        return View(buf, H, W, C, C, 0, buf.element_size())

    def _new_output(self, head, c, H, W, at):
        """A head output, contiguous NCHW fp32 (the reference's head layout), as the View an op writes: C = channel stride = c.
        `at`: where the op array will hold its pointer (what `retarget_outputs` rewrites)."""
        o = torch.empty(self.B, c, H, W, dtype=torch.float32, device=self.pw.device)
        self.outputs[head], self._out_at[head] = o, at
        return View(o, H, W, c, c, 0, 4)

    def _op(self, kind, x=None, out=None, x2=None, emit=True, **kw):
        """Append one op and return its index (emit=False: return the op itself, outside the array).  The Views give the geometry and the pointers: `x` -> in_, H, W, Cin, in_cs; `out` ->
        out, Ho, Wo, Cout, out_cs; `x2` (residual, skip, offsets) -> in2, in2_cs; `kw`: every other field, by its h3d_op name."""
        op = H3dOp()
        op.kind, op.dtype, op.B = kind, _H3D_DT[self.dtype], self.B
        if x is not None:
            op.in_, op.H, op.W, op.Cin, op.in_cs = x.ptr, x.H, x.W, x.C, x.cs
        if out is not None:
            op.out, op.Ho, op.Wo, op.Cout, op.out_cs = out.ptr, out.H, out.W, out.C, out.cs
        if x2 is not None:
            op.in2, op.in2_cs = x2.ptr, x2.cs
        for k, v in kw.items():
            setattr(op, k, v)
        if not emit:
            return op
        self.ops.append(op)
        return len(self.ops) - 1

    def conv(self, x, wkey, out=None, bkey=None, bn=None, stride=1, relu=True, res=None, out_mode=_lib.OUT_NHWC,
             pad_cout_to=None, entry=False):
        """out_mode OUT_NCHW_F32: `out` is the View of a head output (`_new_output`).
        entry: the stride-2 conv1 of a Tree entry under fold_tree_entry.  It goes through csrc/conv2.hip below stream_s2_min_cin channels
        too, and with fewer than 128 output channels on that kernel's one-slot 64-channel tile: the tile that has the fused twin (alone it
        takes what csrc/conv.hip takes for level 2: 0.114 against 0.111 ms at batch 64)."""
        wshape = self.pw.sd[wkey].shape
        if (self.stream_convs and self.pw.dtype in LOWP and wshape[2] == 3 and wshape[1] % 16 == 0
                and (stride == 1 or (stride == 2 and (wshape[1] >= self.stream_s2_min_cin or entry) and self.stream_s2))
                and out_mode == _lib.OUT_NHWC and pad_cout_to is None):
            tile = _lib.TUNE_CONV_STREAM_TILE(4, 2, 4) if entry and stride == 2 and 64 <= wshape[0] < 128 else 0
            return self._conv_stream(x, wkey, out, bkey, bn, relu, res, stride, reserved=tile)
        wp, bp, cout, cin, k, rows = self.pw.conv(wkey, bkey, bn, pad_cout_to)
        assert cin == x.C, (wkey, cin, x.C)
        Ho = (x.H + 2 * (k // 2) - k) // stride + 1
        Wo = (x.W + 2 * (k // 2) - k) // stride + 1
        if out_mode == _lib.OUT_NHWC_F32:
            out = self._alloc(Ho, Wo, cout, torch.float32)
        elif out is None:
            out = self._alloc(Ho, Wo, cout)
        assert (out.H, out.W, out.C) == (Ho, Wo, cout), (wkey, out.H, out.W, out.C, Ho, Wo, cout)
        tune = 0
        if (k == 1 and stride == 1 and self.conv1x1_th16_min_cin and cin >= self.conv1x1_th16_min_cin and cin % 64 == 0
                and cout > 32 and self.pw.dtype in LOWP):
            tune = _lib.TUNE_CONV_1X1_TILE(4 if cout > 64 else 2, 16)       # csrc/conv.hip tuning override: MT, TH = 16
        self._op(_lib.OP_CONV, x, out, res, w=wp.data_ptr(), bias=bp.data_ptr(), ksize=k, stride=stride, relu=int(relu),
                 out_mode=out_mode, wrows=rows, reserved=tune, wexp=self.pw.wexp.get(wp.data_ptr(), 0))
        return out

    def _conv_stream(self, x, wkey, out, bkey, bn, relu, res, stride=1, reserved=0):
        """3x3 conv (stride 1 or 2) through the LDS-DMA kernel (csrc/conv2.hip)."""
        wimg, bp, cout, cin, rows = self.pw.conv_stream(wkey, bkey, bn)
        assert cin == x.C, (wkey, cin, x.C)
        Ho, Wo = (x.H - 1) // stride + 1, (x.W - 1) // stride + 1
        if out is None:
            out = self._alloc(Ho, Wo, cout)
        assert (out.H, out.W, out.C) == (Ho, Wo, cout), (wkey, out.H, out.W, out.C)
        self._op(_lib.OP_CONV_STREAM, x, out, res, w=wimg.data_ptr(), bias=bp.data_ptr(), ksize=3, stride=stride, relu=int(relu),
                 out_mode=_lib.OUT_NHWC, wrows=rows, reserved=reserved)
        return out

    def dcn(self, x, om, wkey, bkey, bn):
        wp, bp, cout, cin, k, rows = self.pw.conv(wkey, bkey, bn, as_half=True)
        assert cin == x.C and k == 3
        out = self._alloc(x.H, x.W, cout)
        self._op(_lib.OP_DCN, x, out, om, w=wp.data_ptr(), bias=bp.data_ptr(), ksize=3, stride=1, relu=1, out_mode=_lib.OUT_NHWC,
                 wrows=rows)
        return out

    def pool(self, x, out=None):
        if out is None:
            out = self._alloc(x.H // 2, x.W // 2, x.C)
        assert out.C == x.C
        self._op(_lib.OP_MAXPOOL, x, out, ksize=2, stride=2)
        return out

    def upadd(self, x, skip, wkey, f16=False, private_skip=False):
        """f16: the sum is written as fp16 (same 2-byte NHWC buffer) for a DeformConv that reads fp16: the F16IN variants of
        csrc/dcn3.hip (H3D_OPF_DCN_STREAM_F16_INPUT, the default) or csrc/dcn4.hip (stream_dcn, `make EXTRA=1`).
        private_skip: the caller knows that no other op reads `skip`.  When the op just lowered is the fused DeformConv that writes it,
        the op carries H3D_OPF_UPADD_FOLDED and the run loop launches the pair as one kernel (include/h3d.h)."""
        w, k = self.pw.up(wkey)
        f = k // 2
        out = self._alloc(x.H * f, x.W * f, x.C)
        assert (skip.H, skip.W, skip.C) == (out.H, out.W, out.C), wkey
        fold = (private_skip and self.ops and self.ops[-1].kind == _lib.OP_DCN_FUSED_STREAM and self.ops[-1].out == skip.ptr
                and (skip.coff, skip.cs) == (0, skip.C))          # the whole buffer: no sibling slice that somebody else could read
        self._op(_lib.OP_UPADD, x, out, skip, w=w.data_ptr(), ksize=k, stride=f, out_mode=_lib.OUT_NHWC_F16 if f16 else _lib.OUT_NHWC,
                 reserved=_lib.OPF_UPADD_FOLDED if fold else 0)
        return out

    # -- network ---------------------------------------------------------------------------------
    def _block(self, x, p, stride, residual, out, entry=False):
        """BasicBlock (model.py:46-60): conv-bn-relu, conv-bn, +residual, relu.  entry: see `conv`."""
        t = self.conv(x, p + ".conv1.weight", bn=p + ".bn1", stride=stride, entry=entry)
        return self.conv(t, p + ".conv2.weight", bn=p + ".bn2", res=residual, out=out)

    def _tree1(self, x, p, cin, cout, stride, level_root, out, cat=None, bottom=None, residual=None):
        """One-level Tree (model.py:209-218).  `cat` = pre-allocated Root input whose trailing
        slices (children) the caller has filled; layout [x2 | x1 | children...].  `bottom`: the
        max-pooled x when the caller already has it (the reference pools the same tensor in the outer
        and in the inner tree, model.py:213)."""
        Ho, Wo = x.H // stride, x.W // stride
        if cat is None:
            cat = self._alloc(Ho, Wo, 2 * cout + (cin if level_root else 0))
        s_x2, s_x1 = cat.slice(0, cout), cat.slice(cout, cout)
        # fold_tree_entry: pool, project and conv1 are lowered next to each other below (the pool by the caller when it passes `bottom`)
        entry = self.fold_tree_entry and self.share_pool and stride == 2 and residual is None and cin != cout
        private = bottom is None and not level_root         # ... and the pooled map is a buffer of its own that `project` alone reads
        if residual is not None:                             # (the caller already has project(pool(x)): csrc/stem3.hip PROJ)
            assert stride > 1 and not level_root and cin != cout and (residual.H, residual.W, residual.C) == (Ho, Wo, cout)
        elif bottom is not None:
            assert stride > 1 and not level_root and (bottom.H, bottom.W, bottom.C) == (Ho, Wo, cin)
        elif stride > 1:
            bottom = self.pool(x, cat.slice(2 * cout, cin) if level_root else None)
        else:
            bottom = x
        n_proj = len(self.ops)
        if residual is not None:
            pass
        elif cin != cout:
            residual = self.conv(bottom, p + ".project.0.weight", bn=p + ".project.1", relu=False)
        else:
            residual = bottom
        self._block(x, p + ".tree1", stride, residual, s_x1, entry=entry)
        if entry:
            self._flag_tree_entry(n_proj - 1, private)
        self._block(s_x1, p + ".tree2", 1, s_x1, s_x2)
        return self.conv(cat, p + ".root.conv.weight", bn=p + ".root.bn", out=out)

    def _flag_tree_entry(self, i, private):
        """fold_tree_entry: ops[i : i + 3] = the max-pool of x, `project` of the pooled map, conv1 of x.  Flagged where conv1 is a stride-2 op of
        csrc/conv2.hip on a one-slot tile (the tiles with the fused twin: the launcher's own choice from 128 output channels on, the tile
        `conv` asked for below that; every level measured faster fused than as three launches: DESIGN.md); the run loop checks the structure
        again and ignores the flag wherever its tile cannot take the triple.  private: nothing else reads the pooled map (level 2)."""
        if i < 0 or i + 3 > len(self.ops):
            return
        pool, proj, conv1 = self.ops[i:i + 3]
        tile = 0 if conv1.Cout >= 128 else _lib.TUNE_CONV_STREAM_TILE(4, 2, 4)
        if (pool.kind == _lib.OP_MAXPOOL and proj.kind == _lib.OP_CONV and conv1.kind == _lib.OP_CONV_STREAM and proj.ksize == 1 and conv1.stride == 2
                and (proj.in_, proj.in_cs) == (pool.out, pool.out_cs) and (conv1.in_, conv1.in_cs) == (pool.in_, pool.in_cs)
                and proj.Cout == conv1.Cout >= 64 and pool.H % 2 == 0 and pool.W % 2 == 0 and conv1.reserved == tile
                and not (proj.reserved or pool.reserved)):
            pool.reserved = _lib.OPF_TREE_ENTRY | (_lib.OPF_TREE_ENTRY_PRIVATE_POOL if private else 0)
            proj.reserved = _lib.OPF_TREE_ENTRY
            conv1.reserved = tile | _lib.OPF_TREE_ENTRY

    def _tree2(self, x, p, cin, cout, out):
        """Two-level Tree with level_root (level3/level4; model.py:209-222): Root input of the inner
        tree2 = [x2 | x1 | bottom | tree1 output]."""
        Ho, Wo = x.H // 2, x.W // 2
        cat = self._alloc(Ho, Wo, 2 * cout + cin + cout)
        pooled = self.pool(x, cat.slice(2 * cout, cin))
        x1 = self._tree1(x, p + ".tree1", cin, cout, 2, False, cat.slice(2 * cout + cin, cout),
                         bottom=pooled if self.share_pool else None)
        return self._tree1(x1, p + ".tree2", cout, cout, 1, False, out, cat=cat)

    def _dcn_f16_ok(self, p):
        """node DeformConvs with 64 input and <= 64 output channels run on csrc/dcn4.hip (fp16 input)."""
        w = self.pw.sd[p + ".conv.weight"]
        return (self.pw.use_dcn and self.fuse_offsets and self.stream_dcn and self.pw.dtype == "bf16"
                and w.shape[1] == 64 and w.shape[0] <= 64)

    def _node_f16_ok(self, p):
        """`node` DeformConvs of a bf16 plan that take an fp16 input (csrc/dcn3.hip F16IN): the fused patch-slot variants with more
        than 32 output channels."""
        w = self.pw.sd[p + ".conv.weight"]
        return (self.node_f16 and self.pw.use_dcn and self.fuse_offsets and self.pw.dtype == "bf16" and self.stream_dcn3 and self.dcn_patches
                and w.shape[1] % 32 == 0 and w.shape[0] > 32 and w.shape[0] % 8 == 0)

    def _deform(self, x, p, x_is_f16=False, in_f16=False):
        """DeformConv (model.py:346-362): DCN or plain 3x3 conv, then BN + ReLU (folded).  in_f16: `x` holds fp16 values in a
        bf16 plan (written by `upadd(..., f16=True)`) and the op carries the fp16-input bit.
        Each fused branch chooses the op kind, the pack (main filters, offset filters, bias, Cout, Cin, rows) and its own fields."""
        pw = self.pw
        cout, cin = pw.sd[p + ".conv.weight"].shape[:2]
        fused = pw.use_dcn and self.fuse_offsets
        kw, has_variants = {}, False
        if x_is_f16:
            kind, pack = _lib.OP_DCN_FUSED_F16, pw.dcn_stream(p)
        elif (fused and pw.dtype in LOWP
                and (self.stream_dcn3 or (self.dense_dcn3 and cout <= 64
                                          # two workgroups per CU only pay with >= 2 x 256 tiles (measured: the 32x32 layer
                                          # of a batch-64 plan, 256 tiles, 0.062 -> 0.076 ms)
                                          and self.B * ((x.H + 15) // 16) * ((x.W + 15) // 16) >= self.dense_dcn3_min_tiles))):
            kind, pack = _lib.OP_DCN_FUSED_STREAM, pw.dcn_stream(p, int(_lib.lib().h3d_dcn_fused_ck(int(cin), int(cout))))
            var = 0
            if self.dcn_patches and cin % 32 == 0:
                var = _lib.OPF_DCN_STREAM_WIDE_MARGIN if self.dcn_wide_margin else _lib.OPF_DCN_STREAM_SLOTS512 if self.dcn_slots512 else pw.dcn_variant.get(p, 0)
            kw = dict(reserved=(var | (DCN_F16IN if in_f16 else 0)) if self.dcn_patches else _lib.OPF_DCN_STREAM_NO_SLOTS)
            has_variants = True
        else:
            assert not in_f16, p
            if fused and pw.dtype == "f16x3" and self.x3_dcn_patches and cin % 32 == 0:
                kind, pack = _lib.OP_DCN_FUSED_STREAM, pw.dcn_stream_x3(p)
                kw = dict(wexp=pw.wexp[pack[0].data_ptr()], wexp2=pw.wexp[pack[1].data_ptr()])
            elif fused:
                kind, pack = _lib.OP_DCN_FUSED, pw.dcn_fused(p)
                kw = dict(wexp=pw.wexp.get(pack[0].data_ptr(), 0), wexp2=pw.wexp.get(pack[1].data_ptr(), 0))
            elif pw.use_dcn:
                if pw.dtype == "f16":
                    raise RuntimeError("fp16 plans run the fused DeformConv kernel only (fuse_offsets=False is a bf16 / f32 debugging path)")
                om = self.conv(x, p + ".conv.conv_offset_mask.weight", bkey=p + ".conv.conv_offset_mask.bias",
                               relu=False, out_mode=_lib.OUT_NHWC_F32, pad_cout_to=32)
                return self.dcn(x, om, p + ".conv.weight", p + ".conv.bias", p + ".actf.0")
            else:
                return self.conv(x, p + ".conv.weight", bkey=p + ".conv.bias", bn=p + ".actf.0")
        wmain, woff, bias, cout, cin, rows = pack
        assert cin == x.C, (p, cin, x.C)
        out = self._alloc(x.H, x.W, cout)
        i = self._op(kind, x, out, in2=woff.data_ptr(), w=wmain.data_ptr(), bias=bias.data_ptr(), ksize=3, stride=1, relu=1,
                     out_mode=_lib.OUT_NHWC, wrows=rows, **kw)
        if has_variants:
            self.dcn_layers.append((p, i))
        return out

    def _ida_projs(self, layers, p, startp, endp):
        """The proj_k DeformConvs of an IDAUp, all in front of its first step (fold_upadd): proj_k reads layers[i] before step i replaces
        it, so lowering them early changes no value."""
        return [self._deform(layers[i], "%s.proj_%d" % (p, i - startp)) for i in range(startp + 1, endp)]

    def _ida(self, layers, p, startp, endp, private=(), projs=None):
        """IDAUp.forward (model.py:384-390) on the python list `layers` (mutated like the reference).
        fold_upadd: `private` = the steps k whose skip layers[i - 1] no op outside this step reads; `projs` = the proj outputs when the
        caller has lowered them already (else they are lowered here, in front of the first step).  The up-sample + add of a private step
        then directly follows the node DeformConv that writes its skip, and `upadd` marks it for the run loop's fold."""
        if self.fold_upadd and projs is None:
            projs = self._ida_projs(layers, p, startp, endp)
        for i in range(startp + 1, endp):
            k = i - startp
            y = projs[k - 1] if projs is not None else self._deform(layers[i], "%s.proj_%d" % (p, k))
            f16 = self._dcn_f16_ok("%s.node_%d" % (p, k))
            if f16 and self.fuse_upnode and self.pw.up("%s.up_%d.weight" % (p, k))[1] // 2 >= self.fuse_upnode_min_f:
                layers[i] = self._updcn(y, layers[i - 1], "%s.up_%d.weight" % (p, k), "%s.node_%d" % (p, k))
                continue
            nf16 = not f16 and self._node_f16_ok("%s.node_%d" % (p, k))
            y = self.upadd(y, layers[i - 1], "%s.up_%d.weight" % (p, k), f16=f16 or nf16, private_skip=self.fold_upadd and k in private)
            layers[i] = self._deform(y, "%s.node_%d" % (p, k), x_is_f16=f16, in_f16=nf16)

    def _updcn(self, x, skip, wkey, p):
        """node(up(x) + skip) in one launch (csrc/dcn4.hip UP = 1): the up-sampled sum never reaches HBM."""
        wup, k = self.pw.up(wkey)
        f = k // 2
        wimg, woimg, bias, cout, cin, rows = self.pw.dcn_stream(p)
        assert (skip.H, skip.W, skip.C) == (x.H * f, x.W * f, x.C) and cin == x.C == 64, wkey
        out = self._alloc(skip.H, skip.W, cout)
        desc = _lib.H3dUpdcnDesc()
        desc.skip, desc.w_up, desc.w_off, desc.skip_cs = skip.ptr, wup.data_ptr(), woimg.data_ptr(), skip.cs
        self.keep.append(desc)
        self._op(_lib.OP_UPDCN_F16, x, out, in2=ctypes.addressof(desc), w=wimg.data_ptr(), bias=bias.data_ptr(), ksize=3, stride=f,
                 relu=1, out_mode=_lib.OUT_NHWC, wrows=rows)
        return out

    def _lower(self):
        H, W = self.H, self.W
        C = arch.CHANNELS
        y0 = res2 = None
        if self.fuse_stem and self.pw.dtype == "f16x3" and C[0] == 16 and C[1] == 32:
            # the f16x3 twin of the fused stem (csrc/stem3x.hip): the two full-resolution maps stay in LDS as split operand fragments
            y1 = self._alloc((H - 1) // 2 + 1, (W - 1) // 2 + 1, C[1])
            w, b = self.pw.stem3_x3()
            self._op(_lib.OP_STEM3, self.image, y1, w=w.data_ptr(), bias=b.data_ptr(), ksize=7, stride=2, relu=1)
        elif self.fuse_stem and self.pw.dtype in LOWP and C[0] == 16 and C[1] == 32 and W % 4 == 0:
            # (W % 4: csrc/stem3.hip reads the image as aligned float4; any other width takes the three launches)
            # base_layer + level0 + level1 in one launch: the two full-resolution maps never reach HBM (nothing else
            # reads them: DLAUp starts at level 2)
            y1 = self._alloc((H - 1) // 2 + 1, (W - 1) // 2 + 1, C[1])
            proj = self.fuse_stem_proj and C[2] == 64 and y1.H % 2 == 0 and y1.W % 2 == 0
            w, b = self.pw.stem3(proj)
            res2 = self._alloc(y1.H // 2, y1.W // 2, C[2]) if proj else None
            self._op(_lib.OP_STEM3, self.image, y1, res2, w=w.data_ptr(), bias=b.data_ptr(), ksize=7, stride=2, relu=1)
        else:
            w, b = self.pw.stem()
            x = self._alloc(H, W, C[0])
            self._op(_lib.OP_STEM, self.image, x, w=w.data_ptr(), bias=b.data_ptr(), ksize=7, stride=1, relu=1,
                     wexp=self.pw.wexp.get(w.data_ptr(), 0))
            y0 = self.conv(x, "base.level0.0.weight", bn="base.level0.1")
            y1 = self.conv(y0, "base.level1.0.weight", bn="base.level1.1", stride=2)
        y2 = self._tree1(y1, "base.level2", C[1], C[2], 2, False, None, residual=res2)
        y3 = self._tree2(y2, "base.level3", C[2], C[3], None)
        y4 = self._tree2(y3, "base.level4", C[3], C[4], None)
        y5 = self._tree1(y4, "base.level5", C[4], C[5], 2, True, None)
        layers = [y0, y1, y2, y3, y4, y5]
        # DLAUp.forward (model.py:409-415)
        outs = [layers[-1]]
        pre = None
        for i in range(3):
            startp, private = len(layers) - i - 2, ()
            if self.fold_upadd and i == 2:
                # The last IDA of DLAUp: only its final map is read again, so from step 2 on every skip (the node output of the step
                # before) is private.  That final map, outs[0] below, is read by ida_up's first step alone, as its skip: ida_up's
                # proj DeformConvs (they read what are outs[0] and outs[1] NOW) are lowered first, so that ida_up's first up-sample +
                # add directly follows the node that writes its skip.
                pre = self._ida_projs([None, outs[0], outs[1]], "ida_up", 0, 3)
                private = tuple(range(2, len(layers) - startp))
            self._ida(layers, "dla_up.ida_%d" % i, startp, len(layers), private=private)
            outs.insert(0, layers[-1])
        # DLASeg.forward (model.py:480-483): ida_up over the three finest maps; only ys[-1] is used, so both skips are private
        ys = [outs[0], outs[1], outs[2]]
        self._ida(ys, "ida_up", 0, 3, private=(1, 2), projs=pre)
        self.feat = ys[-1]
        if self.lower_heads:
            self._lower_heads(self.feat)

    def _lower_heads(self, feat):
        """Output heads on the 64-channel map (model.py:451-460, 485-489; the ResNet-DCN heads have the same form)."""
        Ho, Wo = feat.H, feat.W
        fused = (self.pw.head_conv > 0 and self.pw.head_conv % 64 == 0 and feat.C == 64 and
                 len(self.pw.heads) <= _lib.HEADS_MAX and max(self.pw.heads.values()) <= 96 and self.fuse_heads)
        if fused:
            # one launch per group of heads with the same number of 32-row output tiles, so the
            # narrow heads do not inherit the register footprint of the 72-channel pose head
            def heads_op(names, emit=True):
                """One H3D_OP_HEADS over `names`; a head that already has its output (the sparse twin of the deferred ops) writes the same map."""
                w1, b1, per = self.pw.fused_heads(tuple(names))
                desc = _lib.H3dHeadsDesc()
                desc.nheads = len(per)
                desc.wexp = self.pw.wexp.get(w1.data_ptr(), 0)
                for i, (head, c, w2, b2) in enumerate(per):
                    if head in self.outputs:
                        optr, self._sparse_at[head] = self.outputs[head].data_ptr(), (desc, i)
                    else:
                        optr = self._new_output(head, c, Ho, Wo, (desc, i)).ptr
                    desc.head[i].w2, desc.head[i].b2, desc.head[i].out, desc.head[i].C = w2.data_ptr(), b2.data_ptr(), optr, c
                    desc.head[i].wexp2 = self.pw.wexp.get(w2.data_ptr(), 0)
                self.keep.append(desc)
                return self._op(_lib.OP_HEADS, feat, in2=ctypes.addressof(desc), w=w1.data_ptr(), bias=b1.data_ptr(),
                                Ho=Ho, Wo=Wo, Cout=self.pw.head_conv, ksize=3, stride=1, emit=emit)

            peak = tuple(self.peak_heads or ())
            eager = tuple(h for h in self.pw.heads if h in tuple(self.split_heads or ()) and h not in peak)
            deferred = tuple(h for h in self.pw.heads if h not in eager)
            split = bool(eager) and bool(deferred) and self.pw.dtype in LOWP
            if split:
                heads_op(eager)
                self.n_eager = len(self.ops)
            groups = {}
            for head, c in self.pw.heads.items():
                if split and head in eager:
                    continue
                m2 = (c + 31) // 32
                groups.setdefault(0 if self.mixed_heads else 1 if m2 == 1 else self.wide_heads_m2 or m2, []).append(head)
            for m2 in sorted(groups):
                heads_op(groups[m2])
            if split:
                self.sparse_op = heads_op(deferred, emit=False)
                pk = sum(1 << i for i, h in enumerate(deferred) if h in peak)
                self.sparse_masks = ((1 << len(deferred)) - 1 - pk, pk)
            self.outputs = {h: self.outputs[h] for h in self.pw.heads}      # reference head order
            return
        for head in self.pw.heads:
            if self.pw.head_conv > 0:
                t = self.conv(feat, head + ".0.weight", bkey=head + ".0.bias")
                self._head_conv(t, head, head + ".2.weight", head + ".2.bias")
            else:
                self._head_conv(feat, head, head + ".weight", head + ".bias")

    def _head_conv(self, x, head, wkey, bkey):
        """The last conv of an unfused head: the next op, writing the head's NCHW fp32 output."""
        o = self._new_output(head, self.pw.heads[head], x.H, x.W, len(self.ops))
        self.conv(x, wkey, out=o, bkey=bkey, relu=False, out_mode=_lib.OUT_NCHW_F32)

    def _stem_s2(self, wkey, bkey, bn, cout):
        """Conv2d(3, cout, 7, stride 2, padding 3) + BN + ReLU from the NCHW fp32 images."""
        Ho, Wo = (self.H - 1) // 2 + 1, (self.W - 1) // 2 + 1
        if self.dtype in LOWP and self.stem_s2_direct:
            w, b = self.pw.stem_s2(wkey, bkey, bn)
            x = self._alloc(Ho, Wo, cout)
            self._op(_lib.OP_STEM, self.image, x, w=w.data_ptr(), bias=b.data_ptr(), ksize=7, stride=2, relu=1)
            return x
        patches = self._alloc(Ho, Wo, 160)                   # fp32 plans: im2col + 1x1 conv (csrc/extra.hip)
        self._op(_lib.OP_IM2COL, self.image, patches, ksize=7, stride=2)
        return self.conv(patches, self.pw.im2col_key(wkey), bkey=bkey, bn=bn)

    # -- ResNet-101-DCN (arch_res.py; published CenterNet `resnet_dcn.py`) ---------------------------------------------------
    def _lower_resdcn(self):
        x = self._stem_s2("conv1.weight", None, "bn1", 64)   # conv1 7x7/2 + bn1 + ReLU
        y = self._alloc((x.H - 1) // 2 + 1, (x.W - 1) // 2 + 1, x.C)
        self._op(_lib.OP_MAXPOOL3, x, y, ksize=3, stride=2)
        x = y
        for p, cin, planes, stride, down in arch_res.blocks(101):
            t = self.conv(x, p + ".conv1.weight", bn=p + ".bn1")
            t = self.conv(t, p + ".conv2.weight", bn=p + ".bn2", stride=stride)
            res = self.conv(x, p + ".downsample.0.weight", bn=p + ".downsample.1", stride=stride, relu=False) if down else x
            x = self.conv(t, p + ".conv3.weight", bn=p + ".bn3", res=res)
        for i, planes in enumerate(arch_res.DECONV):
            x = self._deform(x, "deconv_layers.%d" % (6 * i))                # DCN + BN + ReLU
            wkey, bn = self.pw.deconv4_as_conv3("deconv_layers.%d.weight" % (6 * i + 3), "deconv_layers.%d" % (6 * i + 4))
            t = self.conv(x, wkey, bn=bn)                                      # [B,H,W,4C], BN + ReLU folded / fused
            assert t.C == 4 * planes
            x = self._alloc(2 * t.H, 2 * t.W, planes)
            self._op(_lib.OP_DEPTH2SPACE, t, x, ksize=1, stride=1)
        self.feat = x
        if self.lower_heads:
            self._lower_heads(x)

    # -- Hourglass-104 (arch_hg.py; published CenterNet `exkp`) ---------------------------------------------------------
    def _hg_residual(self, x, p, cin, cout, stride):
        """residual: relu(bn2(conv2(relu(bn1(conv1(x))))) + skip(x)), skip = 1x1 conv + BN when stride / width change."""
        t = self.conv(x, p + ".conv1.weight", bn=p + ".bn1", stride=stride)
        skip = x
        if arch_hg.residual_has_skip(cin, cout, stride):
            skip = self.conv(x, p + ".skip.0.weight", bn=p + ".skip.1", stride=stride, relu=False)
        return self.conv(t, p + ".conv2.weight", bn=p + ".bn2", res=skip)

    def _hg_seq(self, x, p, kind, cin, cout, modules):
        for j, (ci, co, st) in enumerate(arch_hg.layer_specs(kind, cin, cout, modules)):
            x = self._hg_residual(x, "%s.%d" % (p, j), ci, co, st)
        return x

    def _hg_kp(self, x, p, n, dims, modules):
        up1 = self._hg_seq(x, p + ".up1", "layer", dims[0], dims[0], modules[0])
        low1 = self._hg_seq(x, p + ".low1", "hg", dims[0], dims[1], modules[0])
        if n > 1:
            low2 = self._hg_kp(low1, p + ".low2", n - 1, dims[1:], modules[1:])
        else:
            low2 = self._hg_seq(low1, p + ".low2", "layer", dims[1], dims[1], modules[1])
        low3 = self._hg_seq(low2, p + ".low3", "revr", dims[1], dims[0], modules[0])
        return self.upadd(low3, up1, self.pw.nearest_up_key(dims[0]))       # up1 + nearest x2 of low3

    def _lower_hourglass(self):
        nstack = 2
        # pre.0: Conv2d(3, 128, 7, stride 2, pad 3) + BN + ReLU
        inter = self._stem_s2("pre.0.conv.weight", None, "pre.0.bn", arch_hg.PRE_DIM)
        inter = self._hg_residual(inter, "pre.1", arch_hg.PRE_DIM, arch_hg.DIMS[0], 2)
        self.all_outputs = []
        for i in range(nstack):
            kp = self._hg_kp(inter, "kps.%d" % i, arch_hg.N, arch_hg.DIMS, arch_hg.MODULES)
            cnv = self.conv(kp, "cnvs.%d.conv.weight" % i, bn="cnvs.%d.bn" % i)
            self.outputs = {}                                   # (the heads of this stack; the last stack's stay the plan's outputs)
            for head in self.pw.heads:
                t = self.conv(cnv, "%s.%d.0.conv.weight" % (head, i), bkey="%s.%d.0.conv.bias" % (head, i))
                self._head_conv(t, head, "%s.%d.1.weight" % (head, i), "%s.%d.1.bias" % (head, i))
            self.all_outputs.append(self.outputs)
            if i < nstack - 1:
                a = self.conv(inter, "inters_.%d.0.weight" % i, bn="inters_.%d.1" % i, relu=False)
                inter = self.conv(cnv, "cnvs_.%d.0.weight" % i, bn="cnvs_.%d.1" % i, res=a)       # relu(inters_(inter) + cnvs_(cnv))
                inter = self._hg_residual(inter, "inters.%d" % i, arch_hg.DIMS[0], arch_hg.DIMS[0], 1)

    def retarget_outputs(self, views):
        """Point the head outputs at caller-provided contiguous [B,C,H,W] fp32 views (sub-batch plans)."""
        for h, v in views.items():
            assert v.is_contiguous() and tuple(v.shape) == tuple(self.outputs[h].shape)
        for h in self.outputs:
            at = self._out_at[h]
            if isinstance(at, int):
                self.op_array[at].out = views[h].data_ptr()
            else:
                at[0].head[at[1]].out = views[h].data_ptr()
            if h in self._sparse_at:
                at = self._sparse_at[h]
                at[0].head[at[1]].out = views[h].data_ptr()
        self.outputs = dict(views)

    def _run_range(self, first, n):
        if self.pending is not None:        # launches of another stream into this plan's maps come first
            torch.cuda.current_stream().wait_event(self.pending)
            self.pending = None
        if n > 0:
            ops = self.op_array if first == 0 else ctypes.byref(self.op_array[first])      # (an element is a view of the array's memory)
            rc = _lib.lib().h3d_run_ops(ops, n, _lib.stream_ptr())
            _lib.check(rc, "h3d_run_ops")
        return self.outputs

    def run(self):
        return self._run_range(0, len(self.ops))

    # -- split_heads plans --------------------------------------------------------------------------
    def run_eager(self):
        """Backbone + the eager heads.  The deferred heads' maps keep whatever they held."""
        return self._run_range(0, self.n_eager)

    def run_sparse(self, inds, K):
        """The deferred heads at inds [B,K] (int64, flat y*W + x of the output map) only, written into their dense maps."""
        _lib.require_cuda(inds)
        if inds.dtype != torch.int64 or not inds.is_contiguous() or tuple(inds.shape) != (self.B, K):
            raise RuntimeError("run_sparse: contiguous int64 inds [%d,%d] expected, got %s %s" % (self.B, K, tuple(inds.shape), inds.dtype))
        if not self.sparse_masks[1]:
            _lib.check(_lib.lib().h3d_heads_sparse(ctypes.byref(self.sparse_op), _lib.ptr(inds), int(K), _lib.stream_ptr()), "h3d_heads_sparse")
        elif self.sparse_masks[0]:
            self._sparse_lists("run_sparse", (inds, K, self.sparse_masks[0]))

    def _sparse_lists(self, what, *lists):
        """ONE h3d_heads_sparse_lists launch: (inds [B,K], K, descriptor-slot mask of the heads evaluated there) per list."""
        arr = (_lib.H3dHeadsList * len(lists))()
        for e, (inds, K, mask) in zip(arr, lists):
            _lib.require_cuda(inds)
            if inds.dtype != torch.int64 or not inds.is_contiguous() or tuple(inds.shape) != (self.B, K):
                raise RuntimeError("%s: contiguous int64 inds [%d,%d] expected, got %s %s" % (what, self.B, K, tuple(inds.shape), inds.dtype))
            e.inds, e.K, e.head_mask = inds.data_ptr(), int(K), mask
        _lib.check(_lib.lib().h3d_heads_sparse_lists(ctypes.byref(self.sparse_op), len(lists), arr, _lib.stream_ptr()), "h3d_heads_sparse_lists")

    def run_sparse_lists(self, inds, K, peak_inds, PK):
        """`run_sparse` and, in the same launch, the peak heads (`peak_heads`) at peak_inds [B,PK] (int64, flat y*W + x)."""
        if self.sparse_op is None or not self.sparse_masks[1]:
            raise RuntimeError("run_sparse_lists: this plan was lowered without peak_heads (dtype %s)" % self.dtype)
        self._sparse_lists("run_sparse_lists", *([(inds, K, self.sparse_masks[0])] if self.sparse_masks[0] else []), (peak_inds, PK, self.sparse_masks[1]))

    def run_deferred(self):
        """The deferred heads' dense launches: the whole maps (the positions `run_sparse` wrote receive the same bits)."""
        return self._run_range(self.n_eager, len(self.ops) - self.n_eager)
