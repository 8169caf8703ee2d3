"""Launch-plan builder and executor for the DLA-34 (+DCNv2) multi_pose network.

Host-side counterpart of the reference's `DLASeg.forward` (models/model.py:475-489): instead of
walking nn.Modules per call, the network is lowered ONCE per (batch, height, width, dtype) into
an array of `h3d_op` descriptors (include/h3d.h) over pre-allocated NHWC buffers and pre-packed
weights; a forward is a single `h3d_run_ops` call on the current stream.

Lowering decisions (DESIGN.md 'Data layout'):
  * activations NHWC (channels-last) bf16 (throughput) or fp32 (parity mode);
  * eval-mode BatchNorm folded into the preceding conv / DCN weights and bias;
  * Root's torch.cat (model.py:160) is free: producers write into channel slices of one buffer;
  * residual add + ReLU are conv epilogues; IDAUp's depthwise deconv + skip add is one kernel;
  * conv_offset_mask (dcn_v2.py:119-122) writes NHWC fp32 offsets/mask-logits consumed in place
    by the DCN kernel (no chunk/cat/sigmoid passes);
  * the `project` conv of the two-level trees (level3/level4) is dead in the reference
    (model.py:212 recomputes the residual inside tree1) and is not lowered;
  * head outputs are written directly as contiguous NCHW fp32, the reference's head layout.

Where it lives: weights.py packs the filters (`PackedWeights`), plan.py lowers the network (`View`, `Plan`), dcn_calibrate.py
chooses and times the DeformConv tile variants; this module holds `DLAEngine`, which caches plans and runs them.
"""
import torch

from . import _lib, dcn_calibrate
# the names other modules, bench.py, tools and tests import from here
from ._lib import H3dOp  # noqa: F401
from .dcn_calibrate import _tiles_over_slots  # noqa: F401
from .plan import DCN_F16IN, Plan, View  # noqa: F401
from .weights import LOWP, PackedWeights, heads_k_perm, pack_head_1x1, pack_head_3x3, x3_exp, x3_split  # noqa: F401
from .weights import _TORCH_DT


class DLAEngine:
    """state_dict -> packed weights -> cached plans.  `forward(images)` returns the head dict
    (fresh views of the plan's output buffers; they are overwritten by the next forward of the
    same shape, like any static-graph runtime -- clone to keep)."""

    def __init__(self, state_dict, heads, use_dcn, dtype="bf16", device="cuda", head_conv=256, arch_name="dla34"):
        if dtype not in _TORCH_DT:
            raise ValueError("dtype must be 'bf16', 'f16', 'f32' or 'f16x3'")
        _lib.lib()                                     # fail loudly now if the HIP library is missing
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Not implemented on the CPU")
        self.pw = PackedWeights(state_dict, heads, use_dcn, dtype, self.device, head_conv, arch_name)
        self.plans = {}
        for k, v in Plan.FLAGS.items():   # lowering switches, see Plan.FLAGS (changing one requires plans.clear())
            setattr(self, k, v)
        self.streams = 1                # >1: run that many sub-batches concurrently on their own HIP streams

    def _flags(self):
        return {k: getattr(self, k) for k in Plan.FLAGS}

    def plan(self, B, H, W, slot=0):
        """slot: independent copies of the plan (own activation and output buffers, shared packed weights) so that
        consecutive batches can be in flight on different HIP streams (bench.py --pipeline)."""
        key = (B, H, W) if slot == 0 else (B, H, W, slot)
        if key not in self.plans:
            with torch.cuda.device(self.device):
                self.plans[key] = Plan(self.pw, B, H, W, **self._flags())
        return self.plans[key]

    def forward(self, images, slot=0):
        _lib.require_cuda(images)
        if images.dim() != 4 or images.shape[1] != 3:
            raise RuntimeError("expected images [B,3,H,W], got %s" % (tuple(images.shape),))
        B, _, H, W = images.shape
        if self.streams > 1 and B % self.streams == 0 and B // self.streams >= 8 and self.pw.arch == "dla34":
            return self._forward_split(images, slot)
        plan = self.plan(B, H, W, slot)
        with torch.cuda.device(self.device):
            self._bind(plan, images)
            return plan.run()

    @staticmethod
    def _bind(plan, images):
        if images.dtype == torch.float32 and images.is_contiguous():
            plan.op_array[0].in_ = images.data_ptr()       # read the caller's batch in place
        else:
            plan.images.copy_(images)
            plan.op_array[0].in_ = plan.images.data_ptr()

    def forward_eager(self, images, slot=0):
        """`split_heads` plans: the backbone and the eager heads only -> the Plan, whose `run_sparse` / `run_deferred` supply the other
        heads (detector.MultiPoseDetector.run).  None when this call has no such plan (another lowering, sub-batch streams): nothing
        was launched, call `forward`."""
        _lib.require_cuda(images)
        if images.dim() != 4 or images.shape[1] != 3:
            raise RuntimeError("expected images [B,3,H,W], got %s" % (tuple(images.shape),))
        B, _, H, W = images.shape
        if not self.split_heads or self.streams > 1:
            return None
        plan = self.plan(B, H, W, slot)
        if plan.sparse_op is None:
            return None
        with torch.cuda.device(self.device):
            self._bind(plan, images)
            plan.run_eager()
        return plan

    def _forward_split(self, images, slot=0):
        """Sub-batches on separate HIP streams: the small-grid layers (level4/5, the 16x16 / 32x32 neck
        layers: 128-512 workgroups on 256 CUs) and every kernel's tail overlap with the other
        sub-batch's launches.  Outputs are written into one full-batch tensor per head.  Every `slot` has its own
        sub-plans, output tensors and internal streams: two batches in flight on different slots share nothing but
        the packed weights."""
        B, _, H, W = images.shape
        n = self.streams
        sub = B // n
        key = ("split", B, H, W, slot)
        with torch.cuda.device(self.device):
            if key not in self.plans:
                plans = [Plan(self.pw, sub, H, W, **self._flags())
                         for _ in range(n)]
                full = {h: torch.empty((B,) + tuple(o.shape[1:]), dtype=o.dtype, device=o.device)
                        for h, o in plans[0].outputs.items()}
                for i, p in enumerate(plans):          # re-point the head outputs into the full-batch tensors
                    p.retarget_outputs({h: full[h][i * sub:(i + 1) * sub] for h in full})
                self.plans[key] = (plans, full, [torch.cuda.Stream(device=self.device) for _ in range(n)])
            plans, full, streams = self.plans[key]
            if not (images.dtype == torch.float32 and images.is_contiguous()):
                images = images.float().contiguous()
            cur = torch.cuda.current_stream()
            ready = torch.cuda.Event()
            ready.record(cur)
            for i, (p, st) in enumerate(zip(plans, streams)):
                st.wait_event(ready)
                with torch.cuda.stream(st):
                    p.op_array[0].in_ = images[i * sub:(i + 1) * sub].data_ptr()
                    p.run()
                    done = torch.cuda.Event()
                    done.record(st)
                cur.wait_event(done)
            self._keepalive = getattr(self, "_keepalive", {})
            self._keepalive[slot] = images
            return full

    # DeformConv calibration and timing tooling: h3d_amd/dcn_calibrate.py
    DCN_VARIANTS = dcn_calibrate.DCN_VARIANTS
    DCN_RULE = dcn_calibrate.DCN_RULE
    dcn_far_samples = dcn_calibrate.dcn_far_samples
    calibrate_dcn_margins = dcn_calibrate.calibrate_dcn_margins
    _dcn_rounds = dcn_calibrate._dcn_rounds
    time_dcn_variants = dcn_calibrate.time_dcn_variants

    __call__ = forward
