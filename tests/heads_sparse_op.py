"""One H3D_OP_HEADS op on a feature map and output maps of the caller's own, with its dense launch as the reference and
h3d_heads_sparse_lists on each of the three sparse paths: shared by tests/test_gpu_heads_sparse_regs.py and tools/ab_heads_sparse.py.
The packed filters come from the sparse op of a DLA-34 plan with the heads below; the map, the batch and the lists are free."""
import ctypes
import functools

import numpy as np
import torch

import h3d_amd  # noqa: F401
from h3d_amd import _lib, arch, synth
from h3d_amd.model import create_model

DEV = "cuda:0"
# one descriptor: a six-head list (1, 2 and 3 output tiles) and a seventh head for a list of its own
HEADS = {"hm": 1, "a1": 1, "a2": 2, "a3": 3, "a10": 10, "a34": 34, "a72": 72, "pk": 2}
SPARSE = ["a1", "a2", "a3", "a10", "a34", "a72", "pk"]
CENTRE, PEAK = 0x3f, 0x40
PATHS = {"regs8": 0, "regs4": _lib.TUNE_HEADS_SPARSE_WAVES4, "lds_patch": _lib.TUNE_HEADS_SPARSE_LDS_PATCH}
NPOS = {"regs8": 256, "regs4": 128, "lds_patch": 64}         # positions per workgroup


@functools.lru_cache(maxsize=None)
def weights(dtype):
    """-> the plan of a DLA-34 with HEADS (its sparse op carries the packed filters of the seven gathered heads), the model that owns it."""
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0).items()}
    m = create_model("dla_34", HEADS, 256, False, dtype=dtype)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).eval()
    m.engine_flags.update({"split_heads": ("hm",), "peak_heads": ("pk",)})
    m(torch.from_numpy(synth.synth_images(2, 64, 128)).to(DEV))
    plan = m.engine(torch.device(DEV)).plan(2, 64, 128)
    torch.cuda.synchronize()
    assert plan.sparse_op is not None and plan.sparse_masks == (CENTRE, PEAK)
    d = ctypes.cast(plan.sparse_op.in2, ctypes.POINTER(_lib.H3dHeadsDesc)).contents
    assert [d.head[i].C for i in range(d.nheads)] == [HEADS[h] for h in SPARSE]
    return plan, m


class Op:
    """The plan's sparse op on a [B, H, W] map with pixel stride `cs`; `dense` holds what its dense launch wrote."""

    def __init__(self, dtype, B, H, W, cs):
        plan, _ = weights(dtype)
        rs = np.random.RandomState(H * 1000 + W)
        feat = torch.full((B, H, W, cs), 1e4, dtype=torch.float32)                   # (the channels beyond 64 belong to nobody)
        feat[..., :64] = torch.from_numpy((rs.randn(B, H, W, 64) * 0.5).astype(np.float32))
        self.feat = feat.to(DEV).to(torch.bfloat16 if dtype == "bf16" else torch.float16)
        self.B, self.H, self.W = B, H, W
        self.out = {h: torch.empty(B, HEADS[h], H, W, dtype=torch.float32, device=DEV) for h in SPARSE}
        self.desc = _lib.H3dHeadsDesc.from_buffer_copy(ctypes.cast(plan.sparse_op.in2, ctypes.POINTER(_lib.H3dHeadsDesc)).contents)
        for i, h in enumerate(SPARSE):
            self.desc.head[i].out = self.out[h].data_ptr()
        self.op = _lib.H3dOp.from_buffer_copy(plan.sparse_op)
        self.op.in_, self.op.in2, self.op.in_cs = self.feat.data_ptr(), ctypes.addressof(self.desc), cs
        self.op.B, self.op.H, self.op.W, self.op.Ho, self.op.Wo = B, H, W, H, W
        # the dense launch of the same op, once
        _lib.check(_lib.lib().h3d_run_ops(ctypes.byref(self.op), 1, _lib.stream_ptr()), "h3d_run_ops")
        torch.cuda.synchronize()
        self.dense = {h: t.clone() for h, t in self.out.items()}
        for h, t in self.dense.items():
            assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, h

    def list_array(self, lists):
        arr = (_lib.H3dHeadsList * len(lists))()
        for e, (inds, mask) in zip(arr, lists):
            assert inds.dtype == torch.int64 and inds.is_contiguous() and inds.shape[0] == self.B
            e.inds, e.K, e.head_mask = inds.data_ptr(), inds.shape[1], mask
        return arr

    def launch(self, path, arr, nlists):
        """One h3d_heads_sparse_lists launch on `path` over the first nlists entries of arr (no fill, no synchronise)."""
        self.op.reserved = PATHS[path]
        try:
            _lib.check(_lib.lib().h3d_heads_sparse_lists(ctypes.byref(self.op), nlists, arr, _lib.stream_ptr()), "h3d_heads_sparse_lists")
        finally:
            self.op.reserved = 0

    def sparse(self, path, *lists):
        """NaN-fill the maps, one launch over (inds [B, K], mask) per list on `path` -> clones of the maps."""
        for t in self.out.values():
            t.fill_(float("nan"))
        self.launch(path, self.list_array(lists), len(lists))
        torch.cuda.synchronize()
        return {h: t.clone() for h, t in self.out.items()}

    def written(self, inds):
        """[B, 1, H, W] bool: the positions of the map that `inds` lists (entries outside [0, H W) list nothing)."""
        HW = self.H * self.W
        m = torch.zeros(self.B, HW + 1, dtype=torch.bool, device=DEV)
        m.scatter_(1, torch.where((inds >= 0) & (inds < HW), inds, torch.full_like(inds, HW)), True)
        return m[:, :HW].reshape(self.B, 1, self.H, self.W)

    def check(self, got, lists, tag):
        """Each head: the dense bits at the positions of the list that names it, NaN everywhere else."""
        for i, h in enumerate(SPARSE):
            m = torch.zeros(self.B, 1, self.H, self.W, dtype=torch.bool, device=DEV)
            for inds, mask in lists:
                if mask >> i & 1:
                    m |= self.written(inds)
            m = m.expand_as(got[h])
            assert torch.equal(got[h][m], self.dense[h][m]), (tag, h, int((got[h][m] != self.dense[h][m]).sum()))
            assert bool(torch.isnan(got[h][~m]).all()), (tag, h, "an element outside the lists was written")
