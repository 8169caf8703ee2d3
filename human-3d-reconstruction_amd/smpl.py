"""SMPL pose/shape -> linear-blend-skinning mesh stage (north_star).

There is NO SMPL code, model file or test in the reference snapshot, and the real
SMPL model is licence-gated, so this stage follows the published formulation (Loper et al.
2015; axis-angle convention of the public `smplx` package) and ships a *synthetic* model of
the true tensor shapes for benchmarking.  A real model drops in through `SMPLModel.from_npz`.
Parity for this stage is "unpinned by the reference" (DESIGN.md).

Device compute: csrc/smpl.hip via `h3d_smpl_*` (include/h3d.h).  Gradients with respect to betas / thetas (or the `pose` / `shape`
head maps): csrc/smpl_bwd.hip, through `lbs_backward` and, when an input requires grad, through autograd (include/h3d.h section 4b).
"""
import numpy as np

from . import _lib, synth

NUM_VERTS = 6890
NUM_JOINTS = 24
NUM_BETAS = 10
NUM_POSE_FEAT = 207
PARENTS = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19,
                    20, 21], dtype=np.int32)


class SMPLModel:
    """Host container of the SMPL tensors (float32 numpy) + lazily-built device pack."""

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, weights, parents=PARENTS, faces=None):
        self.v_template = np.ascontiguousarray(v_template, np.float32)      # [V,3]
        self.shapedirs = np.ascontiguousarray(shapedirs, np.float32)        # [V,3,10]
        self.posedirs = np.ascontiguousarray(posedirs, np.float32)          # [V,3,207]
        self.J_regressor = np.ascontiguousarray(J_regressor, np.float32)    # [24,V]
        self.weights = np.ascontiguousarray(weights, np.float32)            # [V,24]
        self.parents = np.ascontiguousarray(parents, np.int32)
        V = self.v_template.shape[0]
        assert self.shapedirs.shape == (V, 3, NUM_BETAS)
        assert self.posedirs.shape == (V, 3, NUM_POSE_FEAT)
        assert self.J_regressor.shape == (NUM_JOINTS, V)
        assert self.weights.shape == (V, NUM_JOINTS)
        # smpl_pose_kernel walks the joints in their stored order and fetches the parent's transform by a shuffle: parents first
        par = self.parents
        if par.shape != (NUM_JOINTS,) or par[0] != -1 or not all(0 <= par[j] < j for j in range(1, NUM_JOINTS)):
            raise ValueError("SMPLModel: parents must be %d entries with parents[0] == -1 and 0 <= parents[j] < j (parents first), got %s"
                             % (NUM_JOINTS, par.tolist()))
        # the surface (render.MeshRenderer reads it; the skinning stage does not): [F,3] int32 vertex indices, or None
        self.faces = None
        if faces is not None:
            f = np.asarray(faces)
            if f.dtype.kind not in "iu" or f.ndim != 2 or f.shape[1] != 3 or (f.size and (int(f.min()) < 0 or int(f.max()) >= V)):
                raise ValueError("SMPLModel: faces must be integers [F,3] in [0, %d), got %s %s" % (V, f.dtype, f.shape))
            self.faces = np.ascontiguousarray(f, np.int32)
        self._dev = None

    @classmethod
    def synthetic(cls, seed=0, num_verts=NUM_VERTS):
        """Seeded model with the true shapes: body-sized template, small blend shapes,
        row-stochastic joint regressor, 4-sparse skinning weights (as the real model has)."""
        V = num_verts
        v = synth.uniform("smpl.v_template", (V, 3), -1.0, 1.0, seed) * np.array([0.45, 0.9, 0.15], np.float32)
        S = synth.uniform("smpl.shapedirs", (V, 3, NUM_BETAS), -0.03, 0.03, seed)
        P = synth.uniform("smpl.posedirs", (V, 3, NUM_POSE_FEAT), -0.01, 0.01, seed)
        Jr = synth.uniform01("smpl.J_regressor", (NUM_JOINTS, V), seed)
        keep = Jr > 0.97
        none = ~keep.any(1)                 # a small body can leave a joint without an entry above the threshold: it keeps its largest
        keep[none] = Jr[none] == Jr[none].max(1, keepdims=True)
        Jr = np.where(keep, Jr, 0.0)
        Jr = (Jr / Jr.sum(1, keepdims=True)).astype(np.float32)
        u = synth.uniform01("smpl.weights", (V, NUM_JOINTS), seed)
        kth = np.sort(u, axis=1)[:, -4][:, None]
        W = np.where(u >= kth, u, 0.0)
        W = (W / W.sum(1, keepdims=True)).astype(np.float32)
        return cls(v, S, P, Jr, W)

    @classmethod
    def from_npz(cls, path):
        d = np.load(path, allow_pickle=False)
        parents = d["parents"] if "parents" in d else PARENTS
        faces = d["faces"] if "faces" in d else d["f"] if "f" in d else None
        return cls(d["v_template"], d["shapedirs"], d["posedirs"], d["J_regressor"], d["weights"],
                   parents, faces=faces)

    def numpy_dict(self):
        d = {"v_template": self.v_template, "shapedirs": self.shapedirs,
             "posedirs": self.posedirs, "J_regressor": self.J_regressor,
             "weights": self.weights, "parents": self.parents}
        if self.faces is not None:
            d["faces"] = self.faces
        return d


# ----------------------------------------------------------------------------------------------
# device side (csrc/smpl.hip through the C ABI)
def _device_pack(model, device, nnz=None):
    """Layouts the kernels want (include/h3d.h section 4): K-major blend shapes, the joint
    regressor pre-contracted with template/shapedirs (float64 on the host), sparse LBS weights."""
    import torch
    V = model.v_template.shape[0]
    W = model.weights
    if nnz is None:
        nnz = int(max(1, (W != 0).sum(1).max()))
    order = np.argsort(-W, axis=1, kind="stable")[:, :nnz].astype(np.int32)
    wsel = np.take_along_axis(W, order.astype(np.int64), axis=1).astype(np.float32)
    Jr = model.J_regressor.astype(np.float64)
    j_template = (Jr @ model.v_template.astype(np.float64)).astype(np.float32)                 # [24,3]
    j_dirs = np.einsum("jv,vck->jck", Jr, model.shapedirs.astype(np.float64)).astype(np.float32)  # [24,3,10]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    Vpad = ((V + 63) // 64) * 64

    def soa(a):                 # [..., V] -> [..., Vpad] zero padded
        out = np.zeros(a.shape[:-1] + (Vpad,), np.float32)
        out[..., :V] = a
        return out
    return {
        "V": V, "Vpad": Vpad, "nnz": nnz,
        # struct-of-arrays with padded rows: [3][Vpad] and [k][3][Vpad] -- a wave's load of one
        # coordinate is one contiguous, 16-byte aligned row
        "v_template": to(soa(model.v_template.T)),
        "shapedirsT": to(soa(model.shapedirs.transpose(2, 1, 0))),
        "posedirsT": to(soa(model.posedirs.transpose(2, 1, 0))),
        "j_template": to(j_template.reshape(-1)),
        "j_shapedirs": to(j_dirs.reshape(NUM_JOINTS * 3, NUM_BETAS)),
        "parents": to(model.parents.astype(np.int32)),
        "lbs_idx": to(order), "lbs_w": to(wsel),
        # generation 3 (MFMA): K-contiguous direction rows [10 shape | 207 pose | 0], each value as three bf16 terms
        "dirsK3": _dirs_k3(model, Vpad, device),
    }


def _bf16_split3(d):
    """fp32 numpy array -> the bf16 tensors (h, m, lo) of the three-term split: x = h + m + l with h = bf16(x), m = bf16(x - h),
    l = bf16(x - h - m) (round-to-nearest-even at each step, the differences in fp32; exact to 24 significant bits)."""
    import torch
    x = torch.from_numpy(d)
    h = x.to(torch.bfloat16)
    r1 = x - h.float()
    m = r1.to(torch.bfloat16)
    lo = (r1 - m.float()).to(torch.bfloat16)
    return h, m, lo


def _dirs_k3(model, Vpad, device, KP=224):
    """[3][Vpad][KP/16][3 terms][16] bf16: the three-term split (_bf16_split3) of the K-contiguous direction rows -- the operand
    format of csrc/smpl.hip smpl_verts3."""
    import torch
    V = model.v_template.shape[0]
    d = np.zeros((3, Vpad, KP), np.float32)
    d[:, :V, :NUM_BETAS] = model.shapedirs.transpose(1, 0, 2)                      # [V,3,10] -> [3,V,10]
    d[:, :V, NUM_BETAS:NUM_BETAS + NUM_POSE_FEAT] = model.posedirs.transpose(1, 0, 2)
    out = torch.stack([t.reshape(3, Vpad, KP // 16, 16) for t in _bf16_split3(d)], dim=3)     # [3][Vpad][14][3][16]
    return out.contiguous().to(device)


def _dirs_v3(model, Vpad, device, KP=224):
    """[3 terms][KP][3][Vpad] bf16: the three-term split of _dirs_k3 (same rounding) with the vertices contiguous -- the direction
    operand of the transposed contraction of csrc/smpl_bwd.hip (smpl_bwd_coef_kernel)."""
    import torch
    V = model.v_template.shape[0]
    d = np.zeros((KP, 3, Vpad), np.float32)
    d[:NUM_BETAS, :, :V] = model.shapedirs.transpose(2, 1, 0)                      # [V,3,10] -> [10,3,V]
    d[NUM_BETAS:NUM_BETAS + NUM_POSE_FEAT, :, :V] = model.posedirs.transpose(2, 1, 0)
    return torch.stack(_bf16_split3(d), dim=0).contiguous().to(device)


def _pack_for(model, dev, backward=False):
    """The device pack of `model` on `dev`; with backward=True also dirsV3, built on first use (once per model and device)."""
    if model._dev is None or model._dev["v_template"].device != dev:
        model._dev = _device_pack(model, dev)
    d = model._dev
    if backward and "dirsV3" not in d:
        d["dirsV3"] = _dirs_v3(model, d["Vpad"], dev)
    return d


MAX_BACKWARD_NNZ = 4


def lbs_backward(model, betas, thetas, grad_verts=None, grad_joints=None):
    """The gradients of `lbs` (verts [P,V,3], joints [P,24,3]) with respect to betas [P,10] and thetas [P,72], given the upstream
    gradients grad_verts [P,V,3] and / or grad_joints [P,24,3] (None = absent) -> (grad_betas [P,10], grad_thetas [P,72]), fp32.
    Everything is recomputed from betas / thetas (h3d_smpl_backward, include/h3d.h section 4b); the sums run in a fixed order, so two
    calls give the same bits.  Needs <= 4 skinning weights per vertex."""
    import torch
    _lib.require_cuda(betas, thetas, grad_verts, grad_joints)
    dev = betas.device
    d = _pack_for(model, dev, backward=True)
    if d["nnz"] > MAX_BACKWARD_NNZ:
        raise RuntimeError("smpl backward: %d skinning weights per vertex, the limit is %d" % (d["nnz"], MAX_BACKWARD_NNZ))
    betas = betas.detach().contiguous().float()
    P = betas.shape[0]
    thetas = thetas.detach().contiguous().float().view(P, 72)
    if betas.shape != (P, NUM_BETAS):
        raise RuntimeError("lbs_backward: betas [P,10], thetas [P,72]")
    if (grad_verts is not None and grad_verts.shape != (P, d["V"], 3)) or (grad_joints is not None and grad_joints.shape != (P, NUM_JOINTS, 3)):
        raise RuntimeError("lbs_backward: grad_verts [P,V,3], grad_joints [P,24,3]")
    L, gv, gj, ws = _backward_inputs(d, P, dev, grad_verts, grad_joints)
    gb = torch.empty(P, NUM_BETAS, dtype=torch.float32, device=dev)
    gt = torch.empty(P, 72, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.stream_ptr()              # the current stream of `dev`, as the forward
        _lib.check(L.h3d_smpl_backward(_lib.ptr(betas), _lib.ptr(thetas), _lib.ptr(gv), _lib.ptr(gj), *_model_ptrs(d), d["nnz"], P, d["V"],
                                       d["Vpad"], _lib.ptr(gb), _lib.ptr(gt), _lib.ptr(ws), ws.numel() if ws is not None else 0, st), "smpl_backward")
    return gb, gt


def _heads_backward(model, pose_map, shape_map, inds, n, grad_verts, grad_joints):
    """h3d_smpl_heads_backward: -> (grad_pose_map, grad_shape_map), shaped like the maps."""
    import torch
    dev = pose_map.device
    d = _pack_for(model, dev, backward=True)
    B, K = inds.shape
    HW = pose_map.shape[2] * pose_map.shape[3]
    L, gv, gj, ws = _backward_inputs(d, B * n, dev, grad_verts, grad_joints)
    gp = torch.empty_like(pose_map)
    gs = torch.empty_like(shape_map)
    with torch.cuda.device(dev):
        st = _lib.stream_ptr()
        _lib.check(L.h3d_smpl_heads_backward(_lib.ptr(pose_map), _lib.ptr(shape_map), _lib.ptr(inds), B, K, n, HW, _lib.ptr(gv), _lib.ptr(gj),
                                             *_model_ptrs(d), d["nnz"], d["V"], d["Vpad"], _lib.ptr(gp), _lib.ptr(gs), _lib.ptr(ws),
                                             ws.numel() if ws is not None else 0, st), "smpl_heads_backward")
    return gp, gs


def _backward_inputs(d, P, dev, grad_verts, grad_joints):
    """What a call of h3d_smpl_backward / h3d_smpl_heads_backward needs besides the parameters: the library, the upstream gradients as
    dense fp32 (None = absent) and the workspace (None = none needed)."""
    gv = None if grad_verts is None else grad_verts.detach().float().contiguous()       # (an expanded upstream becomes dense here)
    gj = None if grad_joints is None else grad_joints.detach().float().contiguous()
    L = _lib.lib()
    ws = _lib.workspace(L.h3d_smpl_backward_workspace_bytes, P, d["V"], d["Vpad"], d["nnz"], int(gv is not None), device=dev,
                        what="smpl_backward_workspace_bytes")
    return L, gv, gj, ws


def _model_ptrs(d):
    return [_lib.ptr(d[k]) for k in ("j_template", "j_shapedirs", "parents", "v_template", "dirsK3", "dirsV3", "lbs_idx", "lbs_w")]


_functions = None


def _autograd_functions():
    """(lbs Function, lbs_from_heads Function), defined on first use (torch is imported lazily in this module).  The forward inside is
    the kernel the caller asked for; the backward recomputes from the inputs (once_differentiable: no second derivatives)."""
    global _functions
    if _functions is not None:
        return _functions
    import torch
    from torch.autograd.function import once_differentiable

    def _check_nnz(model, dev):
        nnz = _pack_for(model, dev)["nnz"]
        if nnz > MAX_BACKWARD_NNZ:
            raise RuntimeError("smpl backward: %d skinning weights per vertex, the limit is %d (gradients were requested)"
                               % (nnz, MAX_BACKWARD_NNZ))

    class LbsFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, model, kernel, betas, thetas):
            _check_nnz(model, betas.device)
            ctx.model = model
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(betas, thetas)
            return _lbs_forward(model, betas.detach(), thetas.detach(), True, kernel)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_verts, grad_joints):
            betas, thetas = ctx.saved_tensors
            gb, gt = lbs_backward(ctx.model, betas, thetas, grad_verts, grad_joints)
            return None, None, gb.to(betas.dtype).view_as(betas), gt.to(thetas.dtype).view_as(thetas)

    class HeadsFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, model, n, exact, inds, pose_map, shape_map):
            ctx.model, ctx.n = model, n
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(pose_map, shape_map, inds)
            return _lbs_from_heads_forward(model, pose_map.detach(), shape_map.detach(), inds, n, True, exact)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_verts, grad_joints):
            pose_map, shape_map, inds = ctx.saved_tensors
            gp, gs = _heads_backward(ctx.model, pose_map, shape_map, inds, ctx.n, grad_verts, grad_joints)
            return None, None, None, None, gp, gs

    _functions = (LbsFunction, HeadsFunction)
    return _functions


def lbs(model, betas, thetas, return_joints=False, kernel="auto"):
    """betas [P,10], thetas [P,72] (CUDA fp32) -> vertices [P,V,3] (and posed joints [P,24,3]).
    With grad mode on and betas or thetas requiring grad the result carries a graph (gradients by csrc/smpl_bwd.hip, see
    `lbs_backward`; <= 4 skinning weights per vertex); otherwise the call is the plain forward below, launch for launch.
    kernel: "gen3" = blend shapes on the matrix cores (3-term bf16 split; the three 2^-16 products dropped: 2e-6 abs on the displacement),
    "gen3x" = the same with all six products (2^-24: what the f32 parity-mode detectors run), "gen2" = LDS-streamed vector kernel (all
    need <= 4 skinning weights per vertex), "gen1" = register kernel, "auto" = gen3 when applicable and P >= 64, "auto_exact" = gen3x."""
    import torch
    if torch.is_grad_enabled() and (betas.requires_grad or thetas.requires_grad):
        _lib.require_cuda(betas, thetas)
        verts, joints = _autograd_functions()[0].apply(model, kernel, betas, thetas)
        return (verts, joints) if return_joints else verts
    return _lbs_forward(model, betas, thetas, return_joints, kernel)


def _forward_outputs(d, P, dev):
    """Uninitialised pose_feat, A, joints, verts of a forward over P persons."""
    import torch
    return (torch.empty(P, NUM_POSE_FEAT, dtype=torch.float32, device=dev), torch.empty(P, NUM_JOINTS, 12, dtype=torch.float32, device=dev),
            torch.empty(P, NUM_JOINTS, 3, dtype=torch.float32, device=dev), torch.empty(P, d["V"], 3, dtype=torch.float32, device=dev))


def _verts3(L, d, coefK, A, verts, P, Ppad, exact, st):
    """The generation-3 vertex launch on a filled coefficient operand and A."""
    fn = L.h3d_smpl_verts3_exact if exact else L.h3d_smpl_verts3
    _lib.check(fn(_lib.ptr(coefK), _lib.ptr(A), _lib.ptr(d["v_template"]), _lib.ptr(d["dirsK3"]), _lib.ptr(d["lbs_idx"]), _lib.ptr(d["lbs_w"]),
                  d["nnz"], P, Ppad, d["V"], d["Vpad"], _lib.ptr(verts), st), "smpl_verts3")


def _lbs_forward(model, betas, thetas, return_joints, kernel):
    import torch
    _lib.require_cuda(betas, thetas)
    dev = betas.device
    d = _pack_for(model, dev)
    betas = betas.contiguous().float()
    thetas = thetas.contiguous().float().view(betas.shape[0], 72)
    P = betas.shape[0]
    pf, A, joints, verts = _forward_outputs(d, P, dev)
    L = _lib.lib()
    gen3 = kernel in ("gen3", "gen3x") or (kernel in ("auto", "auto_exact") and d["nnz"] <= 4 and P >= 64)
    exact = kernel in ("gen3x", "auto_exact")
    gen2 = kernel == "gen2"
    Ppad = ((P + 127) // 128) * 128
    coefT = torch.zeros(NUM_BETAS + NUM_POSE_FEAT, Ppad, dtype=torch.float32, device=dev) if gen2 else None
    with torch.cuda.device(dev):
        st = _lib.stream_ptr()              # the current stream of `dev` (not of whatever device was current at the call)
        _lib.check(L.h3d_smpl_pose(_lib.ptr(betas), _lib.ptr(thetas), _lib.ptr(d["j_template"]),
                                   _lib.ptr(d["j_shapedirs"]), _lib.ptr(d["parents"]), P, _lib.ptr(pf),
                                   _lib.ptr(A), _lib.ptr(joints), _lib.ptr(coefT), Ppad, st), "smpl_pose")
        if gen3:
            coefK = torch.empty(Ppad, 14, 3, 16, dtype=torch.bfloat16, device=dev)
            _lib.check(L.h3d_smpl_coef_pack(_lib.ptr(betas), _lib.ptr(pf), P, Ppad, _lib.ptr(coefK), st), "smpl_coef_pack")
            _verts3(L, d, coefK, A, verts, P, Ppad, exact, st)
        elif gen2:
            _lib.check(L.h3d_smpl_verts2(_lib.ptr(coefT), _lib.ptr(A), _lib.ptr(d["v_template"]),
                                         _lib.ptr(d["shapedirsT"]), _lib.ptr(d["posedirsT"]), _lib.ptr(d["lbs_idx"]),
                                         _lib.ptr(d["lbs_w"]), d["nnz"], P, Ppad, d["V"], d["Vpad"], _lib.ptr(verts), st),
                       "smpl_verts2")
        else:
            _lib.check(L.h3d_smpl_verts(_lib.ptr(betas), _lib.ptr(pf), _lib.ptr(A), _lib.ptr(d["v_template"]),
                                        _lib.ptr(d["shapedirsT"]), _lib.ptr(d["posedirsT"]), _lib.ptr(d["lbs_idx"]),
                                        _lib.ptr(d["lbs_w"]), d["nnz"], P, d["V"], d["Vpad"], _lib.ptr(verts), st),
                       "smpl_verts")
    return (verts, joints) if return_joints else verts


def lbs_from_heads(model, pose_map, shape_map, inds, n, return_joints=False, exact=False):
    """The detector's SMPL stage straight from the network's outputs: pose_map [B,72,H,W], shape_map [B,10,H,W] (contiguous fp32
    head maps), inds [B,K] int64 (the decode's centre indices), the first `n` detections of every image -> vertices
    [B*n,V,3] (and joints [B*n,24,3]).  Two launches -- `h3d_smpl_pose_heads` (gathers + Rodrigues + kinematic chain + the
    generation-3 coefficient operand) and `h3d_smpl_verts3` -- instead of the five of `_transpose_and_gather_feat` x 2 + `lbs`;
    bit-identical to them (tests/test_gpu_smpl.py).  Needs <= 4 skinning weights per vertex (generation 3).
    With grad mode on and pose_map or shape_map requiring grad the result carries a graph: the gradients arrive at the maps
    (h3d_smpl_heads_backward: zero off the gathered pixels, detections that share a pixel add up)."""
    import torch
    if torch.is_grad_enabled() and (pose_map.requires_grad or shape_map.requires_grad):
        _lib.require_cuda(pose_map, shape_map, inds)
        verts, joints = _autograd_functions()[1].apply(model, n, exact, inds, pose_map, shape_map)
        return (verts, joints) if return_joints else verts
    return _lbs_from_heads_forward(model, pose_map, shape_map, inds, n, return_joints, exact)


def _lbs_from_heads_forward(model, pose_map, shape_map, inds, n, return_joints, exact):
    import torch
    _lib.require_cuda(pose_map, shape_map, inds)
    dev = pose_map.device
    d = _pack_for(model, dev)
    if d["nnz"] > 4:
        raise RuntimeError("lbs_from_heads: more than 4 skinning weights per vertex (use lbs)")
    if (pose_map.dtype != torch.float32 or shape_map.dtype != torch.float32 or not pose_map.is_contiguous() or not shape_map.is_contiguous()
            or inds.dtype != torch.int64 or not inds.is_contiguous()):
        raise RuntimeError("lbs_from_heads: contiguous fp32 head maps and int64 indices expected")
    B, K = inds.shape
    HW = pose_map.shape[2] * pose_map.shape[3]
    if pose_map.shape[:2] != (B, 72) or shape_map.shape[:2] != (B, NUM_BETAS) or shape_map.shape[2:] != pose_map.shape[2:] or not 0 < n <= K:
        raise RuntimeError("lbs_from_heads: pose [B,72,H,W], shape [B,10,H,W], inds [B,K], 0 < n <= K")
    P = B * n
    Ppad = ((P + 127) // 128) * 128
    pf, A, joints, verts = _forward_outputs(d, P, dev)
    coefK = torch.empty(Ppad, 14, 3, 16, dtype=torch.bfloat16, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        st = _lib.stream_ptr()              # the current stream of `dev`
        _lib.check(L.h3d_smpl_pose_heads(_lib.ptr(pose_map), _lib.ptr(shape_map), _lib.ptr(inds), B, K, n, HW, _lib.ptr(d["j_template"]),
                                         _lib.ptr(d["j_shapedirs"]), _lib.ptr(d["parents"]), None, _lib.ptr(pf), _lib.ptr(A), _lib.ptr(joints),
                                         _lib.ptr(coefK), Ppad, st), "smpl_pose_heads")
        _verts3(L, d, coefK, A, verts, P, Ppad, exact, st)
    return (verts, joints) if return_joints else verts
