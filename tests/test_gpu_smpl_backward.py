"""GPU: the SMPL backward (csrc/smpl_bwd.hip) through `smpl.lbs_backward`, autograd through `smpl.lbs` and `smpl.lbs_from_heads`.

The rule of every comparison (tests/smpl_grad_ref.py, which takes it from smpl_ref.check; per case, per gradient tensor): e32 = max |float32
autograd of the torch restatement - its float64 autograd| on the same inputs, and max |gpu - f64| <= 4 * e32 + 2^-23 * max |f64|.  Bodies are
`jointed_model`s, poses `special_thetas` (the 12 pose edges wherever P >= 12), upstream gradients N(0,1) fp32.  The observed ratios are
printed (`pytest -s`) and the largest per tensor recorded in DESIGN.md."""
import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
import smpl_grad_ref as G
import smpl_ref as R
from h3d_amd import smpl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_MODELS, _CASES = {}, {}


def body(V, max_nnz=4):
    if (V, max_nnz) not in _MODELS:
        _MODELS[(V, max_nnz)] = smpl.SMPLModel(**R.jointed_model(V, 0, max_nnz))
    return _MODELS[(V, max_nnz)]


class Case:
    """One (body, persons) pair with its upstream gradients; the references are computed once per upstream combination and shared."""

    def __init__(self, V, P, seed):
        self.m, self.V, self.P = body(V), V, P
        self.betas, self.thetas = R.make_case(P, seed)
        rs = np.random.RandomState(500 + seed)
        self.gv, self.gj = rs.randn(P, V, 3).astype(np.float32), rs.randn(P, 24, 3).astype(np.float32)
        self.bt, self.tt = torch.from_numpy(self.betas).to(DEV), torch.from_numpy(self.thetas).to(DEV)
        self.gvt, self.gjt = torch.from_numpy(self.gv).to(DEV), torch.from_numpy(self.gj).to(DEV)
        self.name = "V%d P%d" % (V, P)
        self._ref = {}

    def ref(self, use_v, use_j):
        if (use_v, use_j) not in self._ref:
            self._ref[(use_v, use_j)] = G.bounds(self.betas, self.thetas, self.m.numpy_dict(), self.gv if use_v else None, self.gj if use_j else None)
        return self._ref[(use_v, use_j)]

    def run(self, use_v=True, use_j=True):
        return smpl.lbs_backward(self.m, self.bt, self.tt, self.gvt if use_v else None, self.gjt if use_j else None)


def case(V, P, seed=1):
    if (V, P, seed) not in _CASES:
        _CASES[(V, P, seed)] = Case(V, P, seed)
    return _CASES[(V, P, seed)]


# V = 100, 193: not multiples of the 64-vertex tile (193 = three full tiles and one lane); P = 1, 3: an odd person in the two-per-wave pose
# kernel, 13: every pose edge, 130: past one 128-person pad / a wave's 32; V = 64, P = 257: past the 256-person workgroup tile
@pytest.mark.parametrize("V,P", [(V, P) for V in (100, 193) for P in (1, 3, 13, 130)] + [(64, 257)])
def test_parity_by_the_rule(V, P):
    c = case(V, P)
    got = c.run()
    assert all(bool(torch.isfinite(g).all()) for g in got)
    c_ref, e32 = c.ref(True, True)
    G.check(c.name + " both", got, c_ref, e32)


def test_the_three_upstream_combinations():
    c = case(100, 13)
    only_v, only_j, both = c.run(True, False), c.run(False, True), c.run(True, True)
    G.check(c.name + " grad_verts only", only_v, *c.ref(True, False))
    G.check(c.name + " grad_joints only", only_j, *c.ref(False, True))
    _, e32 = c.ref(True, True)
    summed = [(a.double() + b.double()).cpu().numpy() for a, b in zip(only_v, only_j)]
    G.check(c.name + " both against the sum of the singles", both, summed, e32)


def test_closed_form_rest_pose_vertex_gradient():
    m, P, V = body(100), 3, 100
    betas = np.random.RandomState(1).randn(P, 10).astype(np.float32)
    thetas = np.zeros((P, 72), np.float32)
    gv = np.random.RandomState(2).randn(P, V, 3).astype(np.float32)
    gb, gt = smpl.lbs_backward(m, torch.from_numpy(betas).to(DEV), torch.from_numpy(thetas).to(DEV), torch.from_numpy(gv).to(DEV), None)
    (rb, rt), e32 = G.bounds(betas, thetas, m.numpy_dict(), gv, None)
    rowsum = m.weights.astype(np.float64).sum(1)
    want = np.einsum("pvc,vck->pk", gv.astype(np.float64) * rowsum[None, :, None], m.shapedirs.astype(np.float64))
    assert np.abs(want - rb).max() <= 1e-12 * np.abs(rb).max()
    G.check("rest pose closed form", (gb, gt), [want, rt], e32)


def test_closed_form_root_joint_gradient():
    m, P = body(100), 3
    betas, thetas = R.make_case(P, 9)
    gj = np.zeros((P, 24, 3), np.float32)
    gj[:, 0] = np.random.RandomState(4).randn(P, 3)
    gb, gt = smpl.lbs_backward(m, torch.from_numpy(betas).to(DEV), torch.from_numpy(thetas).to(DEV), None, torch.from_numpy(gj).to(DEV))
    (rb, rt), e32 = G.bounds(betas, thetas, m.numpy_dict(), None, gj)
    jsd = np.einsum("v,vck->ck", m.J_regressor[0].astype(np.float64), m.shapedirs.astype(np.float64))
    want = gj[:, 0].astype(np.float64) @ jsd
    assert np.abs(want - rb).max() <= 1e-12 * np.abs(rb).max() and np.abs(rt).max() == 0
    G.check("root joint closed form", (gb, gt), [want, np.zeros((P, 72))], e32)
    assert float(gt.abs().max()) == 0.0


def test_two_calls_give_the_same_bits():
    c = case(193, 130)
    a, b = c.run(), c.run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_zero_and_absent_upstreams():
    c = case(100, 3)
    gb, gt = smpl.lbs_backward(c.m, c.bt, c.tt, None, None)
    assert float(gb.abs().max()) == 0.0 and float(gt.abs().max()) == 0.0
    gb, gt = smpl.lbs_backward(c.m, c.bt, c.tt, torch.zeros_like(c.gvt), torch.zeros_like(c.gjt))
    assert float(gb.abs().max()) == 0.0 and float(gt.abs().max()) == 0.0


def test_autograd_through_lbs_is_lbs_backward():
    c = case(100, 13)
    b, t = c.bt.clone().requires_grad_(True), c.tt.clone().requires_grad_(True)
    verts, joints = smpl.lbs(c.m, b, t, return_joints=True, kernel="gen3x")
    assert verts.grad_fn is not None and joints.grad_fn is not None
    plain = smpl.lbs(c.m, c.bt, c.tt, return_joints=True, kernel="gen3x")
    assert torch.equal(verts.detach(), plain[0]) and torch.equal(joints.detach(), plain[1])
    ((verts * c.gvt).sum() + (joints * c.gjt).sum()).backward()
    gb, gt = c.run()
    assert torch.equal(b.grad, gb) and torch.equal(t.grad, gt)


def test_autograd_with_an_expanded_upstream():
    c = case(100, 13)
    b, t = c.bt.clone().requires_grad_(True), c.tt.clone().requires_grad_(True)
    smpl.lbs(c.m, b, t).sum().backward()
    ones = np.ones((c.P, c.V, 3), np.float32)
    target, e32 = G.bounds(c.betas, c.thetas, c.m.numpy_dict(), ones, None)
    G.check(c.name + " verts.sum()", (b.grad, t.grad), target, e32)


def test_no_graph_without_requires_grad_or_under_no_grad():
    c = case(100, 3)
    verts, joints = smpl.lbs(c.m, c.bt, c.tt, return_joints=True)
    assert verts.grad_fn is None and joints.grad_fn is None and not verts.requires_grad
    b = c.bt.clone().requires_grad_(True)
    with torch.no_grad():
        verts = smpl.lbs(c.m, b, c.tt)
    assert verts.grad_fn is None and not verts.requires_grad


def test_lbs_from_heads_delivers_the_gradients_at_the_maps():
    m, B, K, n, H, W, V = body(100), 2, 5, 3, 8, 8, 100
    rs = np.random.RandomState(11)
    pose = (rs.randn(B, 72, H, W) * 0.5).astype(np.float32)
    shape = rs.randn(B, 10, H, W).astype(np.float32)
    inds = np.stack([rs.permutation(H * W)[:K] for _ in range(B)]).astype(np.int64)
    inds[1, 1] = inds[1, 0]                           # image 1: detections 0 and 1 on the same pixel
    pix = inds[:, :n]
    pose[0, :, pix[0, 0] // W, pix[0, 0] % W] = 0.0   # one person at the rest pose
    P = B * n
    gv, gj = rs.randn(P, V, 3).astype(np.float32), rs.randn(P, 24, 3).astype(np.float32)
    pm, sm = torch.from_numpy(pose).to(DEV).requires_grad_(True), torch.from_numpy(shape).to(DEV).requires_grad_(True)
    it = torch.from_numpy(inds).to(DEV)
    verts, joints = smpl.lbs_from_heads(m, pm, sm, it, n, return_joints=True, exact=True)
    assert verts.grad_fn is not None
    with torch.no_grad():
        plain = smpl.lbs_from_heads(m, pm, sm, it, n, return_joints=True, exact=True)
    assert torch.equal(verts.detach(), plain[0]) and torch.equal(joints.detach(), plain[1])
    ((verts * torch.from_numpy(gv).to(DEV)).sum() + (joints * torch.from_numpy(gj).to(DEV)).sum()).backward()
    gp, gs = pm.grad.cpu().numpy().reshape(B, 72, H * W), sm.grad.cpu().numpy().reshape(B, 10, H * W)
    # zero off the gathered pixels
    off = np.ones((B, H * W), bool)
    for b in range(B):
        off[b, pix[b]] = False
    assert not gp.transpose(0, 2, 1)[off].any() and not gs.transpose(0, 2, 1)[off].any()
    # on them: the gradients of the gathered parameters, summed where two detections share a pixel
    thetas = np.stack([pose.reshape(B, 72, -1)[b][:, pix[b]].T for b in range(B)]).reshape(P, 72)
    betas = np.stack([shape.reshape(B, 10, -1)[b][:, pix[b]].T for b in range(B)]).reshape(P, 10)
    def maps(dtype):                                   # the restatement's gradients, scattered as the maps receive them
        rb, rt = [g.double().numpy() for g in G.grads(betas, thetas, m.numpy_dict(), gv, gj, dtype)]
        ws, wp = np.zeros((B, 10, H * W)), np.zeros((B, 72, H * W))
        for p in range(P):
            ws[p // n, :, pix[p // n, p % n]] += rb[p]
            wp[p // n, :, pix[p // n, p % n]] += rt[p]
        return ws, wp
    want, m32 = maps(torch.float64), maps(torch.float32)
    e32 = [float(np.abs(a - r).max()) for a, r in zip(m32, want)]          # the rule's e32, of the map tensors themselves
    G.check("heads maps", (gs, gp), want, e32)
    # the same against the device's own lbs_backward of the gathered parameters
    db, dt = smpl.lbs_backward(m, torch.from_numpy(betas).to(DEV), torch.from_numpy(thetas).to(DEV), torch.from_numpy(gv).to(DEV),
                               torch.from_numpy(gj).to(DEV))
    db, dt = db.cpu().numpy(), dt.cpu().numpy()
    for p in (0, 2, 5):                                # persons alone on their pixel: the same arithmetic, the same bits
        assert np.array_equal(gs[p // n, :, pix[p // n, p % n]], db[p]) and np.array_equal(gp[p // n, :, pix[p // n, p % n]], dt[p])
    shared = pix[1, 0]
    assert np.allclose(gs[1, :, shared], db[3] + db[4], rtol=0, atol=2.0 ** -22 * np.abs(db[3:5]).max())
    assert np.allclose(gp[1, :, shared], dt[3] + dt[4], rtol=0, atol=2.0 ** -22 * np.abs(dt[3:5]).max())


def test_five_skinning_weights_raise_when_gradients_are_requested():
    m = body(100, max_nnz=5)
    betas, thetas = R.make_case(3, 2)
    bt, tt = torch.from_numpy(betas).to(DEV), torch.from_numpy(thetas).to(DEV)
    verts = smpl.lbs(m, bt, tt)                        # the forward still runs (the dense skinning loop)
    assert verts.shape == (3, 100, 3) and bool(torch.isfinite(verts).all())
    with pytest.raises(RuntimeError, match="limit is 4"):
        smpl.lbs(m, bt.clone().requires_grad_(True), tt)
    with pytest.raises(RuntimeError, match="limit is 4"):
        smpl.lbs_backward(m, bt, tt, torch.zeros(3, 100, 3, device=DEV), None)
