"""GPU: the SMPL backward (csrc/smpl_bwd.hip) through `smpl.lbs_backward`, autograd through `smpl.lbs` and `smpl.lbs_from_heads`.

The rule of every comparison (tests/smpl_grad_ref.py, which takes it from smpl_ref.check; per case, per gradient tensor): e32 = max |float32
autograd of the torch restatement - its float64 autograd| on the same inputs, and max |gpu - f64| <= 4 * e32 + 2^-23 * max |f64|.  Bodies are
`jointed_model`s, poses `special_thetas` (the 12 pose edges wherever P >= 12), upstream gradients N(0,1) fp32.  The observed ratios are
printed (`pytest -s`) and the largest per tensor recorded in DESIGN.md.

The same rule person by person (G.check_per_person: e32[p] over person p's row, floored at the median over the persons) runs beside it
wherever a test names it: one near-singular pose sets the whole tensor's e32 several hundred times above an ordinary person's, and the
whole-tensor rule then checks the ordinary persons' grad_thetas to 1e-4 relative only.  The cases from V = 256 up give the kernels more
than one partial of everything: tile groups of the vertex kernel, contraction splits of the coefficient kernel, the pose kernel's loops
over both (counts: G.groups / G.splits, pinned to the sources in tests/test_oracle_smpl_backward.py)."""
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

    def ref_pp(self, use_v, use_j):
        """(target, e32 per person) of G.bounds_per_person, computed once."""
        if (use_v, use_j) not in self._ref:
            self._ref[(use_v, use_j)] = G.bounds_per_person(self.betas, self.thetas, self.m.numpy_dict(), self.gv if use_v else None,
                                                            self.gj if use_j else None)
        return self._ref[(use_v, use_j)]

    def ref(self, use_v, use_j):
        """(target, e32) of G.bounds: the whole tensor's e32 is the largest person's."""
        target, e32 = self.ref_pp(use_v, use_j)
        return target, [float(e.max()) for e in e32]

    def run(self, use_v=True, use_j=True):
        return smpl.lbs_backward(self.m, self.bt, self.tt, self.gvt if use_v else None, self.gjt if use_j else None)

    def check_both(self, what, got, use_v=True, use_j=True):
        """Both rules against this case's references; -> (whole-tensor ratios err / e32, per-person ratios err / limit)."""
        return (G.check("%s %s" % (self.name, what), got, *self.ref(use_v, use_j)),
                G.check_per_person("%s %s" % (self.name, what), got, *self.ref_pp(use_v, use_j)))


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
    G.check_per_person(c.name + " both", got, *c.ref_pp(True, True))


def test_the_three_upstream_combinations():
    c = case(100, 13)
    only_v, only_j, both = c.run(True, False), c.run(False, True), c.run(True, True)
    G.check(c.name + " grad_verts only", only_v, *c.ref(True, False))
    G.check(c.name + " grad_joints only", only_j, *c.ref(False, True))
    G.check_per_person(c.name + " grad_verts only", only_v, *c.ref_pp(True, False))
    G.check_per_person(c.name + " grad_joints only", only_j, *c.ref_pp(False, True))
    _, e32 = c.ref(True, True)
    summed = [(a.double() + b.double()).cpu().numpy() for a, b in zip(only_v, only_j)]
    G.check(c.name + " both against the sum of the singles", both, summed, e32)
    G.check_per_person(c.name + " both against the sum of the singles", both, summed, c.ref_pp(True, True)[1])


# ---- several partials of everything: NG tile groups, NS contraction splits (G.groups / G.splits; the table is pinned in
# tests/test_oracle_smpl_backward.py).  V = 256: one full group; 257: a second group of one tile holding one real vertex; 512: 3 Vpad = exactly
# one split; 513: a last group of one tile and a last split of 192 elements; 1024: both exact; 6890: the real mesh, 27 groups and 14 splits
# with a last split of 768.  P = 3 everywhere; (257, 257): two person blocks of the vertex kernel x two groups; (513, 130): two workgroups
# of the coefficient kernel x two splits, the last wave holding 2 persons; (6890, 13): every pose edge.
PARTIAL_CASES = [(V, 3) for V in (256, 257, 512, 513, 1024, 6890)] + [(257, 257), (513, 130), (6890, 13)]


@pytest.mark.parametrize("V,P", PARTIAL_CASES)
def test_vertex_counts_with_several_groups_and_splits(V, P):
    c = case(V, P)
    print("%s: Vpad %d, %d tile groups, %d splits" % (c.name, G.vpad(V), G.groups(V), G.splits(V)))
    got = c.run()
    assert all(bool(torch.isfinite(g).all()) for g in got)
    c.check_both("both", got)
    again = c.run()
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


class GroupCase(Case):
    """Case(V, 3) whose grad_verts is non-zero only on the real vertices of tile group `g`, without a grad_joints: every other group's
    partial slot holds zeros, so a contribution that lands in, or is read from, another slot is lost or doubled."""

    def __init__(self, V, g, seed=1):
        Case.__init__(self, V, 3, seed)
        lo, hi = g * G.GROUP_TILES * G.TILE, min((g + 1) * G.GROUP_TILES * G.TILE, V)
        assert 0 <= lo < hi
        self.gv[:, :lo] = 0.0
        self.gv[:, hi:] = 0.0
        self.gvt = torch.from_numpy(self.gv).to(DEV)
        self.name = "V%d P3 group %d [%d,%d)" % (V, g, lo, hi)


def group_case(V, g):
    if (V, "group", g) not in _CASES:
        _CASES[(V, "group", g)] = GroupCase(V, g)
    return _CASES[(V, "group", g)]


@pytest.mark.parametrize("V,gs", [(513, (0, 1, 2)), (6890, (0, 13, 26))])
def test_each_tile_group_alone(V, gs):
    assert max(gs) == G.groups(V) - 1
    got = {}
    for g in gs:
        c = group_case(V, g)
        got[g] = c.run(True, False)
        target, _ = c.ref(True, False)
        print("%s: max |f64| grad_betas %.3g grad_thetas %.3g" % (c.name, np.abs(target[0]).max(), np.abs(target[1]).max()))
        assert np.abs(target[0]).max() > 0.01 and np.abs(target[1]).max() > 0.1            # a single group's gradient is not nothing
        c.check_both("grad_verts only", got[g], True, False)
    if len(gs) == G.groups(V):
        # the three groups cover the mesh and the upstream is the full case's, cut up: the gradients add up (fp64 sum of the device's
        # three results) to the full upstream's, within the full upstream's own limits
        full = case(V, 3)
        assert np.array_equal(sum(group_case(V, g).gv for g in gs), full.gv)
        summed = [sum(got[g][i].double().cpu().numpy() for g in gs) for i in range(2)]
        full.check_both("the sum of the single groups against the full upstream", summed, True, False)


def test_a_dirty_workspace_changes_nothing():
    """The partial slots, g_vp and the forward intermediates live in a workspace the allocator hands back unchanged: a call at another
    mesh size and person count in between leaves its values where the next call's slots are."""
    small, large = case(513, 130), case(6890, 13)
    first = small.run()
    mid = large.run()
    third = small.run()
    assert torch.equal(first[0], third[0]) and torch.equal(first[1], third[1])
    small.check_both("after a larger call", third)
    large.check_both("between two smaller calls", mid)


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
    heads_maps_scheme(100, per_person=False)


def test_heads_entry_with_several_partials():
    """The heads entry point (h3d_smpl_heads_backward shares sb_run) at V = 577: 3 tile groups, the last of two tiles, and 2 splits, the last of
    192 elements.  The per-person rule runs over the gathered pixels: a row is one pixel's 10 / 72 map values."""
    assert (G.groups(577), G.splits(577)) == (3, 2)
    heads_maps_scheme(577, per_person=True)


def heads_maps_scheme(V, per_person):
    m, B, K, n, H, W = body(V), 2, 5, 3, 8, 8
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
    G.check("V%d heads maps" % V, (gs, gp), want, e32)
    if per_person:                                     # the rule row by row, a row = one gathered pixel (the shared one holds two persons' sum)
        at = sorted({(b, int(q)) for b in range(B) for q in pix[b]})
        rows = lambda t: np.stack([t[b, :, q] for b, q in at])
        e32_rows = [np.abs(rows(a) - rows(r)).max(1) for a, r in zip(m32, want)]
        assert len(at) == P - 1
        G.check_per_person("V%d heads maps" % V, [rows(gs), rows(gp)], [rows(w) for w in want], e32_rows)
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
