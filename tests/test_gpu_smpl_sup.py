"""GPU: the SMPL 3D supervision (csrc/smpl_sup.hip) -- the label transform through `smpl_sup.smpl_targets`, the three-term loss through
`smpl_sup.supervised_loss_forward / _backward` and under autograd through `smpl_sup.smpl_supervised_loss` (with joints given, and on top
of `smpl.lbs_from_heads`), `train_input.multi_pose_train_batch(..., smpl_labels=)` and `trainer.HeadsTrainer` with the terms switched on.

Labels: every output within 2^-24 + 1e-12 (times max |J| for the joints) of the numpy float64 mirror (tests/smpl_sup_ref.py) -- fp64
arithmetic rounded once; smpl_shape and the weights bit-equal.  Loss and gradients: max |gpu - f64| <= 4 e32 + 1e-7 max |f64| per tensor,
e32 = the float32 restatement's error; the loss scalars pooled over the cases.  The loss is smooth: nothing is excluded.  At theta = 0,
where e32 is large, the pose gradient is held to its closed form instead.  The observed ratios are printed (`pytest -s`) and the largest
recorded in DESIGN.md section 34."""
import copy
import random
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import heads_grad_ref as HR
import losses_ref as LR
import optim_ref
import smpl_grad_ref as G
import smpl_ref as R
import smpl_sup_ref as SR
import targets_ref
import test_gpu_optim as O
from h3d_amd import arch, model, smpl, smpl_sup, synth, train_input, trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = 100
SENT = 777.0
TOL = 2.0 ** -24 + 1e-12

_CASES, _BODY = {}, []


def body():
    if not _BODY:
        _BODY.append(smpl.SMPLModel(**R.jointed_model(V)))
    return _BODY[0]


# ---- the label transform ---------------------------------------------------------------------------------------------------------------------
class LabelCase:
    """B = 3 images, M = 5 annotations, max_objs = 4: image 0 holds five (one beyond max_objs), image 1 none, image 2 three; reg_mask is 0
    in the middle of image 0; valid = 0 rows carry NaN labels."""

    def __init__(self, seed=5):
        rs = np.random.RandomState(seed)
        self.B, self.M, self.N = 3, 5, 4
        B, M, N = self.B, self.M, self.N
        self.pose = (rs.randn(B, M, 72) * 0.6).astype(np.float32)
        self.pose[0, 0, 3:6] = 0.0                           # a joint at the rest pose
        self.pose[2, 0, 0:3] = 3.1 * np.array([0.6, 0.0, 0.8])
        self.shape = rs.randn(B, M, 10).astype(np.float32)
        self.joints = (rs.randn(B, M, 24, 3) * 1.5).astype(np.float32)
        self.valid = np.ones((B, M), np.float32)
        self.valid[0, 3], self.valid[2, 1], self.valid[2, 2] = 0.0, 0.0, 0.5
        for b, m in ((0, 3), (2, 1)):
            self.pose[b, m], self.shape[b, m], self.joints[b, m] = np.nan, np.nan, np.nan
        self.num = np.array([5, 0, 3], np.int32)
        self.reg_mask = np.ones((B, N), np.uint8)
        self.reg_mask[0, 1] = 0
        self.pose_w = ((rs.rand(B, M, 24) < 0.7) * (0.5 + rs.rand(B, M, 24))).astype(np.float32)
        self.joints_w = ((rs.rand(B, M, 24) < 0.7) * (0.5 + rs.rand(B, M, 24))).astype(np.float32)
        self.c = np.array([[30.0, 22.0], [28.0, 20.0], [33.5, 25.0]], np.float32)
        self.s = np.array([64.0, 56.0, 70.0])
        self.opt = NS(max_objs=N, output_res=16)

    def run(self, flipped, rot, weights, with_joints=True, out=None):
        kw = dict(pose_weight=self.pose_w, joint_weight=self.joints_w if with_joints else None) if weights else {}
        return smpl_sup.smpl_targets(self.pose, self.shape, self.valid, self.num, torch.from_numpy(self.reg_mask).to(DEV), rot=rot, flipped=flipped,
                                     c=self.c, s=self.s, joints=self.joints if with_joints else None, opt=self.opt, out=out, **kw)

    def mirror(self, flipped, rot, weights, with_joints=True):
        rot2 = smpl_sup.rot2_from_params(self.c, self.s, rot, 16, 16)
        return SR.labels_np(self.pose, self.shape, self.joints if with_joints else None, self.valid, self.pose_w if weights else None,
                            self.joints_w if (weights and with_joints) else None, self.num, self.reg_mask, flipped, rot2, self.N)


def check_labels(name, got, want):
    for nm in SR.NAMES:
        g, w = got[nm].cpu(), want[nm]
        assert tuple(g.shape) == w.shape and g.dtype == torch.float32, nm
        if nm in ("smpl_rotmat", "smpl_joints"):
            scale = 1.0 if nm == "smpl_rotmat" else float(np.abs(w).max())
            err = float(np.abs(g.double().numpy() - w).max())
            print("%s %s: err %.3g limit %.3g" % (name, nm, err, TOL * scale))
            assert err <= TOL * scale, (name, nm, err)
            zero = (want["smpl_pose_w" if nm == "smpl_rotmat" else "smpl_joints_w"] == 0)
            assert not g.numpy()[zero].any(), (name, nm)                         # entries with weight 0 hold zeros
        else:
            assert torch.equal(g, torch.from_numpy(w.astype(np.float32))), (name, nm)


FLIP, ROT = np.array([1, 0, 1]), np.array([0.0, -30.0, 17.0])


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("flags", ["neither", "flipped", "rot", "both"])
def test_labels_against_the_float64_mirror(flags, weights):
    c = LabelCase()
    flipped = FLIP if flags in ("flipped", "both") else None
    rot = ROT if flags in ("rot", "both") else None
    got = c.run(flipped, rot, weights)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    want = c.mirror(flipped, rot, weights)
    check_labels(flags, got, want)
    assert float(got["smpl_pose_w"][0, 0].abs().max()) > 0 and not got["smpl_pose_w"][1].any() and not got["smpl_pose_w"][0, 1].any()
    assert not got["smpl_shape_w"][2, 3].any() and not got["smpl_rotmat"][0, 3].any()          # beyond num; valid = 0


def test_labels_without_joints_into_misaligned_buffers_with_sentinels():
    c = LabelCase()
    PAD = 9                                                       # 9 floats in front: every view starts 4 bytes past a 16-byte boundary
    specs = smpl_sup.label_specs(c.B, c.N)
    bufs = {k: torch.full((int(np.prod(s)) + 2 * PAD,), SENT, device=DEV) for k, s in specs.items()}
    views = {k: bufs[k][PAD:PAD + int(np.prod(s))].view(s) for k, s in specs.items()}
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views.values())
    got = c.run(FLIP, ROT, True, out=views)
    torch.cuda.synchronize()
    assert all(got[k].data_ptr() == views[k].data_ptr() for k in specs)
    check_labels("sentinels", got, c.mirror(FLIP, ROT, True))
    for k, s in specs.items():
        n = int(np.prod(s))
        assert bool((bufs[k][:PAD] == SENT).all()) and bool((bufs[k][PAD + n:] == SENT).all()) and not bool((views[k] == SENT).any()), k
    none = c.run(FLIP, ROT, False, with_joints=False)             # no joints and no model: the joint term gets weight 0
    check_labels("no joints", none, c.mirror(FLIP, ROT, False, with_joints=False))
    assert not none["smpl_joints"].any() and not none["smpl_joints_w"].any()


def test_labels_with_joints_from_the_model_and_the_refusals():
    c = LabelCase()
    pose, shape = np.nan_to_num(c.pose), np.nan_to_num(c.shape)
    rm = torch.from_numpy(c.reg_mask).to(DEV)
    got = smpl_sup.smpl_targets(pose, shape, c.valid, c.num, rm, rot=ROT, flipped=FLIP, c=c.c, s=c.s, smpl_model=body(), opt=c.opt)
    _, j = smpl.lbs(body(), torch.from_numpy(shape).to(DEV).reshape(-1, 10), torch.from_numpy(pose).to(DEV).reshape(-1, 72), return_joints=True,
                    kernel="auto_exact")
    want = smpl_sup.smpl_targets(pose, shape, c.valid, c.num, rm, rot=ROT, flipped=FLIP, c=c.c, s=c.s, joints=j.view(c.B, c.M, 24, 3), opt=c.opt)
    assert all(torch.equal(got[k], want[k]) for k in SR.NAMES) and float(got["smpl_joints_w"].sum()) > 0
    with pytest.raises(ValueError, match="per-axis"):
        smpl_sup.smpl_targets(pose, shape, c.valid, c.num, rm, rot=ROT, c=c.c, s=np.stack([c.s, c.s], 1), opt=c.opt)
    with pytest.raises(RuntimeError, match=r"\[B,max_objs\]"):
        smpl_sup.smpl_targets(pose, shape, c.valid, c.num, rm[:, :3].contiguous(), opt=c.opt)
    with pytest.raises(RuntimeError, match=r"\[B,M,72\]"):
        smpl_sup.smpl_targets(pose[..., :69], shape, c.valid, c.num, rm, opt=c.opt)
    with pytest.raises(ValueError, match="joint_weight without"):
        smpl_sup.smpl_targets(pose, shape, c.valid, c.num, rm, joint_weight=c.joints_w, opt=c.opt)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        smpl_sup.smpl_targets(pose, shape, c.valid, c.num, rm.cpu(), opt=c.opt)


# ---- the loss: raw calls -----------------------------------------------------------------------------------------------------------------------
# name -> (B, max_objs, n): 16 x 16 maps.  n = 35 of 40: 70 slots = 17 full workgroups of four waves and one with two
SHAPES = {"n4": (2, 4, 4), "n3": (2, 4, 3), "n35": (2, 40, 35)}


def case(name, **kw):
    key = (name, repr(sorted(kw.items())))
    if key not in _CASES:
        B, M, n = SHAPES[name]
        _CASES[key] = SR.Case(B, M, n, 16, 16, seed=40 + 7 * len(key[1]) + n, **kw)
    return _CASES[key]


def lab_dev(c):
    return {k: v.to(DEV) for k, v in c.lab.items()}


def dev_run(c, with_joints=True, want=(True, True, True), out=None, ind=None, pose=None, shape=None):
    """-> (stats [9], grad_pose_map, grad_shape_map, grad_joints) of the raw calls, upstream gradient c.go."""
    stats, a = smpl_sup.supervised_loss_forward((c.pose if pose is None else pose).to(DEV), (c.shape if shape is None else shape).to(DEV),
                                                (c.ind if ind is None else ind).to(DEV), c.joints.to(DEV) if with_joints else None, lab_dev(c), c.n)
    gp, gs, gj = smpl_sup.supervised_loss_backward(a, stats, c.go.to(DEV), want=want, out=out)
    torch.cuda.synchronize()
    return stats, gp, gs, gj


def pooled_e32():
    """The largest relative fp32 error of a loss scalar over the cases and the three terms (losses_ref.pooled_e32)."""
    r = [case(nm).refs() for nm in SHAPES]
    return LR.pooled_e32([float(v) for _, r32 in r for v in r32[0]], [float(v) for r64, _ in r for v in r64[0]])


GRADS = ("grad_pose_map", "grad_shape_map", "grad_joints")


def check_against_refs(name, c, got, with_joints=True):
    r64, r32 = c.refs(with_joints)
    st = got[0].cpu().double()
    ratios = {"loss": LR.check_scalars(name + " losses", [float(v) for v in st[0::3]], [float(v) for v in r64[0]], pooled_e32())}
    for t in range(3):                                            # stats = {loss, l, num} x 3
        assert abs(float(st[3 * t + 1]) - float(r64[1][t])) <= 1e-5 * float(r64[1][t]) + 1e-30
        assert abs(float(st[3 * t + 2]) - float(r64[2][t])) <= 1e-6 * float(r64[2][t])
    for nm, g, a, b in zip(GRADS, got[1:], r64[3:], r32[3:]):
        if a is None:
            assert g is None, nm
            continue
        ratios[nm] = LR.check_tensor("%s %s" % (name, nm), g, a, b)
    return ratios


@pytest.mark.parametrize("name", list(SHAPES))
def test_losses_and_gradients_by_the_rule(name):
    c = case(name)
    got = dev_run(c)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    check_against_refs(name, c, got)
    off = torch.ones(c.B, 256, dtype=torch.bool)                 # zero off the labelled pixels
    for b in range(c.B):
        off[b, c.ind[b, :c.n]] = False
    for g in got[1:3]:
        assert not bool(g.cpu().reshape(c.B, g.shape[1], 256).transpose(1, 2)[off].any())


def test_rest_pose_gradient_equals_its_closed_form():
    """theta_j = 0 exactly: R = I and dR / dtheta_c = (sin a / a) G_c with a = sqrt(3) 1e-8, so g_c = -2 coef wp sum_ab R_lab[a][b] G_c[a][b]
    with G_c the skew generator of axis c -- independent of the restatement.  1e-6 max |g|: one fp32 rounding with 16 ulps of room."""
    c = case("n4")
    stats, gp, _, _ = dev_run(c)
    num = float(c.refs()[0][2][0])
    coef = float(c.go[0]) / (num + 1e-4)
    gens = np.zeros((3, 3, 3))
    gens[0, 1, 2], gens[0, 2, 1] = -1.0, 1.0
    gens[1, 0, 2], gens[1, 2, 0] = 1.0, -1.0
    gens[2, 0, 1], gens[2, 1, 0] = -1.0, 1.0
    want, have = [], []
    for b in range(c.B):
        pix = int(c.ind[b, 0])
        for j in (0, 3):
            assert not c.pose.view(c.B, 24, 3, 256)[b, j, :, pix].any()
            wp, Rl = float(c.lab["smpl_pose_w"][b, 0, j]), c.lab["smpl_rotmat"][b, 0, j].double().numpy().reshape(3, 3)
            assert wp > 0
            want += [-2.0 * coef * wp * float((Rl * gens[k]).sum()) for k in range(3)]
            have += [float(gp.view(c.B, 24, 3, 256)[b, j, k, pix]) for k in range(3)]
    want, have = np.array(want), np.array(have)
    print("rest pose: max |g| %.3g, max err %.3g" % (np.abs(want).max(), np.abs(have - want).max()))
    assert np.abs(want).max() > 0 and np.abs(have - want).max() <= 1e-6 * np.abs(want).max()


def test_autograd_path_has_the_raw_calls_bits():
    c = case("n35")                                               # every slot on a pixel of its own: nothing depends on the order of the atomics
    assert all(len(set(c.ind[b, :c.n].tolist())) == c.n for b in range(c.B))
    raw = dev_run(c)
    pm, sm, j = [t.to(DEV).requires_grad_(True) for t in (c.pose, c.shape, c.joints)]
    out = smpl_sup.smpl_supervised_loss(pm, sm, c.ind.to(DEV), j, lab_dev(c), c.n)
    assert len(out) == 3 and all(o.dim() == 0 for o in out) and all(torch.equal(o, raw[0][3 * t]) for t, o in enumerate(out))
    go = c.go.to(DEV)
    (out[0] * go[0] + out[1] * go[1] + out[2] * go[2]).backward()
    assert torch.equal(pm.grad, raw[1]) and torch.equal(sm.grad, raw[2]) and torch.equal(j.grad, raw[3])
    # n defaults to P / B with joints; only what is needed is computed; a loss that is not used gives its inputs no gradient
    sm2 = c.shape.to(DEV).requires_grad_(True)
    out = smpl_sup.smpl_supervised_loss(c.pose.to(DEV), sm2, c.ind.to(DEV), c.joints.to(DEV), lab_dev(c))
    (out[1] * go[1]).backward()
    assert torch.equal(sm2.grad, raw[2])
    pm3, j3 = c.pose.to(DEV).requires_grad_(True), c.joints.to(DEV).requires_grad_(True)
    out = smpl_sup.smpl_supervised_loss(pm3, c.shape.to(DEV), c.ind.to(DEV), j3, lab_dev(c), c.n)
    (out[2] * go[2]).backward()
    assert torch.equal(j3.grad, raw[3]) and not pm3.grad.any()


def test_joints_none_gives_no_joint_term_and_no_grad_joints():
    c = case("n4")
    full, none = dev_run(c), dev_run(c, with_joints=False)
    assert none[3] is None and not none[0][6:9].any() and torch.equal(none[0][:6], full[0][:6])
    assert torch.equal(none[1], full[1]) and torch.equal(none[2], full[2])
    check_against_refs("joints=None", c, none, with_joints=False)
    pm = c.pose.to(DEV).requires_grad_(True)
    out = smpl_sup.smpl_supervised_loss(pm, c.shape.to(DEV), c.ind.to(DEV), None, lab_dev(c), c.n)
    (out[0] * c.go[0].to(DEV) + out[2]).backward()
    assert float(out[2].detach()) == 0.0 and torch.equal(pm.grad, full[1])


def test_every_subset_of_the_wanted_gradients_gives_the_bits_of_the_full_call():
    c = case("n35")
    full = dev_run(c)
    for mask in range(8):
        want = tuple(bool(mask >> k & 1) for k in range(3))
        got = dev_run(c, want=want)
        for k in range(3):
            assert (got[1 + k] is None) if not want[k] else torch.equal(got[1 + k], full[1 + k]), (want, k)


def test_two_calls_and_a_second_stream_give_the_same_bits():
    c = case("n35")
    first, again = dev_run(c), dev_run(c)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        other = dev_run(c)
    st.synchronize()
    for run in (again, other):
        assert all(torch.equal(a, b) for a, b in zip(first, run))


def test_zero_weights_give_exactly_zero_whatever_the_labels():
    c = case("n4", weights="none")
    assert all(bool(torch.isnan(c.lab[k]).all()) for k in ("smpl_rotmat", "smpl_shape", "smpl_joints"))
    got = dev_run(c)
    assert not got[0].any() and all(not g.any() for g in got[1:])


def test_nan_labels_behind_zero_weights_and_behind_n():
    c = case("n3", nan_behind=True)
    c.ind[:, c.n:] = 1 << 40                                     # the rows behind n: an index far outside the map, NaN labels and weights
    assert bool(torch.isnan(c.lab["smpl_rotmat"][:, :c.n]).any()) and bool(torch.isnan(c.lab["smpl_joints_w"][:, c.n:]).all())
    got = dev_run(c)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    check_against_refs("nan behind", c, got)


def test_ind_outside_the_map_equals_its_zero_weight_twin():
    c = case("n4", bad_ind={(0, 1): 256, (1, 2): -1})
    got = dev_run(c)
    check_against_refs("ind outside", c, got)
    for p in (1, 4 + 2):
        assert not got[3][p].any()
    twin = copy.copy(c)                                           # the same two slots on the map with all their weights 0: the same bits
    twin.ind, twin.lab = c.ind.clone(), {k: v.clone() for k, v in c.lab.items()}
    twin.ind[0, 1], twin.ind[1, 2] = 3, 5
    assert 3 not in c.ind[0].tolist() and 5 not in c.ind[1].tolist()
    for k in ("smpl_pose_w", "smpl_shape_w", "smpl_joints_w"):
        twin.lab[k][0, 1] = 0
        twin.lab[k][1, 2] = 0
    other = dev_run(twin)
    assert all(torch.equal(a, b) for a, b in zip(got, other))


def test_two_slots_on_one_pixel_add_up():
    B, M, n = SHAPES["n4"]
    c = SR.Case(B, M, n, 16, 16, seed=500)
    pix = int(c.ind[1, 0])
    c.ind[1, 1] = pix
    shared = dev_run(c)
    check_against_refs("shared pixel", c, shared)
    # the two single runs: slot 1 moved to a free pixel that holds a copy of the shared pixel's values -- the same losses, the two
    # contributions on pixels of their own
    free = next(q for q in range(256) if q not in c.ind[1].tolist())
    maps = [t.clone() for t in (c.pose, c.shape)]
    for t in maps:
        t.view(B, t.shape[1], 256)[1, :, free] = t.view(B, t.shape[1], 256)[1, :, pix]
    ind = c.ind.clone()
    ind[1, 1] = free
    apart = dev_run(c, ind=ind, pose=maps[0], shape=maps[1])
    assert torch.equal(apart[0], shared[0]) and torch.equal(apart[3], shared[3])
    r64, r32 = c.refs()
    for nm, s, a, g64, g32 in zip(GRADS[:2], shared[1:3], apart[1:3], r64[3:5], r32[3:5]):
        s, a = s.cpu().double().reshape(B, -1, 256), a.cpu().double().reshape(B, -1, 256)
        want = a.clone()
        want[1, :, pix] = a[1, :, pix] + a[1, :, free]
        want[1, :, free] = 0.0
        e32 = float((g32.double() - g64).abs().max())
        err, limit = float((s - want).abs().max()), SR.FACTOR * e32 + 1e-7 * float(g64.abs().max())
        print("shared pixel against the sum of the two single runs, %s: err %.3g limit %.3g" % (nm, err, limit))
        assert err <= limit, (nm, err, limit)


def test_gradients_into_misaligned_buffers_with_sentinels():
    c = case("n35")
    PAD = 9
    sizes = {"gp": tuple(c.pose.shape), "gs": tuple(c.shape.shape), "gj": (c.B * c.n, 24, 3)}
    bufs = {k: torch.full((int(np.prod(s)) + 2 * PAD,), SENT, device=DEV) for k, s in sizes.items()}
    views = {k: bufs[k][PAD:PAD + int(np.prod(s))].view(s) for k, s in sizes.items()}
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views.values())
    got = dev_run(c, out=(views["gp"], views["gs"], views["gj"]))
    full = dev_run(c)
    assert all(torch.equal(a, b) for a, b in zip(got, full))
    for k, s in sizes.items():
        n = int(np.prod(s))
        assert bool((bufs[k][:PAD] == SENT).all()) and bool((bufs[k][PAD + n:] == SENT).all()) and not bool((views[k] == SENT).any()), k


def test_refusals_on_the_device():
    c = case("n4")
    pm, sm, ind, j, lab = c.pose.to(DEV), c.shape.to(DEV), c.ind.to(DEV), c.joints.to(DEV), lab_dev(c)
    f = smpl_sup.smpl_supervised_loss
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        f(c.pose, sm, ind, j, lab, c.n)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        f(pm, sm, ind, j, dict(lab, smpl_shape=c.lab["smpl_shape"]), c.n)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        f(pm.double(), sm, ind, j, lab, c.n)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        f(pm.permute(0, 1, 3, 2), sm, ind, j, lab, c.n)
    with pytest.raises(RuntimeError, match=r"\[B,72,H,W\]"):
        f(pm[:, :71].contiguous(), sm, ind, j, lab, c.n)
    with pytest.raises(RuntimeError, match=r"\[B,max_objs\]"):
        f(pm, sm, ind[:1], j, lab, c.n)
    with pytest.raises(RuntimeError, match="person slots"):
        f(pm, sm, ind, j, lab, c.n + 1)
    with pytest.raises(RuntimeError, match=r"\[B n,24,3\]"):
        f(pm, sm, ind, j[:-1].contiguous(), lab, c.n)
    with pytest.raises(RuntimeError, match="smpl_rotmat"):
        f(pm, sm, ind, j, dict(lab, smpl_rotmat=lab["smpl_rotmat"][:, :3].contiguous()), c.n)
    with pytest.raises(KeyError):
        f(pm, sm, ind, j, {k: v for k, v in lab.items() if k != "smpl_joints_w"}, c.n)


# ---- through lbs_from_heads on the jointed body -------------------------------------------------------------------------------------------------
_MAPS = {}


def maps_refs(name):
    if name not in _MAPS:
        c = case(name)
        _MAPS[name] = tuple(SR.maps_value_and_grads(c, body().numpy_dict(), dt) for dt in (torch.float64, torch.float32))
    return _MAPS[name]


@pytest.mark.parametrize("name", ["n4", "n35"])
def test_gradients_at_the_maps_through_lbs_from_heads_by_the_rule(name):
    c = case(name)
    pm, sm = c.pose.to(DEV).requires_grad_(True), c.shape.to(DEV).requires_grad_(True)
    ind = c.ind.to(DEV)
    _, joints = smpl.lbs_from_heads(body(), pm, sm, ind, c.n, return_joints=True, exact=True)
    out = smpl_sup.smpl_supervised_loss(pm, sm, ind, joints, lab_dev(c), c.n)
    go = c.go.to(DEV)
    (out[0] * go[0] + out[1] * go[1] + out[2] * go[2]).backward()
    torch.cuda.synchronize()
    r64, r32 = maps_refs(name)
    both = [maps_refs(nm) for nm in ("n4", "n35")]
    e32 = LR.pooled_e32([float(v) for _, b in both for v in b[0]], [float(v) for a, _ in both for v in a[0]])
    LR.check_scalars(name + " maps losses", [float(o.detach()) for o in out], [float(v) for v in r64[0]], e32)
    LR.check_tensor(name + " maps grad_pose_map", pm.grad, r64[1], r32[1])
    LR.check_tensor(name + " maps grad_shape_map", sm.grad, r64[2], r32[2])
    # the module: the same call through SmplSupervisedLoss, and without the joint term no SMPL stage runs
    mod = smpl_sup.SmplSupervisedLoss(body(), n=c.n)
    batch = dict(lab_dev(c), ind=ind)
    again = mod({"pose": pm.detach(), "shape": sm.detach()}, batch)
    assert all(torch.equal(a, b.detach()) for a, b in zip(again, out))
    two = smpl_sup.SmplSupervisedLoss(None, n=c.n, use_joints=False)({"pose": pm.detach(), "shape": sm.detach()}, batch)
    assert torch.equal(two[0], out[0].detach()) and torch.equal(two[1], out[1].detach()) and float(two[2]) == 0.0


# ---- multi_pose_train_batch(..., smpl_labels=) -------------------------------------------------------------------------------------------------
def test_train_batch_carries_the_labels_of_smpl_targets_and_leaves_every_other_key():
    rs = np.random.RandomState(3)
    imgs = torch.from_numpy(rs.randint(0, 256, (2, 64, 64, 3)).astype(np.uint8)).to(DEV)
    scenes = [targets_ref.scene(30 + b, 2, M=3, img_w=64, img_h=64, min_size=20.0, max_size=40.0) for b in range(2)]
    boxes, kps = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    opt = NS(input_res=64, output_res=16, max_objs=4, no_color_aug=True)
    params = {"c": np.array([[32.0, 30.0], [31.0, 33.0]], np.float32), "s": np.array([64.0, 72.0]), "rot": np.array([0.0, 17.0]),
              "flipped": np.array([False, True])}
    lab = {"pose": (rs.randn(2, 3, 72) * 0.5).astype(np.float32), "shape": rs.randn(2, 3, 10).astype(np.float32),
           "valid": np.array([[1, 1, 0], [1, 0, 1]], np.float32), "joints": rs.randn(2, 3, 24, 3).astype(np.float32),
           "pose_weight": (0.5 + rs.rand(2, 3, 24)).astype(np.float32)}
    num = [2, 2]
    plain = train_input.multi_pose_train_batch(imgs, boxes, kps, num, opt, params=params)
    both = train_input.multi_pose_train_batch(imgs, boxes, kps, num, opt, params=params, smpl_labels=lab)
    assert set(both) == set(plain) | set(SR.NAMES) and int(plain["reg_mask"].sum()) > 0
    for k, v in plain.items():
        if k == "meta":
            assert all(torch.equal(v[m], both[k][m]) for m in v)
        else:
            assert torch.equal(v, both[k]), k
    hand = smpl_sup.smpl_targets(lab["pose"], lab["shape"], lab["valid"], num, plain["reg_mask"], rot=params["rot"], flipped=params["flipped"],
                                 c=params["c"], s=params["s"], joints=lab["joints"], pose_weight=lab["pose_weight"], opt=opt)
    assert all(torch.equal(hand[k], both[k]) for k in SR.NAMES)
    want = SR.labels_np(lab["pose"], lab["shape"], lab["joints"], lab["valid"], lab["pose_weight"], None, num, plain["reg_mask"].cpu().numpy(),
                        params["flipped"], smpl_sup.rot2_from_params(params["c"], params["s"], params["rot"], 16, 16), 4)
    check_labels("train batch", both, want)
    assert float(both["smpl_pose_w"].sum()) > 0


# ---- the trainer, end to end -------------------------------------------------------------------------------------------------------------------
HEADS9 = dict(O.HEADS, pose=72, shape=10, cam=3)
HC = O.HC
WEIGHTS = dict(smpl_pose_weight=1.0, smpl_shape_weight=1.0, smpl_j3d_weight=1.0)


def make_net9():
    net = model.dla_net(HEADS9, head_conv=HC, dtype="f32")
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS9, True, HC), seed=0)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.to(DEV)


def new_trainer(lr, start, on=True):
    o = O.train_opt(lr)
    for k, v in WEIGHTS.items():
        setattr(o, k, v if on else 0.0)
    tr = trainer.HeadsTrainer(o, make_net9(), smpl_model=body())
    if start is not None:
        with torch.no_grad():
            for h, ps in tr.heads.head_params().items():
                for p, v in zip(ps, start[h]):
                    p.copy_(v.to(DEV))
    return tr


@pytest.fixture(scope="module")
def setting3d():
    """(batch, start head parameters, lr, fp64 series, fp32 series): series = [(loss, pose, shape, j3d)] before each of 6 steps."""
    sizes = [(64, 64), (64, 64)]
    rs = np.random.RandomState(13)
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    scenes = [targets_ref.scene(20 + b, 1, M=2, img_w=w, img_h=h, min_size=24.0, max_size=40.0) for b, (h, w) in enumerate(sizes)]
    boxes, kps = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    lab = {"pose": (rs.randn(2, 2, 72) * 0.3).astype(np.float32), "shape": rs.randn(2, 2, 10).astype(np.float32),
           "valid": np.ones((2, 2), np.float32), "smpl_model": body()}
    np.random.seed(17), random.seed(17)
    batch = train_input.multi_pose_train_batch([torch.from_numpy(i).to(DEV) for i in imgs], boxes, kps, [1, 1], O.train_opt(1e-3),
                                               data_rng=np.random.RandomState(123), smpl_labels=lab)
    n = batch["ind"].shape[1]
    assert int(batch["reg_mask"].sum()) > 0 and float(batch["smpl_pose_w"].sum()) > 0 and float(batch["smpl_joints_w"].sum()) > 0
    tr = new_trainer(1e-3, None)
    feat64 = tr.heads.features(batch["input"]).cpu().double().contiguous()
    start = {}
    for i, (h, c) in enumerate(HEADS9.items()):
        w1, b1, w2, b2 = O.draw_head(1000 * (i + 1), c, feat64)
        if h.startswith("hm"):
            b2 = torch.full((c,), -2.19)
        start[h] = [w1, b1, w2, b2]
    gold = {k: v.cpu() for k, v in batch.items() if torch.is_tensor(v)}
    bd = body().numpy_dict()

    def series(lr, dtype, steps=6):
        ps = {h: [t.to(dtype).clone().requires_grad_(True) for t in v] for h, v in start.items()}
        opt = torch.optim.Adam([t for v in ps.values() for t in v], foreach=False, **dict(optim_ref.DEFAULTS, lr=lr))
        feat, g, mt = feat64.to(dtype), LR.cast(gold, dtype), G.model_tensors(bd, dtype)
        vals = []
        for _ in range(steps):
            opt.zero_grad()
            o = {h: HR.forward(feat, v[0], v[1], v[2].reshape(v[2].shape[0], -1), v[3]) for h, v in ps.items()}
            three = SR.maps_loss(o["pose"], o["shape"], gold["ind"], gold, n, mt, dtype)[0]
            loss = LR.multi_pose(o, g)[0] + three.sum()
            vals.append((float(loss.detach()),) + tuple(float(v) for v in three.detach()))
            loss.backward()
            opt.step()
        return vals

    for lr in O.LRS:                          # the smallest of the list that lowers the restatement's smpl_pose_loss by >= 10 % in 5 steps
        s64 = series(lr, torch.float64)
        if np.isfinite(s64).all() and s64[5][1] <= 0.9 * s64[0][1]:
            return batch, start, lr, s64, series(lr, torch.float32)
    raise AssertionError("no learning rate of %s lowers the restatement's smpl_pose_loss by 10 %%: %s" % (O.LRS, s64))


def head_bits(tr):
    return {h: [p.detach().clone() for p in ps] for h, ps in tr.heads.head_params().items()}


KEYS4 = ("loss",) + smpl_sup.LOSS_KEYS


def test_five_train_steps_follow_the_restatement_and_a_resumed_run_has_the_sixth_steps_bits(setting3d, tmp_path):
    batch, start, lr, s64, s32 = setting3d
    tr = new_trainer(lr, start)
    assert isinstance(tr.loss, smpl_sup.loss_multi_pose_smpl3d) and len(list(tr.heads.parameters())) == 4 * len(HEADS9)
    vals = []
    for _ in range(5):
        out, loss, stats = tr.train_step(dict(batch))
        vals.append(tuple(float(stats[k].detach()) for k in KEYS4))
        assert set(stats) == set(tr.loss_stats) == set(smpl_sup.loss_multi_pose_smpl3d.KEYS) and set(out) == set(HEADS9)
        assert float(loss.detach()) == vals[-1][0]
    path = str(tmp_path / "model_last.pth")
    tr.save_model(path, 5)
    print("Adam lr %g, the three weights 1" % lr)
    for i, nm in enumerate(KEYS4):
        print("%s: f64 %s\n  f32 %s\n  gpu %s" % (nm, [v[i] for v in s64[:5]], [v[i] for v in s32[:5]], [v[i] for v in vals]))
    assert np.isfinite(vals).all()
    for i, nm in enumerate(KEYS4):
        LR.check_tensor("five steps " + nm, torch.tensor([v[i] for v in vals], dtype=torch.float64),
                        torch.tensor([v[i] for v in s64[:5]], dtype=torch.float64), torch.tensor([v[i] for v in s32[:5]], dtype=torch.float64))
    # the uninterrupted run's sixth step, and a fresh trainer resumed from the checkpoint
    tr.train_step(dict(batch))
    sixth = head_bits(tr)
    other = new_trainer(lr, None)
    assert other.load_model(path, resume=True) == 5
    for g in other.optimizer.param_groups:
        g["lr"] = lr                                              # the uninterrupted run never dropped it
    other.train_step(dict(batch))
    torch.cuda.synchronize()
    for h, ps in head_bits(other).items():
        assert all(torch.equal(a, b) for a, b in zip(ps, sixth[h])), h


def test_one_step_moves_pose_and_shape_and_leaves_the_other_heads_their_own_update(setting3d):
    batch, start, lr, _, _ = setting3d
    on, off = new_trainer(lr, start), new_trainer(lr, start, on=False)
    assert type(off.loss).__name__ == "loss_multi_pose"
    first = head_bits(on)
    on.train_step(dict(batch))
    off.train_step(dict(batch))
    torch.cuda.synchronize()
    a, b = head_bits(on), head_bits(off)
    for h in HEADS9:
        if h in ("pose", "shape"):
            assert all(not torch.equal(x, y) for x, y in zip(a[h], first[h])), h         # all four tensors of the head moved
            assert all(torch.equal(x, y) for x, y in zip(b[h], first[h])), h             # ... and only under the new terms
        elif h == "cam":                                                                 # no term reads the camera
            assert all(torch.equal(x, y) for x, y in zip(a[h], first[h])), h
        else:                                                                            # no path from the new terms to these heads
            assert all(torch.equal(x, y) for x, y in zip(a[h], b[h])), h
            assert all(not torch.equal(x, y) for x, y in zip(a[h], first[h])), h
