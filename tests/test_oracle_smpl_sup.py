"""CPU: the yardstick of the SMPL 3D supervision (tests/smpl_sup_ref.py) is differentiable and has the properties and closed forms the
definition implies (include/h3d.h section 4e), the in-plane rotation read from trans_output_rot is the closed form,
and the C ABI returns what its contract says on malformed calls -- every check runs before the first HIP call, no GPU needed."""
import ctypes
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import smpl_sup_ref as SR

import h3d_amd  # noqa: F401
from h3d_amd import _lib, losses, model, smpl, smpl_loss, smpl_sup, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 100


def small_case(**kw):
    return SR.Case(B=2, M=3, n=2, H=4, W=4, seed=1, **kw)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def test_gradcheck_of_the_restatement_in_float64():
    c = small_case()
    p, s, j = [t.double().clone().requires_grad_(True) for t in (c.pose, c.shape, c.joints)]
    fn = lambda p, s, j: SR.sup_loss(p, s, c.ind, j, c.lab, c.n)[0]
    assert torch.autograd.gradcheck(fn, (p, s, j), eps=1e-6, atol=1e-6, rtol=1e-5)
    fn2 = lambda p, s: SR.sup_loss(p, s, c.ind, None, c.lab, c.n)[0][:2]             # without joints: two terms
    assert torch.autograd.gradcheck(fn2, (p, s), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert float(SR.sup_loss(p, s, c.ind, None, c.lab, c.n)[0][2].detach()) == 0.0


# ---- the in-plane rotation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [-30, -1, 0, 17, 90])
def test_rot2_from_trans_output_rot_is_the_closed_form(rot):
    """A2 = [[cos r, sin r], [-sin r, cos r]], r = rot pi / 180.  get_affine_transform holds its three source points in float32 (2^-24
    relative each) and solves in float64, so the normalised linear part carries a few float32 roundings: 4 * 2^-23 absolute."""
    for c, s in (([31.5, 20.25], 57.0), ([320.0, 240.0], 614.4)):
        A = smpl_sup.rot2_from_params([c], [s], [rot], 128, 128)
        want = SR.closed_form_rot2(rot)
        if rot == 0:
            assert A is None                                 # nobody is rotated: the kernel takes the identity
            continue
        assert A.shape == (1, 2, 2) and A.dtype == np.float64
        assert np.abs(A[0] - want).max() <= 4 * 2.0 ** -23, (rot, A[0], want)
        assert abs(np.linalg.det(A[0]) - 1.0) <= 1e-15
    two = smpl_sup.rot2_from_params([[31.5, 20.25], [40.0, 30.0]], [57.0, 80.0], [0.0, rot])
    if rot != 0:
        assert np.array_equal(two[0], np.eye(2))             # the image that is not rotated: exactly the identity


def test_per_axis_scale_with_a_rotation_is_refused():
    s2 = np.array([[64.0, 48.0]])
    with pytest.raises(ValueError, match="per-axis"):
        smpl_sup.rot2_from_params([[10.0, 10.0]], s2, [5.0])
    assert smpl_sup.rot2_from_params([[10.0, 10.0]], s2, [0.0]) is None
    assert smpl_sup.rot2_from_params([[10.0, 10.0]], s2, None) is None
    with pytest.raises(ValueError, match="c and s"):
        smpl_sup.rot2_from_params(None, None, [5.0])


# ---- properties of the transform -----------------------------------------------------------------------------------------------------------
def _annotation(seed=0):
    rs = np.random.RandomState(seed)
    return SR.rodrigues_np(rs.randn(24, 3) * 0.7), rs.randn(24, 3), rs.rand(2, 24)


def test_pi_is_an_involution_and_matches_the_module():
    assert [SR.PI[SR.PI[j]] for j in range(24)] == list(range(24)) and sorted(SR.PI) == list(range(24))
    assert SR.PI == smpl_sup.MIRROR and tuple(SR.PAIRS) == tuple(smpl_sup.MIRROR_PAIRS)
    assert sum(SR.PI[j] != j for j in range(24)) == 18


def test_flipping_twice_restores_the_bits():
    R, J, w = _annotation()
    R2, J2, w2 = SR.transform_one(*SR.transform_one(R, J, w, True, None), True, None)
    assert np.array_equal(R2, R) and np.array_equal(J2, J) and np.array_equal(w2, w)
    R1, J1, w1 = SR.transform_one(R, J, w, True, None)
    assert not np.array_equal(R1, R) and np.array_equal(w1[:, 1], w[:, 2]) and np.array_equal(J1[2], J[1] * [-1, 1, 1])
    assert np.abs(np.linalg.det(R1) - np.linalg.det(R)[SR.PI]).max() <= 1e-14          # S R S keeps the determinant (1 up to the convention's 1e-8)


@pytest.mark.parametrize("rot", [-30.0, 17.0, 90.0])
def test_rotation_and_its_inverse_restore(rot):
    R, J, w = _annotation(1)
    fw = SR.transform_one(R, J, w, False, SR.closed_form_rot2(rot))
    back = SR.transform_one(*fw, False, SR.closed_form_rot2(-rot))
    assert np.abs(back[0] - R).max() <= 1e-14 and np.abs(back[1] - J).max() <= 1e-14 and np.array_equal(back[2], w)
    assert np.array_equal(fw[0][1:], R[1:]) and not np.array_equal(fw[0][0], R[0])          # only the root's rotation turns
    assert np.array_equal(fw[1][:, 2], J[:, 2])


@pytest.mark.parametrize("rot", [-30.0, -1.0, 17.0, 90.0])
def test_orientation_about_z_stays_about_z_with_its_angle_shifted(rot):
    """A2 = [[cos r, sin r], [-sin r, cos r]] turns by -r about z (x towards -y for r > 0): phi -> phi - r."""
    phi = 0.4
    pose = np.zeros((24, 3))
    pose[0, 2] = phi
    R, _, _ = SR.transform_one(SR.rodrigues_np(pose), None, np.ones((1, 24)), False, SR.closed_form_rot2(rot))
    a = phi - rot * np.pi / 180
    want = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    assert np.abs(R[0] - want).max() <= 1e-7                 # (the +1e-8 of the convention tilts the label's axis by 1e-8 / phi)
    assert np.abs(R[0][2] - [0, 0, 1]).max() <= 1e-7 and np.abs(R[0][:, 2] - [0, 0, 1]).max() <= 1e-7


def test_labels_np_gates_and_zero_rows():
    rs = np.random.RandomState(3)
    B, M, N = 2, 4, 3
    pose, shape, joints = rs.randn(B, M, 72), rs.randn(B, M, 10), rs.randn(B, M, 24, 3)
    valid = np.array([[1.0, 0.0, 2.0, 1.0], [1.0, 1.0, 1.0, 1.0]])
    pose[0, 1] = np.nan
    reg_mask = np.array([[1, 1, 1], [1, 0, 1]], np.uint8)
    o = SR.labels_np(pose, shape, joints, valid, None, None, [4, 2], reg_mask, [1, 0], None, N)
    assert o["smpl_shape_w"].tolist() == [[1.0, 0.0, 2.0], [1.0, 0.0, 0.0]]
    assert all(np.isfinite(v).all() for v in o.values())
    assert not o["smpl_rotmat"][0, 1].any() and not o["smpl_rotmat"][1, 1:].any() and o["smpl_pose_w"][0, 2].tolist() == [2.0] * 24
    assert np.array_equal(o["smpl_shape"][0, 2], shape[0, 2])
    assert np.array_equal(o["smpl_joints"][0, 0, 1], joints[0, 0, 2] * [-1, 1, 1])          # image 0 is mirrored
    assert np.array_equal(o["smpl_joints"][1, 0], joints[1, 0])


# ---- closed forms of the loss ----------------------------------------------------------------------------------------------------------------
def _own_labels(c):
    """Labels equal to the prediction's own R, beta and J."""
    idx = c.ind[:, :c.n]
    theta = SR.gather_rows(c.pose.double(), idx).reshape(c.B, c.n, 24, 3)
    lab = {k: v.double().clone() for k, v in c.lab.items()}
    lab["smpl_rotmat"][:, :c.n] = SR.G.rodrigues(theta, torch.float64).reshape(c.B, c.n, 24, 9)
    lab["smpl_shape"][:, :c.n] = SR.gather_rows(c.shape.double(), idx).reshape(c.B, c.n, 10)
    lab["smpl_joints"][:, :c.n] = c.joints.double().reshape(c.B, c.n, 24, 3)
    return lab


def _grads(c, lab, joints=None):
    p, s = [t.double().clone().requires_grad_(True) for t in (c.pose, c.shape)]
    j = (c.joints if joints is None else joints).double().clone().requires_grad_(True)
    loss, l, num = SR.sup_loss(p, s, c.ind, j, lab, c.n)
    return loss.detach(), l.detach(), num.detach(), torch.autograd.grad(loss.sum(), (p, s, j))


def test_labels_equal_to_the_prediction_give_zero_loss_and_zero_gradients():
    c = small_case()
    loss, l, num, gr = _grads(c, _own_labels(c))
    assert float(loss.abs().max()) == 0.0 and float(num.min()) > 0 and all(float(g.abs().max()) == 0.0 for g in gr)


def test_zero_weights_give_zero_loss_and_zero_gradients_whatever_the_labels():
    c = small_case(weights="none")
    assert all(bool(torch.isnan(c.lab[k]).all()) for k in ("smpl_rotmat", "smpl_shape", "smpl_joints"))
    loss, l, num, gr = _grads(c, c.lab)
    assert float(loss.abs().max()) == 0.0 and float(num.abs().max()) == 0.0 and all(float(g.abs().max()) == 0.0 for g in gr)


def test_a_translation_of_all_joints_changes_nothing():
    c = small_case()
    a = _grads(c, c.lab)
    shift = torch.tensor([0.5, -0.25, 2.0], dtype=torch.float64)
    b = _grads(c, c.lab, joints=c.joints.double() + shift)   # added in float64: the root moves with the joints
    assert float((a[0] - b[0]).abs().max()) <= 1e-13 * float(a[0].abs().max())
    assert float((a[3][2] - b[3][2]).abs().max()) <= 1e-13 * float(a[3][2].abs().max())
    assert float(a[3][2].reshape(c.B * c.n, 24, 3).sum(1).abs().max()) <= 1e-15                # the gradient of a translation is zero


def test_doubling_the_shape_residual_quadruples_l_shape():
    c = small_case()
    lab = {k: v.double().clone() for k, v in c.lab.items()}
    beta = SR.gather_rows(c.shape.double(), c.ind[:, :c.n]).reshape(c.B, c.n, 10)
    one = SR.sup_loss(c.pose, c.shape, c.ind, None, lab, c.n)[1][1]
    lab["smpl_shape"][:, :c.n] = beta - 2.0 * (beta - lab["smpl_shape"][:, :c.n])
    two = SR.sup_loss(c.pose, c.shape, c.ind, None, lab, c.n)[1][1]
    assert float(one) > 0 and abs(float(two) - 4.0 * float(one)) <= 1e-13 * float(two)


def test_slot_outside_the_map_equals_its_zero_weight_twin():
    c = small_case(bad_ind={(0, 1): 16, (1, 0): -1})
    base = _grads(c, c.lab)
    twin = small_case()
    for k in ("smpl_pose_w", "smpl_shape_w", "smpl_joints_w"):
        twin.lab[k][0, 1] = 0
        twin.lab[k][1, 0] = 0
    other = _grads(twin, twin.lab)
    assert torch.equal(base[0], other[0]) and all(torch.equal(a, b) for a, b in zip(base[3], other[3]))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
OK, SHAPE, ARG = 0, -1, -5
NEW = ("h3d_smpl_sup_labels", "h3d_smpl_sup_loss_workspace_bytes", "h3d_smpl_sup_loss_forward", "h3d_smpl_sup_loss_backward")
X = 0x1000          # stands for a device pointer that is never dereferenced: every call here returns before the first launch


def test_the_four_symbols_are_exported_declared_and_bound_as_declared():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "h3d.h")).read()
    hdr = re.sub(r"//[^\n]*|/\*.*?\*/", "", hdr, flags=re.S)
    for nm in NEW:
        assert nm in _lib.SIGNATURES and getattr(L, nm) is not None
        m = re.search(r"^int %s\s*\(([^)]*)\)\s*;" % nm, hdr, flags=re.M)
        assert m, nm
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        args = _lib.SIGNATURES[nm]
        assert len(params) == len(args), (nm, len(params), len(args))
        for p, a in zip(params, args):
            if re.match(r"(const )?size_t \*", p):
                assert a == ctypes.POINTER(ctypes.c_size_t), (nm, p)
            elif "*" in p:
                assert a is ctypes.c_void_p, (nm, p)
            else:
                assert a is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[p.rsplit(" ", 1)[0]], (nm, p)
    assert L.h3d_abi_version() == 4


def test_workspace_query():
    L = _lib.lib()
    n = ctypes.c_size_t(7)
    assert L.h3d_smpl_sup_loss_workspace_bytes(2, 4, None) == ARG
    assert L.h3d_smpl_sup_loss_workspace_bytes(2, 4, ctypes.byref(n)) == OK and n.value == 256          # 2 workgroups x 24 bytes
    assert L.h3d_smpl_sup_loss_workspace_bytes(8, 32, ctypes.byref(n)) == OK and n.value == 24 * 64
    assert L.h3d_smpl_sup_loss_workspace_bytes(2, 35, ctypes.byref(n)) == OK and n.value == 512         # 18 workgroups: 432 bytes
    assert L.h3d_smpl_sup_loss_workspace_bytes(0, 4, ctypes.byref(n)) == SHAPE
    assert L.h3d_smpl_sup_loss_workspace_bytes(2, 0, ctypes.byref(n)) == SHAPE
    assert L.h3d_smpl_sup_loss_workspace_bytes(1 << 16, 1 << 15, ctypes.byref(n)) == SHAPE


def _labels(L, pose=X, shape=X, joints=X, valid=X, pose_w=X, joints_w=X, num=X, reg_mask=X, flipped=X, rot2=X, B=2, M=5, N=4, o=(X,) * 6):
    return L.h3d_smpl_sup_labels(pose, shape, joints, valid, pose_w, joints_w, num, reg_mask, flipped, rot2, B, M, N, *o, None)


def test_return_codes_of_the_labels():
    L = _lib.lib()
    for kw in ({"pose": None}, {"shape": None}, {"valid": None}, {"num": None}, {"reg_mask": None}):
        assert _labels(L, **kw) == ARG and b"null pointer" in L.h3d_last_error(), kw
    for i in range(6):
        assert _labels(L, o=tuple(None if k == i else X for k in range(6))) == ARG and b"null pointer" in L.h3d_last_error(), i
    assert _labels(L, joints=None) == ARG and b"joints_w without joints_lab" in L.h3d_last_error()
    for kw in ({"pose": X + 2}, {"valid": X + 1}, {"flipped": X + 2}, {"o": (X, X + 2, X, X, X, X)}):
        assert _labels(L, **kw) == ARG and b"aligned" in L.h3d_last_error(), kw
    assert _labels(L, rot2=X + 4) == ARG and b"8-byte" in L.h3d_last_error()
    for kw in ({"B": 0}, {"M": 0}, {"N": 0}, {"B": -1}, {"B": 1 << 16, "N": 1 << 15}, {"B": 1 << 16, "M": 1 << 15}):
        assert _labels(L, **kw) == SHAPE, kw


def _fwd(L, pose=X, shape=X, ind=X, joints=X, lab=(X,) * 6, B=2, M=4, n=4, HW=256, stats=X, ws=X, ws_bytes=1 << 20):
    return L.h3d_smpl_sup_loss_forward(pose, shape, ind, joints, *lab, B, M, n, HW, stats, ws, ws_bytes, None)


def test_return_codes_of_the_forward():
    L = _lib.lib()
    for kw in ({"pose": None}, {"shape": None}, {"ind": None}, {"stats": None}):
        assert _fwd(L, **kw) == ARG and b"null pointer" in L.h3d_last_error(), kw
    for i in range(4):                                       # rotmat, pose_w, shape, shape_w: always needed
        assert _fwd(L, lab=tuple(None if k == i else X for k in range(6))) == ARG and b"null pointer" in L.h3d_last_error(), i
    for i in (4, 5):                                         # the joint labels: needed with joints only
        assert _fwd(L, lab=tuple(None if k == i else X for k in range(6))) == ARG and b"with joints" in L.h3d_last_error(), i
    assert _fwd(L, ws=None, ws_bytes=0) == ARG and b"workspace" in L.h3d_last_error()
    assert _fwd(L, ws_bytes=255) == ARG and b"workspace" in L.h3d_last_error()
    assert _fwd(L, ws=X + 4) == ARG and b"workspace" in L.h3d_last_error()
    assert _fwd(L, pose=X + 2) == ARG and b"aligned" in L.h3d_last_error()
    assert _fwd(L, ind=X + 4) == ARG and b"8-byte" in L.h3d_last_error()
    for kw in ({"B": 0}, {"B": -1}, {"M": 0}, {"n": 0}, {"HW": 0}, {"n": 5}, {"B": 1 << 16, "M": 1 << 15, "n": 1 << 15}):
        assert _fwd(L, **kw) == SHAPE, kw


def _bwd(L, pose=X, shape=X, ind=X, joints=X, lab=(X,) * 6, B=2, M=4, n=4, HW=256, stats=X, go=X, gp=X, gs=X, gj=X):
    return L.h3d_smpl_sup_loss_backward(pose, shape, ind, joints, *lab, B, M, n, HW, stats, go, gp, gs, gj, None)


def test_return_codes_of_the_backward():
    L = _lib.lib()
    assert _bwd(L, gp=None, gs=None, gj=None) == OK                                           # nothing requested: nothing is launched
    for kw in ({"pose": None}, {"shape": None}, {"ind": None}, {"stats": None}, {"go": None}):
        assert _bwd(L, **kw) == ARG and b"null pointer" in L.h3d_last_error(), kw
    for i in range(4):
        assert _bwd(L, lab=tuple(None if k == i else X for k in range(6))) == ARG and b"null pointer" in L.h3d_last_error(), i
    assert _bwd(L, joints=None) == ARG and b"grad_joints without joints" in L.h3d_last_error()
    assert _bwd(L, gp=X + 2) == ARG and b"aligned" in L.h3d_last_error()
    for kw in ({"B": 0}, {"M": -3}, {"n": 0}, {"HW": -1}, {"n": 5}):
        assert _bwd(L, **kw) == SHAPE, kw


# ---- Python --------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise_not_implemented_on_the_cpu():
    c = small_case()
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        smpl_sup.smpl_supervised_loss(c.pose, c.shape, c.ind, c.joints, c.lab, c.n)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        smpl_sup.smpl_targets(np.zeros((1, 2, 72)), np.zeros((1, 2, 10)), np.ones((1, 2)), [2], torch.ones(1, 32, dtype=torch.uint8))
    with pytest.raises(TypeError, match="reg_mask"):
        smpl_sup.smpl_targets(np.zeros((1, 2, 72)), np.zeros((1, 2, 10)), np.ones((1, 2)), [2], np.ones((1, 32), np.uint8))


HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}


def test_heads_trainer_without_the_new_weights_builds_todays_losses_and_the_new_loss_needs_its_heads():
    net = model.dla_net(HEADS, head_conv=64, dtype="f32")
    net9 = model.dla_net(dict(HEADS, pose=72, shape=10, cam=3), head_conv=64, dtype="f32")
    net8 = model.dla_net(dict(HEADS, pose=72, shape=10), head_conv=64, dtype="f32")
    body = smpl.SMPLModel.synthetic(num_verts=V)
    reg = smpl_loss.KeypointRegressor.synthetic(17, V, 2)
    zero = dict(smpl_pose_weight=0.0, smpl_shape_weight=0.0, smpl_j3d_weight=0)
    for extra in ({}, zero):
        tr = trainer.HeadsTrainer(NS(task="multi_pose", lr=1e-3, **extra), net)
        assert type(tr.loss) is losses.loss_multi_pose and tr.loss_stats == list(losses.loss_multi_pose.KEYS)
        tr = trainer.HeadsTrainer(NS(task="multi_pose", lr=1e-3, **extra), net, body, reg)
        assert type(tr.loss) is losses.loss_multi_pose and tr.loss_stats == list(losses.loss_multi_pose.KEYS)
        tr = trainer.HeadsTrainer(NS(task="multi_pose", lr=1e-3, smpl_kp_weight=0.5, **extra), net9, body, reg)
        assert type(tr.loss) is smpl_loss.loss_multi_pose_smpl and tr.loss_stats == list(losses.loss_multi_pose.KEYS) + ["smpl_kp_loss"]
        tr = trainer.HeadsTrainer(NS(task="ctdet", lr=1e-3, smpl_pose_weight=1.0), model.dla_net({"hm": 3, "wh": 2, "reg": 2}, head_conv=64, dtype="f32"), body)
        assert type(tr.loss) is losses.loss_obj_detection
    tr = trainer.HeadsTrainer(NS(task="multi_pose", lr=1e-3, smpl_pose_weight=1.0), net9)             # no smpl_model: as before
    assert type(tr.loss) is losses.loss_multi_pose
    with pytest.raises(ValueError, match="needs the heads"):
        trainer.HeadsTrainer(NS(task="multi_pose", lr=1e-3, smpl_shape_weight=1.0), net, body)
    with pytest.raises(ValueError, match="needs the heads"):                                          # the keypoint term on: cam as well
        trainer.HeadsTrainer(NS(task="multi_pose", lr=1e-3, smpl_shape_weight=1.0, smpl_kp_weight=1.0), net8, body, reg)
    base = list(losses.loss_multi_pose.KEYS)
    tr = trainer.HeadsTrainer(NS(task="multi_pose", lr=1e-3, smpl_shape_weight=0.5), net8, body)
    assert type(tr.loss) is smpl_sup.loss_multi_pose_smpl3d and tr.loss_stats == base + list(smpl_sup.LOSS_KEYS)
    assert tr.loss.weights == (0.0, 0.5, 0.0) and not tr.loss.smpl_sup.use_joints and tr.loss.smpl_kp is None
    tr = trainer.HeadsTrainer(NS(task="multi_pose", lr=1e-3, smpl_j3d_weight=1.0, smpl_kp_weight=0.5), net9, body, reg)
    assert type(tr.loss) is smpl_sup.loss_multi_pose_smpl3d and tr.loss_stats == base + list(smpl_sup.LOSS_KEYS) + ["smpl_kp_loss"]
    assert tr.loss.smpl_sup.use_joints and tr.loss.smpl_kp is not None and len(list(tr.heads.parameters())) == 36
    assert smpl_sup.loss_multi_pose_smpl3d.KEYS == tuple(base) + smpl_sup.LOSS_KEYS                    # the class attribute is not touched
    tr = trainer.NetworkTrainer(NS(task="multi_pose", lr=1e-3, smpl_pose_weight=1.0), net8, body)
    assert type(tr.loss) is smpl_sup.loss_multi_pose_smpl3d
