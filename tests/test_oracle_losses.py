"""CPU: the restatement everything in tests/test_gpu_losses.py is measured against (tests/losses_ref.py) is the reference's: in fp64 it
reproduces every value and gradient the reference's own `models.losses` classes returned in fp32 (tests/golden/losses_ref.npz, written by
tools/gen_losses_golden.py).  Plus the host-side contract of h3d_amd.losses that needs no GPU.

Tolerances (fixed): the golden numbers are fp32 results, so they carry the reference's own rounding.
  values     2e-5 relative.  A loss is a sum of up to 1088 terms accumulated in fp32 (2^-24 relative per add, far below the bound); the
             bound is set by the clamp: fp32 rounds 1 - 1e-4 to 0.99989998, 2^-25 absolute = 3e-4 relative in 1 - p, so log(1 - p) of an
             element at the upper clamp is off by 3e-4 / 9.2 = 3e-5 of itself, and such elements carry up to a third of these sums.
  gradients  1e-5 of the largest |gradient| of the tensor, per element: two or three fp32 roundings per element (6e-8 each) and the
             fp32 rounding of the 1/num_pos or 1/(den + 1e-4) they share (6e-8); elements at the clamp have gradient zero on both sides."""
import ctypes
import os

import numpy as np
import pytest
import torch

import losses_ref as R

import h3d_amd  # noqa: F401
from h3d_amd import _lib, losses

VALUE_RTOL, GRAD_RTOL = 2e-5, 1e-5


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "losses_ref.npz"))


def _names(g, suffix):
    return sorted(k[:-len(suffix)] for k in g.files if k.endswith(suffix))


def _close(name, got, ref, rtol):
    got, ref = got.detach().double().numpy(), np.asarray(ref, dtype=np.float64)
    err = float(np.abs(got - ref).max())
    lim = rtol * float(np.abs(ref).max())
    print("%s: err %.3g limit %.3g" % (name, err, lim))
    assert err <= lim, (name, err, lim)


def test_focal_restatement_reproduces_the_reference_values_and_gradients(golden):
    names = _names(golden, ".grad_x")
    assert len(names) == 3
    for nm in names:
        x, gt = torch.from_numpy(golden[nm + ".x"]), torch.from_numpy(golden[nm + ".gt"])
        v, g = R.value_and_grad(lambda h: R.focal_logits(h, gt.double()), x, torch.float64)
        _close(nm + " loss", v, golden[nm + ".loss"], VALUE_RTOL)
        _close(nm + " grad_x", g, golden[nm + ".grad_x"], GRAD_RTOL)
        _close(nm + " pred", R.sigmoid_clamp(x.double()), golden[nm + ".pred"], 1e-7)
        pred = torch.from_numpy(golden[nm + ".pred"])
        v, g = R.value_and_grad(lambda h: R.focal(h, gt.double()), pred, torch.float64)
        _close(nm + " loss_p", v, golden[nm + ".loss_p"], VALUE_RTOL)
        _close(nm + " grad_p", g, golden[nm + ".grad_p"], GRAD_RTOL)
    assert float(golden["focal_none.gt"].max()) > 1 and not (golden["focal_none.gt"] == 1).any()
    assert (golden["focal_all.gt"] == 1).all() and (golden["focal_some.gt"] == 1).any()


def test_regression_restatements_reproduce_the_reference_values_and_gradients(golden):
    names = _names(golden, ".feat")
    assert {n.rsplit("_", 1)[0] for n in names} == set(R.REG_CLASSES)
    for nm in names:
        cls = nm.rsplit("_", 1)[0]
        feat, mask, ind, target = [torch.from_numpy(golden[nm + k]) for k in (".feat", ".mask", ".ind", ".target")]
        v, g = R.value_and_grad(lambda h: R.reg(cls, h, mask, ind, target.double()), feat, torch.float64)
        _close(nm + " loss", v, golden[nm + ".loss"], VALUE_RTOL)
        _close(nm + " grad", g, golden[nm + ".grad"], GRAD_RTOL)
        assert float(np.abs(golden[nm + ".grad"]).max()) > 0


def test_golden_inputs_are_what_the_builders_build(golden):
    x, gt = R.focal_inputs(11, (2, 2, 8, 12), "some")
    assert np.array_equal(golden["focal_some.x"], x.numpy()) and np.array_equal(golden["focal_some.gt"], gt.numpy())
    feat, mask, ind, target = R.reg_inputs(21, "RegL1Loss", 3, 2, 32, 8, 12, torch.uint8)
    assert np.array_equal(golden["RegL1Loss_u8.ind"], ind.numpy()) and np.array_equal(golden["RegL1Loss_u8.mask"], mask.numpy())
    i = golden["RegL1Loss_u8.ind"]
    assert i.min() == 0 and i.max() == 95 and (i[:, 2] == i[:, 3]).all() and (golden["RegL1Loss_u8.mask"][:, 2:4] == 1).all()
    assert (i[:, 24:] == 0).all() and (golden["RegL1Loss_u8.mask"][:, 24:] == 0).all()


@pytest.mark.parametrize("task", ["multi_pose", "ctdet"])
@pytest.mark.parametrize("reg_loss", ["l1", "sl1"])
def test_task_restatement_is_the_weighted_sum_of_its_terms(task, reg_loss):
    if task == "multi_pose":
        output, batch = R.multi_pose_inputs(5, 2, 8, 12, M=8)
        loss, st = R.multi_pose(R.cast(output, torch.float64), R.cast(batch, torch.float64), reg_loss)
        crit = "RegL1Loss" if reg_loss == "l1" else "RegLoss"
        o, b = R.cast(output, torch.float64), R.cast(batch, torch.float64)
        want = (R.focal(R.sigmoid_clamp(o["hm"]), b["hm"]) + R.focal(R.sigmoid_clamp(o["hm_hp"]), b["hm_hp"])
                + R.reg("RegWeightedL1Loss", o["hps"], b["hps_mask"], b["ind"], b["hps"]) + 0.1 * R.reg(crit, o["wh"], b["reg_mask"], b["ind"], b["wh"])
                + R.reg(crit, o["reg"], b["reg_mask"], b["ind"], b["reg"]) + R.reg(crit, o["hp_offset"], b["hp_mask"], b["hp_ind"], b["hp_offset"]))
        assert set(st) == {"loss", "hm_loss", "hp_loss", "hm_hp_loss", "hp_offset_loss", "wh_loss", "off_loss"}       # trainer.py:134-136
    else:
        output, batch = R.ctdet_inputs(6, 2, 8, 12, M=8)
        loss, st = R.ctdet(R.cast(output, torch.float64), R.cast(batch, torch.float64), reg_loss)
        crit = "RegL1Loss" if reg_loss == "l1" else "RegLoss"
        o, b = R.cast(output, torch.float64), R.cast(batch, torch.float64)
        want = (R.focal(R.sigmoid_clamp(o["hm"]), b["hm"]) + 0.1 * R.reg(crit, o["wh"], b["reg_mask"], b["ind"], b["wh"])
                + R.reg(crit, o["reg"], b["reg_mask"], b["ind"], b["reg"]))
        assert set(st) == {"loss", "hm_loss", "wh_loss", "off_loss"}                                                   # trainer.py:71-72
    assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want)) and float(st["loss"]) == float(loss)
    if reg_loss == "sl1":
        l1 = (R.multi_pose if task == "multi_pose" else R.ctdet)(R.cast(output, torch.float64), R.cast(batch, torch.float64), "l1")[0]
        assert float(l1) != float(loss)


# ---- the host-side contract of h3d_amd.losses --------------------------------------------------------------------------------------
def test_cpu_tensors_and_other_dtypes_raise():
    x, gt = R.focal_inputs(1, (1, 1, 4, 4))
    feat, mask, ind, target = R.reg_inputs(2, "RegL1Loss", 1, 2, 2, 4, 4)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        losses.FocalLoss()(R.sigmoid_clamp(x), gt)
    for cls in (losses.RegL1Loss, losses.RegLoss, losses.NormRegL1Loss):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            cls()(feat, mask, ind, target)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        losses.RegWeightedL1Loss()(feat, mask[:, :, None].expand_as(target).float(), ind, target)
    out, batch = R.multi_pose_inputs(3, 1, 4, 4, M=2)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        losses.loss_multi_pose(object())([out], batch)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        losses.loss_obj_detection(object())([out], batch)
    with pytest.raises(ValueError, match="reg_loss"):
        losses.loss_multi_pose(type("O", (), {"reg_loss": "l2"})())


def test_non_fp32_pred_raises_like_the_other_mirrors():
    x, gt = R.focal_inputs(1, (1, 1, 4, 4))
    feat, mask, ind, target = R.reg_inputs(2, "RegL1Loss", 1, 2, 2, 4, 4)
    for bad in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match="expected float32 tensors"):
            losses.FocalLoss()(R.sigmoid_clamp(x).to(bad), gt)
        with pytest.raises(RuntimeError, match="expected float32 tensors"):
            losses.RegL1Loss()(feat.to(bad), mask, ind, target)


def test_term_struct_mirrors_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "h3d.h")).read()
    body = hdr[hdr.index("typedef struct h3d_loss_term {"):hdr.index("} h3d_loss_term;")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if decl:
            fields += [n.strip().lstrip("*") for n in decl.split(" ", 2 if decl.startswith("const") else 1)[-1].split(",")]
    assert fields == [n for n, _ in losses.H3dLossTerm._fields_]
    assert ctypes.sizeof(losses.H3dLossTerm) == 88
    for nm in ("FOCAL", "REG_L1", "REG_WEIGHTED_L1", "NORM_REG_L1", "REG_SL1", "MASK_U8", "MASK_F32"):
        assert re.search(r"H3D_LOSS_%s = %d\b" % (nm, getattr(losses, nm)), hdr), nm
    assert "#define H3D_LOSS_FROM_LOGITS %d" % losses.FROM_LOGITS in hdr and "#define H3D_LOSS_MAX_TERMS %d" % losses.MAX_TERMS in hdr
    assert "#define H3D_LOSS_TUNE_GRID8 0x%x" % losses.TUNE_GRID8 in hdr


def _term(**kw):
    t = losses.H3dLossTerm()
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_return_codes_of_the_argument_checks():
    """Everything here returns before the first launch: no GPU needed.  0x1000 stands for a device pointer that is never dereferenced."""
    L = _lib.lib()
    P = 0x1000
    n = ctypes.c_size_t(7)
    one = (losses.H3dLossTerm * 1)(_term(kind=losses.FOCAL, x=P, gt=P, n=100000))
    assert L.h3d_loss_forward(None, 1, P, P, 1 << 20, None) == -5                    # NULL terms: H3D_ERR_ARG
    assert L.h3d_loss_forward(one, 1, None, P, 1 << 20, None) == -5                   # NULL stats
    assert L.h3d_loss_workspace_bytes(one, 1, None) == -5
    assert L.h3d_loss_workspace_bytes(one, 1, ctypes.byref(n)) == 0 and n.value >= 16 * 98 and n.value % 256 == 0   # ceil(1e5 / 1024) workgroups
    assert L.h3d_loss_forward(one, 1, P, P, n.value - 256, None) == -5 and b"workspace" in L.h3d_last_error()
    assert L.h3d_loss_forward(one, 1, P, None, 0, None) == -5 and b"workspace" in L.h3d_last_error()
    nullx = (losses.H3dLossTerm * 1)(_term(kind=losses.FOCAL, x=None, gt=P, n=4))
    assert L.h3d_loss_forward(nullx, 1, P, P, 1 << 20, None) == -5
    neg = (losses.H3dLossTerm * 1)(_term(kind=losses.FOCAL, x=P, gt=P, n=-1))
    assert L.h3d_loss_forward(neg, 1, P, P, 1 << 20, None) == -1                      # H3D_ERR_SHAPE
    negr = (losses.H3dLossTerm * 1)(_term(kind=losses.REG_L1, x=P, gt=P, ind=P, mask=P, B=1, C=-2, HW=4, M=1))
    assert L.h3d_loss_forward(negr, 1, P, P, 1 << 20, None) == -1
    assert L.h3d_loss_backward(negr, 1, P, P, None) == -1
    assert L.h3d_loss_forward(one, -1, P, P, 1 << 20, None) == -1
    bad = (losses.H3dLossTerm * 1)(_term(kind=9, x=P, gt=P, n=4))
    assert L.h3d_loss_forward(bad, 1, P, P, 1 << 20, None) == -5
    many = (losses.H3dLossTerm * 17)(*[_term(kind=losses.FOCAL, x=P, gt=P, n=4) for _ in range(17)])
    assert L.h3d_loss_forward(many, 17, P, P, 1 << 20, None) == -4                    # H3D_ERR_UNSUPPORTED
    assert L.h3d_loss_backward(None, 1, P, P, None) == -5 and L.h3d_loss_backward(one, 1, None, P, None) == -5
    # an empty term needs no workspace and no pointers; the grid is a function of n alone
    empty = (losses.H3dLossTerm * 1)(_term(kind=losses.FOCAL, n=0))
    assert L.h3d_loss_workspace_bytes(empty, 1, ctypes.byref(n)) == 0 and n.value == 0
    big = (losses.H3dLossTerm * 1)(_term(kind=losses.FOCAL, x=P, gt=P, n=1 << 30))
    assert L.h3d_loss_workspace_bytes(big, 1, ctypes.byref(n)) == 0 and n.value == 16 * 2048
    g8 = (losses.H3dLossTerm * 1)(_term(kind=losses.FOCAL, flags=losses.TUNE_GRID8, x=P, gt=P, n=1 << 30))
    assert L.h3d_loss_workspace_bytes(g8, 1, ctypes.byref(n)) == 0 and n.value == 256
