"""CPU: the restatement of tests/targets_ref.py against the reference's own label code (tests/golden/targets_ref.npz, written by
tools/gen_targets_golden.py), the host get_affine_transform against the golden's matrices, and the argument checks of the ABI
(include/h3d.h section 6) through calls that return before any launch."""
import ctypes
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest

import targets_ref as R
from h3d_amd import _lib, targets

ROW_TOL = 2.0 ** -16          # 2 ulp of float32 at magnitude 128: each box edge carries one float32 rounding of a float64 sum
INT_KEYS = ("ind", "reg_mask", "hps_mask", "hp_ind", "hp_mask", "cat_spec_mask", "gt_count")
MAP_KEYS = ("hm", "hm_hp")
ERR_SHAPE, ERR_UNSUPPORTED, ERR_ARG = -1, -4, -5


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "targets_ref.npz"))
    cases = {}
    for key in z.files:
        name, kind, field = key.split(".")
        cases.setdefault(name, {"in": {}, "out": {}})[kind][field] = z[key]
    return cases


def restate(name, case):
    i = case["in"]
    if name.startswith("mp_"):
        res = int(i["res"])
        return R.multi_pose_image(i["boxes"], i["keypoints"], i["num"], i["trans"], float(i["rot"]) != 0, bool(i["flipped"]), int(i["width"]),
                                  out_h=res, out_w=res, max_objs=32)
    return R.ctdet_image(i["boxes"], i["cls"], i["num"], i["trans"], bool(i["flipped"]), int(i["width"]), out_h=int(i["out_h"]),
                         out_w=int(i["out_w"]), num_classes=int(i["classes"]), max_objs=32)


def test_golden_holds_the_cases_the_gpu_tests_name(golden):
    assert {"mp_plain", "mp_flip", "mp_rot", "mp_empty", "mp_res33_clamp"} <= set(golden)
    assert int(golden["mp_empty"]["out"]["gt_count"]) == 0 and int(golden["mp_res33_clamp"]["in"]["num"]) == 40
    for name, case in golden.items():
        if name != "mp_empty":
            assert int(case["out"]["gt_count"]) > 0, name
    assert sum(1 for c in golden.values() if c["out"]["hm"].shape[-1] == 128) <= 3


def test_restatement_equals_the_reference_on_every_array(golden):
    for name, case in golden.items():
        got = restate(name, case)
        assert set(got) == set(case["out"]), name
        for key, ref in case["out"].items():
            g = np.asarray(got[key])
            assert g.shape == ref.shape and g.dtype == ref.dtype, (name, key, g.shape, ref.shape, g.dtype, ref.dtype)
            if key in INT_KEYS:
                assert np.array_equal(g, ref), (name, key)
            elif key in MAP_KEYS:
                assert int((g != ref).sum()) == 0, (name, key, int((g != ref).sum()))          # same float64 exp, same rounding: 0 pixels
            else:
                err = float(np.abs(g.astype(np.float64) - ref).max()) if ref.size else 0.0
                assert err <= ROW_TOL, (name, key, err)


def test_reference_facts_the_kernels_rely_on(golden):
    """hm is 1.0 at every live centre (the 0.9999 of a person without keypoints is overwritten by that person's own splat), a rotated
    image has hm = 0.9999 everywhere with reg_mask = hps_mask = 0 while the other rows stay."""
    o = golden["mp_plain"]["out"]
    n = int(o["gt_count"])
    assert int(golden["mp_plain"]["in"]["num"]) == n and (o["hm"].reshape(-1)[o["ind"][:n]] == 1.0).all()
    assert o["reg_mask"][:n].sum() == n - 1                     # the person without keypoints
    r = golden["mp_rot"]["out"]
    assert (r["hm"] == np.float32(0.9999)).all() and not r["reg_mask"].any() and not r["hps_mask"].any()
    assert r["hp_mask"].any() and r["hm_hp"].max() == 1.0 and np.abs(r["wh"]).max() > 0


def test_host_get_affine_transform_against_the_golden_matrices(golden):
    for name, case in golden.items():
        i = case["in"]
        s = i["s"] if i["s"].ndim else float(i["s"])
        if name.startswith("mp_"):
            size, rot = [int(i["res"])] * 2, float(i["rot"])
        else:
            size, rot = [int(i["out_w"]), int(i["out_h"])], 0.0
        t0 = targets.get_affine_transform(i["c"], s, 0, size)
        t1 = targets.get_affine_transform(i["c"], s, rot, size)
        assert t0.shape == (2, 3) and t0.dtype == np.float64
        assert np.abs(np.stack([t0.reshape(6), t1.reshape(6)]) - i["trans"]).max() <= 1e-9, name
        both = targets.target_transforms(i["c"][None], np.asarray(s)[None], [rot], size[0], size[1]).numpy()
        assert np.array_equal(both[0, 0], t0.reshape(6)) and np.array_equal(both[0, 1], t1.reshape(6))
    # the inverse maps back
    t = targets.get_affine_transform(np.array([320, 240], np.float32), 640.0, 17.0, [128, 128])
    ti = targets.get_affine_transform(np.array([320, 240], np.float32), 640.0, 17.0, [128, 128], inv=1)
    p = np.array([100.0, 50.0, 1.0])
    assert np.abs(ti @ np.append(t @ p, 1.0) - p[:2]).max() < 1e-4


def test_margin_check_of_the_generator():
    d = dict(h=np.array([3.5, 0.0], np.float32), w=np.array([2.25, 7.0], np.float32), live=np.array([True, False]),
             bb=np.array([[1, 1, 3.25, 4.5], [0, 7, 7, 7]], np.float32), r_real=np.array([1.4, 1e-17]), ct=np.array([[2.125, 2.75], [3.5, 7]], np.float32))
    assert abs(R.margins(d, 8, 8) - 0.125) < 1e-12              # ct_x; the clipped y axis of the dead object and its tiny radius do not count
    d["pts"] = np.array([[4.00001, 3.5]], np.float32)
    assert R.margins(d, 8, 8) < 1e-4


# ---- the ABI's argument checks: every call below returns before a launch -------------------------------------------------------------
def _pose_call(L, **kw):
    a = dict(boxes=8, keypoints=8, num=8, trans=8, rot_flag=0, flipped=0, width=0, flip_pairs=0, n_pairs=0, B=1, M=4, J=17, H=8, W=8, N=32,
             outs=[0] * 13, options=0, ws=0, ws_bytes=0)
    a.update(kw)
    return L.h3d_multi_pose_targets(a["boxes"], a["keypoints"], a["num"], a["trans"], a["rot_flag"], a["flipped"], a["width"], a["flip_pairs"],
                                    a["n_pairs"], a["B"], a["M"], a["J"], a["H"], a["W"], a["N"], *a["outs"], a["options"], a["ws"], a["ws_bytes"], None)


def _ctdet_call(L, **kw):
    a = dict(boxes=8, cls=8, num=8, trans=8, flipped=0, width=0, B=1, M=4, H=8, W=8, C=80, N=32, outs=[0] * 9, options=0, ws=0, ws_bytes=0)
    a.update(kw)
    return L.h3d_ctdet_targets(a["boxes"], a["cls"], a["num"], a["trans"], a["flipped"], a["width"], a["B"], a["M"], a["H"], a["W"], a["C"], a["N"],
                               *a["outs"], a["options"], a["ws"], a["ws_bytes"], None)


def test_abi_return_codes_for_bad_arguments():
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.h3d_targets_workspace_bytes(64, 32, 17, ctypes.byref(n)) == 0 and n.value == 64 * 18 * 32 * 16
    assert L.h3d_targets_workspace_bytes(2, 128, 0, ctypes.byref(n)) == 0 and n.value == 2 * 128 * 16
    assert L.h3d_targets_workspace_bytes(2, 32, 17, None) == ERR_ARG
    assert L.h3d_targets_workspace_bytes(-1, 32, 17, ctypes.byref(n)) == ERR_SHAPE
    for call in (_pose_call, _ctdet_call):
        assert call(L, B=0) == 0                                                      # nothing to do, nothing launched
        for opt in (targets.MSE_LOSS, targets.DENSE_HP, targets.DENSE_WH):
            assert call(L, options=opt) == ERR_UNSUPPORTED
        assert b"not built" in L.h3d_last_error()
        assert call(L, options=8) == ERR_ARG
        assert call(L, B=-1) == ERR_SHAPE and call(L, H=0) == ERR_SHAPE and call(L, W=16385) == ERR_SHAPE and call(L, N=0) == ERR_SHAPE
        assert call(L, B=65536) == ERR_SHAPE
        assert call(L, N=513) == ERR_UNSUPPORTED
        assert call(L, boxes=0) == ERR_ARG and call(L, num=0) == ERR_ARG and call(L, trans=0) == ERR_ARG
        assert call(L, flipped=8) == ERR_ARG                                          # a mirror without the widths
        assert call(L, boxes=10) == ERR_ARG and call(L, trans=12) == ERR_ARG          # misaligned
        outs = [0] * (13 if call is _pose_call else 9)
        outs[0] = 16                                                                  # hm wanted: the workspace is checked
        assert call(L, outs=outs) == ERR_ARG and b"workspace" in L.h3d_last_error()
        assert call(L, outs=outs, ws=16, ws_bytes=15) == ERR_ARG and b"workspace" in L.h3d_last_error()
        outs[0], outs[4 if call is _pose_call else 3] = 0, 12                         # ind: int64 at 4 mod 8
        assert call(L, outs=outs) == ERR_ARG
    assert _pose_call(L, J=65) == ERR_UNSUPPORTED and _pose_call(L, keypoints=0) == ERR_ARG
    assert _pose_call(L, n_pairs=-1) == ERR_SHAPE and _pose_call(L, n_pairs=8) == ERR_ARG
    assert _ctdet_call(L, C=0) == ERR_SHAPE and _ctdet_call(L, cls=0) == ERR_ARG


def test_out_of_scope_options_raise_value_error():
    z = np.zeros((1, 1, 4), np.float32)
    kp = np.zeros((1, 1, 17, 3), np.float32)
    for name in ("mse_loss", "dense_hp"):
        with pytest.raises(ValueError):
            targets.multi_pose_targets(z, kp, [1], [[4, 4]], [8.0], opt=NS(**{name: True}))
    for name in ("mse_loss", "dense_wh"):
        with pytest.raises(ValueError):
            targets.ctdet_targets(z, np.zeros((1, 1), np.int32), [1], [[4, 4]], [8.0], opt=NS(**{name: True}))
    with pytest.raises(ValueError):
        targets.multi_pose_targets(z, kp, [1], [[4, 4]], [8.0], flipped=[1], opt=NS(), device="cpu")
