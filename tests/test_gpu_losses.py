"""GPU: h3d_amd.losses (csrc/loss.hip) against the restatement of tests/losses_ref.py (pinned to the reference's classes by
tests/test_oracle_losses.py).

Rules.  Per-element tensors (gradients): max |g - g64| <= 4 e32 + 1e-7 max |g64|, e32 = max |g32 - g64| of the restatement's own fp32
run (the rule of tests/test_gpu_dcn_backward.py); the stored `pred` is bit-equal to h3d_sigmoid_clamp.  Scalar losses: a single number's
fp32 error is a matter of luck, so the yardstick is pooled -- e32 = the largest relative error of the fp32 restatement over the 8 seeds
of a case, and the kernel's relative error on EVERY seed must be <= 4 e32 + 1e-7.  The ratios are printed (`pytest -s`); the worst per
case is recorded in DESIGN.md section 15.

The grid of a focal term is min(ceil(n / 1024), 2048) workgroups: at none of the shapes below does the default grid wrap (the largest,
(2,18,128,128), takes 576), so every focal case also runs with H3D_LOSS_TUNE_GRID8 (at most 8 workgroups: the loop wraps from 8192
elements on); the uncapped-to-capped transition itself is covered by tools/time_losses.py at the workload's shape."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import losses_ref as R
from gpu_helpers import DEV
from h3d_amd import _lib, arch, losses, model, synth, utils
from h3d_amd.detector import Opt

pytestmark = pytest.mark.gpu
SEEDS = tuple(range(100, 108))
FOCAL_SHAPES = [(1, 1, 1, 3), (2, 17, 8, 12), (3, 1, 33, 37), (2, 18, 128, 128)]
F64, F32 = torch.float64, torch.float32


def misaligned(t):
    """A contiguous copy of t on the GPU whose data_ptr() % 16 == 4."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def place(t, mis):
    return misaligned(t) if mis else t.to(DEV)


# ---- references, computed once per (case, seed) on the CPU -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def focal_ref(seed, shape, positives, logits):
    x, gt = R.focal_inputs(seed, shape, positives)
    head = x if logits else R.sigmoid_clamp(x)
    fn = R.focal_logits if logits else R.focal
    v64, g64 = R.value_and_grad(lambda h: fn(h, gt.double()), head, F64)
    v32, g32 = R.value_and_grad(lambda h: fn(h, gt), head, F32)
    return head, gt, v64, g64, v32, g32


@functools.lru_cache(maxsize=None)
def reg_ref(seed, cls, B, C, M, mask_f32, zero_mask=False):
    feat, mask, ind, target = R.reg_inputs(seed, cls, B, C, M, 8, 12, F32 if mask_f32 else torch.uint8, zero_mask)
    v64, g64 = R.value_and_grad(lambda h: R.reg(cls, h, mask, ind, target.double()), feat, F64)
    v32, g32 = R.value_and_grad(lambda h: R.reg(cls, h, mask, ind, target), feat, F32)
    return feat, mask, ind, target, v64, g64, v32, g32


def run_focal(head, gt, logits, mis=False, flags=0):
    """-> (loss, grad, pred | None, stats) through the Function, on `head` placed aligned or 4 bytes off."""
    h = place(head, mis).requires_grad_(True)
    term = losses.focal_term(h, place(gt, mis), from_logits=logits, flags=flags)
    ls, total = losses.fused([term])
    g, = torch.autograd.grad(ls[0], h)
    return ls[0].detach(), g, term.pred, total.detach()


# ---- focal ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logits", [True, False], ids=["from_logits", "probabilities"])
@pytest.mark.parametrize("shape", FOCAL_SHAPES)
def test_focal_values_gradients_and_stored_pred(shape, logits):
    refs = [focal_ref(s, shape, "some", logits) for s in SEEDS]
    e32 = R.pooled_e32([r[4] for r in refs], [r[2] for r in refs])
    for mis, flags in ((False, 0), (True, 0), (False, losses.TUNE_GRID8), (True, losses.TUNE_GRID8)):
        got = []
        for s, (head, gt, v64, g64, v32, g32) in zip(SEEDS, refs):
            loss, g, pred, _ = run_focal(head, gt, logits, mis, flags)
            got.append(loss.cpu())
            if s in SEEDS[:2]:
                R.check_tensor("focal %s mis=%d flags=%x seed %d grad" % (shape, mis, flags, s), g, g64, g32)
                if logits:
                    assert torch.equal(pred, utils._sigmoid(head.to(DEV))), "stored pred is not h3d_sigmoid_clamp's"
                else:
                    assert pred is None
        R.check_scalars("focal %s logits=%d mis=%d flags=%x" % (shape, logits, mis, flags), got, [r[2] for r in refs], e32)


@pytest.mark.parametrize("positives", ["none", "all"])
@pytest.mark.parametrize("logits", [True, False], ids=["from_logits", "probabilities"])
def test_focal_zero_positives_and_all_positive_maps(positives, logits):
    shape = (2, 3, 8, 12)
    refs = [focal_ref(s, shape, positives, logits) for s in SEEDS]
    e32 = R.pooled_e32([r[4] for r in refs], [r[2] for r in refs])
    got = []
    for s, (head, gt, v64, g64, v32, g32) in zip(SEEDS, refs):
        loss, g, pred, _ = run_focal(head, gt, logits)
        got.append(loss.cpu())
        R.check_tensor("focal %s seed %d grad" % (positives, s), g, g64, g32)
    R.check_scalars("focal positives=%s logits=%d" % (positives, logits), got, [r[2] for r in refs], e32)
    # the device-side `num_pos == 0` select: aux = {pos, neg, num_pos}
    head, gt = refs[0][0], refs[0][1]
    st = losses.forward_terms([losses.focal_term(head.to(DEV), gt.to(DEV), from_logits=logits)]).cpu()
    assert float(st[3]) == (0 if positives == "none" else gt.numel())
    if positives == "none":
        assert float(st[1]) == 0 and float(st[0]) == -float(st[2])


# ---- regression -----------------------------------------------------------------------------------------------------------------------
REG_KIND = {"RegL1Loss": losses.RegL1Loss, "RegWeightedL1Loss": losses.RegWeightedL1Loss, "NormRegL1Loss": losses.NormRegL1Loss,
            "RegLoss": losses.RegLoss}


def run_reg(cls, feat, mask, ind, target):
    h = feat.to(DEV).requires_grad_(True)
    loss = REG_KIND[cls]()(h, mask.to(DEV), ind.to(DEV), target.to(DEV))
    g, = torch.autograd.grad(loss, h)
    return loss.detach(), g


@pytest.mark.parametrize("mask_f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("bcm", [(1, 1, 1), (3, 2, 32), (1, 34, 32), (3, 34, 1)], ids=lambda v: "B%d_C%d_M%d" % v)
@pytest.mark.parametrize("cls", R.REG_CLASSES)
def test_regression_values_and_gradients(cls, bcm, mask_f32):
    B, C, M = bcm
    refs = [reg_ref(s, cls, B, C, M, mask_f32) for s in SEEDS]
    e32 = R.pooled_e32([r[6] for r in refs], [r[4] for r in refs])
    got = []
    for s, (feat, mask, ind, target, v64, g64, v32, g32) in zip(SEEDS, refs):
        loss, g = run_reg(cls, feat, mask, ind, target)
        got.append(loss.cpu())
        R.check_tensor("%s %s f32mask=%d seed %d grad" % (cls, bcm, mask_f32, s), g, g64, g32)
    R.check_scalars("%s %s f32mask=%d" % (cls, bcm, mask_f32), got, [r[4] for r in refs], e32)
    if M == 32:
        ind = refs[0][2]
        assert int(ind.min()) == 0 and int(ind.max()) == 95 and bool((ind[:, 2] == ind[:, 3]).all())


@pytest.mark.parametrize("cls", R.REG_CLASSES)
def test_all_zero_mask_gives_exactly_zero_loss_and_gradient(cls):
    feat, mask, ind, target = reg_ref(SEEDS[0], cls, 3, 2, 32, False, True)[:4]
    assert int(mask.sum()) == 0
    loss, g = run_reg(cls, feat, mask, ind, target)
    assert float(loss) == 0.0 and not bool(g.any())
    loss, g = run_reg(cls, feat, mask.float(), ind, target)
    assert float(loss) == 0.0 and not bool(g.any())


def test_out_of_range_ind_contributes_nothing_and_reads_nothing():
    feat, mask, ind, target = R.reg_inputs(7, "RegL1Loss", 2, 2, 32, 8, 12)
    mask[:, :6] = 1
    bad = ind.clone()
    bad[:, 0], bad[:, 1], bad[:, 4] = -1, 96, 1 << 40
    masked = mask.clone()
    masked[:, [0, 1, 4]] = 0
    a = run_reg("RegL1Loss", feat, mask, bad, target)
    b = run_reg("RegL1Loss", feat, masked, ind, target)
    assert torch.equal(a[0], b[0]) and float((a[1] - b[1]).abs().max()) <= 1e-7 * float(b[1].abs().max())


# ---- determinism, streams, guards ------------------------------------------------------------------------------------------------------
def _multi_pose_terms(output, batch, reg_kind=losses.REG_L1):
    o, b = {k: v.to(DEV) for k, v in output.items()}, {k: v.to(DEV) for k, v in batch.items()}
    return [losses.focal_term(o["hm"], b["hm"], 1.0, from_logits=True),
            losses.reg_term(losses.REG_WEIGHTED_L1, o["hps"], b["hps_mask"], b["ind"], b["hps"], 1.0),
            losses.reg_term(reg_kind, o["wh"], b["reg_mask"], b["ind"], b["wh"], 0.1),
            losses.reg_term(reg_kind, o["reg"], b["reg_mask"], b["ind"], b["reg"], 1.0),
            losses.reg_term(reg_kind, o["hp_offset"], b["hp_mask"], b["hp_ind"], b["hp_offset"], 1.0),
            losses.focal_term(o["hm_hp"], b["hm_hp"], 1.0, from_logits=True)]


def test_two_runs_are_bit_equal_and_backward_is_bit_equal_where_ind_does_not_repeat():
    output, batch = R.multi_pose_inputs(3, 2, 33, 37)
    terms = _multi_pose_terms(output, batch)
    s1, s2 = losses.forward_terms(terms), losses.forward_terms(terms)
    assert torch.equal(s1, s2) and bool(torch.isfinite(s1).all())
    coef = torch.tensor([1.0, 0.5, 2.0, 1.0, 1.0, 3.0], device=DEV)
    runs = []
    for _ in range(2):
        grads = [torch.empty_like(t.x) for t in terms]
        losses.backward_terms(terms, s1, coef, grads)
        runs.append(grads)
    for i, t in enumerate(terms):
        a, b = runs[0][i], runs[1][i]
        if t.kind == losses.FOCAL:
            assert torch.equal(a, b)
            continue
        B, C = t.x.shape[:2]
        cnt = torch.zeros(B, t.x.shape[2] * t.x.shape[3], device=DEV).scatter_add_(1, t.ind, torch.ones_like(t.ind, dtype=F32))
        single = (cnt <= 1)[:, None, :].expand(B, C, -1).reshape(t.x.shape)
        assert torch.equal(a[single], b[single]) and bool((cnt > 1).any())
        assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max())


def test_a_non_default_stream_gives_the_same_result():
    output, batch = R.multi_pose_inputs(4, 2, 8, 12)
    terms = _multi_pose_terms(output, batch)
    ref = losses.forward_terms(terms)
    coef = torch.ones(6, device=DEV)
    g_ref = [torch.empty_like(t.x) for t in terms]
    losses.backward_terms(terms, ref, coef, g_ref)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = losses.forward_terms(terms)
        g = [torch.empty_like(t.x) for t in terms]
        losses.backward_terms(terms, got, coef, g)
    st.synchronize()
    assert torch.equal(got, ref)
    assert torch.equal(g[0], g_ref[0]) and torch.equal(g[5], g_ref[5])
    for a, b in zip(g[1:5], g_ref[1:5]):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


def test_no_grad_returns_tensors_without_grad_fn():
    output, batch = R.multi_pose_inputs(4, 1, 8, 12)
    o = {k: v.to(DEV).requires_grad_(True) for k, v in output.items()}
    b = {k: v.to(DEV) for k, v in batch.items()}
    with torch.no_grad():
        loss, st = losses.loss_multi_pose(Opt())([dict(o)], b)
        single = losses.FocalLoss()(utils._sigmoid(o["hm"]), b["hm"])
    assert loss.grad_fn is None and not loss.requires_grad and loss.dim() == 0 and loss.dtype == F32 and loss.is_cuda
    assert all(v.grad_fn is None for v in st.values()) and single.grad_fn is None
    loss2, _ = losses.loss_multi_pose(Opt())([dict(o)], b)
    assert loss2.grad_fn is not None and torch.equal(loss2.detach(), loss)


# ---- fused task losses ------------------------------------------------------------------------------------------------------------------
def _task(task, reg_loss, seed=21, B=2, H=8, W=12):
    if task == "multi_pose":
        output, batch = R.multi_pose_inputs(seed, B, H, W)
        return output, batch, R.multi_pose, losses.loss_multi_pose(Opt(reg_loss=reg_loss))
    output, batch = R.ctdet_inputs(seed, B, H, W)
    return output, batch, R.ctdet, losses.loss_obj_detection(Opt(task="ctdet", num_classes=3, reg_loss=reg_loss))


@pytest.mark.parametrize("reg_loss", ["l1", "sl1"])
@pytest.mark.parametrize("task", ["multi_pose", "ctdet"])
def test_fused_task_loss_equals_the_per_class_calls_and_the_restatement(task, reg_loss):
    rows = []
    for seed in SEEDS:
        output, batch, ref_fn, mod = _task(task, reg_loss, seed)
        l64, st64 = ref_fn(R.cast(output, F64), R.cast(batch, F64), reg_loss)
        l32, st32 = ref_fn(output, batch, reg_loss)
        o, b = {k: v.to(DEV) for k, v in output.items()}, {k: v.to(DEV) for k, v in batch.items()}
        outs = [dict(o)]
        loss, st = mod(outs, b)
        assert set(st) == set(st64) and st["loss"] is loss
        assert torch.equal(outs[0]["hm"], utils._sigmoid(o["hm"])) and torch.equal(o["hm"].cpu(), output["hm"])
        # the per-class calls combined with the weights
        crit = losses.RegL1Loss() if reg_loss == "l1" else losses.RegLoss()
        single = {"hm_loss": losses.FocalLoss()(utils._sigmoid(o["hm"]), b["hm"]),
                  "wh_loss": crit(o["wh"], b["reg_mask"], b["ind"], b["wh"]), "off_loss": crit(o["reg"], b["reg_mask"], b["ind"], b["reg"])}
        if task == "multi_pose":
            single.update({"hm_hp_loss": losses.FocalLoss()(utils._sigmoid(o["hm_hp"]), b["hm_hp"]),
                           "hp_loss": losses.RegWeightedL1Loss()(o["hps"], b["hps_mask"], b["ind"], b["hps"]),
                           "hp_offset_loss": crit(o["hp_offset"], b["hp_mask"], b["hp_ind"], b["hp_offset"])})
        for k, v in single.items():
            assert torch.equal(v, st[k]), (k, float(v), float(st[k]))       # the same kernels on the same values
        w = R.WEIGHTS
        comb = sum(float(w[n]) * float(single[k]) for k, n in (("hm_loss", "hm_weight"), ("wh_loss", "wh_weight"), ("off_loss", "off_weight"),
                                                                 ("hp_loss", "hp_weight"), ("hm_hp_loss", "hm_hp_weight"),
                                                                 ("hp_offset_loss", "off_weight")) if k in single)
        assert abs(comb - float(loss)) <= 2e-7 * abs(comb)                  # fp64 sum of fp32 terms, rounded once
        rows.append((st, st64, st32))
    for k in rows[0][1]:
        e32 = R.pooled_e32([r[2][k] for r in rows], [r[1][k] for r in rows])
        R.check_scalars("%s %s %s" % (task, reg_loss, k), [r[0][k].cpu() for r in rows], [r[1][k] for r in rows], e32)


@pytest.mark.parametrize("task", ["multi_pose", "ctdet"])
@pytest.mark.parametrize("what", ["loss", "hm_loss", "hm_loss+wh_loss"])
def test_fused_backward_from_any_combination_of_the_returned_scalars(task, what):
    output, batch, ref_fn, mod = _task(task, "l1")
    heads = sorted(output)

    def ref(dtype):
        leaves = {k: output[k].to(dtype).clone().requires_grad_(True) for k in heads}
        _, st = ref_fn(leaves, R.cast(batch, dtype), "l1")
        return torch.autograd.grad(sum(st[k] for k in what.split("+")), [leaves[k] for k in heads], allow_unused=True)
    g64, g32 = ref(F64), ref(F32)
    o = {k: output[k].to(DEV).requires_grad_(True) for k in heads}
    _, st = mod([dict(o)], {k: v.to(DEV) for k, v in batch.items()})
    got = torch.autograd.grad(sum(st[k] for k in what.split("+")), [o[k] for k in heads], allow_unused=True)
    for k, g, r64, r32 in zip(heads, got, g64, g32):
        if r64 is None:
            assert g is None or not bool(g.any()), k
            continue
        R.check_tensor("%s d(%s)/d %s" % (task, what, k), g, r64, r32)


def test_a_term_whose_head_needs_no_grad_leaves_its_buffer_untouched():
    output, batch = R.multi_pose_inputs(9, 2, 8, 12)
    terms = _multi_pose_terms(output, batch)
    stats = losses.forward_terms(terms)
    coef = torch.ones(6, device=DEV)
    full = [torch.empty_like(t.x) for t in terms]
    losses.backward_terms(terms, stats, coef, full)
    for i in range(6):
        bufs = [torch.full_like(t.x, 777.0) for t in terms]
        losses.backward_terms(terms, stats, coef, [bufs[j] if j == i else None for j in range(6)])
        torch.cuda.synchronize()
        for j in range(6):
            if j != i:
                assert bool((bufs[j] == 777.0).all()), (i, j)
        assert float((bufs[i] - full[i]).abs().max()) <= 1e-6 * float(full[i].abs().max())
    # through autograd: only `wh` requires grad
    o = {k: v.to(DEV) for k, v in output.items()}
    o["wh"].requires_grad_(True)
    loss, _ = losses.loss_multi_pose(Opt())([dict(o)], {k: v.to(DEV) for k, v in batch.items()})
    loss.backward()
    assert o["wh"].grad is not None and all(o[k].grad is None for k in o if k != "wh")
    assert float((o["wh"].grad - 0.1 * full[2]).abs().max()) <= 1e-6 * float(full[2].abs().max())


def test_empty_terms_and_no_terms():
    L = _lib.lib()
    stats = torch.full((1,), 5.0, device=DEV)
    _lib.check(L.h3d_loss_forward(None, 0, _lib.ptr(stats), None, 0, _lib.stream_ptr()), "loss_forward")
    assert float(stats[0]) == 0.0
    e = torch.empty(0, device=DEV)
    x, gt = R.focal_inputs(1, (1, 1, 4, 4))
    st = losses.forward_terms([losses.focal_term(e, e), losses.focal_term(x.to(DEV), gt.to(DEV), 2.0, from_logits=True),
                               losses.reg_term(losses.REG_L1, torch.empty(2, 0, 4, 4, device=DEV), torch.zeros(2, 3, dtype=torch.uint8, device=DEV),
                                               torch.zeros(2, 3, dtype=torch.int64, device=DEV), torch.empty(2, 3, 0, device=DEV))]).cpu()
    assert st[:4].tolist() == [0, 0, 0, 0] and st[8:12].tolist() == [0, 0, 0, 0] and float(st[4]) > 0
    assert float(st[12]) == pytest.approx(2 * float(st[4]), rel=1e-7)


# ---- gradcheck (eps / atol / rtol of tests/test_gpu_dcn_backward.py's) -----------------------------------------------------------------
def test_gradcheck_focal_and_regl1_through_the_functions():
    x, gt = R.focal_inputs(3, (1, 1, 1, 3))
    gt[0, 0, 0, 0] = 1.0
    p = (0.2 + 0.6 * torch.rand(1, 1, 1, 3, generator=torch.Generator().manual_seed(1))).to(DEV).requires_grad_(True)
    gtd = gt.to(DEV)
    assert torch.autograd.gradcheck(lambda t: losses.FocalLoss()(t, gtd), (p,), eps=1e-3, atol=1e-4, rtol=1e-2, nondet_tol=1e-5)
    feat, mask, ind, target = R.reg_inputs(25, "RegL1Loss", 1, 1, 1, 8, 12)
    mask[:] = 1
    target[:] = feat.reshape(-1)[int(ind[0, 0])] + 0.5           # eps = 1e-3 must not straddle the kink of |.|
    f = feat.to(DEV).requires_grad_(True)
    m, i, t = mask.to(DEV), ind.to(DEV), target.to(DEV)
    assert torch.autograd.gradcheck(lambda h: losses.RegL1Loss()(h, m, i, t), (f,), eps=1e-3, atol=1e-4, rtol=1e-2, nondet_tol=1e-5)


# ---- the validation path ---------------------------------------------------------------------------------------------------------------
def test_validation_path_dla_net_then_loss_multi_pose():
    heads = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}
    sd = synth.synth_state_dict(arch.state_dict_shapes(heads, True), seed=0)
    m = model.dla_net(heads, dtype="f32")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    with torch.no_grad():
        outputs = m(torch.from_numpy(synth.synth_images(1, 64, 96, seed=17)).to(DEV))
        kept = {k: v for k, v in outputs[0].items()}
        before = {k: v.clone() for k, v in kept.items()}
        _, batch = R.multi_pose_inputs(31, 1, 16, 24)
        loss, st = losses.loss_multi_pose(Opt())(outputs, {k: v.to(DEV) for k, v in batch.items()})
    want, st64 = R.multi_pose({k: v.cpu().double() for k, v in before.items()}, R.cast(batch, F64))
    w32, _ = R.multi_pose({k: v.cpu() for k, v in before.items()}, batch)
    e32 = R.rel(w32, want)
    print("validation loss %.6g ref %.6g rel err %.3g (fp32 restatement %.3g)" % (float(loss), float(want), R.rel(loss.cpu(), want), e32))
    assert R.rel(loss.cpu(), want) <= 1e-5          # the upper end of the fp32 restatement's own error over seeds (2e-8 .. 1e-5)
    for k in st64:
        assert R.rel(st[k].cpu(), st64[k]) <= 1e-5, k
    for k, v in kept.items():
        assert torch.equal(v, before[k]), k          # the plan's head buffers are not written
    assert torch.equal(outputs[0]["hm"], utils._sigmoid(before["hm"])) and torch.equal(outputs[0]["hm_hp"], utils._sigmoid(before["hm_hp"]))
    assert outputs[0]["hm"].data_ptr() != kept["hm"].data_ptr()
