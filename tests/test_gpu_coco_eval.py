"""GPU: csrc/eval.hip (`h3d_coco_match`, `h3d_coco_accumulate`) and h3d_amd/coco_eval.py against the numpy mirror coco_eval.evaluate_numpy,
which tests/test_oracle_coco_eval.py holds to the loop restatement of include/h3d.h section 8.

Bit-equal, nothing excluded: dt_match, dt_ignore, gt_ignore, the ranks, the rounded records (score, box, area, keypoints), the box IoU
matrix, precision, recall, stats.  The OKS matrix is held to 4 ulp: exp is the one operation of the definition that is not correctly
rounded, the device's and numpy's are each within 1 ulp, and the 17 terms are summed in the same order.  For the matches behind an OKS
matrix to be comparable bit for bit the keypoint cases must keep every decision away from those last bits (coco_eval_cases.margins_hold,
asserted on the mirror's matrix: the seeds are fixed and chosen so that it holds)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import coco_eval_cases as cases
from gpu_helpers import DEV
from h3d_amd import _lib, arch, coco_eval as C, model, synth, trainer
from h3d_amd.detector import MultiPoseDetector, Opt

pytestmark = pytest.mark.gpu
CHUNK, MAX_G = _lib.COCO_SCAN_CHUNK, _lib.COCO_MAX_G


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def ulps(a, b):
    """The distance in representable doubles between two arrays of non-negative finite doubles."""
    return int(np.abs(bits(a) - bits(b)).max()) if np.size(a) else 0


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def check(res, gt, iou_type, det_cls=None, det_num=None, round2=True, want_ious=True):
    """match + accumulate on the device against the mirror -> (device match dict, mirror EvalResult, device precision, recall)."""
    kp = iou_type == "keypoints"
    ref = C.evaluate_numpy(res, gt, iou_type, det_cls, det_num, round2)
    rm = ref.extra["match"]
    if kp:
        assert cases.margins_hold(rm, gt), "the case puts a decision within 1e-9 of the last bits of an OKS value: pick another seed"
    m = C.match(dev(res), gt, iou_type, dev(det_cls, np.int32), dev(det_num, np.int32), round2, want_ious=want_ious)
    precision, recall = C.accumulate(m, gt)
    torch.cuda.synchronize()
    for k in ("dt_match", "dt_ignore", "gt_ignore", "dt_rank"):
        assert np.array_equal(m[k].cpu().numpy(), rm[k]), k
    for k in ("dt_score", "dt_box", "dt_area") + (("dt_keypoints",) if kp else ()):
        assert np.array_equal(bits(m[k].cpu().numpy()), bits(rm[k])), k
    if want_ious:
        got = m["ious"].cpu().numpy()
        worst = ulps(got, rm["ious"])
        print("%s matrix %s: worst distance %d ulp" % (iou_type, got.shape, worst))
        assert worst <= (4 if kp else 0)
    else:
        assert m["ious"] is None
    p, r = precision.cpu().numpy(), recall.cpu().numpy()
    assert np.array_equal(bits(p), bits(ref.precision)) and np.array_equal(bits(r), bits(ref.recall))
    assert np.array_equal(bits(C.summarize_stats(p, r, iou_type)), bits(ref.stats))
    return m, ref, p, r


# the shapes: D around the keypoint maxDet (20 | 21), beyond one wave of ranks (65) and at the bbox maxDet (100); G beyond a 64-bit matched
# mask (65); none of either; one image and five
KP_SHAPES = [(1, 0, 9), (1, 1, 1), (5, 1, 0), (5, 20, 9), (5, 21, 9), (1, 21, 1), (5, 65, 65), (1, 100, 9), (5, 100, 65), (5, 0, 0)]
# (seed, spread of the box corners) of the keypoint cases: the crowded ones are spread out, or two ground truths without labelled joints
# both hold all of a detection's joints inside their tripled boxes and tie at an OKS of exactly 1
KP_SEEDS = {(5, 65, 65): (301, 1500.0), (5, 100, 65): (303, 1500.0)}
BB_SHAPES = [(1, 0, 9), (1, 1, 1), (5, 1, 0), (5, 20, 9), (5, 21, 65), (5, 65, 9), (1, 100, 65), (5, 100, 9)]


@pytest.mark.parametrize("N,D,G", KP_SHAPES, ids=lambda v: str(v))
def test_keypoints_against_the_mirror(N, D, G):
    seed, spread = KP_SEEDS.get((N, D, G), (100 + D + G, 400.0))
    res, gt, num = cases.scene(seed, N, D, G, "keypoints", spread=spread)
    m, ref, _, _ = check(res, gt, "keypoints", None, num)
    if G >= 9 and N > 1:
        labelled = (gt.keypoints[..., 2] > 0).sum(-1)
        valid = np.arange(G)[None] < gt.num[:, None]
        assert (valid & (labelled == 0)).any() and (valid & (labelled > 0)).any(), "the case is meant to hold k1 = 0 ground truths"


@pytest.mark.parametrize("N,D,G", BB_SHAPES, ids=lambda v: str(v))
def test_boxes_of_three_classes_against_the_mirror(N, D, G):
    res, gt, num = cases.scene(200 + D + G, N, D, G, "bbox", K=3)
    check(res, gt, "bbox", None, num)
    check(res[:, :, :5].copy(), gt, "bbox", res[:, :, 5].astype(np.int32), num, round2=False)     # classes given apart, no rounding


@pytest.mark.parametrize("iou_type", ["keypoints", "bbox"])
def test_all_scores_equal(iou_type):
    res, gt, num = cases.scene(7, 5, 30, 9, iou_type, K=1 if iou_type == "keypoints" else 2, equal_scores=True)
    assert len(np.unique(res[:, :, 4][np.arange(res.shape[1])[None] < num[:, None]])) == 1 and num.max() == 30
    check(res, gt, iou_type, None, num)


def test_a_cell_without_ground_truth_is_minus_one():
    res, gt, num = cases.scene(8, 5, 30, 9, "bbox", K=2, min_side=120.0)            # every area above 96^2 x 0.4: nothing small
    assert gt.area[np.arange(gt.G)[None] < gt.num[:, None]].min() > 32.0 ** 2
    _, _, p, r = check(res, gt, "bbox", None, num)
    assert np.all(p[:, :, :, 1, :] == -1) and np.all(r[:, :, 1, :] == -1) and np.all(p[:, :, :, 0, :] >= 0)


def test_the_matrix_in_global_memory_and_in_the_workspace():
    # D G 8 bytes above the 96 KiB the kernel keeps in LDS: the walk reads the public matrix, or, without it, the workspace
    for iou_type, D, G in (("bbox", 100, 130), ("keypoints", 100, 130)):
        res, gt, num = cases.scene(307, 2, D, G, iou_type, spread=1500.0)
        assert D * G * 8 > 96 * 1024
        check(res, gt, iou_type, None, num)
        check(res, gt, iou_type, None, num, want_ious=False)
    res, gt, num = cases.scene(10, 3, 21, 9, "keypoints")
    check(res, gt, "keypoints", None, num, want_ious=False)                           # ... and in LDS without the public matrix


def test_more_ground_truths_than_the_limit_are_refused():
    G = MAX_G + 1
    gt = C.GroundTruth(np.zeros((1, G, 4)), None, np.zeros((1, G)), np.zeros((1, G)), None, [1], 1)
    res = torch.zeros(1, 4, 6, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported.*ground truths"):
        C.match(res, gt, "bbox")
    with pytest.raises(RuntimeError, match="unsupported.*detections"):
        C.match(torch.zeros(1, _lib.COCO_MAX_D + 1, 6, device=DEV), C.GroundTruth(np.zeros((1, 1, 4)), None, [[0]], [[0]], None, [0], 1), "bbox")
    ok = C.GroundTruth(np.zeros((1, MAX_G, 4)), None, np.zeros((1, MAX_G)), np.zeros((1, MAX_G)), None, [MAX_G], 1)
    m = C.match(res, ok, "bbox")                                                      # the limit itself runs
    torch.cuda.synchronize()
    assert m["gt_ignore"].shape == (1, 4, MAX_G) and int(m["dt_match"].max()) == -1


def test_two_scan_chunks_plus_three_detections():
    N, D = 21, 100
    res, gt, _ = cases.scene(11, N, D, 4, "bbox", full_dets=True)
    num = np.full(N, D, np.int32)
    num[-1] = 2 * CHUNK + 3 - (N - 1) * D
    assert 0 < num[-1] <= D and int(num.sum()) == 2 * CHUNK + 3
    m, _, _, _ = check(res, gt, "bbox", None, num)
    order, seg = C.sort_detections(m, 1)
    assert seg.tolist() == [0, 2 * CHUNK + 3]


def test_evaluator_fed_in_two_batches_equals_one_call():
    for iou_type in ("keypoints", "bbox"):
        res, gt, num = cases.scene(12, 5, 21, 9, iou_type, K=1 if iou_type == "keypoints" else 3)
        one = C.evaluate(dev(res), gt, iou_type, None, dev(num))
        ev = C.CocoEvaluator(gt, iou_type)
        ev.update([3, 4], dev(res[3:]), det_num=dev(num[3:]))
        ev.update(torch.tensor([0, 1, 2]), dev(res[:3]), det_num=dev(num[:3]))
        two = ev.compute()
        assert np.array_equal(bits(one.precision), bits(two.precision)) and np.array_equal(bits(one.recall), bits(two.recall))
        assert np.array_equal(bits(one.stats), bits(two.stats)) and len(one.stats) == (10 if iou_type == "keypoints" else 12)
        ref = C.evaluate_numpy(res, gt, iou_type, None, num)
        assert np.array_equal(bits(one.stats), bits(ref.stats))


def test_a_perfect_detection_and_a_second_stream():
    b = np.array([[[10.25, 20.5, 60.0, 80.0]]])
    k = np.concatenate([np.array([[30.0, 40.0]]) + np.arange(17)[:, None], np.full((17, 1), 2.0)], 1)[None, None]
    gt = C.GroundTruth(b, k, [[2400.0]], [[0]], None, [1], 1)
    res = np.zeros((1, 1, 39), np.float32)
    res[0, 0, :5] = [10.25, 20.5, 70.25, 100.5, 0.9]
    res[0, 0, 5:] = k[0, 0, :, :2].reshape(-1)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        kp, bb = C.evaluate(dev(res), gt, "keypoints"), C.evaluate(dev(res), gt, "bbox")
    for r in (kp, bb):
        sel = r.stats[r.stats > -1]
        assert len(sel) >= 6 and np.abs(sel - 1).max() <= 1e-12
    assert len(kp.summarize()) == 10 and len(bb.summarize()) == 12


# ---- the trainer's val() -------------------------------------------------------------------------------------------------------------------
HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}


def test_heads_trainer_val_on_four_images_equals_evaluate_on_the_detectors_results():
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(arch.state_dict_shapes(HEADS, True, 64), seed=0).items()}
    x = torch.from_numpy(synth.synth_images(4, 128, 128)).to(DEV)
    c, s = np.full((4, 2), 64.0, np.float32), np.full(4, 128.0, np.float32)
    det = MultiPoseDetector(Opt(input_h=128, input_w=128, head_conv=64, dtype="f32", K=20), sd, device=DEV)
    results = torch.cat([det.run(x[i:i + 2], meta={"c": c[i:i + 2], "s": s[i:i + 2]})["results"] for i in (0, 2)])
    assert results.shape == (4, 20, 39)
    # ground truth: every image's three best detections, to two decimals, so the run scores against itself on the keypoints (a net with
    # synthetic weights may put x2 left of x1: the boxes are put upright and the area kept positive)
    top = C.round2(results[:, :3].cpu().numpy().astype(np.float64))
    lo, hi = np.minimum(top[..., 0:2], top[..., 2:4]), np.maximum(top[..., 0:2], top[..., 2:4])
    boxes = np.concatenate([lo, hi - lo], -1)
    kps = np.concatenate([top[..., 5:39].reshape(4, 3, 17, 2), np.full((4, 3, 17, 1), 2.0)], -1)
    gt = C.GroundTruth(boxes, kps, boxes[..., 2] * boxes[..., 3] + 1.0, np.zeros((4, 3)), None, [3] * 4, 1)
    net = model.dla_net(HEADS, head_conv=64, dtype="f32")
    net.load_state_dict(sd)
    tr = trainer.HeadsTrainer(NS(task="multi_pose", lr=1e-4, K=20), net.to(DEV))
    loader = [{"input": x[i:i + 2], "meta": {"c": c[i:i + 2], "s": s[i:i + 2], "index": [i, i + 1]}} for i in (0, 2)]
    kp_stats, bb_stats = tr.val(loader, gt)
    kp, bb = C.evaluate(results, gt, "keypoints"), C.evaluate(results, gt, "bbox")
    print("val keypoints", kp_stats, "bbox", bb_stats)
    assert kp_stats.shape == (10,) and bb_stats.shape == (12,) and np.isfinite(kp_stats).all() and np.isfinite(bb_stats).all()
    assert np.array_equal(bits(kp_stats), bits(kp.stats)) and np.array_equal(bits(bb_stats), bits(bb.stats))
    assert kp_stats[0] > 0 and kp_stats[5] > 0 and bb_stats[0] >= 0 and set(tr.last_val) == {"keypoints", "bbox"}
    ref = C.evaluate_numpy(results.cpu().numpy(), gt, "bbox")
    assert np.array_equal(bits(bb.stats), bits(ref.stats))
