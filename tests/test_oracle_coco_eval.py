"""CPU: coco_eval.evaluate_numpy (the vectorised host mirror of csrc/eval.hip) against the loop restatement of include/h3d.h section 8
(tests/coco_eval_ref.py: every maxDet matched on its own, envelope loop + searchsorted), and known answers that anchor both.

Both sides are numpy float64 and use the same exp, so everything is compared for equality: matches, ignore flags, ranks, rounded
scores, the IoU / OKS matrix, precision, recall, stats."""
import numpy as np
import pytest

import coco_eval_cases as cases
import coco_eval_ref as R
from h3d_amd import coco_eval as C


def both(res, gt, iou_type, det_cls=None, det_num=None, round2=True):
    got = C.evaluate_numpy(res, gt, iou_type, det_cls, det_num, round2)
    ref = R.evaluate_ref(res, gt, iou_type, det_cls, det_num, round2)
    m = got.extra["match"]
    assert np.array_equal(got.precision, ref["precision"]) and np.array_equal(got.recall, ref["recall"])
    assert np.array_equal(got.stats, ref["stats"])
    assert np.array_equal(m["gt_ignore"], ref["gt_ignore"])
    # the restatement only sees the detections the largest maxDet keeps (rank -1 beyond it); the mirror leaves those unmatched
    kept = ref["dt_rank"] >= 0
    assert np.array_equal(kept, (m["dt_rank"] >= 0) & (m["dt_rank"] < max(C.PARAMS[iou_type]["max_dets"])))
    assert np.array_equal(m["dt_rank"][kept], ref["dt_rank"][kept]) and np.array_equal(m["dt_score"][kept], ref["dt_score"][kept])
    assert np.array_equal(m["dt_match"], ref["dt_match"]) and np.array_equal(m["dt_ignore"], ref["dt_ignore"])
    # the restatement's matrix holds the pairs of one class; the mirror's holds every pair
    seen = ref["ious"] != 0
    assert np.array_equal(m["ious"][seen], ref["ious"][seen])
    return got, ref


@pytest.mark.parametrize("iou_type,N,D,G,K,kw", [
    ("keypoints", 5, 21, 9, 1, {}), ("keypoints", 3, 30, 4, 1, dict(equal_scores=True)), ("keypoints", 1, 1, 1, 1, {}),
    ("keypoints", 2, 0, 3, 1, {}), ("keypoints", 2, 5, 0, 1, {}),
    ("bbox", 5, 30, 9, 3, {}), ("bbox", 4, 12, 6, 1, dict(equal_scores=True)), ("bbox", 3, 25, 5, 2, dict(min_side=100.0)),
], ids=lambda v: str(v) if not isinstance(v, dict) else ",".join(v) or "-")
def test_mirror_equals_the_loop_restatement(iou_type, N, D, G, K, kw):
    for seed in (1, 2):
        res, gt, num = cases.scene(seed, N, D, G, iou_type, K, **kw)
        both(res, gt, iou_type, None, num)
    res, gt, num = cases.scene(3, N, D, G, iou_type, K, **kw)
    both(res, gt, iou_type, None, num, round2=False)


def grid_gt(N, per_image, K, kp, seed=0):
    """Ground truths 500 px apart (no overlap, OKS between two of them ~ 0), two-decimal coordinates, all labelled, no crowd; with K > 1
    an image holds at most one of a class."""
    rs = np.random.RandomState(seed)
    G = per_image
    boxes, kps, area = np.zeros((N, G, 4)), np.zeros((N, G, 17, 3)), np.zeros((N, G))
    cls = np.zeros((N, G), np.int32)
    for n in range(N):
        for g in range(G):
            w, h = np.round(np.exp(rs.uniform(np.log(10), np.log(200), 2)), 2)
            boxes[n, g] = [500.0 * g + 3.25, 7.5, w, h]
            area[n, g] = w * h
            cls[n, g] = g % K
            xy = np.round(boxes[n, g, :2] + rs.uniform(0, 1, (17, 2)) * boxes[n, g, 2:], 2)
            kps[n, g] = np.concatenate([xy, np.full((17, 1), 2.0)], 1)
    return C.GroundTruth(boxes, kps if kp else None, area, np.zeros((N, G)), cls, np.full(N, G), K)


def exact_detections(gt, kp, seed=0):
    rs = np.random.RandomState(seed)
    N, G = gt.N, gt.G
    res = np.zeros((N, G, 39 if kp else 6), np.float32)
    b = gt.boxes
    res[:, :, 0], res[:, :, 1], res[:, :, 2], res[:, :, 3] = b[..., 0], b[..., 1], b[..., 0] + b[..., 2], b[..., 1] + b[..., 3]
    res[:, :, 4] = (rs.permutation(N * G).reshape(N, G) + 1) / (N * G + 1.0)
    if kp:
        res[:, :, 5:] = gt.keypoints[..., :2].reshape(N, G, 34)
    else:
        res[:, :, 5] = gt.cls
    return res


@pytest.mark.parametrize("iou_type,K,per", [("keypoints", 1, 3), ("bbox", 3, 3)])
def test_a_every_ground_truth_detected_exactly(iou_type, K, per):
    kp = iou_type == "keypoints"
    gt = grid_gt(6, per, K, kp)
    got, _ = both(exact_detections(gt, kp), gt, iou_type, round2=False)
    rng = np.asarray(C.PARAMS[iou_type]["area_rng"])
    hit = 0
    for k in range(K):
        for a in range(len(rng)):
            npig = int(((gt.cls == k) & (gt.area >= rng[a, 0]) & (gt.area <= rng[a, 1])).sum())
            p, r = got.precision[:, :, k, a, :], got.recall[:, k, a, :]
            if npig:
                assert np.abs(p - 1).max() <= 1e-12 and np.array_equal(r, np.ones_like(r))
                hit += 1
            else:
                assert np.array_equal(p, -np.ones_like(p)) and np.array_equal(r, -np.ones_like(r))
    assert hit >= 2
    assert all(abs(s - 1) <= 1e-12 or s == -1 for s in got.stats) and abs(got.stats[0] - 1) <= 1e-12


def one_image(boxes_xywh, dets_xyxy_score, crowd=None, area=None):
    b = np.asarray(boxes_xywh, np.float64)[None]
    G = b.shape[1]
    gt = C.GroundTruth(b, None, b[..., 2] * b[..., 3] if area is None else np.asarray(area)[None], np.zeros((1, G)) if crowd is None else
                       np.asarray(crowd)[None], None, [G], 1)
    return np.asarray(dets_xyxy_score, np.float32)[None], gt


def test_b_hit_miss_hit():
    res, gt = one_image([[10, 10, 50, 50], [200, 10, 50, 50]], [[10, 10, 60, 60, .9], [400, 400, 450, 450, .8], [200, 10, 250, 60, .7]])
    got, _ = both(res, gt, "bbox")
    want = (51 + 50 * 2.0 / 3.0) / 101
    assert abs(got.stats[0] - want) <= 1e-12 and abs(got.stats[1] - want) <= 1e-12 and got.stats[8] == 1.0
    assert np.array_equal(got.extra["match"]["dt_match"][0, 0, :, :], np.tile([0, -1, 1], (10, 1)))


def test_c_the_last_of_two_identical_ground_truths_is_matched():
    res, gt = one_image([[10, 10, 50, 50], [10, 10, 50, 50]], [[10, 10, 60, 60, .9], [10, 10, 60, 60, .8]])
    got, _ = both(res, gt, "bbox")
    assert np.array_equal(got.extra["match"]["dt_match"][0, 0], np.tile([1, 0], (10, 1)))


def test_d_a_crowd_box_takes_two_detections():
    res, gt = one_image([[0, 0, 200, 200]], [[10, 10, 60, 60, .9], [100, 100, 180, 150, .8]], crowd=[1])
    got, _ = both(res, gt, "bbox")
    m = got.extra["match"]
    assert np.array_equal(m["dt_match"][0, 0], np.zeros((10, 2))) and np.array_equal(m["dt_ignore"][0, 0], np.ones((10, 2)))
    assert np.array_equal(m["ious"][0], [[1.0], [1.0]]) and np.all(got.precision == -1)


def test_e_a_detection_keeps_its_weaker_not_ignored_match():
    # ground truth 0 is a crowd the detection lies in (IoU 1), ground truth 1 overlaps it by 0.62
    res, gt = one_image([[0, 0, 200, 200], [0, 0, 100, 62]], [[0, 0, 100, 100, .9]], crowd=[1, 0])
    got, _ = both(res, gt, "bbox")
    m = got.extra["match"]
    assert m["ious"][0, 0, 0] == 1.0 and m["ious"][0, 0, 1] == 0.62
    assert m["dt_match"][0, 0, :, 0].tolist() == [1, 1, 1] + [0] * 7 and m["dt_ignore"][0, 0, :, 0].tolist() == [0, 0, 0] + [1] * 7
    assert got.recall[:, 0, 0, 2].tolist() == [1.0] * 3 + [0.0] * 7


def test_f_an_image_without_detections_counts_its_ground_truth():
    b = np.array([[[10, 10, 50, 50]], [[30, 30, 40, 40]]], np.float64)
    gt = C.GroundTruth(b, None, b[..., 2] * b[..., 3], np.zeros((2, 1)), None, [1, 1], 1)
    res = np.zeros((2, 1, 5), np.float32)
    res[0, 0] = [10, 10, 60, 60, .9]
    got, _ = both(res, gt, "bbox", det_num=[1, 0])
    assert np.array_equal(got.recall[:, 0, 0, :], np.full((10, 3), 0.5))
    assert abs(got.stats[0] - 51.0 / 101.0) <= 1e-12


def test_g_round2_is_the_two_decimal_formatting():
    rs = np.random.RandomState(0)
    v = np.concatenate([rs.uniform(-1000, 1000, 60000), rs.uniform(-1, 1, 20000), rs.uniform(0, 1e5, 20000)]).astype(np.float32)
    ties = np.concatenate([[0.125, 0.375], 0.125 + 0.25 * np.arange(-4000, 4000), (2.5e-3 * np.arange(0, 4000)).astype(np.float32)]).astype(np.float32)
    for a in (v, ties):
        got = C.round2(a.astype(np.float64))
        want = np.array([float("{:.2f}".format(x)) for x in a.astype(np.float64).tolist()])
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
        assert np.array_equal(got, [R.to_float(x) for x in a.tolist()])
    assert C.round2(0.125) == 0.12 and C.round2(0.375) == 0.38


def test_from_coco_summarize_and_json(tmp_path, capsys):
    ds = {"images": [{"id": 9}, {"id": 4}], "categories": [{"id": 1}],
          "annotations": [{"image_id": 9, "category_id": 1, "bbox": [10, 10, 50, 50], "area": 2000.0, "iscrowd": 0, "keypoints": [20, 20, 2] * 17, "num_keypoints": 17},
                          {"image_id": 4, "category_id": 1, "bbox": [5, 5, 20, 20], "area": 300.0, "iscrowd": 0, "keypoints": [0, 0, 0] * 17, "num_keypoints": 0}]}
    import json
    path = tmp_path / "ann.json"
    path.write_text(json.dumps(ds))
    gt = C.GroundTruth.from_coco(str(path))
    assert gt.image_ids == [4, 9] and gt.num.tolist() == [1, 1] and gt.boxes[1, 0].tolist() == [10, 10, 50, 50] and gt.num_classes == 1
    res = np.zeros((2, 1, 39), np.float32)
    res[1, 0, :5] = [10, 10, 60, 60, 0.987]
    res[1, 0, 5:] = 20.004
    got = C.evaluate_numpy(res, gt, "keypoints", det_num=[0, 1])
    lines = got.summarize()
    out = capsys.readouterr().out
    assert len(lines) == 10 and lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= 20 ] = 1.000" and lines[0] in out
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50      | area=   all | maxDets= 20 ] = 1.000"
    recs = C.to_coco_json(res, gt, "keypoints", det_num=[0, 1])
    assert recs == [{"image_id": 9, "category_id": 1, "bbox": [10.0, 10.0, 50.0, 50.0], "score": 0.99, "keypoints": [20.0, 20.0, 1.0] * 17}]
