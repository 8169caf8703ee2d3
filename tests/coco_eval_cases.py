"""Synthetic evaluation cases shared by tests/test_oracle_coco_eval.py and tests/test_gpu_coco_eval.py: padded ground truth and float32
detections (jittered copies of ground truths and stray ones), small enough for the loop restatement."""
import numpy as np

from h3d_amd import coco_eval as C


def scene(seed, N, D, G, iou_type, K=1, equal_scores=False, min_side=6.0, max_side=320.0, full_dets=False, empty_gt_image=True, spread=400.0):
    """-> (results [N,D,39 | 6] float32, GroundTruth, det_num [N]).  One image holds exactly G ground truths (the others 0 .. G, one of
    them none when empty_gt_image), one exactly D detections (the others 0 .. D unless full_dets).  About one ground truth in seven has no
    labelled joint, one in ten is a crowd; sides are log-uniform so that all three area ranges are hit; corners are uniform in [0, spread)."""
    rs = np.random.RandomState(seed)
    kp = iou_type == "keypoints"
    W = 39 if kp else 6
    boxes, kps, area = np.zeros((N, G, 4)), np.zeros((N, G, 17, 3)), np.zeros((N, G))
    crowd, cls, num = np.zeros((N, G), np.uint8), np.zeros((N, G), np.int32), np.zeros(N, np.int32)
    res, det_num = np.zeros((N, D, W), np.float32), np.zeros(N, np.int32)
    for n in range(N):
        ng = G if n == 0 else (0 if n == 1 and empty_gt_image else rs.randint(0, G + 1))
        nd = D if n == 0 or full_dets else rs.randint(0, D + 1)
        num[n], det_num[n] = ng, nd
        for g in range(ng):
            w, h = np.exp(rs.uniform(np.log(min_side), np.log(max_side), 2))
            x, y = rs.uniform(0, spread, 2)
            boxes[n, g] = np.round([x, y, w, h], 2)
            area[n, g] = np.round(w * h * rs.uniform(0.4, 0.9), 3)
            crowd[n, g] = rs.rand() < 0.1
            cls[n, g] = rs.randint(K)
            if kp and rs.rand() > 1.0 / 7.0:
                v = rs.randint(0, 3, 17)
                v[rs.randint(17)] = 2
                xy = np.round(boxes[n, g, :2] + rs.uniform(0, 1, (17, 2)) * boxes[n, g, 2:], 0)
                kps[n, g] = np.concatenate([xy * (v[:, None] > 0), v[:, None]], 1)
        for d in range(nd):
            if ng and rs.rand() < 0.75:
                g = rs.randint(ng)
                b = boxes[n, g]
                j = rs.uniform(0, 0.25) * rs.uniform(-1, 1, 4) * np.array([b[2], b[3], b[2], b[3]])
                box = np.array([b[0], b[1], b[0] + b[2], b[1] + b[3]]) + j
                c = cls[n, g] if rs.rand() < 0.9 else rs.randint(K)
                base = np.where(kps[n, g, :, 2:3] > 0, kps[n, g, :, :2], b[:2] + rs.uniform(0, 1, (17, 2)) * b[2:])
                pts = base + rs.uniform(0, 0.08) * np.sqrt(area[n, g]) * rs.randn(17, 2)
            else:
                w, h = np.exp(rs.uniform(np.log(min_side), np.log(max_side), 2))
                x, y = rs.uniform(0, spread, 2)
                box, c = np.array([x, y, x + w, y + h]), rs.randint(K)
                pts = box[:2] + rs.uniform(0, 1, (17, 2)) * np.array([w, h])
            res[n, d, :4] = box
            res[n, d, 4] = 0.5 if equal_scores else rs.uniform(0.02, 1.0)
            if kp:
                res[n, d, 5:39] = pts.reshape(-1)
            else:
                res[n, d, 5] = c
    gt = C.GroundTruth(boxes, kps if kp else None, area, crowd, cls, num, K)
    return res, gt, det_num


def margins_hold(m, gt, tol=1e-9):
    """The condition under which an OKS matrix that differs in its last bits decides every match alike, on the mirror's matrix: no
    value of a (detection, ground truth) pair lies within tol of a threshold, and no two values of one detection that the walk can take
    (>= the lowest threshold - tol: anything smaller is passed over at every threshold) lie within tol of each other unless the two
    ground truths are identical (then so are the values, on any implementation)."""
    thr = np.minimum(C.IOU_THRS, 1 - 1e-10)
    for n in range(gt.N):
        nd, ng = int(m["det_num"][n]), int(gt.num[n])
        v = m["ious"][n, :nd, :ng]
        if v.size == 0:
            continue
        if np.abs(v[:, :, None] - thr[None, None]).min() <= tol:
            return False
        for d in range(nd):
            cand = np.nonzero(v[d] >= thr[0] - tol)[0]
            for i in cand:
                for j in cand:
                    if i < j and abs(v[d, i] - v[d, j]) <= tol:
                        same = (np.array_equal(gt.keypoints[n, i], gt.keypoints[n, j]) and np.array_equal(gt.boxes[n, i], gt.boxes[n, j])
                                and gt.area[n, i] == gt.area[n, j])
                        if not same:
                            return False
    return True
