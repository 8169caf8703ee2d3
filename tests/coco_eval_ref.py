"""A literal restatement of COCO's evaluation (include/h3d.h section 8) with Python loops, independent of h3d_amd/coco_eval.py: records ->
per (image, class, area range, maxDet) greedy matching -> per (class, area range, maxDet) accumulate -> summary.  No shortcut: every
maxDet is matched on its own, and precision comes from the right-to-left envelope loop and searchsorted, as COCOeval writes it.

    evaluate_ref(results, gt, iou_type, det_cls=None, det_num=None, round2=True) -> dict(precision, recall, stats, and, for the largest
    maxDet, ious / dt_match / dt_ignore / gt_ignore / dt_score / dt_rank in the layout of coco_eval.match)

`gt` is anything with boxes [N,G,4], keypoints [N,G,17,3], area, iscrowd, cls [N,G], num [N] and num_classes."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, 10)
REC_THRS = np.linspace(.0, 1.00, 101)
SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
ALL, SMALL, MEDIUM, LARGE = [0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]
SETUP = {"keypoints": ([20], [ALL, MEDIUM, LARGE], ["all", "medium", "large"]),
         "bbox": ([1, 10, 100], [ALL, SMALL, MEDIUM, LARGE], ["all", "small", "medium", "large"])}


def to_float(v):
    """The export rounding as section 8 defines it (= float("{:.2f}".format(v)) on a widened float32)."""
    return float(np.rint(float(v) * 100.0)) / 100.0


def box_iou(d, g, crowd):
    iw = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    ih = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = iw * ih
    union = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - inter
    return inter / union


def oks(dt, gt):
    vars_ = (SIGMAS * 2) ** 2
    g = gt["keypoints"]
    xg, yg, vg = g[0::3], g[1::3], g[2::3]
    k1 = sum(1 for v in vg if v > 0)
    bb = gt["bbox"]
    x0, x1, y0, y1 = bb[0] - bb[2], bb[0] + bb[2] * 2, bb[1] - bb[3], bb[1] + bb[3] * 2
    d = dt["keypoints"]
    xd, yd = d[0::3], d[1::3]
    total, n = 0.0, 0
    for j in range(17):
        if k1 > 0:
            dx, dy = xd[j] - xg[j], yd[j] - yg[j]
        else:
            dx = max(0.0, x0 - xd[j]) + max(0.0, xd[j] - x1)
            dy = max(0.0, y0 - yd[j]) + max(0.0, yd[j] - y1)
        e = (dx * dx + dy * dy) / vars_[j] / (gt["area"] + np.spacing(1)) / 2
        if k1 > 0 and not vg[j] > 0:
            continue
        total = total + float(np.exp(-e))
        n += 1
    return total / n


def records(results, gt, iou_type, det_cls, det_num, round2):
    """-> (dts, gts): per image, per class, lists of dicts in input order."""
    N, D = results.shape[:2]
    K = gt.num_classes
    r2 = to_float if round2 else float
    dts = [[[] for _ in range(K)] for _ in range(N)]
    gts = [[[] for _ in range(K)] for _ in range(N)]
    for n in range(N):
        nd = D if det_num is None else int(det_num[n])
        for d in range(nd):
            row = [float(v) for v in results[n, d]]
            k = 0 if det_cls is None else int(det_cls[n, d])
            bbox = [r2(row[0]), r2(row[1]), r2(row[2] - row[0]), r2(row[3] - row[1])]
            rec = {"idx": d, "bbox": bbox, "score": r2(row[4]), "area": bbox[2] * bbox[3]}
            if iou_type == "keypoints":
                kp = []
                for j in range(17):
                    kp += [r2(row[5 + 2 * j]), r2(row[6 + 2 * j]), 1.0]
                rec["keypoints"] = kp
            if 0 <= k < K:
                dts[n][k].append(rec)
        for g in range(int(gt.num[n])):
            kp = [float(v) for v in np.asarray(gt.keypoints[n, g]).reshape(-1)]
            crowd = bool(gt.iscrowd[n, g])
            ignore = crowd or (iou_type == "keypoints" and sum(1 for v in kp[2::3] if v > 0) == 0)
            gts[n][int(gt.cls[n, g])].append({"idx": g, "bbox": [float(v) for v in gt.boxes[n, g]], "area": float(gt.area[n, g]), "iscrowd": crowd,
                                              "keypoints": kp, "ignore": ignore})
    return dts, gts


def evaluate_img(dt, gt, iou_type, rng, max_det):
    """COCOeval.evaluateImg for one (image, class): None without ground truth and detections."""
    if not gt and not dt:
        return None
    for g in gt:
        g["_ignore"] = bool(g["ignore"] or g["area"] < rng[0] or g["area"] > rng[1])
    gtind = sorted(range(len(gt)), key=lambda i: gt[i]["_ignore"])                 # stable
    gt = [gt[i] for i in gtind]
    dtind = sorted(range(len(dt)), key=lambda i: -dt[i]["score"])                  # stable
    dt = [dt[i] for i in dtind[:max_det]]
    T, G, Dn = len(IOU_THRS), len(gt), len(dt)
    ious = [[(oks(d, g) if iou_type == "keypoints" else box_iou(d["bbox"], g["bbox"], g["iscrowd"])) for g in gt] for d in dt]
    gtm = [[0] * G for _ in range(T)]
    dtm = [[0] * Dn for _ in range(T)]
    dtig = [[False] * Dn for _ in range(T)]
    gtig = [g["_ignore"] for g in gt]
    for tind, t in enumerate(IOU_THRS):
        for dind in range(Dn):
            iou = min(t, 1 - 1e-10)
            m = -1
            for gind in range(G):
                if gtm[tind][gind] > 0 and not gt[gind]["iscrowd"]:
                    continue
                if m > -1 and not gtig[m] and gtig[gind]:
                    break
                if ious[dind][gind] < iou:
                    continue
                iou = ious[dind][gind]
                m = gind
            if m == -1:
                continue
            dtig[tind][dind] = gtig[m]
            dtm[tind][dind] = gt[m]["idx"] + 1
            gtm[tind][m] = dt[dind]["idx"] + 1
    for tind in range(T):
        for dind in range(Dn):
            outside = dt[dind]["area"] < rng[0] or dt[dind]["area"] > rng[1]
            dtig[tind][dind] = dtig[tind][dind] or (dtm[tind][dind] == 0 and outside)
    return {"dt": dt, "gt": gt, "ious": ious, "dtm": dtm, "dtig": dtig, "gtig": gtig, "scores": [d["score"] for d in dt]}


def evaluate_ref(results, gt, iou_type, det_cls=None, det_num=None, round2=True):
    results = np.asarray(results, np.float32)
    max_dets, rngs, labels = SETUP[iou_type]
    if det_cls is None and iou_type == "bbox" and results.shape[2] == 6:
        det_cls = results[:, :, 5].astype(np.int64)
    N, D = results.shape[:2]
    G, K, A, M, T, R = gt.boxes.shape[1], gt.num_classes, len(rngs), len(max_dets), len(IOU_THRS), len(REC_THRS)
    dts, gts = records(results, gt, iou_type, det_cls, det_num, round2)
    imgs = {(k, a, mi, n): evaluate_img(dts[n][k], gts[n][k], iou_type, rngs[a], max_dets[mi])
            for k in range(K) for a in range(A) for mi in range(M) for n in range(N)}
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            for mi, md in enumerate(max_dets):
                E = [imgs[k, a, mi, n] for n in range(N)]
                E = [e for e in E if e is not None]
                if not E:
                    continue
                scores = np.array([s for e in E for s in e["scores"][:md]], np.float64)
                inds = np.argsort(-scores, kind="mergesort")
                dtm = np.array([[v for e in E for v in e["dtm"][t][:md]] for t in range(T)]).reshape(T, -1)[:, inds]
                dtig = np.array([[v for e in E for v in e["dtig"][t][:md]] for t in range(T)], bool).reshape(T, -1)[:, inds]
                gtig = np.array([v for e in E for v in e["gtig"]], bool)
                npig = int(np.count_nonzero(~gtig))
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
                tp_sum = np.cumsum(tps, axis=1).astype(np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros(R).tolist()
                    recall[t, k, a, mi] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    at = np.searchsorted(rc, REC_THRS, side="left")
                    try:
                        for ri, pi in enumerate(at):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, mi] = np.array(q)
    out = {"precision": precision, "recall": recall, "stats": summarize(precision, recall, iou_type)}
    # the per-image results of the largest maxDet, in the layout of coco_eval.match
    mi = M - 1
    out.update(ious=np.zeros((N, D, G)), dt_match=np.full((N, A, T, D), -1, np.int32), dt_ignore=np.zeros((N, A, T, D), np.uint8),
               gt_ignore=np.zeros((N, A, G), np.uint8), dt_score=np.zeros((N, D)), dt_rank=np.full((N, D), -1, np.int32))
    for (k, a, m_, n), e in imgs.items():
        if m_ != mi or e is None:
            continue
        for gi, g in enumerate(e["gt"]):
            out["gt_ignore"][n, a, g["idx"]] = e["gtig"][gi]
        for di, d in enumerate(e["dt"]):
            out["dt_score"][n, d["idx"]], out["dt_rank"][n, d["idx"]] = d["score"], di
            for gi, g in enumerate(e["gt"]):
                out["ious"][n, d["idx"], g["idx"]] = e["ious"][di][gi]
            for t in range(T):
                out["dt_match"][n, a, t, d["idx"]] = e["dtm"][t][di] - 1
                out["dt_ignore"][n, a, t, d["idx"]] = e["dtig"][t][di]
    return out


def summarize(precision, recall, iou_type):
    max_dets, _, labels = SETUP[iou_type]

    def one(ap, iou_thr, area, max_det):
        a, m = labels.index(area), max_dets.index(max_det)
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    if iou_type == "keypoints":
        sel = [(1, None, "all"), (1, .5, "all"), (1, .75, "all"), (1, None, "medium"), (1, None, "large"),
               (0, None, "all"), (0, .5, "all"), (0, .75, "all"), (0, None, "medium"), (0, None, "large")]
        return np.array([one(ap, thr, area, 20) for ap, thr, area in sel])
    sel = [(1, None, "all", 100), (1, .5, "all", 100), (1, .75, "all", 100), (1, None, "small", 100), (1, None, "medium", 100),
           (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10), (0, None, "all", 100), (0, None, "small", 100),
           (0, None, "medium", 100), (0, None, "large", 100)]
    return np.array([one(*s) for s in sel])
