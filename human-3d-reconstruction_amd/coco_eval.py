"""COCO keypoint (OKS) and box AP on the device: what the reference's val() gets from pycocotools' COCOeval (datasets/coco_hp.py:92-138,
datasets/coco.py:126-135), computed from the device tensors the detectors produce (csrc/eval.hip, include/h3d.h section 8, DESIGN.md
section 25).  pycocotools is not a dependency: include/h3d.h section 8 is the written definition, tests/coco_eval_ref.py restates it with
loops, `evaluate_numpy` is the vectorised host mirror, and the kernels are bit-equal to both except for the OKS matrix (exp).

    GroundTruth(...) / GroundTruth.from_coco(dict_or_path)        the padded per-image ground truth, ascending image id
    evaluate(results, gt, iou_type, det_cls, det_num, round2)     -> EvalResult(precision, recall, stats); .summarize() prints COCOeval's lines
    match(...) / accumulate(...)                                  the two raw steps: one launch, two sorts + two launches
    evaluate_numpy(...), match_numpy(...), accumulate_numpy(...)  the host mirror
    CocoEvaluator(gt, iou_type).update(image_index, results) / .compute()
    to_coco_json(results, gt, iou_type)                           the reference's result records

`results` is [N,K,39] as detector.multi_pose_post_process returns it (box x1 y1 x2 y2, score, 17 (x, y)), or [N,K,6] for ctdet (box,
score, class; [N,K,5] with det_cls).  round2 applies the reference's export rounding float("{:.2f}".format(v)).  Nothing is synchronised
with the host before the final precision / recall tensors are read for the summary."""
import json

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
KP_VARS = (SIGMAS * 2) ** 2
EPS = float(np.spacing(1))                      # 2^-52
PARAMS = {
    "keypoints": dict(max_dets=[20], area_lbl=["all", "medium", "large"], area_rng=[[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]),
    "bbox": dict(max_dets=[1, 10, 100], area_lbl=["all", "small", "medium", "large"],
                 area_rng=[[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]),
}
# (ap, iouThr index or None, area label, maxDet) per line of COCOeval.summarize
SUMMARY = {
    "keypoints": [(1, None, "all", 20), (1, 0, "all", 20), (1, 5, "all", 20), (1, None, "medium", 20), (1, None, "large", 20),
                  (0, None, "all", 20), (0, 0, "all", 20), (0, 5, "all", 20), (0, None, "medium", 20), (0, None, "large", 20)],
    "bbox": [(1, None, "all", 100), (1, 0, "all", 100), (1, 5, "all", 100), (1, None, "small", 100), (1, None, "medium", 100),
             (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10), (0, None, "all", 100), (0, None, "small", 100),
             (0, None, "medium", 100), (0, None, "large", 100)],
}


def _params(iou_type):
    if iou_type not in PARAMS:
        raise ValueError("coco_eval: iou_type %r (keypoints | bbox)" % (iou_type,))
    p = PARAMS[iou_type]
    return np.asarray(p["area_rng"], np.float64), np.asarray(p["max_dets"], np.int32)


def round2(v):
    """float("{:.2f}".format(v)) for finite |v| < 2^20, on float64 arrays."""
    return np.rint(np.asarray(v, np.float64) * 100.0) / 100.0


class GroundTruth:
    """boxes [N,G,4] (x, y, w, h), keypoints [N,G,17,3] or None, area [N,G], iscrowd [N,G], cls [N,G] (0 .. num_classes-1), num [N]:
    numpy, float64 / uint8 / int32, images in ascending image id (COCOeval's np.unique(imgIds))."""

    def __init__(self, boxes, keypoints, area, iscrowd, cls, num, num_classes=1, image_ids=None, cat_ids=None):
        self.boxes = np.ascontiguousarray(boxes, np.float64)
        N, G = self.boxes.shape[:2]
        self.keypoints = np.zeros((N, G, 17, 3)) if keypoints is None else np.ascontiguousarray(keypoints, np.float64).reshape(N, G, 17, 3)
        self.area = np.ascontiguousarray(area, np.float64).reshape(N, G)
        self.iscrowd = np.ascontiguousarray(np.asarray(iscrowd) != 0, np.uint8).reshape(N, G)
        self.cls = (np.zeros((N, G), np.int32) if cls is None else np.ascontiguousarray(cls, np.int32)).reshape(N, G)
        self.num = np.ascontiguousarray(num, np.int32).reshape(N)
        if self.boxes.shape != (N, G, 4) or (N and (self.num.min() < 0 or self.num.max() > G)):
            raise ValueError("GroundTruth: boxes %s, num in [%s, %s]" % (self.boxes.shape, self.num.min(), self.num.max()))
        self.N, self.G, self.num_classes = N, G, int(num_classes)
        self.image_ids = list(range(N)) if image_ids is None else [int(i) for i in image_ids]
        self.cat_ids = list(range(1, self.num_classes + 1)) if cat_ids is None else [int(c) for c in cat_ids]
        self._dev = {}

    @classmethod
    def from_coco(cls, dict_or_path, cat_ids=None, image_ids=None):
        """A COCO annotation dict (or the path of its json): images in ascending id, an image's annotations in file order, the classes
        the ascending category ids (cat_ids: only these; image_ids: only these images)."""
        ds = dict_or_path
        if not isinstance(ds, dict):
            with open(ds) as f:
                ds = json.load(f)
        cats = sorted({int(c["id"]) for c in ds.get("categories", [])} or {int(a["category_id"]) for a in ds["annotations"]})
        if cat_ids is not None:
            cats = sorted(int(c) for c in cat_ids)
        imgs = sorted({int(i["id"]) for i in ds["images"]} if image_ids is None else {int(i) for i in image_ids})
        at, kc = {i: n for n, i in enumerate(imgs)}, {c: k for k, c in enumerate(cats)}
        per = [[] for _ in imgs]
        for a in ds["annotations"]:
            if int(a["image_id"]) in at and int(a["category_id"]) in kc:
                per[at[int(a["image_id"])]].append(a)
        N, G = len(imgs), max([len(p) for p in per] + [0])
        boxes, kps, area = np.zeros((N, G, 4)), np.zeros((N, G, 17, 3)), np.zeros((N, G))
        crowd, kls, num = np.zeros((N, G), np.uint8), np.zeros((N, G), np.int32), np.zeros(N, np.int32)
        for n, p in enumerate(per):
            num[n] = len(p)
            for g, a in enumerate(p):
                boxes[n, g] = a["bbox"]
                area[n, g] = a["area"] if "area" in a else a["bbox"][2] * a["bbox"][3]
                crowd[n, g] = int(a.get("iscrowd", 0)) != 0
                kls[n, g] = kc[int(a["category_id"])]
                if "keypoints" in a:
                    kps[n, g] = np.asarray(a["keypoints"], np.float64).reshape(17, 3)
        return cls(boxes, kps, area, crowd, kls, num, len(cats), imgs, cats)

    def subset(self, n):
        """The first n images."""
        return GroundTruth(self.boxes[:n], self.keypoints[:n], self.area[:n], self.iscrowd[:n], self.cls[:n], self.num[:n], self.num_classes,
                           self.image_ids[:n], self.cat_ids)

    def select(self, index):
        """The images at the positions `index`, in that order (mesh_eval.MeshEvaluator matches one batch at a time)."""
        i = np.asarray(index, np.int64).reshape(-1)
        return GroundTruth(self.boxes[i], self.keypoints[i], self.area[i], self.iscrowd[i], self.cls[i], self.num[i], self.num_classes,
                           [self.image_ids[k] for k in i], self.cat_ids)

    def to(self, device):
        """The device tensors (made once per device)."""
        import torch
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = {k: torch.from_numpy(getattr(self, k)).to(device) for k in ("boxes", "keypoints", "area", "iscrowd", "cls", "num")}
        return self._dev[device]


class EvalResult:
    """precision [T,R,K,A,M], recall [T,K,A,M] (numpy float64, -1 = no ground truth in the cell), stats = COCOeval's summary vector."""

    def __init__(self, iou_type, precision, recall, extra=None):
        self.iou_type, self.precision, self.recall = iou_type, precision, recall
        self.stats = summarize_stats(precision, recall, iou_type)
        self.extra = extra or {}

    def summarize(self, file=None):
        lines = []
        for (ap, thr, lbl, md), s in zip(SUMMARY[self.iou_type], self.stats):
            iou = "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1]) if thr is None else "{:0.2f}".format(IOU_THRS[thr])
            lines.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
                "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, lbl, md, s))
        for ln in lines:
            print(ln, file=file)
        return lines


def summarize_stats(precision, recall, iou_type):
    """COCOeval._summarize over the twelve (bbox) or ten (keypoints) selections: the mean of the entries > -1, -1 if there are none."""
    p = PARAMS[iou_type]
    out = []
    for ap, thr, lbl, md in SUMMARY[iou_type]:
        a, m = p["area_lbl"].index(lbl), p["max_dets"].index(md)
        s = precision[:, :, :, a, m] if ap else recall[:, :, a, m]
        if thr is not None:
            s = s[thr:thr + 1]
        sel = s[s > -1]
        out.append(-1.0 if sel.size == 0 else float(np.mean(sel)))
    return np.asarray(out, np.float64)


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------------------
def _host_inputs(results, gt, iou_type, det_cls, det_num):
    res = np.ascontiguousarray(results, np.float32)
    if res.ndim != 3 or res.shape[0] != gt.N or res.shape[2] < (39 if iou_type == "keypoints" else 5):
        raise ValueError("coco_eval: results %s for %d images and iou_type %r" % (res.shape, gt.N, iou_type))
    N, D = res.shape[:2]
    if det_cls is None:
        det_cls = res[:, :, 5].astype(np.int32) if iou_type == "bbox" and res.shape[2] == 6 else np.zeros((N, D), np.int32)
    det_num = np.full(N, D, np.int32) if det_num is None else np.clip(np.asarray(det_num, np.int32), 0, D)
    return res, np.ascontiguousarray(det_cls, np.int32).reshape(N, D), det_num


def _box_iou(d, g, crowd):
    """d [nd,4], g [ng,4] xywh, crowd [ng] -> [nd,ng]."""
    iw = np.minimum(d[:, None, 0] + d[:, None, 2], g[None, :, 0] + g[None, :, 2]) - np.maximum(d[:, None, 0], g[None, :, 0])
    ih = np.minimum(d[:, None, 1] + d[:, None, 3], g[None, :, 1] + g[None, :, 3]) - np.maximum(d[:, None, 1], g[None, :, 1])
    inter = iw * ih
    da, ga = (d[:, 2] * d[:, 3])[:, None], (g[:, 2] * g[:, 3])[None]
    union = np.where(crowd[None], da, da + ga - inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = inter / union
    return np.where((iw <= 0) | (ih <= 0), 0.0, v)


def _oks(dk, gk, gb, garea):
    """dk [nd,34], gk [ng,17,3], gb [ng,4], garea [ng] -> [nd,ng]: the sum runs in joint order."""
    vis = gk[:, :, 2] > 0
    k1 = vis.sum(1)
    den = garea + EPS
    x0, x1, y0, y1 = gb[:, 0] - gb[:, 2], gb[:, 0] + gb[:, 2] * 2, gb[:, 1] - gb[:, 3], gb[:, 1] + gb[:, 3] * 2
    s = np.zeros((dk.shape[0], gk.shape[0]))
    for j in range(17):
        xd, yd = dk[:, None, 2 * j], dk[:, None, 2 * j + 1]
        dx = np.where(k1[None] > 0, xd - gk[None, :, j, 0], np.maximum(0.0, x0[None] - xd) + np.maximum(0.0, xd - x1[None]))
        dy = np.where(k1[None] > 0, yd - gk[None, :, j, 1], np.maximum(0.0, y0[None] - yd) + np.maximum(0.0, yd - y1[None]))
        e = (dx * dx + dy * dy) / KP_VARS[j] / den[None] / 2
        s = s + np.where((k1[None] == 0) | vis[None, :, j], np.exp(-e), 0.0)
    return s / np.where(k1 > 0, k1, 17)[None]


def match_numpy(results, gt, iou_type, det_cls=None, det_num=None, round2_=True):
    """The mirror of `match`: the same dict on the host (numpy)."""
    rng, max_dets = _params(iou_type)
    res, det_cls, det_num = _host_inputs(results, gt, iou_type, det_cls, det_num)
    kp = iou_type == "keypoints"
    N, D, G, A, T = gt.N, res.shape[1], gt.G, len(rng), len(IOU_THRS)
    maxdet = int(max_dets.max())
    out = dict(ious=np.zeros((N, D, G)), dt_match=np.full((N, A, T, D), -1, np.int32), dt_ignore=np.zeros((N, A, T, D), np.uint8),
               gt_ignore=np.zeros((N, A, G), np.uint8), dt_score=np.zeros((N, D)), dt_rank=np.full((N, D), -1, np.int32),
               dt_box=np.zeros((N, D, 4)), dt_area=np.zeros((N, D)), dt_keypoints=np.zeros((N, D, 34)) if kp else None,
               det_cls=det_cls, det_num=det_num, iou_type=iou_type)
    thr = np.minimum(IOU_THRS, 1 - 1e-10)
    ar = np.arange(A)
    for n in range(N):
        nd, ng = int(det_num[n]), int(gt.num[n])
        r = res[n, :nd].astype(np.float64)
        box = np.stack([r[:, 0], r[:, 1], r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]], 1) if nd else np.zeros((0, 4))
        sc, dk = r[:, 4], r[:, 5:39]
        if round2_:
            box, sc, dk = round2(box), round2(sc), round2(dk)
        area = box[:, 2] * box[:, 3]
        out["dt_box"][n, :nd], out["dt_score"][n, :nd], out["dt_area"][n, :nd] = box, sc, area
        if kp:
            out["dt_keypoints"][n, :nd] = dk
        dcls = det_cls[n, :nd]
        order = np.argsort(-sc, kind="mergesort")
        crank = np.zeros(nd, np.int64)
        for c in np.unique(dcls):
            idx = np.nonzero(dcls == c)[0]
            crank[idx[np.argsort(-sc[idx], kind="mergesort")]] = np.arange(len(idx))
        out["dt_rank"][n, :nd] = crank
        gb, garea, crowd, gcls = gt.boxes[n, :ng], gt.area[n, :ng], gt.iscrowd[n, :ng] != 0, gt.cls[n, :ng]
        base = crowd | ((gt.keypoints[n, :ng, :, 2] > 0).sum(1) == 0) if kp else crowd
        gig = base[None] | (garea[None] < rng[:, :1]) | (garea[None] > rng[:, 1:])               # [A,ng]
        out["gt_ignore"][n, :, :ng] = gig
        if nd and ng:
            out["ious"][n, :nd, :ng] = _oks(dk, gt.keypoints[n, :ng], gb, garea) if kp else _box_iou(box, gb, crowd)
        mat = out["ious"][n]
        gorder = np.stack([np.argsort(gig[a], kind="mergesort") for a in range(A)]) if ng else np.zeros((A, 0), np.int64)
        nvalid = (~gig).sum(1)
        matched = np.zeros((A, T, max(ng, 1)), bool)
        for d in order:
            if crank[d] >= maxdet:
                continue
            best = np.broadcast_to(thr[None], (A, T)).copy()
            m = np.full((A, T), -1, np.int64)
            mig = np.zeros((A, T), bool)
            stopped = np.zeros((A, T), bool)
            for q in range(ng):
                g = gorder[:, q]
                g_ig = (q >= nvalid)[:, None]
                active = ~stopped & (gcls[g] == dcls[d])[:, None] & ~(matched[ar, :, g] & ~crowd[g][:, None])
                brk = active & (m >= 0) & ~mig & g_ig
                stopped |= brk
                v = mat[d, g][:, None]
                upd = active & ~brk & ~(v < best)
                best, m, mig = np.where(upd, v, best), np.where(upd, g[:, None], m), np.where(upd, g_ig, mig)
            hit = m >= 0
            outside = ((area[d] < rng[:, 0]) | (area[d] > rng[:, 1]))[:, None]
            out["dt_match"][n, :, :, d] = m
            out["dt_ignore"][n, :, :, d] = np.where(hit, mig, outside)
            ai, ti = np.nonzero(hit)
            matched[ai, ti, m[hit]] = True
    return out


def accumulate_numpy(m, gt, iou_type=None):
    """The mirror of `accumulate`: (precision [T,R,K,A,M], recall [T,K,A,M])."""
    iou_type = iou_type or m["iou_type"]
    rng, max_dets = _params(iou_type)
    N, A, T, D = m["dt_match"].shape
    K, M, R = gt.num_classes, len(max_dets), len(REC_THRS)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    rank = m["dt_rank"].reshape(-1)
    score = np.where(rank >= 0, m["dt_score"].reshape(-1), -np.inf)
    order = np.argsort(-score, kind="stable")
    cls = m["det_cls"].reshape(-1)
    valid = np.arange(gt.G)[None] < gt.num[:, None]
    matched = np.moveaxis(m["dt_match"], 3, 1).reshape(N * D, A, T) >= 0
    ignored = np.moveaxis(m["dt_ignore"], 3, 1).reshape(N * D, A, T) != 0
    for k in range(K):
        sel = order[(cls[order] == k) & (rank[order] >= 0)]
        for a in range(A):
            npig = int((valid & (gt.cls == k) & (m["gt_ignore"][:, a] == 0)).sum())
            if npig == 0:
                continue
            for mi, md in enumerate(max_dets):
                keep = sel[rank[sel] < md]
                mt, ig = matched[keep, a], ignored[keep, a]                              # [L,T]
                tp = np.cumsum(mt & ~ig, 0).astype(np.float64)
                fp = np.cumsum(~mt & ~ig, 0).astype(np.float64)
                rc = tp / npig
                pr = tp / (fp + tp + EPS)
                L = len(keep)
                recall[:, k, a, mi] = rc[-1] if L else 0.0
                for t in range(T):
                    q = np.zeros(R)
                    if L:
                        env = np.maximum.accumulate(pr[::-1, t])[::-1]
                        at = np.searchsorted(rc[:, t], REC_THRS, side="left")
                        ok = at < L
                        q[ok] = env[at[ok]]
                    precision[t, :, k, a, mi] = q
    return precision, recall


def evaluate_numpy(results, gt, iou_type, det_cls=None, det_num=None, round2=True):
    """The host mirror of `evaluate` (numpy; results on the host): the same precision, recall and stats, bit for bit but for what the
    device's exp moves in the OKS matrix.  .extra['match'] holds match_numpy's dict."""
    m = match_numpy(results, gt, iou_type, det_cls, det_num, round2)
    precision, recall = accumulate_numpy(m, gt, iou_type)
    return EvalResult(iou_type, precision, recall, {"match": m})


# ---- the device path ---------------------------------------------------------------------------------------------------------------------------
_CONST = {}


def _constants(dev, iou_type):
    import torch
    key = (dev, iou_type)
    if key not in _CONST:
        rng, _ = _params(iou_type)
        _CONST[key] = tuple(torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev) for a in (rng, IOU_THRS, KP_VARS, REC_THRS))
    return _CONST[key]


def match(results, gt, iou_type, det_cls=None, det_num=None, round2=True, want_ious=True):
    """results [N,D,39] (keypoints) or [N,D,6] / [N,D,5] (bbox) float32 on the device, det_cls [N,D], det_num [N] (None = all D) -> dict of
    device tensors: ious [N,D,G] (None with want_ious=False), dt_match / dt_ignore [N,A,T,D], gt_ignore [N,A,G], dt_score, dt_rank,
    dt_area [N,D], dt_box [N,D,4], dt_keypoints [N,D,34] (include/h3d.h section 8).  One launch."""
    import ctypes
    import torch
    from . import _lib
    what = "coco_eval.match"
    rng, max_dets = _params(iou_type)
    kp = iou_type == "keypoints"
    _lib.require_cuda(results, det_cls, det_num)
    if results.dim() != 3 or results.shape[0] != gt.N or results.dtype != torch.float32 or results.shape[2] < (39 if kp else 5):
        raise RuntimeError("%s: results must be float32 [%d,D,%s], got %s %s" % (what, gt.N, "39" if kp else "5+", results.dtype, tuple(results.shape)))
    dev = results.device
    results = results.detach().contiguous()
    N, D, W = results.shape
    G, A, T = gt.G, len(rng), len(IOU_THRS)
    if det_cls is None and not kp and W == 6:
        det_cls = results[:, :, 5].to(torch.int32)
    if det_cls is not None:
        det_cls = det_cls.detach().to(device=dev, dtype=torch.int32).contiguous()
        if tuple(det_cls.shape) != (N, D):
            raise RuntimeError("%s: det_cls must be [%d,%d], got %s" % (what, N, D, tuple(det_cls.shape)))
    if det_num is not None:
        det_num = torch.as_tensor(det_num).detach().to(device=dev, dtype=torch.int32).contiguous()
        if tuple(det_num.shape) != (N,):
            raise RuntimeError("%s: det_num must be [%d], got %s" % (what, N, tuple(det_num.shape)))
    g = gt.to(dev)
    d_rng, d_thr, d_vars, _ = _constants(dev, iou_type)
    f64, i32, u8 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev), dict(dtype=torch.uint8, device=dev)
    L = _lib.lib()
    # the size query checks the limits before anything is allocated; with the public matrix asked for, the walk reads that
    nbytes = ctypes.c_size_t(0)
    _lib.check(L.h3d_coco_match_workspace_bytes(N, D, G, ctypes.byref(nbytes)), "h3d_coco_match_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev) if nbytes.value and not want_ious else None
    out = dict(ious=torch.empty(N, D, G, **f64) if want_ious else None, dt_match=torch.empty(N, A, T, D, **i32),
               dt_ignore=torch.empty(N, A, T, D, **u8), gt_ignore=torch.empty(N, A, G, **u8), dt_score=torch.empty(N, D, **f64),
               dt_rank=torch.empty(N, D, **i32), dt_box=torch.empty(N, D, 4, **f64), dt_area=torch.empty(N, D, **f64),
               dt_keypoints=torch.empty(N, D, 34, **f64) if kp else None, det_cls=det_cls, det_num=det_num, iou_type=iou_type)
    with torch.cuda.device(dev):
        _lib.check(L.h3d_coco_match(
            _lib.ptr(results), W, _lib.ptr(det_cls), _lib.ptr(det_num), _lib.ptr(g["boxes"]), _lib.ptr(g["keypoints"] if kp else None),
            _lib.ptr(g["area"]), _lib.ptr(g["iscrowd"]), _lib.ptr(g["cls"]), _lib.ptr(g["num"]), N, D, G,
            _lib.COCO_KEYPOINTS if kp else _lib.COCO_BBOX, _lib.COCO_ROUND2 if round2 else 0, int(max_dets.max()), _lib.ptr(d_rng), A,
            _lib.ptr(d_thr), T, _lib.ptr(d_vars), _lib.ptr(out["ious"]), _lib.ptr(out["dt_match"]), _lib.ptr(out["dt_ignore"]),
            _lib.ptr(out["gt_ignore"]), _lib.ptr(out["dt_score"]), _lib.ptr(out["dt_rank"]), _lib.ptr(out["dt_box"]), _lib.ptr(out["dt_area"]),
            _lib.ptr(out["dt_keypoints"]), _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream_ptr()), "h3d_coco_match")
    return out


def sort_detections(m, num_classes):
    """match's dict -> (order [N D] int64, seg_start [K+1] int32) on the device: every detection slot by class, inside a class by rounded
    score descending, stable (two stable torch sorts); slots without a detection or outside the classes come last."""
    import torch
    rank = m["dt_rank"].reshape(-1)
    dev = rank.device
    cls = torch.zeros_like(rank) if m["det_cls"] is None else m["det_cls"].reshape(-1)
    cls = torch.where((rank < 0) | (cls < 0) | (cls >= num_classes), torch.full_like(cls, num_classes), cls).to(torch.int64)
    score = torch.where(rank >= 0, m["dt_score"].reshape(-1), torch.full((), -float("inf"), dtype=torch.float64, device=dev))
    o1 = torch.sort(score, descending=True, stable=True)[1]
    o2 = torch.sort(cls[o1], stable=True)[1]
    seg = torch.zeros(num_classes + 2, dtype=torch.int64, device=dev)
    seg[1:] = torch.cumsum(torch.bincount(cls, minlength=num_classes + 1), 0)
    return o1[o2].contiguous(), seg[:num_classes + 1].to(torch.int32).contiguous()


def accumulate(m, gt, iou_type=None):
    """match's dict -> (precision [T,R,K,A,M], recall [T,K,A,M]) float64 on the device: two sorts and two launches."""
    import ctypes
    import torch
    from . import _lib
    iou_type = iou_type or m["iou_type"]
    rng, max_dets = _params(iou_type)
    N, A, T, D = m["dt_match"].shape
    dev = m["dt_match"].device
    K, M, R, G = gt.num_classes, len(max_dets), len(REC_THRS), gt.G
    g = gt.to(dev)
    L = _lib.lib()
    ws = _lib.workspace(L.h3d_coco_accumulate_workspace_bytes, K, A, device=dev)
    order, seg = sort_detections(m, K)
    precision = torch.empty(T, R, K, A, M, dtype=torch.float64, device=dev)
    recall = torch.empty(T, K, A, M, dtype=torch.float64, device=dev)
    md = (ctypes.c_int32 * M)(*[int(v) for v in max_dets])
    with torch.cuda.device(dev):
        _lib.check(L.h3d_coco_accumulate(
            _lib.ptr(order), _lib.ptr(seg), _lib.ptr(m["dt_rank"]), _lib.ptr(m["dt_match"]), _lib.ptr(m["dt_ignore"]), _lib.ptr(m["gt_ignore"]),
            _lib.ptr(g["cls"]), _lib.ptr(g["num"]), N, D, G, K, A, T, md, M, _lib.ptr(_constants(dev, iou_type)[3]), R, _lib.ptr(precision),
            _lib.ptr(recall), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "h3d_coco_accumulate")
    return precision, recall


def evaluate(results, gt, iou_type, det_cls=None, det_num=None, round2=True, keep_match=False):
    """-> EvalResult: precision, recall (numpy, read back once at the end) and COCOeval's stats; .summarize() prints its lines.
    keep_match: .extra['match'] holds match's dict, the matrix included."""
    m = match(results, gt, iou_type, det_cls, det_num, round2, want_ious=keep_match)
    precision, recall = accumulate(m, gt, iou_type)
    return EvalResult(iou_type, precision.cpu().numpy(), recall.cpu().numpy(), {"match": m} if keep_match else None)


class CocoEvaluator:
    """Collects a validation run batch by batch: update(image_index, results, det_cls, det_num) keeps the batch's records on the device
    (image_index: the images' positions in `gt`), compute() evaluates what was seen; an image never updated has no detections."""

    def __init__(self, gt, iou_type, round2=True):
        _params(iou_type)
        self.gt, self.iou_type, self.round2 = gt, iou_type, round2
        self.reset()

    def reset(self):
        self._batches = []

    def update(self, image_index, results, det_cls=None, det_num=None):
        import torch
        idx = torch.as_tensor(image_index, dtype=torch.int64).reshape(-1).to(results.device)
        if results.dim() != 3 or results.shape[0] != idx.numel():
            raise RuntimeError("CocoEvaluator.update: results %s for %d images" % (tuple(results.shape), idx.numel()))
        self._batches.append((idx, results.detach().float().clone(), None if det_cls is None else det_cls.detach().clone(),
                              None if det_num is None else torch.as_tensor(det_num).detach().clone()))

    def compute(self, iou_type=None, keep_match=False):
        """-> EvalResult of what was seen so far (iou_type: evaluate the same records as another type, 'bbox' after 'keypoints')."""
        import torch
        iou_type = iou_type or self.iou_type
        if not self._batches:
            raise RuntimeError("CocoEvaluator.compute: no update() yet")
        dev = self._batches[0][1].device
        N, D, W = self.gt.N, max(b[1].shape[1] for b in self._batches), self._batches[0][1].shape[2]
        res = torch.zeros(N, D, W, dtype=torch.float32, device=dev)
        num = torch.zeros(N, dtype=torch.int32, device=dev)
        cls = torch.zeros(N, D, dtype=torch.int32, device=dev) if any(b[2] is not None for b in self._batches) else None
        for idx, r, c, k in self._batches:
            res[idx, :r.shape[1]] = r
            num[idx] = r.shape[1] if k is None else k.to(device=dev, dtype=torch.int32)
            if c is not None:
                cls[idx, :r.shape[1]] = c.to(device=dev, dtype=torch.int32)
            elif cls is not None and iou_type == "bbox" and W == 6:
                cls[idx, :r.shape[1]] = r[:, :, 5].to(torch.int32)
        return evaluate(res, self.gt, iou_type, cls, num, self.round2, keep_match)


def to_coco_json(results, gt, iou_type="keypoints", det_cls=None, det_num=None):
    """The reference's result records (convert_eval_format): a list of dicts with image_id, category_id, bbox (x, y, w, h), score and,
    for keypoints, the 51 keypoint values (v = 1), every number rounded to two decimals."""
    res, det_cls, det_num = _host_inputs(np.asarray(results.detach().cpu() if hasattr(results, "detach") else results), gt, iou_type,
                                         None if det_cls is None else np.asarray(det_cls.cpu() if hasattr(det_cls, "cpu") else det_cls),
                                         None if det_num is None else np.asarray(det_num.cpu() if hasattr(det_num, "cpu") else det_num))
    out = []
    for n in range(gt.N):
        for d in range(int(det_num[n])):
            r = res[n, d].astype(np.float64)
            rec = {"image_id": gt.image_ids[n], "category_id": gt.cat_ids[int(det_cls[n, d])],
                   "bbox": [float(v) for v in round2([r[0], r[1], r[2] - r[0], r[3] - r[1]])], "score": float(round2(r[4]))}
            if iou_type == "keypoints":
                rec["keypoints"] = [float(v) for v in np.concatenate([round2(r[5:39]).reshape(17, 2), np.ones((17, 1))], 1).reshape(-1)]
            out.append(rec)
    return out
