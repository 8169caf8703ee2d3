"""numpy restatement of the training targets (h3d_amd/targets.py, csrc/targets.hip): COCOHP._get_label (datasets/coco_hp.py:215-309) and
the ctdet label block of COCO.__getitem__ (datasets/coco.py:203-248), vectorised over the objects of an image, with the reference's
number types at every step.  No reference import: tests/test_oracle_targets.py pins it to the reference's own output
(tests/golden/targets_ref.npz, tools/gen_targets_golden.py); the GPU tests use it for the cases they generate.

Per image: multi_pose_image(...) / ctdet_image(...) -> {name: array} with the device's names and shapes (gt_det padded to max_objs rows,
gt_count beside it); multi_pose_batch / ctdet_batch stack them."""
import numpy as np

F32, F64 = np.float32, np.float64
FLIP_IDX = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
HM_ROT = F32(0.9999)


def affine(t, xy):
    """float64 2x3 times float32 [x, y, 1], rounded to float32 once: xy [n,2] -> [n,2]."""
    x, y = xy[:, 0].astype(F64), xy[:, 1].astype(F64)
    t = np.asarray(t, F64).reshape(2, 3)
    return np.stack([t[0, 0] * x + t[0, 1] * y + t[0, 2], t[1, 0] * x + t[1, 1] * y + t[1, 2]], axis=1).astype(F32)


def box_path(boxes, t, flipped, width, out_w, out_h):
    """xywh -> xyxy, the mirror, trans_output, the clip: -> bbox [n,4], h [n], w [n], all float32."""
    b = np.asarray(boxes, F32)
    xyxy = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], axis=1)
    if flipped:
        x0 = F32(width) - xyxy[:, 2] - F32(1)
        x1 = F32(width) - xyxy[:, 0] - F32(1)
        xyxy[:, 0], xyxy[:, 2] = x0, x1
    bb = np.concatenate([affine(t, xyxy[:, :2]), affine(t, xyxy[:, 2:])], axis=1)
    bb[:, [0, 2]] = np.clip(bb[:, [0, 2]], 0, out_w - 1)
    bb[:, [1, 3]] = np.clip(bb[:, [1, 3]], 0, out_h - 1)
    return bb, bb[:, 3] - bb[:, 1], bb[:, 2] - bb[:, 0]


def gaussian_radius(h, w, min_overlap=0.7):
    """max(0, int(gaussian_radius((ceil(h), ceil(w))))) of utils/image.py:97-117 in float64, in its operation order; -> (int radius,
    the float64 value in front of the truncation)."""
    mo = min_overlap
    height, width = np.ceil(np.asarray(h, F64)), np.ceil(np.asarray(w, F64))
    b1 = height + width
    c1 = width * height * (1 - mo) / (1 + mo)
    r1 = (b1 + np.sqrt(b1 * b1 - 4 * c1)) / 2
    b2 = 2 * (height + width)
    c2 = (1 - mo) * width * height
    r2 = (b2 + np.sqrt(b2 * b2 - 16 * c2)) / 2
    a3 = 4 * mo
    b3 = -2 * mo * (height + width)
    c3 = (mo - 1) * width * height
    r3 = (b3 + np.sqrt(b3 * b3 - 4 * a3 * c3)) / 2
    r = np.minimum(np.minimum(r1, r2), r3)
    return np.maximum(0, np.trunc(r)).astype(np.int64), r


def splat(hm, x, y, r):
    """draw_umich_gaussian (utils/image.py:128-143) without the eps * max threshold, which never changes a value."""
    H, W = hm.shape
    x, y, r = int(x), int(y), int(r)
    x0, x1, y0, y1 = max(x - r, 0), min(x + r + 1, W), max(y - r, 0), min(y + r + 1, H)
    if x1 <= x0 or y1 <= y0:
        return
    sigma = (2 * r + 1) / 6
    dy, dx = np.ogrid[y0 - y:y1 - y, x0 - x:x1 - x]
    g = np.exp(-(dx * dx + dy * dy).astype(F64) / (2 * sigma * sigma))
    np.maximum(hm[y0:y1, x0:x1], g.astype(F32), out=hm[y0:y1, x0:x1])


def multi_pose_image(boxes, keypoints, num, trans, rot_flag=False, flipped=False, width=0, flip_idx=FLIP_IDX, out_h=128, out_w=128, max_objs=32,
                     detail=None):
    """boxes [M,4], keypoints [M,J,3], trans [2,6] float64 (trans_output, trans_output_rot).  `detail`, a dict, receives the values that
    feed a truncation, a ceil, a comparison or a gate (the golden generator's margin check)."""
    boxes, keypoints = np.asarray(boxes, F32).reshape(-1, 4), np.asarray(keypoints, F32)
    J, N = keypoints.shape[1], max_objs
    n = max(0, min(int(num), N, boxes.shape[0]))
    t = np.asarray(trans, F64).reshape(2, 6)
    out = {"hm": np.zeros((1, out_h, out_w), F32), "hm_hp": np.zeros((J, out_h, out_w), F32), "wh": np.zeros((N, 2), F32),
           "reg": np.zeros((N, 2), F32), "ind": np.zeros(N, np.int64), "reg_mask": np.zeros(N, np.uint8), "hps": np.zeros((N, 2 * J), F32),
           "hps_mask": np.zeros((N, 2 * J), np.uint8), "hp_offset": np.zeros((N * J, 2), F32), "hp_ind": np.zeros(N * J, np.int64),
           "hp_mask": np.zeros(N * J, np.int64), "gt_det": np.zeros((N, 6 + 2 * J), F32), "gt_count": np.int32(0)}
    bb, h, w = box_path(boxes[:n], t[0], flipped, width, out_w, out_h)
    live = ((h > 0) & (w > 0)) | bool(rot_flag)
    radius, r_real = gaussian_radius(h, w)
    ct = np.stack([(bb[:, 0] + bb[:, 2]) / F32(2), (bb[:, 1] + bb[:, 3]) / F32(2)], axis=1).astype(F32)
    ct_int = ct.astype(np.int32)
    pts = keypoints[:n].copy()
    if flipped:
        pts[:, :, 0] = F32(width) - pts[:, :, 0] - F32(1)
        for a, b in flip_idx:
            pts[:, [a, b]] = pts[:, [b, a]]
    vis = (pts[:, :, 2] > 0) & live[:, None]
    moved = affine(t[1], pts[:, :, :2].reshape(-1, 2)).reshape(n, J, 2)
    xy = np.where(vis[:, :, None], moved, pts[:, :, :2])            # what gt_det keeps: transformed where visible (and live)
    inside = vis & (xy[:, :, 0] >= 0) & (xy[:, :, 0] < out_w) & (xy[:, :, 1] >= 0) & (xy[:, :, 1] < out_h)
    pt_int = np.where(inside[:, :, None], xy, 0).astype(np.int32)
    k = np.flatnonzero(live)
    out["wh"][k] = np.stack([w, h], axis=1)[k]
    out["ind"][k] = ct_int[k, 1].astype(np.int64) * out_w + ct_int[k, 0]
    out["reg"][k] = (ct[k].astype(F64) - ct_int[k]).astype(F32)
    out["reg_mask"][k] = (pts[k, :, 2].sum(axis=1) != 0) & (not rot_flag)
    rel = np.where(inside[:, :, None], xy.astype(F64) - ct_int[:, None, :], 0).astype(F32)
    off = np.where(inside[:, :, None], xy.astype(F64) - pt_int, 0).astype(F32)
    out["hps"][:n] = rel.reshape(n, 2 * J)
    out["hps_mask"][:n] = np.repeat(inside & (not rot_flag), 2, axis=1)
    out["hp_offset"][:n * J] = off.reshape(n * J, 2)
    out["hp_ind"][:n * J] = np.where(inside, pt_int[:, :, 1].astype(np.int64) * out_w + pt_int[:, :, 0], 0).reshape(-1)
    out["hp_mask"][:n * J] = inside.reshape(-1)
    for i in k:
        for j in np.flatnonzero(inside[i]):
            splat(out["hm_hp"][j], pt_int[i, j, 0], pt_int[i, j, 1], radius[i])
        splat(out["hm"][0], ct_int[i, 0], ct_int[i, 1], radius[i])
    if rot_flag:
        out["hm"][:] = HM_ROT
    out["gt_count"] = np.int32(len(k))
    out["gt_det"][:len(k)] = np.concatenate([bb[k], np.ones((len(k), 1), F32), xy[k].reshape(len(k), 2 * J), np.zeros((len(k), 1), F32)], axis=1)
    if detail is not None:
        detail.update(h=h, w=w, bb=bb, live=live, r_real=r_real, ct=ct, pts=moved[vis])
    return out


def ctdet_image(boxes, cls, num, trans, flipped=False, width=0, out_h=128, out_w=128, num_classes=80, max_objs=128, detail=None):
    boxes, cls = np.asarray(boxes, F32).reshape(-1, 4), np.asarray(cls, np.int64).reshape(-1)
    C, N = num_classes, max_objs
    n = max(0, min(int(num), N, boxes.shape[0]))
    t = np.asarray(trans, F64).reshape(2, 6)
    out = {"hm": np.zeros((C, out_h, out_w), F32), "wh": np.zeros((N, 2), F32), "reg": np.zeros((N, 2), F32), "ind": np.zeros(N, np.int64),
           "reg_mask": np.zeros(N, np.uint8), "cat_spec_wh": np.zeros((N, 2 * C), F32), "cat_spec_mask": np.zeros((N, 2 * C), np.uint8),
           "gt_det": np.zeros((N, 6), F32), "gt_count": np.int32(0)}
    bb, h, w = box_path(boxes[:n], t[0], flipped, width, out_w, out_h)
    c = cls[:n]
    live = (h > 0) & (w > 0) & (c >= 0) & (c < C)
    radius, r_real = gaussian_radius(h, w)
    ct = np.stack([(bb[:, 0] + bb[:, 2]) / F32(2), (bb[:, 1] + bb[:, 3]) / F32(2)], axis=1).astype(F32)
    ct_int = ct.astype(np.int32)
    k = np.flatnonzero(live)
    out["wh"][k] = np.stack([w, h], axis=1)[k]
    out["ind"][k] = ct_int[k, 1].astype(np.int64) * out_w + ct_int[k, 0]
    out["reg"][k] = (ct[k].astype(F64) - ct_int[k]).astype(F32)
    out["reg_mask"][k] = 1
    for i in k:
        out["cat_spec_wh"][i, 2 * c[i]:2 * c[i] + 2] = out["wh"][i]
        out["cat_spec_mask"][i, 2 * c[i]:2 * c[i] + 2] = 1
        splat(out["hm"][c[i]], ct_int[i, 0], ct_int[i, 1], radius[i])
    hw, hh = w[k] / F32(2), h[k] / F32(2)
    out["gt_count"] = np.int32(len(k))
    out["gt_det"][:len(k)] = np.stack([ct[k, 0] - hw, ct[k, 1] - hh, ct[k, 0] + hw, ct[k, 1] + hh, np.ones(len(k), F32), c[k].astype(F32)], axis=1)
    if detail is not None:
        detail.update(h=h, w=w, bb=bb, live=live, r_real=r_real, ct=ct)
    return out


def _stack(items):
    return {k: np.stack([it[k] for it in items]) for k in items[0]}


def _per_image(x, b, default):
    return default if x is None else x[b]


def multi_pose_batch(boxes, keypoints, num, trans, rot_flag=None, flipped=None, width=None, **kw):
    return _stack([multi_pose_image(boxes[b], keypoints[b], num[b], trans[b], bool(_per_image(rot_flag, b, 0)), bool(_per_image(flipped, b, 0)),
                                    int(_per_image(width, b, 0)), **kw) for b in range(len(boxes))])


def ctdet_batch(boxes, cls, num, trans, flipped=None, width=None, **kw):
    return _stack([ctdet_image(boxes[b], cls[b], num[b], trans[b], bool(_per_image(flipped, b, 0)), int(_per_image(width, b, 0)), **kw)
                   for b in range(len(boxes))])


# ---- seeded scenes (shared by the golden generator, the CPU and the GPU tests) ----------------------------------------------------
def scene(seed, n, M=None, J=17, img_w=640, img_h=480, min_size=8.0, max_size=220.0, vis_p=0.7, quarter=True):
    """n annotations of an img_w x img_h image in M rows: boxes xywh and keypoints inside (and a little around) their box, every value a
    multiple of 1/4 (float32-exact, as the reference sums xywh in float64 first).  -> boxes [M,4] f32, keypoints [M,J,3] f32."""
    rs = np.random.RandomState(seed)
    M = n if M is None else M
    boxes, kps = np.zeros((M, 4), F32), np.zeros((M, J, 3), F32)
    q = (lambda a: np.round(a * 4) / 4) if quarter else (lambda a: a)
    for k in range(n):
        w, h = rs.uniform(min_size, max_size), rs.uniform(min_size, max_size)
        x, y = rs.uniform(-0.1 * img_w, img_w - 0.5 * w), rs.uniform(-0.1 * img_h, img_h - 0.5 * h)
        boxes[k] = q(np.array([x, y, w, h]))
        kps[k, :, 0] = q(rs.uniform(x - 0.1 * w, x + 1.1 * w, J))
        kps[k, :, 1] = q(rs.uniform(y - 0.1 * h, y + 1.1 * h, J))
        kps[k, :, 2] = (rs.uniform(size=J) < vis_p) * rs.randint(1, 3, J)
    return boxes, kps


def margins(detail, out_w, out_h):
    """The smallest distance of a value that feeds a truncation, a ceil, a comparison or a gate from its threshold: the integers, for
    h, w (ceil, and the gate at 0), the radius and the centre (truncation: no threshold inside (-1, 1)) and the transformed keypoints (the
    [0, res) gate and the truncation).  An axis whose two edges both sit on a clip bound is exact in every implementation and is left out."""
    def to_int(a, zero_ok=False):
        a = np.asarray(a, F64).reshape(-1)
        d = np.abs(a - np.round(a))
        if zero_ok:
            d = d[np.abs(a) >= 0.5]
        return d.min() if d.size else np.inf
    bb, live = detail["bb"], detail["live"]
    free_x = ~(np.isin(bb[:, 0], (0, out_w - 1)) & np.isin(bb[:, 2], (0, out_w - 1)))
    free_y = ~(np.isin(bb[:, 1], (0, out_h - 1)) & np.isin(bb[:, 3], (0, out_h - 1)))
    m = min(to_int(detail["w"][free_x]), to_int(detail["h"][free_y]), to_int(detail["r_real"][live], True),
            to_int(detail["ct"][live & free_x, 0], True), to_int(detail["ct"][live & free_y, 1], True))
    if "pts" in detail:
        m = min(m, to_int(detail["pts"]))
    return float(m)
