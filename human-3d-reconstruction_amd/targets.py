"""Training targets on the device: the label half of the reference's dataset items -- COCOHP._get_label + _get_dataset
(datasets/coco_hp.py:215-362) and the ctdet block of COCO.__getitem__ (datasets/coco.py:203-266) -- for a whole batch, computed by
libh3d_hip.so (csrc/targets.hip, include/h3d.h section 6) in two launches.

    get_affine_transform(center, scale, rot, output_size)      utils/image.py:27-62 with the 3-point solve written out (no cv2)
    target_transforms(c, s, rot, out_w, out_h)                 -> [B,2,6] float64: trans_output, trans_output_rot per image
    multi_pose_targets(boxes, keypoints, num, c, s, ...)       -> the dict _get_dataset returns (batched, minus 'input') + meta.gt_det
    ctdet_targets(boxes, cls, num, c, s, ...)                  -> the dict COCO.__getitem__ returns (batched, minus 'input')

The dicts feed h3d_amd.losses.loss_multi_pose / loss_obj_detection unchanged.  Out of scope (ValueError here, H3D_ERR_UNSUPPORTED from the
ABI): mse_loss (draw_msra_gaussian), dense_hp and dense_wh (draw_dense_reg depends on the object order).  c, s, rot, flipped are inputs
here: the train branch of _get_input that draws them and builds 'input' (random crop, colour augmentation) is h3d_amd/train_input.py,
whose multi_pose_train_batch / ctdet_train_batch return these dicts with 'input'."""

import numpy as np
import torch

from . import _lib

MSE_LOSS, DENSE_HP, DENSE_WH = 1, 2, 4             # H3D_TARGETS_*
COCO_FLIP_IDX = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]          # coco_hp.py:39-40
POSE_OUTPUTS = ("hm", "hm_hp", "wh", "reg", "ind", "reg_mask", "hps", "hps_mask", "hp_offset", "hp_ind", "hp_mask", "gt_det", "gt_count")
CTDET_OUTPUTS = ("hm", "wh", "reg", "ind", "reg_mask", "cat_spec_wh", "cat_spec_mask", "gt_det", "gt_count")


def _solve3(src, dst):
    """The 2x3 matrix that maps three points onto three points (what cv2.getAffineTransform returns): Cramer's rule in float64."""
    (x0, y0), (x1, y1), (x2, y2) = np.asarray(src, np.float64)
    det = x0 * (y1 - y2) - y0 * (x1 - x2) + (x1 * y2 - x2 * y1)
    rows = []
    for u0, u1, u2 in np.asarray(dst, np.float64).T:
        rows.append([(u0 * (y1 - y2) - y0 * (u1 - u2) + (u1 * y2 - u2 * y1)) / det,
                     (x0 * (u1 - u2) - u0 * (x1 - x2) + (x1 * u2 - x2 * u1)) / det,
                     (x0 * (y1 * u2 - y2 * u1) - y0 * (x1 * u2 - x2 * u1) + u0 * (x1 * y2 - x2 * y1)) / det])
    return np.array(rows, np.float64)


def get_affine_transform(center, scale, rot, output_size, shift=(0.0, 0.0), inv=0):
    """utils/image.py:27-62: the crop transform through three point pairs (centre, the point half a source width above it turned by
    `rot` degrees, and the third corner of the right angle), the points held in float32 as the reference holds them, solved in float64.
    `center` is taken as float32, as the datasets build it."""
    center = np.asarray(center, np.float32)
    scale = np.asarray(scale) if isinstance(scale, (np.ndarray, list, tuple)) else np.array([scale, scale], np.float32)
    shift = np.asarray(shift, np.float32)
    dst_w, dst_h = output_size[0], output_size[1]
    rad = np.pi * rot / 180
    sn, cs = np.sin(rad), np.cos(rad)
    up = np.float64(scale[0]) * -0.5                               # the source direction [0, -src_w / 2] ...
    src_dir = np.array([0.0 * cs - up * sn, 0.0 * sn + up * cs], np.float64)     # ... turned by rot, in float64
    moved = scale * shift
    src, dst = np.zeros((3, 2), np.float32), np.zeros((3, 2), np.float32)
    src[0] = center + moved
    src[1] = center.astype(np.float64) + src_dir + moved
    dst[0] = [dst_w * 0.5, dst_h * 0.5]
    dst[1] = dst[0] + np.array([0, dst_w * -0.5], np.float32)
    for p in (src, dst):
        d = p[0] - p[1]
        p[2] = p[1] + np.array([-d[1], d[0]], np.float32)
    return _solve3(dst, src) if inv else _solve3(src, dst)


def target_transforms(c, s, rot, out_w, out_h):
    """[B,2,6] float64 (CPU): per image trans_output = get_affine_transform(c, s, 0, [out_w, out_h]) and trans_output_rot = the same
    with the image's rot (coco_hp.py:223-224), row-major 2x3 each.  s: [B] or [B,2]; rot: [B] or None."""
    c = np.asarray(c, np.float32).reshape(-1, 2)
    B = c.shape[0]
    s = np.asarray(s)
    rot = np.zeros(B) if rot is None else np.asarray(rot, np.float64).reshape(B)
    out = np.empty((B, 2, 6), np.float64)
    for b in range(B):
        sb = s[b] if s.ndim == 2 else float(s.reshape(B)[b])
        out[b, 0] = get_affine_transform(c[b], sb, 0, [out_w, out_h]).reshape(6)
        out[b, 1] = out[b, 0] if rot[b] == 0 else get_affine_transform(c[b], sb, float(rot[b]), [out_w, out_h]).reshape(6)
    return torch.from_numpy(out)


def _dev(x, dtype, device):
    if x is None:
        return None
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.detach().to(device=device, dtype=dtype).contiguous()


def _workspace(B, max_objs, J, device):
    return _lib.workspace(_lib.lib().h3d_targets_workspace_bytes, B, max_objs, J, device=device, min_bytes=16)


def pose_output_specs(B, max_objs, J, H, W):
    """name -> (shape, dtype) of every output of h3d_multi_pose_targets."""
    N = max_objs
    return {"hm": ((B, 1, H, W), torch.float32), "hm_hp": ((B, J, H, W), torch.float32), "wh": ((B, N, 2), torch.float32),
            "reg": ((B, N, 2), torch.float32), "ind": ((B, N), torch.int64), "reg_mask": ((B, N), torch.uint8),
            "hps": ((B, N, 2 * J), torch.float32), "hps_mask": ((B, N, 2 * J), torch.uint8), "hp_offset": ((B, N * J, 2), torch.float32),
            "hp_ind": ((B, N * J), torch.int64), "hp_mask": ((B, N * J), torch.int64), "gt_det": ((B, N, 6 + 2 * J), torch.float32),
            "gt_count": ((B,), torch.int32)}


def ctdet_output_specs(B, max_objs, C, H, W):
    N = max_objs
    return {"hm": ((B, C, H, W), torch.float32), "wh": ((B, N, 2), torch.float32), "reg": ((B, N, 2), torch.float32),
            "ind": ((B, N), torch.int64), "reg_mask": ((B, N), torch.uint8), "cat_spec_wh": ((B, N, 2 * C), torch.float32),
            "cat_spec_mask": ((B, N, 2 * C), torch.uint8), "gt_det": ((B, N, 6), torch.float32), "gt_count": ((B,), torch.int32)}


def _outputs(specs, want, out, device):
    """The output tensors of a call: those handed in through `out` (checked), else torch.empty for the names in `want`."""
    res = {}
    for name, (shape, dtype) in specs.items():
        t = None if out is None else out.get(name)
        if out is None and name in want:
            t = torch.empty(shape, dtype=dtype, device=device)
        if t is not None:
            _lib.require_cuda(t)
            if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous():
                raise RuntimeError("targets: output %s must be contiguous %s of %s, got %s of %s" % (name, shape, dtype, tuple(t.shape), t.dtype))
            res[name] = t
    return res


def multi_pose_targets_raw(boxes, keypoints, num, trans, rot_flag, flipped, width, flip_pairs, Hout, Wout, max_objs, want=POSE_OUTPUTS,
                           out=None, options=0):
    """One h3d_multi_pose_targets call on device tensors: boxes [B,M,4] f32, keypoints [B,M,J,3] f32, num [B] i32, trans [B,2,6] f64,
    rot_flag / flipped / width [B] i32 or None, flip_pairs [n,2] i32 or None.  Returns {name: tensor} for the names in `want` (freshly
    allocated), or exactly the tensors of `out` (name -> tensor, a missing name = NULL = not written)."""
    _lib.require_cuda(boxes, keypoints, num, trans, rot_flag, flipped, width, flip_pairs)
    B, M = boxes.shape[:2]
    J = keypoints.shape[2]
    dev = boxes.device
    o = _outputs(pose_output_specs(B, max_objs, J, Hout, Wout), want, out, dev)
    ws = _workspace(B, max_objs, J, dev) if ("hm" in o or "hm_hp" in o) else None
    p = _lib.ptr
    with torch.cuda.device(dev):
        rc = _lib.lib().h3d_multi_pose_targets(
            p(boxes), p(keypoints), p(num), p(trans), p(rot_flag), p(flipped), p(width), p(flip_pairs),
            0 if flip_pairs is None else flip_pairs.shape[0], B, M, J, Hout, Wout, max_objs,
            p(o.get("hm")), p(o.get("hm_hp")), p(o.get("wh")), p(o.get("reg")), p(o.get("ind")), p(o.get("reg_mask")), p(o.get("hps")),
            p(o.get("hps_mask")), p(o.get("hp_offset")), p(o.get("hp_ind")), p(o.get("hp_mask")), p(o.get("gt_det")), p(o.get("gt_count")),
            options, p(ws), 0 if ws is None else ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "h3d_multi_pose_targets")
    return o


def ctdet_targets_raw(boxes, cls, num, trans, flipped, width, Hout, Wout, num_classes, max_objs, want=CTDET_OUTPUTS, out=None, options=0):
    """One h3d_ctdet_targets call on device tensors (cls [B,M] i32; the rest as multi_pose_targets_raw)."""
    _lib.require_cuda(boxes, cls, num, trans, flipped, width)
    B, M = boxes.shape[:2]
    dev = boxes.device
    o = _outputs(ctdet_output_specs(B, max_objs, num_classes, Hout, Wout), want, out, dev)
    ws = _workspace(B, max_objs, 0, dev) if "hm" in o else None
    p = _lib.ptr
    with torch.cuda.device(dev):
        rc = _lib.lib().h3d_ctdet_targets(
            p(boxes), p(cls), p(num), p(trans), p(flipped), p(width), B, M, Hout, Wout, num_classes, max_objs,
            p(o.get("hm")), p(o.get("wh")), p(o.get("reg")), p(o.get("ind")), p(o.get("reg_mask")), p(o.get("cat_spec_wh")),
            p(o.get("cat_spec_mask")), p(o.get("gt_det")), p(o.get("gt_count")), options, p(ws), 0 if ws is None else ws.numel(),
            _lib.stream_ptr())
    _lib.check(rc, "h3d_ctdet_targets")
    return o


def _opt(opt, name, default):
    return getattr(opt, name, default)


def _refuse(opt, names):
    for name in names:
        if _opt(opt, name, False):
            raise ValueError("targets: opt.%s is out of scope (draw_msra_gaussian / draw_dense_reg are not built)" % name)


def _common(boxes, num, c, s, rot, flipped, width, out_w, out_h, device):
    device = torch.device("cuda" if device is None else device)
    boxes = _dev(boxes, torch.float32, device)
    if boxes.dim() != 3 or boxes.shape[2] != 4:
        raise RuntimeError("targets: boxes must be [B,M,4] (COCO xywh), got %s" % (tuple(boxes.shape),))
    B = boxes.shape[0]
    num = _dev(num, torch.int32, device).reshape(B)
    c_np = np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c, np.float32).reshape(B, 2)
    s_np = np.asarray(s.cpu() if isinstance(s, torch.Tensor) else s)
    rot_np = None if rot is None else np.asarray(rot.cpu() if isinstance(rot, torch.Tensor) else rot, np.float64).reshape(B)
    trans = target_transforms(c_np, s_np, rot_np, out_w, out_h).to(device)
    rot_flag = None if rot_np is None else torch.from_numpy((rot_np != 0).astype(np.int32)).to(device)
    flipped = None if flipped is None else _dev(np.asarray(flipped.cpu() if isinstance(flipped, torch.Tensor) else flipped).astype(np.int32),
                                                torch.int32, device).reshape(B)
    if flipped is not None and width is None:
        raise ValueError("targets: `width` (the image widths the mirror uses) is needed with `flipped`")
    width = None if width is None else _dev(width, torch.int32, device).reshape(B)
    return device, boxes, num, trans, rot_flag, flipped, width, c_np, s_np


def multi_pose_targets(boxes, keypoints, num, c, s, rot=None, flipped=None, width=None, opt=None, device=None):
    """COCOHP._get_label + _get_dataset for a batch: boxes [B,M,4] (COCO xywh), keypoints [B,M,J,3] (x, y, v), num [B] annotations per
    image (above opt.max_objs = 32: clamped), c [B,2] / s [B] the crop of _get_input, rot [B] degrees, flipped [B], width [B] image widths
    (needed with flipped).  opt: output_res (or output_h / output_w), max_objs, flip_idx, reg_offset, hm_hp, reg_hp_offset.
    -> {'hm', 'reg_mask', 'ind', 'wh', 'hps', 'hps_mask'[, 'reg'][, 'hm_hp'][, 'hp_offset', 'hp_ind', 'hp_mask'], 'meta'} on the device;
    meta = {'c', 's', 'gt_det' [B,max_objs,40] (rows past gt_count are zero), 'gt_count' [B]}."""
    _refuse(opt, ("mse_loss", "dense_hp"))
    res = _opt(opt, "output_res", None)
    H, W = (res, res) if res else (_opt(opt, "output_h", 128), _opt(opt, "output_w", 128))
    device, boxes, num, trans, rot_flag, flipped, width, c_np, s_np = _common(boxes, num, c, s, rot, flipped, width, W, H, device)
    keypoints = _dev(keypoints, torch.float32, device)
    if keypoints.dim() == 3:
        keypoints = keypoints.reshape(keypoints.shape[0], keypoints.shape[1], -1, 3)
    if keypoints.dim() != 4 or keypoints.shape[:2] != boxes.shape[:2] or keypoints.shape[3] != 3:
        raise RuntimeError("targets: keypoints must be [B,M,J,3] beside boxes [B,M,4], got %s" % (tuple(keypoints.shape),))
    pairs = _opt(opt, "flip_idx", COCO_FLIP_IDX)
    flip_pairs = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(device) if (flipped is not None and len(pairs)) else None
    want = ["hm", "reg_mask", "ind", "wh", "hps", "hps_mask", "gt_det", "gt_count"]
    want += ["reg"] if _opt(opt, "reg_offset", True) else []
    want += ["hm_hp"] if _opt(opt, "hm_hp", True) else []
    want += ["hp_offset", "hp_ind", "hp_mask"] if _opt(opt, "reg_hp_offset", True) else []
    o = multi_pose_targets_raw(boxes, keypoints, num, trans, rot_flag, flipped, width, flip_pairs, H, W, _opt(opt, "max_objs", 32), want)
    o["meta"] = {"c": torch.from_numpy(c_np), "s": torch.from_numpy(np.asarray(s_np, np.float32)), "gt_det": o.pop("gt_det"),
                 "gt_count": o.pop("gt_count")}
    return o


def ctdet_targets(boxes, cls, num, c, s, flipped=None, width=None, opt=None, device=None):
    """The label block of COCO.__getitem__ (coco.py:203-266) for a batch: cls [B,M] = the class index (cat_ids already applied).
    opt: output_h, output_w, num_classes (80), max_objs (128, coco.py:38), reg_offset, cat_spec_wh.
    -> {'hm', 'reg_mask', 'ind', 'wh' | ('cat_spec_wh', 'cat_spec_mask')[, 'reg'], 'meta'} on the device."""
    _refuse(opt, ("mse_loss", "dense_wh"))
    H, W = _opt(opt, "output_h", 128), _opt(opt, "output_w", 128)
    device, boxes, num, trans, _, flipped, width, c_np, s_np = _common(boxes, num, c, s, None, flipped, width, W, H, device)
    cls = _dev(cls, torch.int32, device)
    if tuple(cls.shape) != tuple(boxes.shape[:2]):
        raise RuntimeError("targets: cls must be [B,M] beside boxes [B,M,4], got %s" % (tuple(cls.shape),))
    want = ["hm", "reg_mask", "ind", "gt_det", "gt_count"]
    want += ["cat_spec_wh", "cat_spec_mask"] if _opt(opt, "cat_spec_wh", False) else ["wh"]
    want += ["reg"] if _opt(opt, "reg_offset", True) else []
    o = ctdet_targets_raw(boxes, cls, num, trans, flipped, width, H, W, _opt(opt, "num_classes", 80), _opt(opt, "max_objs", 128), want)
    o["meta"] = {"c": torch.from_numpy(c_np), "s": torch.from_numpy(np.asarray(s_np, np.float32)), "gt_det": o.pop("gt_det"),
                 "gt_count": o.pop("gt_count")}
    return o
