"""Training input on the device: the image half of the reference's dataset items -- the train branch of COCOHP._get_input
(datasets/coco_hp.py:151-212), the same block of COCO.__getitem__ (datasets/coco.py:156-198) and color_aug (utils/image.py:200-232) --
for a batch of uint8 frames, computed by libh3d_hip.so (csrc/augment.hip, include/h3d.h section 3b) in two launches (one without
colour augmentation).

    draw_params(sizes, opt, task, ...)                    the reference's random draws, in the reference's order -> c, s, rot, flipped, order, alpha, light
    train_input(images, params, res, ...)                 -> [B,3,res_h,res_w] fp32: warp (crop, rotation, mirror), colour augmentation, standardise
    multi_pose_train_batch(images, boxes, keypoints, ...) -> the dict COCOHP.__getitem__ returns, batched, 'input' included
    ctdet_train_batch(images, boxes, cls, ...)            -> the dict COCO.__getitem__ returns, batched, 'input' included

The dicts feed h3d_amd.losses.loss_multi_pose / loss_obj_detection unchanged.  The host draws the parameters and builds the 2x3 matrices
in float64 (targets.get_affine_transform, inverted as cv::warpAffine inverts them); everything per pixel runs on the device.  Out of
scope: decoding the frames (cv2.imread)."""
import ctypes
import random

import numpy as np
import torch

from . import _lib, targets
from .preprocess import MEAN, STD, _invert

CTDET_MEAN = (0.40789654, 0.44719302, 0.47026115)      # datasets/coco.py:26-29 (BGR)
CTDET_STD = (0.28863828, 0.27408164, 0.27809835)
EIG_VAL = np.array([0.2141788, 0.01817699, 0.00341571], np.float32)                      # coco_hp.py:63-69 / coco.py:72-78
EIG_VEC = np.array([[-0.58752847, -0.69563484, 0.41340352], [-0.5832747, 0.00994535, -0.81221408], [-0.56089297, 0.71832671, 0.41158938]],
                   np.float32)
BRIGHTNESS, CONTRAST, SATURATION = _lib.TRAIN_BRIGHTNESS, _lib.TRAIN_CONTRAST, _lib.TRAIN_SATURATION
_DATA_RNG = np.random.RandomState(123)                 # the datasets' self._data_rng: one stream for the life of the process

_DESC = np.dtype(_lib.H3dTrainImage)


def _get_border(border, size):
    i = 1
    while size - border // i <= border // i:
        i *= 2
    return border // i


def _opt(opt, name, default):
    return getattr(opt, name, default)


def draw_params(sizes, opt, task="multi_pose", np_random=np.random, data_rng=None, py_random=random):
    """The draws of one training item per image, in the reference's order and from the reference's three streams -- np_random (the crop:
    choice, 2 x randint | 3 x randn; random [+ randn] for the rotation, multi_pose only; random for the mirror), py_random (the shuffle of
    [brightness, contrast, saturation]) and data_rng (3 x uniform(-0.4, 0.4) in the shuffled order, normal(scale=0.1, size=3)); the
    same seeds give the reference's values.  sizes: (h, w) per image.  opt: not_rand_crop, shift, scale, aug_rot, rotate, flip,
    no_color_aug (no colour draws), and for ctdet keep_res / pad.
    -> {'c' [B,2] float32 (mirrored already where flipped), 's' [B] float64 ([B,2] with keep_res), 'rot' [B] float64, 'flipped' [B] bool,
        'order' [B,3] int32, 'alpha' [B,3] float64 (per step of order), 'light' [B,3] float64 = np.dot(eig_vec, eig_val * alpha)}."""
    if task not in ("multi_pose", "ctdet"):
        raise ValueError("draw_params: task %r (multi_pose or ctdet)" % (task,))
    data_rng = _DATA_RNG if data_rng is None else data_rng
    keep_res = task == "ctdet" and _opt(opt, "keep_res", False)
    B = len(sizes)
    out = {"c": np.zeros((B, 2), np.float32), "s": np.zeros((B, 2) if keep_res else (B,), np.float64), "rot": np.zeros(B, np.float64),
           "flipped": np.zeros(B, bool), "order": np.tile(np.arange(3, dtype=np.int32), (B, 1)), "alpha": np.ones((B, 3), np.float64),
           "light": np.zeros((B, 3), np.float64)}
    for b, (h, w) in enumerate(sizes):
        h, w = int(h), int(w)
        c = np.array([w / 2., h / 2.], dtype=np.float32)
        if keep_res:
            pad = _opt(opt, "pad", 31)
            s = np.array([(w | pad) + 1, (h | pad) + 1], dtype=np.float32)
        else:
            s = max(h, w) * 1.0
        rot = 0
        if not _opt(opt, "not_rand_crop", False):
            s = s * np_random.choice(np.arange(0.6, 1.4, 0.1))
            w_border, h_border = _get_border(128, w), _get_border(128, h)
            c[0] = np_random.randint(low=w_border, high=w - w_border)
            c[1] = np_random.randint(low=h_border, high=h - h_border)
        else:
            if keep_res:
                raise ValueError("draw_params: not_rand_crop with keep_res (the reference adds a 2-vector to c[0] there)")
            sf, cf = _opt(opt, "scale", 0.4), _opt(opt, "shift", 0.1)
            c[0] = c[0] + s * np.clip(np_random.randn() * cf, -2 * cf, 2 * cf)
            c[1] = c[1] + s * np.clip(np_random.randn() * cf, -2 * cf, 2 * cf)
            s = s * np.clip(np_random.randn() * sf + 1, 1 - sf, 1 + sf)
        if task == "multi_pose" and np_random.random() < _opt(opt, "aug_rot", 0):
            rf = _opt(opt, "rotate", 0)
            rot = np.clip(np_random.randn() * rf, -rf * 2, rf * 2)
        if np_random.random() < _opt(opt, "flip", 0.5):
            out["flipped"][b] = True
            c[0] = w - c[0] - 1
        out["c"][b], out["s"][b], out["rot"][b] = c, s, rot
        if not _opt(opt, "no_color_aug", False):
            ops = [BRIGHTNESS, CONTRAST, SATURATION]
            py_random.shuffle(ops)
            out["order"][b] = ops
            for k in range(3):
                out["alpha"][b, k] = 1. + data_rng.uniform(low=-0.4, high=0.4)
            out["light"][b] = np.dot(EIG_VEC, EIG_VAL * data_rng.normal(scale=0.1, size=(3,)))
    return out


def input_matrices(c, s, rot, res_w, res_h):
    """[B,6] float64: per image the inverse (dst -> src) of get_affine_transform(c, s, rot, [res_w, res_h]).  s: [B] or [B,2]."""
    c = np.asarray(c, np.float32).reshape(-1, 2)
    B = c.shape[0]
    s = np.asarray(s)
    rot = np.zeros(B) if rot is None else np.asarray(rot, np.float64).reshape(B)
    out = np.empty((B, 6), np.float64)
    for b in range(B):
        sb = s[b] if s.ndim == 2 else float(s.reshape(B)[b])
        out[b] = _invert(targets.get_affine_transform(c[b], sb, float(rot[b]), [res_w, res_h]))
    return out


def _source(images):
    """-> (one uint8 device buffer, [(offset, h, w, row_bytes)]).  A [B,h,w,3] tensor is used in place; a list of [h,w,3] tensors (rows
    may be padded: strides (row_bytes, 3, 1)) is copied once into one buffer."""
    if isinstance(images, torch.Tensor):
        _lib.require_cuda(images)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
            raise ValueError("train_input expects a uint8 [B,h,w,3] tensor or a list of [h,w,3] tensors, got %s %s" % (images.dtype, tuple(images.shape)))
        images = images.contiguous()
        B, h, w, _ = images.shape
        return images.reshape(-1), [(b * h * w * 3, h, w, 3 * w) for b in range(B)]
    images = list(images)
    _lib.require_cuda(*images)
    flat, where, at = [], [], 0
    for t in images:
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("train_input expects uint8 [h,w,3] tensors, got %s %s" % (t.dtype, tuple(t.shape)))
        h, w, _ = t.shape
        if not (t.stride(2) == 1 and t.stride(1) == 3 and t.stride(0) >= 3 * w):
            t = t.contiguous()
        rb = t.stride(0) if h > 1 else 3 * w
        n = (h - 1) * rb + 3 * w                           # the last row's padding need not exist
        flat.append(torch.as_strided(t, (n,), (1,)))
        where.append((at, h, w, rb))
        at += n
    if not flat:
        raise ValueError("train_input: no images")
    return torch.cat(flat), where


_CONST = {}      # (mean, std, device) -> (mean [3], std [3]) on the device: uploaded once, not per batch


def _mean_std(mean, std, dev):
    key = (tuple(mean), tuple(std), str(dev))
    if key not in _CONST:
        if len(_CONST) >= 32:
            _CONST.pop(next(iter(_CONST)))
        _CONST[key] = (torch.tensor(mean, dtype=torch.float32, device=dev), torch.tensor(std, dtype=torch.float32, device=dev))
        torch.cuda.current_stream(dev).synchronize()
    return _CONST[key]


def descriptors(where, params, res_w, res_h, color_aug=True):
    """The h3d_train_image array of a batch (numpy, one record per image) from the frames' places and the drawn parameters."""
    B = len(where)
    d = np.zeros(B, _DESC)
    d["minv"] = input_matrices(params["c"], params["s"], params.get("rot"), res_w, res_h)
    flipped = params.get("flipped")
    d["flipped"] = 0 if flipped is None else np.asarray(flipped).reshape(B).astype(np.int32)
    for b, (at, h, w, rb) in enumerate(where):
        d["offset"][b], d["h"][b], d["w"][b], d["row_bytes"][b] = at, h, w, rb
    d["order"] = np.arange(3, dtype=np.int32)
    d["alpha"] = d["one_minus_alpha"] = 0
    if color_aug:
        alpha = np.asarray(params["alpha"], np.float64).reshape(B, 3)
        d["order"] = np.asarray(params["order"], np.int32).reshape(B, 3)
        d["alpha"] = alpha.astype(np.float32)              # `image *= alpha` with a Python float: the float32 loop
        d["one_minus_alpha"] = (1 - alpha).astype(np.float32)          # `image2 *= (1 - alpha)`: the difference in double, then float32
        d["light"] = np.asarray(params["light"], np.float64).reshape(B, 3)
    return d


@torch.no_grad()
def train_input(images, params, res, mean=MEAN, std=STD, color_aug=True, out=None, return_gs_mean=False):
    """images: [B,h,w,3] uint8 (BGR, as cv2.imread yields) on the device, or a list of [h_i,w_i,3] device tensors.  params: the dict of
    draw_params (c, s[, rot][, flipped] and with color_aug order, alpha, light).  res: the input resolution, an int or (res_h, res_w).
    -> inp [B,3,res_h,res_w] fp32 on the device (written into `out` when given); with return_gs_mean also the [B] float32 grey means
    contrast_ blends with."""
    res_h, res_w = (res, res) if isinstance(res, int) else (int(res[0]), int(res[1]))
    buf, where = _source(images)
    dev, B = buf.device, len(where)
    if out is None:
        out = torch.empty(B, 3, res_h, res_w, dtype=torch.float32, device=dev)
    else:
        _lib.require_cuda(out)
        if tuple(out.shape) != (B, 3, res_h, res_w) or out.dtype != torch.float32 or not out.is_contiguous():
            raise RuntimeError("train_input: out must be contiguous float32 %s, got %s of %s" % ((B, 3, res_h, res_w), tuple(out.shape), out.dtype))
    desc = descriptors(where, params, res_w, res_h, color_aug)
    mean_t, std_t = _mean_std(mean, std, dev)
    options = 0 if color_aug else _lib.TRAIN_INPUT_NO_COLOR_AUG
    with torch.cuda.device(dev):
        desc_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(dev)
        ws = _lib.workspace(_lib.lib().h3d_train_input_workspace_bytes, B, res_h, res_w, options, device=dev)
        gs_mean = torch.empty(B, dtype=torch.float32, device=dev) if (return_gs_mean and color_aug) else None
        rc = _lib.lib().h3d_train_input(_lib.ptr(buf), buf.numel(), ctypes.c_void_p(desc.ctypes.data), _lib.ptr(desc_dev), B, _lib.ptr(mean_t),
                                        _lib.ptr(std_t), res_h, res_w, options, _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.ptr(out),
                                        _lib.ptr(gs_mean), _lib.stream_ptr())
    _lib.check(rc, "h3d_train_input")
    return (out, gs_mean) if return_gs_mean else out


def _sizes(images):
    if isinstance(images, torch.Tensor):
        return [(int(images.shape[1]), int(images.shape[2]))] * int(images.shape[0])
    return [(int(t.shape[0]), int(t.shape[1])) for t in images]


def _input_res(opt):
    res = _opt(opt, "input_res", None)
    return (res, res) if res else (_opt(opt, "input_h", 512), _opt(opt, "input_w", 512))


def multi_pose_train_batch(images, boxes, keypoints, num, opt, np_random=np.random, data_rng=None, py_random=random, params=None, smpl_labels=None):
    """COCOHP.__getitem__ with split == 'train' for a batch: images as train_input takes them, boxes / keypoints / num as
    targets.multi_pose_targets takes them.  The parameters are drawn here (draw_params; or handed in through `params`), and the input and
    the labels are built from the same c, s, rot, flipped and image widths.  opt: input_res (or input_h / input_w), no_color_aug and
    what draw_params and multi_pose_targets read.  -> multi_pose_targets' dict + 'input' [B,3,res_h,res_w].
    smpl_labels: a dict of pose [B,M,72], shape [B,M,10], valid [B,M] and optionally joints, joint_weight, pose_weight, smpl_model (what
    smpl_sup.smpl_targets takes); the result then also carries the six SMPL label tensors, moved with the same rot and flipped."""
    sizes = _sizes(images)
    if params is None:
        params = draw_params(sizes, opt, "multi_pose", np_random, data_rng, py_random)
    dev = images.device if isinstance(images, torch.Tensor) else images[0].device
    inp = train_input(images, params, _input_res(opt), MEAN, STD, color_aug=not _opt(opt, "no_color_aug", False))
    ret = targets.multi_pose_targets(boxes, keypoints, num, params["c"], params["s"], rot=params["rot"], flipped=params["flipped"],
                                     width=[w for _, w in sizes], opt=opt, device=dev)
    ret["input"] = inp
    if smpl_labels is not None:
        from . import smpl_sup
        lab = smpl_labels
        ret.update(smpl_sup.smpl_targets(lab["pose"], lab["shape"], lab["valid"], num, ret["reg_mask"], rot=params["rot"], flipped=params["flipped"],
                                         c=params["c"], s=params["s"], joints=lab.get("joints"), joint_weight=lab.get("joint_weight"),
                                         pose_weight=lab.get("pose_weight"), smpl_model=lab.get("smpl_model"), opt=opt))
    return ret


def ctdet_train_batch(images, boxes, cls, num, opt, np_random=np.random, data_rng=None, py_random=random, params=None):
    """COCO.__getitem__ with split == 'train' for a batch (no rotation): as multi_pose_train_batch, with targets.ctdet_targets.  With
    opt.keep_res the frames of a batch must share one (h | pad) + 1, (w | pad) + 1, which is then the input size."""
    sizes = _sizes(images)
    if params is None:
        params = draw_params(sizes, opt, "ctdet", np_random, data_rng, py_random)
    dev = images.device if isinstance(images, torch.Tensor) else images[0].device
    res = _input_res(opt)
    if _opt(opt, "keep_res", False):
        pad = _opt(opt, "pad", 31)
        all_res = {((h | pad) + 1, (w | pad) + 1) for h, w in sizes}
        if len(all_res) != 1:
            raise ValueError("ctdet_train_batch: keep_res needs one input size per batch, got %s" % sorted(all_res))
        res = all_res.pop()
    inp = train_input(images, params, res, CTDET_MEAN, CTDET_STD, color_aug=not _opt(opt, "no_color_aug", False))
    ret = targets.ctdet_targets(boxes, cls, num, params["c"], params["s"], flipped=params["flipped"], width=[w for _, w in sizes], opt=opt,
                                device=dev)
    ret["input"] = inp
    return ret
