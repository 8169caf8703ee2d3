"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the image half of a training item: the train branch of COCOHP._get_input
(datasets/coco_hp.py:151-212) / COCO.__getitem__ (datasets/coco.py:156-198) after the random draws, and color_aug
(utils/image.py:200-232) with every cast written out.  The warp is oracle.preprocess.warp_affine (OpenCV's fixed-point bilinear scheme,
parity with cv2 unpinned); the crop matrix is the host's targets.get_affine_transform, which tests/test_oracle_targets.py holds to the
reference's matrices.

What numpy does in color_aug (numpy 2: a Python float is a weak scalar beside a float32 array):
    gs = cv2.cvtColor(image, BGR2GRAY)          float32; restated as (B*0.114f + G*0.587f) + R*0.299f (parity with cv2 unpinned)
    gs_mean = gs.mean()                         float32 pairwise sum / n        -> mean_mode "numpy"
                                                the device sums in fp64, exact up to 2^18 pixels: the correctly rounded mean -> "f64"
    brightness_: image *= alpha                 float32 * float32(alpha)
    contrast_:   image *= alpha; gs_mean * (1 - alpha) -> float32 * float32(1 - alpha), a float32 scalar; image += it
    saturation_: image *= alpha; gs *= (1 - alpha) (float32, in place: gs is not read again); image += gs[:, :, None]
    lighting_:   image += np.dot(eigvec, eigval * alpha): a float64 vector; the in-place add runs in float64 and casts once
then (image - mean) / std in float32 and HWC -> CHW."""
import numpy as np

from oracle.preprocess import warp_affine
from h3d_amd.targets import get_affine_transform

BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
MEAN = np.array([0.40789654, 0.44719302, 0.47026115], np.float32).reshape(1, 1, 3)
STD = np.array([0.28863828, 0.27408164, 0.27809835], np.float32).reshape(1, 1, 3)


def grayscale(image):
    """image [h,w,3] float32 (BGR) -> [h,w] float32."""
    return (image[:, :, 0] * np.float32(0.114) + image[:, :, 1] * np.float32(0.587)) + image[:, :, 2] * np.float32(0.299)


def grey_mean(gs, mean_mode):
    if mean_mode == "numpy":
        return gs.mean()
    assert mean_mode == "f64", mean_mode
    assert gs.size <= 2 ** 18                    # the float64 sum below is exact (every term a multiple of 2^-35 below 2)
    return np.float32(gs.astype(np.float64).sum() / np.float64(gs.size))


def color_aug(image, order, alpha, light, mean_mode="f64"):
    """image [h,w,3] float32 in 0..1 -> (the augmented image, gs_mean).  order: the three operations in their drawn order; alpha [3]:
    the Python floats 1 + uniform(-0.4, 0.4), per step; light [3] float64."""
    assert image.dtype == np.float32 and sorted(int(o) for o in order) == [0, 1, 2]
    gs = grayscale(image)
    gs_mean = grey_mean(gs, mean_mode)
    assert gs.dtype == np.float32 and gs_mean.dtype == np.float32
    x = image.copy()
    for op, al in zip(order, alpha):
        a, oma = np.float32(float(al)), np.float32(1 - float(al))
        x = x * a
        if op == CONTRAST:
            x = x + np.float32(gs_mean * oma)
        elif op == SATURATION:
            x = x + (gs * oma)[:, :, None]
        assert x.dtype == np.float32
    x = (x.astype(np.float64) + np.asarray(light, np.float64).reshape(1, 1, 3)).astype(np.float32)
    return x, gs_mean


def train_image(img, c, s, rot, flipped, res_w, res_h, order=None, alpha=None, light=None, mean=MEAN, std=STD, color=True, mean_mode="f64"):
    """img [h,w,3] uint8; c: the centre AFTER the mirror (c[0] = w - c[0] - 1 where flipped), as the reference and draw_params hold it.
    -> (inp [3,res_h,res_w] float32, gs_mean float32 | None)."""
    if flipped:
        img = img[:, ::-1, :]
    trans = get_affine_transform(np.asarray(c, np.float32), s, rot, [res_w, res_h])
    inp = warp_affine(img, trans, (res_w, res_h))
    inp = inp.astype(np.float32) / np.float32(255.)
    gs_mean = None
    if color:
        inp, gs_mean = color_aug(inp, order, alpha, light, mean_mode)
    inp = (inp - np.asarray(mean, np.float32).reshape(1, 1, 3)) / np.asarray(std, np.float32).reshape(1, 1, 3)
    assert inp.dtype == np.float32
    return np.ascontiguousarray(inp.transpose(2, 0, 1)), gs_mean


def train_batch(images, params, res_w, res_h, mean=MEAN, std=STD, color=True, mean_mode="f64"):
    """The batch form: images a list of [h,w,3] uint8 arrays, params the dict of h3d_amd.train_input.draw_params."""
    out, means = [], []
    s = np.asarray(params["s"])
    for b, img in enumerate(images):
        sb = s[b] if s.ndim == 2 else float(s[b])
        rot = 0.0 if params.get("rot") is None else float(params["rot"][b])
        flipped = False if params.get("flipped") is None else bool(params["flipped"][b])
        kw = dict(order=params["order"][b], alpha=params["alpha"][b], light=params["light"][b]) if color else {}
        inp, m = train_image(img, params["c"][b], sb, rot, flipped, res_w, res_h, mean=mean, std=std, color=color, mean_mode=mean_mode, **kw)
        out.append(inp)
        means.append(m)
    return np.stack(out), (np.array(means, np.float32) if color else None)
