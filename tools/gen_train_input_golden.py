"""Regenerates tests/golden/train_input_ref.npz: the reference's own training-input code run on the CPU on seeded noise frames.

multi_pose: `datasets/coco_hp.py` is imported by file path and the unbound COCOHP._get_input is called with a namespace as `self` and
split = 'train'.  ctdet: `datasets/coco.py` is imported by file path too and the unbound COCO.__getitem__ is called the same way (no
annotations: the label half of the item is tests/golden/targets_ref.npz's business).  Their imports need cv2 and pycocotools, which are
not installed; the stand-ins:
    cv2.getAffineTransform   the 3-point solve of h3d_amd.targets (Cramer's rule in float64)
    cv2.warpAffine           oracle.preprocess.warp_affine (OpenCV's fixed-point bilinear scheme; parity with cv2 unpinned)
    cv2.cvtColor             (B*0.114f + G*0.587f) + R*0.299f in float32 (BGR2GRAY on float input; parity with cv2 unpinned)
    cv2.imread               a seeded noise frame of the case's size
    pycocotools              empty
np.random, random and the dataset's _data_rng = RandomState(123) are seeded per case.  Per case the file holds the frame, the seed, the
options draw_params reads, and what the reference returned: c, s, rot, flipped and inp.  COCO.__getitem__ does not return `flipped`: the
item is built a second time with the same seeds and opt.flip = 0, and flipped = (c differs) -- c[0] is an integer or a random float and
w is even, so a mirrored c[0] = w - c[0] - 1 never equals the plain one.
Usage: python tools/gen_train_input_golden.py <reference src/lib directory>"""
import importlib.util
import os
import random
import sys
import types
from types import SimpleNamespace as NS

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) < 2:
    sys.exit("usage: python tools/gen_train_input_golden.py <reference src/lib directory>")
REF = sys.argv[1]
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

import h3d_amd  # noqa: E402,F401
from h3d_amd import targets, train_input  # noqa: E402
from oracle.preprocess import warp_affine  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "train_input_ref.npz")
FRAME = {}                                    # what the stub cv2.imread returns: set per case


def _stubs():
    cv2 = types.ModuleType("cv2")
    cv2.getAffineTransform = lambda src, dst: targets._solve3(src, dst)
    cv2.INTER_LINEAR, cv2.COLOR_BGR2GRAY = 1, 6
    cv2.imread = lambda path: FRAME["img"].copy()
    cv2.warpAffine = lambda img, t, size, flags=0: warp_affine(img, t, size)

    def cvtColor(image, code):
        assert code == cv2.COLOR_BGR2GRAY and image.dtype == np.float32
        return (image[:, :, 0] * np.float32(0.114) + image[:, :, 1] * np.float32(0.587)) + image[:, :, 2] * np.float32(0.299)
    cv2.cvtColor = cvtColor
    pc, pcc, pce = types.ModuleType("pycocotools"), types.ModuleType("pycocotools.coco"), types.ModuleType("pycocotools.cocoeval")
    pcc.COCO = pce.COCOeval = object
    pc.coco, pc.cocoeval = pcc, pce
    sys.modules.update({"cv2": cv2, "pycocotools": pc, "pycocotools.coco": pcc, "pycocotools.cocoeval": pce})


_stubs()
_spec = importlib.util.spec_from_file_location("ref_coco_hp", os.path.join(REF, "datasets", "coco_hp.py"))
ref_hp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_hp)                 # (reference)
# coco_hp.py put the utils directory itself on sys.path, where utils/utils.py hides the `utils` package coco.py imports from: name it
_spec = importlib.util.spec_from_file_location("utils", os.path.join(REF, "utils", "__init__.py"), submodule_search_locations=[os.path.join(REF, "utils")])
sys.modules["utils"] = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sys.modules["utils"])
_spec = importlib.util.spec_from_file_location("ref_coco", os.path.join(REF, "datasets", "coco.py"))
ref_coco = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_coco)               # (reference)

# name -> frame (h, w), input (h, w) and the options the draws depend on.  Frames <= 48 x 64, inputs <= 64 x 64.
BASE = dict(not_rand_crop=False, shift=0.1, scale=0.4, aug_rot=0.0, rotate=0.0, flip=0.0, no_color_aug=False)
CASES = {
    "mp_rand_crop": dict(BASE, task="multi_pose", seed=21, frame=(48, 64), input=(64, 64)),
    "mp_not_rand_crop": dict(BASE, task="multi_pose", seed=22, frame=(40, 56), input=(48, 48), not_rand_crop=True),
    "mp_rot": dict(BASE, task="multi_pose", seed=23, frame=(48, 64), input=(40, 40), aug_rot=1.0, rotate=30.0),
    "mp_flip": dict(BASE, task="multi_pose", seed=24, frame=(37, 62), input=(33, 33), flip=1.0),
    "mp_no_color_aug": dict(BASE, task="multi_pose", seed=25, frame=(48, 64), input=(64, 64), flip=0.5, no_color_aug=True),
    "ct_40x56": dict(BASE, task="ctdet", seed=26, frame=(48, 64), input=(40, 56), flip=0.5),
    "ct_flip_not_rand_crop": dict(BASE, task="ctdet", seed=27, frame=(44, 60), input=(32, 48), flip=1.0, not_rand_crop=True),
}
OPT_KEYS = ("not_rand_crop", "shift", "scale", "aug_rot", "rotate", "flip", "no_color_aug")


class _NoAnnotations:
    def loadImgs(self, ids):
        return [{"file_name": "noise.jpg"}]

    def getAnnIds(self, imgIds, iscrowd=0):
        return []

    def loadAnns(self, ids):
        return []


def _seed(seed):
    np.random.seed(seed)
    random.seed(seed)
    return np.random.RandomState(123)


def run_case(cfg, flip=None):
    """-> (inp, c, s, rot) of the reference for the case's seeds (flip: an override of opt.flip)."""
    seed, (in_h, in_w) = cfg["seed"], cfg["input"]
    o = {k: cfg[k] for k in OPT_KEYS}
    if flip is not None:
        o["flip"] = flip
    mean = np.array(train_input.MEAN, np.float32).reshape(1, 1, 3)
    std = np.array(train_input.STD, np.float32).reshape(1, 1, 3)
    if cfg["task"] == "multi_pose":
        assert in_h == in_w
        me = NS(opt=NS(input_res=in_h, **o), split="train", _data_rng=_seed(seed), _eig_val=train_input.EIG_VAL, _eig_vec=train_input.EIG_VEC,
                mean=mean, std=std)
        inp, c, s, rot, flipped = ref_hp.COCOHP._get_input(me, FRAME["img"].copy())          # (reference)
        return inp, c, s, rot, flipped
    opt = NS(keep_res=False, pad=31, input_h=in_h, input_w=in_w, down_ratio=4, mse_loss=False, dense_wh=False, cat_spec_wh=False, reg_offset=True,
             debug=1, hm_gauss=2, **o)
    me = NS(images=[0], coco=_NoAnnotations(), img_dir="", max_objs=8, opt=opt, split="train", num_classes=2, cat_ids={1: 0, 2: 1},
            mean=np.array(train_input.CTDET_MEAN, np.float32).reshape(1, 1, 3), std=np.array(train_input.CTDET_STD, np.float32).reshape(1, 1, 3),
            _data_rng=_seed(seed), _eig_val=train_input.EIG_VAL, _eig_vec=train_input.EIG_VEC)
    ret = ref_coco.COCO.__getitem__(me, 0)                                                   # (reference)
    return ret["input"], ret["meta"]["c"], ret["meta"]["s"], 0, None


def main():
    arrays = {}
    for name, cfg in CASES.items():
        h, w = cfg["frame"]
        assert w % 2 == 0
        FRAME["img"] = np.random.RandomState(cfg["seed"] + 1000).randint(0, 256, (h, w, 3)).astype(np.uint8)
        inp, c, s, rot, flipped = run_case(cfg)
        if flipped is None:
            flipped = not np.array_equal(run_case(cfg, flip=0.0)[1], c)
        assert inp.dtype == np.float32 and inp.shape == (3,) + tuple(cfg["input"])
        rec = {"img": FRAME["img"], "seed": np.int32(cfg["seed"]), "task": np.array(cfg["task"]), "input": np.array(cfg["input"], np.int32),
               "c": np.asarray(c, np.float32), "s": np.asarray(s, np.float64), "rot": np.float64(rot), "flipped": np.bool_(flipped), "inp": inp}
        rec.update({"opt_" + k: np.asarray(cfg[k]) for k in OPT_KEYS})
        for k, v in rec.items():
            arrays["%s.%s" % (name, k)] = v
        print("%s: c = %s, s = %s, rot = %.4f, flipped = %s, inp in [%.3f, %.3f]" % (name, c, s, rot, bool(flipped), inp.min(), inp.max()))
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(arrays), size))
    assert size < 400000, size


if __name__ == "__main__":
    main()
