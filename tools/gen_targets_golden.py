"""Regenerates tests/golden/targets_ref.npz: the reference's own label code run on the CPU on seeded scenes (tests/targets_ref.py: scene).

multi_pose: `datasets/coco_hp.py` is imported by file path and the unbound COCOHP._get_label is called with a namespace as `self`.  Its
imports need cv2 and pycocotools, which are not installed: a stub cv2 whose only function is getAffineTransform (a numpy 3-point solve)
and an empty pycocotools stand in for them -- nothing else of either is reached by _get_label.
ctdet: `datasets/coco.py` is imported by file path too and the unbound COCO.__getitem__ is called with a namespace as `self`: a stub
`self.coco` hands out the scene's annotations, cv2.imread returns a blank image of the scene's size and cv2.warpAffine a blank input
(the image half of the item is not kept).  split = 'val' gives the plain cases; the mirrored case runs the train branch with
opt.flip = 1 under a seeded np.random (its random crop decides c and s, which meta hands back) and no colour augmentation.  Each
case runs twice, with and without opt.cat_spec_wh, for the two sets of keys.

Per case the file holds the inputs, the two transforms and every returned array (gt_det padded to max_objs rows, gt_count beside it).
A case is rejected (the next seed is tried) when a value that feeds a truncation, a ceil, a comparison or the [0, res) gate lies within
1e-4 of its threshold: the last bit of a float64 dot product then cannot change an integer.  Every case keeps a live object, except
the empty one.  Usage: python tools/gen_targets_golden.py [reference src/lib directory]"""
import importlib.util
import os
import sys
import types
from types import SimpleNamespace as NS

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src/lib"
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

import targets_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "targets_ref.npz")
MARGIN = 1e-4
IMREAD_SHAPE = [480, 640]                     # [height, width] of the blank image the stub cv2.imread returns


def _stubs():
    cv2 = types.ModuleType("cv2")

    def getAffineTransform(src, dst):
        A = np.concatenate([np.asarray(src, np.float64), np.ones((3, 1))], axis=1)
        return np.linalg.solve(A, np.asarray(dst, np.float64)).T
    cv2.getAffineTransform = getAffineTransform
    cv2.INTER_LINEAR = 1
    cv2.imread = lambda path: np.zeros(IMREAD_SHAPE + [3], np.uint8)
    cv2.warpAffine = lambda img, t, size, flags=0: np.zeros((size[1], size[0], 3), np.uint8)
    pc, pcc, pce = types.ModuleType("pycocotools"), types.ModuleType("pycocotools.coco"), types.ModuleType("pycocotools.cocoeval")
    pcc.COCO = pce.COCOeval = object
    pc.coco, pc.cocoeval = pcc, pce
    sys.modules.update({"cv2": cv2, "pycocotools": pc, "pycocotools.coco": pcc, "pycocotools.cocoeval": pce})


_stubs()
_spec = importlib.util.spec_from_file_location("ref_coco_hp", os.path.join(REF, "datasets", "coco_hp.py"))
ref_hp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_hp)                 # (reference)
ref_image = sys.modules["image"]                 # (reference) utils/image.py, as coco_hp.py imported it
# coco_hp.py put the utils directory itself on sys.path, where utils/utils.py hides the `utils` package coco.py imports from: name it
_spec = importlib.util.spec_from_file_location("utils", os.path.join(REF, "utils", "__init__.py"), submodule_search_locations=[os.path.join(REF, "utils")])
sys.modules["utils"] = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sys.modules["utils"])
_spec = importlib.util.spec_from_file_location("ref_coco", os.path.join(REF, "datasets", "coco.py"))
ref_coco = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_coco)               # (reference)

# name -> scene and crop.  Maps at 128 x 128 in three cases, the rest at 8..40.
POSE_CASES = {
    "mp_plain": dict(seed=1, n=5, res=128, c=(320, 240), s=640.0, rot=0.0, flipped=False, no_kp=(3,)),
    "mp_flip": dict(seed=2, n=4, res=128, c=(300, 250), s=600.0, rot=0.0, flipped=True),
    "mp_rot": dict(seed=3, n=4, res=128, c=(320, 240), s=640.0, rot=17.0, flipped=False),
    "mp_res20": dict(seed=4, n=6, res=20, c=(320, 240), s=700.0, rot=0.0, flipped=True, no_kp=(1,)),
    "mp_res33_clamp": dict(seed=5, n=40, res=33, c=(320, 240), s=640.0, rot=0.0, flipped=False),
    "mp_res40_rot_flip": dict(seed=6, n=3, res=40, c=(330, 230), s=520.0, rot=-31.0, flipped=True),
    "mp_empty": dict(seed=7, n=0, res=8, c=(320, 240), s=640.0, rot=0.0, flipped=False),
}
# input_h / input_w = 4 x the map; keep_res: the input is the image size rounded up to pad + 1 and s = [input_w, input_h]
CTDET_CASES = {
    "ct_12x20": dict(seed=11, n=7, img=(640, 480), input=(48, 80), classes=80, split="val"),
    "ct_32x40_flip": dict(seed=12, n=9, img=(640, 480), input=(128, 160), classes=80, split="train"),
    "ct_8x8_c3": dict(seed=13, n=5, img=(640, 480), input=(32, 32), classes=3, split="val"),
    "ct_16x24_keep_res": dict(seed=14, n=6, img=(80, 48), input=(64, 96), classes=80, split="val", keep_res=15),
}
IMG_W, IMG_H, J, MAX_OBJS = 640, 480, 17, 32
NAMES = "gt_det hm reg reg_mask ind wh hps hps_mask hm_hp hp_offset hp_ind hp_mask".split()


def pose_case(cfg, seed):
    boxes, kps = R.scene(seed, cfg["n"], J=J, img_w=IMG_W, img_h=IMG_H)
    for k in cfg.get("no_kp", ()):
        kps[k, :, 2] = 0
    anns = [{"bbox": [float(v) for v in boxes[k]], "category_id": 1, "keypoints": [float(v) for v in kps[k].reshape(-1)]} for k in range(cfg["n"])]
    res = cfg["res"]
    me = NS(opt=NS(output_res=res, mse_loss=False, dense_hp=False, hm_gauss=2), num_joints=J, max_objs=MAX_OBJS, num_classes=1,
            flip_idx=R.FLIP_IDX)
    c = np.array(cfg["c"], np.float32)
    ret = ref_hp.COCOHP._get_label(me, c, cfg["s"], cfg["rot"], IMG_W, cfg["flipped"], anns)          # (reference)
    out = dict(zip(NAMES, ret[:len(NAMES)]))
    gt = np.zeros((MAX_OBJS, 6 + 2 * J), np.float32)
    count = len(out["gt_det"])
    if count:
        gt[:count] = np.array(out["gt_det"], np.float32)
    out["gt_det"], out["gt_count"] = gt, np.int32(count)
    trans = np.stack([ref_image.get_affine_transform(c, cfg["s"], 0, [res, res]).reshape(6),
                      ref_image.get_affine_transform(c, cfg["s"], cfg["rot"], [res, res]).reshape(6)])
    detail = {}
    R.multi_pose_image(boxes, kps, cfg["n"], trans, cfg["rot"] != 0, cfg["flipped"], IMG_W, out_h=res, out_w=res, max_objs=MAX_OBJS, detail=detail)
    inputs = {"boxes": boxes, "keypoints": kps, "num": np.int32(cfg["n"]), "c": c, "s": np.float32(cfg["s"]), "rot": np.float64(cfg["rot"]),
              "flipped": np.int32(cfg["flipped"]), "width": np.int32(IMG_W), "res": np.int32(res), "trans": trans, "seed": np.int32(seed)}
    return inputs, out, R.margins(detail, res, res), count


class _Annotations:
    """What COCO.__getitem__ asks of pycocotools' COCO object, for one image."""

    def __init__(self, anns):
        self.anns = anns

    def loadImgs(self, ids):
        return [{"file_name": "blank.jpg"}]

    def getAnnIds(self, imgIds, iscrowd=0):
        return list(range(len(self.anns)))

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]


def ctdet_case(cfg, seed):
    img_w, img_h = cfg["img"]
    input_h, input_w = cfg["input"]
    C, out_h, out_w = cfg["classes"], input_h // 4, input_w // 4
    boxes, _ = R.scene(seed, cfg["n"], J=1, img_w=img_w, img_h=img_h, min_size=img_w / 80.0, max_size=img_w / 3.0)
    cls = np.random.RandomState(seed + 500).randint(0, C, cfg["n"]).astype(np.int32)
    if cfg["n"] > 2:
        cls[1] = cls[0]                                         # two objects of one class
    anns = [{"bbox": [float(v) for v in boxes[k]], "category_id": int(cls[k]) + 1} for k in range(cfg["n"])]
    IMREAD_SHAPE[:] = [img_h, img_w]
    item = {}
    for cat_spec_wh in (False, True):
        opt = NS(keep_res="keep_res" in cfg, pad=cfg.get("keep_res", 0), input_h=input_h, input_w=input_w, down_ratio=4, not_rand_crop=False,
                 flip=1.0, no_color_aug=True, mse_loss=False, dense_wh=False, cat_spec_wh=cat_spec_wh, reg_offset=True, debug=1, hm_gauss=2)
        me = NS(images=[0], coco=_Annotations(anns), img_dir="", max_objs=MAX_OBJS, opt=opt, split=cfg["split"], num_classes=C,
                cat_ids={c + 1: c for c in range(C)}, mean=np.zeros((1, 1, 3), np.float32), std=np.ones((1, 1, 3), np.float32),
                _data_rng=np.random.RandomState(123), _eig_val=None, _eig_vec=None)
        np.random.seed(seed)                                    # the train branch draws its crop from np.random
        ret = ref_coco.COCO.__getitem__(me, 0)                  # (reference)
        assert ("cat_spec_wh" in ret) == cat_spec_wh and ("wh" in ret) != cat_spec_wh
        item.update(ret)
    meta = item["meta"]
    flipped = cfg["split"] == "train"
    c, s = np.asarray(meta["c"], np.float32), meta["s"]
    count = 0 if not np.any(item["reg_mask"]) else len(meta["gt_det"])
    gt_det = np.zeros((MAX_OBJS, 6), np.float32)
    gt_det[:count] = meta["gt_det"][:count]
    out = {k: item[k] for k in ("hm", "wh", "reg", "ind", "reg_mask", "cat_spec_wh", "cat_spec_mask")}
    out.update(gt_det=gt_det, gt_count=np.int32(count))
    t = ref_image.get_affine_transform(c, s, 0, [out_w, out_h])                                      # (reference)
    trans = np.stack([t.reshape(6), t.reshape(6)])
    detail = {}
    R.ctdet_image(boxes, cls, cfg["n"], trans, flipped, img_w, out_h=out_h, out_w=out_w, num_classes=C, max_objs=MAX_OBJS, detail=detail)
    inputs = {"boxes": boxes, "cls": cls, "num": np.int32(cfg["n"]), "c": c, "s": np.asarray(s, np.float64), "flipped": np.int32(flipped),
              "width": np.int32(img_w), "out_h": np.int32(out_h), "out_w": np.int32(out_w), "classes": np.int32(C), "trans": trans,
              "seed": np.int32(seed)}
    return inputs, out, R.margins(detail, out_w, out_h), count


def main():
    arrays = {}
    for cases, fn in ((POSE_CASES, pose_case), (CTDET_CASES, ctdet_case)):
        for name, cfg in cases.items():
            for attempt in range(200):
                seed = cfg["seed"] + 100 * attempt
                inputs, out, margin, count = fn(cfg, seed)
                if margin >= MARGIN and (count > 0 or cfg["n"] == 0):
                    break
                print("%s: seed %d rejected (margin %.3g, %d live)" % (name, seed, margin, count))
            assert margin >= MARGIN, (name, margin)
            assert count > 0 or cfg["n"] == 0, name
            print("%s: seed %d, margin %.3g, %d live objects" % (name, seed, margin, count))
            for k, v in inputs.items():
                arrays["%s.in.%s" % (name, k)] = np.asarray(v)
            for k, v in out.items():
                arrays["%s.out.%s" % (name, k)] = np.asarray(v)
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(arrays), size))
    assert size < 330000, size


if __name__ == "__main__":
    main()
